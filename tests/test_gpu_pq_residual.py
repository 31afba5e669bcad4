"""Residual PQ shadows (nvdb_hip_pq_build_residual / _train_residual / _reconstruct / _kind and the searches over such a shadow)
against plain numpy fp64 of the header's definitions.  Fixture: test_gpu_pq.py's -- 5000 rows, partitions [0, 0, 37, 101, 2300,
4990, 5000]: an empty list, one shorter than a wave, boundaries off the 64-row grid, a 256-row encode tile that spans three
lists, one list of two segments, a 10-row tail.  Centroids: the f32 mean of each list (the empty one: ones).

Score bound (test_scores): the GPU's s = fl(b + S).  b is a dot product of dim elements as 64 chains of ceil(dim / 64) fmas and a
six-level tree: |b - q.c| <= (ceil(dim / 64) + 6) eps * sum_t |q_t c_t|.  S is test_gpu_pq.py's: tables of dsub fmas, M additions:
|S - S64| <= (dsub + M) eps * sum_m A[m][code].  The last addition adds eps |b + S| <= eps (sum |q c| + sum A).  Together, to
first order in eps = 2^-24, with 1 % for the higher orders:
    tol = 1.01 eps ((ceil(dim / 64) + 7) sum_t |q_t c_t| + (dsub + M + 1) sum_m A[m][code])."""
import numpy as np
import pytest

import nvdb_amd

pytestmark = pytest.mark.gpu

N, ROW_BASE, SEED = 5000, 1_000_003, 20261126
OFFSETS = np.array([0, 0, 37, 101, 2300, 4990, 5000], dtype=np.uint64)
NPARTS, BIG = len(OFFSETS) - 1, 4
LIST_OF = np.repeat(np.arange(NPARTS), np.diff(OFFSETS).astype(np.int64))
U64MAX = np.iinfo(np.uint64).max
F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8
EPS = 2.0 ** -24
#        dtype dim  M      reaches
CASES = [(F16, 32, 4),     # G = 8, dword codes, DMAX = 8
         (F16, 96, 48),    # G = 2, three 16-byte pieces
         (F16, 128, 128),  # G = 1, dsub = 1
         (F16, 128, 4),    # dsub = 32: the widest encode build
         (F32, 64, 16), (I8, 64, 16)]
_cache = {}


def rows_f32(base, scales, dtype):
    if dtype == I8:
        return base.astype(np.float32) * scales[:, None].astype(np.float32)
    return base.view(np.float16).astype(np.float32) if dtype == F16 else base


def make_codebooks(X, M, seed=5):
    rs = np.random.RandomState(seed)
    sub = X.reshape(len(X), M, X.shape[1] // M)
    cb = np.stack([sub[rs.choice(len(X), 256, replace=False), m] for m in range(M)])
    return (cb + 0.01 * rs.standard_normal(cb.shape)).astype(np.float32)


def new_ctx(c, cents):
    ctx = nvdb_amd.HipContext(0)
    ctx.upload_corpus(c["base"], c["dtype"], c["scales"], ROW_BASE)
    ctx.set_partitions(OFFSETS)
    if cents is not None:
        ctx.set_centroids(cents)
    return ctx


def case(dtype, dim, M):
    """One corpus with its residual shadow, built once; the numpy residuals E are float32 by definition."""
    key = (dtype, dim, M)
    if key not in _cache:
        base, scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
        c = dict(base=base, scales=scales, dtype=dtype, X=rows_f32(base, scales, dtype))
        cents = np.ones((NPARTS, dim), dtype=np.float32)
        for p in range(NPARTS):
            if OFFSETS[p + 1] > OFFSETS[p]:
                cents[p] = c["X"][int(OFFSETS[p]):int(OFFSETS[p + 1])].mean(0, dtype=np.float32)
        c.update(cents=cents, E=c["X"] - cents[LIST_OF])
        c["cb"] = make_codebooks(c["E"], M)
        c["ctx"] = new_ctx(c, cents)
        c["ctx"].pq_build(c["cb"], residual=True)
        c.update(codes=c["ctx"].pq_download_codes(), queries=nvdb_amd.synth_rows_f32(SEED + 1, 0, 19, dim))
        _cache[key] = c
    return _cache[key]


def probe_table(nq):
    q = np.arange(nq)
    return np.stack([np.full(nq, BIG), q % 6, (q * 5 + 1) % 6], axis=1).astype(np.uint32)


def union_rows(probe_row):
    return np.concatenate([np.arange(OFFSETS[p], OFFSETS[p + 1], dtype=np.int64) for p in sorted(set(int(p) for p in probe_row))])


@pytest.mark.parametrize("dtype,dim,M", CASES)
def test_encode_and_reconstruct(dtype, dim, M):
    c = case(dtype, dim, M)
    dsub, codes, ctx = dim // M, c["codes"], c["ctx"]
    assert ctx.pq_kind() == dict(residual=True) and ctx.pq_info() == dict(M=M, dsub=dsub, code_bytes=N * M)
    sub = c["E"].astype(np.float64).reshape(N, M, dsub)
    for m in range(M):
        d64 = ((sub[:, m, None, :] - c["cb"][m].astype(np.float64)[None]) ** 2).sum(-1)              # [N, 256]
        got = d64[np.arange(N), codes[:, m]]
        print(f"m={m} worst d(code) / min d = 1 + {(got / np.maximum(d64.min(1), 1e-300)).max() - 1:.3e}  (bound {2 * (dsub + 3) * EPS:.3e})")
        assert (got <= d64.min(1) * (1 + 2 * (dsub + 3) * EPS)).all(), m
    cw = c["cb"][np.arange(M), codes].reshape(N, dim)                                                # the codeword of every sub-vector
    want = c["cents"][LIST_OF] + cw
    assert np.array_equal(ctx.pq_reconstruct().view(np.uint32), want.view(np.uint32))
    for r in (0, 36, 37, 100, 101, 4989, 4999):
        assert np.array_equal(ctx.pq_reconstruct(r, 1).view(np.uint32), want[r:r + 1].view(np.uint32)), r
    assert np.array_equal(ctx.pq_reconstruct(36, 66).view(np.uint32), want[36:102].view(np.uint32))


@pytest.mark.parametrize("R", [10, N])
@pytest.mark.parametrize("dtype,dim,M", CASES)
def test_scores(dtype, dim, M, R):
    c = case(dtype, dim, M)
    dsub, codes, queries, probe = dim // M, c["codes"], c["queries"], probe_table(19)
    ids, scores, counts = c["ctx"].pq_search_partitions(queries, R, probe)
    assert c["ctx"].stats()["path"] == 9
    marange = np.arange(M)
    for q in range(19):
        prod = queries[q].astype(np.float64).reshape(M, 1, dsub) * c["cb"].astype(np.float64)         # [M, 256, dsub]
        L64, A64 = prod.sum(-1), np.abs(prod).sum(-1)
        qc = queries[q].astype(np.float64)[None] * c["cents"].astype(np.float64)                     # [NPARTS, dim]
        rows = union_rows(probe[q])
        s64 = qc.sum(1)[LIST_OF[rows]] + L64[marange, codes[rows]].sum(1)
        tol = 1.01 * EPS * ((-(-dim // 64) + 7) * np.abs(qc).sum(1)[LIST_OF[rows]] + (dsub + M + 1) * A64[marange, codes[rows]].sum(1)).max()
        cnt = min(R, len(rows))
        assert counts[q] == cnt and (ids[q, cnt:] == U64MAX).all() and np.isneginf(scores[q, cnt:]).all()
        local = (ids[q, :cnt] - np.uint64(ROW_BASE)).astype(np.int64)
        assert np.isin(local, rows).all() and len(set(local)) == cnt                                   # (R = N: a permutation of the union)
        pos = np.searchsorted(rows, local)
        err = np.abs(scores[q, :cnt].astype(np.float64) - s64[pos]).max()
        print(f"q={q} max |score - s64| = {err:.3e} (tol {tol:.3e})")
        assert err <= tol
        rest = np.delete(s64, pos)
        assert not rest.size or s64[pos].min() >= rest.max() - 2 * tol
        assert (np.lexsort((local, -scores[q, :cnt])) == np.arange(cnt)).all()


@pytest.mark.parametrize("dtype,dim,M", CASES)
def test_zero_centroids_equal_the_non_residual_build(dtype, dim, M):
    """0 + S is exact and x - 0 = x: under all-zero centroids the residual path must repeat the non-residual one to the bit --
    which pins the list lookup, the sink and the base terms' indexing together."""
    c = case(dtype, dim, M)
    ctx = new_ctx(c, np.zeros((NPARTS, dim), dtype=np.float32))
    got = []
    for residual in (False, True):
        ctx.pq_build(c["cb"], residual=residual)
        assert ctx.pq_kind()["residual"] == residual
        got.append((ctx.pq_download_codes(),) + tuple(x for R in (10, N) for x in ctx.pq_search_partitions(c["queries"], R, probe_table(19))))
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    cw = c["cb"][np.arange(M), got[0][0]].reshape(N, dim)
    ctx.pq_build(c["cb"])
    assert np.array_equal(ctx.pq_reconstruct(4989, 11).view(np.uint32), cw[4989:].view(np.uint32))  # non-residual: the codeword alone
    ctx.close()


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("dtype", [F16, I8])
def test_train_equals_training_on_the_residual_matrix(dtype, iters):
    c = case(dtype, 64, 16) if dtype == I8 else case(dtype, 96, 48)
    M = c["cb"].shape[0]
    plain = nvdb_amd.HipContext(0)
    plain.upload_corpus(c["E"], F32, None, 0)
    want = plain.pq_train(M, iters, SEED, 0)
    got = c["ctx"].pq_train(M, iters, SEED, 0, residual=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, c["ctx"].pq_train(M, iters, SEED, 0))                             # (and not the non-residual trainer's)
    plain.close()


def test_fused_refine_equals_its_halves():
    c = case(F16, 96, 48)
    ctx, queries, K, R, nprobe = c["ctx"], c["queries"], 10, 100, 3
    ids, _, _ = ctx.pq_search_ivf(queries, R, nprobe)
    cand = np.where(ids == U64MAX, np.uint64(0xFFFFFFFF), ids - np.uint64(ROW_BASE)).astype(np.uint32)
    rid, rdist = ctx.refine_l2_topk(queries, cand, K)
    fi, fd = ctx.pq_refine_ivf(queries, K, R, nprobe)
    assert (rid != 0xFFFFFFFF).any()
    assert np.array_equal(fi, np.where(rid == 0xFFFFFFFF, U64MAX, rid.astype(np.uint64) + np.uint64(ROW_BASE)))
    assert np.array_equal(fd.view(np.uint32), rdist.view(np.uint32))


def test_lifecycle_and_arguments():
    dim, M = 32, 4
    base, _ = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, F32)
    base = base.copy()
    base[[5, 50]] = np.nan                                               # rows of NaN (lists 1 and 2) ...
    c = dict(base=base, scales=None, dtype=F32)
    cents = np.ones((NPARTS, dim), dtype=np.float32)
    cents[1] = np.nan                                                    # ... and a NaN centroid (list 1: rows 0 .. 36)
    cb = make_codebooks(np.nan_to_num(base), M)
    q, probe = nvdb_amd.synth_rows_f32(SEED + 1, 0, 2, dim), np.array([[1, 2, 5]] * 2, dtype=np.uint32)

    def invalid(fn, word):
        with pytest.raises(nvdb_amd.NvdbError) as e:
            fn()
        assert e.value.status == 1 and word in str(e.value), str(e.value)

    ctx = nvdb_amd.HipContext(0)
    ctx.upload_corpus(base, F32, None, ROW_BASE)
    invalid(lambda: ctx.pq_build(cb, residual=True), "nvdb_hip_set_partitions")
    invalid(lambda: ctx.pq_train(M, 0, SEED, residual=True), "nvdb_hip_set_partitions")
    ctx.set_partitions(OFFSETS)
    invalid(lambda: ctx.pq_build(cb, residual=True), "nvdb_hip_set_centroids")
    ctx.pq_build(cb)                                                     # a non-residual shadow survives a failed residual build,
    invalid(lambda: ctx.pq_build(cb, residual=True), "nvdb_hip_set_centroids")
    ctx.set_centroids(cents)                                             # ... new centroids and a new table
    invalid(lambda: ctx.pq_build(np.zeros((6, 256, 5), np.float32), residual=True), "M must be")
    ctx.set_partitions(OFFSETS)
    assert ctx.pq_kind() == dict(residual=False) and ctx.pq_search_partitions(q, 10, probe)[2].tolist() == [10, 10]
    ctx.set_centroids(cents)
    ctx.pq_build(cb, residual=True)
    # no fault; NaN residuals get code 0; a NaN base term makes every row of its list no candidate (the NaN row's own score is
    # b + the tables' entries of code 0: finite, as under a non-residual shadow)
    codes = ctx.pq_download_codes()
    assert (codes[:37] == 0).all() and (codes[50] == 0).all() and codes[37:101].any()
    ids, scores, counts = ctx.pq_search_partitions(q, N, probe)
    assert counts.tolist() == [64 + 10] * 2                              # lists 2 and 5
    assert (ids[0, :counts[0]] - np.uint64(ROW_BASE) >= 37).all() and np.isfinite(scores[0, :counts[0]]).all()
    invalid(lambda: ctx.pq_build(np.zeros((6, 256, 5), np.float32)), "M must be")
    assert ctx.pq_kind() == dict(residual=True)                          # a failed build of either kind leaves the residual shadow
    for change in (lambda: ctx.set_centroids(cents), lambda: ctx.set_partitions(OFFSETS)):
        change()
        invalid(lambda: ctx.pq_search_partitions(q, 10, probe), "nvdb_hip_pq_build")
        invalid(lambda: ctx.pq_reconstruct(0, 1), "nvdb_hip_pq_build")
        assert ctx.pq_kind() == dict(residual=False) and ctx.pq_info()["M"] == 0
        ctx.set_centroids(cents)
        ctx.pq_build(cb, residual=True)
    ctx.close()
