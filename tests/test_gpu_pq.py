"""PQ candidate scan (nvdb_hip_pq_build / _search_partitions / _search_ivf / _refine_ivf and the index forms) against plain numpy
fp64 of the header's definitions: encode within the fp32 rounding bound of a sum of dsub squared differences, scores within the
bound of two nested fp32 sums, membership of the R best up to that bound, the fused pipeline equal to its two halves, lifecycle.

Fixture: 5000 rows; partitions [0, 0, 37, 101, 2300, 4990, 5000] -- one empty, one shorter than a tile, starts off the 64-row
grid, one of 2690 rows (two segments), a 10-row tail.  Codebooks: 256 sampled row sub-vectors plus small noise, codewords 3 and 7
of sub-quantiser 0 bit-identical.  (dim, M) covers every group size G and both code-load widths."""
import numpy as np
import pytest

import nvdb_amd

pytestmark = pytest.mark.gpu

N, ROW_BASE, SEED = 5000, 1_000_003, 20261126
OFFSETS = np.array([0, 0, 37, 101, 2300, 4990, 5000], dtype=np.uint64)
BIG = 4
U64MAX = np.iinfo(np.uint64).max
F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8
EPS = 2.0 ** -24
#        dtype dim  M     G   code loads
CASES = [(F16, 32, 4),    # 8, dwords
         (F16, 64, 16),   # 8, 16 bytes
         (F16, 80, 20),   # 4, dwords
         (F16, 96, 48),   # 2, three 16-byte pieces; dsub 2
         (F16, 128, 128),  # 1, 16 bytes; dsub 1
         (F32, 64, 16), (I8, 64, 16)]
_cache = {}


def rows_f32(base, scales, dtype):
    """The rows as f32 queries: f32 as it is, f16 widened exactly, int8 float(x) * scale rounded once."""
    if dtype == F16:
        return base.view(np.float16).astype(np.float32)
    if dtype == I8:
        return base.astype(np.float32) * scales[:, None].astype(np.float32)
    return base


def make_codebooks(X, M, seed=5):
    rs = np.random.RandomState(seed)
    dsub = X.shape[1] // M
    sub = X.reshape(len(X), M, dsub)
    cb = np.stack([sub[rs.choice(len(X), 256, replace=False), m] for m in range(M)])
    cb = (cb + 0.01 * rs.standard_normal(cb.shape)).astype(np.float32)
    cb[0, 7] = cb[0, 3]
    return cb


def case(dtype, dim, M):
    """One resident corpus with its codes, built once: the fp64 reference is shared by every test of the case."""
    key = (dtype, dim, M)
    if key not in _cache:
        base, scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
        X = rows_f32(base, scales, dtype)
        cb = make_codebooks(X, M)
        ctx = nvdb_amd.HipContext(0)
        ctx.upload_corpus(base, dtype, scales, ROW_BASE)
        ctx.set_partitions(OFFSETS)
        ctx.pq_build(cb)
        queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, 19, dim)
        _cache[key] = dict(ctx=ctx, X=X, cb=cb, codes=ctx.pq_download_codes(), queries=queries, base=base, scales=scales)
    return _cache[key]


def probe_table(nq):
    """Every query probes the 2690-row partition (19 queries: more than one group, the last partial); the other slots walk over
    the table, the empty partition and duplicates included."""
    if nq == 1:
        return np.array([[BIG, 1, 5]], dtype=np.uint32)
    q = np.arange(nq)
    return np.stack([np.full(nq, BIG), q % 6, (q * 5 + 1) % 6], axis=1).astype(np.uint32)


def union_rows(probe_row):
    return np.concatenate([np.arange(OFFSETS[p], OFFSETS[p + 1], dtype=np.int64) for p in sorted(set(int(p) for p in probe_row))])


@pytest.mark.parametrize("dtype,dim,M", CASES)
def test_encode(dtype, dim, M):
    c = case(dtype, dim, M)
    dsub = dim // M
    assert c["ctx"].pq_info() == dict(M=M, dsub=dsub, code_bytes=N * M)
    sub = c["X"].astype(np.float64).reshape(N, M, dsub)
    for m in range(M):
        d64 = ((sub[:, m, None, :] - c["cb"][m].astype(np.float64)[None]) ** 2).sum(-1)              # [N, 256]
        got = d64[np.arange(N), c["codes"][:, m]]
        worst = (got / np.maximum(d64.min(1), 1e-300)).max()
        print(f"m={m} worst d(code) / min d = 1 + {worst - 1:.3e}  (bound {2 * (dsub + 3) * EPS:.3e})")
        assert (got <= d64.min(1) * (1 + 2 * (dsub + 3) * EPS)).all(), (m, worst)
    assert (c["codes"][:, 0] == 3).any() and not (c["codes"][:, 0] == 7).any()                      # the duplicated pair: the lower index


@pytest.mark.parametrize("R", [1, 10, 100, 3000])
@pytest.mark.parametrize("nq", [1, 19])
@pytest.mark.parametrize("dtype,dim,M", CASES)
def test_scores_and_membership(dtype, dim, M, nq, R):
    c = case(dtype, dim, M)
    dsub, codes = dim // M, c["codes"]
    queries, probe = c["queries"][:nq], probe_table(nq)
    ids, scores, counts = c["ctx"].pq_search_partitions(queries, R, probe)
    assert c["ctx"].stats()["path"] == 9
    marange = np.arange(M)
    for q in range(nq):
        qs = queries[q].astype(np.float64).reshape(M, 1, dsub)
        prod = qs * c["cb"].astype(np.float64)                                                        # [M, 256, dsub]
        L64, A64 = prod.sum(-1), np.abs(prod).sum(-1)
        rows = union_rows(probe[q])
        s64 = L64[marange, codes[rows]].sum(1)
        tol = 1.01 * (dsub + M) * EPS * A64[marange, codes[rows]].sum(1).max()
        cnt = min(R, len(rows))
        assert counts[q] == cnt
        assert (ids[q, cnt:] == U64MAX).all() and np.isneginf(scores[q, cnt:]).all()
        local = (ids[q, :cnt] - np.uint64(ROW_BASE)).astype(np.int64)
        assert np.isin(local, rows).all() and len(set(local)) == cnt
        pos = np.searchsorted(rows, local)
        err = np.abs(scores[q, :cnt].astype(np.float64) - s64[pos]).max()
        print(f"q={q} max |score - s64| = {err:.3e} (tol {tol:.3e})")
        assert err <= tol
        rest = np.delete(s64, pos)
        if rest.size:
            assert s64[pos].min() >= rest.max() - 2 * tol
        order = np.lexsort((local, -scores[q, :cnt]))
        assert (order == np.arange(cnt)).all()                                                         # (GPU score desc, id asc)


def test_fused_refine_equals_its_halves():
    dtype, dim, M = F16, 64, 16
    c = case(dtype, dim, M)
    ctx, queries = c["ctx"], c["queries"]
    K, R, nprobe = 10, 100, 3
    cents = nvdb_amd.synth_rows_f32(SEED + 2, 0, len(OFFSETS) - 1, dim)

    def halves(cx, row_base):
        ids, _, _ = cx.pq_search_ivf(queries, R, nprobe)
        cand = np.where(ids == U64MAX, np.uint64(0xFFFFFFFF), ids - np.uint64(row_base)).astype(np.uint32)
        rid, rdist = cx.refine_l2_topk(queries, cand, K)
        return rid, rdist

    ctx.set_centroids(cents)
    rid, rdist = halves(ctx, ROW_BASE)
    fi, fd = ctx.pq_refine_ivf(queries, K, R, nprobe)
    assert (rid != 0xFFFFFFFF).any()
    assert np.array_equal(fi, np.where(rid == 0xFFFFFFFF, U64MAX, rid.astype(np.uint64) + np.uint64(ROW_BASE)))
    assert np.array_equal(fd.view(np.uint32), rdist.view(np.uint32))
    assert np.array_equal(ctx.pq_refine_ivf(queries, K, R, nprobe, want_dist=False)[0], fi)

    # the index built from the same rows: its lists are its own, the answers come in the source corpus' ids (perm applied)
    ix = nvdb_amd.IvfIndex(ctx, cents)
    ix.pq_build(c["cb"])
    perm = ix.info()["perm"].astype(np.uint64)
    pid, _, _ = ix.ctx.pq_search_ivf(queries, R, nprobe)
    iid, _, _ = ix.pq_search(queries, R, nprobe)
    assert np.array_equal(iid, np.where(pid == U64MAX, U64MAX, np.uint64(ROW_BASE) + perm[np.minimum(pid, N - 1)]))
    rid, rdist = halves(ix.ctx, 0)
    fi, fd = ix.pq_refine(queries, K, R, nprobe)
    assert np.array_equal(fi, np.where(rid == 0xFFFFFFFF, U64MAX, np.uint64(ROW_BASE) + perm[np.minimum(rid, N - 1)]))
    assert np.array_equal(fd.view(np.uint32), rdist.view(np.uint32))
    ix.close()


def test_lifecycle():
    dtype, dim = F16, 32
    base, _ = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
    cb = make_codebooks(rows_f32(base, None, dtype), 4)
    q = nvdb_amd.synth_rows_f32(SEED + 1, 0, 2, dim)
    probe = probe_table(1).repeat(2, 0)
    ctx = nvdb_amd.HipContext(0)
    ctx.upload_corpus(base, dtype, None, ROW_BASE)
    ctx.set_partitions(OFFSETS)

    def no_codes():
        with pytest.raises(nvdb_amd.NvdbError) as e:
            ctx.pq_search_partitions(q, 10, probe)
        assert e.value.status == 1 and "nvdb_hip_pq_build" in str(e.value)
        assert ctx.pq_info() == dict(M=0, dsub=0, code_bytes=0)

    no_codes()
    ctx.pq_build(cb)
    for bad_m in (3, 6, 132):                                           # rejected with nothing changed
        with pytest.raises(nvdb_amd.NvdbError) as e:
            ctx.pq_build(np.zeros((bad_m, 256, max(1, dim // bad_m)), np.float32))
        assert e.value.status == 1
        assert ctx.pq_info()["M"] == 4
    assert ctx.pq_search_partitions(q, 10, probe)[2].tolist() == [10, 10]
    ctx.insert_rows(base[:1], part_of=[5])
    no_codes()
    ctx.pq_build(cb)
    live = np.ones((1, N + 1), bool)
    live[0, 50] = False
    ctx.set_row_masks(live)
    assert ctx.compact_rows(0)[0] == N
    no_codes()
    ctx.close()
