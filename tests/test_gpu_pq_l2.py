"""PQ shadows scored by squared L2 distance (nvdb_hip_pq_set_metric / _pq_metric / _pq_norms and every PQ search under metric 1)
against the header's rules: the norms within the bound of a chain of dim fmas over non-negative terms, the L2 order bit for bit
from the dot run's score bits and the norm bits (z = s - n / 2 is one IEEE subtraction: numpy float32 repeats it), the distances
against fp64 |q - xhat|^2 of the GPU's own reconstruction.  Fixture: test_gpu_pq.py's rows, partitions and probes, every row r
scaled by 0.5 + (r % 7) / 4 before upload: the norms spread over a factor of 4, so a scan that drops the bias or subtracts n for
n / 2 returns another order.  Kinds as test_gpu_pq4.py: plain, residual, residual under a random orthonormal rotation."""
import numpy as np
import pytest

import nvdb_amd
from test_gpu_pq import N, ROW_BASE, SEED, OFFSETS, U64MAX, F32, F16, I8, EPS, rows_f32, probe_table, union_rows, make_codebooks
from test_gpu_pq4 import make_codebooks as make_codebooks4, unpack, bits
from test_gpu_pq_residual import NPARTS, LIST_OF

pytestmark = pytest.mark.gpu

#        bits dtype dim  M   G  kind      (G: the header's group classes; nq = two full groups and a partial one)
CASES = [(8, F16, 64, 16, 8, "plain"), (8, F16, 64, 16, 8, "resid"), (8, F16, 64, 16, 8, "rot"),   # 16-byte pieces
         (8, F16, 48, 24, 4, "plain"), (8, F16, 96, 48, 2, "plain"), (8, F16, 96, 96, 1, "plain"),  # dwords; dsub 2; dsub 1
         (4, F16, 64, 32, 32, "plain"), (4, F16, 64, 32, 32, "resid"), (4, F16, 64, 32, 32, "rot"),
         (4, F16, 96, 48, 16, "plain"), (4, F16, 96, 96, 8, "plain"),
         (8, F32, 64, 16, 8, "plain"), (4, I8, 64, 32, 32, "plain")]
_cache = {}


def case(nbits, dtype, dim, M, G, kind):
    """One scaled corpus with its shadow, built once; dot: the dot metric's results at R = the largest union + 5, taken before the
    metric changes; the context is left under the L2 metric."""
    key = (nbits, dtype, dim, M, kind)
    if key not in _cache:
        f = nvdb_amd.synth_rows_f32(SEED, ROW_BASE, N, dim) * (0.5 + (np.arange(N) % 7) / 4).astype(np.float32)[:, None]
        base, scales = (f, None) if dtype == F32 else (nvdb_amd.f32_to_f16(f), None) if dtype == F16 else nvdb_amd.quantize_i8(f)
        X = rows_f32(base, scales, dtype)
        cents = np.ones((NPARTS, dim), dtype=np.float32)
        for p in range(NPARTS):
            if OFFSETS[p + 1] > OFFSETS[p]:
                cents[p] = X[int(OFFSETS[p]):int(OFFSETS[p + 1])].mean(0, dtype=np.float32)
        A = np.linalg.qr(np.random.RandomState(dim).standard_normal((dim, dim)))[0].astype(np.float32) if kind == "rot" else None
        E = X if kind == "plain" else X - cents[LIST_OF]
        cb = (make_codebooks4 if nbits == 4 else make_codebooks)(E if A is None else (E.astype(np.float64) @ A.astype(np.float64).T).astype(np.float32), M)
        ctx = nvdb_amd.HipContext(0)
        ctx.upload_corpus(base, dtype, scales, ROW_BASE)
        ctx.set_partitions(OFFSETS)
        ctx.set_centroids(cents)
        ctx.pq_build(cb, residual=kind != "plain", rotation=A)
        nq = 2 * G + 3
        queries, probe = nvdb_amd.synth_rows_f32(SEED + 1, 0, nq, dim), probe_table(nq)
        R = max(len(union_rows(p)) for p in probe) + 5
        assert ctx.pq_metric() == "dot"
        dot = ctx.pq_search_partitions(queries, R, probe)
        ctx.pq_set_metric("l2")
        codes = ctx.pq_download_codes()
        _cache[key] = dict(ctx=ctx, cb=cb, cents=cents, queries=queries, probe=probe, R=R, dot=dot, norms=ctx.pq_norms(), xhat=ctx.pq_reconstruct(),
                           codes=unpack(codes) if nbits == 4 else codes, base=base, scales=scales)
    return _cache[key]


def l2_order(dot, norms, q):
    """The header's order for query q from the dot run's bits: (local rows, z), z descending then row ascending, NaN z left out."""
    ids, scores, counts = dot
    local = (ids[q, :counts[q]] - np.uint64(ROW_BASE)).astype(np.int64)
    with np.errstate(invalid="ignore"):
        z = scores[q, :counts[q]] - np.float32(0.5) * norms[local]                                  # float32 throughout
    keep = np.array([i for i in np.lexsort((local, -z)) if not np.isnan(z[i])], dtype=np.int64)
    return local[keep], z[keep]


def check_order(c, got, R):
    ids, dist, counts = got
    for q in range(len(c["queries"])):
        local, _ = l2_order(c["dot"], c["norms"], q)
        cnt = min(R, len(local))
        assert counts[q] == cnt and np.array_equal(ids[q, :cnt], local[:cnt].astype(np.uint64) + np.uint64(ROW_BASE)), q
        assert (ids[q, cnt:] == U64MAX).all() and np.isposinf(dist[q, cnt:]).all()
        assert (dist[q, 1:cnt] >= dist[q, :cnt - 1]).all()                                          # non-decreasing along the order


@pytest.mark.parametrize("nbits,dtype,dim,M,G,kind", CASES)
def test_norms_order_and_distances(nbits, dtype, dim, M, G, kind):
    c = case(nbits, dtype, dim, M, G, kind)
    ctx, queries, probe, dsub, resid = c["ctx"], c["queries"], c["probe"], dim // M, kind != "plain"
    x64 = c["xhat"].astype(np.float64); n64 = (x64 ** 2).sum(1)
    print(f"norms: worst |n - n64| / ((dim + 1) eps n64) = {(np.abs(c['norms'] - n64) / ((dim + 1) * EPS * n64)).max():.3f}")
    assert (np.abs(c["norms"] - n64) <= (dim + 1) * EPS * n64).all()
    assert ctx.pq_metric() == "l2" and np.array_equal(bits(ctx.pq_norms(36, 66)), bits(c["norms"][36:102]))
    got = ctx.pq_search_partitions(queries, c["R"], probe)
    assert ctx.stats()["path"] == 9 and check_order(c, got, c["R"]) is None
    check_order(c, ctx.pq_search_partitions(queries, 10, probe), 10)
    qtab, marange, worst = (ctx.pq_rotate(queries) if kind == "rot" else queries), np.arange(M), 0.0
    for q in range(len(queries)):
        local, z = l2_order(c["dot"], c["norms"], q)
        q64 = queries[q].astype(np.float64)
        A64 = np.abs(qtab[q].astype(np.float64).reshape(M, 1, dsub) * c["cb"].astype(np.float64)).sum(-1)[marange, c["codes"][local]].sum(1)
        E_s = 1.01 * EPS * (resid * (-(-dim // 64) + 7) * np.abs(q64[None] * c["cents"].astype(np.float64)).sum(1)[LIST_OF[local]] + (dsub + M + resid) * A64).max()
        d64 = ((q64[None] - x64[local]) ** 2).sum(1)
        tol = 1.01 * (2 * E_s + (dim + 1) * EPS * n64[local] + 2 * EPS * np.abs(z) + (-(-dim // 64) + 7) * EPS * (q64 ** 2).sum() + EPS * np.abs(d64))
        worst = max(worst, (np.abs(got[1][q, :len(local)] - d64) / tol).max())
    print(f"worst |dist - d64| / tol: {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("nbits", [8, 4])
def test_identity_rotation_repeats_the_unrotated_norms(nbits):
    """One definition of n on both routes: the slab route (a rotation) and the code route give the same bits where A = I."""
    c = case(nbits, F16, 64, 16 if nbits == 8 else 32, 8 if nbits == 8 else 32, "plain")
    ctx = nvdb_amd.HipContext(0)
    ctx.upload_corpus(c["base"], F16, c["scales"], ROW_BASE)
    ctx.pq_build(c["cb"], rotation=np.eye(64, dtype=np.float32))
    assert ctx.pq_set_metric("l2") is None and np.array_equal(bits(ctx.pq_norms()), bits(c["norms"]))
    ctx.close()


@pytest.mark.parametrize("nbits", [8, 4])
def test_non_finite_codeword_rows_are_no_candidates(nbits):
    """Rows with +inf in sub-vector 1 find no winner there and get code 0, which is made +inf itself: exactly those rows use the
    non-finite codeword.  Their s is +-inf and their h +inf: z is NaN (no candidate) or -inf (the last candidates)."""
    M = 16 if nbits == 8 else 32
    c = case(nbits, F16, 64, M, 8 if nbits == 8 else 32, "plain")
    base, cb, hit = c["base"].copy(), c["cb"].copy(), np.arange(N) % 50 == 3
    base[hit, 64 // M] = 0x7C00
    cb[1, 0, 0] = np.inf
    ctx = nvdb_amd.HipContext(0)
    ctx.upload_corpus(base, F16, None, ROW_BASE)
    ctx.set_partitions(OFFSETS)
    ctx.pq_build(cb)
    codes = ctx.pq_download_codes()
    assert np.array_equal((unpack(codes) if nbits == 4 else codes)[:, 1] == 0, hit)
    dot = ctx.pq_search_partitions(c["queries"], c["R"], c["probe"])
    ctx.pq_set_metric("l2")
    d = dict(c, dot=dot, norms=ctx.pq_norms())
    assert np.isposinf(d["norms"][hit]).all() and np.isfinite(d["norms"][~hit]).all()
    got = ctx.pq_search_partitions(c["queries"], c["R"], c["probe"])
    check_order(d, got, c["R"])                                                                       # ids and counts: NaN z left out
    lost = dot[2].astype(np.int64) - got[2]
    assert (lost > 0).any() and (lost < [hit[union_rows(p)].sum() for p in c["probe"]]).any()         # both fates occur
    ctx.close()


def test_fused_refine_index_form_and_state():
    c = case(4, F16, 64, 32, 32, "resid")
    ctx, queries, K, R, nprobe = c["ctx"], c["queries"], 10, 100, 3

    def halves(cx, row_base):
        ids, dist, _ = cx.pq_search_ivf(queries, R, nprobe)
        assert np.isposinf(dist[ids == U64MAX]).all() and (dist[:, 1:] >= dist[:, :-1]).all()
        return cx.refine_l2_topk(queries, np.where(ids == U64MAX, np.uint64(0xFFFFFFFF), ids - np.uint64(row_base)).astype(np.uint32), K)

    rid, rdist = halves(ctx, ROW_BASE)
    fi, fd = ctx.pq_refine_ivf(queries, K, R, nprobe)
    assert (rid != 0xFFFFFFFF).any() and np.array_equal(bits(fd), bits(rdist))
    assert np.array_equal(fi, np.where(rid == 0xFFFFFFFF, U64MAX, rid.astype(np.uint64) + np.uint64(ROW_BASE)))
    ix = nvdb_amd.IvfIndex(ctx, c["cents"])                               # the index form: its own lists, the source corpus' ids
    ix.pq_build(c["cb"], residual=True)
    assert ix.pq_metric() == "dot" and ix.pq_set_metric("l2") is None and ix.pq_metric() == "l2" and ix.pq_norms(7, 3).shape == (3,)
    perm = ix.info()["perm"].astype(np.uint64)
    pid, pdist, pcnt = ix.ctx.pq_search_ivf(queries, R, nprobe)
    iid, idist, icnt = ix.pq_search(queries, R, nprobe)
    assert np.array_equal(iid, np.where(pid == U64MAX, U64MAX, np.uint64(ROW_BASE) + perm[np.minimum(pid, N - 1)])) and np.array_equal(bits(idist), bits(pdist))
    rid, rdist = halves(ix.ctx, 0)
    fi, fd = ix.pq_refine(queries, K, R, nprobe)
    assert np.array_equal(fi, np.where(rid == 0xFFFFFFFF, U64MAX, np.uint64(ROW_BASE) + perm[np.minimum(rid, N - 1)])) and np.array_equal(bits(fd), bits(rdist))
    ix.close()
    # state: back to dot repeats the dot bits; a rebuild returns the metric to dot; set_partitions drops a residual shadow and its norms
    ctx.pq_set_metric("dot")
    for a, b in zip(ctx.pq_search_partitions(queries, c["R"], c["probe"]), c["dot"]):
        assert np.array_equal(a, b)                                       # (scores hold no NaN: value equality is bit equality up to -0)
    with pytest.raises(nvdb_amd.NvdbError) as e:
        ctx.pq_norms()
    assert e.value.status == 1 and "nvdb_hip_pq_set_metric" in str(e.value)
    with pytest.raises(ValueError):
        ctx.pq_set_metric("cosine")
    ctx.pq_set_metric("l2")
    ctx.pq_build(c["cb"], residual=True)
    assert ctx.pq_metric() == "dot" and ctx.pq_set_metric("l2") is None
    ctx.set_partitions(OFFSETS)
    assert ctx.pq_metric() == "dot" and ctx.pq_info()["M"] == 0
    for call in (lambda: ctx.pq_set_metric("l2"), ctx.pq_norms):
        with pytest.raises(nvdb_amd.NvdbError) as e:
            call()
        assert e.value.status == 1 and "no PQ codes" in str(e.value)
    ctx.pq_set_metric("dot")                                              # the default already: fine without a shadow
    del _cache[(4, F16, 64, 32, "resid")]
    ctx.close()
