"""Range search on the GPU (nvdb_hip_range_search / nvdb_hip_range_results): every row whose score reaches a per-query radius.

Expected result of a query = the rows with Oracle.scores(...) >= r, ordered (score descending, id ascending, +0.0 == -0.0);
lims, ids and score BITS are compared exactly, on every route.  Radii are taken from each query's own oracle scores, so the
boundary row (and every tie with it) is hit exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import nvdb_amd
import pyoracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20250901
INF = np.float32(np.inf)


# ------------------------------------------------------------------------------------------------ helpers
def kth_best(S, k):
    """[nq] the k-th best (1-based) non-NaN score of every row of the score matrix S."""
    out = np.empty(S.shape[0], dtype=np.float32)
    for q in range(S.shape[0]):
        s = S[q][~np.isnan(S[q])]
        out[q] = np.sort(s)[::-1][min(k, len(s)) - 1]                 # (fewer rows than k: the worst score)
    return out


def above_max(S):
    return np.nextafter(kth_best(S, 1), INF).astype(np.float32)


def expected(S, radius, row_base=0):
    lims = np.zeros(S.shape[0] + 1, dtype=np.uint64)
    ids, scores = [], []
    for q in range(S.shape[0]):
        with np.errstate(invalid="ignore"):
            rows = np.nonzero(S[q] >= radius[q])[0]                  # C comparison: NaN on either side is false
        s = S[q][rows]
        order = np.lexsort((rows, -(s + np.float32(0.0))))            # score desc (+-0 equal), id asc
        ids.append(rows[order].astype(np.uint64) + np.uint64(row_base))
        scores.append(s[order])
        lims[q + 1] = lims[q] + np.uint64(len(rows))
    return lims, np.concatenate(ids) if ids else np.zeros(0, np.uint64), np.concatenate(scores) if scores else np.zeros(0, np.float32)


def check(ctx, queries, radius, S, row_base=0, what=""):
    radius = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (queries.shape[0],)))
    lims, ids, scores = ctx.range_search(queries, radius)
    el, ei, es = expected(S, radius, row_base)
    assert np.array_equal(lims, el), (what, "lims", np.nonzero(np.diff(lims.astype(np.int64)) != np.diff(el.astype(np.int64)))[0][:8])
    assert np.array_equal(ids, ei), (what, "ids")
    assert np.array_equal(scores.view(np.uint32), es.view(np.uint32)), (what, "score bits")
    st = ctx.stats()
    assert st["bound_violations"] == 0, st
    return (lims, ids, scores), st


def mixed_radii(S):
    """Every query gets one of: just above its best score (empty), its 1st / 10th / 300th best (boundary and ties included), -inf (all)."""
    kinds = [above_max(S), kth_best(S, 1), kth_best(S, 10), kth_best(S, 300), np.full(S.shape[0], -INF, np.float32)]
    return np.array([kinds[q % 5][q] for q in range(S.shape[0])], dtype=np.float32)


def score_matrix(oracle, base, dtype, queries, scales=None):
    return np.stack([oracle.scores(base, dtype, q, scales) for q in queries])


def make_ctx(base, dtype, scales=None, row_base=0, **opts):
    ctx = nvdb_amd.HipContext(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.upload_corpus(base, dtype, scales, row_base)
    return ctx


# ------------------------------------------------------------------------------------------------ shared corpora (references computed once)
@pytest.fixture(scope="module")
def f16_768(oracle):
    n, d, nq = 20007, 768, 200
    base = oracle.f32_to_f16(nvdb_amd.synth_rows_f32(SEED, 0, n, d))
    queries = np.ascontiguousarray(nvdb_amd.synth_rows_f32(SEED + 1, 0, nq, d))
    S = score_matrix(oracle, base, po.DT_F16, queries)
    ctx = make_ctx(base, nvdb_amd.DT_F16)
    yield dict(base=base, queries=queries, S=S, ctx=ctx)
    ctx.close()


@pytest.fixture(scope="module")
def i8_768(oracle):
    n, d, nq = 20009, 768, 200
    base, scales = oracle.quantize_i8(nvdb_amd.synth_rows_f32(SEED + 2, 0, n, d))
    queries = np.ascontiguousarray(nvdb_amd.synth_rows_f32(SEED + 3, 0, nq, d))
    S = score_matrix(oracle, base, po.DT_I8, queries, scales)
    return dict(base=base, scales=scales, queries=queries, S=S)


# ------------------------------------------------------------------------------------------------ fp16 / int8 d = 768, every route
@pytest.mark.parametrize("nq", [5, 200])
def test_f16_768_routes_agree_with_oracle(f16_768, nq):
    """n = 20 007 (padded corpus); nq = 5: the NB = 1 build, nq = 200: the m16 build on two query tiles.  path 2, 1, 0 identical."""
    ctx, q, S = f16_768["ctx"], f16_768["queries"][:nq], f16_768["S"][:nq]
    radius = mixed_radii(S)
    got = {}
    try:
        for path, want in ((2, 5), (1, 6), (0, 5)):
            ctx.set_option("path", path)
            got[path], st = check(ctx, q, radius, S, what=f"path {path}")
            assert st["path"] == want, st
            assert st["rows_scanned"] > 0
    finally:
        ctx.set_option("path", 0)
    for path in (1, 0):
        for a, b in zip(got[2], got[path]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), path
    # the same radius for every query, as a scalar
    r = float(kth_best(S, 10).min())
    check(ctx, q, r, S, what="scalar radius")


@pytest.mark.parametrize("nq", [5, 200])
def test_i8_768_routes_agree_with_oracle(i8_768, nq):
    """n = 20 009; the filter_i8s small-batch and large-batch builds."""
    ctx = make_ctx(i8_768["base"], nvdb_amd.DT_I8, i8_768["scales"])
    q, S = i8_768["queries"][:nq], i8_768["S"][:nq]
    radius = mixed_radii(S)
    got = {}
    for path, want in ((2, 5), (1, 6), (0, 5)):
        ctx.set_option("path", path)
        got[path], st = check(ctx, q, radius, S, what=f"path {path}")
        assert st["path"] == want, st
    for path in (1, 0):
        for a, b in zip(got[2], got[path]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), path
    ctx.close()


def test_i8_negative_row_scale_takes_the_in_loop_build(oracle, i8_768):
    scales = i8_768["scales"].copy()
    scales[5::97] *= np.float32(-1.0)
    nq = 200
    q = i8_768["queries"][:nq]
    S = i8_768["S"][:nq].copy()
    S[:, 5::97] = score_matrix(oracle, np.ascontiguousarray(i8_768["base"][5::97]), po.DT_I8, q, np.ascontiguousarray(scales[5::97]))
    ctx = make_ctx(i8_768["base"], nvdb_amd.DT_I8, scales, path=2)
    _, st = check(ctx, q, mixed_radii(S), S)
    assert st["path"] == 5
    ctx.close()


# ------------------------------------------------------------------------------------------------ the other filter families
@pytest.mark.parametrize("dtype,d", [("f16", 1024), ("f16", 2048), ("f32", 100), ("i8", 384), ("i8", 100)])
def test_other_filter_families(oracle, dtype, d):
    """fp16 d = 1024 (MB = 1), d = 2048 (K-split), fp32 d = 100 (zero-padded fp16 shadow), int8 d = 384, d = 100 (padded int8 shadow)."""
    n, nq = 6000 + 11, 40
    rows = nvdb_amd.synth_rows_f32(SEED + 10 + d, 0, n, d)
    queries = np.ascontiguousarray(nvdb_amd.synth_rows_f32(SEED + 11 + d, 0, nq, d))
    scales = None
    if dtype == "f16":
        base, dt = oracle.f32_to_f16(rows), po.DT_F16
    elif dtype == "f32":
        base, dt = rows, po.DT_F32
    else:
        (base, scales), dt = oracle.quantize_i8(rows), po.DT_I8
    S = score_matrix(oracle, base, dt, queries, scales)
    ctx = make_ctx(base, dt, scales)
    radius = mixed_radii(S)
    got = {}
    for path, want in ((2, 5), (1, 6)):
        ctx.set_option("path", path)
        got[path], st = check(ctx, queries, radius, S, what=f"{dtype} d={d} path {path}")
        assert st["path"] == want, st
    for a, b in zip(got[2], got[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    ctx.close()


def test_q8_shadow_fp16_filter_and_exact_agree(f16_768):
    n, nq = 20000, 200
    base, q, S = f16_768["base"][:n], f16_768["queries"][:nq], np.ascontiguousarray(f16_768["S"][:nq, :n])
    radius = mixed_radii(S)
    shadow = make_ctx(base, nvdb_amd.DT_F16, q8_shadow=1, path=2)
    plain = make_ctx(base, nvdb_amd.DT_F16, q8_shadow=0, path=2)
    a, st = check(shadow, q, radius, S, what="q8 shadow")
    assert st["path"] == 5 and shadow.shadow_info()["resident"] and shadow.shadow_info()["last_filter"] == "shadow"
    b, st = check(plain, q, radius, S, what="fp16 filter")
    assert st["path"] == 5 and plain.shadow_info()["last_filter"] == "f16"
    plain.set_option("path", 1)
    c, st = check(plain, q, radius, S, what="exact")
    assert st["path"] == 6
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and np.array_equal(x.view(np.uint8), z.view(np.uint8))
    assert not shadow.shadow_info()["demoted"]                         # a generous radius says nothing about the corpus
    shadow.close()
    plain.close()


# ------------------------------------------------------------------------------------------------ exact-only shapes
@pytest.mark.parametrize("dtype,d,n", [("i8", 7, 5003), ("f16", 300, 3001), ("f16", 768, 1), ("f16", 768, 63)])
def test_exact_route_shapes(oracle, dtype, d, n):
    """Dims without a filter build of their own and corpora below the filter route's size: option path = 1 (and whatever the automatic
    choice is) against the oracle."""
    nq = 12
    rows = nvdb_amd.synth_rows_f32(SEED + 30 + d + n, 0, n, d)
    queries = np.ascontiguousarray(nvdb_amd.synth_rows_f32(SEED + 31 + d + n, 0, nq, d))
    scales = None
    if dtype == "f16":
        base, dt = oracle.f32_to_f16(rows), po.DT_F16
    else:
        (base, scales), dt = oracle.quantize_i8(rows), po.DT_I8
    S = score_matrix(oracle, base, dt, queries, scales)
    ctx = make_ctx(base, dt, scales, path=1)
    a, st = check(ctx, queries, mixed_radii(S), S, what=f"{dtype} d={d} n={n} path 1")
    assert st["path"] == 6, st
    ctx.set_option("path", 0)
    b, st = check(ctx, queries, mixed_radii(S), S, what=f"{dtype} d={d} n={n} path 0")
    assert st["path"] == (6 if n < 2048 else 5), st                   # (small dims stream a zero-padded shadow copy)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    ctx.close()


# ------------------------------------------------------------------------------------------------ ties, odd inputs
def test_ties_every_copy_in_id_order(oracle, f16_768):
    """Each row stored four times; the radius is a duplicated score: the four copies of the boundary row are all there, ids ascending."""
    rows, nq = f16_768["base"][:2000], 16
    base = np.ascontiguousarray(np.tile(rows, (4, 1)))
    q = f16_768["queries"][:nq]
    S = np.ascontiguousarray(np.tile(f16_768["S"][:nq, :2000], (1, 4)))
    radius = kth_best(S, 10)                                           # inside a group of four equal scores (9 .. 12)
    ctx = make_ctx(base, nvdb_amd.DT_F16)
    for path, want in ((2, 5), (1, 6)):
        ctx.set_option("path", path)
        (lims, ids, scores), st = check(ctx, q, radius, S, what=f"ties path {path}")
        assert st["path"] == want
        assert np.all(np.diff(lims.astype(np.int64)) == 12)
        assert np.all(np.diff(ids[:4].astype(np.int64)) == 2000) and len(np.unique(scores[:4].view(np.uint32))) == 1
    ctx.close()


def test_non_finite_queries_and_radii_inside_a_batch(oracle, f16_768):
    ctx, base = f16_768["ctx"], f16_768["base"]
    q = f16_768["queries"][:20].copy()
    q[3, 17] = np.nan
    q[7, 400] = np.inf
    q[11, :] = 0.0
    q[12, :] = 0.0
    S = f16_768["S"][:20].copy()
    for i in (3, 7, 11, 12):
        S[i] = oracle.scores(base, po.DT_F16, q[i])
    radius = kth_best(f16_768["S"][:20], 10)
    radius[3] = -INF                                                   # every score is NaN: nothing belongs
    radius[7] = 0.0                                                    # +inf scores belong, -inf and NaN scores do not
    radius[5] = np.nan                                                 # a NaN radius: empty
    radius[11], radius[12] = np.float32(0.0), np.float32(-0.0)        # all-zero query: every row, whichever zero
    try:
        for path in (2, 1):
            ctx.set_option("path", path)
            (lims, _, _), st = check(ctx, q, radius, S, what=f"non-finite path {path}")
            n = np.diff(lims.astype(np.int64))
            assert n[3] == 0 and n[5] == 0 and n[11] == base.shape[0] and n[12] == base.shape[0] and n[0] == 10
            assert n[7] == int(np.sum(S[7] == INF))
            if path == 2:
                assert st["path"] == 5 and st["overflow_queries"] >= 5, st   # redone on the exact route: 3, 5, 7 and the two that return every row
    finally:
        ctx.set_option("path", 0)


# ------------------------------------------------------------------------------------------------ overflow handling
def test_list_overflow_redoes_only_the_flagged_queries(f16_768):
    ctx, nq = f16_768["ctx"], 40
    q, S = f16_768["queries"][:nq], f16_768["S"][:nq]
    radius = kth_best(S, 300)
    radius[::2] = kth_best(S, 1)[::2]
    try:
        ctx.set_option("path", 2)
        ctx.set_option("cand_cap", 64)
        _, st = check(ctx, q, radius, S, what="cand_cap 64")
        assert st["path"] == 5 and 0 < st["overflow_queries"] <= nq // 2, st
        ctx.set_option("cand_cap", 0)
        radius = kth_best(S, 10)
        radius[[4, 19, 33]] = kth_best(S, 9000)[[4, 19, 33]]
        _, st = check(ctx, q, radius, S, what="9000th best")
        assert st["path"] == 5 and st["overflow_queries"] == 3, st
    finally:
        ctx.set_option("cand_cap", 0)
        ctx.set_option("path", 0)


# ------------------------------------------------------------------------------------------------ conventions
def test_results_before_any_range_search_are_invalid(f16_768):
    ctx = make_ctx(f16_768["base"][:3000], nvdb_amd.DT_F16)
    ids, sc = np.zeros(4, np.uint64), np.zeros(4, np.float32)
    assert ctx.lib.nvdb_hip_range_results(ctx.h, ids.ctypes.data, sc.ctypes.data) == 1
    ctx.close()


def test_conventions(oracle, f16_768):
    ctx, base, q, S = f16_768["ctx"], f16_768["base"], f16_768["queries"], f16_768["S"]
    L = ctx.lib
    # nq = 0
    lims = np.full(1, 77, dtype=np.uint64)
    assert L.nvdb_hip_range_search(ctx.h, None, 0, None, lims.ctypes.data, None) == 0 and lims[0] == 0
    # null pointers
    r5 = np.zeros(5, np.float32)
    lims6 = np.zeros(6, np.uint64)
    assert L.nvdb_hip_range_search(ctx.h, q.ctypes.data, 5, r5.ctypes.data, None, None) == 1
    assert L.nvdb_hip_range_search(ctx.h, None, 5, r5.ctypes.data, lims6.ctypes.data, None) == 1
    assert L.nvdb_hip_range_search(ctx.h, q.ctypes.data, 5, None, lims6.ctypes.data, None) == 1
    assert L.nvdb_hip_range_results(ctx.h, None, None) == 1
    # the result budget: lims complete, nothing held
    try:
        ctx.set_option("range_max_mb", 1)
        with pytest.raises(nvdb_amd.NvdbError) as e:
            ctx.range_search(q[:5], -INF)
        assert e.value.status == 3 and "range_max_mb" in str(e.value) and str(5 * base.shape[0]) in str(e.value)
        assert np.array_equal(e.value.lims, expected(S[:5], np.full(5, -INF, np.float32))[0])
        ids, sc = np.zeros(8, np.uint64), np.zeros(8, np.float32)
        assert L.nvdb_hip_range_results(ctx.h, ids.ctypes.data, sc.ctypes.data) == 1
    finally:
        ctx.set_option("range_max_mb", 4096)
    # a flat search after a range search shares its workspace
    check(ctx, q[:64], kth_best(S[:64], 10), S[:64])
    ids, sc = ctx.search_batch(q[:64], 10)
    ri, rs = oracle.flat_topk(base, po.DT_F16, q[:64], 10)
    assert np.array_equal(ids, ri) and np.array_equal(sc.view(np.uint32), rs.view(np.uint32))
    # ... and a range search after a flat search
    check(ctx, q[:64], kth_best(S[:64], 10), S[:64])
    # a new corpus invalidates the held results
    ctx2 = make_ctx(base[:3000], nvdb_amd.DT_F16)
    ctx2.range_search(q[:4], kth_best(S[:4, :3000], 3))
    ctx2.upload_corpus(base[:2500], nvdb_amd.DT_F16)
    ids, sc = np.zeros(64, np.uint64), np.zeros(64, np.float32)
    assert ctx2.lib.nvdb_hip_range_results(ctx2.h, ids.ctypes.data, sc.ctypes.data) == 1
    ctx2.close()


def test_sub_batch_boundary(oracle):
    """nq = 1030: a sub-batch of 1024 and one of 6."""
    n, d, nq = 4096, 128, 1030
    base = oracle.f32_to_f16(nvdb_amd.synth_rows_f32(SEED + 50, 0, n, d))
    queries = np.ascontiguousarray(nvdb_amd.synth_rows_f32(SEED + 51, 0, nq, d))
    S = score_matrix(oracle, base, po.DT_F16, queries)
    ctx = make_ctx(base, nvdb_amd.DT_F16)
    radius = kth_best(S, 10)
    radius[1::7] = kth_best(S, 300)[1::7]
    radius[1027] = -INF
    _, st = check(ctx, queries, radius, S)
    assert st["path"] == 5 and st["overflow_queries"] == 1, st
    ctx.set_option("path", 1)
    _, st = check(ctx, queries, radius, S)
    assert st["path"] == 6
    ctx.close()


def test_global_row_base_is_added(f16_768):
    n, nq = 5000, 9
    base, q, S = f16_768["base"][:n], f16_768["queries"][:nq], np.ascontiguousarray(f16_768["S"][:nq, :n])
    ctx = make_ctx(base, nvdb_amd.DT_F16, row_base=1 << 33)
    for path in (2, 1):
        ctx.set_option("path", path)
        (_, ids, _), _ = check(ctx, q, mixed_radii(S), S, row_base=1 << 33)
        assert ids.min() >= (1 << 33)
    ctx.close()


# ------------------------------------------------------------------------------------------------ the C++ host layer
def test_host_layer_range_search_dot(tmp_path, f16_768):
    """nvdb::FlatIndexHIP::range_search_dot / _batch (three host threads at once, serialised by the index) == the ctypes call."""
    L = C.CDLL(os.path.join(ROOT, "nano-vectordb_amd", "lib", "libnvdb_host_capi.so"))
    L.nvdb_host_dataset_open.restype = C.c_void_p
    L.nvdb_host_dataset_open.argtypes = [C.c_char_p]
    L.nvdb_host_dataset_close.argtypes = [C.c_void_p]
    L.nvdb_host_last_error.restype = C.c_char_p
    L.nvdb_host_hip_range_search.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    n, nq = 6000, 24
    base, q, S = f16_768["base"][:n], np.ascontiguousarray(f16_768["queries"][:nq]), np.ascontiguousarray(f16_768["S"][:nq, :n])
    radius = mixed_radii(S)
    ctx = make_ctx(base, nvdb_amd.DT_F16)
    (want_l, want_i, want_s), _ = check(ctx, q, radius, S)
    ctx.close()
    p = str(tmp_path / "b16.vecbin")
    po.write_vecbin(p, base, po.DT_F16)
    h = L.nvdb_host_dataset_open(p.encode())
    assert h, L.nvdb_host_last_error()
    lims = np.zeros(nq + 1, np.uint64)
    ids, sc = np.zeros(len(want_i), np.uint64), np.zeros(len(want_i), np.float32)
    rc = L.nvdb_host_hip_range_search(h, q.ctypes.data, nq, radius.ctypes.data, 3, lims.ctypes.data, len(ids), ids.ctypes.data, sc.ctypes.data)
    L.nvdb_host_dataset_close(h)
    assert rc == 0, L.nvdb_host_last_error()
    assert np.array_equal(lims, want_l) and np.array_equal(ids, want_i) and np.array_equal(sc.view(np.uint32), want_s.view(np.uint32))
