"""The int8 filter shadow under ONE common scale (option shadow_common_scale, csrc/shadow_scale_plan.h) and the filter build that
tests raw accumulator bits on it (shadow_i8c_kernel, csrc/kernels_filter_i8s.h).  Ids and score bits must equal path 1 and the same
corpus loaded with shadow_common_scale = 0; on a common-scale shadow the bits-domain build and the per-row build (the option set to 0
AFTER the load) must file the same candidates.  Small corpora with q8_shadow = 1 (the automatic rule would want 2^20 rows), d = 768:
  N = 390    chunk0_rows = 256: the filter streams 2 tiles behind the exact bootstrap chunk, the last 6 rows are the exact tail
  N = 4807   75 tiles (no power of two: the permuted tile order cycle-walks), k = 10 on the MFMA bootstrap, k = 64 on the exact chunk
  N = 20037  313 tiles, k = 64 on the MFMA bootstrap too
batches 129 (one query beyond a single tile of 128: the 64-queries-per-wave side of the launcher) and 1024."""
import numpy as np
import pytest

import nvdb_amd

pytestmark = pytest.mark.gpu

SEED = 20240613
D = 768


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _ctx(base, common, chunk0=None):
    c = nvdb_amd.HipContext(0)
    c.set_option("q8_shadow", 1)
    if not common:
        c.set_option("shadow_common_scale", 0)
    if chunk0:
        c.set_option("chunk0_rows", chunk0)
    c.upload_corpus(base, nvdb_amd.DT_F16)
    assert c.shadow_info()["resident"]
    return c


def _filter(c, q, k):
    c.set_option("path", 2)
    got = c.search_batch(q, k)
    st, info = c.stats(), c.shadow_info()
    assert st["path"] == 2 and st["bound_violations"] == 0 and st["overflow_queries"] == 0, st
    assert info["last_filter"] == "shadow" and not info["demoted"], info
    return got, st


def _exact(c, q, k):
    c.set_option("path", 1)
    got = c.search_batch(q, k)
    assert c.stats()["path"] == 1
    return got


def _check(common, plain, q, k, want_common=True):
    """common: the context under test; plain: the same rows loaded with shadow_common_scale = 0"""
    assert common.shadow_scale_info()["common"] == want_common and not plain.shadow_scale_info()["common"]
    ref = _exact(plain, q, k)
    got, st = _filter(common, q, k)
    assert _same(got, ref), "common-scale shadow != path 1"
    assert _same(_exact(common, q, k), ref)
    off, st_off = _filter(plain, q, k)
    assert _same(off, ref), "per-row shadow != path 1"
    if want_common:
        # the per-row build on the SAME common-scale shadow: same log, same candidates
        common.set_option("shadow_common_scale", 0)
        twin, st_twin = _filter(common, q, k)
        common.set_option("shadow_common_scale", -1)
        assert _same(twin, ref)
        assert st_twin["candidates"] == st["candidates"] and st_twin["chunks"] == st["chunks"] and st_twin["rows_scanned"] == st["rows_scanned"], (st, st_twin)
    print(f"n={common.corpus_info()['n']} nq={len(q)} k={k}: candidates {st['candidates']} (per-row shadow {st_off['candidates']}), "
          f"stage-1 tiles {st['i8_stage1_tiles']} / {st_off['i8_stage1_tiles']}")
    return st


@pytest.fixture(scope="module", params=[390, 4807, 20037])
def pair(request):
    n = request.param
    base = nvdb_amd.synth_rows_f32(SEED + 800 + n, 0, n, D).astype(np.float16)
    chunk0 = 256 if n < 1000 else None
    a, b = _ctx(base, True, chunk0), _ctx(base, False, chunk0)
    queries = nvdb_amd.synth_rows_f32(SEED + 801 + n, 0, 1024, D)
    queries[3] *= np.float32(977.0)
    queries[4, :7] *= np.float32(31.0)
    queries[5] = np.round(queries[5] * 40) / 40
    yield a, b, queries
    a.close()
    b.close()


@pytest.mark.parametrize("k", [10, 64])
@pytest.mark.parametrize("nq", [129, 1024])
def test_common_scale_keeps_every_bit(pair, nq, k):
    a, b, queries = pair
    info = a.shadow_scale_info()
    assert info["scale"] > 0 and 0 < info["resid_common"] <= info["resid_row"] * 1.25, info
    _check(a, b, queries[:nq], k)


def _edge_corpus(n):
    """Every row scaled so that its largest |element| is exactly M (fp16-exact): every reference scale equals s_c, every row's largest
    element sits at the clipping edge 127 x s_c.  Rows 5 / 6: all +M / all -M (every byte +127 / -127: the largest |H| a flat query
    reaches); 40 copies of row 77 and a cluster of 200 near-copies of one centre (ties and near-ties at the bar)."""
    M = np.float32(0.125)
    b = nvdb_amd.synth_rows_f32(SEED + 900, 0, n, D)
    rs = np.random.RandomState(11)
    centre = nvdb_amd.synth_rows_f32(SEED + 901, 0, 1, D)[0]
    cl_at = rs.choice(np.arange(100, n), size=200, replace=False)
    b[cl_at] = centre[None, :] * (1.0 - 0.004 * rs.rand(200, 1)).astype(np.float32) + np.float32(0.002) * nvdb_amd.synth_rows_f32(SEED + 902, 0, 200, D)
    dup_at = np.setdiff1d(rs.choice(np.arange(100, n), size=60, replace=False), cl_at)[:40]
    b[dup_at] = b[77]
    b = b / np.abs(b).max(axis=1, keepdims=True) * M
    b[5] = M
    b[6] = -M
    h = b.astype(np.float16)
    assert (np.abs(h.astype(np.float32)).max(axis=1) == M).all()
    return h, centre, dup_at


@pytest.fixture(scope="module")
def edge():
    n = 4807
    base, centre, dup_at = _edge_corpus(n)
    a, b = _ctx(base, True), _ctx(base, False)
    yield a, b, base, centre
    a.close()
    b.close()


@pytest.mark.parametrize("nq", [129, 1024])
def test_clipping_edge_extreme_rows_and_near_ties(edge, nq):
    a, b, base, centre = edge
    info = a.shadow_scale_info()
    assert info["common"] and info["scale"] == np.float32(0.125) / np.float32(127.0), info
    q = nvdb_amd.synth_rows_f32(SEED + 903, 0, nq, D)
    q[0] = 1.0                                            # flat queries: rows 5 / 6 give the largest |H|
    q[1] = -1.0
    q[2] = base[77].astype(np.float32)                    # 41 rows tie at the top
    q[3] = centre                                         # ~200 rows within one bound of each other
    q[4] = centre * np.float32(0.37)
    for k in (10, 64):
        _check(a, b, q, k)


@pytest.mark.parametrize("nq", [129, 1024])
def test_a_batch_whose_every_score_is_negative(edge, nq):
    """|rows| against negative queries: every score of the batch is below zero, the bars sit where the biased accumulator reads
    2^23 + H / 2."""
    a, b, base, _ = edge
    pos = np.abs(base.view(np.float16))
    ca, cb = _ctx(pos, True), _ctx(pos, False)
    try:
        q = -np.abs(nvdb_amd.synth_rows_f32(SEED + 904, 0, nq, D)) - np.float32(1e-3)
        got = _check(ca, cb, q, 10)
        assert (_exact(cb, q, 10)[1] < 0).all()
        assert got["candidates"] >= 10 * nq
    finally:
        ca.close()
        cb.close()


def test_outlier_declined_insert_above_the_scale_and_compaction():
    n = 4807
    base = nvdb_amd.synth_rows_f32(SEED + 910, 0, n, D).astype(np.float16)
    queries = nvdb_amd.synth_rows_f32(SEED + 911, 0, 129, D)
    # an outlier row 10x longer that quantises exactly under its own scale: under s_c every other row would pay -> declined
    out = base.copy()
    c10 = np.float16(10.0 / np.sqrt(D))
    out[1234] = c10
    out[1234, ::2] = -c10
    a, b = _ctx(out, True), _ctx(out, False)
    try:
        info = a.shadow_scale_info()
        assert not info["common"] and info["resid_common"] > 1.25 * info["resid_row"] > 0, info
        _check(a, b, queries, 10, want_common=False)
    finally:
        a.close()
        b.close()
    # insert: a row below s_c keeps the fact, a row above clears it; results stay exact; then a compaction
    a = _ctx(base, True)
    try:
        s_c = a.shadow_scale_info()["scale"]
        assert a.shadow_scale_info()["common"]
        small = (base[:3].astype(np.float32) * np.float32(0.5)).astype(np.float16)
        a.insert_rows(small)
        assert a.shadow_scale_info()["common"] and a.shadow_scale_info()["scale"] == s_c
        cur = np.concatenate([base, small])
        b = _ctx(cur, False)
        _check(a, b, queries, 10)
        b.close()
        big = (base[10:12].astype(np.float32) * np.float32(3.0)).astype(np.float16)
        a.insert_rows(big)
        assert not a.shadow_scale_info()["common"]
        cur = np.concatenate([cur, big])
        b = _ctx(cur, False)
        _check(a, b, queries, 10, want_common=False)
        b.close()
        live = np.ones((1, len(cur)), dtype=bool)
        live[0, 7::13] = False
        a.set_row_masks(live)
        n_new, old = a.compact_rows(0)
        assert n_new == int(live.sum()) and not a.shadow_scale_info()["common"]
        b = _ctx(cur[live[0]], False)
        _check(a, b, queries, 10, want_common=False)
        b.close()
    finally:
        a.close()
    # a compaction of a common-scale shadow keeps the fact (every scale entry is still s_c)
    a = _ctx(base, True)
    try:
        live = np.ones((1, n), dtype=bool)
        live[0, 5::7] = False
        a.set_row_masks(live)
        a.compact_rows(0)
        assert a.shadow_scale_info()["common"]
        b = _ctx(base[live[0]], False)
        _check(a, b, queries, 10)
        b.close()
    finally:
        a.close()
