"""Exact running thresholds on the int8-shadow flat search (option shadow_exact_thr, default 1): the thresholding selects re-score
their best 2k entries from the fp16 rows and put ONE error bound under that exact k-th best score, instead of two bounds under the
k-th list score.  Results must not move by a bit -- option on == option off == path 1 == the oracle -- while fewer rows pass the
filter's first stage and fewer candidates reach the rescore.  Corpora of 200 009 rows (several chunks at every batch size) with
q8_shadow = 1 set before the load; the automatic rule would want 2^20 rows."""
import numpy as np
import pytest

import nvdb_amd
import pyoracle as po

pytestmark = pytest.mark.gpu

SEED = 20240613
N = 200_009
KMAX = 64
STAT_KEYS = ("path", "chunks", "rows_scanned", "candidates", "overflow_queries", "bound_violations", "i8_stage1_tiles", "i8_stage2_blocks")


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _search(c, queries, k, thr):
    c.set_option("shadow_exact_thr", thr)
    got = c.search_batch(queries, k)
    st = c.stats()
    info = c.shadow_info()
    c.set_option("shadow_exact_thr", 1)
    return got, st, info


def _exact(c, queries, k):
    c.set_option("path", 1)
    got = c.search_batch(queries, k)
    assert c.stats()["path"] == 1
    c.set_option("path", 0)
    return got


def _tricky_queries(seed, nq, d):
    """test_int8_two_stage_kernel_matches_two_plane_kernel's query tricks"""
    queries = nvdb_amd.synth_rows_f32(seed, 0, nq, d)
    if nq > 5:
        queries[3] *= np.float32(977.0)
        queries[4, :7] *= np.float32(31.0)                   # heavy-tailed query
        queries[5] = np.round(queries[5] * 40) / 40          # few distinct levels
    return queries


@pytest.fixture(scope="module", params=[768, 384])
def shadowed(request, oracle):
    """One shadow context per dim over generated fp16 rows, 300 queries, and the oracle's top-64 of every query -- computed once;
    the top-k of a smaller k is its prefix (one total order: score descending, id ascending)."""
    d = request.param
    c = nvdb_amd.HipContext(0)
    c.set_option("q8_shadow", 1)
    c.generate_corpus(SEED + 600 + d, N, d, nvdb_amd.DT_F16)
    assert c.shadow_info()["resident"]
    base, _ = nvdb_amd.synth_corpus(SEED + 600 + d, 0, N, d, nvdb_amd.DT_F16)
    queries = _tricky_queries(SEED + 601 + d, 300, d)
    ref = oracle.flat_topk(base, po.DT_F16, queries, KMAX)
    totals = {"candidates": [0, 0], "i8_stage1_tiles": [0, 0]}
    yield c, d, queries, ref, totals
    c.close()


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("nq", [300, 64, 1])
def test_exact_thresholds_keep_every_bit_and_cut_the_survivors(shadowed, nq, k):
    c, d, queries, (ref_ids, ref_sc), totals = shadowed
    q = queries[:nq]
    on, st_on, info_on = _search(c, q, k, 1)
    off, st_off, info_off = _search(c, q, k, 0)
    for st, info in ((st_on, info_on), (st_off, info_off)):
        assert st["path"] == 2 and st["bound_violations"] == 0 and st["overflow_queries"] == 0, st
        assert info["resident"] and not info["demoted"] and info["last_filter"] == "shadow", info
    assert _same(on, off), "option on != option off"
    assert _same(on, _exact(c, q, k)), "option on != path 1"
    assert np.array_equal(on[0], ref_ids[:nq, :k]) and np.array_equal(on[1].view(np.uint32), ref_sc[:nq, :k].view(np.uint32)), "!= oracle"
    c.search_check()
    # the same launches (the plan does not know the option) over fewer survivors
    assert st_on["chunks"] == st_off["chunks"] and st_on["rows_scanned"] == st_off["rows_scanned"]
    print(f"d={d} nq={nq} k={k}: candidates {st_on['candidates']} / {st_off['candidates']}, stage-1 tiles {st_on['i8_stage1_tiles']} / {st_off['i8_stage1_tiles']}")
    for key in totals:
        assert st_on[key] <= st_off[key], (key, st_on[key], st_off[key])
        totals[key][0] += st_on[key]
        totals[key][1] += st_off[key]


def test_survivors_fall_in_total(shadowed):
    """The sums over the cases above on this dim's context (run alone: over one case of its own)."""
    c, d, queries, _, totals = shadowed
    if totals["candidates"][1] == 0:
        for thr in (1, 0):
            _, st, _ = _search(c, queries, 10, thr)
            for key in totals:
                totals[key][1 - thr] += st[key]
    for key, (on, off) in totals.items():
        assert off > 0 and on < off, (d, key, on, off)


@pytest.fixture(scope="module")
def adversarial(oracle):
    """An uploaded fp16 corpus (d = 768) with 40 exact copies of one row spread over the chunks and a cluster of 200 rows whose scores
    against their centre lie inside one error bound of each other (the shadow's bound is about 0.0075 ||q|| here)."""
    d = 768
    base32 = nvdb_amd.synth_rows_f32(SEED + 700, 0, N, d)
    rs = np.random.RandomState(7)
    dup_src = 77_777
    dup_at = np.sort(rs.choice(N, size=40, replace=False))
    dup_at[0], dup_at[-1] = 11, N - 3                        # the bootstrap's rows and the last tile among them
    base32[dup_at] = base32[dup_src]
    centre = nvdb_amd.synth_rows_f32(SEED + 701, 0, 1, d)[0]
    cl_at = rs.choice(np.setdiff1d(np.arange(N), np.append(dup_at, dup_src)), size=200, replace=False)
    noise = nvdb_amd.synth_rows_f32(SEED + 702, 0, 200, d)
    base32[cl_at] = centre[None, :] * (1.0 - 0.004 * rs.rand(200, 1)).astype(np.float32) + np.float32(0.01) * noise
    base = oracle.f32_to_f16(base32)
    c = nvdb_amd.HipContext(0)
    c.set_option("q8_shadow", 1)
    c.upload_corpus(base, nvdb_amd.DT_F16)
    assert c.shadow_info()["resident"]
    queries = _tricky_queries(SEED + 703, 60, d)             # (<= 64 queries: the longest lists, so that the two-bound band of option 0 fits them too)
    queries[0] = oracle.f16_to_f32(base[dup_src:dup_src + 1])[0]     # 41 rows tie at the top: the k-th place is decided by id
    queries[1] = centre                                              # ~200 rows inside one bound of the k-th best
    queries[2] = centre * np.float32(0.37) + np.float32(0.02) * noise[0]
    yield c, base, queries
    c.close()


@pytest.mark.parametrize("k", [10, 64])
@pytest.mark.parametrize("nq", [60, 3])
def test_ties_and_clusters_at_the_kth_place(adversarial, oracle, nq, k):
    c, base, queries = adversarial
    q = queries[:nq]
    on, st_on, info = _search(c, q, k, 1)
    off, st_off, _ = _search(c, q, k, 0)
    assert st_on["path"] == 2 and st_on["bound_violations"] == 0 and st_on["overflow_queries"] == 0, st_on
    assert st_off["bound_violations"] == 0 and st_off["overflow_queries"] == 0, st_off
    assert info["last_filter"] == "shadow" and not info["demoted"], info
    ref_ids, ref_sc = oracle.flat_topk(base, po.DT_F16, q[:3], k)
    assert _same(on, off) and _same(on, _exact(c, q, k))
    assert np.array_equal(on[0][:3], ref_ids) and np.array_equal(on[1][:3].view(np.uint32), ref_sc.view(np.uint32))
    assert len(np.unique(on[1][0, :min(k, 41)])) == 1          # the tie is what the query met
    assert st_on["candidates"] <= st_off["candidates"] and st_on["i8_stage1_tiles"] <= st_off["i8_stage1_tiles"]
    c.search_check()


def test_a_query_of_zeros():
    """Every score ties at 0: every row passes any threshold under that, the query's list overflows and the retry ladder answers
    (demoting the shadow: hence a context of its own) -- with the option as without it."""
    d = 768
    q = _tricky_queries(SEED + 711, 9, d)
    q[4] = 0.0
    res = {}
    for thr in (1, 0):
        c = nvdb_amd.HipContext(0)
        c.set_option("q8_shadow", 1)
        c.generate_corpus(SEED + 710, N, d, nvdb_amd.DT_F16)
        res[thr], st, _ = _search(c, q, 10, thr)
        assert st["bound_violations"] == 0 and st["overflow_queries"] > 0, st
        assert _same(res[thr], _exact(c, q, 10)), thr
        c.close()
    assert _same(res[1], res[0])
    assert res[1][0][4].tolist() == list(range(10)) and not res[1][1][4].any()


def test_smallest_bootstraps_the_plan_allows(adversarial):
    """"Fewer than k real entries keep the old bound" guards the select against a list shorter than k.  No option reaches it from
    outside: boot_tiles is a floor under the plan's max(64, 8k) tile maxima, and the exact bootstrap chunk (mfma_boot = 0) has at
    least 256 rows >= k.  What can be forced is the shortest first list: k = 64 out of a 256-row exact bootstrap chunk (M = 2k =
    half the chunk, list scores already exact), and the smallest MFMA bootstrap (64 tile maxima at k = 1: M = 2)."""
    c, _, queries = adversarial
    q = queries[:20]
    for opts, k in ((dict(mfma_boot=0, chunk0_rows=256), 64), (dict(mfma_boot=0, chunk0_rows=256), 10), (dict(), 1)):
        for key, v in opts.items():
            c.set_option(key, v)
        try:
            on, st_on, info = _search(c, q, k, 1)
            off, st_off, _ = _search(c, q, k, 0)
            assert st_on["path"] == 2 and info["last_filter"] == "shadow" and not info["demoted"], (st_on, info)
            assert st_on["bound_violations"] == 0 and st_on["overflow_queries"] == 0, st_on
            assert st_off["bound_violations"] == 0 and st_off["overflow_queries"] == 0, st_off
            assert _same(on, off) and _same(on, _exact(c, q, k))
            assert st_on["candidates"] <= st_off["candidates"]
        finally:
            c.set_option("mfma_boot", 1)
            c.set_option("chunk0_rows", 512)


def _launches_and_stats(c, queries, k):
    out = {}
    for thr in (1, 0):
        got, st, info = _search(c, queries, k, thr)
        out[thr] = (got, {key: st[key] for key in STAT_KEYS}, info["last_filter"])
    return out


@pytest.mark.parametrize("case", ["wide_k", "native_i8", "f16_no_shadow"])
def test_other_searches_do_not_see_the_option(shadowed, case):
    """k = 100 on the shadow (wide k), a native int8 corpus, an fp16 corpus without a shadow: the same statistics -- chunks, rows,
    candidates, stage counts -- and the same bits with the option on and off."""
    c, d, queries, _, _ = shadowed
    k, own = 10, None
    if case == "wide_k":
        k = 100
    else:
        own = c = nvdb_amd.HipContext(0)
        c.set_option("q8_shadow", 0)
        c.generate_corpus(SEED + 600 + d, 60_011, d, nvdb_amd.DT_I8 if case == "native_i8" else nvdb_amd.DT_F16)
        assert not c.shadow_info()["resident"]
    try:
        for nq in (300, 8):
            out = _launches_and_stats(c, queries[:nq], k)
            assert _same(out[1][0], out[0][0]), (case, nq)
            assert out[1][1] == out[0][1], (case, nq, out[1][1], out[0][1])
            assert out[1][2] == out[0][2]
            assert out[1][1]["overflow_queries"] == 0 and out[1][1]["bound_violations"] == 0
            if case != "wide_k":
                assert out[1][1]["path"] == 2 and out[1][2] == {"native_i8": "i8", "f16_no_shadow": "f16"}[case]
    finally:
        if own is not None:
            own.close()
