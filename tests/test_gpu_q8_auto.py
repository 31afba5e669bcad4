"""The int8 filter shadow as the library's own choice (option q8_shadow = -1, the default): built at corpus load for fp16
corpora that are large enough and fit the HBM budget, streamed by the flat search, with the fp16 filter kept beside it as
the first fallback.  Everything is compared with path 1 (the exact fp32-order kernel) on the same context: ids and score
bits, tie groups as tests/parity.py defines them.  d = 768 throughout; the thresholds are lowered so that 40K rows qualify."""
import ctypes as C

import numpy as np
import pytest

import nvdb_amd
from parity import assert_topk_equal

pytestmark = pytest.mark.gpu

SEED = 20240613
D = 768
N = 40_037                                                   # ragged: not a multiple of the 64-row tile


def _ctx(**options):
    c = nvdb_amd.HipContext(0)
    for key, v in options.items():
        c.set_option(key, v)
    return c


def _exact(c, queries, k):
    c.set_option("path", 1)
    ids, sc = c.search_batch(queries, k)
    assert c.stats()["path"] == 1
    c.set_option("path", 0)
    return ids, sc


def _assert_same(got, want, what, base32=None, queries=None):
    """ids and score bits; a boundary tie group may differ in ids only if every id carries exactly the boundary score."""
    (ids, sc), (ei, es) = got, want
    assert ids.shape == ei.shape, what
    for qi in range(len(ids)):
        score_of = None
        if base32 is not None:
            score_of = lambda i, qi=qi: np.float32(np.dot(base32[i].astype(np.float64), queries[qi].astype(np.float64)))   # noqa: E731
        assert_topk_equal(ids[qi], sc[qi], ei[qi], es[qi], score_of=score_of, what=f"{what}/q{qi}")
        assert np.array_equal(ids[qi], ei[qi]), f"{what}/q{qi}: canonical (score desc, id asc) order differs"


@pytest.fixture(scope="module")
def corpus():
    """One auto context and one q8_shadow = 0 context over the same generated fp16 rows, 200 queries (row 0 a self-match), and
    the exact answers, each computed once on the auto context."""
    auto = _ctx(q8_auto_min_rows=1024)
    auto.generate_corpus(SEED + 300, N, D, nvdb_amd.DT_F16)
    plain = _ctx(q8_shadow=0)
    plain.generate_corpus(SEED + 300, N, D, nvdb_amd.DT_F16)
    queries = nvdb_amd.synth_rows_f32(SEED + 301, 0, 200, D)
    queries[0] = nvdb_amd.synth_rows_f32(SEED + 300, 12345, 1, D)[0]
    exact = {}

    def want(nq, k):
        if (nq, k) not in exact:
            exact[(nq, k)] = _exact(auto, queries[:nq], k)
        return exact[(nq, k)]
    yield auto, plain, queries, want
    auto.close()
    plain.close()


@pytest.mark.parametrize("k", [10, 64])
@pytest.mark.parametrize("nq", [200, 64, 8])
def test_auto_builds_the_shadow_and_streams_it(corpus, nq, k):
    auto, plain, queries, want = corpus
    info = auto.shadow_info()
    assert info["resident"] and info["bytes"] == N * (D + 4) and not info["demoted"], info
    got = auto.search_batch(queries[:nq], k)
    st = auto.stats()
    assert st["path"] == 2 and st["bound_violations"] == 0 and st["overflow_queries"] == 0, st
    assert auto.shadow_info()["last_filter"] == "shadow"
    _assert_same(got, want(nq, k), f"auto/nq{nq}/k{k}")
    # the same search without the shadow: the fp16 filter, identical bits
    assert not plain.shadow_info()["resident"]
    off = plain.search_batch(queries[:nq], k)
    assert plain.stats()["path"] == 2 and plain.shadow_info()["last_filter"] == "f16"
    assert np.array_equal(got[0], off[0]) and np.array_equal(got[1].view(np.uint32), off[1].view(np.uint32))
    # the device API's sticky self-check is clean on both
    auto.search_check()
    plain.search_check()


@pytest.mark.parametrize("rule", ["few_rows", "over_budget", "f32", "i8", "d2048"])
def test_auto_builds_nothing_when_a_rule_fails(rule):
    n, d, dt, opts = 40_000, D, nvdb_amd.DT_F16, dict(q8_auto_min_rows=1024)
    if rule == "few_rows":
        opts = dict(q8_auto_min_rows=n + 1)
    elif rule == "over_budget":
        opts["q8_auto_max_mb"] = 1                          # the shadow would take 40 000 x 772 B = 29.4 MB
    elif rule == "f32":
        dt = nvdb_amd.DT_F32
    elif rule == "i8":
        dt = nvdb_amd.DT_I8
    else:
        n, d = 12_000, 2048                                  # an fp16 filter build, no int8 build
    c = _ctx(**opts)
    c.generate_corpus(SEED + 310, n, d, dt)
    info = c.shadow_info()
    assert not info["resident"] and info["bytes"] == 0 and not info["demoted"], (rule, info)
    queries = nvdb_amd.synth_rows_f32(SEED + 311, 0, 70, d)
    got = c.search_batch(queries, 10)
    st = c.stats()
    assert st["path"] == 2 and st["bound_violations"] == 0 and st["overflow_queries"] == 0, (rule, st)
    assert c.shadow_info()["last_filter"] == ("i8" if rule == "i8" else "f16")
    c.search_check()
    _assert_same(got, _exact(c, queries, 10), f"auto off/{rule}")
    c.close()


def test_a_nan_row_drops_the_shadow(oracle):
    """fmaxf drops a NaN, so the row maximum alone does not see it; its residual does.  No shadow for such a corpus."""
    n = 40_000
    base32 = nvdb_amd.synth_rows_f32(SEED + 320, 0, n, D)
    base = oracle.f32_to_f16(base32)
    base[n // 2, 300] = 0x7E00                               # a quiet NaN in the middle of the corpus
    queries = nvdb_amd.synth_rows_f32(SEED + 321, 0, 70, D)
    c = _ctx(q8_auto_min_rows=1024)
    c.upload_corpus(base, nvdb_amd.DT_F16)
    assert not c.shadow_info()["resident"]
    got = c.search_batch(queries, 10)
    assert c.shadow_info()["last_filter"] in ("f16", None)
    want = _exact(c, queries, 10)
    c.close()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    # the explicit option promises the same
    c = _ctx(q8_shadow=1)
    c.upload_corpus(base, nvdb_amd.DT_F16)
    assert not c.shadow_info()["resident"]
    c.close()


def test_an_overflowing_shadow_is_demoted_to_the_fp16_filter(oracle):
    """Rows that quantise badly (test_int8_filter_shadow_of_rows_that_quantise_badly_stays_exact's recipe: forty rows of ten times
    the norm, one row with a dominant element) set the shadow's band for EVERY query: ||q|| x the largest residual, about 0.08 where
    the scores of unit rows have sigma 1 / sqrt(768) = 0.036.  The bootstrap's threshold (k-th largest of 80 tile maxima of a
    1/8 sample, about 0.1 here) minus that band lets roughly a quarter of the first chunk through, so with the lists at their
    minimum (4k = 40 entries) the shadow overflows at any corpus size the filter path takes; 20 037 rows (one chunk) is the
    smallest used in this file.  The fp16 filter's band is 7.5e-4 x ||q|| x max||x|| = 0.0075; at 40 entries it may need the
    ladder's longest-lists rung as well (a chunk of 8 x the bootstrap's rows brings ~8k rows above ANY bootstrap threshold),
    but it is the fp16 filter, not path 1, that answers."""
    n, nq, k = 20_037, 50, 10
    base32 = nvdb_amd.synth_rows_f32(SEED + 330, 0, n, D)
    base32[100:140] *= np.float32(10.0)
    base32[200, 5] = np.float32(0.9)
    base = oracle.f32_to_f16(base32)
    base32 = oracle.f16_to_f32(base)
    queries = nvdb_amd.synth_rows_f32(SEED + 331, 0, nq, D)
    queries[0] = base32[200]
    c = _ctx(q8_auto_min_rows=1024, cand_cap=1)             # (raised to 4k by the plan: the minimum)
    c.upload_corpus(base, nvdb_amd.DT_F16)
    assert c.shadow_info()["resident"] and not c.shadow_info()["demoted"]
    first = c.search_batch(queries, k)
    st = c.stats()                                           # the FIRST attempt's statistics: the shadow's overflow
    assert st["path"] == 2 and st["overflow_queries"] > 0 and st["bound_violations"] == 0, st
    info = c.shadow_info()
    assert info["resident"] and info["demoted"] and info["last_filter"] == "f16", info     # answered by the fp16 filter, not path 1
    c.set_option("cand_cap", 0)
    second = c.search_batch(queries, k)                      # starts on the fp16 filter: nothing overflows, nothing is retried
    st = c.stats()
    assert st["path"] == 2 and st["overflow_queries"] == 0 and st["bound_violations"] == 0, st
    assert c.shadow_info()["last_filter"] == "f16" and c.shadow_info()["demoted"]
    want = _exact(c, queries, k)
    _assert_same(first, want, "demotion/first", base32, queries)
    _assert_same(second, want, "demotion/second", base32, queries)
    c.upload_corpus(base, nvdb_amd.DT_F16)                   # a reload forgets the demotion
    info = c.shadow_info()
    assert info["resident"] and not info["demoted"], info
    c.close()


def test_group_with_auto_shadows_equals_the_single_context(corpus):
    _, plain, queries, _ = corpus
    g = nvdb_amd.DeviceGroup([0, 0])
    g.set_option("q8_auto_min_rows", 1024)
    g.generate_corpus(SEED + 300, N, D, nvdb_amd.DT_F16)
    out = (C.c_uint64 * 4)()
    for rep in range(2):
        for nq in (200, 8):
            ids, sc, st = g.search_batch(queries[:nq], 10, want_stats=True)
            assert st["shards"] == 2 and st["host_merge_fallbacks"] == 0, st
            wi, ws = plain.search_batch(queries[:nq], 10)
            assert np.array_equal(ids, wi) and np.array_equal(sc.view(np.uint32), ws.view(np.uint32)), (rep, nq)
    for shard in range(2):
        assert g.lib.nvdb_hip_shadow_info(g.lib.nvdb_hip_group_ctx(g.h, shard), out) == 0
        assert out[0] == 1 and out[2] == 0 and out[3] == 2, list(out)       # resident, not demoted, the shadow streamed
    g.close()
