"""Option i8_dense8 (default 1): the int8 flat search at d = 768, batches > 128, runs the 16x16x64 logged kernel on 8 waves of 32
queries instead of 4 waves of 64.  Ids, score bits and the candidates that reach the rescore must not move: i8_dense8 = 1 == 0 == the
exact kernel (path 1).

`i8_stage1_tiles` counts (wave, 32-row block) pairs that went to the log, and a wave is 64 queries on the 4-wave build and 32 on the
8-wave build -- each 64-query group of the one is two 32-query groups of the other.  So under the same thresholds a flagged pair of
the 4-wave build is one or two flagged pairs of the 8-wave build: tiles(0) <= tiles(1) <= 2 x tiles(0), and no equality where both
halves of a group are flagged (N = 10M, batch 1024, k = 10 on the int8 shadow: 635 794 against 725 989 with 33 114 candidates and
identical results in both; native int8: 296 034 against 323 171).  That relation is what is asserted, next to equal `candidates`,
which the thresholds of every launch determine.

fp16 corpus of 200 037 rows (a padded last tile) with q8_shadow = 1 set before the load, the bench's generator and queries."""
import numpy as np
import pytest

import nvdb_amd

pytestmark = pytest.mark.gpu

SEED = 20240613
N, D = 200_037, 768


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _run(c, q, k, dense8):
    c.set_option("i8_dense8", dense8)
    try:
        got = c.search_batch(q, k)
        st = c.stats()
        c.search_check()
    finally:
        c.set_option("i8_dense8", 1)
    assert st["path"] == 2 and st["bound_violations"] == 0 and st["overflow_queries"] == 0, st
    return got, st


def _exact(c, q, k):
    c.set_option("path", 1)
    try:
        got = c.search_batch(q, k)
        assert c.stats()["path"] == 1
        c.search_check()
    finally:
        c.set_option("path", 0)
    return got


@pytest.fixture(scope="module")
def queries():
    return nvdb_amd.synth_rows_f32(SEED + 1, 0, 1024, D)


@pytest.fixture(scope="module")
def shadow_ctx():
    c = nvdb_amd.HipContext(0)
    c.set_option("q8_shadow", 1)
    c.generate_corpus(SEED, N, D, nvdb_amd.DT_F16)
    assert c.shadow_info()["resident"]
    yield c
    c.close()


@pytest.fixture(scope="module")
def exact_top64(shadow_ctx, queries):
    """path 1 once for all 1024 queries at k = 64; a smaller k is its prefix (one total order: score descending, id ascending)"""
    return _exact(shadow_ctx, queries, 64)


def _check_pair(c, q, k, want):
    on, st_on = _run(c, q, k, 1)
    off, st_off = _run(c, q, k, 0)
    print(f"nq={len(q)} k={k}: candidates {st_on['candidates']} / {st_off['candidates']}, stage-1 tiles {st_on['i8_stage1_tiles']} / {st_off['i8_stage1_tiles']}, chunks {st_on['chunks']}")
    assert _same(on, off), "i8_dense8 = 1 != 0"
    assert _same(on, want), "i8_dense8 = 1 != path 1"
    assert st_on["candidates"] == st_off["candidates"] and st_on["chunks"] == st_off["chunks"] and st_on["rows_scanned"] == st_off["rows_scanned"]
    assert 0 < st_off["i8_stage1_tiles"] <= st_on["i8_stage1_tiles"] <= 2 * st_off["i8_stage1_tiles"], (st_on, st_off)
    return st_on, st_off


# 1024: four query tiles, the SYNC build; 300: the last workgroup has waves without queries; 256: one query tile, the build without rendezvous
@pytest.mark.parametrize("nq,k", [(1024, 10), (300, 10), (256, 10), (1024, 64)])
def test_eight_waves_on_every_chunk_change_nothing(shadow_ctx, queries, exact_top64, nq, k):
    assert shadow_ctx.shadow_info()["resident"]
    want = (exact_top64[0][:nq, :k], exact_top64[1][:nq, :k])
    _check_pair(shadow_ctx, queries[:nq], k, want)
    assert shadow_ctx.shadow_info()["last_filter"] == "shadow"


def test_native_int8_corpus(queries):
    c = nvdb_amd.HipContext(0)
    try:
        c.generate_corpus(SEED, N, D, nvdb_amd.DT_I8)
        q = queries[:1024]
        _check_pair(c, q, 10, _exact(c, q, 10))
        assert c.shadow_info()["last_filter"] == "i8"
    finally:
        c.close()


def test_the_default_is_the_eight_wave_build(shadow_ctx, queries):
    c, q = shadow_ctx, queries[:1024]
    c.search_batch(q, 10)
    default = c.stats()
    _, on = _run(c, q, 10, 1)
    _, off = _run(c, q, 10, 0)
    assert default["i8_stage1_tiles"] == on["i8_stage1_tiles"] != off["i8_stage1_tiles"]
