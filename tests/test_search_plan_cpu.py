"""The plan of a flat search (csrc/nvdb_plan.h: route, list capacity, query tiling, bootstrap, chunk boundaries) through the
developer library's nvdb_hip_debug_plan.  Pure integer arithmetic: no GPU.  Invariants over a grid of shapes, and rows
worked out by hand from the planning code as it stood before it became a function (none comes from a GPU run)."""
import itertools

import pytest

import nvdb_amd

SELECT_MAX_CAP = 8192
F16, F32, I8 = nvdb_amd.DT_F16, nvdb_amd.DT_F32, nvdb_amd.DT_I8
I8_DIMS = (256, 384, 768, 896, 1536)
ALL_DIMS = (128, 256, 384, 768, 896, 1536, 2048, 3072)
# name -> (shape fields, fdims the dtype allows)
KINDS = {
    "f16": (dict(dtype=F16), ALL_DIMS),
    "f32+shadow16": (dict(dtype=F32, has_shadow16=1), ALL_DIMS),
    "i8": (dict(dtype=I8), I8_DIMS),
    "f16+q8shadow": (dict(dtype=F16, has_shadow8=1, q8shadow=1), I8_DIMS),
}


def plan(n, d, nq, k, owned=1, options=None, **shape):
    return nvdb_amd.debug_plan(dict(n=n, dim=d, fdim=d, owned=owned, num_cu=256, **shape), nq, k, options or {})


def expected_tile_rows(kind, d, nq):
    """Rows per tile of the build that streams this shape (nvdb_launch_f16.cpp / nvdb_launch_i8.cpp): the int8 two-stage
    kernel has 64-row tiles up to d = 768; the fp16 16x16x32 build (batches > 128, d <= 768) has 64-row tiles up to d = 384."""
    if kind in ("i8", "f16+q8shadow"):
        return 64 if d <= 768 else 32
    return 64 if (d <= 384 and nq > 128) else 32


@pytest.mark.parametrize("kind", list(KINDS))
def test_plan_invariants_over_the_grid(kind):
    shape, dims = KINDS[kind]
    grid = itertools.product(dims, (1, 8, 64, 128, 129, 256, 1024, 2048), (1, 10, 64, 65, 100, 1024, 1025),
                             (2047, 2048, 40000, 40037, 1000000, 2097152, 10000000), (1, 0), ({}, {"path": 1}))
    routes = set()
    for d, nq, k, n, owned, opts in grid:
        p = plan(n, d, nq, k, owned=owned, options=opts, **shape)
        what = (kind, d, nq, k, n, owned, opts, p)
        k_eff = min(k, n)
        routes.add(p["route"])
        assert p["k_eff"] == k_eff, what
        assert p["QT"] * p["QPB"] >= nq > (p["QT"] - 1) * p["QPB"] and p["nq_pad"] == p["QT"] * p["QPB"], what
        assert p["cap"] <= SELECT_MAX_CAP, what
        if k > 1024 or (k_eff > 64 and (opts or n < 2048)):          # (n < 4 * chunk0_rows: the exact path is chosen)
            assert p["route"] == 3, what
        if opts:
            assert p["route"] in (1, 3), what
        if p["route"] != 2:
            assert p["n_chunks"] == 0 and p["stat_rows_scanned"] == n, what
            continue
        t = p["tile_rows"]
        assert t == p["helper_tile_rows"] == expected_tile_rows(kind, d, nq), what
        if k_eff <= 2048:
            assert p["cap"] >= 4 * k_eff, what
        padded = bool(owned or shape.get("has_shadow16") or shape.get("has_shadow8"))
        assert p["padded"] == padded and p["n_al"] % t == 0 and n - p["n_al"] < t, what
        assert p["n_al"] <= n or padded, what
        assert p["tail_exact"] == (p["n_al"] < n), what
        lo, hi = p["chunk_lo"], p["chunk_hi"]
        assert lo[0] == p["r0"] and hi[-1] == p["n_al"] and p["r0"] % t == 0, what
        assert all(a < b and a % t == 0 and b % t == 0 for a, b in zip(lo, hi)), what
        assert all(hi[i] == lo[i + 1] for i in range(len(lo) - 1)), what               # no gap, no overlap
        assert p["stat_chunks"] == len(lo), what
        assert p["stat_rows_scanned"] == (p["n_al"] - p["r0"] + max(0, n - p["n_al"])) * p["QT"], what
        if p["boot"] == 0:
            assert max(64, 8 * k_eff) <= p["boot_tiles"] <= p["cap"] and p["boot_rows"] == 32 * p["boot_tiles"] and p["r0"] == 0, what
        assert not p["perm_on"] or p["boot"] == 0, what
        if p["k_wide"]:
            assert k_eff > 64 and 2 <= p["growth"] <= p["cap"] // (3 * k_eff) and p["boot"] in (0, 2), what
    assert routes == {1, 2, 3}


def _chunks(p):
    return list(zip(p["chunk_lo"], p["chunk_hi"]))


def test_fp16_d768_batch_1024_on_a_million_rows():
    """Auto path: 2.  cap 2048 (batch > 64).  Batch > 128: 64 queries per wave, QPB 256, QT 4.  d > 384: 32-row tiles.  Growth 8.
    Bootstrap max(64, 8k) = 80 tiles = 2560 rows; chunks reach 20480, 163840, 1310720: J = 3, one launch earlier would need
    ceil(1e6 / (64 * 32)) = 489 -> 492 tiles > 256, so 80 stay.  First chunk 2560 * 8 rows, then 7 x the rows before."""
    p = plan(1000000, 768, 1024, 10, dtype=F16)
    assert (p["route"], p["QPB"], p["QT"], p["cap"], p["tile_rows"], p["growth"], p["boot_tiles"], p["boot"], p["perm_on"]) == \
        (2, 256, 4, 2048, 32, 8, 80, 0, 1), p
    assert _chunks(p) == [(0, 20480), (20480, 163840), (163840, 1000000)]
    assert (p["stat_chunks"], p["stat_rows_scanned"], p["prog_words"], p["prep_inits"]) == (3, 4000000, 16 * 256 * 8, 1)


def test_int8_d768_batch_256_below_and_at_the_logged_builds_corpus_size():
    """Below 64 * 32 * 1024 = 2097152 rows: growth 3; chunks from 80 tiles reach 7680 .. 622080, 1866240 (J = 6), one launch earlier
    needs ceil(1e6 / (243 * 32)) = 129 -> 132 tiles <= 256: bootstrap 132 tiles = 4224 rows.  At that size: the build that logs
    first-stage survivors gets growth 6 and a 1024-tile bootstrap."""
    p = plan(1000000, 768, 256, 10, dtype=I8)
    assert (p["route"], p["QPB"], p["QT"], p["cap"], p["tile_rows"], p["growth"], p["boot_tiles"], p["boot"], p["perm_on"]) == \
        (2, 256, 1, 2048, 64, 3, 132, 0, 1), p
    assert _chunks(p) == [(0, 12672), (12672, 38016), (38016, 114048), (114048, 342144), (342144, 1000000)]
    p = plan(2097152, 768, 256, 10, dtype=I8)
    assert (p["route"], p["tile_rows"], p["growth"], p["boot_tiles"], p["boot_rows"], p["boot"]) == (2, 64, 6, 1024, 32768, 0), p
    assert _chunks(p) == [(0, 196608), (196608, 1179648), (1179648, 2097152)]
    # signed row scales keep the second stage in the tile loop: growth 3 at any size
    assert plan(2097152, 768, 256, 10, dtype=I8, i8_scales_signed=1)["growth"] == 3
    assert plan(2097152, 768, 256, 10, dtype=I8, options={"i8_defer": 1})["growth"] == 3


def test_fp16_d256_batch_256_adopted_with_a_ragged_tail():
    """16x16x32 build at d <= 384: 64-row tiles.  Not padded: n_al = 625 * 64 = 40000, rows [40000, 40037) on the exact kernel.
    Chunks from 80 tiles reach 20480, 163840 (J = 2): one launch earlier needs ceil(40037 / (8 * 32)) = 157 -> 160 tiles."""
    p = plan(40037, 256, 256, 10, owned=0, dtype=F16)
    assert (p["route"], p["QPB"], p["QT"], p["tile_rows"], p["padded"], p["n_al"], p["tail_exact"], p["boot_tiles"], p["boot"], p["perm_on"]) == \
        (2, 256, 1, 64, 0, 40000, 1, 160, 0, 1), p
    assert _chunks(p) == [(0, 40000)] and p["stat_rows_scanned"] == 40037
    assert plan(40037, 256, 128, 10, owned=0, dtype=F16)["tile_rows"] == 32          # batches <= 128: the 32x32x16 build
    q = plan(40037, 256, 256, 10, owned=1, dtype=F16)                                # padded: the last tile is streamed whole
    assert (q["n_al"], q["tail_exact"]) == (40064, 0)


def test_fp16_d2048_runs_the_k_split_build_at_64_queries_per_workgroup():
    """No MFMA bootstrap build beyond d = 768: rows [0, 512) (chunk0_rows) on the exact kernel, then 7 x the rows before."""
    p = plan(40000, 2048, 65, 10, dtype=F16)
    assert (p["route"], p["QPB"], p["QT"], p["nq_pad"], p["cap"], p["tile_rows"], p["boot"], p["r0"], p["perm_on"]) == \
        (2, 64, 2, 128, 2048, 32, 1, 512, 0), p
    assert _chunks(p) == [(512, 4096), (4096, 32768), (32768, 40000)] and p["stat_rows_scanned"] == 2 * (40000 - 512)
    assert plan(40000, 1536, 65, 10, dtype=F16)["QPB"] == 128                        # 16-row-tile build: 128 per workgroup


def test_k_100_rides_the_filter_path_with_an_mfma_or_a_seeded_bootstrap():
    """64 < k: the longest lists, 8k = 800 tile maxima.  d = 768: MFMA bootstrap over 25600 rows.  d = 896 has no bootstrap build:
    the any-k machinery seeds the lists from rows [0, 32 * 8 * 100)."""
    p = plan(1000000, 768, 256, 100, dtype=F16)
    assert (p["route"], p["k_wide"], p["cap"], p["growth"], p["boot_tiles"], p["boot"], p["perm_on"]) == (2, 1, 8192, 8, 800, 0, 1), p
    assert _chunks(p) == [(0, 204800), (204800, 1000000)]
    p = plan(1000000, 896, 256, 100, dtype=F16)
    assert (p["route"], p["k_wide"], p["cap"], p["QPB"], p["QT"], p["growth"], p["boot"], p["r0"], p["perm_on"]) == (2, 1, 8192, 128, 2, 8, 2, 25600, 0), p
    assert _chunks(p) == [(25600, 204800), (204800, 1000000)]
    # bootstrap unavailable (more tiles asked for than the corpus has): any-k, reached after the prep launch
    p = plan(60000, 768, 40, 100, dtype=F16, options={"path": 2, "boot_tiles": 4096, "chunk0_rows": 4096})
    assert (p["route"], p["prep"], p["prep_inits"]) == (3, 1, 1), p
    p = plan(60000, 768, 40, 2000, dtype=F16)                                        # k > 1024: any-k at once, no prep launch
    assert (p["route"], p["prep"], p["prep_inits"]) == (3, 0, 0), p


def test_exact_path_prescan_head():
    """Path 1 at 2^20 rows: more than 8 queries scan max(2^15, (n / 64) & ~255) = 32768 rows first; 8 queries (VALU kernel) do not."""
    p = plan(1 << 20, 128, 64, 10, dtype=F16, options={"path": 1})
    assert (p["route"], p["head"], p["cap"], p["QPB"], p["QT"], p["stat_chunks"], p["stat_rows_scanned"], p["prep"]) == \
        (1, 32768, 8192, 128, 1, 2, 1 << 20, 0), p
    p = plan(1 << 20, 128, 8, 10, dtype=F16, options={"path": 1})
    assert (p["route"], p["head"], p["stat_chunks"]) == (1, 0, 1), p


def test_options_and_shapes_are_checked_as_in_a_real_context():
    with pytest.raises(nvdb_amd.NvdbError) as e:
        plan(40000, 768, 8, 10, dtype=F16, options={"path": 7})
    assert e.value.status == 1 and "path must be" in str(e.value)
    with pytest.raises(nvdb_amd.NvdbError) as e:                                     # fp32 without its fp16 shadow, filter path forced
        plan(40000, 768, 8, 10, dtype=F32, options={"path": 2})
    assert e.value.status == 3 and "MFMA filter path needs" in str(e.value)
    # Every chunk at least doubles the rows seen, so 64 chunks hold any corpus -- except the filter path forced onto fewer
    # rows than one tile, where the bootstrap chunk and every chunk after it are empty: reported, not expanded for ever.
    with pytest.raises(nvdb_amd.NvdbError) as e:
        plan(10, 768, 1, 5, dtype=F16, options={"path": 2})
    assert e.value.status == 5 and "chunks" in str(e.value)
