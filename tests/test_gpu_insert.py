"""In-place insertion (nvdb_hip_reserve_rows / nvdb_hip_insert_rows / nvdb_hip_ivf_add_rows): every check is equality, no tolerance.

After an insertion the context must be what a fresh context is that uploaded the resulting rows with the same options, table and
planes (new rows live): rows, scales, planes, corpus_info with the norm bound, shadow_info, and the searches of every route.  The
expected order is built in numpy: old rows tagged with their partition, then the new rows tagged with part_of, stable-sorted by
partition.  Shapes are tests/test_gpu_compact.py's (N, OFFSETS and planes of tests/test_gpu_row_masks.py); the new rows are
synthetic rows of another seed.

"Each inserted row is its own best hit": the queries include inserted rows, and the first hit of every such query must be the
oracle's (score desc, id asc) first hit over the expected rows.  At d >= 100 that IS the inserted row (unit rows, the next best
score is below 0.6); at d = 3 / 5 / 7 a quantised or near-parallel neighbour can legitimately beat a row's self-score (numpy finds
293 such rows among the 9000 int8 d = 5 ones), so there the oracle's first hit is the reference."""
import ctypes as C

import numpy as np
import pytest

import nvdb_amd
from test_gpu_row_masks import N, ROW_BASE, SEED, OFFSETS, NPARTS, PLANES, ALL_LIVE, ALTERNATING, HALF, SPARSE, U64MAX, topk
from test_gpu_compact import LIVE, CORPORA, SLABS, BLOCK, corpus, as_f32, same

pytestmark = pytest.mark.gpu

F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8
NEW_SEED, NEW_MAX = SEED + 7, 9000
USED = [ALL_LIVE, ALTERNATING, HALF, SPARSE]               # the planes every context of this file carries
MASKS = PLANES[USED]
P257 = 5                                                   # the 257-row partition
MIDDLE = 4                                                 # the 65-row partition
_new = {}


def new_rows_of(dtype, dim, m):
    if (dtype, dim) not in _new:
        _new[(dtype, dim)] = nvdb_amd.synth_corpus(NEW_SEED, 0, NEW_MAX, dim, dtype)
    rows, sc = _new[(dtype, dim)]
    return rows[:m], (sc[:m] if sc is not None else None)


def rows_as_f32(dtype, rows, sc):
    if dtype == F16:
        return rows.view(np.float16).astype(np.float32)
    if dtype == I8:
        return rows.astype(np.float32) * sc[:, None]
    return rows.copy()


def make_pattern(name):
    """-> (m, part_of or None, table)."""
    rs = np.random.RandomState(31337)
    u32 = lambda x: np.asarray(x, dtype=np.uint32)
    return {
        "end_no_table": (1, None, False),
        "empty_partition_0": (1, u32([0]), True),
        "partition_1_shifts_everything": (1, u32([1]), True),
        "one_per_partition": (NPARTS, u32(np.arange(NPARTS)[::-1]), True),
        "m63_middle": (63, u32([MIDDLE] * 63), True),
        "m64_middle": (64, u32([MIDDLE] * 64), True),
        "m65_middle": (65, u32([MIDDLE] * 65), True),
        "m9000_into_257": (9000, u32([P257] * 9000), True),
        "m5000_random": (5000, u32(rs.randint(0, NPARTS, size=5000)), True),
        "all_into_last": (700, None, True),
    }[name]


PATTERNS = ["end_no_table", "empty_partition_0", "partition_1_shifts_everything", "one_per_partition", "m63_middle", "m64_middle", "m65_middle",
            "m9000_into_257", "m5000_random", "all_into_last"]


class Expected:
    """The numpy model of one insertion into (old rows, old offsets, old planes)."""

    def __init__(self, dtype, dim, m, part_of, table, rows=None, scales=None, offsets=OFFSETS, planes=MASKS):
        base, sc = corpus(dtype, dim) if rows is None else (rows, scales)
        n = len(base)
        add, add_sc = new_rows_of(dtype, dim, m)
        off = offsets.astype(np.int64) if table else np.array([0, n], dtype=np.int64)
        nparts = len(off) - 1
        p_old = np.searchsorted(off, np.arange(n), side="right") - 1          # (the last p with off[p] <= r: empty partitions never win)
        p_new = np.full(m, nparts - 1, dtype=np.int64) if part_of is None else part_of.astype(np.int64)
        parts = np.concatenate([p_old, p_new])
        order = np.argsort(parts, kind="stable")
        where = np.empty(n + m, dtype=np.int64)
        where[order] = np.arange(n + m)
        self.m, self.n_new, self.table = m, n + m, table
        self.add, self.add_sc = add, add_sc
        self.order = order
        self.new_rows = where[n:].astype(np.uint64)
        self.rows = np.ascontiguousarray(np.concatenate([base, add])[order])
        self.scales = np.ascontiguousarray(np.concatenate([sc, add_sc])[order]) if sc is not None else None
        self.offsets = np.concatenate([[0], np.cumsum(np.bincount(parts, minlength=nparts))]).astype(np.uint64)
        self.planes = np.concatenate([planes, np.ones((len(planes), m), bool)], axis=1)[:, order]


def make_ctx(dtype, dim, rows=None, scales=None, slab=None, growth=None):
    """A fresh context with the options of tests/test_gpu_compact.py's corpora (q8 filter shadow for fp16 d = 768)."""
    base, sc = corpus(dtype, dim)
    ctx = nvdb_amd.HipContext(0)
    if (dtype, dim) == (F16, 768):
        ctx.set_option("q8_shadow", 1)
    if slab is not None:
        ctx.set_option("compact_slab_rows", slab)
    if growth is not None:
        ctx.set_option("insert_growth_pct", growth)
    ctx.upload_corpus(base if rows is None else rows, dtype, sc if rows is None else scales, ROW_BASE)
    return ctx


def old_ctx(dtype, dim, table, **kw):
    ctx = make_ctx(dtype, dim, **kw)
    if table:
        ctx.set_partitions(OFFSETS)
    ctx.set_row_masks(MASKS)
    return ctx


def fresh_ctx(dtype, dim, exp):
    ctx = make_ctx(dtype, dim, exp.rows, exp.scales)
    if exp.table:
        ctx.set_partitions(exp.offsets)
    ctx.set_row_masks(exp.planes)
    return ctx


def same_state(ctx, fresh, exp, norm=True):
    info, want = ctx.corpus_info(), fresh.corpus_info()
    if not norm:                                            # (after a compaction the norm bound is an upper bound, by the header)
        info.pop("max_row_norm"), want.pop("max_row_norm")
    assert info == want and info["n"] == exp.n_new
    rows, scales = ctx.download_rows(0, exp.n_new)
    assert rows.tobytes() == exp.rows.tobytes()
    if exp.scales is not None:
        assert scales.tobytes() == exp.scales.tobytes()
    got = ctx.get_row_masks()
    assert got.shape == (len(exp.planes), (exp.n_new + 31) // 32) and np.array_equal(got, nvdb_amd.pack_row_masks(exp.planes, exp.n_new))
    a, b = ctx.shadow_info(), fresh.shadow_info()
    assert (a["resident"], a["bytes"]) == (b["resident"], b["bytes"])


def queries_of(dtype, dim, exp):
    """Six synthetic queries and up to three inserted rows (the first, the second, the last) -> (queries, rows of the inserted ones)."""
    pick = sorted(set([0, min(1, exp.m - 1), exp.m - 1]))
    own = rows_as_f32(dtype, exp.add[pick], exp.add_sc[pick] if exp.add_sc is not None else None)
    return np.concatenate([nvdb_amd.synth_rows_f32(SEED + 1, 0, 6, dim), own]), exp.new_rows[pick]


def same_searches(oracle, ctx, fresh, dtype, dim, exp, flat_only=False):
    """ids, score bits and counts of every route on both contexts; the inserted rows among the queries find themselves."""
    queries, own = queries_of(dtype, dim, exp)
    nq = len(queries)
    mo = (np.arange(nq, dtype=np.uint32) % len(MASKS)).astype(np.uint32)
    for path in (1, 2):
        for c in (ctx, fresh):
            c.set_option("path", path)
        for k in (10, 100):
            got = ctx.search_batch(queries, k)
            same(got, fresh.search_batch(queries, k))
            assert ctx.stats()["path"] == fresh.stats()["path"]
            if path == 2 and k == 10:
                assert ctx.stats()["path"] == 2             # the filter route ran: it streamed the moved rows or their moved shadow
        ids10, s10 = ctx.search_batch(queries, 10)
        for j, row in enumerate(own):
            q = nq - len(own) + j
            sc = oracle.scores(exp.rows, dtype, queries[q], exp.scales)
            eid, _, _ = topk(sc, np.arange(exp.n_new), 1)
            assert ids10[q, 0] == eid[0], (path, q)
            if dim >= 100:
                assert ids10[q, 0] == ROW_BASE + row, (path, q)   # each inserted row is its own best hit
        same(ctx.range_search(queries, s10[:, 9]), fresh.range_search(queries, s10[:, 9]))
        assert ctx.stats()["path"] == fresh.stats()["path"]
        same(ctx.search_masked(queries, 10, mo), fresh.search_masked(queries, 10, mo))           # both routes of the masked flat top-k
    for c in (ctx, fresh):
        c.set_option("path", 0)
    if flat_only or not exp.table:
        return
    nparts = len(exp.offsets) - 1
    all_parts = np.tile(np.arange(nparts, dtype=np.uint32), (nq, 1))
    one_part = (np.arange(nq, dtype=np.uint32) % nparts)[:, None].copy()
    for probe in (one_part, all_parts):
        got = ctx.search_partitions(queries, 10, probe)
        same(got, fresh.search_partitions(queries, 10, probe))
        same(ctx.search_partitions_anyk(queries, 100, probe), fresh.search_partitions_anyk(queries, 100, probe))
        same(ctx.range_search_partitions(queries, s10[:, 9], probe), fresh.range_search_partitions(queries, s10[:, 9], probe))
        same(ctx.search_partitions_masked(queries, 10, probe, mo), fresh.search_partitions_masked(queries, 10, probe, mo))
    ids, _, _ = ctx.search_partitions(queries, 10, all_parts)
    for j, row in enumerate(own):
        if dim >= 100:
            assert ids[nq - len(own) + j, 0] == ROW_BASE + row


def close_all(*ctxs):
    for c in ctxs:
        if c is not None:
            c.close()


# ---- 1. equals a fresh upload: every corpus, every pattern, every slab size (in place: the slab walk and the bounce buffer run) ----
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype,dim", CORPORA)
def test_equals_a_fresh_upload(oracle, dtype, dim, pattern):
    m, part_of, table = make_pattern(pattern)
    exp = Expected(dtype, dim, m, part_of, table)
    add, add_sc = new_rows_of(dtype, dim, m)
    fresh = fresh_ctx(dtype, dim, exp)
    ctx = None
    try:
        for slab in SLABS:
            ctx = old_ctx(dtype, dim, table, slab=slab)
            ctx.reserve_rows(N + m)
            n_new, new_rows = ctx.insert_rows(add, add_sc, part_of)
            assert n_new == N + m and np.array_equal(new_rows, exp.new_rows), (slab, pattern)
            same_state(ctx, fresh, exp)
            same_searches(oracle, ctx, fresh, dtype, dim, exp)
            ctx.close()
            ctx = None
    finally:
        close_all(ctx, fresh)


# ---- 2. both capacity routes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dim", CORPORA)
def test_growth_and_reserved_routes(oracle, dtype, dim):
    m, part_of, table = make_pattern("m5000_random")
    exp = Expected(dtype, dim, m, part_of, table)
    add, add_sc = new_rows_of(dtype, dim, m)
    fresh = fresh_ctx(dtype, dim, exp)
    grown = old_ctx(dtype, dim, table, growth=0)            # (a) exact growth: every array reallocated to n + m rows
    default = old_ctx(dtype, dim, table)                    #     the default growth (50 %), then a second insertion into the room it left
    reserved = old_ctx(dtype, dim, table)                   # (b) in place
    try:
        queries, _ = queries_of(dtype, dim, exp)
        before = [reserved.search_batch(queries, 10), reserved.search_partitions(queries, 10, np.zeros((len(queries), 1), dtype=np.uint32) + 6)]
        reserved.reserve_rows(N + m)
        reserved.reserve_rows(10)                           # never shrinks
        same(reserved.search_batch(queries, 10), before[0])                                  # reserve_rows alone changes no result
        same(reserved.search_partitions(queries, 10, np.zeros((len(queries), 1), dtype=np.uint32) + 6), before[1])
        rows, scales = reserved.download_rows(0, N)
        assert rows.tobytes() == corpus(dtype, dim)[0].tobytes() and reserved.corpus_info()["n"] == N
        for ctx in (grown, reserved):
            n_new, new_rows = ctx.insert_rows(add, add_sc, part_of)
            assert n_new == N + m and np.array_equal(new_rows, exp.new_rows)
            same_state(ctx, fresh, exp)
            same_searches(oracle, ctx, fresh, dtype, dim, exp)
        half = m // 2                                       # two insertions compose: the second fits the capacity the first one grew to
        e1 = Expected(dtype, dim, half, part_of[:half], table)
        n1, r1 = default.insert_rows(add[:half], add_sc[:half] if add_sc is not None else None, part_of[:half])
        assert n1 == N + half and np.array_equal(r1, e1.new_rows)
        n2, r2 = default.insert_rows(add[half:], add_sc[half:] if add_sc is not None else None, part_of[half:])
        assert n2 == N + m
        same_state(default, fresh, exp)
        same_searches(oracle, default, fresh, dtype, dim, exp, flat_only=True)
    finally:
        close_all(fresh, grown, default, reserved)


@pytest.mark.parametrize("dtype,dim", CORPORA)
def test_insert_after_compaction_zeroes_behind_the_new_end(oracle, dtype, dim):
    """(c) compact `dead_block` (the 9000 rows at the end), insert 10 rows: the rows behind the new end are stale rows of the old
    corpus unless the call zeroes them; the filter routes must equal a fresh upload."""
    live = LIVE["dead_block"]
    base, sc = corpus(dtype, dim)
    kept, kept_sc = np.ascontiguousarray(base[live]), (np.ascontiguousarray(sc[live]) if sc is not None else None)
    new_off = np.concatenate([[0], np.cumsum(live)])[OFFSETS.astype(np.int64)].astype(np.uint64)
    exp = Expected(dtype, dim, 10, None, True, rows=kept, scales=kept_sc, offsets=new_off, planes=np.ones((1, len(kept)), bool))
    add, add_sc = new_rows_of(dtype, dim, 10)
    ctx = make_ctx(dtype, dim)
    fresh = make_ctx(dtype, dim, exp.rows, exp.scales)
    try:
        ctx.set_partitions(OFFSETS)
        ctx.set_row_masks(live[None])
        n_c, _ = ctx.compact_rows(0)
        assert n_c == N - BLOCK
        n_new, new_rows = ctx.insert_rows(add, add_sc)      # no part_of: behind the last row, into the last partition
        assert n_new == n_c + 10 and np.array_equal(new_rows, np.arange(n_c, n_c + 10, dtype=np.uint64))
        fresh.set_partitions(exp.offsets)
        fresh.set_row_masks(exp.planes)
        same_state(ctx, fresh, exp, norm=False)
        queries, own = queries_of(dtype, dim, exp)
        for path in (2, 1):
            ctx.set_option("path", path)
            fresh.set_option("path", path)
            for k in (10, 100):
                same(ctx.search_batch(queries, k), fresh.search_batch(queries, k))
            assert ctx.stats()["path"] == fresh.stats()["path"]
            ids10, s10 = ctx.search_batch(queries, 10)
            same(ctx.range_search(queries, s10[:, 9]), fresh.range_search(queries, s10[:, 9]))
            same(ctx.search_masked(queries, 10), fresh.search_masked(queries, 10))
        last = np.full((len(queries), 1), NPARTS - 1, dtype=np.uint32)
        same(ctx.search_partitions(queries, 10, last), fresh.search_partitions(queries, 10, last))
    finally:
        close_all(ctx, fresh)


# ---- 3. round trip -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dim", [(F16, 768), (I8, 768), (I8, 5), (F32, 3)])
def test_insert_tombstone_compact_is_the_identity(dtype, dim):
    m, part_of, table = make_pattern("m5000_random")
    add, add_sc = new_rows_of(dtype, dim, m)
    base, sc = corpus(dtype, dim)
    queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, 7, dim)
    all_parts = np.tile(np.arange(NPARTS, dtype=np.uint32), (7, 1))
    mo = (np.arange(7, dtype=np.uint32) % len(MASKS)).astype(np.uint32)

    def searches(ctx):
        out = []
        for path in (1, 2):
            ctx.set_option("path", path)
            out += [ctx.search_batch(queries, 10), ctx.search_masked(queries, 10, mo)]
        ctx.set_option("path", 0)
        return out + [ctx.search_partitions(queries, 10, all_parts), ctx.search_partitions_masked(queries, 10, all_parts, mo)]
    ctx = old_ctx(dtype, dim, table)
    try:
        before = searches(ctx)
        n_new, new_rows = ctx.insert_rows(add, add_sc, part_of)
        ctx.update_row_mask(0, new_rows, False)             # plane 0 was all live: now exactly the new rows are dead
        n_back, old = ctx.compact_rows(0)
        assert n_back == N and np.array_equal(old, np.setdiff1d(np.arange(n_new, dtype=np.uint32), new_rows.astype(np.uint32)))
        rows, scales = ctx.download_rows(0, N)
        assert rows.tobytes() == base.tobytes() and (sc is None or scales.tobytes() == sc.tobytes())
        assert np.array_equal(ctx.get_row_masks(), nvdb_amd.pack_row_masks(MASKS, N))
        info = ctx.corpus_info()
        assert info["n"] == N and info["row_base"] == ROW_BASE
        for a, b in zip(searches(ctx), before):             # (the partition searches pin the table)
            same(a, b)
    finally:
        ctx.close()


# ---- 4. a new row that forbids the resident shadow -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dim,value", [(F16, 768, np.inf), (F32, 768, 70000.0)])
def test_shadow_drop(dtype, dim, value):
    base, _ = corpus(dtype, dim)
    add = nvdb_amd.synth_corpus(NEW_SEED, 0, 1, dim, dtype)[0].copy()
    if dtype == F16:
        add[0, 5] = np.float16(value).view(np.uint16)
    else:
        add[0, 5] = value
    rows = np.concatenate([base, add])
    ctx = make_ctx(dtype, dim)
    fresh = make_ctx(dtype, dim, rows, None)
    try:
        if dtype == F16:
            assert ctx.shadow_info()["resident"]
        n_new, new_rows = ctx.insert_rows(add)
        assert n_new == N + 1 and new_rows[0] == N
        assert ctx.corpus_info() == fresh.corpus_info()
        a, b = ctx.shadow_info(), fresh.shadow_info()
        assert (a["resident"], a["bytes"]) == (b["resident"], b["bytes"]) and not a["resident"]
        got, _ = ctx.download_rows(0, N + 1)
        assert got.tobytes() == rows.tobytes()
        queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, 5, dim)
        for path in ((1,) if dtype == F16 else (1, 0)):      # (the exact scan; fp32: and the automatic route, the scan again without a shadow)
            ctx.set_option("path", path)
            fresh.set_option("path", path)
            same(ctx.search_batch(queries, 10), fresh.search_batch(queries, 10))
            assert ctx.stats()["path"] == fresh.stats()["path"]
        if dtype == F32:                                    # the fp16 shadow is gone on both: no filter route for an fp32 corpus
            for c in (ctx, fresh):
                c.set_option("path", 2)
                with pytest.raises(nvdb_amd.NvdbError) as e:
                    c.search_batch(queries, 10)
                assert e.value.status == 3
    finally:
        close_all(ctx, fresh)


# ---- 5. the index ------------------------------------------------------------------------------------------------------------------
NLISTS, NPROBE = 37, 5
_centroids = {}


def centroids(dtype, dim):
    if (dtype, dim) not in _centroids:
        src = make_ctx(dtype, dim)
        try:
            cen = src.train_centroids(NLISTS, 2, 7)
            _centroids[(dtype, dim)] = (cen, src.assign_rows(cen))
        finally:
            src.close()
    return _centroids[(dtype, dim)]


def ivf_searches(ivf, queries, mo):
    top = ivf.search(queries, 10, NPROBE, want_probe=True)
    return [top, ivf.search_anyk(queries, 100, NPROBE, masked=False, want_probe=True),
            ivf.range_search(queries, top[1][:, 9].copy(), NPROBE, masked=False, want_probe=True),
            ivf.search_masked(queries, 10, NPROBE, mo, want_probe=True)]


@pytest.mark.parametrize("m", [1, 65, 5000])
@pytest.mark.parametrize("dtype,dim", [(F16, 768), (I8, 768), (F32, 768), (F16, 100)])
def test_ivf_add_rows_equals_a_full_build(dtype, dim, m):
    base, sc = corpus(dtype, dim)
    cen, assign_all = centroids(dtype, dim)
    head = make_ctx(dtype, dim, base[:N - m], sc[:N - m] if sc is not None else None)
    full = make_ctx(dtype, dim)
    ivf = want = None
    try:
        ivf = nvdb_amd.IvfIndex(head, cen)
        want = nvdb_amd.IvfIndex(full, cen)
        first, assign = ivf.add_rows(base[N - m:], sc[N - m:] if sc is not None else None)
        assert first == N - m and np.array_equal(assign, assign_all[N - m:])
        assert np.array_equal(assign, full.assign_rows(cen, N - m, m))
        a, b = ivf.info(), want.info()
        assert a["n"] == b["n"] == N and np.array_equal(a["offsets"], b["offsets"]) and np.array_equal(a["perm"], b["perm"])
        same(ivf.ctx.download_rows(0, N)[:1 if sc is None else 2], want.ctx.download_rows(0, N)[:1 if sc is None else 2])
        assert ivf.ctx.corpus_info() == want.ctx.corpus_info()
        queries = np.concatenate([nvdb_amd.synth_rows_f32(SEED + 1, 0, 6, dim), as_f32(dtype, dim, np.array([N - m, N - 1]))])
        mo = (np.arange(len(queries), dtype=np.uint32) % len(MASKS)).astype(np.uint32)
        ivf.set_row_masks(MASKS)                            # by ORIGINAL row, now N of them
        want.set_row_masks(MASKS)
        for x, y in zip(ivf_searches(ivf, queries, mo), ivf_searches(want, queries, mo)):
            same(x, y)
        ids, _, _ = ivf.search(queries, 10, NLISTS)
        assert ids[-2, 0] == ROW_BASE + N - m and ids[-1, 0] == ROW_BASE + N - 1             # the added rows find themselves
    finally:
        for x in (ivf, want):
            if x is not None:
                x.close()
        close_all(head, full)


def test_ivf_compact_then_add_rows(oracle):
    """ivf_compact on a random-half plane, then add_rows: ids stay ORIGINAL ids, the new ones start at the old src_n, and the searches
    equal the oracle over the surviving plus the new rows, ties by (list, original id)."""
    dtype, dim, m = F16, 768, 700
    base, _ = corpus(dtype, dim)
    cen, assign_all = centroids(dtype, dim)
    head = make_ctx(dtype, dim, base[:N - m], None)
    ivf = None
    try:
        ivf = nvdb_amd.IvfIndex(head, cen)
        live = np.ones(N, bool)
        live[:N - m] = np.random.RandomState(8).rand(N - m) < 0.5
        ivf.set_row_masks(live[None, :N - m])
        n_c = ivf.compact(0)
        assert n_c == int(live[:N - m].sum())
        ivf.update_row_mask(0, np.flatnonzero(live)[:1].astype(np.uint64), True)             # (a no-op that builds the inverse: add_rows must extend it)
        first, assign = ivf.add_rows(base[N - m:])
        assert first == N - m and np.array_equal(assign, assign_all[N - m:])
        info = ivf.info()
        rows_live = np.flatnonzero(live)
        order = rows_live[np.argsort(assign_all[rows_live], kind="stable")]
        assert info["n"] == n_c + m and np.array_equal(info["perm"], order.astype(np.uint32))
        assert np.array_equal(info["offsets"], np.concatenate([[0], np.cumsum(np.bincount(assign_all[rows_live], minlength=NLISTS))]).astype(np.uint64))
        got, _ = ivf.ctx.download_rows(0, n_c + m)
        assert got.tobytes() == base[order].tobytes()
        queries = np.concatenate([nvdb_amd.synth_rows_f32(SEED + 1, 0, 6, dim), as_f32(dtype, dim, np.array([N - m, N - 1]))])
        nq = len(queries)
        ids, sc, cnt, probe = ivf.search(queries, 10, NPROBE, want_probe=True)
        aid, asc, acnt, aprobe = ivf.search_anyk(queries, 100, NPROBE, masked=False, want_probe=True)
        lims, rid, rsc, rprobe = ivf.range_search(queries, sc[:, 9].copy(), NPROBE, masked=False, want_probe=True)
        assert np.array_equal(probe, aprobe) and np.array_equal(probe, rprobe)
        tie = assign_all.astype(np.int64)
        for q in range(nq):
            s = oracle.scores(base, dtype, queries[q])
            cand = np.flatnonzero(live & np.isin(assign_all, probe[q]))
            for k, (gi, gs, gc) in ((10, (ids[q], sc[q], cnt[q])), (100, (aid[q], asc[q], acnt[q]))):
                eid, esc, ecnt = topk(s, cand, k, tie=tie)
                assert gc == ecnt and np.array_equal(gi, eid) and np.array_equal(gs.view(np.uint32), esc.view(np.uint32)), (q, k)
            rc = cand[s[cand] >= sc[q, 9]]
            eid, esc, ecnt = topk(s, rc, len(rc), tie=tie)
            a, b = int(lims[q]), int(lims[q + 1])
            assert b - a == ecnt and np.array_equal(rid[a:b], eid) and np.array_equal(rsc[a:b].view(np.uint32), esc.view(np.uint32)), q
        assert ids[-2, 0] == ROW_BASE + N - m and ids[-1, 0] == ROW_BASE + N - 1
        # the planes speak of ORIGINAL rows, N of them now; the new rows came in live, and an update reaches them
        assert nvdb_amd.unpack_row_masks(ivf.ctx.get_row_masks(), n_c + m).all()
        ivf.update_row_mask(0, np.array([N - 1, 3], dtype=np.uint64), False)
        mids, _, _ = ivf.search_masked(queries, 10, NLISTS, np.zeros(nq, dtype=np.uint32))
        assert ROW_BASE + N - 1 not in mids and mids[-2, 0] == ROW_BASE + N - m
    finally:
        if ivf is not None:
            ivf.close()
        head.close()


# ---- 6. statuses -----------------------------------------------------------------------------------------------------------------
def test_statuses():
    import torch
    dtype, dim = F16, 100
    base, _ = corpus(dtype, dim)
    add, _ = new_rows_of(dtype, dim, 4)
    lib = nvdb_amd.load_library()
    out_n = C.c_uint64(7)
    new_rows = np.full(4, 7, dtype=np.uint64)

    def call(ctx, rows, m, part_of):
        return lib.nvdb_hip_insert_rows(ctx.h, rows.ctypes.data if rows is not None else None, None, m, part_of.ctypes.data if part_of is not None else None,
                                        new_rows.ctypes.data, C.byref(out_n))

    def untouched():
        return out_n.value == 7 and (new_rows == 7).all()
    ctx = make_ctx(dtype, dim)
    i8 = make_ctx(I8, 5)
    empty = nvdb_amd.HipContext(0)
    adopted = nvdb_amd.HipContext(0)
    try:
        q = nvdb_amd.synth_rows_f32(SEED + 1, 0, 4, dim)
        ref = ctx.search_batch(q, 10)
        zero = np.zeros(4, dtype=np.uint32)
        assert call(empty, add, 4, None) == 4 and untouched()                                # NVDB_ERR_NO_CORPUS
        assert lib.nvdb_hip_reserve_rows(empty.h, 10) == 4
        assert call(ctx, None, 4, None) == 1 and untouched()                                 # null rows
        assert call(i8, new_rows_of(I8, 5, 4)[0], 4, None) == 1 and untouched()              # int8 without scales
        assert call(ctx, add, 4, zero) == 1 and untouched()                                  # part_of without a table
        same(ctx.search_batch(q, 10), ref)
        ctx.set_partitions(OFFSETS)
        ctx.set_row_masks(MASKS)
        pref = ctx.search_partitions(q, 10, np.tile(np.arange(NPARTS, dtype=np.uint32), (4, 1)))
        assert call(ctx, add, 4, np.array([0, 1, NPARTS, 2], dtype=np.uint32)) == 1 and untouched()   # an entry >= nparts
        assert lib.nvdb_hip_set_option(ctx.h, b"insert_growth_pct", -1) == 1 and lib.nvdb_hip_set_option(ctx.h, b"insert_growth_pct", 401) == 1
        assert lib.nvdb_hip_set_option(ctx.h, b"insert_growth_pct", 400) == 0 and lib.nvdb_hip_set_option(ctx.h, b"insert_growth_pct", 0) == 0
        assert ctx.corpus_info()["n"] == N and np.array_equal(ctx.get_row_masks(), nvdb_amd.pack_row_masks(MASKS, N))
        same(ctx.search_batch(q, 10), ref)
        same(ctx.search_partitions(q, 10, np.tile(np.arange(NPARTS, dtype=np.uint32), (4, 1))), pref)
        assert call(ctx, add, 0, zero) == 0 and out_n.value == N and (new_rows == 7).all()   # m == 0: NVDB_OK, *out_n = n
        assert call(ctx, None, 0, None) == 0 and out_n.value == N
        assert ctx.corpus_info()["n"] == N
        same(ctx.search_batch(q, 10), ref)
        same(ctx.search_partitions(q, 10, np.tile(np.arange(NPARTS, dtype=np.uint32), (4, 1))), pref)
        out_n.value = 7
        t = torch.from_numpy(base.view(np.int16)).cuda()
        adopted.adopt_corpus(t.data_ptr(), N, dim, dtype, None, ROW_BASE)
        aref = adopted.search_batch(q, 10)
        assert call(adopted, add, 4, None) == 3 and untouched()                              # NVDB_ERR_UNSUPPORTED
        assert lib.nvdb_hip_reserve_rows(adopted.h, N + 10) == 3
        assert adopted.corpus_info()["n"] == N and np.array_equal(t.cpu().numpy().view(np.uint16), base)
        same(adopted.search_batch(q, 10), aref)
    finally:
        close_all(ctx, i8, empty, adopted)
