"""Range search on the probe path (nvdb_hip_range_search_partitions / _ivf / _masked, nvdb_hip_ivf_range_search) against the oracle.

Expected slice of a query = the oracle's score vector restricted to the rows that are in a probed partition AND live in the query's
mask, keeping score >= radius (the C comparison: NaN on either side is false), ordered by np.lexsort((rows, -s)).  lims, ids and
score BITS must be equal: no tolerance, no excluded case.  Radii are taken from each query's own oracle scores, so the boundary row
and every tie with it are hit exactly.  The corpus shape is tests/test_gpu_partitions.py's, the planes tests/test_gpu_row_masks.py's."""
import numpy as np
import pytest

import nvdb_amd
import pyoracle as po

pytestmark = pytest.mark.gpu

N, ROW_BASE, SEED = 30000, 1_000_003, 20250117
# an empty partition, a single row, around a wave (63 / 64 / 65), around a workgroup (257), one far larger than a segment, the rest
SIZES = [0, 1, 63, 64, 65, 257, 20000]
OFFSETS = np.concatenate([[0], np.cumsum(SIZES + [N - sum(SIZES)])]).astype(np.uint64)
NPARTS = len(OFFSETS) - 1
EMPTY, BIG = 0, 6
SENT = 0xFFFFFFFF
NQ_MAX = 70
INF = np.float32(np.inf)
F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8


def make_planes(n):
    rs = np.random.RandomState(77)
    planes = [np.ones(n, bool), np.zeros(n, bool)]                      # 0 all live, 1 none
    for r in (0, 31, 32, 63, 64, n - 1):                                # 2 .. 7: exactly one live row at a word / tile / corpus edge
        p = np.zeros(n, bool)
        p[r] = True
        planes.append(p)
    planes.append(rs.rand(n) < 0.5)                                     # 8 random 50 %
    return np.stack(planes)


PLANES = make_planes(N)
NMASKS = len(PLANES)
ALL_LIVE, NONE_LIVE, HALF = 0, 1, 8
TOMBSTONES = np.array([0, 31, 32, 32, 63, 64, N - 1], dtype=np.uint64)   # a duplicate, and two rows of one word, in one call


def slices(score_of, rows_of, radius, nq, row_base=0, tie_of=None):
    """score_of(q) -> [n] scores, rows_of(q) -> candidate local rows (ascending) -> (lims, ids, scores)."""
    lims = np.zeros(nq + 1, dtype=np.uint64)
    ids, scores = [np.zeros(0, np.uint64)], [np.zeros(0, np.float32)]
    for q in range(nq):
        rows = rows_of(q)
        s = score_of(q)[rows]
        with np.errstate(invalid="ignore"):
            keep = s >= radius[q]
        rows, s = rows[keep], s[keep]
        order = np.lexsort((rows, -s) if tie_of is None else (rows, tie_of[rows], -s))
        ids.append(rows[order].astype(np.uint64) + np.uint64(row_base))
        scores.append(s[order])
        lims[q + 1] = lims[q] + np.uint64(len(rows))
    return lims, np.concatenate(ids), np.concatenate(scores)


def assert_same(got, want, what=""):
    (gl, gi, gs), (wl, wi, ws) = got[:3], want
    assert np.array_equal(gl, wl), (what, "lims", np.nonzero(np.diff(gl.astype(np.int64)) != np.diff(wl.astype(np.int64)))[0][:8])
    assert np.array_equal(gi, wi), (what, "ids")
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (what, "score bits")


def kth_best(s, k):
    """The k-th best (1-based) non-NaN score of s; fewer than k: the worst; none: 0."""
    s = s[~np.isnan(s)]
    return np.float32(np.sort(s)[::-1][min(k, len(s)) - 1]) if len(s) else np.float32(0.0)


class Case:
    """One resident corpus (dtype, dim) with the partition table, the planes, queries and lazily computed oracle scores."""

    def __init__(self, orc, dtype, dim, base=None, scales=None, queries=None):
        self.orc, self.dtype, self.dim = orc, dtype, dim
        if base is None:
            base, scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
        self.base, self.scales = base, scales
        self.queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ_MAX, dim) if queries is None else queries
        self.ctx = nvdb_amd.HipContext(0)
        self.ctx.upload_corpus(self.base, dtype, self.scales, ROW_BASE)
        self.ctx.set_partitions(OFFSETS)
        self.ctx.set_row_masks(PLANES)
        self._scores = {}

    def scores(self, q):
        if q not in self._scores:
            self._scores[q] = self.orc.scores(self.base, self.dtype, self.queries[q], self.scales)
        return self._scores[q]

    def union(self, probe_row, live=None):
        rows = np.concatenate([np.arange(OFFSETS[p], OFFSETS[p + 1], dtype=np.int64) for p in sorted(set(int(p) for p in probe_row if p != SENT))] +
                              [np.empty(0, np.int64)])
        return rows if live is None else rows[live[rows]]

    def mixed_radii(self, probe):
        """Per query, in turn: its own 1st, 10th, 65th, 300th best score of the probed union, a value above its best, -inf."""
        out = np.empty(len(probe), dtype=np.float32)
        for q in range(len(probe)):
            s = self.scores(q)[self.union(probe[q])]
            kind = q % 6
            out[q] = -INF if kind == 5 else np.nextafter(kth_best(s, 1), INF) if kind == 4 else kth_best(s, (1, 10, 65, 300)[kind])
        return out

    def check(self, probe, radius, mask_of=None, masked=None, planes=PLANES, what=""):
        probe = np.asarray(probe, dtype=np.uint32)
        nq = probe.shape[0]
        radius = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))
        got = self.ctx.range_search_partitions(self.queries[:nq], radius, probe, mask_of, masked)
        is_masked = (mask_of is not None) if masked is None else masked

        def rows_of(q):
            m = SENT if not is_masked else 0 if mask_of is None else int(mask_of[q])
            return self.union(probe[q], None if m == SENT else planes[m])
        want = slices(self.scores, rows_of, radius, nq, ROW_BASE)
        assert_same(got, want, what)
        st = self.ctx.stats()
        assert st["path"] == 7 and st["candidates"] == int(want[0][-1]), st
        return got


@pytest.fixture(scope="module")
def cases(oracle):
    made = {}

    def get(dtype, dim):
        if (dtype, dim) not in made:
            made[(dtype, dim)] = Case(oracle, dtype, dim)
        return made[(dtype, dim)]
    yield get
    for c in made.values():
        c.ctx.close()


def cycle(nq, shift=0):
    """Every plane and the "no mask" number in turn."""
    m = (np.arange(nq) + shift) % (NMASKS + 1)
    return np.where(m == NMASKS, SENT, m).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ every build of the scan
# staged QW <= 2 (f16 768), staged QW = 4 (f16 384), staged (i8 768, f32 384), direct aligned (f32 768: a tile does not fit the
# LDS), direct unaligned (i8 100, f32 7, f16 1)
BUILDS = [(F16, 768), (F16, 384), (I8, 768), (F32, 384), (F32, 768), (I8, 100), (F32, 7), (F16, 1)]


@pytest.mark.parametrize("dtype,dim", BUILDS)
def test_builds(cases, dtype, dim):
    c = cases(dtype, dim)
    nq, nprobe = 9, 3
    rs = np.random.RandomState(1000 * dtype + dim)
    probe = rs.randint(0, NPARTS, size=(nq, nprobe)).astype(np.uint32)
    probe[5] = [BIG, 7, 5]                                              # (the -inf query takes a large union)
    radius = c.mixed_radii(probe)
    plain = c.check(probe, radius, what="unmasked")
    c.check(probe, radius, cycle(nq), what="every plane")
    c.check(probe, radius, np.array([HALF, SENT, HALF, ALL_LIVE, HALF, HALF, NONE_LIVE, HALF, SENT], dtype=np.uint32), what="50 % plane")
    # an all-live plane equals the unmasked call bit for bit (mask_of NULL: plane 0)
    live = c.check(probe, radius, None, masked=True, what="plane 0")
    for a, b in zip(plain, live):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ one walk, two sinks
# 12 uneven partitions over 6000 rows: an empty one, a single row, around a wave, one longer than a segment (PART_SEG_ROWS = 2048:
# two items, a ragged last tile), the rest
WALK_N, WALK_K = 6000, 10
WALK_SIZES = [0, 1, 63, 64, 65, 257, 2500, 300, 700, 900, 500]
WALK_OFFSETS = np.concatenate([[0], np.cumsum(WALK_SIZES + [WALK_N - sum(WALK_SIZES)])]).astype(np.uint64)
WALK_ONE, WALK_BIG = 1, 6


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype,dim", [(F16, 768), (I8, 100), (F32, 384)])       # staged; direct unaligned; QW = 4
def test_topk_and_range_walk_the_same_rows(dtype, dim, masked):
    """The top-k scan and the range scan are one tile walk with two sinks: with radius[q] = query q's k-th returned score, every
    top-k entry is in the range slice with the same score bits, and every range entry strictly above the radius is in the top-k.
    A query with fewer than k live rows takes radius -inf and gets exactly its top-k entries.  All 70 queries probe the one-row
    partition (groups of 32, 32 and 6), 68 of them the 2500-row one."""
    nq, nprobe, k = NQ_MAX, 4, WALK_K
    assert len(WALK_OFFSETS) == 13 and WALK_SIZES[WALK_BIG] > 2048
    base, scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, WALK_N, dim, dtype)
    queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, nq, dim)
    rs = np.random.RandomState(31 * dtype + dim)
    probe = rs.randint(0, len(WALK_SIZES) + 1, size=(nq, nprobe)).astype(np.uint32)
    probe[:, 0] = WALK_ONE
    probe[:, 1] = WALK_BIG
    probe[:2] = [WALK_ONE, EMPTY, SENT, SENT]                           # one row in all: fewer than k
    mask_of = cycle(nq) if masked else None                              # planes of make_planes: all, none, single rows, 50 %, "no mask"
    ctx = nvdb_amd.HipContext(0)
    try:
        ctx.upload_corpus(base, dtype, scales, ROW_BASE)
        ctx.set_partitions(WALK_OFFSETS)
        if masked:
            ctx.set_row_masks(make_planes(WALK_N))
            ids, sc, cnt = ctx.search_partitions_masked(queries, k, probe, mask_of)
        else:
            ids, sc, cnt = ctx.search_partitions(queries, k, probe)
        assert cnt[0] == 1 and cnt.max() == k and (cnt < k).any()
        radius = np.where(cnt < k, -INF, sc[:, k - 1]).astype(np.float32)
        lims, rids, rsc = ctx.range_search_partitions(queries, radius, probe, mask_of)
    finally:
        ctx.close()
    for q in range(nq):
        lo, hi, m = int(lims[q]), int(lims[q + 1]), int(cnt[q])
        in_range = dict(zip(rids[lo:hi].tolist(), rsc[lo:hi].view(np.uint32).tolist()))
        assert len(in_range) == hi - lo, (q, "a row twice")
        top = dict(zip(ids[q, :m].tolist(), sc[q, :m].view(np.uint32).tolist()))
        for i, bits in top.items():
            assert in_range.get(i) == bits, (q, i, "top-k entry missing from the range slice, or other score bits")
        above = rids[lo:hi][rsc[lo:hi] > radius[q]].tolist()
        assert all(i in top for i in above), (q, "a range entry above the radius that the top-k does not hold")
        if m < k:
            assert in_range == top, (q, "fewer than k live rows")


# ------------------------------------------------------------------------------------------------ grouping, sizes, budgets
@pytest.mark.parametrize("dtype,dim", [(F16, 768), (I8, 100)])
def test_grouping_and_sizes(cases, dtype, dim):
    c = cases(dtype, dim)
    big = np.full((NQ_MAX, 1), BIG, dtype=np.uint32)
    # all 70 queries probe the 20 000-row partition with radius -inf: several groups and segments, 20 000 results per query --
    # slabs above 8192 keys take the global sort steps
    all_rows = c.check(big, -INF, what="70 x 20000")
    assert np.all(np.diff(all_rows[0].astype(np.int64)) == 20000)
    # the LDS / global sort boundary: 8192 and 8193 results
    r = np.array([kth_best(c.scores(q)[c.union([BIG])], 8192 + (q & 1)) for q in range(8)], dtype=np.float32)
    got = c.check(big[:8], r, what="8192 / 8193")
    assert np.diff(got[0].astype(np.int64)).tolist() == [8192, 8193] * 4
    # every query a different partition
    each = np.arange(NPARTS, dtype=np.uint32)[:, None]
    c.check(each, -INF, what="one partition each")
    c.check(each, c.mixed_radii(each), cycle(NPARTS, 3), what="one partition each, masked")
    # a 1 MB block budget: sub-batches of a few queries, the same bytes
    try:
        c.ctx.set_option("largek_budget_mb", 1)
        cut = c.check(big, -INF, what="largek_budget_mb = 1")
        for a, b in zip(all_rows, cut):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert c.ctx.stats()["chunks"] > 10
        c.check(each, c.mixed_radii(each), what="largek_budget_mb = 1, one partition each")
    finally:
        c.ctx.set_option("largek_budget_mb", 8192)
    # a 1 MB result budget: complete lims, nothing held
    try:
        c.ctx.set_option("range_max_mb", 1)
        with pytest.raises(nvdb_amd.NvdbError) as e:
            c.ctx.range_search_partitions(c.queries, -INF, big)
        assert e.value.status == 3 and "range_max_mb" in str(e.value) and str(NQ_MAX * 20000) in str(e.value)
        assert np.array_equal(e.value.lims, all_rows[0])
        ids, sc = np.zeros(8, np.uint64), np.zeros(8, np.float32)
        assert c.ctx.lib.nvdb_hip_range_results(c.ctx.h, ids.ctypes.data, sc.ctypes.data) == 1
    finally:
        c.ctx.set_option("range_max_mb", 4096)


def test_masked_cut_keeps_every_querys_plane_and_radius(cases):
    """largek_budget_mb = 1 (65536 candidate entries per launch set) with 20 queries on the 20000-row partition: sub-batches of at
    most three queries.  Every query has a plane and a radius of its own, so a sub-batch that read another window's mask numbers
    or radii (the offsets by its first query) answers with other rows: the bytes of the default-budget run, and the oracle's."""
    c = cases(F16, 768)
    nq = 20
    probe = np.array([[BIG, q % NPARTS, SENT] for q in range(nq)], dtype=np.uint32)
    mo = cycle(nq, 3)                                                   # planes 3 .. 8, "no mask", 0 .. : they change inside every sub-batch and across the cuts
    radius = np.array([kth_best(c.scores(q)[c.union(probe[q])], 1 + 37 * q) for q in range(nq)], dtype=np.float32)
    assert len(set(radius.tolist())) == nq and len(set(mo[:3].tolist())) == 3 and not np.array_equal(mo[:3], mo[3:6])
    whole = c.check(probe, radius, mo, what="default budget")
    chunks = c.ctx.stats()["chunks"]
    try:
        c.ctx.set_option("largek_budget_mb", 1)
        cut = c.check(probe, radius, mo, what="largek_budget_mb = 1, masked, own radii")
        for a, b in zip(whole, cut):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert c.ctx.stats()["chunks"] >= (nq + 2) // 3 and c.ctx.stats()["chunks"] > chunks     # (at least one launch per sub-batch)
    finally:
        c.ctx.set_option("largek_budget_mb", 8192)


def test_probe_table_edge_cases(cases):
    c = cases(I8, 100)
    probe = np.array([[SENT, 5, SENT, 2],          # sentinel slots
                      [3, 3, 3, 3],                # a partition named four times
                      [EMPTY, SENT, SENT, SENT],   # the empty partition alone
                      [1, 2, EMPTY, 1],            # a union of exactly 64 rows
                      [SENT, SENT, SENT, SENT]], dtype=np.uint32)
    lims, ids, sc = c.check(probe, -INF)
    assert np.diff(lims.astype(np.int64)).tolist() == [257 + 63, 64, 0, 64, 0]
    c.check(probe, c.mixed_radii(probe))
    c.check(probe, c.mixed_radii(probe), np.array([HALF, 2, SENT, 5, NONE_LIVE], dtype=np.uint32))   # (plane 2: row 0 alone, plane 5: row 63)
    # nprobe == 0: all-zero lims, an empty result that range_results hands out
    lims, ids, sc = c.ctx.range_search_partitions(c.queries[:4], -INF, np.zeros((4, 0), np.uint32))
    assert lims.tolist() == [0] * 5 and len(ids) == 0 and len(sc) == 0


# ------------------------------------------------------------------------------------------------ special values
def test_special_radii_and_a_nan_query(cases, oracle):
    c = cases(F16, 384)
    nq = 9
    probe = np.tile(np.array([[5, BIG, 2]], dtype=np.uint32), (nq, 1))
    radius = c.mixed_radii(probe)
    radius[0], radius[1], radius[2] = np.nan, INF, -INF
    c.check(probe, radius, what="NaN / +inf / -inf radius")
    # a query with a NaN element: no fault; its slice may be anything, the other queries' slices are exact
    q = c.queries[:nq].copy()
    q[4, 17] = np.nan
    got = c.ctx.range_search_partitions(q, radius, probe)
    want = slices(c.scores, lambda i: c.union(probe[i]), radius, nq, ROW_BASE)
    gl, wl = got[0].astype(np.int64), want[0].astype(np.int64)
    for i in range(nq):
        if i == 4:
            continue
        assert gl[i + 1] - gl[i] == wl[i + 1] - wl[i], i
        assert np.array_equal(got[1][gl[i]:gl[i + 1]], want[1][wl[i]:wl[i + 1]]), i
        assert np.array_equal(got[2][gl[i]:gl[i + 1]].view(np.uint32), want[2][wl[i]:wl[i + 1]].view(np.uint32)), i
    got = c.ctx.range_search_partitions(q, radius, probe, cycle(nq))
    assert len(got[0]) == nq + 1


def test_tie_group_straddling_the_radius(oracle):
    """Duplicate rows (as tests/test_gpu_partitions.py::test_ties_resolve_to_the_smaller_id): the radius is the duplicated score, so
    every copy belongs, in id order, across partitions and segments."""
    dim = 384
    base, _ = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, F16)
    base = base.copy()
    a, b, two, big = int(OFFSETS[5]), int(OFFSETS[7]), int(OFFSETS[2]), int(OFFSETS[BIG])
    base[b:b + 257] = base[a:a + 257]                       # partition 5's rows again at the start of partition 7
    base[big + 3000:big + 3064] = base[two:two + 1]         # 64 copies of partition 2's first row inside the big partition
    queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ_MAX, dim).copy()
    queries[0] = base[a + 5].view(np.float16).astype(np.float32)    # a query that IS a duplicated row: the copies lead its slice
    queries[1] = base[two].view(np.float16).astype(np.float32)
    c = Case(oracle, F16, dim, base, None, queries)
    try:
        probe = np.array([[5, 7], [BIG, 2], [7, 5]], dtype=np.uint32)
        radius = np.array([kth_best(c.scores(0)[c.union(probe[0])], 1), kth_best(c.scores(1)[c.union(probe[1])], 1),
                           kth_best(c.scores(2)[c.union(probe[2])], 10)], dtype=np.float32)
        lims, ids, sc = c.check(probe, radius)
        assert lims.tolist()[:3] == [0, 2, 2 + 65]
        assert ids[:2].tolist() == [ROW_BASE + a + 5, ROW_BASE + b + 5] and sc[0] == sc[1]
        assert ids[2:67].tolist() == [ROW_BASE + two] + [ROW_BASE + big + 3000 + j for j in range(64)] and (sc[2:67] == sc[2]).all()
        assert (lims[3] - lims[2]) % 2 == 0                 # partition 5 twice: every score comes in pairs
        # under a plane that kills every second copy
        c.check(probe, radius, np.array([HALF, HALF, SENT], dtype=np.uint32))
    finally:
        c.ctx.close()


def test_positive_zero_radius_takes_negative_zero_scores(oracle):
    """int8 rows with negative scales against an all-zero query score -0.0; radius +0.0 takes them, and the slice carries their bits."""
    dim = 100
    base, scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, I8)
    scales = scales.copy()
    scales[::3] *= np.float32(-1.0)
    queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ_MAX, dim).copy()
    queries[0] = 0.0
    queries[1] = 0.0
    c = Case(oracle, I8, dim, base, scales, queries)
    try:
        assert np.signbit(c.scores(0)).any() and not np.signbit(c.scores(0)).all() and (c.scores(0) == 0).all()
        probe = np.array([[5, 2, SENT], [BIG, 1, 5], [5, 2, 3]], dtype=np.uint32)
        radius = np.array([0.0, -0.0, kth_best(c.scores(2)[c.union([5, 2, 3])], 10)], dtype=np.float32)
        lims, ids, sc = c.check(probe, radius)
        assert lims.tolist()[:3] == [0, 257 + 63, 257 + 63 + 20000 + 1 + 257]
        assert np.signbit(sc[:320]).any() and np.array_equal(ids[:320], np.sort(ids[:320]))      # one tie group: id order
        c.check(probe, radius, np.array([HALF, HALF, HALF], dtype=np.uint32))
    finally:
        c.ctx.close()


# ------------------------------------------------------------------------------------------------ masks
def test_after_a_tombstone_update(cases, oracle):
    c = cases(F16, 768)
    ctx = nvdb_amd.HipContext(0)
    try:
        ctx.upload_corpus(c.base, F16, None, ROW_BASE)
        ctx.set_partitions(OFFSETS)
        ctx.set_row_masks(2)                                # two planes, all live
        model = np.ones((2, N), bool)
        ctx.update_row_mask(1, TOMBSTONES, False)           # two rows of one word plus a duplicate
        model[1, TOMBSTONES.astype(np.int64)] = False
        own, c.ctx = c.ctx, ctx                             # the checker on this context, the case's oracle scores
        try:
            mo = np.array([1, 0, 1, SENT, 1, 1, 0, 1, 1], dtype=np.uint32)
            probe = np.tile(np.array([1, 2, 7], dtype=np.uint32), (9, 1))      # rows 0 .. 63 and the tail: the tombstones' partitions
            c.check(probe, -INF, mo, planes=model)
            c.check(probe, c.mixed_radii(probe), mo, planes=model)
            # the flat form: the deleted rows are gone from a range search over the whole corpus
            r = np.array([kth_best(c.scores(q), 10) for q in range(9)], dtype=np.float32)
            r[4] = c.scores(4)[31]                          # a deleted row's own score: it would be on the boundary
            got = ctx.range_search_masked(c.queries[:9], r, mo)
            want = slices(c.scores, lambda q: np.flatnonzero(model[mo[q]]) if mo[q] != SENT else np.arange(N), r, 9, ROW_BASE)
            assert_same(got, want, "flat, tombstones")
            assert ROW_BASE + 31 not in got[1][int(got[0][4]):int(got[0][5])].tolist()
        finally:
            c.ctx = own
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the masked flat range search
FLAT_SEED = 20250901


@pytest.fixture(scope="module")
def flat_f16(oracle):
    """tests/test_gpu_range.py's filter-route shape: n = 20 007 fp16 d = 768 (a padded corpus)."""
    n, d, nq = 20007, 768, 40
    base = oracle.f32_to_f16(nvdb_amd.synth_rows_f32(FLAT_SEED, 0, n, d))
    queries = np.ascontiguousarray(nvdb_amd.synth_rows_f32(FLAT_SEED + 1, 0, nq, d))
    S = np.stack([oracle.scores(base, po.DT_F16, q) for q in queries])
    rs = np.random.RandomState(5)
    planes = np.stack([np.ones(n, bool), rs.rand(n) < 0.5, rs.rand(n) < 0.01, np.zeros(n, bool)])
    return dict(n=n, base=base, queries=queries, S=S, planes=planes)


def flat_check(ctx, f, radius, mask_of, nq, what):
    planes, S = f["planes"], f["S"]
    got = ctx.range_search_masked(f["queries"][:nq], radius, mask_of)
    want = slices(lambda q: S[q], lambda q: np.arange(f["n"]) if mask_of[q] == SENT else np.flatnonzero(planes[mask_of[q]]), radius, nq)
    assert_same(got, want, what)
    st = ctx.stats()
    assert st["bound_violations"] == 0, st
    return got, st


def flat_radii(f, mask_of, nq):
    """Per query, in turn: the 1st / 10th / 300th best LIVE score, a value above the best, -inf."""
    out = np.empty(nq, dtype=np.float32)
    for q in range(nq):
        s = f["S"][q] if mask_of[q] == SENT else f["S"][q][f["planes"][mask_of[q]]]
        kind = q % 5
        out[q] = -INF if kind == 4 else np.nextafter(kth_best(s, 1), INF) if kind == 3 else kth_best(s, (1, 10, 300)[kind])
    return out


@pytest.mark.parametrize("shadow", [0, 1])
def test_flat_masked_routes_agree_with_oracle(f16_flat_ctx, flat_f16, shadow):
    """path 2 (the MASKED keep step behind the fp16 filter / the int8 shadow filter), 1 (the partition range scan), 0: one answer."""
    ctx = f16_flat_ctx(shadow)
    f, nq = flat_f16, 40
    mask_of = np.array([(0, 1, 2, SENT, 1, 3)[q % 6] for q in range(nq)], dtype=np.uint32)
    radius = flat_radii(f, mask_of, nq)
    got = {}
    try:
        for path, want_path in ((2, 5), (1, 7), (0, 5)):
            ctx.set_option("path", path)
            got[path], st = flat_check(ctx, f, radius, mask_of, nq, f"shadow {shadow} path {path}")
            assert st["path"] == want_path and st["rows_scanned"] > 0, st
            if path == 2:
                assert ctx.shadow_info()["last_filter"] == ("shadow" if shadow else "f16")
        for path in (1, 0):
            for a, b in zip(got[2], got[path]):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), path
        # dead rows crowd the lists: 1 % live, the radius at the 10th live best is reached by ~1000 rows
        ctx.set_option("path", 2)
        sparse = np.full(nq, 2, dtype=np.uint32)
        r = np.array([kth_best(f["S"][q][f["planes"][2]], 10) for q in range(nq)], dtype=np.float32)
        (lims, _, _), st = flat_check(ctx, f, r, sparse, nq, "1 % live")
        assert np.all(np.diff(lims.astype(np.int64)) == 10) and st["path"] == 5 and st["candidates"] > 50 * 10 * nq, st
        ctx.set_option("cand_cap", 64)                                  # ... until they overflow: the flagged queries go to the scan
        (lims, _, _), st = flat_check(ctx, f, r, sparse, nq, "1 % live, 64-entry lists")
        assert st["path"] == 5 and st["overflow_queries"] > 0, st
        ctx.set_option("cand_cap", 0)
        # with masks resident the unmasked range search is what it was
        r = np.array([kth_best(f["S"][q], 10) for q in range(nq)], dtype=np.float32)
        got_u = ctx.range_search(f["queries"][:nq], r)
        assert_same(got_u, slices(lambda q: f["S"][q], lambda q: np.arange(f["n"]), r, nq), "unmasked, masks resident")
        assert ctx.stats()["path"] == 5
    finally:
        ctx.set_option("cand_cap", 0)
        ctx.set_option("path", 0)


@pytest.fixture(scope="module")
def f16_flat_ctx(flat_f16):
    made = {}

    def get(shadow):
        if shadow not in made:
            ctx = nvdb_amd.HipContext(0)
            ctx.set_option("q8_shadow", shadow)
            ctx.upload_corpus(flat_f16["base"], F16)
            ctx.set_row_masks(flat_f16["planes"])
            made[shadow] = ctx
        return made[shadow]
    yield get
    for ctx in made.values():
        ctx.close()


def test_flat_masked_small_dims_and_a_shape_without_a_filter(cases, oracle):
    """int8 d = 100 and fp16 d = 1 stream a zero-padded shadow copy, so the automatic route filters (path 5) and path = 1 takes the
    partition range scan over the whole corpus (path 7).  An fp32 corpus loaded with f32_shadow = 0 has no filter at all: the
    automatic route is the scan, and forcing the filter is refused.  The result is the oracle's on every route."""
    nq = 9
    mo = cycle(nq, 5)

    def run(ctx, c, path):
        r = np.array([kth_best(c.scores(q), (1, 10, 300)[q % 3]) for q in range(nq)], dtype=np.float32)
        r[8] = -INF
        ctx.set_option("path", path)
        try:
            got = ctx.range_search_masked(c.queries[:nq], r, mo)
        finally:
            ctx.set_option("path", 0)
        want = slices(c.scores, lambda q: np.arange(N) if mo[q] == SENT else np.flatnonzero(PLANES[mo[q]]), r, nq, ROW_BASE)
        assert_same(got, want, (c.dtype, c.dim, path))
        return ctx.stats()["path"]

    for dtype, dim in ((I8, 100), (F16, 1)):
        c = cases(dtype, dim)
        assert run(c.ctx, c, 0) == 5
        assert run(c.ctx, c, 1) == 7
    c = cases(F32, 7)
    ctx = nvdb_amd.HipContext(0)
    try:
        ctx.set_option("f32_shadow", 0)
        ctx.upload_corpus(c.base, F32, None, ROW_BASE)
        ctx.set_row_masks(PLANES)
        assert run(ctx, c, 0) == 7
        assert run(ctx, c, 1) == 7
        with pytest.raises(nvdb_amd.NvdbError) as e:
            run(ctx, c, 2)
        assert e.value.status == 3
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the IVF index
IVF_N, IVF_SEED, IVF_NPARTS = 2113, 20250611, 37


@pytest.mark.parametrize("dtype,dim", [(F16, 768), (I8, 100)])
def test_ivf_index_range_search(oracle, dtype, dim):
    n, nq = IVF_N, 9
    base, scales = nvdb_amd.synth_corpus(IVF_SEED, ROW_BASE, n, dim, dtype)
    v = np.random.RandomState(100 + dim).standard_normal((IVF_NPARTS, dim))
    cen = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    queries = nvdb_amd.synth_rows_f32(IVF_SEED + 1, 0, nq, dim)
    src = nvdb_amd.HipContext(0)
    src.upload_corpus(base, dtype, scales, ROW_BASE)
    ivf = nvdb_amd.IvfIndex(src, cen)
    try:
        info = ivf.info()
        assign = np.empty(n, dtype=np.int64)
        for p in range(IVF_NPARTS):
            assign[info["perm"][int(info["offsets"][p]):int(info["offsets"][p + 1])]] = p
        S = [oracle.scores(base, dtype, q, scales) for q in queries]
        planes = make_planes(n)                             # ORIGINAL rows
        ivf.set_row_masks(planes)
        for nprobe in (3, IVF_NPARTS):
            _, _, _, want_probe = ivf.search(queries, 10, nprobe, want_probe=True)
            rows_all = [np.flatnonzero(np.isin(assign, want_probe[q])) for q in range(nq)]
            radius = np.array([-INF if q % 5 == 4 else kth_best(S[q][rows_all[q]], (1, 10, 65, 300)[q % 4]) for q in range(nq)], dtype=np.float32)
            got = ivf.range_search(queries, radius, nprobe, want_probe=True)
            assert np.array_equal(got[3], want_probe)
            assert_same(got, slices(lambda q: S[q], lambda q: rows_all[q], radius, nq, ROW_BASE, tie_of=assign), f"nprobe {nprobe}")
            mo = cycle(nq, 7)
            got = ivf.range_search(queries, radius, nprobe, mo, want_probe=True)
            assert np.array_equal(got[3], want_probe)
            want = slices(lambda q: S[q], lambda q: rows_all[q] if mo[q] == SENT else rows_all[q][planes[mo[q]][rows_all[q]]], radius, nq, ROW_BASE, tie_of=assign)
            assert_same(got, want, f"nprobe {nprobe}, masked")
        # every list, radius -inf, no mask: every row exactly once
        lims, ids, sc = ivf.range_search(queries, -INF, IVF_NPARTS)
        assert np.all(np.diff(lims.astype(np.int64)) == n)
        for q in range(nq):
            assert np.array_equal(np.sort(ids[q * n:(q + 1) * n]), np.arange(n, dtype=np.uint64) + ROW_BASE)
        # the context-level form over the index's own context answers in list positions
        lims2, pos, sc2 = ivf.ctx.range_search_ivf(queries, -INF, IVF_NPARTS)
        assert np.array_equal(lims2, lims) and np.array_equal(info["perm"][pos.astype(np.int64)].astype(np.uint64) + ROW_BASE, ids)
        assert np.array_equal(sc2.view(np.uint32), sc.view(np.uint32))
    finally:
        ivf.close()
        src.close()


# ------------------------------------------------------------------------------------------------ conventions
def test_conventions(cases):
    lib = nvdb_amd.load_library()
    dim = 100
    q = nvdb_amd.synth_rows_f32(SEED + 1, 0, 4, dim)
    r = np.full(4, -INF, dtype=np.float32)
    probe = np.array([[1, 2]] * 4, dtype=np.uint32)
    mo = np.zeros(4, dtype=np.uint32)
    lims = np.full(5, 7, dtype=np.uint64)
    pr = np.full((4, 2), 7, dtype=np.uint32)

    def parts(ctx, nq=4, probe=probe, nprobe=2, mask_of=None, masked=0, queries=q, radius=r):
        return lib.nvdb_hip_range_search_partitions(ctx.h, queries.ctypes.data if queries is not None else None, nq, radius.ctypes.data if radius is not None else None,
                                                    probe.ctypes.data if probe is not None else None, nprobe, mask_of.ctypes.data if mask_of is not None else None,
                                                    masked, lims.ctypes.data, None)

    def ivf(ctx, masked=0):
        return lib.nvdb_hip_range_search_ivf(ctx.h, q.ctypes.data, 4, r.ctypes.data, 2, mo.ctypes.data, masked, lims.ctypes.data, pr.ctypes.data, None)

    def flat(ctx, mask_of=mo):
        return lib.nvdb_hip_range_search_masked(ctx.h, q.ctypes.data, 4, r.ctypes.data, mask_of.ctypes.data if mask_of is not None else None, lims.ctypes.data, None)

    ctx = nvdb_amd.HipContext(0)
    try:
        # no corpus resident
        assert parts(ctx) == 4 and ivf(ctx) == 4 and flat(ctx) == 4
        assert "Empty base" in lib.nvdb_hip_last_error(ctx.h).decode()
        base, scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, I8)
        ctx.upload_corpus(base, I8, scales, ROW_BASE)
        # no partition table; no planes
        assert parts(ctx) == 1 and "partition" in lib.nvdb_hip_last_error(ctx.h).decode()
        assert ivf(ctx) == 1
        assert flat(ctx) == 1 and "row masks" in lib.nvdb_hip_last_error(ctx.h).decode()
        ctx.set_partitions(OFFSETS)
        assert ivf(ctx) == 1 and "centroids" in lib.nvdb_hip_last_error(ctx.h).decode()
        assert parts(ctx, mask_of=mo, masked=1) == 1 and "row masks" in lib.nvdb_hip_last_error(ctx.h).decode()
        assert (lims == 7).all() and (pr == 7).all()                         # nothing written so far
        # null pointers
        assert lib.nvdb_hip_range_search_partitions(ctx.h, q.ctypes.data, 4, r.ctypes.data, probe.ctypes.data, 2, None, 0, None, None) == 1
        assert parts(ctx, queries=None) == 1 and parts(ctx, radius=None) == 1 and parts(ctx, probe=None) == 1
        # a probe entry >= nparts that is not the sentinel: refused on the host
        badp = probe.copy()
        badp[3, 1] = NPARTS
        assert parts(ctx, probe=badp) == 1 and "probe" in lib.nvdb_hip_last_error(ctx.h).decode()
        ids, sc = np.zeros(8, np.uint64), np.zeros(8, np.float32)
        assert lib.nvdb_hip_range_results(ctx.h, ids.ctypes.data, sc.ctypes.data) == 1     # ... and nothing is held
        # mask_of against the planes
        ctx.set_row_masks(2)
        bad = np.array([0, 1, 2, 0], dtype=np.uint32)
        lims[:] = 7
        assert parts(ctx, mask_of=bad, masked=1) == 1 and flat(ctx, bad) == 1 and (lims == 7).all()
        assert parts(ctx, mask_of=bad, masked=0) == 0                          # unmasked: mask_of is ignored
        assert lims.tolist() == [0, 64, 128, 192, 256]
        assert parts(ctx, mask_of=None, masked=1) == 0 and lims.tolist() == [0, 64, 128, 192, 256]   # NULL: plane 0
        assert flat(ctx, None) == 0 and lims.tolist() == [0, N, 2 * N, 3 * N, 4 * N]
        # nq == 0; nprobe == 0
        lims[:] = 7
        assert parts(ctx, nq=0, queries=None, radius=None, probe=None) == 0 and lims[0] == 0 and (lims[1:] == 7).all()
        assert lib.nvdb_hip_range_search_masked(ctx.h, None, 0, None, None, lims.ctypes.data, None) == 0
        assert parts(ctx, probe=None, nprobe=0) == 0 and (lims == 0).all()
        # a range search of any kind replaces the held result
        a = ctx.range_search_partitions(q, r, probe)
        b = ctx.range_search(q[:1], np.float32(np.inf))
        assert int(a[0][-1]) == 256 and int(b[0][-1]) == 0
        assert lib.nvdb_hip_range_results(ctx.h, ids.ctypes.data, sc.ctypes.data) == 0     # the flat search's (empty) result
        # a new corpus drops table, planes and the held result
        ctx.range_search_partitions(q, r, probe)
        ctx.upload_corpus(base, I8, scales, ROW_BASE)
        assert lib.nvdb_hip_range_results(ctx.h, ids.ctypes.data, sc.ctypes.data) == 1
        assert parts(ctx) == 1
    finally:
        ctx.close()
    # calls of different sizes reuse the workspace; top-k searches in between see their own results
    c = cases(I8, 100)
    rs = np.random.RandomState(5)
    for nq, npr in ((70, 3), (9, 3), (33, 2)):
        p = rs.randint(0, NPARTS, size=(nq, npr)).astype(np.uint32)
        c.check(p, c.mixed_radii(p))
        ids, sc, cnt = c.ctx.search_partitions(c.queries[:nq], 10, p)
        for qq in range(0, nq, 7):
            rows = c.union(p[qq])
            order = np.lexsort((rows, -c.scores(qq)[rows]))[:10]
            assert np.array_equal(ids[qq, :len(order)], rows[order].astype(np.uint64) + ROW_BASE)
        assert c.ctx.stats()["path"] == 4
