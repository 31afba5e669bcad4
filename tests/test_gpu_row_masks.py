"""Row masks (nvdb_hip_set_row_masks / update_row_mask / get_row_masks and the masked searches) against the oracle.

The checker is the oracle's full score vector per query, restricted to the rows that are in a probed partition AND live in the
query's mask, top-k by (score desc, id asc): ids, score BITS and counts must be equal -- where equal scores meet both sides order
by id, so there is no tolerance and no excluded case.  The corpus shape is tests/test_gpu_partitions.py's."""
import ctypes as C

import numpy as np
import pytest

import nvdb_amd
import pyoracle as po

pytestmark = pytest.mark.gpu

N, ROW_BASE, SEED = 30000, 1_000_003, 20250117
SIZES = [0, 1, 63, 64, 65, 257, 20000]
OFFSETS = np.concatenate([[0], np.cumsum(SIZES + [N - sum(SIZES)])]).astype(np.uint64)
NPARTS = len(OFFSETS) - 1
BIG = 6
SENT = 0xFFFFFFFF
U64MAX = np.iinfo(np.uint64).max
NQ_MAX = 70
F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8


def make_planes():
    rs = np.random.RandomState(77)
    planes = [np.ones(N, bool), np.zeros(N, bool)]                      # 0 all live, 1 all dead
    for r in (0, 31, 32, 63, 64, N - 1):                                # 2 .. 7: exactly one live row at a word / tile / corpus edge
        p = np.zeros(N, bool)
        p[r] = True
        planes.append(p)
    planes.append(np.arange(N) % 2 == 0)                                # 8 alternating bits
    p = np.zeros(N, bool)
    p[int(OFFSETS[BIG + 1]) - 5:int(OFFSETS[BIG + 1])] = True           # 9 the last 5 rows of the 20000-row partition (a ragged final tile)
    planes.append(p)
    planes.append(rs.rand(N) < 0.5)                                     # 10 random 50 %
    planes.append(rs.rand(N) < 0.01)                                    # 11 random 1 %: many unions hold fewer than k live rows
    return np.stack(planes)


PLANES = make_planes()
NMASKS = len(PLANES)
ALL_LIVE, ALL_DEAD, ALTERNATING, BIG_TAIL, HALF, SPARSE = 0, 1, 8, 9, 10, 11


def topk(scores, rows, k, tie=None):
    """rows: candidate local rows -> (ids [k] with ROW_BASE, score bits [k], count), (score desc, [tie,] row asc)."""
    s = scores[rows]
    order = np.lexsort((rows, -s) if tie is None else (rows, tie[rows], -s))[:k]
    ids = np.full(k, U64MAX, dtype=np.uint64)
    sc = np.full(k, -np.inf, dtype=np.float32)
    ids[:len(order)] = rows[order].astype(np.uint64) + ROW_BASE
    sc[:len(order)] = s[order]
    return ids, sc, min(k, len(rows))


class Case:
    """One resident corpus (dtype, dim) with the partition table, the mask planes, queries and lazily computed oracle scores."""

    def __init__(self, orc, dtype, dim):
        self.orc, self.dtype, self.dim = orc, dtype, dim
        self.base, self.scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
        self.queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ_MAX, dim)
        self.ctx = nvdb_amd.HipContext(0)
        self.ctx.upload_corpus(self.base, dtype, self.scales, ROW_BASE)
        self.ctx.set_partitions(OFFSETS)
        self.ctx.set_row_masks(PLANES)
        self._scores = {}

    def scores(self, q):
        if q not in self._scores:
            self._scores[q] = self.orc.scores(self.base, self.dtype, self.queries[q], self.scales)
        return self._scores[q]

    def expect(self, q, parts, k, live):
        """parts: probed partitions (None: every row); live: bool [N] (None: no mask)."""
        in_union = np.ones(N, bool)
        if parts is not None:
            in_union[:] = False
            for p in set(parts):
                in_union[int(OFFSETS[p]):int(OFFSETS[p + 1])] = True
        if live is not None:
            in_union &= live
        return topk(self.scores(q), np.flatnonzero(in_union), k)

    def compare(self, got, want_of, nq):
        ids, sc, counts = got
        for q in range(nq):
            eid, esc, ecnt = want_of(q)
            assert counts[q] == ecnt, (q, counts[q], ecnt)
            assert np.array_equal(ids[q], eid), (q, ids[q], eid)
            assert np.array_equal(sc[q].view(np.uint32), esc.view(np.uint32)), (q, sc[q], esc)

    def check_parts(self, probe, k, mask_of, planes=PLANES):
        probe = np.asarray(probe, dtype=np.uint32)
        nq = probe.shape[0]
        mo = None if mask_of is None else np.asarray(mask_of, dtype=np.uint32)
        got = self.ctx.search_partitions_masked(self.queries[:nq], k, probe, mo)

        def want(q):
            m = 0 if mo is None else int(mo[q])
            return self.expect(q, [p for p in probe[q] if p != SENT], k, None if m == SENT else planes[m])
        self.compare(got, want, nq)
        return got

    def check_flat(self, nq, k, mask_of, planes=PLANES):
        mo = None if mask_of is None else np.asarray(mask_of, dtype=np.uint32)
        got = self.ctx.search_masked(self.queries[:nq], k, mo)

        def want(q):
            m = 0 if mo is None else int(mo[q])
            return self.expect(q, None, k, None if m == SENT else planes[m])
        self.compare(got, want, nq)
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


# one case per build: staged (f16 768, f32 384, i8 384), direct aligned (f32 768: a tile does not fit the LDS), direct unaligned (f16 7,
# i8 100, f32 1); then the corners of nq / k / nprobe on a staged and a direct build
GRID = [(dt, d, 9, 10, 3) for dt, d in ((F16, 768), (F32, 384), (I8, 384), (F32, 768), (F16, 7), (I8, 100), (F32, 1))] + \
       [(dt, d, nq, k, npr) for dt, d in ((F16, 768), (I8, 100)) for nq, k, npr in ((70, 64, 3), (1, 1, 1), (70, 10, 1))]


@pytest.mark.parametrize("dtype,dim,nq,k,nprobe", GRID)
def test_parity_grid(cases, dtype, dim, nq, k, nprobe):
    c = cases(dtype, dim)
    rs = np.random.RandomState(1000 * dtype + dim + nq + k + nprobe)
    probe = rs.randint(0, NPARTS, size=(nq, nprobe)).astype(np.uint32)
    c.check_parts(probe, k, cycle(nq))                                              # every plane, random unions
    dense = rs.choice([ALL_LIVE, ALTERNATING, BIG_TAIL, HALF, SPARSE, SENT], size=nq)
    big = np.concatenate([np.full((nq, 1), BIG, dtype=np.uint32), probe[:, 1:]], axis=1)
    c.check_parts(big, k, dense)                                                    # the big partition under the planes that have rows in it
    c.check_parts(probe, k, None)                                                   # mask_of == NULL: plane 0 for every query


@pytest.mark.parametrize("dtype,dim", [(F16, 768), (I8, 100), (F32, 384)])
def test_mixed_masks_in_one_group(cases, dtype, dim):
    """All 70 queries probe the 20000-row partition, neighbours under different planes: a wave must not share liveness between
    its queries."""
    c = cases(dtype, dim)
    mo = np.array([HALF, SPARSE, ALTERNATING, SENT] * 18, dtype=np.uint32)[:NQ_MAX]
    ids, sc, counts = c.check_parts(np.full((NQ_MAX, 1), BIG, dtype=np.uint32), 10, mo)
    assert (counts == 10).all()
    c.check_parts(np.full((NQ_MAX, 1), BIG, dtype=np.uint32), 64, np.roll(mo, 1))
    # the same group under planes that leave 5, 0 and at most 1 of its rows
    mo = np.array([BIG_TAIL, ALL_DEAD, 3, SENT, 7] * 14, dtype=np.uint32)[:NQ_MAX]
    ids, sc, counts = c.check_parts(np.full((NQ_MAX, 1), BIG, dtype=np.uint32), 10, mo)
    assert counts[0] == 5 and counts[1] == 0 and counts[3] == 10
    assert (ids[1] == U64MAX).all() and np.isneginf(sc[1]).all() and (ids[0, 5:] == U64MAX).all() and np.isneginf(sc[0, 5:]).all()


@pytest.mark.parametrize("dtype,dim", [(F16, 768), (I8, 100)])
@pytest.mark.parametrize("nq", [1, 9, 70])
def test_flat(cases, dtype, dim, nq):
    c = cases(dtype, dim)
    rs = np.random.RandomState(nq)
    probe = rs.randint(0, NPARTS, size=(9, 3)).astype(np.uint32)
    before = c.ctx.search_partitions(c.queries[:9], 10, probe)
    c.check_flat(nq, 10, cycle(nq, 5))                      # with the partition table set
    c.check_flat(nq, 64, cycle(nq, 8))
    c.check_flat(nq, 10, None)
    st = c.ctx.stats()
    assert st["path"] == 4 and st["rows_scanned"] >= N
    after = c.ctx.search_partitions(c.queries[:9], 10, probe)   # the table still serves the probe search, identically
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()


def test_flat_without_a_partition_table(oracle):
    c = Case.__new__(Case)
    c.orc, c.dtype, c.dim = oracle, F16, 100
    c.base, c.scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, c.dim, F16)
    c.queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ_MAX, c.dim)
    c._scores = {}
    c.ctx = nvdb_amd.HipContext(0)
    try:
        c.ctx.upload_corpus(c.base, F16, None, ROW_BASE)
        c.ctx.set_row_masks(PLANES)
        for nq in (1, 9, 70):
            c.check_flat(nq, 10, cycle(nq, 3))
        ids = np.full((2, 10), 7, dtype=np.uint64)
        sc = np.full((2, 10), 7.0, dtype=np.float32)
        cnt = np.full(2, 7, dtype=np.uint32)
        probe = np.zeros((2, 1), dtype=np.uint32)
        # no table was made on the way
        assert c.ctx.lib.nvdb_hip_search_partitions(c.ctx.h, c.queries.ctypes.data, 2, 10, probe.ctypes.data, 1, ids.ctypes.data, sc.ctypes.data,
                                                    cnt.ctypes.data, None) == 1
        assert (ids == 7).all()
    finally:
        c.ctx.close()


def _ivf_setup(c, nparts=16):
    cen = np.random.RandomState(100 + c.dim).standard_normal((nparts, c.dim)).astype(np.float32)
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    ivf = nvdb_amd.IvfIndex(c.ctx, cen)
    info = ivf.info()
    assign = np.empty(N, dtype=np.int64)                    # the build itself is tests/test_gpu_ivf.py's subject: read its lists
    for p in range(nparts):
        assign[info["perm"][int(info["offsets"][p]):int(info["offsets"][p + 1])]] = p
    return ivf, cen, info, assign


def _ivf_expect(c, cen, assign, q, k, nprobe, live):
    """tests/test_gpu_ivf.py's order: the nprobe best centroids (ties by number), then (score desc, partition, original row)."""
    cs = c.orc.scores(cen, po.DT_F32, c.queries[q])
    probes = np.lexsort((np.arange(len(cen)), -cs))[:nprobe]
    ok = np.isin(assign, probes)
    if live is not None:
        ok &= live
    return topk(c.scores(q), np.flatnonzero(ok), k, tie=assign) + (probes.astype(np.uint32),)


@pytest.mark.parametrize("dtype,dim", [(F16, 768), (I8, 100)])
def test_ivf_in_original_ids(cases, dtype, dim):
    c = cases(dtype, dim)
    ivf, cen, info, assign = _ivf_setup(c)
    try:
        ivf.set_row_masks(PLANES)                           # planes indexed by ORIGINAL row
        perm = info["perm"]
        assert np.array_equal(nvdb_amd.unpack_row_masks(ivf.ctx.get_row_masks(), N), PLANES[:, perm])
        nq, nprobe = 9, 3
        mo = np.array([HALF, SPARSE, ALTERNATING, SENT, ALL_LIVE, ALL_DEAD, BIG_TAIL, 2, 7], dtype=np.uint32)
        for k in (10, 64):
            ids, sc, counts, probe = ivf.search_masked(c.queries[:nq], k, nprobe, mo, want_probe=True)
            pid, psc, pcnt, pprobe = ivf.ctx.search_ivf_masked(c.queries[:nq], k, nprobe, mo, want_probe=True)   # positions, row base 0
            for q in range(nq):
                m = int(mo[q])
                eid, esc, ecnt, eprobe = _ivf_expect(c, cen, assign, q, k, nprobe, None if m == SENT else PLANES[m])
                assert np.array_equal(probe[q], eprobe) and np.array_equal(pprobe[q], eprobe)
                assert counts[q] == ecnt and pcnt[q] == ecnt, (q, counts[q], pcnt[q], ecnt)
                assert np.array_equal(ids[q], eid), (q, ids[q], eid)
                assert np.array_equal(sc[q].view(np.uint32), esc.view(np.uint32)) and np.array_equal(psc[q].view(np.uint32), esc.view(np.uint32))
                assert np.array_equal(perm[pid[q, :ecnt].astype(np.int64)].astype(np.uint64) + ROW_BASE, eid[:ecnt]) and (pid[q, ecnt:] == U64MAX).all()
        # the unmasked index search ignores the masks
        ids, sc, counts = ivf.search(c.queries[:nq], 10, nprobe)
        for q in range(nq):
            eid, esc, ecnt, _ = _ivf_expect(c, cen, assign, q, 10, nprobe, None)
            assert np.array_equal(ids[q], eid) and np.array_equal(sc[q].view(np.uint32), esc.view(np.uint32)) and counts[q] == ecnt
    finally:
        ivf.close()


TOMBSTONES = np.array([0, 31, 32, 32, 63, 64, N - 1], dtype=np.uint64)   # a duplicate, and two rows of one word, in one call


def test_update(cases):
    c = cases(F16, 768)
    ctx = nvdb_amd.HipContext(0)
    try:
        ctx.upload_corpus(c.base, F16, None, ROW_BASE)
        ctx.set_partitions(OFFSETS)
        ctx.set_row_masks(2)                                # two planes, all live
        model = np.ones((2, N), bool)
        assert np.array_equal(nvdb_amd.unpack_row_masks(ctx.get_row_masks(), N), model)
        assert ctx.get_row_masks().shape == (2, (N + 31) // 32) and (ctx.get_row_masks()[:, -1] >> np.uint32(N % 32) == 0).all()   # tail bits read back as 0
        ctx.update_row_mask(1, TOMBSTONES, False)
        model[1, TOMBSTONES.astype(np.int64)] = False
        ctx.update_row_mask(1, [32], True)
        model[1, 32] = True
        ctx.update_row_mask(1, [], False)                   # nrows == 0: OK, nothing changes
        assert np.array_equal(nvdb_amd.unpack_row_masks(ctx.get_row_masks(), N), model)
        own, c.ctx = c.ctx, ctx                             # the checkers on this context, the case's oracle scores
        try:
            mo = np.array([1, 0, 1, SENT, 1, 1, 0, 1, 1], dtype=np.uint32)
            c.check_parts(np.tile(np.arange(NPARTS, dtype=np.uint32), (9, 1)), 64, mo, planes=model)
            c.check_parts(np.tile(np.array([1, 2, 7], dtype=np.uint32), (9, 1)), 64, mo, planes=model)   # rows 0 .. 63 and the tail: the tombstones' partitions
            c.check_flat(9, 10, mo, planes=model)
        finally:
            c.ctx = own
    finally:
        ctx.close()


def test_update_through_the_ivf_index(cases):
    c = cases(F16, 768)
    ivf, cen, info, assign = _ivf_setup(c)
    try:
        ivf.set_row_masks(2)
        model = np.ones((2, N), bool)
        ivf.update_row_mask(1, TOMBSTONES, False)           # ORIGINAL rows
        model[1, TOMBSTONES.astype(np.int64)] = False
        ivf.update_row_mask(1, [32], True)
        model[1, 32] = True
        assert np.array_equal(nvdb_amd.unpack_row_masks(ivf.ctx.get_row_masks(), N), model[:, info["perm"]])
        nq, nparts = 9, len(cen)
        mo = np.array([1, 0, 1, SENT, 1, 1, 0, 1, 1], dtype=np.uint32)
        ids, sc, counts = ivf.search_masked(c.queries[:nq], 64, nparts, mo)        # every list: the tombstones are in the union
        for q in range(nq):
            m = int(mo[q])
            eid, esc, ecnt, _ = _ivf_expect(c, cen, assign, q, 64, nparts, None if m == SENT else model[m])
            assert np.array_equal(ids[q], eid) and np.array_equal(sc[q].view(np.uint32), esc.view(np.uint32)) and counts[q] == ecnt
        bad = np.array([5, N], dtype=np.uint64)
        assert ivf.lib.nvdb_hip_ivf_update_row_mask(ivf.h, 1, bad.ctypes.data, 2, 0) == 1
        assert ivf.lib.nvdb_hip_ivf_update_row_mask(ivf.h, 2, bad.ctypes.data, 1, 0) == 1
        assert np.array_equal(nvdb_amd.unpack_row_masks(ivf.ctx.get_row_masks(), N), model[:, info["perm"]])
    finally:
        ivf.close()


def test_unmasked_entry_points_ignore_resident_masks(cases):
    c = cases(F16, 100)
    rs = np.random.RandomState(3)
    probe = rs.randint(0, NPARTS, size=(9, 3)).astype(np.uint32)
    cen = rs.standard_normal((NPARTS, c.dim)).astype(np.float32)
    fresh = nvdb_amd.HipContext(0)
    try:
        fresh.upload_corpus(c.base, F16, None, ROW_BASE)
        fresh.set_partitions(OFFSETS)
        fresh.set_centroids(cen)
        c.ctx.set_centroids(cen)                            # (set_partitions / set_centroids keep the masks)
        assert c.ctx.get_row_masks().shape[0] == NMASKS
        for call in (lambda x: x.search_partitions(c.queries[:9], 10, probe), lambda x: x.search_ivf(c.queries[:9], 10, 3, want_probe=True),
                     lambda x: x.search_batch(c.queries[:9], 10), lambda x: x.search_batch(c.queries[:70], 64)):
            for a, b in zip(call(c.ctx), call(fresh)):
                assert a.tobytes() == b.tobytes()
            assert c.ctx.stats()["path"] == fresh.stats()["path"]
        c.ctx.set_partitions(OFFSETS)
        assert np.array_equal(nvdb_amd.unpack_row_masks(c.ctx.get_row_masks(), N), PLANES)
    finally:
        fresh.close()


def test_conventions():
    lib = nvdb_amd.load_library()
    dim = 100
    q = nvdb_amd.synth_rows_f32(SEED + 1, 0, 4, dim)
    probe = np.array([[1, 2]] * 4, dtype=np.uint32)
    ids = np.full((4, 65), 7, dtype=np.uint64)
    sc = np.full((4, 65), 7.0, dtype=np.float32)
    cnt = np.full(4, 7, dtype=np.uint32)
    pr = np.full((4, 2), 7, dtype=np.uint32)
    mo = np.array([0, 1, SENT, 2], dtype=np.uint32)
    rows = np.array([1, 2], dtype=np.uint64)

    def untouched():
        return (ids == 7).all() and (sc == 7.0).all() and (cnt == 7).all() and (pr == 7).all()

    def parts(ctx, k, nprobe, mask_of, p=probe):
        return lib.nvdb_hip_search_partitions_masked(ctx.h, q.ctypes.data, 4, k, p.ctypes.data if p is not None else None, nprobe,
                                                     mask_of.ctypes.data if mask_of is not None else None, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None)

    def ivf(ctx, k, nprobe, mask_of):
        return lib.nvdb_hip_search_ivf_masked(ctx.h, q.ctypes.data, 4, k, nprobe, mask_of.ctypes.data if mask_of is not None else None,
                                              ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, pr.ctypes.data, None)

    def flat(ctx, k, mask_of):
        return lib.nvdb_hip_search_batch_masked(ctx.h, q.ctypes.data, 4, k, mask_of.ctypes.data if mask_of is not None else None,
                                                ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None)

    ctx = nvdb_amd.HipContext(0)
    try:
        # no corpus resident
        assert lib.nvdb_hip_set_row_masks(ctx.h, None, 1) == 4
        assert lib.nvdb_hip_update_row_mask(ctx.h, 0, rows.ctypes.data, 2, 0) == 4
        assert parts(ctx, 10, 2, mo) == 4 and flat(ctx, 10, mo) == 4 and ivf(ctx, 10, 2, mo) == 4
        assert ctx.get_row_masks().shape == (0, 0)
        base, _ = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, F16)
        ctx.upload_corpus(base, F16, None, ROW_BASE)
        ctx.set_partitions(OFFSETS)
        ctx.set_centroids(np.ones((NPARTS, dim), dtype=np.float32))
        # masks absent -> INVALID, nothing written
        assert parts(ctx, 10, 2, mo) == 1 and "mask" in lib.nvdb_hip_last_error(ctx.h).decode()
        assert parts(ctx, 10, 2, None) == 1 and flat(ctx, 10, mo) == 1 and flat(ctx, 10, None) == 1 and ivf(ctx, 10, 2, mo) == 1
        assert lib.nvdb_hip_update_row_mask(ctx.h, 0, rows.ctypes.data, 2, 0) == 1
        assert untouched()
        assert lib.nvdb_hip_set_row_masks(ctx.h, None, SENT) == 1
        ctx.set_row_masks(3)
        # a mask_of entry >= nmasks that is not the "no mask" number -> INVALID, nothing written
        bad = np.array([0, 1, 3, 2], dtype=np.uint32)
        assert parts(ctx, 10, 2, bad) == 1 and flat(ctx, 10, bad) == 1 and ivf(ctx, 10, 2, bad) == 1
        assert untouched()
        # an update row >= n, or a mask >= nmasks -> INVALID, nothing changed
        before = ctx.get_row_masks()
        badrows = np.array([5, N], dtype=np.uint64)
        assert lib.nvdb_hip_update_row_mask(ctx.h, 0, badrows.ctypes.data, 2, 0) == 1
        assert lib.nvdb_hip_update_row_mask(ctx.h, 3, rows.ctypes.data, 2, 0) == 1
        assert np.array_equal(ctx.get_row_masks(), before)
        assert lib.nvdb_hip_update_row_mask(ctx.h, 0, None, 0, 0) == 0
        # k == 0 / nq == 0: OK, nothing written; k = 65: UNSUPPORTED
        assert parts(ctx, 0, 2, mo) == 0 and flat(ctx, 0, mo) == 0 and ivf(ctx, 0, 2, mo) == 0
        assert lib.nvdb_hip_search_batch_masked(ctx.h, q.ctypes.data, 0, 10, mo.ctypes.data, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None) == 0
        assert parts(ctx, 65, 2, mo) == 3 and flat(ctx, 65, mo) == 3 and ivf(ctx, 65, 2, mo) == 3
        assert untouched()
        # a probe entry >= nparts: refused on the host as in the unmasked call
        badp = probe.copy()
        badp[3, 1] = NPARTS
        assert parts(ctx, 10, 2, mo, badp) == 1 and untouched()
        # nprobe == 0: every count 0, all padding
        assert parts(ctx, 10, 0, mo, None) == 0
        assert (cnt == 0).all() and (ids.ravel()[:40] == U64MAX).all() and np.isneginf(sc.ravel()[:40]).all() and (ids.ravel()[40:] == 7).all()
        cnt[:] = 7
        assert ivf(ctx, 10, 0, mo) == 0 and (cnt == 0).all()
        # a good call with timing and statistics; then a new corpus drops the masks
        ctx.update_row_mask(1, np.arange(int(OFFSETS[1]), int(OFFSETS[3])), False)       # plane 1: partitions 1 and 2 are dead
        gid, gsc, gcnt, t = ctx.search_partitions_masked(q, 10, probe, mo, want_timing=True)
        assert gcnt.tolist() == [10, 0, 10, 10] and (gid[1] == U64MAX).all() and np.isneginf(gsc[1]).all()
        assert t.kernel_ms > 0 and t.total_ms >= t.kernel_ms and t.K == 10 and t.threads == 64 * t.nwarps > 0
        st = ctx.stats()
        assert st["path"] == 4 and st["rows_scanned"] == 64 and st["chunks"] >= 1
        ctx.upload_corpus(base, F16, None, ROW_BASE)
        assert ctx.get_row_masks().shape[0] == 0
        nm, w = C.c_uint32(7), C.c_uint64(7)
        assert lib.nvdb_hip_get_row_masks(ctx.h, C.byref(nm), C.byref(w), None) == 0 and nm.value == 0 and w.value == 0
        ctx.set_partitions(OFFSETS)
        ids[:], sc[:], cnt[:] = 7, 7.0, 7
        assert parts(ctx, 10, 2, mo) == 1 and flat(ctx, 10, None) == 1 and untouched()
        ctx.set_row_masks(0)                                # dropping what is not there is fine
        ctx.set_row_masks(PLANES)
        ctx.set_row_masks(0)
        assert ctx.get_row_masks().shape[0] == 0 and parts(ctx, 10, 2, mo) == 1
    finally:
        ctx.close()

