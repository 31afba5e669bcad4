"""Partitioned probe search (nvdb_hip_search_partitions / nvdb_hip_search_ivf) against the oracle.

The checker is the oracle's full score vector per query, masked to the rows of the probed partitions, top-k by (score desc,
id asc): ids and score BITS must be equal -- where equal scores meet both sides order by id, so there is no set-wise slack."""
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
U64MAX = np.iinfo(np.uint64).max
NQ_MAX = 70


class Case:
    """One resident corpus (dtype, dim) with its partition table, queries and lazily computed oracle scores."""

    def __init__(self, orc, dtype, dim):
        self.orc, self.dtype, self.dim = orc, dtype, dim
        self.base, self.scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
        self.queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ_MAX, dim)
        self.ctx = nvdb_amd.HipContext(0)
        self.ctx.upload_corpus(self.base, dtype, self.scales, ROW_BASE)
        self.ctx.set_partitions(OFFSETS)
        self._scores = {}

    def scores(self, q):
        if q not in self._scores:
            self._scores[q] = self.orc.scores(self.base, self.dtype, self.queries[q], self.scales)
        return self._scores[q]

    def expect(self, q, parts, k, offsets=OFFSETS):
        rows = np.concatenate([np.arange(offsets[p], offsets[p + 1], dtype=np.int64) for p in sorted(set(parts))] + [np.empty(0, np.int64)])
        s = self.scores(q)[rows]
        order = np.lexsort((rows, -s))[:k]
        ids = np.full(k, U64MAX, dtype=np.uint64)
        sc = np.full(k, -np.inf, dtype=np.float32)
        ids[:len(order)] = rows[order].astype(np.uint64) + ROW_BASE
        sc[:len(order)] = s[order]
        return ids, sc, min(k, len(rows))

    def check(self, probe, k, nq=None):
        probe = np.asarray(probe, dtype=np.uint32)
        nq = probe.shape[0] if nq is None else nq
        ids, sc, counts = self.ctx.search_partitions(self.queries[:nq], k, probe)
        for q in range(nq):
            eid, esc, ecnt = self.expect(q, [p for p in probe[q] if p != SENT], k)
            assert counts[q] == ecnt, (q, counts[q], ecnt)
            assert np.array_equal(ids[q], eid), (q, ids[q], eid)
            assert np.array_equal(sc[q].view(np.uint32), esc.view(np.uint32)), (q, sc[q], esc)
        return ids, sc, counts


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


F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8
# every dim for every dtype at nq = 9, k = 10; then the corners of nq / k / nprobe on the builds that differ: rows staged through LDS
# (f16 384 / 768, f32 100 / 384, i8 384 / 768), direct aligned (f32 768: a tile does not fit the LDS), direct unaligned (the rest)
GRID = [(dt, d, 9, 10, 3) for dt in (F32, F16, I8) for d in (1, 7, 100, 384, 768)] + [
    (F16, 768, 70, 64, 3), (F16, 768, 1, 1, 1), (F16, 384, 70, 10, 1), (F32, 7, 70, 10, 1), (F32, 100, 70, 64, 3), (F32, 768, 9, 64, 1),
    (F32, 384, 1, 64, 3), (I8, 100, 70, 64, 3), (I8, 768, 70, 1, 1), (I8, 384, 1, 10, 1), (F16, 1, 70, 64, 3),
]


@pytest.mark.parametrize("dtype,dim,nq,k,nprobe", GRID)
def test_parity_grid(cases, dtype, dim, nq, k, nprobe):
    c = cases(dtype, dim)
    rs = np.random.RandomState(1000 * dtype + dim + nq + k + nprobe)
    probe = rs.randint(0, NPARTS, size=(nq, nprobe)).astype(np.uint32)
    c.check(probe, k)


@pytest.mark.parametrize("dtype,dim", [(F16, 768), (I8, 100), (F32, 384)])
def test_grouping(cases, dtype, dim):
    c = cases(dtype, dim)
    # all 70 queries probe the 20 000-row partition: more than one group of queries, over several segments
    c.check(np.full((NQ_MAX, 1), BIG, dtype=np.uint32), 10)
    # every query a different partition
    c.check(np.arange(NPARTS, dtype=np.uint32)[:, None], 10)


def test_probe_table_edge_cases(cases):
    c = cases(F16, 100)
    probe = np.array([[SENT, 5, SENT, 2],          # sentinel slots
                      [3, 3, 3, 3],                # a partition named over and over
                      [EMPTY, SENT, SENT, SENT],   # the empty partition alone
                      [1, 2, EMPTY, 1],            # a union of exactly 64 rows
                      [SENT, SENT, SENT, SENT]], dtype=np.uint32)
    ids, sc, counts = c.check(probe, 10)
    assert counts[2] == 0 and (ids[2] == U64MAX).all() and np.isneginf(sc[2]).all()
    assert counts[4] == 0 and (ids[4] == U64MAX).all()
    assert counts[1] == 10
    ids, sc, counts = c.check(probe, 64)
    assert counts[1] == 64 and counts[3] == 64 and counts[0] == 64
    probe = np.array([[1, EMPTY], [1, 2]], dtype=np.uint32)
    ids, sc, counts = c.check(probe, 64)           # a union smaller than k: count < k, padding after it
    assert counts.tolist() == [1, 64] and (ids[0, 1:] == U64MAX).all() and np.isneginf(sc[0, 1:]).all()
    ids, sc, counts = c.check(np.array([[1, 3]], dtype=np.uint32), 64)
    assert counts.tolist() == [64]
    ids, sc, counts = c.check(np.array([[1, 2]], dtype=np.uint32), 10)
    assert counts.tolist() == [10]


def test_ties_resolve_to_the_smaller_id(oracle):
    dim = 384
    c = Case.__new__(Case)
    c.orc, c.dtype, c.dim = oracle, F16, dim
    c.base, c.scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, F16)
    c.base = c.base.copy()
    a, b, two, big = int(OFFSETS[5]), int(OFFSETS[7]), int(OFFSETS[2]), int(OFFSETS[BIG])
    c.base[b:b + 257] = c.base[a:a + 257]                   # partition 5's rows again at the start of partition 7
    c.base[big + 3000:big + 3064] = c.base[two:two + 1]     # 64 copies of partition 2's first row inside the big partition
    c.queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ_MAX, dim).copy()
    c.queries[0] = c.base[a + 5].view(np.float16).astype(np.float32)    # a query that IS a duplicated row: the copies lead its list
    c.queries[1] = c.base[two].view(np.float16).astype(np.float32)
    c._scores = {}
    c.ctx = nvdb_amd.HipContext(0)
    try:
        c.ctx.upload_corpus(c.base, F16, None, ROW_BASE)
        c.ctx.set_partitions(OFFSETS)
        ids, sc, _ = c.check(np.array([[5, 7], [BIG, 2], [7, 5]], dtype=np.uint32), 64)
        assert ids[0, 0] == ROW_BASE + a + 5 and ids[0, 1] == ROW_BASE + b + 5 and sc[0, 0] == sc[0, 1]
        assert ids[1, 0] == ROW_BASE + two and ids[1, 1:].tolist() == [ROW_BASE + big + 3000 + j for j in range(63)]
        assert (sc[1] == sc[1, 0]).all()
        c.check(np.array([[5, 7]] * 9, dtype=np.uint32), 10)
    finally:
        c.ctx.close()


def _centroids(c):
    f = c.base.view(np.float16).astype(np.float32) if c.dtype == F16 else c.base.astype(np.float32)
    if c.dtype == I8:
        f = f * c.scales[:, None]
    cen = np.zeros((NPARTS, c.dim), dtype=np.float32)
    for p in range(NPARTS):
        lo, hi = int(OFFSETS[p]), int(OFFSETS[p + 1])
        if hi > lo:
            cen[p] = f[lo:hi].mean(axis=0, dtype=np.float32)
    return cen


@pytest.mark.parametrize("dtype,dim", [(F16, 768), (F32, 100), (I8, 7)])
def test_all_partitions_equal_the_full_scan(cases, dtype, dim):
    c = cases(dtype, dim)
    nq, k = 9, 10
    fid, fsc = c.ctx.search_batch(c.queries[:nq], k)
    probe = np.tile(np.arange(NPARTS, dtype=np.uint32), (nq, 1))
    ids, sc, counts = c.ctx.search_partitions(c.queries[:nq], k, probe)
    assert np.array_equal(ids, fid) and np.array_equal(sc.view(np.uint32), fsc.view(np.uint32)) and (counts == k).all()
    c.ctx.set_centroids(_centroids(c))
    ids, sc, counts, pr = c.ctx.search_ivf(c.queries[:nq], k, NPARTS, want_probe=True)
    assert np.array_equal(ids, fid) and np.array_equal(sc.view(np.uint32), fsc.view(np.uint32)) and (counts == k).all()
    assert all(sorted(r) == list(range(NPARTS)) for r in pr.tolist())


@pytest.mark.parametrize("dtype,dim", [(F16, 100), (F32, 384)])
def test_ivf(cases, oracle, dtype, dim):
    c = cases(dtype, dim)
    cen = _centroids(c)
    c.ctx.set_centroids(cen)
    nq, k = 9, 10
    ids, sc, counts, pr = c.ctx.search_ivf(c.queries[:nq], k, 3, want_probe=True)
    eprobe, _ = oracle.flat_topk(cen, po.DT_F32, c.queries[:nq], 3)
    assert np.array_equal(pr.astype(np.uint64), eprobe)
    pid, psc, pcnt = c.check(pr, k)
    assert np.array_equal(ids, pid) and np.array_equal(sc.view(np.uint32), psc.view(np.uint32)) and np.array_equal(counts, pcnt)
    # nprobe > nparts clamps to nparts
    ids, sc, counts, pr = c.ctx.search_ivf(c.queries[:nq], k, NPARTS + 5, want_probe=True)
    aid, asc, acnt = c.ctx.search_ivf(c.queries[:nq], k, NPARTS)
    assert np.array_equal(ids, aid) and np.array_equal(sc.view(np.uint32), asc.view(np.uint32)) and np.array_equal(counts, acnt)
    assert (pr[:, NPARTS:] == SENT).all() and all(sorted(r[:NPARTS]) == list(range(NPARTS)) for r in pr.tolist())


def _raw_search(ctx, queries, nq, k, probe, nprobe, ids, sc, counts):
    return ctx.lib.nvdb_hip_search_partitions(ctx.h, queries.ctypes.data, nq, k, probe.ctypes.data if probe is not None else None, nprobe,
                                              ids.ctypes.data, sc.ctypes.data, counts.ctypes.data, None)


def test_conventions(cases):
    lib = nvdb_amd.load_library()
    dim = 100
    q = nvdb_amd.synth_rows_f32(SEED + 1, 0, 4, dim)
    probe = np.array([[1, 2]] * 4, dtype=np.uint32)
    ids = np.full((4, 64), 7, dtype=np.uint64)
    sc = np.full((4, 64), 7.0, dtype=np.float32)
    cnt = np.full(4, 7, dtype=np.uint32)
    ctx = nvdb_amd.HipContext(0)
    try:
        # no corpus resident
        assert lib.nvdb_hip_set_partitions(ctx.h, OFFSETS.ctypes.data, NPARTS) == 4
        assert lib.nvdb_hip_set_centroids(ctx.h, q.ctypes.data) == 4
        assert _raw_search(ctx, q, 4, 10, probe, 2, ids, sc, cnt) == 4
        assert lib.nvdb_hip_search_ivf(ctx.h, q.ctypes.data, 4, 10, 2, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None, None) == 4
        assert "Empty base" in lib.nvdb_hip_last_error(ctx.h).decode()
        base, _ = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, F16)
        ctx.upload_corpus(base, F16, None, ROW_BASE)
        # no partitions set
        assert _raw_search(ctx, q, 4, 10, probe, 2, ids, sc, cnt) == 1
        assert "partition" in lib.nvdb_hip_last_error(ctx.h).decode()
        assert lib.nvdb_hip_set_centroids(ctx.h, q.ctypes.data) == 1
        assert lib.nvdb_hip_search_ivf(ctx.h, q.ctypes.data, 4, 10, 2, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None, None) == 1
        # bad offsets tables
        for bad in ([1, N], [0, N - 1], [0, 10, 5, N], [0, N + 1]):
            t = np.array(bad, dtype=np.uint64)
            assert lib.nvdb_hip_set_partitions(ctx.h, t.ctypes.data, len(bad) - 1) == 1, bad
        assert lib.nvdb_hip_set_partitions(ctx.h, None, 3) == 1
        assert lib.nvdb_hip_set_partitions(ctx.h, OFFSETS.ctypes.data, 0) == 1
        assert _raw_search(ctx, q, 4, 10, probe, 2, ids, sc, cnt) == 1          # a refused table sets nothing
        ctx.set_partitions(OFFSETS)
        # search_ivf without centroids
        assert lib.nvdb_hip_search_ivf(ctx.h, q.ctypes.data, 4, 10, 2, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None, None) == 1
        assert "centroids" in lib.nvdb_hip_last_error(ctx.h).decode()
        # k == 0 / nq == 0: OK, nothing written
        assert _raw_search(ctx, q, 4, 0, probe, 2, ids, sc, cnt) == 0
        assert _raw_search(ctx, q, 0, 10, probe, 2, ids, sc, cnt) == 0
        assert (ids == 7).all() and (sc == 7.0).all() and (cnt == 7).all()
        # k > 64
        assert _raw_search(ctx, q, 4, 65, probe, 2, ids, sc, cnt) == 3
        assert (ids == 7).all()
        # a probe entry >= nparts that is not the sentinel: refused on the host, nothing written
        badp = probe.copy()
        badp[3, 1] = NPARTS
        assert _raw_search(ctx, q, 4, 10, badp, 2, ids, sc, cnt) == 1
        assert (ids == 7).all() and (sc == 7.0).all()
        # nprobe == 0: every count 0, all padding
        assert _raw_search(ctx, q, 4, 10, None, 0, ids, sc, cnt) == 0
        assert (cnt == 0).all() and (ids.ravel()[:40] == U64MAX).all() and np.isneginf(sc.ravel()[:40]).all() and (ids.ravel()[40:] == 7).all()
        # a good call, then a new corpus drops the table (and the centroids)
        gid, gsc, gcnt = ctx.search_partitions(q, 10, probe)
        assert (gcnt == 10).all() and (gid != U64MAX).all()
        ctx.set_centroids(np.zeros((NPARTS, dim), dtype=np.float32))
        ctx.upload_corpus(base, F16, None, ROW_BASE)
        assert _raw_search(ctx, q, 4, 10, probe, 2, ids, sc, cnt) == 1
        assert lib.nvdb_hip_search_ivf(ctx.h, q.ctypes.data, 4, 10, 2, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None, None) == 1
        ctx.set_partitions(OFFSETS)
        assert lib.nvdb_hip_search_ivf(ctx.h, q.ctypes.data, 4, 10, 2, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None, None) == 1   # the centroids went with the table
        rid, rsc, rcnt = ctx.search_partitions(q, 10, probe)
        assert np.array_equal(rid, gid) and np.array_equal(rsc.view(np.uint32), gsc.view(np.uint32))
    finally:
        ctx.close()
    # two consecutive calls with different nq reuse the workspace and stay correct; the timing struct is filled
    c = cases(F16, 100)
    rs = np.random.RandomState(5)
    c.check(rs.randint(0, NPARTS, size=(70, 3)), 10)
    c.check(rs.randint(0, NPARTS, size=(9, 3)), 10)
    c.check(rs.randint(0, NPARTS, size=(33, 2)), 64)
    *_, t = c.ctx.search_partitions(c.queries[:9], 10, rs.randint(0, NPARTS, size=(9, 3)), want_timing=True)
    assert t.kernel_ms > 0 and t.total_ms >= t.kernel_ms and t.K == 10 and t.threads == 64 * t.nwarps > 0
    st = c.ctx.stats()
    assert st["path"] == 4 and st["rows_scanned"] > 0


def test_size_2m_rows_256_partitions(oracle):
    n, dim, nparts, nq, nprobe, k = 2_000_000, 768, 256, 256, 8, 10
    ctx = nvdb_amd.HipContext(0)
    try:
        ctx.generate_corpus(SEED, n, dim, F16, ROW_BASE)
        offsets = (np.arange(nparts + 1, dtype=np.uint64) * n) // nparts
        ctx.set_partitions(offsets)
        queries = nvdb_amd.synth_rows_f32(SEED + 2, 0, nq, dim)
        rs = np.random.RandomState(11)
        probe = rs.randint(0, nparts, size=(nq, nprobe)).astype(np.uint32)
        ids, sc, counts = ctx.search_partitions(queries, k, probe)
        assert (counts == k).all()
        for q in rs.choice(nq, 8, replace=False):
            rows, scores = [], []
            for p in sorted(set(probe[q].tolist())):
                lo, hi = int(offsets[p]), int(offsets[p + 1])
                block, _ = ctx.download_rows(lo, hi - lo)
                rows.append(np.arange(lo, hi, dtype=np.int64))
                scores.append(oracle.scores(block, po.DT_F16, queries[q]))
            rows, scores = np.concatenate(rows), np.concatenate(scores)
            order = np.lexsort((rows, -scores))[:k]
            assert np.array_equal(ids[q], rows[order].astype(np.uint64) + ROW_BASE), q
            assert np.array_equal(sc[q].view(np.uint32), scores[order].view(np.uint32)), q
    finally:
        ctx.close()
