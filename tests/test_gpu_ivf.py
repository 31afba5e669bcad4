"""IVF-Flat build on the GPU (nvdb_hip_assign_rows / train_centroids / ivf_build / ivf_search) against the oracle.

Assignment: per row, the first maximum of the oracle's scores of the centroid table (an f32 corpus) for the row taken as an f32
query.  Search: the oracle's scores of the ORIGINAL corpus restricted to the rows whose assignment is probed, ordered
(score desc, partition, original row) -- ids and score BITS must be equal.  Training: numpy fp64 restatements."""
import numpy as np
import pytest

import nvdb_amd
import pyoracle as po

pytestmark = pytest.mark.gpu

F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8
N, ROW_BASE, SEED, NPARTS = 2113, 1_000_003, 20250611, 37        # two full assignment batches of 1024 rows plus 65
DUP_A, DUP_B, ZERO = 5, 20, 30                                     # centroid 20 repeats centroid 5; centroid 30 is all zero
U64MAX = np.iinfo(np.uint64).max
SENT = 0xFFFFFFFF
NQ_MAX = 70
DIMS = (1, 7, 100, 384, 768)


def row_as_f32(base, dtype, scales):
    """The row as an f32 query: f32 itself, f16 widened exactly, int8 float(x) * scale with one rounding."""
    if dtype == F32:
        return np.ascontiguousarray(base, dtype=np.float32)
    if dtype == F16:
        return base.view(np.float16).astype(np.float32)
    return base.astype(np.float32) * scales.astype(np.float32)[:, None]


def unit_rows(rs, n, dim):
    v = rs.standard_normal((n, dim))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def centroid_table(dim):
    cen = unit_rows(np.random.RandomState(100 + dim), NPARTS, dim)
    cen[DUP_B] = cen[DUP_A]
    cen[ZERO] = 0.0
    return cen


def oracle_assign(orc, cen, rows_f32):
    return np.array([int(np.argmax(orc.scores(cen, po.DT_F32, r))) for r in rows_f32], dtype=np.uint32)   # argmax: the first maximum


class Case:
    """One source corpus (dtype, dim) resident with ROW_BASE, its centroid table, the oracle's assignment and -- lazily -- the index."""

    def __init__(self, orc, dtype, dim):
        self.orc, self.dtype, self.dim = orc, dtype, dim
        self.base, self.scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
        self.rows_f32 = row_as_f32(self.base, dtype, self.scales)
        self.cen = centroid_table(dim)
        self.queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ_MAX, dim)
        self.src = nvdb_amd.HipContext(0)
        self.src.upload_corpus(self.base, dtype, self.scales, ROW_BASE)
        self.assign = oracle_assign(orc, self.cen, self.rows_f32)
        self._ivf = None
        self._scores, self._cscores = {}, {}

    def ivf(self):
        if self._ivf is None:
            self.flat_before = self.src.search_batch(self.queries[:9], 10)
            self._ivf = nvdb_amd.IvfIndex(self.src, self.cen)
        return self._ivf

    def scores(self, q):
        if q not in self._scores:
            self._scores[q] = self.orc.scores(self.base, self.dtype, self.queries[q], self.scales)
            self._cscores[q] = self.orc.scores(self.cen, po.DT_F32, self.queries[q])
        return self._scores[q], self._cscores[q]

    def expect(self, q, k, nprobe):
        s, cs = self.scores(q)
        np_eff = min(nprobe, NPARTS)
        probes = np.lexsort((np.arange(NPARTS), -cs))[:np_eff]
        rows = np.flatnonzero(np.isin(self.assign, probes))
        order = np.lexsort((rows, self.assign[rows], -s[rows]))[:k]
        ids = np.full(k, U64MAX, dtype=np.uint64)
        sc = np.full(k, -np.inf, dtype=np.float32)
        ids[:len(order)] = rows[order].astype(np.uint64) + ROW_BASE
        sc[:len(order)] = s[rows[order]]
        return ids, sc, min(k, len(rows)), probes.astype(np.uint32)

    def close(self):
        if self._ivf is not None:
            self._ivf.close()
        self.src.close()


@pytest.fixture(scope="module")
def cases(oracle):
    made = {}

    def get(dtype, dim):
        if (dtype, dim) not in made:
            made[(dtype, dim)] = Case(oracle, dtype, dim)
        return made[(dtype, dim)]
    yield get
    for c in made.values():
        c.close()


ALL = [(dt, d) for dt in (F32, F16, I8) for d in DIMS]


@pytest.mark.parametrize("dtype,dim", ALL)
def test_assignment_parity(cases, dtype, dim):
    c = cases(dtype, dim)
    got = c.src.assign_rows(c.cen)
    assert got.dtype == np.uint32 and got.shape == (N,)
    bad = np.flatnonzero(got != c.assign)
    assert bad.size == 0, (bad[:10], got[bad[:10]], c.assign[bad[:10]])
    assert not (got == DUP_B).any()                               # the tie with its duplicate goes to the lower number
    sub = c.src.assign_rows(c.cen, row0=1000, nrows=90)           # straddles the first batch boundary
    assert np.array_equal(sub, c.assign[1000:1090])
    assert c.src.assign_rows(c.cen, row0=17, nrows=0).size == 0
    assert c.src.assign_rows(c.cen, row0=N, nrows=0).size == 0


@pytest.mark.parametrize("dtype,dim", ALL)
def test_build_layout(cases, dtype, dim):
    c = cases(dtype, dim)
    ivf = c.ivf()
    info = ivf.info()
    perm = np.argsort(c.assign, kind="stable").astype(np.uint32)
    assert info["n"] == N and info["nparts"] == NPARTS
    assert np.array_equal(info["offsets"], np.concatenate([[0], np.cumsum(np.bincount(c.assign, minlength=NPARTS))]).astype(np.uint64))
    assert np.array_equal(info["perm"], perm)
    rows, scales = ivf.ctx.download_rows(0, N)
    assert rows.tobytes() == c.base[perm].tobytes()
    if dtype == I8:
        assert scales.tobytes() == c.scales[perm].tobytes()
    ci = ivf.ctx.corpus_info()
    assert ci["n"] == N and ci["dim"] == dim and ci["dtype"] == dtype and ci["row_base"] == 0
    # the source is as it was
    srows, sscales = c.src.download_rows(0, N)
    assert srows.tobytes() == c.base.tobytes() and (dtype != I8 or sscales.tobytes() == c.scales.tobytes())
    assert c.src.corpus_info()["row_base"] == ROW_BASE
    ids, sc = c.src.search_batch(c.queries[:9], 10)
    assert np.array_equal(ids, c.flat_before[0]) and np.array_equal(sc.view(np.uint32), c.flat_before[1].view(np.uint32))


# per dtype one dim whose probe scan stages the rows through LDS and one that reads them directly (tests/test_gpu_partitions.py)
SEARCH = [(F16, 768), (F16, 100), (F32, 384), (F32, 768), (I8, 384), (I8, 7)]


@pytest.mark.parametrize("nq", [9, 70])
@pytest.mark.parametrize("dtype,dim", SEARCH)
def test_search_parity(cases, dtype, dim, nq):
    c = cases(dtype, dim)
    ivf = c.ivf()
    for k in (1, 10, 64):
        for nprobe in (1, 3, NPARTS):
            ids, sc, counts, probe = ivf.search(c.queries[:nq], k, nprobe, want_probe=True)
            for q in range(nq):
                eid, esc, ecnt, eprobe = c.expect(q, k, nprobe)
                where = (k, nprobe, q)
                assert np.array_equal(probe[q], eprobe), (where, probe[q], eprobe)
                assert counts[q] == ecnt, (where, counts[q], ecnt)
                assert np.array_equal(ids[q], eid), (where, ids[q], eid)
                assert np.array_equal(sc[q].view(np.uint32), esc.view(np.uint32)), (where, sc[q], esc)
                assert (ids[q, ecnt:] == U64MAX).all() and np.isneginf(sc[q, ecnt:]).all()


def test_equal_scores_are_ordered_by_partition_then_original_id(oracle):
    """200 rows that score EQUALLY for the query: copies of one row whose last coordinate -- where the query is 0 -- is +0.5 on the
    even copies and -0.5 on the odd ones; the two centroids +-e_last put half of the copies on each side."""
    n, dim, first, copies = 700, 100, 150, 200
    base32 = nvdb_amd.synth_rows_f32(SEED + 7, 0, n, dim).copy()
    base32[:, -1] = np.where(np.arange(n) % 3 == 0, 0.25, -0.25)            # every other row sits clearly on one side too
    v = base32[first].copy()
    v[-1] = 0.0
    dup = np.arange(first, first + copies)
    base32[dup] = v
    base32[dup, -1] = np.where((dup - first) % 2 == 0, 0.5, -0.5)
    base = nvdb_amd.f32_to_f16(base32)
    query = base[first].view(np.float16).astype(np.float32)[None, :].copy()
    query[0, -1] = 0.0
    cen = np.zeros((2, dim), dtype=np.float32)
    cen[0, -1], cen[1, -1] = 1.0, -1.0
    s = oracle.scores(base, po.DT_F16, query[0])
    assert len(set(s[dup].view(np.uint32).tolist())) == 1 and (np.delete(s, dup) < s[first]).all()
    src = nvdb_amd.HipContext(0)
    try:
        src.upload_corpus(base, F16, None, ROW_BASE)
        assign = src.assign_rows(cen)
        assert (assign[dup] == (dup - first) % 2).all()
        ivf = nvdb_amd.IvfIndex(src, cen)
        try:
            ids, sc, counts = ivf.search(query, 64, 2)
            even = dup[(dup - first) % 2 == 0]                               # partition 0's copies come first: 100 of them, 64 fit
            assert ids[0].tolist() == (even[:64] + ROW_BASE).tolist()
            assert (sc[0].view(np.uint32) == s[first:first + 1].view(np.uint32)).all() and counts[0] == 64
            ids, sc, counts = ivf.search(query, 64, 1, want_probe=False)     # one list only (whichever ranks first): its copies, ascending
            got = ids[0].astype(np.int64) - ROW_BASE
            assert (np.diff(got) > 0).all() and len(set(((got - first) % 2).tolist())) == 1 and np.isin(got, dup).all()
        finally:
            ivf.close()
        # 30 copies on side 0, 170 on side 1: the cut falls inside partition 1
        side = np.where(dup - first < 30, 0.5, -0.5)
        base32[dup, -1] = side
        base = nvdb_amd.f32_to_f16(base32)
        src.upload_corpus(base, F16, None, ROW_BASE)
        ivf = nvdb_amd.IvfIndex(src, cen)
        try:
            ids, sc, counts = ivf.search(query, 64, 2)
            assert ids[0].tolist() == (dup[:64] + ROW_BASE).tolist() and len(set(sc[0].view(np.uint32).tolist())) == 1
            ids, sc, counts = ivf.search(query, 40, 2)
            assert ids[0].tolist() == (dup[:40] + ROW_BASE).tolist()
        finally:
            ivf.close()
    finally:
        src.close()


@pytest.mark.parametrize("dtype,dim", [(F16, 768), (F32, 7), (I8, 100)])
def test_full_probe_equals_the_flat_search(cases, dtype, dim):
    c = cases(dtype, dim)
    nq, k = 9, 10
    for q in range(nq):                                                       # precondition: no two equal scores among the best k + 1
        top = np.sort(c.scores(q)[0])[::-1][:k + 1]
        assert len(set(top.view(np.uint32).tolist())) == k + 1, q
    fid, fsc = c.src.search_batch(c.queries[:nq], k)
    ids, sc, counts = c.ivf().search(c.queries[:nq], k, NPARTS)
    assert np.array_equal(ids, fid) and np.array_equal(sc.view(np.uint32), fsc.view(np.uint32)) and (counts == k).all()


# ------------------------------------------------------------------------------------------------------------------ training
TN, TPARTS = 4000, 16


class TrainCase:
    def __init__(self, dtype, dim):
        self.dtype, self.dim = dtype, dim
        self.base, self.scales = nvdb_amd.synth_corpus(SEED + 3, 0, TN, dim, dtype)
        self.rows64 = row_as_f32(self.base, dtype, self.scales).astype(np.float64)
        self.init = unit_rows(np.random.RandomState(dim + dtype), TPARTS, dim)
        self.ctx = nvdb_amd.HipContext(0)
        self.ctx.upload_corpus(self.base, dtype, self.scales, 0)

    def step(self, cen, rows):
        """One update in numpy fp64 from `cen` over the training rows `rows`: membership from assign_rows (pinned by the parity tests)."""
        assign = self.ctx.assign_rows(cen)[rows]
        out = np.array(cen, dtype=np.float32, copy=True)
        for p in range(len(out)):
            members = self.rows64[rows[assign == p]]
            if len(members) == 0:
                continue
            mean = members.mean(axis=0, dtype=np.float64)
            norm = np.sqrt(np.sum(mean * mean))
            if norm > 0 and np.isfinite(norm):
                out[p] = (mean / norm).astype(np.float32)
        return out, assign

    def objective(self, cen):
        return float(np.mean(np.max(self.rows64 @ cen.astype(np.float64).T, axis=1)))


@pytest.fixture(scope="module")
def train_cases():
    made = {}

    def get(dtype, dim):
        if (dtype, dim) not in made:
            made[(dtype, dim)] = TrainCase(dtype, dim)
        return made[(dtype, dim)]
    yield get
    for t in made.values():
        t.ctx.close()


def ulp_distance(a, b):
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


TRAIN = [(F16, 32), (F16, 768), (I8, 32), (I8, 768)]


@pytest.mark.parametrize("dtype,dim", TRAIN)
def test_training_is_reproducible_and_seeded(train_cases, dtype, dim):
    t = train_cases(dtype, dim)
    a = t.ctx.train_centroids(TPARTS, 2, seed=5)
    b = t.ctx.train_centroids(TPARTS, 2, seed=5)
    assert a.tobytes() == b.tobytes()
    assert t.ctx.train_centroids(TPARTS, 2, seed=6).tobytes() != a.tobytes()
    assert t.ctx.train_centroids(TPARTS, 0, seed=6).tobytes() != t.ctx.train_centroids(TPARTS, 0, seed=5).tobytes()


@pytest.mark.parametrize("dtype,dim", TRAIN)
def test_training_start_is_distinct_unit_rows(train_cases, dtype, dim):
    t = train_cases(dtype, dim)
    cen = t.ctx.train_centroids(TPARTS, 0, seed=5)
    image = (t.rows64 / np.sqrt(np.sum(t.rows64 * t.rows64, axis=1, keepdims=True))).astype(np.float32)
    where = {}
    for r in range(TN):
        where.setdefault(image[r].tobytes(), r)
    rows = [where.get(cen[p].tobytes()) for p in range(TPARTS)]
    assert None not in rows, rows
    assert len(set(rows)) == TPARTS, rows
    norms = np.sqrt(np.sum(cen.astype(np.float64) ** 2, axis=1))
    assert (np.abs(norms - 1.0) <= 2.0 ** -23).all(), norms


@pytest.mark.parametrize("dtype,dim", TRAIN)
def test_training_step_matches_fp64(train_cases, dtype, dim):
    """One step from a given start.  Tolerance: 1 f32 ulp per component -- the fp64 accumulation error is far below half an f32 ulp,
    so only the double rounding can move a value, and by one step at most."""
    t = train_cases(dtype, dim)
    got = t.ctx.train_centroids(TPARTS, 1, seed=0, init=t.init)
    want, assign = t.step(t.init, np.arange(TN))
    assert len(np.unique(assign)) == TPARTS                                   # every centroid has members here
    d = ulp_distance(got, want)
    print(f"one step, dtype {dtype} dim {dim}: max ulp distance {d.max()}, components off by one {int((d == 1).sum())} of {d.size}")
    assert d.max() <= 1, (d.max(), np.argwhere(d > 1)[:5])
    # the empty-cluster rule: centroid 11 repeats centroid 3, every tie goes to 3, 11 keeps its bits
    init = t.init.copy()
    init[11] = init[3]
    got = t.ctx.train_centroids(TPARTS, 1, seed=0, init=init)
    want, assign = t.step(init, np.arange(TN))
    assert not (assign == 11).any()
    assert got[11].tobytes() == init[11].tobytes()
    assert ulp_distance(got, want).max() <= 1
    # a subsample: rows floor(i * 4000 / 1000)
    rows = (np.arange(1000) * TN) // 1000
    got = t.ctx.train_centroids(TPARTS, 1, seed=0, max_train_rows=1000, init=t.init)
    want, _ = t.step(t.init, rows)
    d = ulp_distance(got, want)
    print(f"one step on 1000 rows: max ulp distance {d.max()}")
    assert d.max() <= 1, (d.max(), np.argwhere(d > 1)[:5])
    assert got.tobytes() != t.ctx.train_centroids(TPARTS, 1, seed=0, init=t.init).tobytes()
    # three centroids: lists of more than 512 members, summed in several chunks
    got = t.ctx.train_centroids(3, 1, seed=0, init=t.init[:3])
    want, assign = t.step(t.init[:3], np.arange(TN))
    assert np.bincount(assign, minlength=3).min() > 512
    d = ulp_distance(got, want)
    print(f"one step, three centroids: max ulp distance {d.max()}")
    assert d.max() <= 1, (d.max(), np.argwhere(d > 1)[:5])


@pytest.mark.parametrize("dtype,dim", TRAIN)
def test_training_objective_does_not_decrease(train_cases, dtype, dim):
    """O(t) = mean over the rows of the dot product with the best centroid (numpy fp64).  Exact arithmetic makes it monotone; 1e-6
    covers the f32 rounding of the unit centroids."""
    t = train_cases(dtype, dim)
    obj = [t.objective(t.ctx.train_centroids(TPARTS, it, seed=5)) for it in (0, 1, 2, 4)]
    print(f"objective, dtype {dtype} dim {dim}: {obj}")
    for prev, cur in zip(obj, obj[1:]):
        assert cur >= prev - 1e-6, obj


# ------------------------------------------------------------------------------------------------------------------ conventions
def test_argument_rules(cases):
    c = cases(F16, 100)
    lib = c.src.lib
    ivf = c.ivf()
    out = np.full(8, 7, dtype=np.uint32)
    cen_out = np.full((N + 1, 100), 7.0, dtype=np.float32)
    # more centroids than training rows
    assert lib.nvdb_hip_train_centroids(c.src.h, N + 1, 1, 0, 0, None, cen_out.ctypes.data) == 1
    assert lib.nvdb_hip_train_centroids(c.src.h, 16, 1, 0, 10, None, cen_out.ctypes.data) == 1
    assert lib.nvdb_hip_train_centroids(c.src.h, 0, 1, 0, 0, None, cen_out.ctypes.data) == 1
    assert (cen_out == 7.0).all()
    # rows out of range, bad tables
    assert lib.nvdb_hip_assign_rows(c.src.h, c.cen.ctypes.data, NPARTS, N - 4, 5, out.ctypes.data) == 1
    assert lib.nvdb_hip_assign_rows(c.src.h, c.cen.ctypes.data, NPARTS, N + 1, 0, out.ctypes.data) == 1
    assert lib.nvdb_hip_assign_rows(c.src.h, None, NPARTS, 0, 5, out.ctypes.data) == 1
    assert lib.nvdb_hip_assign_rows(c.src.h, c.cen.ctypes.data, 0, 0, 5, out.ctypes.data) == 1
    assert lib.nvdb_hip_assign_rows(c.src.h, c.cen.ctypes.data, SENT, 0, 5, out.ctypes.data) == 1
    assert lib.nvdb_hip_assign_rows(c.src.h, c.cen.ctypes.data, NPARTS, 0, 5, None) == 1
    assert (out == 7).all()
    assert lib.nvdb_hip_assign_rows(c.src.h, c.cen.ctypes.data, NPARTS, N - 5, 5, out.ctypes.data) == 0
    assert np.array_equal(out[:5], c.assign[N - 5:]) and (out[5:] == 7).all()
    # search conventions are the probe search's
    q = c.queries[:4]
    ids = np.full((4, 65), 7, dtype=np.uint64)
    sc = np.full((4, 65), 7.0, dtype=np.float32)
    cnt = np.full(4, 7, dtype=np.uint32)
    raw = lambda k, nprobe: lib.nvdb_hip_ivf_search(ivf.h, q.ctypes.data, 4, k, nprobe, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None, None)  # noqa: E731
    assert raw(65, 3) == 3 and (ids == 7).all()
    assert raw(0, 3) == 0 and (ids == 7).all() and (cnt == 7).all()
    assert raw(10, 0) == 0
    assert (cnt == 0).all() and (ids.ravel()[:40] == U64MAX).all() and np.isneginf(sc.ravel()[:40]).all() and (ids.ravel()[40:] == 7).all()
    pid, psc, pcnt = ivf.search(q, 10, 0)
    assert (pid == U64MAX).all() and np.isneginf(psc).all() and (pcnt == 0).all()
    # no corpus resident
    empty = nvdb_amd.HipContext(0)
    try:
        with pytest.raises(nvdb_amd.NvdbError) as e:
            nvdb_amd.IvfIndex(empty, c.cen)
        assert e.value.status == 4 and "Empty base" in str(e.value)
        assert lib.nvdb_hip_assign_rows(empty.h, c.cen.ctypes.data, NPARTS, 0, 0, out.ctypes.data) == 4
        assert lib.nvdb_hip_train_centroids(empty.h, 4, 1, 0, 0, None, cen_out.ctypes.data) == 4
    finally:
        empty.close()


def test_source_outlives_the_index_and_the_index_the_source(oracle):
    dim = 100
    base, _ = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, F16)
    cen = centroid_table(dim)
    q = nvdb_amd.synth_rows_f32(SEED + 1, 0, 9, dim)
    src = nvdb_amd.HipContext(0)
    try:
        src.upload_corpus(base, F16, None, ROW_BASE)
        before = src.search_batch(q, 10)
        ivf = nvdb_amd.IvfIndex(src, cen)
        first = ivf.search(q, 10, 3)
        ivf.close()
        after = src.search_batch(q, 10)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
        ivf = nvdb_amd.IvfIndex(src, cen)
    finally:
        src.close()                                                           # the HBM of the source goes back; the index stands alone
    try:
        again = ivf.search(q, 10, 3)
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes()
        assert (again[0][again[0] != U64MAX] >= ROW_BASE).all()
    finally:
        ivf.close()


def test_non_finite_rows_are_survived():
    """Data only: one NaN row and one Inf row.  Every call returns, every assignment names a centroid."""
    n, dim, nparts = 300, 100, 8
    base = nvdb_amd.synth_rows_f32(SEED + 9, 0, n, dim).copy()
    base[5, :] = np.nan
    base[9, 3] = np.inf
    cen = unit_rows(np.random.RandomState(3), nparts, dim)
    q = nvdb_amd.synth_rows_f32(SEED + 1, 0, 4, dim)
    src = nvdb_amd.HipContext(0)
    try:
        src.upload_corpus(base, F32, None, 0)
        assign = src.assign_rows(cen)
        assert assign.shape == (n,) and (assign < nparts).all()
        ivf = nvdb_amd.IvfIndex(src, cen)
        try:
            info = ivf.info()
            assert sorted(info["perm"].tolist()) == list(range(n)) and info["offsets"][-1] == n
            ids, sc, counts = ivf.search(q, 10, 3)
            assert ids.shape == (4, 10) and (counts <= 10).all()
        finally:
            ivf.close()
    finally:
        src.close()
