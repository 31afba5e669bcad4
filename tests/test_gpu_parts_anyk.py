"""Probe search for any k (nvdb_hip_search_partitions_anyk / _ivf_anyk, nvdb_hip_ivf_search_anyk) against the oracle.

The checker is tests/test_gpu_partitions.py's: the oracle's score vector per query, restricted to the rows of the probed union that
are live in the query's plane, np.lexsort((rows, -s))[:k].  Ids, score BITS and counts must be equal -- where equal scores meet both
sides order by id, so there is no set-wise slack.  The corpus shape is that file's, the planes tests/test_gpu_row_masks.py's."""
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
F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8
# around the wavefront lists, a power of two and one more, PART_SEG_ROWS and one more, the in-LDS sort's edge, more than N
KS = [65, 100, 128, 129, 1000, 2048, 2049, 8192, 8193, 30001]


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


def union_rows(probe_row, live=None, offsets=OFFSETS):
    rows = np.concatenate([np.arange(offsets[p], offsets[p + 1], dtype=np.int64) for p in sorted(set(int(p) for p in probe_row if p != SENT))] +
                          [np.empty(0, np.int64)])
    return rows if live is None else rows[live[rows]]


def expect_rows(s, rows, k, row_base=ROW_BASE, tie=None):
    """The k best of `rows` under scores s[rows]: (ids [k], scores [k], count); ties by row (or by (tie[row], row))."""
    sr = s[rows]
    order = np.lexsort((rows, -sr) if tie is None else (rows, tie[rows], -sr))[:k]
    ids = np.full(k, U64MAX, dtype=np.uint64)
    sc = np.full(k, -np.inf, dtype=np.float32)
    ids[:len(order)] = rows[order].astype(np.uint64) + np.uint64(row_base)
    sc[:len(order)] = sr[order]
    return ids, sc, min(k, len(rows))


def assert_query(got, want, what):
    (gi, gs, gc), (wi, ws, wc) = got, want
    assert gc == wc, (what, "count", gc, wc)
    bad = np.flatnonzero(gi != wi)
    assert bad.size == 0, (what, "ids", bad[:5], gi[bad[:5]], wi[bad[:5]])
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (what, "score bits")


class Case:
    """One resident corpus (dtype, dim) with the partition table, the planes, queries and lazily computed oracle scores."""

    def __init__(self, orc, dtype, dim, base=None, scales=None, queries=None, planes=PLANES):
        self.orc, self.dtype, self.dim = orc, dtype, dim
        if base is None:
            base, scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
        self.base, self.scales = base, scales
        self.queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ_MAX, dim) if queries is None else queries
        self.ctx = nvdb_amd.HipContext(0)
        self.ctx.upload_corpus(self.base, dtype, self.scales, ROW_BASE)
        self.ctx.set_partitions(OFFSETS)
        if planes is not None:
            self.ctx.set_row_masks(planes)
        self._scores = {}

    def scores(self, q):
        if q not in self._scores:
            self._scores[q] = self.orc.scores(self.base, self.dtype, self.queries[q], self.scales)
        return self._scores[q]

    def check(self, probe, ks, mask_of=None, masked=None, planes=PLANES, what=""):
        """One call per k of `ks` over the same probe table; every query against the oracle; the statistics of the k > 64 calls."""
        probe = np.asarray(probe, dtype=np.uint32)
        nq = probe.shape[0]
        is_masked = (mask_of is not None) if masked is None else masked
        rows = []
        for q in range(nq):
            m = SENT if not is_masked else 0 if mask_of is None else int(mask_of[q])
            rows.append(union_rows(probe[q], None if m == SENT else planes[m]))
        out = None
        for k in ([ks] if np.isscalar(ks) else ks):
            out = ids, sc, counts = self.ctx.search_partitions_anyk(self.queries[:nq], k, probe, mask_of, masked)
            assert ids.shape == (nq, k) and sc.shape == (nq, k) and counts.shape == (nq,)
            st = self.ctx.stats()
            for q in range(nq):
                assert_query((ids[q], sc[q], counts[q]), expect_rows(self.scores(q), rows[q], k), f"{what} k {k} query {q}")
            if k > 64 and probe.shape[1] > 0:
                assert st["path"] == 8 and st["candidates"] == sum(len(r) for r in rows), (k, st)
        return out


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


def big_probe(nq, nprobe, seed):
    """Random probes whose first column is the 20000-row partition: the union exceeds k at the large values."""
    probe = np.random.RandomState(seed).randint(0, NPARTS, size=(nq, nprobe)).astype(np.uint32)
    probe[:, 0] = BIG
    return probe


# rows staged through LDS (f16 768), direct aligned (f32 768: a tile does not fit the LDS), direct unaligned (i8 100)
@pytest.mark.parametrize("nq,nprobe", [(9, 1), (9, 3), (70, 1), (70, 3)])
@pytest.mark.parametrize("dtype,dim", [(F16, 768), (F32, 768), (I8, 100)])
def test_k_grid(cases, dtype, dim, nq, nprobe):
    c = cases(dtype, dim)
    c.check(big_probe(nq, nprobe, 1000 * dtype + dim + nq + nprobe), KS if nq == 9 else [65, 100, 2049, 8193, 30001], what=f"grid {dtype} {dim}")


@pytest.mark.parametrize("dtype,dim", [(F16, 768), (I8, 100)])
def test_k_up_to_64_is_the_twin_byte_for_byte(cases, dtype, dim):
    c = cases(dtype, dim)
    nq = 33
    probe = big_probe(nq, 3, 5)
    probe[1] = [EMPTY, SENT, 1]
    mo = (np.arange(nq) % (NMASKS + 1)).astype(np.uint32)
    mo[mo == NMASKS] = SENT
    for k in (1, 10, 64):
        a = c.ctx.search_partitions_anyk(c.queries[:nq], k, probe)
        b = c.ctx.search_partitions(c.queries[:nq], k, probe)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), k
        a = c.ctx.search_partitions_anyk(c.queries[:nq], k, probe, mo)
        b = c.ctx.search_partitions_masked(c.queries[:nq], k, probe, mo)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), k
        a = c.ctx.search_partitions_anyk(c.queries[:nq], k, probe, masked=True)         # plane 0 for every query
        b = c.ctx.search_partitions_masked(c.queries[:nq], k, probe, None)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), k


def test_unions_around_k(cases):
    c = cases(F16, 768)
    # partitions 1 .. 5 hold 1 / 63 / 64 / 65 / 257 rows
    probe = np.array([[1, 3, SENT],                # 65 rows
                      [2, 4, SENT],                # 128
                      [3, SENT, SENT],             # 64
                      [4, SENT, 4],                # 65, a partition named twice
                      [2, 3, SENT],                # 127
                      [1, 2, 4],                   # 129
                      [1, 2, 3],                   # 128
                      [EMPTY, SENT, SENT],         # the empty partition alone
                      [SENT, SENT, SENT],          # nothing
                      [5, 1, EMPTY]], dtype=np.uint32)   # 258
    for k, want in ((65, [65, 65, 64, 65, 65, 65, 65, 0, 0, 65]), (128, [65, 128, 64, 65, 127, 128, 128, 0, 0, 128]),
                    (129, [65, 128, 64, 65, 127, 129, 128, 0, 0, 129]), (258, [65, 128, 64, 65, 127, 129, 128, 0, 0, 258])):
        ids, sc, counts = c.check(probe, k, what="unions")
        assert counts.tolist() == want
        for q, n in enumerate(want):               # counts and padding, explicitly
            assert (ids[q, :n] != U64MAX).all() and (ids[q, n:] == U64MAX).all() and np.isneginf(sc[q, n:]).all() and np.isfinite(sc[q, :n]).all()
            assert len(set(ids[q, :n].tolist())) == n
    # a sub-batch in which no union holds a row, and nprobe == 0
    ids, sc, counts = c.check(np.array([[EMPTY, SENT], [SENT, SENT]], dtype=np.uint32), 100)
    assert (counts == 0).all() and (ids == U64MAX).all() and np.isneginf(sc).all()
    ids, sc, counts = c.ctx.search_partitions_anyk(c.queries[:4], 100, np.zeros((4, 0), dtype=np.uint32))
    assert (counts == 0).all() and (ids == U64MAX).all() and np.isneginf(sc).all()


def test_built_ties(oracle):
    """Tie groups that straddle the k-th place: a radix pass that loses a member, or a cut at the k-th key that takes the wrong
    ones, shows here first.  Query 0's 50th best row of the union is copied over 199 rows -- 70 inside one segment, 70
    spread over every segment of the big partition, 59 in two other partitions -- so the group starts at rank 50 of the
    union at the latest and ends beyond rank 200.  Partition 5 becomes 257 copies of one row (the selection rests on the position alone); partition 4 and 30 rows of the
    last partition become zero rows (scores +-0)."""
    dim = 384
    base, _ = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, F16)
    base = base.copy()
    queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ_MAX, dim)
    big, last, p5, p4 = int(OFFSETS[BIG]), int(OFFSETS[7]), int(OFFSETS[5]), int(OFFSETS[4])
    s0 = oracle.scores(base, po.DT_F16, queries[0])
    u = union_rows([BIG, 7, 3])
    src = int(u[np.argsort(-s0[u], kind="stable")[49]])
    group = np.concatenate([big + 300 + np.arange(70), big + 137 + 283 * np.arange(70), p5 - 65 - 64 + np.arange(29), last + 11 + 7 * np.arange(30)])
    group = group[group != src]
    base[group] = base[src]
    base[p5:p5 + 257] = base[p5 + 3]
    base[p4:p4 + 65] = 0
    base[last + 1000:last + 1030] = 0
    c = Case(oracle, F16, dim, base=base, queries=queries, planes=None)
    try:
        members = np.sort(np.concatenate([group, [src]]))
        probe = np.array([[BIG, 7, 3], [BIG, 7, 3]], dtype=np.uint32)       # (3: the 64-row partition holds 29 members)
        for k in (65, 100, 150):
            ids, sc, counts = c.check(probe, k, what="tie group")
            tied = np.flatnonzero(sc[0] == s0[src])
            assert tied.size >= k - 60 and tied[-1] == k - 1, (k, tied.size)     # the group reaches the cut
            got = ids[0, tied].astype(np.int64) - ROW_BASE
            assert np.array_equal(got, members[:tied.size]), k                  # the lowest ids win, in order
        c.check(np.array([[5], [5]], dtype=np.uint32), [65, 100, 256, 257, 300], what="all identical")
        ids, sc, counts = c.check(np.array([[5, 4, 3, 7]], dtype=np.uint32), [65, 100, 129, 386, 9000], what="zero rows")
        assert (sc[0] == 0).sum() >= 95
    finally:
        c.ctx.close()


def test_masked(cases, oracle):
    c = cases(F16, 768)
    nq = 12
    probe = big_probe(nq, 2, 9)
    probe[3] = [1, 2]                              # planes 2 .. 7 leave at most one live row in any union
    # every plane and "no mask" in turn: fewer than k live rows (none, one), half of the union, all of it
    mo = (np.arange(nq) % (NMASKS + 1)).astype(np.uint32)
    mo[mo == NMASKS] = SENT
    ids, sc, counts = c.check(probe, [65, 100, 8193], mo, what="masked")
    assert counts[NONE_LIVE] == 0 and (counts[2:8] <= 1).all() and counts[ALL_LIVE] == 8193
    # masked == 0 with planes resident equals the unmasked result; mask_of is ignored
    a = c.ctx.search_partitions_anyk(c.queries[:nq], 100, probe, mo, masked=False)
    b = c.check(probe, 100, what="unmasked under planes")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # planes of this test's own: exactly k = 100 live rows in query 0's union, and one with query 0's 50 best rows dead
    s0 = c.scores(0)
    u0 = union_rows(probe[0])
    exact = np.ones(N, bool)
    exact[u0] = False
    exact[u0[::len(u0) // 100][:100]] = True
    best_dead = np.ones(N, bool)
    best_dead[u0[np.argsort(-s0[u0], kind="stable")[:50]]] = False
    planes = np.stack([exact, best_dead])
    try:
        c.ctx.set_row_masks(planes)
        p0 = np.tile(probe[0], (2, 1))
        for k in (99, 100, 101, 150):
            ids, sc, counts = c.check(p0, k, np.array([1, 0], dtype=np.uint32), planes=planes, what="own planes")
            assert counts.tolist() == [k, min(k, 100)]
        assert not np.isin(ids[0], u0[~best_dead[u0]].astype(np.uint64) + ROW_BASE).any()
        # the tombstone path: the current best row goes; the count drops where the union was short
        live = np.ones((1, N), bool)
        c.ctx.set_row_masks(live)
        short = np.array([[1, 2], [BIG, SENT]], dtype=np.uint32)           # 64 rows; 20000 rows
        ids, sc, counts = c.check(short, 100, masked=True, planes=live, what="before the tombstones")
        assert counts.tolist() == [64, 100]
        gone = (ids[:, 0] - ROW_BASE).astype(np.uint64)
        c.ctx.update_row_mask(0, gone, False)
        live[0, gone.astype(np.int64)] = False
        ids2, sc2, counts2 = c.check(short, 100, masked=True, planes=live, what="after the tombstones")
        assert counts2.tolist() == [63, 100] and ids2[0, 0] == ids[0, 1] and ids2[1, 0] == ids[1, 1]
    finally:
        c.ctx.set_row_masks(PLANES)


def test_sub_batch_cut(cases):
    """largek_budget_mb = 1: 65536 candidate entries per launch set; 70 queries on the 20000-row partition run in sub-batches of 3."""
    c = cases(F16, 768)
    probe = np.full((NQ_MAX, 1), BIG, dtype=np.uint32)
    probe[5] = EMPTY
    mo = np.where(np.arange(NQ_MAX) % 3 == 0, HALF, SENT).astype(np.uint32)
    want = {k: c.check(probe, k, mo, what="default budget") for k in (100, 8193)}
    chunks = c.ctx.stats()["chunks"]
    try:
        c.ctx.set_option("largek_budget_mb", 1)
        for k in (100, 8193):
            got = c.ctx.search_partitions_anyk(c.queries, k, probe, mo)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want[k])), k
            st = c.ctx.stats()
            assert st["path"] == 8 and st["chunks"] > chunks, st
    finally:
        c.ctx.set_option("largek_budget_mb", 8192)


def _centroids(c):
    f = c.base.view(np.float16).astype(np.float32)
    cen = np.zeros((NPARTS, c.dim), dtype=np.float32)
    for p in range(NPARTS):
        lo, hi = int(OFFSETS[p]), int(OFFSETS[p + 1])
        if hi > lo:
            cen[p] = f[lo:hi].mean(axis=0, dtype=np.float32)
    return cen


def test_search_ivf_anyk(cases):
    c = cases(F16, 768)
    c.ctx.set_centroids(_centroids(c))
    nq, k = 9, 100
    *_, want_probe = c.ctx.search_ivf(c.queries[:nq], 10, 3, want_probe=True)
    ids, sc, counts, pr = c.ctx.search_ivf_anyk(c.queries[:nq], k, 3, want_probe=True)
    assert np.array_equal(pr, want_probe)
    pid, psc, pcnt = c.check(pr, k, what="ivf")
    assert np.array_equal(ids, pid) and np.array_equal(sc.view(np.uint32), psc.view(np.uint32)) and np.array_equal(counts, pcnt)
    mo = np.full(nq, HALF, dtype=np.uint32)
    ids, sc, counts = c.ctx.search_ivf_anyk(c.queries[:nq], k, 3, mo)
    pid, psc, pcnt = c.check(pr, k, mo, what="ivf masked")
    assert np.array_equal(ids, pid) and np.array_equal(sc.view(np.uint32), psc.view(np.uint32)) and np.array_equal(counts, pcnt)
    # nprobe > nparts clamps; out_probe keeps the caller's row length
    ids, sc, counts, pr = c.ctx.search_ivf_anyk(c.queries[:nq], k, NPARTS + 2, want_probe=True)
    assert (pr[:, NPARTS:] == SENT).all() and (counts == k).all()
    fid, fsc = c.ctx.search_batch(c.queries[:nq], k)
    assert np.array_equal(ids, fid) and np.array_equal(sc.view(np.uint32), fsc.view(np.uint32))


def test_search_ivf_anyk_sub_batch_cut(cases):
    """The IVF form under largek_budget_mb = 1, masked, with the probe table asked for: the coarse step's probes feed several
    sub-batches (each takes its own window of mask_of), the bytes are the default budget's and the table is search_ivf's."""
    c = cases(F16, 768)
    c.ctx.set_centroids(_centroids(c))
    nq, nprobe = 20, 5
    mo = (np.arange(nq) % (NMASKS + 1)).astype(np.uint32)
    mo[mo == NMASKS] = SENT
    *_, want_probe = c.ctx.search_ivf(c.queries[:nq], 10, nprobe, want_probe=True)
    assert sum(len(union_rows(want_probe[q])) for q in range(nq)) > 3 * 65536          # (several sub-batches under a 1 MB budget)
    want = {k: c.ctx.search_ivf_anyk(c.queries[:nq], k, nprobe, mo, want_probe=True) for k in (100, 8193)}
    chunks = c.ctx.stats()["chunks"]
    for k in (100, 8193):                                               # (the default-budget run itself: the oracle's rows over that table)
        pid, psc, pcnt = c.check(want_probe, k, mo, what="ivf, default budget")
        assert all(x.tobytes() == y.tobytes() for x, y in zip(want[k][:3], (pid, psc, pcnt))), k
    try:
        c.ctx.set_option("largek_budget_mb", 1)
        for k in (100, 8193):
            got = c.ctx.search_ivf_anyk(c.queries[:nq], k, nprobe, mo, want_probe=True)
            st = c.ctx.stats()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want[k])), k
            assert np.array_equal(got[3], want_probe), k
            assert st["path"] == 8 and st["chunks"] > chunks, st
    finally:
        c.ctx.set_option("largek_budget_mb", 8192)


IVF_N, IVF_SEED, IVF_NPARTS = 2113, 20250611, 37


def test_ivf_index_search_anyk(oracle):
    """Ids in original rows, equal scores by (list, original row).  Column 0 of every query is zero and rows 40 .. 79 are row 7 with
    column 0 set to +8 or -8: the same score bits for every query, but the copies are assigned to other lists than row 7."""
    n, nq, dim, k = IVF_N, 9, 100, 100
    base, _ = nvdb_amd.synth_corpus(IVF_SEED, ROW_BASE, n, dim, F16)
    base = base.copy()
    base[40:80] = base[7]
    base[40:80:2, 0] = np.float16(8.0).view(np.uint16)
    base[41:80:2, 0] = np.float16(-8.0).view(np.uint16)
    v = np.random.RandomState(100 + dim).standard_normal((IVF_NPARTS, dim))
    cen = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    queries = nvdb_amd.synth_rows_f32(IVF_SEED + 1, 0, nq, dim).copy()
    queries[:, 0] = 0
    queries[0, 1:] = base[7, 1:].view(np.float16).astype(np.float32)    # the copies lead query 0's list
    src = nvdb_amd.HipContext(0)
    src.upload_corpus(base, F16, None, ROW_BASE)
    ivf = nvdb_amd.IvfIndex(src, cen)
    try:
        info = ivf.info()
        assign = np.empty(n, dtype=np.int64)
        for p in range(IVF_NPARTS):
            assign[info["perm"][int(info["offsets"][p]):int(info["offsets"][p + 1])]] = p
        assert len(set(assign[40:80].tolist())) >= 2
        S = [oracle.scores(base, po.DT_F16, q) for q in queries]
        assert (S[0][40:80] == S[0][7]).all()
        planes = make_planes(n)                             # ORIGINAL rows
        ivf.set_row_masks(planes)
        mo = (np.arange(nq) % (NMASKS + 1)).astype(np.uint32)
        mo[mo == NMASKS] = SENT
        mo[0] = HALF
        for nprobe in (5, IVF_NPARTS):
            *_, want_probe = ivf.search(queries, 10, nprobe, want_probe=True)
            rows_all = [np.flatnonzero(np.isin(assign, want_probe[q])) for q in range(nq)]
            ids, sc, counts, pr = ivf.search_anyk(queries, k, nprobe, want_probe=True)
            assert np.array_equal(pr, want_probe)
            for q in range(nq):
                assert_query((ids[q], sc[q], counts[q]), expect_rows(S[q], rows_all[q], k, tie=assign), f"index nprobe {nprobe} query {q}")
            ids, sc, counts = ivf.search_anyk(queries, k, nprobe, mo)
            for q in range(nq):
                rows = rows_all[q] if mo[q] == SENT else rows_all[q][planes[mo[q]][rows_all[q]]]
                assert_query((ids[q], sc[q], counts[q]), expect_rows(S[q], rows, k, tie=assign), f"index masked nprobe {nprobe} query {q}")
        # every list: the 41 equal rows lead query 0's list, by (list, original row) and NOT by original row
        ids, sc, counts = ivf.search_anyk(queries[:1], k, IVF_NPARTS)
        lead = ids[0, :41].astype(np.int64) - ROW_BASE
        assert sorted(lead.tolist()) == [7] + list(range(40, 80)) and lead.tolist() != sorted(lead.tolist())
        assert lead.tolist() == sorted(lead.tolist(), key=lambda r: (assign[r], r))
    finally:
        ivf.close()
        src.close()


def test_errors_leave_the_outputs_untouched(cases):
    lib = nvdb_amd.load_library()
    c = cases(I8, 100)
    nq, k = 4, 100
    q = np.ascontiguousarray(c.queries[:nq])
    probe = np.array([[1, BIG]] * nq, dtype=np.uint32)
    ids = np.full((nq, k), 7, dtype=np.uint64)
    sc = np.full((nq, k), 7.0, dtype=np.float32)
    cnt = np.full(nq, 7, dtype=np.uint32)
    mo = np.zeros(nq, dtype=np.uint32)

    def parts(ctx, probe, mask_of, masked, k=k, nq=nq, nprobe=2):
        return lib.nvdb_hip_search_partitions_anyk(ctx.h, q.ctypes.data, nq, k, probe.ctypes.data if probe is not None else None, nprobe,
                                                   mask_of.ctypes.data if mask_of is not None else None, masked, ids.ctypes.data, sc.ctypes.data,
                                                   cnt.ctypes.data, None)

    def ivf(ctx, mask_of, masked):
        return lib.nvdb_hip_search_ivf_anyk(ctx.h, q.ctypes.data, nq, k, 2, mask_of.ctypes.data if mask_of is not None else None, masked,
                                            ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None, None)

    def untouched():
        return (ids == 7).all() and (sc == 7.0).all() and (cnt == 7).all()

    badp = probe.copy()
    badp[3, 1] = NPARTS                            # a probe entry >= nparts that is not the sentinel
    assert parts(c.ctx, badp, None, 0) == 1 and "nparts" in lib.nvdb_hip_last_error(c.ctx.h).decode() and untouched()
    badm = mo.copy()
    badm[2] = NMASKS                               # a mask_of entry >= nmasks
    assert parts(c.ctx, probe, badm, 1) == 1 and "nmasks" in lib.nvdb_hip_last_error(c.ctx.h).decode() and untouched()
    assert parts(c.ctx, probe, badm, 0) == 0 and not untouched()          # masked == 0 ignores mask_of
    ids[:], sc[:], cnt[:] = 7, 7.0, 7
    assert parts(c.ctx, None, None, 0) == 1 and untouched()               # null probe table
    assert parts(c.ctx, probe, None, 0, k=0) == 0 and parts(c.ctx, probe, None, 0, nq=0) == 0 and untouched()
    ctx = nvdb_amd.HipContext(0)
    try:
        assert parts(ctx, probe, None, 0) == 4 and ivf(ctx, None, 0) == 4 and untouched()         # no corpus
        ctx.upload_corpus(c.base, I8, c.scales, ROW_BASE)
        assert parts(ctx, probe, None, 0) == 1 and "partition" in lib.nvdb_hip_last_error(ctx.h).decode() and untouched()      # no table
        assert ivf(ctx, None, 0) == 1 and untouched()
        ctx.set_partitions(OFFSETS)
        assert ivf(ctx, None, 0) == 1 and "centroids" in lib.nvdb_hip_last_error(ctx.h).decode() and untouched()              # no centroids
        assert parts(ctx, probe, mo, 1) == 1 and "row masks" in lib.nvdb_hip_last_error(ctx.h).decode() and untouched()       # masked without planes
        assert parts(ctx, probe, None, 1) == 1 and untouched()
        assert parts(ctx, probe, mo, 0) == 0 and (cnt == 100).all()       # ... and the same context answers
    finally:
        ctx.close()


def test_statistics_and_timing(cases):
    c = cases(F16, 768)
    probe = np.array([[BIG, 5], [1, 2], [EMPTY, SENT]], dtype=np.uint32)
    mo = np.array([HALF, SENT, ALL_LIVE], dtype=np.uint32)
    *_, t = c.ctx.search_partitions_anyk(c.queries[:3], 100, probe, mo, want_timing=True)
    st = c.ctx.stats()
    live = int(PLANES[HALF][union_rows(probe[0])].sum()) + 64
    assert st["path"] == 8 and st["candidates"] == live and st["rows_scanned"] >= 20000 + 257 + 64 and st["chunks"] >= 1, st
    assert t.kernel_ms > 0 and t.total_ms >= t.kernel_ms and t.K == 100 and t.threads == 64 * t.nwarps > 0
    c.ctx.search_partitions_anyk(c.queries[:3], 64, probe)
    assert c.ctx.stats()["path"] == 4              # k <= 64 is the twin, statistics included
