"""The probe, range, mask and IVF paths on corpora whose rows pass 4 GiB of bytes, 2^32 elements and a global id of 2^32.

Every other module of these paths runs on at most 92 MB; here each path meets the "seam" rows of its corpus -- a row whose own bytes
straddle a byte offset of 2^32 / 2^33 / 2^34, whose elements straddle element index 2^32 (row * dim), or whose global id is 2^32
(ROW_BASE + row) -- and asserts that result rows came from beyond every one of them.  A narrowed offset in a load reads other rows of
the same allocation: nothing faults, the neighbours are plausible and wrong.

  tag    dtype, dim  build             N           seam rows
  A      f16, 768    staged            5 700 013   2 796 202 (2^32 B)  4 000 000 (id 2^32)  5 592 405 (2^33 B, 2^32 elements)
  B      i8, 768     staged, scales    5 700 013   4 000 000 (id 2^32)  5 592 405 (2^32 B, 2^32 elements)
  C      f32, 768    direct aligned    5 700 013   1 398 101 (2^32 B)  2 796 202 (2^33 B)  4 000 000  5 592 405 (2^34 B, 2^32 elements)
  D      f16, 100    direct unaligned  43 100 003  21 474 836 (2^32 B)  42 949 672 (2^32 elements)        (probe paths only)
  small  f16, 768    staged            40 009      made up: 10 000, 20 000, 30 000

Corpora are generated on the device; every host-side row comes back through download_rows.  The partition table lays partitions of
64, 1, 257, 65 and 63 rows around each seam row (the seam in the middle of the 257) and a long one behind them (20 000 rows: several
segments), a partition of the last 1000 rows and an empty one; the stretches between are giant partitions that only the full-probe
checks name.  The "probed set" -- the small, long and last partitions, at most about 85 000 rows -- is downloaded once per corpus
and scored by the oracle: there ids, score BITS and counts must equal the oracle's (score desc, id asc), as in the small modules.
On all rows the checks compare with the flat search_batch, which tests/test_gpu_parity.py pins at 10M and 100M rows, and rescore
the returned rows with the oracle.

The checker must not be the thing under test: the table builder and every expectation take the seam rows and N as arguments, and
the instance `small` runs the very same checks in the regime tests/test_gpu_partitions.py, test_gpu_row_masks.py, test_gpu_range_parts.py,
test_gpu_parts_anyk.py and test_gpu_ivf.py already pin (there the long partitions are 5000 rows: three of 20 000 do not fit).  It comes
first; a failure there is a failure of this file, and the large instances mean something only once it passes.

One class per corpus, in file order, so that a corpus is generated once and closed before the next one is generated.  The whole
file takes about 15 s on an MI355X; the slowest case is the first IVF test of a corpus, which assigns all rows and builds the index
(5 567 assignment batches): 1.4 s on A and B, 2.1 s on C.

The comparisons with the flat search need queries whose k + 1 best scores are pairwise distinct.  At these sizes the synthetic
corpus does tie (D holds rows with equal bits; C two different rows with the same fp32 score among a query's best 101), so
Case.flat_queries passes such a query over -- after the oracle has confirmed the tie on the rows copied back.

IVF search with nprobe = 3: the queries are downloaded rows next to the seams and k = 1.  In a synthetic corpus the only row known to
lie inside the downloaded windows is the query's own; that it is the best of ALL rows is asserted through the flat search first."""
import numpy as np
import pytest

import nvdb_amd
import pyoracle as po
from test_gpu_ivf import centroid_table, oracle_assign, row_as_f32, ulp_distance, unit_rows

pytestmark = pytest.mark.gpu

F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8
SEED = 20251020
ROW_BASE = 2**32 - 4_000_000                       # global ids pass 2^32 at local row 4 000 000
SENT = 0xFFFFFFFF
U64MAX = np.iinfo(np.uint64).max
INF = np.float32(np.inf)
NQ_MAX = 70
SMALL_SIZES = (64, 1, 257, 65, 63)                 # around a wave, a single row, around a workgroup; the seam row is row 128 of the 257
SEAM_AT = 64 + 1 + 128
LAST_ROWS = 1000
K_LONG = 8193                                      # slab of 16384 keys > PA_LDS_KEYS (8192): sorted in global memory, then emitted
NPARTS_IVF = 37

SPECS = {
    # tag: dtype, dim, n, seams, long partition, row base
    "small": (F16, 768, 40_009, (10_000, 20_000, 30_000), 5_000, 1_000_003),
    "A": (F16, 768, 5_700_013, (2_796_202, 4_000_000, 5_592_405), 20_000, ROW_BASE),
    "B": (I8, 768, 5_700_013, (4_000_000, 5_592_405), 20_000, ROW_BASE),
    "C": (F32, 768, 5_700_013, (1_398_101, 2_796_202, 4_000_000, 5_592_405), 20_000, ROW_BASE),
    "D": (F16, 100, 43_100_003, (21_474_836, 42_949_672), 20_000, ROW_BASE),
}
ITEM = {F32: 4, F16: 2, I8: 1}


def test_the_seam_rows_straddle_what_the_table_says():
    """Pure arithmetic: each large corpus' seam rows are the rows whose bytes / elements / id contain the boundary."""
    for tag in "ABCD":
        dtype, dim, n, seams, _, base = SPECS[tag]
        row_bytes = dim * ITEM[dtype]
        want = {(1 << b) // row_bytes for b in (32, 33, 34) if (1 << b) // row_bytes < n and (1 << b) % row_bytes}
        want.add((1 << 32) // dim)
        if tag != "D":
            want.add((1 << 32) - base)
        assert sorted(want) == sorted(seams), (tag, sorted(want))
        assert all(0 < s < n - 1 for s in seams) and n % 64 and n % 256


# ------------------------------------------------------------------------------------------------------------ table and expectations
class Table:
    """Partitions over n rows for the given seam rows: [empty] then per seam [gap, 64, 1, 257, 65, 63, long] then [gap, last 1000]."""

    def __init__(self, n, seams, long_rows):
        self.n, self.seams, self.long_rows = n, tuple(sorted(seams)), long_rows
        bounds, kinds = [0, 0], ["empty"]
        for s in self.seams:
            start = s - SEAM_AT
            assert start > bounds[-1], "seams too close for the runs"
            bounds.append(start)
            kinds.append("gap")
            for size in SMALL_SIZES + (long_rows,):
                bounds.append(bounds[-1] + size)
                kinds.append("long" if size == long_rows else "small")
        assert n - LAST_ROWS > bounds[-1]
        bounds += [n - LAST_ROWS, n]
        kinds += ["gap", "last"]
        self.offsets = np.array(bounds, dtype=np.uint64)
        self.kinds = kinds
        self.nparts = len(kinds)
        self.empty, self.last = 0, self.nparts - 1

    def small(self, j):
        """The five small partitions of seam j (64, 1, 257, 65, 63)."""
        return [2 + 7 * j + i for i in range(5)]

    def p257(self, j):
        return 4 + 7 * j

    def long(self, j):
        return 7 + 7 * j

    def run(self, j):
        return self.small(j) + [self.long(j)]

    def span(self, p):
        return int(self.offsets[p]), int(self.offsets[p + 1])

    def stretches(self):
        """The probed set as contiguous (lo, hi) row ranges: one per seam run, and the last partition."""
        return [(self.span(self.small(j)[0])[0], self.span(self.long(j))[1]) for j in range(len(self.seams))] + [self.span(self.last)]

    def rows_of(self, parts):
        out = [np.empty(0, np.int64)]
        for p in sorted(set(int(p) for p in parts if p != SENT)):
            assert self.kinds[p] != "gap", "the oracle does not see the giant partitions"
            lo, hi = self.span(p)
            out.append(np.arange(lo, hi, dtype=np.int64))
        return np.concatenate(out)


def test_the_table_builder():
    t = Table(40_009, (30_000, 10_000, 20_000), 5_000)
    assert t.offsets[0] == 0 and t.offsets[-1] == 40_009 and (np.diff(t.offsets.astype(np.int64)) >= 0).all() and t.nparts == 3 + 7 * 3
    for j, s in enumerate((10_000, 20_000, 30_000)):
        lo, hi = t.span(t.p257(j))
        assert hi - lo == 257 and lo + 128 == s
        assert [t.span(p)[1] - t.span(p)[0] for p in t.run(j)] == [64, 1, 257, 65, 63, 5_000]
        assert t.kinds[t.long(j)] == "long" and all(t.kinds[p] == "small" for p in t.small(j))
    assert t.span(t.empty) == (0, 0) and t.span(t.last) == (39_009, 40_009)
    assert sum(hi - lo for lo, hi in t.stretches()) == 3 * 5_450 + 1_000


def topk_of(s, rows, k, row_base, tie=None):
    """The k best of the candidate local rows `rows` with scores s (aligned with rows): (ids [k], scores [k], count)."""
    order = np.lexsort((rows, -s) if tie is None else (rows, tie, -s))[:k]
    ids = np.full(k, U64MAX, dtype=np.uint64)
    sc = np.full(k, -np.inf, dtype=np.float32)
    ids[:len(order)] = rows[order].astype(np.uint64) + np.uint64(row_base)
    sc[:len(order)] = s[order]
    return ids, sc, min(k, len(rows))


def range_of(s, rows, radius, row_base):
    keep = s >= radius
    rows, s = rows[keep], s[keep]
    order = np.lexsort((rows, -s))
    return rows[order].astype(np.uint64) + np.uint64(row_base), s[order]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


class Case:
    """One generated corpus with its table, the downloaded probed set, queries, lazily the oracle's scores, planes and the index."""

    def __init__(self, orc, tag):
        self.orc, self.tag = orc, tag
        self.dtype, self.dim, self.n, seams, long_rows, self.row_base = SPECS[tag]
        self.t = Table(self.n, seams, long_rows)
        self.seams = self.t.seams
        self.ctx = nvdb_amd.HipContext(0)
        self.ctx.generate_corpus(SEED, self.n, self.dim, self.dtype, self.row_base)
        self.ctx.set_partitions(self.t.offsets)
        self.rows, self.base, self.scales = self.download_probed_set()
        self.queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ_MAX, self.dim)
        self._scores, self._ivf, self._masks, self._flat = {}, None, None, None

    def close(self):
        if self._ivf is not None:
            self._ivf.close()
        self.ctx.close()

    def download_probed_set(self, ctx=None):
        rows, base, scales = [], [], []
        for lo, hi in self.t.stretches():
            b, s = (ctx or self.ctx).download_rows(lo, hi - lo)
            rows.append(np.arange(lo, hi, dtype=np.int64))
            base.append(b)
            scales.append(s)
        return np.concatenate(rows), np.concatenate(base), (np.concatenate(scales) if self.dtype == I8 else None)

    def at(self, rows):
        """Positions of local rows inside the probed set."""
        pos = np.searchsorted(self.rows, rows)
        assert np.array_equal(self.rows[pos], rows)
        return pos

    def scores(self, q):
        if q not in self._scores:
            self._scores[q] = self.orc.scores(self.base, self.dtype, self.queries[q], self.scales)
        return self._scores[q]

    def union(self, probe_row, live=None):
        rows = self.t.rows_of(probe_row)
        return rows if live is None else rows[live[rows]]

    def probe_table(self, nq, both_longs=False):
        """Query q: the 257-row partition and the long partition of seam q mod S; a slot that walks the empty partition, the sentinel,
        every small partition of every seam and the last partition; for q >= S (or always) the long partition of the next seam."""
        t, S = self.t, len(self.seams)
        fill = [t.empty, SENT] + [p for j in range(S) for p in t.small(j)] + [t.last]
        out = np.full((nq, 4), SENT, dtype=np.uint32)
        for q in range(nq):
            j = q % S
            out[q, 0], out[q, 1], out[q, 2] = t.p257(j), t.long(j), fill[q % len(fill)]
            if q >= S or both_longs:
                out[q, 3] = t.long((j + 1) % S)
        return out

    def assert_beyond_every_seam(self, ids, what):
        """Some returned row lies strictly behind each seam row and before the next one (or the end)."""
        ids = np.asarray(ids).ravel()
        local =(ids[ids != U64MAX] - np.uint64(self.row_base)).astype(np.int64)
        for s, nxt in zip(self.seams, self.seams[1:] + (self.n,)):
            assert ((local > s) & (local < nxt)).any(), (self.tag, what, "no result row behind seam row", s)

    def rescore(self, q, ids, sc, every=1):
        """The returned scores are, bit for bit, the oracle's score of the returned rows copied back one by one."""
        for j in range(0, len(ids), every):
            row, scale = self.ctx.download_rows(int(ids[j] - np.uint64(self.row_base)), 1)
            s = self.orc.scores(row, self.dtype, self.queries[q], scale)
            assert same_bits(s[:1], sc[j:j + 1]), (self.tag, q, j, int(ids[j]), s[0], sc[j])

    def flat_queries(self, nq=9, pool=18, k=100):
        """Query numbers for the comparisons with the flat search: the first nq of the first `pool` queries whose k + 1 best flat
        scores are pairwise distinct -- the precondition, without which the order inside a tie (by id / by list) and the size of a
        range result are the data's business.  Millions of synthetic rows do tie now and then (two rows with the same bits; two
        different rows with the same score): such a query is passed over only after the oracle has scored both rows of each tie
        to the very same bits, so a list that repeats a score for another reason fails here.  -> (numbers, ids, scores) at k + 1."""
        if self._flat is None:
            ids, sc = self.ctx.search_batch(self.queries[:pool], k + 1)
            good = []
            for q in range(pool):
                assert len(set(ids[q].tolist())) == k + 1, (self.tag, q, "the flat list repeats an id")
                ties = np.flatnonzero(sc[q, :-1].view(np.uint32) == sc[q, 1:].view(np.uint32))
                for j in ties:
                    self.rescore(q, ids[q, j:j + 2], sc[q, j:j + 2])
                if ties.size == 0:
                    good.append(q)
            assert len(good) >= nq, (self.tag, "too few queries without a tie among their best", k + 1, good)
            good = np.array(good[:nq])
            self._flat = (good, ids[good], sc[good])
        return self._flat

    # -- row masks
    def masks(self):
        """Plane 0 random 50 %, plane 1 all live but the seam rows and every query's oracle top-3 of its probed union; set, then
        tombstones through update_row_mask; the device image must equal the host's over all W words."""
        if self._masks is None:
            n = self.n
            probe = self.probe_table(NQ_MAX)
            planes = np.stack([np.random.RandomState(77).rand(n) < 0.5, np.ones(n, bool)])
            planes[1, list(self.seams)] = False
            for q in range(NQ_MAX):
                rows = self.union(probe[q])
                planes[1, rows[np.lexsort((rows, -self.scores(q)[self.at(rows)]))[:3]]] = False
            self.ctx.set_row_masks(planes)
            assert np.array_equal(self.ctx.get_row_masks(), nvdb_amd.pack_row_masks(planes, n))
            dead = np.array(list(self.seams) + [n - 1, 0, self.seams[0], n - 1 - 32], dtype=np.uint64)    # a duplicate; two words at the end
            self.ctx.update_row_mask(0, dead, live=False)
            planes[0, dead.astype(np.int64)] = False
            alive = np.array([self.seams[-1], 0, n - 1], dtype=np.uint64)                                  # (0 and n - 1 already are)
            self.ctx.update_row_mask(1, alive, live=True)
            planes[1, alive.astype(np.int64)] = True
            got = self.ctx.get_row_masks()
            want = nvdb_amd.pack_row_masks(planes, n)
            assert got.shape == want.shape == (2, (n + 31) // 32)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (self.tag, "mask words differ", bad[:8])
            self._masks = (planes, probe, (np.arange(NQ_MAX) % 3).astype(np.uint32))
            self._masks[2][self._masks[2] == 2] = SENT
        return self._masks

    # -- IVF
    def ivf(self):
        if self._ivf is None:
            self.cen = centroid_table(self.dim)
            self.full_assign = self.ctx.assign_rows(self.cen)
            self._ivf = nvdb_amd.IvfIndex(self.ctx, self.cen)
        return self._ivf


@pytest.fixture(scope="module")
def corpora(oracle):
    """The one corpus resident at a time: asking for another tag closes the current one first."""
    held = {}

    def get(tag):
        if tag not in held:
            for c in held.values():
                c.close()
            held.clear()
            held[tag] = Case(oracle, tag)
        return held[tag]
    yield get
    for c in held.values():
        c.close()


# ------------------------------------------------------------------------------------------------------------ the checks
class ProbeChecks:
    """Checks 1-3 (oracle on the probed set) and 5 (flat search on all rows)."""
    TAG = None

    @pytest.fixture()
    def c(self, corpora):
        return corpora(self.TAG)

    @pytest.mark.parametrize("nq,k", [(9, 1), (9, 10), (9, 64), (70, 10), (70, 64)])
    def test_search_partitions(self, c, nq, k):
        probe = c.probe_table(nq)
        ids, sc, counts = c.ctx.search_partitions(c.queries[:nq], k, probe)
        assert c.ctx.stats()["path"] == 4
        for q in range(nq):
            rows = c.union(probe[q])
            eid, esc, ecnt = topk_of(c.scores(q)[c.at(rows)], rows, k, c.row_base)
            assert counts[q] == ecnt, (q, counts[q], ecnt)
            assert np.array_equal(ids[q], eid), (q, ids[q], eid)
            assert same_bits(sc[q], esc), (q, sc[q], esc)
        c.assert_beyond_every_seam(ids, f"search_partitions k {k}")
        # the empty partition and sentinel slots alone
        ids, sc, counts = c.ctx.search_partitions(c.queries[:2], k, np.array([[c.t.empty, SENT], [SENT, SENT]], dtype=np.uint32))
        assert (counts == 0).all() and (ids == U64MAX).all() and np.isneginf(sc).all()

    @pytest.mark.parametrize("k", [100, 1024, K_LONG])
    def test_search_partitions_anyk(self, c, k):
        nq = 9
        probe = c.probe_table(nq, both_longs=True)
        ids, sc, counts = c.ctx.search_partitions_anyk(c.queries[:nq], k, probe)
        st = c.ctx.stats()
        assert st["path"] == 8, st
        for q in range(nq):
            rows = c.union(probe[q])
            assert len(rows) > k
            eid, esc, ecnt = topk_of(c.scores(q)[c.at(rows)], rows, k, c.row_base)
            bad = np.flatnonzero(ids[q] != eid)
            assert counts[q] == ecnt and bad.size == 0, (q, counts[q], ecnt, bad[:5], ids[q][bad[:5]], eid[bad[:5]])
            assert same_bits(sc[q], esc), q
        c.assert_beyond_every_seam(ids, f"search_partitions_anyk k {k}")

    def test_range_search_partitions(self, c):
        nq = 9
        probe = c.probe_table(nq)
        for kth in (10, 500):
            radius = np.array([np.sort(c.scores(q)[c.at(c.union(probe[q]))])[::-1][kth - 1] for q in range(nq)], dtype=np.float32)
            lims, ids, sc = c.ctx.range_search_partitions(c.queries[:nq], radius, probe)
            assert c.ctx.stats()["path"] == 7
            for q in range(nq):
                rows = c.union(probe[q])
                eid, esc = range_of(c.scores(q)[c.at(rows)], rows, radius[q], c.row_base)
                lo, hi = int(lims[q]), int(lims[q + 1])
                assert hi - lo == len(eid) >= kth, (kth, q, hi - lo, len(eid))
                assert np.array_equal(ids[lo:hi], eid) and same_bits(sc[lo:hi], esc), (kth, q)
            if kth == 500:
                c.assert_beyond_every_seam(ids, "range_search_partitions")
        # radius -inf: every row of a seam run, each seam in turn
        for j in range(len(c.seams)):
            run = np.array([c.t.run(j)] * 2, dtype=np.uint32)
            lims, ids, sc = c.ctx.range_search_partitions(c.queries[:2], np.full(2, -INF), run)
            rows = c.union(run[0])
            assert lims.tolist() == [0, len(rows), 2 * len(rows)]
            for q in range(2):
                eid, esc = range_of(c.scores(q)[c.at(rows)], rows, -INF, c.row_base)
                assert np.array_equal(ids[q * len(rows):(q + 1) * len(rows)], eid) and same_bits(sc[q * len(rows):(q + 1) * len(rows)], esc), (j, q)

    def test_full_probe_equals_the_flat_search(self, c):
        qn, f101, s101 = c.flat_queries()                                   # precondition: the k + 1 best flat scores are pairwise distinct
        nq = len(qn)
        q = c.queries[qn]
        probe = np.tile(np.arange(c.t.nparts, dtype=np.uint32), (nq, 1))
        fid, fsc = c.ctx.search_batch(q, 10)
        assert np.array_equal(fid, f101[:, :10]) and same_bits(fsc, s101[:, :10])
        ids, sc, counts = c.ctx.search_partitions(q, 10, probe)
        assert np.array_equal(ids, fid) and same_bits(sc, fsc) and (counts == 10).all()
        f100, s100 = c.ctx.search_batch(q, 100)
        assert np.array_equal(f100, f101[:, :100]) and same_bits(s100, s101[:, :100])
        ids, sc, counts = c.ctx.search_partitions_anyk(q, 100, probe)
        assert np.array_equal(ids, f100) and same_bits(sc, s100) and (counts == 100).all()
        lims, rid, rsc = c.ctx.range_search_partitions(q, fsc[:, 9].copy(), probe)
        assert lims.tolist() == list(range(0, 10 * nq + 1, 10))
        assert np.array_equal(rid.reshape(nq, 10), fid) and same_bits(rsc.reshape(nq, 10), fsc)
        for i, qi in enumerate(qn):
            c.rescore(int(qi), ids[i], sc[i])
        c.assert_beyond_every_seam(ids, "full probe, k = 100")


class MaskChecks:
    """Check 4: set_row_masks / update_row_mask / get_row_masks and the masked probe searches against the oracle on live rows."""

    def test_tombstones_and_the_mask_image(self, c):
        planes, _, _ = c.masks()
        assert not planes[0, list(c.seams)].any() and not planes[0, 0] and not planes[0, c.n - 1]
        assert planes[1, c.seams[-1]] and not planes[1, c.seams[0]]

    def live_rows(self, c, q):
        planes, probe, mask_of = c.masks()
        m = int(mask_of[q])
        return c.union(probe[q], None if m == SENT else planes[m])

    @pytest.mark.parametrize("nq,k", [(9, 10), (70, 10), (70, 64)])
    def test_search_partitions_masked(self, c, nq, k):
        _, probe, mask_of = c.masks()
        ids, sc, counts = c.ctx.search_partitions_masked(c.queries[:nq], k, probe[:nq], mask_of[:nq])
        for q in range(nq):
            rows = self.live_rows(c, q)
            eid, esc, ecnt = topk_of(c.scores(q)[c.at(rows)], rows, k, c.row_base)
            assert counts[q] == ecnt and np.array_equal(ids[q], eid) and same_bits(sc[q], esc), (q, int(mask_of[q]), ids[q], eid)
        c.assert_beyond_every_seam(ids, "search_partitions_masked")

    @pytest.mark.parametrize("k", [100, 1024])
    def test_search_partitions_anyk_masked(self, c, k):
        _, probe, mask_of = c.masks()
        nq = 9
        ids, sc, counts = c.ctx.search_partitions_anyk(c.queries[:nq], k, probe[:nq], mask_of[:nq])
        assert c.ctx.stats()["path"] == 8
        for q in range(nq):
            rows = self.live_rows(c, q)
            eid, esc, ecnt = topk_of(c.scores(q)[c.at(rows)], rows, k, c.row_base)
            assert counts[q] == ecnt and np.array_equal(ids[q], eid) and same_bits(sc[q], esc), (q, int(mask_of[q]))
        c.assert_beyond_every_seam(ids, "masked any-k")

    def test_range_search_partitions_masked(self, c):
        _, probe, mask_of = c.masks()
        nq = 9
        for kth in (10, 500):
            radius = np.array([np.sort(c.scores(q)[c.at(self.live_rows(c, q))])[::-1][kth - 1] for q in range(nq)], dtype=np.float32)
            lims, ids, sc = c.ctx.range_search_partitions(c.queries[:nq], radius, probe[:nq], mask_of[:nq])
            for q in range(nq):
                rows = self.live_rows(c, q)
                eid, esc = range_of(c.scores(q)[c.at(rows)], rows, radius[q], c.row_base)
                lo, hi = int(lims[q]), int(lims[q + 1])
                assert hi - lo == len(eid) and np.array_equal(ids[lo:hi], eid) and same_bits(sc[lo:hi], esc), (kth, q, int(mask_of[q]))
        c.assert_beyond_every_seam(ids, "masked range search")


class FlatChecks:
    """Check 6: the flat range search and the masked flat searches on the MFMA filter route at this size."""

    def streams(self, c):
        return {F16: "shadow", F32: "shadow", I8: "i8"}[c.dtype]            # fp16 / fp32: the int8 shadow is automatic from 2^20 rows

    def test_range_search(self, c):
        nq = 9
        q = c.queries[:nq]
        f65, s65 = c.ctx.search_batch(q, 65)
        assert all(len(set(r.view(np.uint32).tolist())) == 65 for r in s65)
        f64, s64 = c.ctx.search_batch(q, 64)
        assert np.array_equal(f64, f65[:, :64]) and same_bits(s64, s65[:, :64])
        for k in (10, 64):
            lims, ids, sc = c.ctx.range_search(q, s64[:, k - 1].copy())
            st, sh = c.ctx.stats(), c.ctx.shadow_info()
            assert st["path"] == 5 and st["bound_violations"] == 0 and sh["last_filter"] == self.streams(c), (st, sh)
            assert c.dtype == I8 or sh["resident"]
            assert lims.tolist() == list(range(0, k * nq + 1, k)), (k, lims)
            assert np.array_equal(ids.reshape(nq, k), f64[:, :k]) and same_bits(sc.reshape(nq, k), s64[:, :k]), k
        c.assert_beyond_every_seam(f64, "flat top-64 / range_search")

    def test_masked_flat_routes(self, c):
        nq, k = 9, 10
        q = c.queries[:nq]
        f65, s65 = c.ctx.search_batch(q, 65)
        assert all(len(set(r.view(np.uint32).tolist())) == 65 for r in s65)
        f64, s64 = f65[:, :64], s65[:, :64]
        local = (f64 - np.uint64(c.row_base)).astype(np.int64)
        plane = np.ones((1, c.n), bool)
        rs = np.random.RandomState(5)
        for qi in range(nq):
            # 40 of the top-64.  The stretch behind the last seam is the short one, so: the first row from there (rank p <= 49) is kept
            # and p - 9 of the rows ahead of it are killed -- it becomes the 10th live row, the last result and the masked range
            # search's radius; the other rows from behind the last seam are killed first, then rows behind rank p at random
            far = np.flatnonzero(local[qi] > c.seams[-1])
            p = next((int(r) for r in far if r <= 49), None)
            kill = [] if p is None else rs.permutation(p)[:max(0, p - 9)].tolist()
            behind = [int(r) for r in far if r != p] + [int(r) for r in rs.permutation(64) if r not in far and (p is None or r > p)]
            kill += behind[:40 - len(kill)]
            assert len(set(kill)) == 40 and p not in kill
            plane[0, local[qi][kill]] = False
        assert all(not plane[0, s + 1:nxt].all() for s, nxt in zip(c.seams, c.seams[1:] + (c.n,))), "no dead row behind some seam"
        had = c.ctx.get_row_masks() if c._masks is not None else None
        c.ctx.set_row_masks(plane)
        try:
            want_ids, want_sc = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float32)
            for qi in range(nq):
                live = np.flatnonzero(plane[0, local[qi]])
                assert len(live) >= k and len(live) < 64
                want_ids[qi], want_sc[qi] = f64[qi, live[:k]], s64[qi, live[:k]]
            ids, sc, counts = c.ctx.search_masked(q, k, None)
            st, sh = c.ctx.stats(), c.ctx.shadow_info()
            note = f"search_masked: flagged {st['overflow_queries']}, bound violations {st['bound_violations']}, sticky {st['sticky_overflow']} / {st['sticky_violations']}"
            print(c.tag, note)
            assert st["path"] == 2 and sh["last_filter"] == self.streams(c), (note, st, sh)
            assert np.array_equal(ids, want_ids) and same_bits(sc, want_sc) and (counts == k).all(), note
            lims, rid, rsc = c.ctx.range_search_masked(q, want_sc[:, k - 1].copy(), None)
            st, sh = c.ctx.stats(), c.ctx.shadow_info()
            note = f"range_search_masked: flagged {st['overflow_queries']}, bound violations {st['bound_violations']}, sticky {st['sticky_overflow']} / {st['sticky_violations']}"
            print(c.tag, note)
            assert st["path"] == 5 and sh["last_filter"] == self.streams(c), (note, st, sh)
            assert lims.tolist() == list(range(0, k * nq + 1, k)), (note, lims)
            assert np.array_equal(rid.reshape(nq, k), want_ids) and same_bits(rsc.reshape(nq, k), want_sc), note
            c.assert_beyond_every_seam(ids, "masked flat top-k")
        finally:
            c.ctx.set_row_masks(had)


class LargeKChecks:
    """Check 7: search_batch for k = 2000 (the any-k flat path) at this size."""

    def test_search_batch_k_2000(self, c):
        nq, k = 3, 2000
        q = c.queries[:nq]
        ids, sc = c.ctx.search_batch(q, k)
        assert ids.shape == (nq, k)
        f64, s64 = c.ctx.search_batch(q, 64)
        assert np.array_equal(ids[:, :64], f64) and same_bits(sc[:, :64], s64)
        assert np.all((sc[:, :-1] > sc[:, 1:]) | ((sc[:, :-1] == sc[:, 1:]) & (ids[:, :-1] < ids[:, 1:])))
        for qi in range(nq):
            assert len(set(ids[qi].tolist())) == k and int(ids[qi].max()) < c.row_base + c.n and int(ids[qi].min()) >= c.row_base
            c.rescore(qi, ids[qi], sc[qi], every=50)
            better = c.rows[c.scores(qi) > sc[qi, -1]] + c.row_base
            assert set(better.tolist()) <= set(ids[qi].tolist()), qi
        c.assert_beyond_every_seam(ids, "search_batch k = 2000")


class IvfChecks:
    """Checks 8-10: assignment, layout and gather, search of the IVF build."""

    def windows(self, c, half):
        """Local rows within `half` of every seam row, and the last 100 rows: all inside the probed set."""
        return np.concatenate([np.arange(s - half, s + half + 1, dtype=np.int64) for s in c.seams] + [np.arange(c.n - 100, c.n, dtype=np.int64)])

    def rows_f32(self, c, rows):
        pos = c.at(rows)
        return row_as_f32(c.base[pos], c.dtype, None if c.scales is None else c.scales[pos])

    def test_assignment(self, c):
        c.ivf()
        rows = self.windows(c, 100)
        want = oracle_assign(c.orc, c.cen, self.rows_f32(c, rows))
        assert c.full_assign.shape == (c.n,) and np.array_equal(c.full_assign[rows], want), np.flatnonzero(c.full_assign[rows] != want)[:10]
        for i, s in enumerate(c.seams):                                      # windows that straddle each seam, read through row0 / nrows
            got = c.ctx.assign_rows(c.cen, row0=s - 100, nrows=201)
            assert np.array_equal(got, want[i * 201:(i + 1) * 201]), s
        assert np.array_equal(c.ctx.assign_rows(c.cen, row0=c.n - 100, nrows=100), want[-100:])

    def test_layout_and_gather(self, c):
        ivf = c.ivf()
        info = ivf.info()
        perm = info["perm"]
        assert info["n"] == c.n and info["nparts"] == NPARTS_IVF and perm.shape == (c.n,)
        assert (np.bincount(perm, minlength=c.n) == 1).all()
        assert np.array_equal(perm, np.argsort(c.full_assign, kind="stable").astype(np.uint32))
        assert np.array_equal(info["offsets"], np.concatenate([[0], np.cumsum(np.bincount(c.full_assign, minlength=NPARTS_IVF))]).astype(np.uint64))
        # the source is byte for byte what it was before the build
        rows, base, scales = c.download_probed_set()
        assert base.tobytes() == c.base.tobytes() and (c.scales is None or scales.tobytes() == c.scales.tobytes())
        assert c.ctx.corpus_info()["row_base"] == c.row_base and ivf.ctx.corpus_info()["row_base"] == 0

        def same_row(j, drow, dscale):
            srow, sscale = c.ctx.download_rows(int(perm[j]), 1)
            assert drow.tobytes() == srow.tobytes(), (c.tag, "position", j, "source row", int(perm[j]))
            assert dscale is None or dscale.tobytes() == sscale.tobytes(), (c.tag, "scale at position", j)
        for s in c.seams:                                                    # destination positions around every seam
            drows, dscales = ivf.ctx.download_rows(s - 40, 81)
            for i in range(81):
                same_row(s - 40 + i, drows[i], None if dscales is None else dscales[i:i + 1])
        far = np.flatnonzero(perm > c.seams[-1])                             # ... and positions whose SOURCE row lies behind the last seam
        assert len(far) >= 200
        for j in far[np.linspace(0, len(far) - 1, 200).astype(np.int64)]:
            drow, dscale = ivf.ctx.download_rows(int(j), 1)
            same_row(int(j), drow[0], dscale)

    def test_search_full_probe(self, c):
        qn, f101, s101 = c.flat_queries()                                    # precondition: no two equal scores among the best k + 1
        q = c.queries[qn]
        ids, sc, counts = c.ivf().search(q, 10, NPARTS_IVF)
        assert np.array_equal(ids, f101[:, :10]) and same_bits(sc, s101[:, :10]) and (counts == 10).all()
        assert int(ids.min()) >= c.row_base
        ids, sc, counts = c.ivf().search_anyk(q, 100, NPARTS_IVF)            # the same at k = 100, so that every stretch between seams is met
        assert np.array_equal(ids, f101[:, :100]) and same_bits(sc, s101[:, :100]) and (counts == 100).all()
        c.assert_beyond_every_seam(ids, "ivf full probe")

    def test_search_three_probes(self, c):
        ivf = c.ivf()
        qrows = np.array([s + d for s in c.seams for d in (0, 1, 57)][:9] + [c.n - 1], dtype=np.int64)
        queries = self.rows_f32(c, qrows)
        nq = len(qrows)
        fid, fsc = c.ctx.search_batch(queries, 2)                            # precondition: the query's own row is the best of ALL rows, alone
        assert np.array_equal(fid[:, 0], qrows.astype(np.uint64) + np.uint64(c.row_base)) and (fsc[:, 0] > fsc[:, 1]).all()
        ids, sc, counts, probe = ivf.search(queries, 1, 3, want_probe=True)
        for i in range(nq):
            cs = c.orc.scores(c.cen, po.DT_F32, queries[i])
            probes = np.lexsort((np.arange(NPARTS_IVF), -cs))[:3]
            assert np.array_equal(probe[i], probes.astype(np.uint32)), (i, probe[i], probes)
            rows = c.rows[np.isin(c.full_assign[c.rows], probes)]            # the downloaded rows whose (pinned) assignment is probed
            s = c.orc.scores(c.base[c.at(rows)], c.dtype, queries[i], None if c.scales is None else c.scales[c.at(rows)])
            eid, esc, ecnt = topk_of(s, rows, 1, c.row_base, tie=c.full_assign[rows])
            assert eid[0] == fid[i, 0] and same_bits(esc, fsc[i, :1]), (i, "the oracle's best downloaded row is not the flat search's")
            assert counts[i] == ecnt and np.array_equal(ids[i], eid) and same_bits(sc[i], esc), (i, ids[i], eid)
        c.assert_beyond_every_seam(ids, "ivf nprobe 3")


class TrainChecks:
    """Check 11: one training step on 4000 rows spread over the whole corpus against numpy fp64.  Tolerance: 1 f32 ulp per component
    (tests/test_gpu_ivf.py::test_training_step_matches_fp64 derives it; it does not depend on N)."""

    def test_training_step(self, c):
        nparts, tn = 16, 4000
        init = unit_rows(np.random.RandomState(c.dim + c.dtype), nparts, c.dim)
        got = c.ctx.train_centroids(nparts, 1, seed=0, max_train_rows=tn, init=init)
        rows = (np.arange(tn, dtype=np.int64) * c.n) // tn
        assert (rows > c.seams[-1]).any()
        f32 = np.empty((tn, c.dim), dtype=np.float32)
        for i, r in enumerate(rows):
            b, s = c.ctx.download_rows(int(r), 1)
            f32[i] = row_as_f32(b, c.dtype, s)[0]
        assign = oracle_assign(c.orc, init, f32)
        rows64 = f32.astype(np.float64)
        want = init.copy()
        for p in range(nparts):
            members = rows64[assign == p]
            assert len(members) > 0
            mean = members.mean(axis=0, dtype=np.float64)
            want[p] = (mean / np.sqrt(np.sum(mean * mean))).astype(np.float32)
        d = ulp_distance(got, want)
        print(f"one step over {tn} of {c.n} rows: max ulp distance {d.max()}, components off by one {int((d == 1).sum())} of {d.size}")
        assert d.max() <= 1, (d.max(), np.argwhere(d > 1)[:5])


# ------------------------------------------------------------------------------------------------------------ one class per corpus, in this order
class TestSmall(ProbeChecks, MaskChecks, IvfChecks):
    TAG = "small"


class TestA(ProbeChecks, MaskChecks, FlatChecks, LargeKChecks, IvfChecks, TrainChecks):
    TAG = "A"


class TestB(ProbeChecks, MaskChecks, FlatChecks, IvfChecks):
    TAG = "B"


class TestC(ProbeChecks, IvfChecks):
    TAG = "C"


class TestD(ProbeChecks):
    TAG = "D"
