"""The reference's dot-product order at every dim tail, on every route that restates it.

The score of a (query, row) pair must carry the bits of the reference's AVX2 kernels.  The GPU code restates that accumulation
order in exact_scores<> (exact scan, any-k score matrix, part_walk of the probe / range / masked scans, rescore_kernel),
rescore8_kernel (its own body loop, shuffle reduction and tails), score8<> (rescore_lds_kernel, the select's exact bar) and, for the
refine's squared L2 distance, l2_f16_ref_order<> / l2_f32_ref_order<>.  Each has tail code of its own:

  * f32 and f16 take dim & ~7 elements in the vector body, int8 dim & ~15: a whole group of 8 can fall to the scalar tail;
  * the f32 tail is ONE unfused multiply-then-add group of four, then fused steps; the f16 and int8 tails are fused throughout;
  * the f16 refine puts leftover pairs into accumulator 0 and drops the odd last element (dim >> 1 pairs).

Dims.  GOLDEN_DIMS (37, 31, 15, 13, 300, 100): the real reference's 48 dot products per dtype are in tests/golden/flat_golden.npz.
SWEEP_DIMS 17 .. 48: every residue mod 16 twice, each behind a non-empty vector body.  LONG_DIMS 391, 777, 1545 (384 + 7,
768 + 9, 1536 + 9): rescore8_kernel's 48-way unrolled loop and exact_scores' 2-way unroll run through their remainders.  For the
sweep and the long dims the real reference's bits are in tests/golden/dot_tails_golden.npz (oracle/make_golden.py dot_tails).

Truth.  Inputs are golden_inputs.make_dot_inputs(d), sha-checked against the fixture.  The 48 x n score matrix comes from the
oracle; its diagonal over the 48 fixture rows must equal the reference's recorded bits -- asserted on the CPU, when a corpus is
built, before any GPU call on it.  Expected results are the oracle's scores ordered (score desc, id asc); every comparison is
ids and score BITS.  The exact scan and the any-k search return every pair, and there the diagonal of what the GPU returned is
compared with the reference's recorded bits directly, at every dim.

Corpora per (dtype, dim).  small: the 48 fixture rows (f32 / f16 bits / int8 with the fixture's per-row scales).  wide: the same 48
rows followed by nvdb_amd.synth_corpus filler up to n = 4100 >= 4 x chunk0_rows, so that the filter route runs through the
zero-padded shadows and the last tile is ragged.  Queries: the 48 fixture queries.

Routes (one test per dtype and route, the dims looped inside; each asserts stats()["path"]):
  exact scan   small, path = 1, k = 48, nq 1 / 2 / 4 / 9 / 48: scan_exact_kernel at QG 1 / 2 / 4 / 8 and the group shifted back
  any-k        k = 65, nq 1 / 3 / 48, path 3: scores_exact_kernel at every QG.  On the 48-row corpus k = 65 clamps to 48 BEFORE the
               route is chosen (plan_search: k_eff = min(k, n), any-k needs k_eff > 64), so that call is the exact scan: asserted
               as such (path 1, same result).  The any-k path itself runs on the first 65 rows of the wide corpus -- the 48 fixture
               rows and 17 filler rows -- where k = 65 = n returns every pair.
  filter       wide, path = 2, k 10 / 64, nq 48, rescore8 2 / 1 / 0: rescore_lds_kernel / score8 where rows are 16-byte multiples,
               rescore8_kernel elsewhere and at rescore8 = 1, rescore_kernel<DT, true / false> at 0; zero overflow, zero bound
               violations, the three results identical.  int8 at dim 1545 has no filter (int8 dims end at 1536): the forced route
               must be refused.
  range        small, path = 1, radius = each query's 10th-best oracle score, and -inf: path 6
  probe        wide, partitions of 64, 1, 257 and the rest; search_partitions k = 10 at nprobe 1 / 3 and nq 1 / 9 / 48 (path 4),
               one range_search_partitions (7), one search_partitions_anyk at k = 100 (8), one masked search under a random
               half-live plane (4): part_walk at every QW class
  adopted      dims 37, 31, 15, 13: an exactly-sized torch tensor adopted; the exact scan and one probe search read the unaligned
               loads at the true end of the allocation
  refine       wide, f16 and f32, refine_v2 0 and 1, R = 48 (the fixture rows, shuffled per query), K = 10, at the sweep, the
               golden tail dims and the long dims; truth is oracle.refine(mode = 0).  Both drop the odd last element of an f16 row
               as the reference kernel does (its D / 2 pairs); no disagreement was found.

Which part_walk build a dim takes (PartBuild, nvdb_partitions.cpp: staged where a row is whole 16-byte chunks of at most 1536
bytes; else direct, aligned where aligned_rows() holds):
  f32   staged: dim % 4 == 0 (20, 24, .. 48, 100, 300); direct unaligned: every other dim (none of these dims is direct aligned)
  f16   staged: dim % 8 == 0 (24, 32, 40, 48); direct unaligned: every other dim
  int8  staged: dim % 16 == 0 (32, 48); direct aligned: dim % 16 == 8 (24, 40); direct unaligned: every other dim

Wall time on an MI355X: 20 cases, 8 s of tests when the module runs alone (10 - 20 s with start-up); the slowest are the three
filter cases at 1.5 s each (41 dims x 2 k x 3 rescore kernels x 48 queries), the probe cases take 0.7 s, all others under 0.3 s.
The first test of a session that touches PyTorch's GPU side also pays its initialisation (2 - 11 s were seen): alone, that is
test_adopted_unpadded[f32]; in the whole suite an earlier module has paid it."""
import os

import numpy as np
import pytest

import nvdb_amd
import pyoracle as po
from golden_inputs import TAIL_LONG_DIMS, TAIL_SWEEP_DIMS, make_dot_inputs, sha
from parity import assert_topk_equal

pytestmark = pytest.mark.gpu

F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8
TAGS = {"f32": F32, "f16": F16, "i8": I8}
GOLDEN_DIMS = (37, 31, 15, 13, 300, 100)
GOLDEN_TAIL_DIMS = (37, 31, 15, 13)
SWEEP_DIMS = TAIL_SWEEP_DIMS
LONG_DIMS = TAIL_LONG_DIMS
ALL_DIMS = GOLDEN_DIMS + SWEEP_DIMS + LONG_DIMS
REFINE_DIMS = SWEEP_DIMS + GOLDEN_TAIL_DIMS + LONG_DIMS
M = 48                                             # fixture rows = fixture queries
N_WIDE = 4100                                      # >= 4 x chunk0_rows (512); 4100 % 32 = 4: a ragged last tile
N_ANYK = 65                                        # the fewest rows at which k = 65 is not clamped under the any-k threshold
FILL_SEED = 20261020
PART_OFFSETS = np.array([0, 64, 65, 322, N_WIDE], dtype=np.uint64)      # partitions of 64, 1, 257 and the rest
SENT = 0xFFFFFFFF
U64MAX = np.iinfo(np.uint64).max
INF = np.float32(np.inf)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def tails_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dot_tails_golden.npz"))


class Case:
    """One (dtype, dim): the wide corpus (its first 48 rows are the small one), the queries, the oracle's score matrix and the
    real reference's recorded diagonal.  Built on the CPU; the golden-diagonal assertion runs here, before any GPU call."""

    def __init__(self, orc, fixtures, tag, d):
        self.tag, self.dt, self.d = tag, TAGS[tag], d
        q, x32, x16, x8, sc = make_dot_inputs(d)
        fx = fixtures[0] if d in GOLDEN_DIMS else fixtures[1]
        assert bytes(fx[f"dot{d}_sha"]).hex() == sha(q, x32, x16, x8, sc), f"input drift for dim {d}: numpy stream changed?"
        self.recorded = fx[f"dot{d}_simd_{tag}"]
        self.queries = q
        fill, fill_sc = nvdb_amd.synth_corpus(FILL_SEED + d, 0, N_WIDE - M, d, self.dt)
        head = {"f32": x32, "f16": x16, "i8": x8}[tag]
        self.base = np.ascontiguousarray(np.concatenate([head, fill]))
        self.scales = np.ascontiguousarray(np.concatenate([sc, fill_sc])) if tag == "i8" else None
        self.S = np.stack([orc.scores(self.base, self.dt, q[i], self.scales) for i in range(M)])        # [48, N_WIDE]
        self.S.setflags(write=False)
        assert np.array_equal(bits(np.diagonal(self.S[:, :M])), self.recorded), (tag, d, "the oracle's diagonal is not the reference's")

    def rows(self, n):
        return self.base[:n], (self.scales[:n] if self.scales is not None else None)

    def upload(self, ctx, n):
        b, s = self.rows(n)
        ctx.upload_corpus(b, self.dt, s)

    def order(self, qi, rows):
        """Local rows `rows` in (score desc, id asc) order for query qi."""
        rows = np.asarray(rows, dtype=np.int64)
        return rows[np.lexsort((rows, -self.S[qi, rows]))]

    def topk(self, qi, rows, k):
        o = self.order(qi, rows)[:k]
        ids = np.full(k, U64MAX, dtype=np.uint64)
        sc = np.full(k, -np.inf, dtype=np.float32)
        ids[:len(o)], sc[:len(o)] = o.astype(np.uint64), self.S[qi, o]
        return ids, sc, len(o)

    def in_range(self, qi, rows, radius):
        rows = np.asarray(rows, dtype=np.int64)
        o = self.order(qi, rows[self.S[qi, rows] >= radius])
        return o.astype(np.uint64), self.S[qi, o]

    def assert_every_pair(self, ids, sc, n, nq, what):
        """A result that holds all n rows for the first nq queries: the oracle's order and bits; with every fixture query present,
        the diagonal of what the GPU returned against the real reference's recorded bits."""
        assert ids.shape == sc.shape == (nq, n), (what, ids.shape)
        for qi in range(nq):
            o = self.order(qi, np.arange(n))
            assert np.array_equal(ids[qi], o.astype(np.uint64)), (what, "ids", qi)
            assert same_bits(sc[qi], self.S[qi, o]), (what, "score bits", qi, sc[qi][:4], self.S[qi, o][:4])
        if nq == M:
            diag = np.array([sc[qi][ids[qi] == qi][0] for qi in range(M)], dtype=np.float32)
            assert np.array_equal(bits(diag), self.recorded), (what, "GPU diagonal is not the reference's recorded bits")


@pytest.fixture(scope="module")
def cases(oracle, golden, tails_golden):
    held = {}

    def get(tag, d):
        if (tag, d) not in held:
            held[(tag, d)] = Case(oracle, (golden, tails_golden), tag, d)
        return held[(tag, d)]
    return get


@pytest.fixture(scope="module")
def ctxs():
    """One context per dtype for the whole module; every test leaves the options as it found them."""
    held = {tag: nvdb_amd.HipContext(0) for tag in TAGS}
    yield held
    for c in held.values():
        c.close()


def probe_table(nq, nprobe):
    """Query q probes partitions q, q + 1, .. (mod 4): every partition meets groups of every size class as nq grows."""
    return np.array([[(q + j) % 4 for j in range(nprobe)] for q in range(nq)], dtype=np.uint32)


def union(probe_row, offsets=PART_OFFSETS):
    return np.concatenate([np.arange(int(offsets[p]), int(offsets[p + 1]), dtype=np.int64) for p in sorted(set(int(p) for p in probe_row))])


# ------------------------------------------------------------------------------------------------------------ the routes
@pytest.mark.parametrize("tag", list(TAGS))
def test_exact_scan(ctxs, cases, tag):
    ctx = ctxs[tag]
    ctx.set_option("path", 1)
    try:
        for d in ALL_DIMS:
            c = cases(tag, d)
            c.upload(ctx, M)
            for nq in (1, 2, 4, 9, 48):
                ids, sc = ctx.search_batch(c.queries[:nq], M)
                assert ctx.stats()["path"] == 1, (tag, d, nq, ctx.stats())
                c.assert_every_pair(ids, sc, M, nq, f"exact scan {tag} dim {d} nq {nq}")
    finally:
        ctx.set_option("path", 0)


@pytest.mark.parametrize("tag", list(TAGS))
def test_anyk(ctxs, cases, tag):
    ctx = ctxs[tag]
    for d in ALL_DIMS:
        c = cases(tag, d)
        c.upload(ctx, M)                                       # 48 rows: k = 65 clamps to 48 before the route is chosen -> the exact scan
        ids, sc = ctx.search_batch(c.queries, 65)
        assert ctx.stats()["path"] == 1, (tag, d, ctx.stats())
        c.assert_every_pair(ids, sc, M, M, f"k = 65 on 48 rows {tag} dim {d}")
        c.upload(ctx, N_ANYK)                                  # 65 rows: k = 65 = n, the any-k path, every pair comes back
        for nq in (1, 3, 48):
            ids, sc = ctx.search_batch(c.queries[:nq], 65)
            assert ctx.stats()["path"] == 3, (tag, d, nq, ctx.stats())
            c.assert_every_pair(ids, sc, N_ANYK, nq, f"any-k {tag} dim {d} nq {nq}")


@pytest.mark.parametrize("tag", list(TAGS))
def test_filter_and_rescore(ctxs, cases, tag):
    ctx = ctxs[tag]
    ctx.set_option("path", 2)
    try:
        for d in ALL_DIMS:
            c = cases(tag, d)
            c.upload(ctx, N_WIDE)
            if tag == "i8" and d > 1536:                       # no int8 filter beyond 1536: the forced route is refused, not rerouted
                with pytest.raises(nvdb_amd.NvdbError) as e:
                    ctx.search_batch(c.queries, 10)
                assert e.value.status == 3, e.value
                continue
            for k in (10, 64):
                want = [c.topk(qi, np.arange(N_WIDE), k) for qi in range(M)]
                got = {}
                for r8 in (2, 1, 0):
                    ctx.set_option("rescore8", r8)
                    ids, sc = ctx.search_batch(c.queries, k)
                    st = ctx.stats()
                    what = f"filter {tag} dim {d} k {k} rescore8 {r8}"
                    assert st["path"] == 2 and st["bound_violations"] == 0 and st["overflow_queries"] == 0, (what, st)
                    assert ids.shape == (M, k), what
                    for qi in range(M):
                        assert_topk_equal(ids[qi], sc[qi], want[qi][0], want[qi][1], score_of=lambda i, qi=qi: c.S[qi, i], what=f"{what} q{qi}")
                    got[r8] = (ids, sc)
                for r8 in (1, 0):
                    assert np.array_equal(got[r8][0], got[2][0]) and same_bits(got[r8][1], got[2][1]), (tag, d, k, "rescore8", r8, "differs from 2")
    finally:
        ctx.set_option("rescore8", 2)
        ctx.set_option("path", 0)


@pytest.mark.parametrize("tag", list(TAGS))
def test_range_exact_route(ctxs, cases, tag):
    ctx = ctxs[tag]
    ctx.set_option("path", 1)
    try:
        for d in ALL_DIMS:
            c = cases(tag, d)
            c.upload(ctx, M)
            rows = np.arange(M)
            tenth = np.array([c.S[qi, c.order(qi, rows)[9]] for qi in range(M)], dtype=np.float32)
            for radius in (tenth, np.full(M, -INF)):
                lims, ids, sc = ctx.range_search(c.queries, radius)
                assert ctx.stats()["path"] == 6, (tag, d, ctx.stats())
                for qi in range(M):
                    eid, esc = c.in_range(qi, rows, radius[qi])
                    lo, hi = int(lims[qi]), int(lims[qi + 1])
                    assert hi - lo == len(eid) >= 10, (tag, d, qi, hi - lo, len(eid))
                    assert np.array_equal(ids[lo:hi], eid) and same_bits(sc[lo:hi], esc), (tag, d, qi, "range, exact route")
    finally:
        ctx.set_option("path", 0)


@pytest.mark.parametrize("tag", list(TAGS))
def test_probe(ctxs, cases, tag):
    ctx = ctxs[tag]
    plane = np.random.RandomState(99).rand(1, N_WIDE) < 0.5
    for d in ALL_DIMS:
        c = cases(tag, d)
        c.upload(ctx, N_WIDE)
        ctx.set_partitions(PART_OFFSETS)
        for nprobe in (1, 3):
            for nq in (1, 9, 48):
                probe = probe_table(nq, nprobe)
                ids, sc, counts = ctx.search_partitions(c.queries[:nq], 10, probe)
                assert ctx.stats()["path"] == 4, (tag, d, ctx.stats())
                for qi in range(nq):
                    eid, esc, ecnt = c.topk(qi, union(probe[qi]), 10)
                    what = (tag, d, "search_partitions", nprobe, nq, qi)
                    assert counts[qi] == ecnt and np.array_equal(ids[qi], eid) and same_bits(sc[qi], esc), (what, ids[qi], eid)
        probe = probe_table(9, 3)
        radius = np.array([c.S[qi, c.order(qi, union(probe[qi]))[9]] for qi in range(9)], dtype=np.float32)
        lims, ids, sc = ctx.range_search_partitions(c.queries[:9], radius, probe)
        assert ctx.stats()["path"] == 7, (tag, d, ctx.stats())
        for qi in range(9):
            eid, esc = c.in_range(qi, union(probe[qi]), radius[qi])
            lo, hi = int(lims[qi]), int(lims[qi + 1])
            assert hi - lo == len(eid) >= 10 and np.array_equal(ids[lo:hi], eid) and same_bits(sc[lo:hi], esc), (tag, d, "range_search_partitions", qi)
        ids, sc, counts = ctx.search_partitions_anyk(c.queries[:9], 100, probe)
        assert ctx.stats()["path"] == 8, (tag, d, ctx.stats())
        for qi in range(9):
            eid, esc, ecnt = c.topk(qi, union(probe[qi]), 100)
            assert counts[qi] == ecnt == 100 and np.array_equal(ids[qi], eid) and same_bits(sc[qi], esc), (tag, d, "search_partitions_anyk", qi)
        probe = probe_table(M, 3)
        ctx.set_row_masks(plane)
        ids, sc, counts = ctx.search_partitions_masked(c.queries, 10, probe)
        assert ctx.stats()["path"] == 4, (tag, d, ctx.stats())
        for qi in range(M):
            rows = union(probe[qi])
            eid, esc, ecnt = c.topk(qi, rows[plane[0, rows]], 10)
            assert counts[qi] == ecnt and np.array_equal(ids[qi], eid) and same_bits(sc[qi], esc), (tag, d, "search_partitions_masked", qi)
    ctx.set_row_masks(None)


@pytest.mark.parametrize("tag", list(TAGS))
def test_adopted_unpadded(cases, tag):
    """The corpus is a torch tensor of exactly 48 x dim elements: the last row's tail is the end of what was asked for."""
    import torch
    offsets = np.array([0, 1, 17, M], dtype=np.uint64)
    ctx = nvdb_amd.HipContext(0)
    try:
        ctx.set_option("path", 1)
        for d in GOLDEN_TAIL_DIMS:
            c = cases(tag, d)
            b, s = c.rows(M)
            t_rows = torch.from_numpy(b.view(np.int16) if tag == "f16" else b).cuda()
            t_scales = torch.from_numpy(s).cuda() if s is not None else None
            assert t_rows.numel() == M * d
            ctx.adopt_corpus(t_rows.data_ptr(), M, d, c.dt, t_scales.data_ptr() if t_scales is not None else None)
            ids, sc = ctx.search_batch(c.queries, M)
            assert ctx.stats()["path"] == 1, (tag, d, ctx.stats())
            c.assert_every_pair(ids, sc, M, M, f"adopted exact scan {tag} dim {d}")
            ctx.set_partitions(offsets)
            probe = np.array([[2, qi % 2] for qi in range(M)], dtype=np.uint32)
            ids, sc, counts = ctx.search_partitions(c.queries, 10, probe)
            assert ctx.stats()["path"] == 4, (tag, d, ctx.stats())
            for qi in range(M):
                eid, esc, ecnt = c.topk(qi, union(probe[qi], offsets), 10)
                assert counts[qi] == ecnt and np.array_equal(ids[qi], eid) and same_bits(sc[qi], esc), (tag, d, "adopted search_partitions", qi)
    finally:
        ctx.close()


@pytest.mark.parametrize("tag", ["f16", "f32"])
def test_refine(ctxs, cases, oracle, tag):
    ctx = ctxs[tag]
    rs = np.random.RandomState(7)
    cand = np.stack([rs.permutation(M) for _ in range(M)]).astype(np.uint32)
    try:
        for d in REFINE_DIMS:
            c = cases(tag, d)
            c.upload(ctx, N_WIDE)
            oid, odist = oracle.refine(c.base[:M], c.dt, c.queries, cand, 10, mode=0)
            for v in (0, 1):
                ctx.set_option("refine_v2", v)
                ids, dist = ctx.refine_l2_topk(c.queries, cand, 10)
                assert np.array_equal(ids, oid), (tag, d, "refine_v2", v, "ids", np.argwhere(ids != oid)[:4])
                assert same_bits(dist, odist), (tag, d, "refine_v2", v, "distance bits", np.argwhere(bits(dist) != bits(odist))[:4])
    finally:
        ctx.set_option("refine_v2", 2)
