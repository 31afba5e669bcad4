"""The MFMA filters at the edge of their error bounds, on the GPU.

tests/filter_bound_cases.py builds, per (family, dim), a corpus whose exact k-th neighbour of one query has a filter value as far
under its score as the geometry allows while k + 8 rows just under it are overstated; tests/test_filter_bound_cpu.py asserts, from a
numpy model alone, how much of the granted band that uses.  Here every distinct filter kernel build (one (dim, batch) each, read off
the launch tables of nvdb_launch_f16.cpp / nvdb_launch_i8.cpp) searches those corpora on the filter route at three placements of the
planted rows, through the top-k, the range search and the masked flat top-k:

  * ids and score BITS equal the oracle's for every query of the batch (no tie exemption: the planted scores are strict),
  * stats.path == 2 (range: 5), no overflow, bound_violations == 0, and the victim at rank k,
  * "teeth": one placement per family again with the developer option debug_bound_pct = floor(80 x reached share) -- the run must
    NOT come back clean (NVDB_ERR_INTERNAL with bound_violations > 0, or ids that differ), or the case proves nothing.

The other queries of a batch are random unit rows (14 distinct ones, repeated), so every lane and wave is busy; the adversarial query
sits in the first and in the last wave.  Oracle score vectors are computed once per (family, dim) and permuted with the rows."""
import numpy as np
import pytest

import filter_bound_cases as fb
import nvdb_amd
import pyoracle as po
from test_gpu_range import expected as range_expected

pytestmark = pytest.mark.gpu

K, N = fb.K, fb.N
NF = 14
SEED = 20251019
DT = {"f16": (nvdb_amd.DT_F16, po.DT_F16), "f32": (nvdb_amd.DT_F32, po.DT_F32), "i8": (nvdb_amd.DT_I8, po.DT_I8)}
UPLOAD_OPTS = {"F16": dict(q8_shadow=0), "F32": dict(f32_shadow=1, q8_shadow=0), "I8Q": dict(), "I8LO": dict(), "SH8": dict(q8_shadow=1)}
STREAMS = {"F16": "f16", "F32": "f16", "I8Q": "i8", "I8LO": "i8", "SH8": "shadow"}
DEFAULTS = dict(i8_dense8=1, shadow_exact_thr=1, tile_permute=1, path=0, debug_bound_pct=100)
NVDB_ERR_INTERNAL = 5


def variants(family, dim):
    """(batch, options) per distinct filter kernel build of the shape."""
    if family == "F16":
        return [(1, {}), (64, {}), (300, {})] if dim == 768 else [(300, {})]
    if family in ("I8Q", "I8LO"):
        return [(64, {}), (300, dict(i8_dense8=1)), (300, dict(i8_dense8=0))] if dim == 768 else [(300, {})]
    if family == "SH8":
        return [(300, dict(shadow_exact_thr=1)), (300, dict(shadow_exact_thr=0))]
    return [(64, {})]


class Bench:
    """One (family, dim): the case, the batch's distinct queries (0: the adversarial one) and their oracle scores by canonical id."""

    def __init__(self, oracle, family, dim):
        self.case = c = fb.build(family, dim)
        self.family, self.dim = family, dim
        self.dt, odt = DT[c.dtype]
        self.distinct = np.ascontiguousarray(np.vstack([c.query[None, :], nvdb_amd.synth_rows_f32(SEED + dim, 0, NF, dim)]))
        rows = c.rows.view(np.uint16) if c.dtype == "f16" else c.rows
        self.S = np.stack([oracle.scores(rows, odt, q, c.scales) for q in self.distinct])
        # the oracle ranks the planted neighbourhood as the builder's fp64 does
        o = np.lexsort((np.arange(N), -self.S[0].astype(np.float64)))
        assert np.array_equal(o[:K], c.expected) and len(np.unique(self.S[0][o[:K + 9]])) == K + 9

    def batch(self, nq):
        """Which distinct query sits where: the adversarial one first (wave 0) and last (the last wave)."""
        idx = 1 + (np.arange(nq) - 1) % NF
        idx[0] = idx[nq - 1] = 0
        return idx

    def placed(self, kind):
        pos = fb.placement(kind)
        c = self.case
        rows = fb.permuted(c.rows, pos)
        S = np.empty_like(self.S)
        S[:, pos] = self.S
        top = np.stack([np.lexsort((np.arange(N), -s.astype(np.float64)))[:K] for s in S])
        return pos, rows.view(np.uint16) if c.dtype == "f16" else rows, fb.permuted(c.scales, pos) if c.scales is not None else None, S, top


@pytest.fixture(scope="module")
def ctx_dev():
    c = nvdb_amd.HipContext(0, dev=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def benches(oracle):
    made = {}

    def get(family, dim):
        if (family, dim) not in made:
            for key in [k for k in made if k[1] != 768]:       # the d = 768 cases come back for the masked route and the short bounds
                del made[key]
                fb.drop(*key)
            made[(family, dim)] = Bench(oracle, family, dim)
        return made[(family, dim)]
    return get


def upload(ctx, b, rows, scales):
    for key, v in {**DEFAULTS, **UPLOAD_OPTS[b.family]}.items():
        ctx.set_option(key, v)
    ctx.upload_corpus(rows, b.dt, scales)
    if b.family == "SH8":
        assert ctx.shadow_info()["resident"]


def check_topk(ctx, b, pos, S, top, nq, what):
    idx = b.batch(nq)
    ids, sc = ctx.search_batch(b.distinct[idx], K)
    st = ctx.stats()
    assert st["path"] == 2 and st["overflow_queries"] == 0 and st["bound_violations"] == 0, (what, st)
    sh = ctx.shadow_info()
    assert sh["last_filter"] == STREAMS[b.family] and not sh["demoted"], (what, sh)
    want = top[idx]
    assert np.array_equal(ids, want.astype(np.uint64)), (what, "ids", np.flatnonzero(np.any(ids != want.astype(np.uint64), axis=1))[:8])
    want_sc = np.take_along_axis(S[idx], want, axis=1)
    assert np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32)), (what, "score bits")
    for q in {0, nq - 1}:                                      # the adversarial query: the tops, then the victim at rank k
        assert ids[q, K - 1] == pos[fb.VICTIM] and set(ids[q, :K - 1]) == set(pos[fb.TOPS]), (what, q, ids[q])


def check_range(ctx, b, pos, S, top, nq, what):
    """radius = each query's exact k-th best score (the adversarial query: the victim's): the victim is in, every decoy is out."""
    idx = b.batch(nq)
    Sq = S[idx]
    radius = np.take_along_axis(Sq, top[idx][:, K - 1:K], axis=1)[:, 0].copy()
    ctx.set_option("path", 2)
    lims, ids, sc = ctx.range_search(b.distinct[idx], radius)
    st = ctx.stats()
    assert st["path"] == 5 and st["overflow_queries"] == 0 and st["bound_violations"] == 0, (what, st)
    el, ei, es = range_expected(Sq, radius)
    assert np.array_equal(lims, el), (what, "lims")
    assert np.array_equal(ids, ei), (what, "ids")
    assert np.array_equal(sc.view(np.uint32), es.view(np.uint32)), (what, "score bits")
    for q in {0, nq - 1}:
        got = set(ids[int(lims[q]):int(lims[q + 1])])
        assert len(got) == K and pos[fb.VICTIM] in got and not (got & set(pos[fb.DECOYS])), (what, q)


@pytest.mark.parametrize("family,dim", fb.CASES, ids=[f"{f}-{d}" for f, d in fb.CASES])
def test_every_build_keeps_the_victim_at_the_edge_of_the_band(ctx_dev, benches, family, dim):
    b = benches(family, dim)
    ctx = ctx_dev
    try:
        for kind in (0, 1, 2):
            pos, rows, scales, S, top = b.placed(kind)
            upload(ctx, b, rows, scales)
            # placement 1: tiles stream in storage order, so the decoys at the front ARE the bootstrap's and the bar is at its
            # tightest when the victim's partial last tile streams
            ctx.set_option("tile_permute", 0 if kind == 1 else 1)
            for nq, opts in variants(family, dim):
                for key, v in opts.items():
                    ctx.set_option(key, v)
                ctx.set_option("path", 2)
                check_topk(ctx, b, pos, S, top, nq, f"{family}-{dim} placement {kind} nq {nq} {opts}")
                if kind == 0:
                    check_range(ctx, b, pos, S, top, min(nq, 64), f"{family}-{dim} range nq {nq} {opts}")
    finally:
        for key, v in DEFAULTS.items():
            ctx.set_option(key, v)


def test_masked_flat_route_keeps_the_victim(ctx_dev, benches):
    """nvdb_hip_search_batch_masked on the filter route (path = 2, as tests/test_gpu_masked_filter.py forces it): an all-live plane
    and a plane that kills the decoys; the bar there is one bound under an exact score, so the victim uses `share_range` of it."""
    b = benches("F16", 768)
    ctx = ctx_dev
    nq = 64
    pos, rows, scales, S, top = b.placed(0)
    planes = np.ones((2, N), dtype=bool)
    planes[1, pos[fb.DECOYS]] = False
    idx = b.batch(nq)
    mask_of = (np.arange(nq) % 2).astype(np.uint32)
    mask_of[0], mask_of[nq - 1] = 0, 1
    try:
        upload(ctx, b, rows, scales)
        ctx.set_row_masks(planes)
        ctx.set_option("path", 2)
        ids, sc, counts = ctx.search_masked(b.distinct[idx], K, mask_of)
        st = ctx.stats()
        assert st["path"] == 2 and st["overflow_queries"] == 0 and st["bound_violations"] == 0, st
        for q in range(nq):
            live = np.flatnonzero(planes[mask_of[q]])
            s = S[idx[q]][live]
            order = live[np.lexsort((live, -s.astype(np.float64)))[:K]]
            assert counts[q] == K and np.array_equal(ids[q], order.astype(np.uint64)), (q, ids[q], order)
            assert np.array_equal(sc[q].view(np.uint32), S[idx[q]][order].view(np.uint32)), q
        for q in (0, nq - 1):
            assert ids[q, K - 1] == pos[fb.VICTIM]
    finally:
        for key, v in DEFAULTS.items():
            ctx.set_option(key, v)


# (family, dim, batch, options, placement).  I8LO runs placement 1: the first-stage test compares with the bar a row meets WHEN IT
# STREAMS, so qdelta is only at its edge when the decoys have already raised the bar (they are the bootstrap's) and the victim streams last;
# the band under tau is tested by the selects after every chunk, whatever the order.
TEETH = [("F16", 768, 300, {}, 0), ("I8Q", 768, 300, {}, 0), ("I8LO", 768, 300, {}, 1), ("SH8", 768, 300, dict(shadow_exact_thr=1), 0),
         ("SH8", 768, 300, dict(shadow_exact_thr=0), 0), ("F32", 768, 64, {}, 0)]


@pytest.mark.parametrize("family,dim,nq,opts,kind", TEETH, ids=[f"{f}-{d}-{'-'.join(map(str, o.values())) or 'default'}" for f, d, _, o, _ in TEETH])
def test_a_short_bound_does_not_come_back_clean(benches, family, dim, nq, opts, kind):
    """The same search with the corpus norms the query prep is handed cut to floor(80 x reached share) per cent (the share is the
    one tests/test_filter_bound_cpu.py asserts from the numpy model): the band no longer reaches the victim."""
    b = benches(family, dim)
    pct = fb.bound_pct(family, dim)
    pos, rows, scales, S, top = b.placed(kind)
    idx = b.batch(nq)
    ctx = nvdb_amd.HipContext(0, dev=True)                     # its own context: a violation is sticky
    try:
        upload(ctx, b, rows, scales)
        for key, v in {**opts, "tile_permute": 0 if kind == 1 else 1, "path": 2}.items():
            ctx.set_option(key, v)
        check_topk(ctx, b, pos, S, top, nq, f"{family}-{dim} before the short bound")
        ctx.set_option("debug_bound_pct", pct)
        try:
            ids, _ = ctx.search_batch(b.distinct[idx], K)
        except nvdb_amd.NvdbError as e:
            st = ctx.stats()
            assert e.status == NVDB_ERR_INTERNAL and st["bound_violations"] > 0, (e.status, str(e), st)
            outcome = f"NVDB_ERR_INTERNAL, bound_violations = {st['bound_violations']}"
        else:
            st = ctx.stats()
            differ = np.flatnonzero(np.any(ids != top[idx].astype(np.uint64), axis=1))
            assert len(differ) > 0, f"{family}-{dim}: clean at {pct} % of the bound -- the case has no teeth ({st})"
            assert {0, nq - 1} <= set(differ) and pos[fb.VICTIM] not in ids[0], (differ, ids[0])
            outcome = f"ids differ for queries {differ.tolist()[:4]} (the victim is gone), bound_violations = {st['bound_violations']}"
        print(f"\nteeth {family}-{dim} {opts}: share {b.case.share_topk:.4f}, debug_bound_pct {pct}: {outcome}")
    finally:
        ctx.set_option("debug_bound_pct", 100)
        ctx.close()
