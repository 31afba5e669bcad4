"""In-place compaction (nvdb_hip_compact_rows / nvdb_hip_ivf_compact): every check is equality, no tolerance.

After a compaction on plane `live` the context must be what a fresh context is that uploaded base[live] with the same options:
rows, scales, searches on every route, the partition table, the other planes.  And across the call the unmasked searches after
must return, mapped through out_old_rows, what the masked searches returned before.  Shapes are tests/test_gpu_row_masks.py's."""
import ctypes as C

import numpy as np
import pytest

import nvdb_amd
import pyoracle as po
from test_gpu_row_masks import N, ROW_BASE, SEED, SIZES, OFFSETS, NPARTS, PLANES, HALF, SPARSE, ALTERNATING, U64MAX, topk

pytestmark = pytest.mark.gpu

F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8
SLABS = (64, 4096, None)                                    # None: the default.  At this N both the direct and the bounce route run
BLOCK = 9000


def make_planes():
    rs = np.random.RandomState(4242)
    out = {"all_live": np.ones(N, bool)}
    for name, r in (("row0_dead", 0), ("last_dead", N - 1)):
        p = np.ones(N, bool)
        p[r] = False
        out[name] = p
    p = np.ones(N, bool)
    p[np.minimum(np.arange(0, N, 64) + rs.randint(0, 64, size=(N + 63) // 64), N - 1)] = False
    out["one_dead_per_tile"] = p
    out["alternating"] = np.arange(N) % 2 == 0
    for r in (0, 31, 32, 63, 64, N - 1):                    # exactly one live row at a word / tile / corpus edge
        p = np.zeros(N, bool)
        p[r] = True
        out["only_%d" % r] = p
    out["random_half"] = rs.rand(N) < 0.5
    out["random_1pct"] = rs.rand(N) < 0.01
    p = np.ones(N, bool)
    p[N - BLOCK:] = False                                   # the block at the very end: its rows are the stale rows a bad pad would keep
    out["dead_block"] = p
    return out


LIVE = make_planes()
SEARCHED = ["row0_dead", "last_dead", "one_dead_per_tile", "alternating", "random_half", "random_1pct", "dead_block"]
CORPORA = [(F16, 768), (I8, 768), (F32, 768), (F16, 100), (F16, 7), (F32, 3), (I8, 5)]
_corpus = {}


def corpus(dtype, dim):
    if (dtype, dim) not in _corpus:
        _corpus[(dtype, dim)] = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
    return _corpus[(dtype, dim)]


def load(dtype, dim, rows=None, scales=None, slab=None):
    """A fresh context with the options of this file's corpora: the fp16 d = 768 one carries the q8 filter shadow, the f32 one its
    fp16 shadow (the default), int8 d = 5 the padded-dim shadow."""
    base, sc = corpus(dtype, dim)
    ctx = nvdb_amd.HipContext(0)
    if (dtype, dim) == (F16, 768):
        ctx.set_option("q8_shadow", 1)
    if slab is not None:
        ctx.set_option("compact_slab_rows", slab)
    ctx.upload_corpus(base if rows is None else rows, dtype, sc if rows is None else scales, ROW_BASE)
    return ctx


def live_rows(dtype, dim, live):
    base, sc = corpus(dtype, dim)
    return np.ascontiguousarray(base[live]), (np.ascontiguousarray(sc[live]) if sc is not None else None)


def as_f32(dtype, dim, rows):
    """Corpus rows as queries."""
    base, sc = corpus(dtype, dim)
    if dtype == F16:
        return base[rows].view(np.float16).astype(np.float32)
    if dtype == I8:
        return base[rows].astype(np.float32) * sc[rows, None]
    return base[rows].copy()


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ---- 1. the rows, the scales and the map, on every mover build and both routes ------------------------------------------------
@pytest.mark.parametrize("plane", list(LIVE))
@pytest.mark.parametrize("dtype,dim", CORPORA)
def test_rows_scales_and_map(dtype, dim, plane):
    live = LIVE[plane]
    want_rows, want_scales = live_rows(dtype, dim, live)
    for slab in SLABS:
        ctx = load(dtype, dim, slab=slab)
        try:
            ctx.set_row_masks(live[None])
            n_new, old = ctx.compact_rows(0)
            assert n_new == int(live.sum()) and np.array_equal(old, np.flatnonzero(live).astype(np.uint32))
            info = ctx.corpus_info()
            assert info["n"] == n_new and info["row_base"] == ROW_BASE and info["dim"] == dim and info["dtype"] == dtype
            rows, scales = ctx.download_rows(0, n_new)
            assert rows.tobytes() == want_rows.tobytes(), (slab, plane)
            if dtype == I8:
                assert scales.tobytes() == want_scales.tobytes()
            got = ctx.get_row_masks()
            assert got.shape == (1, (n_new + 31) // 32) and nvdb_amd.unpack_row_masks(got, n_new).all()
            assert n_new % 32 == 0 or (got[0, -1] >> np.uint32(n_new % 32)) == 0
        finally:
            ctx.close()


# ---- 2. + 3. searches: against a fresh upload of the live rows, against the oracle, against the masked searches before ---------
# d = 768 under every plane; the narrow corpora -- whose filters stream the padded-dim int8 shadow (int8 d = 5: 256-byte rows and
# its own scale buffer) or the padded fp16 shadow (fp16 d = 100 / 7, f32 d = 3) -- under the planes that delete the corpus' tail:
# path 2 and the range search then read the MOVED shadow and the padding behind its new end
SEARCH_GRID = [(dt, 768, pl) for dt in (F16, I8, F32) for pl in SEARCHED] + \
              [(dt, d, pl) for dt, d in ((I8, 5), (F16, 100), (F16, 7), (F32, 3)) for pl in ("last_dead", "random_half", "dead_block")]


@pytest.mark.parametrize("dtype,dim,plane", SEARCH_GRID)
def test_searches(oracle, dtype, dim, plane):
    live = LIVE[plane]
    base, sc = corpus(dtype, dim)
    dead_tail = np.flatnonzero(~live)[-3:]                  # rows deleted from the very end (where the plane has them there)
    queries = np.concatenate([nvdb_amd.synth_rows_f32(SEED + 1, 0, 6, dim), as_f32(dtype, dim, dead_tail)])
    nq = len(queries)
    all_parts = np.tile(np.arange(NPARTS, dtype=np.uint32), (nq, 1))
    one_part = (np.arange(nq, dtype=np.uint32) % NPARTS)[:, None].copy()
    ctx = load(dtype, dim)
    fresh = None
    try:
        ctx.set_partitions(OFFSETS)
        ctx.set_row_masks(live[None])
        before_flat = {k: ctx.search_masked(queries, k) for k in (10, 64)}
        before_parts = {(k, name): ctx.search_partitions_masked(queries, k, probe) for k in (10, 64) for name, probe in (("one", one_part), ("all", all_parts))}
        n_new, old = ctx.compact_rows(0)
        assert n_new % 64 != 0 and n_new == int(live.sum())
        rows, scales = live_rows(dtype, dim, live)
        fresh = load(dtype, dim, rows, scales)
        new_off = np.concatenate([[0], np.cumsum(live)])[OFFSETS.astype(np.int64)].astype(np.uint64)   # rank(OFFSETS)
        fresh.set_partitions(new_off)
        old64 = old.astype(np.uint64)

        def mapped(ids):
            out = ids.copy()
            ok = ids != U64MAX
            assert (ids[ok] >= ROW_BASE).all() and (ids[ok] < ROW_BASE + n_new).all()   # no id at or behind the new end
            out[ok] = old64[(ids[ok] - ROW_BASE).astype(np.int64)] + ROW_BASE
            return out

        scores = [oracle.scores(base, dtype, q, sc) for q in queries]
        for path in (1, 2):
            ctx.set_option("path", path)
            fresh.set_option("path", path)
            for k in (10, 100):
                ids, s = ctx.search_batch(queries, k)              # (every (path, k, plane) of the grid must succeed, on both contexts)
                same((ids, s), fresh.search_batch(queries, k))
                assert ctx.stats()["path"] == fresh.stats()["path"]
                if path == 2 and k == 10 and n_new >= 10000:
                    assert ctx.stats()["path"] == 2             # the filter route ran: it streamed the moved rows or their moved shadow
                assert ids.shape[1] == min(k, n_new)
                for q in range(nq):
                    eid, esc, ecnt = topk(scores[q], np.flatnonzero(live), k)
                    assert np.array_equal(mapped(ids[q]), eid[:ecnt]) and np.array_equal(s[q].view(np.uint32), esc[:ecnt].view(np.uint32)), (path, k, q)
            ids10, s10 = ctx.search_batch(queries, 10)
            lims, rid, rsc = ctx.range_search(queries, s10[:, 9])
            same((lims, rid, rsc), fresh.range_search(queries, s10[:, 9]))
            assert ctx.stats()["path"] == fresh.stats()["path"]
            for q in range(nq):
                cand = np.flatnonzero(live & (scores[q] >= s10[q, 9]))
                eid, esc, ecnt = topk(scores[q], cand, len(cand))
                a, b = int(lims[q]), int(lims[q + 1])
                assert b - a == ecnt and np.array_equal(mapped(rid[a:b]), eid) and np.array_equal(rsc[a:b].view(np.uint32), esc.view(np.uint32))
        ctx.set_option("path", 0)
        fresh.set_option("path", 0)
        # 3. the invariant across the call
        for k in (10, 64):
            bid, bsc, bcnt = before_flat[k]
            ids, s = ctx.search_batch(queries, k)
            ke = ids.shape[1]
            assert (bcnt == ke).all() and np.array_equal(mapped(ids), bid[:, :ke]) and np.array_equal(s.view(np.uint32), bsc[:, :ke].view(np.uint32))
            for name, probe in (("one", one_part), ("all", all_parts)):
                bid, bsc, bcnt = before_parts[(k, name)]
                ids, s, cnt = ctx.search_partitions(queries, k, probe)
                assert np.array_equal(cnt, bcnt) and np.array_equal(mapped(ids), bid) and np.array_equal(s.view(np.uint32), bsc.view(np.uint32)), (k, name)
                same((ids, s, cnt), fresh.search_partitions(queries, k, probe))            # the rewritten table == rank(OFFSETS)
    finally:
        ctx.close()
        if fresh is not None:
            fresh.close()


# ---- 4. the other planes ---------------------------------------------------------------------------------------------------------
def test_every_resident_plane_goes_through_the_map(oracle):
    dtype, dim = F16, 768
    base, _ = corpus(dtype, dim)
    live = PLANES[HALF]
    ctx = load(dtype, dim)
    try:
        ctx.set_row_masks(PLANES)
        n_new, old = ctx.compact_rows(HALF)
        assert n_new == int(live.sum())
        got = ctx.get_row_masks()
        assert got.shape == (len(PLANES), (n_new + 31) // 32)
        want = PLANES[:, live].copy()
        want[HALF] = True
        assert np.array_equal(got, nvdb_amd.pack_row_masks(want, n_new))                   # packed: the tail bits are 0 as well
        queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, 9, dim)
        mo = np.array([ALTERNATING, SPARSE, 0, 1, HALF, ALTERNATING, 9, 3, SPARSE], dtype=np.uint32)
        ids, sc, cnt = ctx.search_masked(queries, 10, mo)
        for q in range(9):
            s = oracle.scores(base, dtype, queries[q])
            eid, esc, ecnt = topk(s, np.flatnonzero(PLANES[mo[q]] & live), 10)
            ok = ids[q] != U64MAX
            back = ids[q].copy()
            back[ok] = old[(ids[q][ok] - ROW_BASE).astype(np.int64)].astype(np.uint64) + ROW_BASE
            assert cnt[q] == ecnt and np.array_equal(back, eid) and np.array_equal(sc[q].view(np.uint32), esc.view(np.uint32)), q
    finally:
        ctx.close()


# ---- 5. statuses ----------------------------------------------------------------------------------------------------------------
def test_statuses():
    import torch
    dtype, dim = F16, 100
    base, _ = corpus(dtype, dim)
    lib = nvdb_amd.load_library()
    out_n = C.c_uint64(7)
    old = np.full(N, 7, dtype=np.uint32)

    def call(ctx, mask):
        return lib.nvdb_hip_compact_rows(ctx.h, mask, C.byref(out_n), old.ctypes.data)

    def untouched():
        return out_n.value == 7 and (old == 7).all()
    ctx = load(dtype, dim)
    empty = nvdb_amd.HipContext(0)
    adopted = nvdb_amd.HipContext(0)
    try:
        assert call(empty, 0) == 4 and untouched()                                           # NVDB_ERR_NO_CORPUS
        assert call(ctx, 0) == 1 and untouched()                                             # no planes: NVDB_ERR_INVALID
        ctx.set_row_masks(np.stack([np.ones(N, bool), np.zeros(N, bool)]))
        assert call(ctx, 2) == 1 and untouched()                                             # mask >= nmasks
        q = nvdb_amd.synth_rows_f32(SEED + 1, 0, 4, dim)
        ref = ctx.search_batch(q, 10)
        assert call(ctx, 1) == 1 and untouched()                                             # the all-dead plane
        assert ctx.corpus_info()["n"] == N and ctx.get_row_masks().shape == (2, (N + 31) // 32)
        same(ctx.search_batch(q, 10), ref)                                                   # unchanged and still searchable
        assert call(ctx, 0) == 0 and out_n.value == N and np.array_equal(old, np.arange(N, dtype=np.uint32))   # all live: the identity map
        rows, _ = ctx.download_rows(0, N)
        assert rows.tobytes() == base.tobytes() and ctx.corpus_info()["n"] == N
        same(ctx.search_batch(q, 10), ref)
        out_n.value = 7
        old[:] = 7
        t = torch.from_numpy(base.view(np.int16)).cuda()
        adopted.adopt_corpus(t.data_ptr(), N, dim, dtype, None, ROW_BASE)
        adopted.set_row_masks(LIVE["alternating"][None])
        assert call(adopted, 0) == 3 and untouched()                                         # NVDB_ERR_UNSUPPORTED
        assert adopted.corpus_info()["n"] == N and np.array_equal(t.cpu().numpy().view(np.uint16), base)
        assert lib.nvdb_hip_set_option(ctx.h, b"compact_slab_rows", 100) == 1 and lib.nvdb_hip_set_option(ctx.h, b"compact_slab_rows", 0) == 1
    finally:
        for c in (ctx, empty, adopted):
            c.close()


# ---- 6. twice ----------------------------------------------------------------------------------------------------------------------
def test_two_compactions_compose():
    dtype, dim = I8, 768
    base, sc = corpus(dtype, dim)
    first = LIVE["random_half"]
    ctx = load(dtype, dim, slab=4096)
    try:
        ctx.set_row_masks(np.stack([first, LIVE["alternating"]]))
        n1, old1 = ctx.compact_rows(0)
        gone = np.array([0, 1, 63, 64, 65, n1 - 1, 5000, 5001, 5002], dtype=np.uint64)      # NEW row numbers
        ctx.update_row_mask(0, gone, False)
        model = np.ones(n1, bool)
        model[gone.astype(np.int64)] = False
        assert np.array_equal(nvdb_amd.unpack_row_masks(ctx.get_row_masks(), n1), np.stack([model, LIVE["alternating"][first]]))
        n2, old2 = ctx.compact_rows(0)
        assert n2 == n1 - len(gone) and np.array_equal(old2, np.flatnonzero(model).astype(np.uint32))
        both = old1[old2]                                                                    # the composition of the two maps
        rows, scales = ctx.download_rows(0, n2)
        assert rows.tobytes() == base[both].tobytes() and scales.tobytes() == sc[both].tobytes()
        assert np.array_equal(nvdb_amd.unpack_row_masks(ctx.get_row_masks(), n2), np.stack([np.ones(n2, bool), LIVE["alternating"][both]]))
    finally:
        ctx.close()


# ---- the index ----------------------------------------------------------------------------------------------------------------------
def test_ivf_compact():
    dtype, dim, nlists, nprobe = F16, 768, 37, 5
    rs = np.random.RandomState(99)
    src = load(dtype, dim)
    ivf = None
    try:
        cen = src.train_centroids(nlists, 2, 7)
        ivf = nvdb_amd.IvfIndex(src, cen)
        info = ivf.info()
        perm, off = info["perm"].copy(), info["offsets"].astype(np.int64)
        sizes = np.diff(off)
        whole = int(np.argmax(sizes > 0))                                                    # one whole list
        edge = int(np.flatnonzero(sizes > 2)[-1])                                            # the first and the last row of another
        assert whole != edge
        live = rs.rand(N) < 0.5                                                              # by ORIGINAL row
        live[perm[off[whole]:off[whole + 1]]] = False
        live[perm[off[edge]]] = False
        live[perm[off[edge + 1] - 1]] = False
        ivf.set_row_masks(1)
        ivf.update_row_mask(0, np.flatnonzero(~live), False)
        queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, 9, dim)
        zero = np.zeros(9, dtype=np.uint32)
        b_top = ivf.search_masked(queries, 10, nprobe, zero, want_probe=True)
        b_any = ivf.search_anyk(queries, 100, nprobe, zero, masked=True, want_probe=True)
        radius = b_top[1][:, 9].copy()
        b_rng = ivf.range_search(queries, radius, nprobe, zero, masked=True, want_probe=True)
        with pytest.raises(nvdb_amd.NvdbError) as e:                                       # a refused call leaves the index as it was
            ivf.compact(1)
        assert e.value.status == 1
        kept = ivf.info()
        assert kept["n"] == N and np.array_equal(kept["perm"], perm) and np.array_equal(kept["offsets"].astype(np.int64), off)
        same(ivf.search_masked(queries, 10, nprobe, zero, want_probe=True), b_top)
        n_new = ivf.compact(0)
        assert n_new == int(live.sum())
        same(ivf.search(queries, 10, nprobe, want_probe=True), b_top)
        same(ivf.search_anyk(queries, 100, nprobe, masked=False, want_probe=True), b_any)
        same(ivf.range_search(queries, radius, nprobe, masked=False, want_probe=True), b_rng)
        after = ivf.info()
        live_pos = live[perm]
        assert after["n"] == n_new and np.array_equal(after["perm"], perm[live_pos])
        want_off = np.concatenate([[0], np.cumsum(live_pos)])[off].astype(np.uint64)         # cumulative sum of the lists' live counts
        assert np.array_equal(after["offsets"], want_off) and want_off[whole] == want_off[whole + 1]
        assert ivf.ctx.corpus_info()["n"] == n_new
        assert ivf.compact(0) == n_new                                                      # no row dead: nothing changes
        again_info = ivf.info()
        assert np.array_equal(again_info["perm"], after["perm"]) and np.array_equal(again_info["offsets"], after["offsets"])
        # updates still address ORIGINAL rows; one that is gone is ignored
        perm2 = after["perm"]
        again = np.concatenate([perm2[[0, 1, n_new - 1]].astype(np.uint64), np.flatnonzero(~live)[:1].astype(np.uint64)])
        ivf.update_row_mask(0, again, False)
        model = ~np.isin(perm2, again)
        assert np.array_equal(nvdb_amd.unpack_row_masks(ivf.ctx.get_row_masks(), n_new)[0], model)
        live2 = live.copy()
        live2[again.astype(np.int64)] = False
        ids, sc, cnt = ivf.search_masked(queries, 10, nlists, zero)
        assert (ids[ids != U64MAX] >= ROW_BASE).all() and live2[(ids[ids != U64MAX] - ROW_BASE).astype(np.int64)].all() and (cnt == 10).all()
    finally:
        if ivf is not None:
            ivf.close()
        src.close()


# ---- the 2^32 seam --------------------------------------------------------------------------------------------------------------------
def test_rows_cross_the_4gib_seam():
    """fp16 d = 768: row 2 796 202 straddles byte 2^32.  50 000 tombstones below it and a block of 10 000 just above: rows cross the
    seam downwards, and the rows around the NEW seam and the last ones are the generator's rows at out_old_rows."""
    n, dim, seam, seed = 2_900_000, 768, 2_796_202, 77
    rs = np.random.RandomState(5)
    dead = np.concatenate([rs.choice(seam, 50_000, replace=False), np.arange(seam + 1, seam + 10_001)]).astype(np.uint64)
    ctx = nvdb_amd.HipContext(0)
    try:
        ctx.generate_corpus(seed, n, dim, F16)
        ctx.set_row_masks(1)
        ctx.update_row_mask(0, dead, False)
        n_new, old = ctx.compact_rows(0)
        assert n_new == n - 60_000 and n_new > seam + 1
        live = np.ones(n, bool)
        live[dead.astype(np.int64)] = False
        assert np.array_equal(old, np.flatnonzero(live).astype(np.uint32))
        for row0, cnt in ((seam - 1000, 2000), (n_new - 64, 64)):
            got, _ = ctx.download_rows(row0, cnt)
            for j in range(cnt):
                want, _ = nvdb_amd.synth_corpus(seed, int(old[row0 + j]), 1, dim, F16)
                assert got[j].tobytes() == want[0].tobytes(), (row0 + j, int(old[row0 + j]))
    finally:
        ctx.close()
