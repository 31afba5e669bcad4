"""The masked flat top-k (nvdb_hip_search_batch_masked / HipContext.search_masked) on the MFMA filter route, forced with option
path = 2, against the oracle.

The checker is tests/test_gpu_row_masks.py's: the oracle's full score vector per query, restricted to the rows that are live in the
query's plane, top-k by (score desc, id asc): ids, score BITS and counts must be equal -- no tolerance, no excluded case.  Every
call is also compared byte for byte with the same call on the partition scan (path = 1): the result does not depend on the route.
Corpora are small (20037 rows: a ragged tail behind the last whole tile); oracle score vectors are computed once per (corpus, query)
and shared by the builds that hold the same corpus."""
import numpy as np
import pytest

import nvdb_amd
import pyoracle as po

pytestmark = pytest.mark.gpu

N, ROW_BASE, SEED = 20037, 1_000_003, 20250611
F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8
SENT = 0xFFFFFFFF
U64MAX = np.iinfo(np.uint64).max
K = 10
NQ_MAX = 1030


def make_planes():
    rs = np.random.RandomState(78)
    planes = [np.ones(N, bool), np.zeros(N, bool)]                      # 0 all live, 1 all dead
    for r in (0, 31, 32, 63, 64, N - 1):                                # 2 .. 7: exactly one live row at a word / tile / corpus edge
        p = np.zeros(N, bool)
        p[r] = True
        planes.append(p)
    planes.append(np.arange(N) % 2 == 0)                                # 8 alternating
    planes.append(rs.rand(N) < 0.5)                                     # 9 random 50 %
    planes.append(rs.rand(N) < 0.01)                                    # 10 random 1 %: with k = 64 most prefixes hold fewer than k live rows
    for cnt in (K - 1, K):                                              # 11, 12: exactly k - 1 / k live rows in the whole corpus
        p = np.zeros(N, bool)
        p[rs.choice(N, cnt, replace=False)] = True
        planes.append(p)
    planes.append(np.ones(N, bool))                                     # 13 scratch (test_sticky_state edits it and puts it back)
    return np.stack(planes)


PLANES = make_planes()
NMASKS = len(PLANES)
ALL_LIVE, ALL_DEAD, ALTERNATING, HALF, SPARSE, KM1, KEQ, SCRATCH = 0, 1, 8, 9, 10, 11, 12, 13

# build -> (corpus, options set before the upload, what the filter streams)
BUILDS = {
    "f16": ("f16_768", dict(q8_shadow=0), "f16"),
    "shadow": ("f16_768", dict(q8_shadow=1), "shadow"),
    "i8": ("i8_768", dict(), "i8"),
    "f32": ("f32_768", dict(f32_shadow=1, q8_shadow=0), "f16"),
    "f16_1536": ("f16_1536", dict(q8_shadow=0), "f16"),
}
CORPORA = {"f16_768": (F16, 768), "i8_768": (I8, 768), "f32_768": (F32, 768), "f16_1536": (F16, 1536)}


def topk(scores, rows, k):
    s = scores[rows]
    order = np.lexsort((rows, -s))[:k]
    ids = np.full(k, U64MAX, dtype=np.uint64)
    sc = np.full(k, -np.inf, dtype=np.float32)
    ids[:len(order)] = rows[order].astype(np.uint64) + ROW_BASE
    sc[:len(order)] = s[order]
    return ids, sc, min(k, len(rows))


class Corpus:
    """Rows, queries and the oracle's score vectors (lazily, once per query)."""

    def __init__(self, orc, dtype, dim, base=None, scales=None):
        self.orc, self.dtype, self.dim = orc, dtype, dim
        if base is None:
            base, scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
        self.base, self.scales = base, scales
        self.queries = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ_MAX, dim)
        self._scores = {}

    def scores(self, q):
        if q not in self._scores:
            self._scores[q] = self.orc.scores(self.base, self.dtype, self.queries[q], self.scales)
        return self._scores[q]


class Build:
    def __init__(self, corpus, opts, streams, planes=PLANES):
        self.corpus, self.streams, self.planes = corpus, streams, planes
        self.ctx = nvdb_amd.HipContext(0)
        for key, v in opts.items():
            self.ctx.set_option(key, v)
        self.ctx.upload_corpus(corpus.base, corpus.dtype, corpus.scales, ROW_BASE)
        self.ctx.set_row_masks(planes)
        self.ctx.set_option("path", 2)

    def both_routes(self, queries, k, mo):
        got = self.ctx.search_masked(queries, k, mo)
        st = self.ctx.stats()
        self.ctx.set_option("path", 1)
        try:
            scan = self.ctx.search_masked(queries, k, mo)
            assert self.ctx.stats()["path"] == 4
        finally:
            self.ctx.set_option("path", 2)
        return got, st, scan

    def check(self, nq, k, mask_of, planes=None, oracle_on=None, clean=True):
        """oracle_on: the queries compared with the oracle (None: all of them); every query is compared with the scan."""
        planes = self.planes if planes is None else planes
        mo = np.asarray(mask_of, dtype=np.uint32)
        got, st, scan = self.both_routes(self.corpus.queries[:nq], k, mo)
        assert st["path"] == 2, st
        if clean:
            assert st["overflow_queries"] == 0 and st["bound_violations"] == 0, st
            assert self.ctx.shadow_info()["last_filter"] == self.streams
        for a, b in zip(got, scan):
            assert a.tobytes() == b.tobytes()
        ids, sc, counts = got
        for q in (range(nq) if oracle_on is None else oracle_on):
            m = int(mo[q])
            live = np.arange(N) if m == SENT else np.flatnonzero(planes[m])
            eid, esc, ecnt = topk(self.corpus.scores(q), live, k)
            assert counts[q] == ecnt, (q, m, counts[q], ecnt)
            assert np.array_equal(ids[q], eid), (q, m, ids[q], eid)
            assert np.array_equal(sc[q].view(np.uint32), esc.view(np.uint32)), (q, m, sc[q], esc)
        return got, st


@pytest.fixture(scope="module")
def corpora(oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Corpus(oracle, *CORPORA[name])
        return made[name]
    return get


@pytest.fixture(scope="module")
def builds(corpora):
    made = {}

    def get(name):
        if name not in made:
            cname, opts, streams = BUILDS[name]
            made[name] = Build(corpora(cname), opts, streams)
        return made[name]
    yield get
    for b in made.values():
        b.ctx.close()


def cycle(nq, shift=0):
    """Every plane and the "no mask" number in turn."""
    m = (np.arange(nq) + shift) % (NMASKS + 1)
    return np.where(m == NMASKS, SENT, m).astype(np.uint32)


@pytest.mark.parametrize("build,nq", [(b, nq) for b in BUILDS for nq in (1, 9)] + [("shadow", 200), ("i8", 200), ("f16", 200)])
def test_route_and_planes(builds, build, nq):
    """Fails without the route: the parent reports path 4 for this call."""
    b = builds(build)
    if build == "shadow":
        assert b.ctx.shadow_info()["resident"]
    b.check(nq, K, cycle(nq, 9 if nq == 1 else 0))          # nq = 1: the random 50 % plane; else every plane and "no mask" in one batch
    if nq == 9:
        b.check(9, K, cycle(9, 9))                          # ... the second half of the planes: 1 %, exactly k - 1 / k live rows, no mask
        b.check(9, 64, np.array([SPARSE, HALF, SPARSE, SENT, KM1, KEQ, ALL_DEAD, SPARSE, 7], dtype=np.uint32))   # k = 64 under 1 %: most prefixes hold < k live rows
        b.check(9, 1, cycle(9, 3))
        b.check(9, K, np.full(9, HALF, dtype=np.uint32))    # one plane, one group


def test_counts_and_padding(builds):
    b = builds("f16")
    mo = np.array([ALL_DEAD, KM1, KEQ, 2, 7, SENT], dtype=np.uint32)
    (ids, sc, counts), _ = b.check(6, K, mo)
    assert counts.tolist() == [0, K - 1, K, 1, 1, K]
    assert (ids[0] == U64MAX).all() and np.isneginf(sc[0]).all() and ids[1, K - 1] == U64MAX and np.isneginf(sc[1, K - 1])
    assert ids[3, 0] == ROW_BASE and ids[4, 0] == ROW_BASE + N - 1 and (ids[3, 1:] == U64MAX).all()


def test_two_sub_batches(builds):
    """nq = 1030: a sub-batch of 1024 and one of 6; every query against the scan, a sample against the oracle."""
    b = builds("f16")
    sample = list(range(0, 1030, 64)) + list(range(1020, 1030))
    b.check(1030, K, cycle(1030), oracle_on=sample)


def test_mask_of_null_is_plane_zero(builds):
    b = builds("f16")
    got = b.ctx.search_masked(b.corpus.queries[:9], K, None)
    assert b.ctx.stats()["path"] == 2
    want = b.ctx.search_masked(b.corpus.queries[:9], K, np.zeros(9, dtype=np.uint32))
    for a, w in zip(got, want):
        assert a.tobytes() == w.tobytes()
    b.check(9, K, np.zeros(9, dtype=np.uint32))


def test_adopted_corpus_with_a_ragged_tail(corpora):
    """An adopted corpus is not padded to whole tiles: the filter pass scores the rows behind the last whole tile exactly."""
    import torch
    cor = corpora("f16_768")
    dev = torch.from_numpy(cor.base.view(np.int16)).cuda()
    b = Build.__new__(Build)
    b.corpus, b.streams, b.planes = cor, "f16", PLANES
    b.ctx = nvdb_amd.HipContext(0)
    try:
        b.ctx.set_option("q8_shadow", 0)
        b.ctx.adopt_corpus(dev.data_ptr(), N, cor.dim, F16, None, ROW_BASE)
        b.ctx.set_row_masks(PLANES)
        b.ctx.set_option("path", 2)
        only_tail = np.zeros(N, bool)
        only_tail[N - 5:] = True                            # live rows in the ragged tail alone
        planes = PLANES.copy()
        planes[SCRATCH] = only_tail
        b.ctx.set_row_masks(planes)
        b.check(9, K, np.array([SCRATCH, HALF, 7, SENT, SCRATCH, ALL_LIVE, ALTERNATING, SPARSE, SCRATCH], dtype=np.uint32), planes=planes)
    finally:
        b.ctx.close()
        del dev


@pytest.fixture(scope="module")
def planted(oracle, corpora):
    """The fp16 corpus with, per query 0 .. 3, its own vector planted as 2k rows that are DEAD in the query's plane -- k inside the
    bootstrap prefix (the first rows), k far beyond it -- and, for query 4 under the 50 % plane, three identical live rows whose
    score lands at ranks k - 1, k, k + 1, one in the first tile, one far beyond the prefix."""
    src = corpora("f16_768")
    base = src.base.copy()
    planes = [PLANES[HALF].copy() for _ in range(4)] + [PLANES[HALF].copy()]
    q16 = oracle.f32_to_f16(src.queries[:4])
    for q in range(4):
        rows = np.concatenate([np.arange(K) * 4 + q, 12000 + np.arange(K) * 7 + q])   # rows 0 .. 39 and 12000 ..
        base[rows] = q16[q]
        for p in planes[:4]:
            p[rows] = True                                  # live for the other queries: they must simply rank them
        planes[q][rows] = False
    cor = Corpus(oracle, F16, 768, base=base)
    cor.queries = src.queries
    # ties: the row at rank k - 1 among query 4's live rows, copied over a live row of the first tile and one beyond row 15000
    live = np.flatnonzero(planes[4])
    s = cor.scores(4)
    order = live[np.lexsort((live, -s[live]))]
    star = order[K - 2]
    low = [r for r in order[4 * K:] if 40 <= r < 64][0]
    high = [r for r in order[4 * K:] if r > 15000][0]
    base[low] = base[star]
    base[high] = base[star]
    cor._scores.clear()
    b = Build(cor, dict(q8_shadow=0), "f16", planes=np.stack(planes))
    yield b, sorted(int(r) for r in (star, low, high))
    b.ctx.close()


def test_adversarial_dead_rows(planted):
    """A bootstrap that ignored the mask would set the bar at the planted rows' score (the query's own norm), above every live row."""
    b, _ = planted
    (ids, sc, counts), _ = b.check(4, K, np.arange(4, dtype=np.uint32))
    assert (counts == K).all()
    (ids, sc, counts), _ = b.check(4, 64, np.arange(4, dtype=np.uint32))
    assert (counts == 64).all()
    # under "no mask" the planted rows are the answer
    (ids, _, _), _ = b.check(4, K, np.full(4, SENT, dtype=np.uint32))
    for q in range(4):
        assert set(int(i) - ROW_BASE for i in ids[q]) <= set(range(40)) | set(range(12000, 12000 + 7 * K + 4))


def test_ties_at_the_bar(planted):
    b, tied = planted
    mo = np.full(5, 4, dtype=np.uint32)
    (ids, sc, counts), _ = b.check(5, K, mo)
    got = [int(i) - ROW_BASE for i in ids[4]]
    assert got[K - 2:] == tied[:2] and tied[2] not in got, (got, tied)
    assert sc[4, K - 2] == sc[4, K - 1]
    (ids, _, _), _ = b.check(5, K + 1, mo)                  # one more: all three, by id
    assert [int(i) - ROW_BASE for i in ids[4]][K - 2:] == tied


def test_overflow_redoes_only_the_flagged_queries(builds):
    b = builds("f16")
    mo = np.array([ALL_LIVE, HALF, ALTERNATING] * 3, dtype=np.uint32)
    b.ctx.set_option("cand_cap", 64)
    try:
        _, st = b.check(9, 64, mo, clean=False)
        assert st["overflow_queries"] > 0 and st["bound_violations"] == 0, st
        assert st["rows_scanned"] < N * 9, st                # not a full scan of every query
        # a query the bootstrap answers (fewer than k live rows) is not flagged
        _, st = b.check(2, 64, np.array([KM1, KEQ], dtype=np.uint32), clean=False)
        assert st["overflow_queries"] == 0
    finally:
        b.ctx.set_option("cand_cap", 0)


@pytest.mark.parametrize("build", ["f16", "i8"])
def test_non_finite_query(builds, build):
    """A non-finite query element is flagged and served by the scan: no fault; that query's order is unspecified."""
    b = builds(build)
    q = b.corpus.queries[:6].copy()
    q[1, 5] = np.nan
    q[4, 700] = np.inf
    mo = np.array([HALF, HALF, SENT, ALTERNATING, ALL_LIVE, SPARSE], dtype=np.uint32)
    ids, sc, counts = b.ctx.search_masked(q, K, mo)
    st = b.ctx.stats()
    assert st["path"] == 2 and st["overflow_queries"] >= 2 and st["bound_violations"] == 0, st
    assert (counts[[0, 2, 3, 5]] == K).all()
    for i in (0, 2, 3, 5):
        m = int(mo[i])
        eid, esc, _ = topk(b.corpus.scores(i), np.arange(N) if m == SENT else np.flatnonzero(PLANES[m]), K)
        assert np.array_equal(ids[i], eid) and np.array_equal(sc[i].view(np.uint32), esc.view(np.uint32))


def test_sticky_state(builds):
    """A range search and an unmasked search_batch around the masked call return the same bytes; update_row_mask is seen."""
    b = builds("shadow")
    ctx, q = b.ctx, b.corpus.queries[:9]
    flat0 = ctx.search_batch(q, K)
    radius = flat0[1][:, -1].copy()
    rng0 = ctx.range_search(q, radius)
    b.check(9, K, cycle(9))
    flat1 = ctx.search_batch(q, K)
    rng1 = ctx.range_search(q, radius)
    for a, c in zip(flat0 + rng0, flat1 + rng1):
        assert a.tobytes() == c.tobytes()
    mo = np.full(9, SCRATCH, dtype=np.uint32)
    (ids, _, _), _ = b.check(9, K, mo)
    best = np.unique(ids[:, 0] - np.uint64(ROW_BASE))
    planes = PLANES.copy()
    planes[SCRATCH, best.astype(np.int64)] = False
    ctx.update_row_mask(SCRATCH, best, False)
    try:
        (ids2, _, _), _ = b.check(9, K, mo, planes=planes)
        assert not np.isin(ids2 - np.uint64(ROW_BASE), best).any()
    finally:
        ctx.update_row_mask(SCRATCH, best, True)
    b.check(9, K, mo)


def test_forced_route_without_a_filter_is_refused(oracle):
    """path = 2 on an fp32 corpus without its fp16 shadow: NVDB_ERR_UNSUPPORTED with the range search's message, nothing written."""
    base, _ = nvdb_amd.synth_corpus(SEED, 0, 3000, 128, F32)
    ctx = nvdb_amd.HipContext(0)
    try:
        ctx.set_option("f32_shadow", 0)
        ctx.set_option("q8_shadow", 0)
        ctx.upload_corpus(base, F32, None, 0)
        ctx.set_row_masks(1)
        ctx.set_option("path", 2)
        q = nvdb_amd.synth_rows_f32(SEED + 1, 0, 2, 128)
        ids = np.full((2, K), 7, dtype=np.uint64)
        sc = np.full((2, K), 7.0, dtype=np.float32)
        cnt = np.full(2, 7, dtype=np.uint32)
        assert ctx.lib.nvdb_hip_search_batch_masked(ctx.h, q.ctypes.data, 2, K, None, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None) == 3
        assert "MFMA filter path needs" in ctx.lib.nvdb_hip_last_error(ctx.h).decode()
        assert (ids == 7).all() and (sc == 7.0).all() and (cnt == 7).all()
        ctx.set_option("path", 0)                           # automatic: the scan, as before
        got = ctx.search_masked(q, K, None)
        assert ctx.stats()["path"] == 4 and (got[2] == K).all()
    finally:
        ctx.close()
