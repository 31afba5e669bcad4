"""Which filter streams is decided per search, and nothing of one search's choice reaches the next: ONE context is driven through
the call sequences that share its workspace -- flat search (host and device API), range search, masked flat search on the filter
route -- while option q8_shadow flips the choice between the int8 shadow and the fp16 rows and option tile_permute flips the
tile order.

After every call: ids and score BITS equal the oracle's (flat: Oracle.flat_topk; range / masked: the oracle's full score vectors,
cut at the radius / restricted to the live rows), the statistics name the filter route with no list overflow and no bound
violation, and the context's shadow-state query names the filter the current options ask for.  The sequence runs forward on one
context and in reverse order on a fresh one; an int8 corpus of the same shape streams its own rows throughout.

Shapes: d = 256, 4133 rows (owned: padded to whole tiles, the last one ragged), k = 5; batches of 5 queries (the NB = 1 builds) and
130 (the NB = 2 builds, two query tiles for the fp16 rows).  The oracle's references are computed once per corpus."""
import numpy as np
import pytest

import nvdb_amd
import pyoracle as po

pytestmark = pytest.mark.gpu

N, D, K, SEED = 4133, 256, 5, 20261021
BATCHES = (5, 130)
U64MAX = np.iinfo(np.uint64).max
PATH_FLAT, PATH_RANGE = 2, 5                                            # nvdb_hip_scan_stats::path of the two filter routes


class Reference:
    """Corpus, queries, one live-row plane and what the oracle says about them."""

    def __init__(self, orc, dtype):
        self.dtype = dtype
        rows = nvdb_amd.synth_rows_f32(SEED, 0, N, D)
        self.base, self.scales = (orc.quantize_i8(rows) if dtype == po.DT_I8 else (orc.f32_to_f16(rows), None))
        self.queries = np.ascontiguousarray(nvdb_amd.synth_rows_f32(SEED + 1, 0, max(BATCHES), D))
        self.S = np.stack([orc.scores(self.base, dtype, q, self.scales) for q in self.queries])
        self.top_ids, self.top_sc = orc.flat_topk(self.base, dtype, self.queries, K, self.scales)
        self.live = np.random.RandomState(7).rand(N) < 0.5
        # radius: every query's 10th best score -- the boundary row and its ties are hit exactly
        self.radius = np.sort(self.S, axis=1)[:, -10].astype(np.float32)

    def range_expected(self, nq):
        lims, ids, sc = np.zeros(nq + 1, np.uint64), [], []
        for q in range(nq):
            rows = np.flatnonzero(self.S[q] >= self.radius[q])
            s = self.S[q][rows]
            order = np.lexsort((rows, -(s + np.float32(0.0))))          # score desc (+-0 equal), id asc
            ids.append(rows[order].astype(np.uint64))
            sc.append(s[order])
            lims[q + 1] = lims[q] + np.uint64(len(rows))
        return lims, np.concatenate(ids), np.concatenate(sc)

    def masked_expected(self, nq):
        rows = np.flatnonzero(self.live)
        ids, sc = np.empty((nq, K), np.uint64), np.empty((nq, K), np.float32)
        for q in range(nq):
            s = self.S[q][rows]
            order = np.lexsort((rows, -s))[:K]
            ids[q], sc[q] = rows[order], s[order]
        return ids, sc


@pytest.fixture(scope="module")
def refs(oracle):
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = Reference(oracle, dtype)
        return made[dtype]
    return get


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


class Driver:
    """One context; every step checks its results against the oracle and the reported filter against the options in force."""

    def __init__(self, ref, nq):
        self.ref, self.nq, self.q = ref, nq, ref.queries[:nq]
        self.ctx = nvdb_amd.HipContext(0)
        self.ctx.set_option("q8_shadow", 1)
        self.ctx.upload_corpus(ref.base, ref.dtype, ref.scales)
        self.ctx.set_row_masks(ref.live[None, :])
        self.shadow_on = True
        assert self.ctx.shadow_info()["resident"] == (ref.dtype != po.DT_I8)

    def streams(self):
        return "i8" if self.ref.dtype == po.DT_I8 else "shadow" if self.shadow_on else "f16"

    def reported(self, st, path, what):
        info = self.ctx.shadow_info()
        assert st["path"] == path and st["overflow_queries"] == 0 and st["bound_violations"] == 0, (what, st)
        assert info["last_filter"] == self.streams() and not info["demoted"], (what, info)

    def flat_matches(self, ids, sc, what):
        assert np.array_equal(ids, self.ref.top_ids[:self.nq]), (what, "ids")
        assert same_bits(sc, self.ref.top_sc[:self.nq]), (what, "score bits")

    # ---- the steps
    def flat(self, what="flat"):
        ids, sc = self.ctx.search_batch(self.q, K)
        self.flat_matches(ids, sc, what)
        self.reported(self.ctx.stats(), PATH_FLAT, what)
        return ids, sc

    def flat_dev(self):
        import torch
        dev = torch.device("cuda", 0)
        t_q = torch.from_numpy(self.q).to(dev)
        t_ids = torch.empty((self.nq, K), dtype=torch.int64, device=dev)
        t_sc = torch.empty((self.nq, K), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        self.ctx.search_batch_dev(t_q.data_ptr(), self.nq, K, t_ids.data_ptr(), t_sc.data_ptr(), None)
        torch.cuda.synchronize()
        st = self.ctx.search_check()
        self.flat_matches(t_ids.cpu().numpy().astype(np.uint64), t_sc.cpu().numpy(), "flat, device API")
        self.reported(st, PATH_FLAT, "flat, device API")

    def range(self):
        lims, ids, sc = self.ctx.range_search(self.q, self.ref.radius[:self.nq])
        el, ei, es = self.ref.range_expected(self.nq)
        assert np.array_equal(lims, el) and np.array_equal(ids, ei) and same_bits(sc, es), "range"
        self.reported(self.ctx.stats(), PATH_RANGE, "range")

    def masked(self):
        self.ctx.set_option("path", 2)
        try:
            ids, sc, counts = self.ctx.search_masked(self.q, K)
        finally:
            self.ctx.set_option("path", 0)
        ei, es = self.ref.masked_expected(self.nq)
        assert np.all(counts == K) and np.array_equal(ids, ei) and same_bits(sc, es), "masked flat"
        self.reported(self.ctx.stats(), PATH_FLAT, "masked flat")

    def permute(self, order):
        got = []
        for on in order:
            self.ctx.set_option("tile_permute", on)
            got.append(self.flat(f"flat, tile_permute={on}"))
        assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes(), "tile order changed a result"

    def shadow(self, on):
        self.ctx.set_option("q8_shadow", on)
        self.shadow_on = bool(on)


# (step, the filter kind an fp16 corpus reports after it in FORWARD order; None: an option change)
SEQUENCE = [
    (lambda d: d.flat(), "shadow"),
    (lambda d: d.range(), "shadow"),
    (lambda d: d.shadow(0), None),
    (lambda d: d.range(), "f16"),
    (lambda d: d.flat_dev(), "f16"),
    (lambda d: d.masked(), "f16"),
    (lambda d: d.permute((0, 1)), "f16"),
    (lambda d: d.shadow(1), None),
    (lambda d: d.flat(), "shadow"),
]


def run(ref, nq, steps, kinds=None):
    d = Driver(ref, nq)
    try:
        for i, (step, kind) in enumerate(steps):
            step(d)                                                     # (asserts the results and the filter the options in force ask for)
            if kinds and kind:
                assert d.ctx.shadow_info()["last_filter"] == kind, (i, kind)
    finally:
        d.ctx.close()


@pytest.mark.parametrize("nq", BATCHES)
def test_sequence_forward(refs, nq):
    """flat (shadow), range (shadow), q8_shadow = 0, range (fp16), flat through the device API (fp16), masked flat at path = 2,
    flat under tile_permute = 0 then 1 (identical), q8_shadow = 1, flat (shadow)."""
    run(refs(po.DT_F16), nq, SEQUENCE, kinds=True)


@pytest.mark.parametrize("nq", BATCHES)
def test_sequence_reversed(refs, nq):
    """The same steps last to first on a fresh context: the option changes swap places, so the middle block now streams the shadow
    (the tile orders, masked flat, device API, range) and the last two calls the fp16 rows."""
    run(refs(po.DT_F16), nq, SEQUENCE[::-1])


@pytest.mark.parametrize("nq", BATCHES)
def test_int8_corpus_streams_itself_throughout(refs, nq):
    """An int8 corpus of the same shape: q8_shadow changes nothing, every call reports the corpus' own rows."""
    run(refs(po.DT_I8), nq, SEQUENCE)
