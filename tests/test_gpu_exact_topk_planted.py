"""The exact MFMA path's top-k filing (kernels_exact_mfma.h: exact_topk_offer / exact_topk_flush) and score store on PLANTED corpora.

Random rows exercise the list filing for the first few hundred rows only (afterwards almost no tile beats the bar) and the
existing tests hold one tie pair.  Here the corpus is arranged so that the filing runs all the time or at its edges: a tie group
of 70 rows across the k-th place, scores that rise (every tile files, the bar moves every time) or fall (only the first tiles
file) with the row number, and all k best rows inside one tile -- the first or the ragged last one.

Shape: d = 128, n = 1077 = 67 whole 16-row tiles + a ragged tile of 5 rows, just over the 1024 rows below which the launcher
leaves the MFMA path.  Everything goes through the public search with option path = 1, on the four kernel builds of
test_exact_scores_on_the_fp32_matrix_cores; the MFMA builds must equal the VALU kernels in ids and score bits, and the oracle."""
import numpy as np
import pytest

import nvdb_amd
import pyoracle as po
from test_gpu_parity import SEED, _check_against_oracle

pytestmark = pytest.mark.gpu

N, D = 1077, 128
TAGS = ["f16", "f32", "i8"]
DTYPES = {"f16": (nvdb_amd.DT_F16, po.DT_F16), "f32": (nvdb_amd.DT_F32, po.DT_F32), "i8": (nvdb_amd.DT_I8, po.DT_I8)}
# 16: one 16-query block, four row slices per workgroup; 32: two blocks, two slices; 40: three blocks, one idle wave;
# 64: one full group (staged builds only); 89: one staged group + 25 queries on the register-direct build
BATCHES = [16, 32, 40, 64, 89]
# the kernel builds of test_exact_scores_on_the_fp32_matrix_cores
MODES = {"img": dict(exact_mfma=1, exact_img=1, exact_lds=1), "lds": dict(exact_mfma=1, exact_img=0, exact_lds=2),
         "reg": dict(exact_mfma=1, exact_img=0, exact_lds=0), "valu": dict(exact_mfma=0, exact_img=0, exact_lds=0)}


def _corpus(tag, seed):
    return nvdb_amd.synth_corpus(seed, 0, N, D, DTYPES[tag][0])


def _row_as_query(oracle, tag, base, scales, i):
    """the fp32 image of row i (what the kernels multiply with)"""
    if tag == "f16":
        return oracle.f16_to_f32(base[i]).astype(np.float32)
    return base[i].astype(np.float32) * (np.float32(scales[i]) if tag == "i8" else np.float32(1.0))


def _reordered(base, scales, order):
    """row j of the result = row order[j]; an int8 row moves with its scale"""
    return np.ascontiguousarray(base[order]), (None if scales is None else np.ascontiguousarray(scales[order]))


def _open(tag, base, scales):
    c = nvdb_amd.HipContext(0)
    c.upload_corpus(base, DTYPES[tag][0], scales)
    c.set_option("path", 1)
    return c


def _run(c, queries, k, path=1):
    """every build; the MFMA builds bit for bit against the VALU kernels.  Returns the image build's result."""
    out = {}
    for name, opts in MODES.items():
        for key, val in opts.items():
            c.set_option(key, val)
        out[name] = c.search_batch(queries, k)
        assert c.stats()["path"] == path, (name, c.stats()["path"])
    for name in ("img", "lds", "reg"):
        assert np.array_equal(out[name][0], out["valu"][0]), (name, "ids")
        assert np.array_equal(out[name][1].view(np.uint32), out["valu"][1].view(np.uint32)), (name, "score bits")
    return out["img"]


def _best_first(c, q):
    """row ids by (score desc, id asc) of ONE query: a single query stays on the VALU kernels (k = n: the any-k path, every row's score)"""
    ids, _ = c.search_batch(q[None, :], N)
    assert ids.shape == (1, N)
    return ids[0].astype(np.int64)


def _queries(nq, seed):
    return nvdb_amd.synth_rows_f32(seed, 0, nq, D)


def _oracle_check(oracle, tag, base, scales, queries, res, k, planted, what):
    sub = np.unique(np.r_[planted, 1, 15, len(queries) - 1])
    _check_against_oracle(oracle, base, DTYPES[tag][1], scales, queries[sub], res[0][sub], res[1][sub], k, what)


# 70 copies of one row: rows 0 and n - 1, six in tile 20 (320 and 321 are two of ONE lane's four rows), the other 62 on tiles of
# their own, spread over every row slice and workgroup, at varying positions in the tile
TIE_ROWS = sorted({0, N - 1, 320, 321, 325, 330, 331, 335} | {16 * t + (7 * t) % 16 for t in range(1, 67) if t != 20 and t % 17 != 0})
assert len(TIE_ROWS) == 70 and sum(1 for r in TIE_ROWS if r // 16 == 20) == 6


@pytest.fixture(scope="module")
def tie_corpus():
    made = {}

    def get(tag):
        if tag not in made:
            base, scales = _corpus(tag, SEED + 300)
            for r in TIE_ROWS[1:]:
                base[r] = base[TIE_ROWS[0]]
                if scales is not None:
                    scales[r] = scales[TIE_ROWS[0]]
            made[tag] = (base, scales)
        return made[tag]
    return get


@pytest.mark.parametrize("nq", BATCHES)
@pytest.mark.parametrize("tag", TAGS)
def test_tie_group_across_the_kth_place(oracle, tie_corpus, tag, nq):
    """70 rows with one score and the k-th place inside the group: the k lowest ids win, ascending --
    whatever order the tiles, slices and workgroups file them in."""
    base, scales = tie_corpus(tag)
    queries = _queries(nq, SEED + 301)
    queries[0] = _row_as_query(oracle, tag, base, scales, TIE_ROWS[0])
    c = _open(tag, base, scales)
    for k in (1, 63, 64):
        res = _run(c, queries, k)
        assert res[0][0].tolist() == TIE_ROWS[:k], (tag, nq, k)
        assert len(set(res[1][0].view(np.uint32).tolist())) == 1, "one score for the whole group"
        _oracle_check(oracle, tag, base, scales, queries, res, k, [0], f"planted ties/{tag}/nq{nq}/k{k}")
    c.close()


@pytest.mark.parametrize("nq", BATCHES)
@pytest.mark.parametrize("tag", TAGS)
def test_scores_rising_and_falling_with_the_row_number(oracle, tag, nq):
    """Rows ordered by one query's score, ascending: with q every tile files entries and the bar moves every time; with -q only the
    first tiles file."""
    base, scales = _corpus(tag, SEED + 310)
    queries = _queries(nq, SEED + 311)
    q = queries[0].copy()
    c = _open(tag, base, scales)
    order = _best_first(c, q)[::-1]                       # worst first
    c.close()
    base, scales = _reordered(base, scales, order)
    rising = oracle.scores(base, DTYPES[tag][1], q, scales)
    assert np.all(np.diff(rising) >= 0) and rising[0] < rising[-1], "the plant: scores rise with the row number"
    c = _open(tag, base, scales)
    for sign in (1.0, -1.0):
        queries[0] = np.float32(sign) * q
        for k in (1, 10, 64):
            res = _run(c, queries, k)
            assert res[0][0][0] in ((N - 1, N - 2) if sign > 0 else (0, 1)), (tag, nq, k, sign)      # (two: a tie for the best score orders by id)
            _oracle_check(oracle, tag, base, scales, queries, res, k, [0], f"planted {'rising' if sign > 0 else 'falling'}/{tag}/nq{nq}/k{k}")
    c.close()


@pytest.mark.parametrize("nq", BATCHES)
@pytest.mark.parametrize("tag", TAGS)
def test_all_k_best_in_one_tile(oracle, tag, nq):
    """The k best rows of query 0 inside ONE 16-row tile: the first (k = 5, and k = 16: the whole tile), and the ragged last one
    (k = 5 = its rows)."""
    base0, scales0 = _corpus(tag, SEED + 320)
    queries = _queries(nq, SEED + 321)
    c = _open(tag, base0, scales0)
    best = _best_first(c, queries[0])
    c.close()
    for k, first_row in ((5, 0), (16, 0), (5, N - 5)):
        order = np.arange(N)
        home = np.arange(first_row, first_row + k)
        # the k best swap places with whoever sits in the tile (a best row that is already there stays)
        movers = [b for b in best[:k] if b not in home]
        free = [h for h in home if h not in best[:k]]
        for b, h in zip(movers, free):
            order[h], order[b] = b, h
        base, scales = _reordered(base0, scales0, order)
        c = _open(tag, base, scales)
        res = _run(c, queries, k)
        c.close()
        assert set(res[0][0].tolist()) == set(home.tolist()), (tag, nq, k, first_row)
        _oracle_check(oracle, tag, base, scales, queries, res, k, [0], f"planted one tile/{tag}/nq{nq}/k{k}/row{first_row}")


@pytest.mark.parametrize("nq", [16, 89])
@pytest.mark.parametrize("tag", TAGS)
def test_score_matrix_with_a_ragged_last_float4(oracle, tie_corpus, tag, nq):
    """k = 100 is the any-k path: the score matrix comes from the same tiles, and n % 4 = 1 leaves the last 16-byte store of every score
    row ragged.  On the tie corpus, so that the selection behind it meets the group as well."""
    base, scales = tie_corpus(tag)
    queries = _queries(nq, SEED + 301)
    queries[0] = _row_as_query(oracle, tag, base, scales, TIE_ROWS[0])
    c = _open(tag, base, scales)
    res = _run(c, queries, 100, path=3)
    c.close()
    assert res[0][0][:70].tolist() == TIE_ROWS
    _oracle_check(oracle, tag, base, scales, queries, res, 100, [0], f"planted score matrix/{tag}/nq{nq}")
