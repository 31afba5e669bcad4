"""Exact-L2 refine on candidate lists built to break a wave-resident top-K with a cross-wave merge.

The other refine tests draw candidates at random, which never yields equal distances on distinct ids, ordered arrival, the K
best inside one wave or inside the last partial step, a skipped slot behind a very close row, R at a step boundary, the first
and last row of the allocation, or a valid candidate at or beyond the padding distance 1e30.  Here every list is BUILT from
fp64 distances computed in this module, and every list runs on each row of BUILDS, which together reach all product kernels
(v3 whole rows, v2 column chunks through LDS, v1 lane per row; the three kernel templates of kernels_refine.h).

Every finite case asserts
  * ids and distance bits == oracle.refine(mode=0), the restatement of the reference kernel's fp32 order;
  * independently of the oracle, in numpy fp64: the returned ids, as a multiset, are the K smallest by (fp64 distance, id);
    returned distances are within GAMMA * dist of the fp64 value; distances ascend and equal distances ascend by id;
  * padding is exactly 0xFFFFFFFF / 1e30 and never precedes a valid entry.
GAMMA: a squared L2 distance is a sum of dim non-negative terms; each term carries the rounding of q - x twice (it is
squared) and at most dim roundings of the fma chain that accumulates it, so the relative error is at most
gamma = (dim + 2) u / (1 - (dim + 2) u) with u = 2^-24.  Two candidates a (among the K best in fp64) and b (not) may
therefore swap only when d_b - d_a <= gamma (d_a + d_b): the one tolerated difference ("tie exemption").  The lists take their
ordinary rows from a pool in which any two fp64 distances are further apart than twice that, so the exemption should never be
needed; a CPU test checks on the inputs alone that at most 5 % of the (query, case) pairs could fall under it, and the last GPU
test checks the same on what the GPU returned.

Ties: the reference keeps, among equal distances, whichever candidate arrived first (`dist >= max_val` rejects,
cuda_refine.cu:267; thread 0 merges the threads' lists in thread order, :465-474, and its final selection sort compares
distances only, :479-488), so its output inside a tie group follows the list order.  This project and its oracle use the
deterministic (distance asc, id asc) instead: a deliberate deviation.  Inside a tie group that lies wholly among the K best the
two differ only in the order of the tied ids; where the group straddles the K-th place they differ in the id SET (the reference
keeps the members that arrived first, this project the smallest ids -- in the straddle lists below, where the winners arrive
last, the reference would return other ids).  The tie cases pin that the smaller id wins whatever the list order.  Two tie
groups are planted: 64 bit-identical copies, and 16 rows of two different contents (+-0.5 in a coordinate where query 2 is 0)
whose distances to query 2 are equal -- only the second can show a read of the wrong row inside a tie group.

Tests that need the GPU carry the gpu mark one by one: the checks of the list generators and of the exemption cap at the top
of the module run without one.  The last GPU test runs every finite case once more and counts the exemptions itself.
"""
import math
import os
import re
import zlib
from collections import Counter
from functools import lru_cache

import numpy as np
import pytest

import nvdb_amd
import pyoracle as po

gpu = pytest.mark.gpu

SEED = 20240613
N = 4096
PAD = 0xFFFFFFFF
PAD_DIST_BITS = np.float32(1e30).view(np.uint32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nano-vectordb_amd", "csrc")

# (waves, candidates per wave and step) of each kernel body; slot s of a list belongs to wave (s // rows) % waves, position
# s % rows, step s // (waves * rows).  test_slot_geometry_matches_the_kernel_bodies reads the same figures from the headers.
GEOM = {"v3": (3, 16), "v2": (4, 64), "v1": (4, 64)}
V3_SLOT_BYTES = {768: 16 * 1040 + 8 * 1040, 512: 16 * 1040, 384: 16 * 784, 256: 16 * 528}   # refine3_slot_bytes<DIM>()

# (name, dtype tag, dim, option refine_v2, kernel that must run)
BUILDS = [("v3-768", "f16", 768, 2, "v3"), ("v3-512", "f16", 512, 2, "v3"), ("v3-384", "f16", 384, 2, "v3"),
          ("v3-256", "f16", 256, 2, "v3"), ("v2-1536", "f16", 1536, 2, "v2"), ("v2-1024", "f16", 1024, 2, "v2"),
          ("v2-f32-768", "f32", 768, 2, "v2"), ("v2-forced-768", "f16", 768, 1, "v2"), ("v1-forced-768", "f16", 768, 0, "v1"),
          ("v1-64", "f16", 64, 2, "v1"), ("v1-unaligned-100", "f16", 100, 2, "v1"), ("v1-unaligned-f32-37", "f32", 37, 2, "v1")]
BUILD_NAMES = [b[0] for b in BUILDS]

# planted rows
DUP_IDS = (5 + 63 * np.arange(64)).astype(np.uint32)        # 64 bit-identical rows at scattered ids
PM_IDS = (11 + 257 * np.arange(16)).astype(np.uint32)       # query 2 itself but for +0.5 (even members) / -0.5 (odd) where the query is 0
HUGE_IDS = np.array([2000, 2001], dtype=np.uint32)          # +65504 and -65504 throughout
PM_COORD = 9
GROUPS = {"copies": DUP_IDS, "plusminus": PM_IDS}
Q_PLAIN, Q_ON_DUP, Q_PM, Q_EDGES, Q_BIG, Q_OVERFLOW, Q_INF, Q_NAN = range(8)
FINITE_Q = [Q_PLAIN, Q_ON_DUP, Q_PM, Q_EDGES]

TIES_K = (1, 10, 64)
SIZES_K = (1, 3, 64)
SIZES_R = (1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 255, 256, 257)   # step - 1, step, step + 1 of every body, and its wave granule
SENTINEL_SHAPES = ((100, 3), (100, 64), (40, 64))                  # (R, K); the last has fewer valid candidates than K


def gamma_of(dim):
    u = 2.0 ** -24
    return (dim + 2) * u / (1.0 - (dim + 2) * u)


# ----------------------------------------------------------------------------- slot placement
def stride_of(kernel):
    w, g = GEOM[kernel]
    return w * g


def slot_of(kernel, wave, step, pos):
    w, g = GEOM[kernel]
    assert 0 <= wave < w and 0 <= pos < g
    return step * w * g + wave * g + pos


def where_of(kernel, slot):
    w, g = GEOM[kernel]
    return (slot // g) % w, slot // (w * g), slot % g          # wave, step, position


def scatter_slots(kernel, count, R):
    """`count` distinct slots inside the whole steps of a list of R entries; neighbours differ in wave AND in step."""
    w, g = GEOM[kernel]
    steps = R // (w * g)
    period = w * steps // math.gcd(w, steps)
    assert steps >= 2 and count <= period * g
    return [slot_of(kernel, i % w, i % steps, (i // period + 5 * (i % period)) % g) for i in range(count)]


def build_list(R, placed, fill):
    """A list of R slots: `placed` {slot: id} first, the free slots take `fill` in order, what is left stays 0xFFFFFFFF."""
    out = np.full(R, PAD, dtype=np.uint32)
    free = np.array([s for s in range(R) if s not in placed], dtype=np.int64)
    for s, i in placed.items():
        assert 0 <= s < R
        out[s] = i
    k = min(len(free), len(fill))
    out[free[:k]] = np.asarray(fill[:k], dtype=np.uint32)
    return out


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


# ----------------------------------------------------------------------------- corpus, queries, fp64 distances
class Build:
    def __init__(self, name, tag, d, v2, kernel):
        self.name, self.tag, self.d, self.v2, self.kernel = name, tag, d, v2, kernel
        self.gamma = gamma_of(d)
        f16 = tag == "f16"
        self.dt = po.DT_F16 if f16 else po.DT_F32
        to_rows = (lambda x: nvdb_amd.f32_to_f16(x)) if f16 else (lambda x: np.ascontiguousarray(x, dtype=np.float32))
        widen = (lambda r: r.view(np.float16).astype(np.float64)) if f16 else (lambda r: r.astype(np.float64))
        base = to_rows(nvdb_amd.synth_rows_f32(SEED + 70, 0, N, d))
        q = nvdb_amd.synth_rows_f32(SEED + 71, 0, 8, d)
        base[DUP_IDS] = base[DUP_IDS[0]]
        q[Q_ON_DUP] = widen(base[DUP_IDS[0]]).astype(np.float32)            # distance exactly 0 to all 64 copies
        q[Q_PM, PM_COORD] = 0.0
        pm = np.repeat(widen(to_rows(q[Q_PM][None, :])), len(PM_IDS), axis=0)   # the 16 closest rows of query 2, all at ~0.25
        pm[:, PM_COORD] = np.where(np.arange(len(PM_IDS)) % 2 == 0, 0.5, -0.5)
        base[PM_IDS] = to_rows(pm.astype(np.float32))
        q[Q_EDGES] = widen(to_rows(q[Q_EDGES][None, :]))[0].astype(np.float32)   # a query that rows can equal exactly
        near = np.repeat(q[Q_EDGES][None, :], 2, axis=0)
        near[0, 1] += np.float32(2.0 ** -6)
        near[1, 1] += np.float32(2.0 ** -5)
        base[[0, N - 1]] = to_rows(near)                                        # first and last row: the closest to query 3
        base[HUGE_IDS] = to_rows(np.array([[65504.0], [-65504.0]], dtype=np.float32).repeat(d, axis=1))
        q[[Q_BIG, Q_OVERFLOW, Q_INF, Q_NAN]] = q[Q_PLAIN]
        q[Q_BIG, 0] = 1.2e15                              # every distance ~1.44e30: finite, beyond the padding's 1e30
        q[Q_OVERFLOW, 0] = 3e19                      # (3e19)^2 overflows fp32: every distance +inf
        q[Q_INF, 5] = np.inf
        q[Q_NAN, 5] = np.nan
        self.base, self.queries = base, q
        rows64 = widen(base)
        with np.errstate(all="ignore"):
            self.D = np.stack([((q[i].astype(np.float64) - rows64) ** 2).sum(axis=1) for i in range(6)])   # fp64, [query, row]
        planted = np.concatenate([DUP_IDS, PM_IDS, HUGE_IDS, np.array([0, N - 1], dtype=np.uint32)])
        assert len(set(planted.tolist())) == len(planted)
        ordinary = np.setdiff1d(np.arange(N, dtype=np.uint32), planted)
        self.sep = [self._separated(self.D[i], ordinary, planted) for i in FINITE_Q]

    def _separated(self, D, ordinary, planted):
        """Ordinary ids, ascending by fp64 distance, any two (and any one and a planted row) further apart than twice the bound."""
        g2 = 2.0 * self.gamma
        order = ordinary[np.lexsort((ordinary, D[ordinary]))]
        keep = [order[0]]
        for i in order[1:]:
            if D[i] - D[keep[-1]] > g2 * (D[i] + D[keep[-1]]):
                keep.append(i)
        keep = np.array(keep, dtype=np.uint32)
        dp = D[planted][None, :]
        dk = D[keep][:, None]
        return keep[(np.abs(dk - dp) > g2 * (dk + dp)).all(axis=1)]


@lru_cache(maxsize=None)
def get_build(name):
    return Build(*BUILDS[BUILD_NAMES.index(name)])


def _shuffled_fill(ids, need, rs):
    ids = np.asarray(ids, dtype=np.uint32)[:need]
    return rs.permutation(np.concatenate([ids, np.full(need - len(ids), PAD, dtype=np.uint32)]))


# ----------------------------------------------------------------------------- the lists.  Each returns (queries used, cand [Q, R]).
def lists_ties(bd, descending, group="copies"):
    """A tie group (the 64 copies, or the 16 +-0.5 rows) on slots whose neighbours differ in wave and step, ids ascending or
    descending along the list; the free slots hold the same shuffled ordinary rows in both orders."""
    R = 4 * stride_of(bd.kernel)
    ids = np.sort(GROUPS[group])
    slots = scatter_slots(bd.kernel, len(ids), R)
    cand = [build_list(R, dict(zip(slots, ids[::-1] if descending else ids)), _shuffled_fill(bd.sep[j], R - len(ids), _rs(bd.name, "ties", group, j)))
            for j in range(4)]
    return FINITE_Q, np.stack(cand)


def lists_straddle(bd, group="copies"):
    """K = 10: at most six rows closer than the tie group, so the group straddles the K-th place; four members that must win
    (the smallest ids) sit in the last four slots, the smallest one last.  (For the +-0.5 rows the members have one distance only
    to query 2; to the other queries they have two, and the list is an ordinary one.)"""
    R = 4 * stride_of(bd.kernel) + 4
    ids = np.sort(GROUPS[group])
    n = len(ids)
    slots = scatter_slots(bd.kernel, n - 4, R - 4)
    cand = []
    for j, qi in enumerate(FINITE_Q):
        dd = bd.D[qi][ids].min()
        sep = bd.sep[j]
        closer, farther = sep[bd.D[qi][sep] < dd][:6], sep[bd.D[qi][sep] > bd.D[qi][ids].max()]
        placed = dict(zip(slots, ids[4:]))
        placed.update({R - 4 + i: ids[3 - i] for i in range(4)})
        cand.append(build_list(R, placed, _shuffled_fill(np.concatenate([closer, farther[:R - n - 6]]), R - n, _rs(bd.name, "straddle", group, j))))
    return FINITE_Q, np.stack(cand)


def lists_falling(bd):
    return FINITE_Q, np.stack([bd.sep[j][:257][::-1] for j in range(4)])     # every candidate replaces the current best


def lists_rising(bd):
    return FINITE_Q, np.stack([bd.sep[j][:257] for j in range(4)])           # nothing is inserted after the first K


def lists_confined(bd, K=10):
    """The K best inside the slots of ONE wave (query j: wave j mod waves), spread over three steps."""
    w, g = GEOM[bd.kernel]
    R = 3 * w * g
    cand = []
    for j in range(4):
        slots = [slot_of(bd.kernel, j % w, i % 3, (3 * (i // 3) + 1 + j) % g) for i in range(K)]
        rs = _rs(bd.name, "confined", j)
        cand.append(build_list(R, dict(zip(slots, rs.permutation(bd.sep[j][:K]))), _shuffled_fill(bd.sep[j][K:], R - K, rs)))
    return FINITE_Q, np.stack(cand)


def lists_last_step(bd, K):
    """The K best in the final, partial step (K + 2 slots long: the other lanes of that step carry 0xFFFFFFFF)."""
    st = stride_of(bd.kernel)
    R = st + K + 2
    cand = []
    for j in range(4):
        rs = _rs(bd.name, "last", j, K)
        cand.append(build_list(R, dict(zip(range(st + 1, st + 1 + K), rs.permutation(bd.sep[j][:K]))), _shuffled_fill(bd.sep[j][K:], R - K, rs)))
    return FINITE_Q, np.stack(cand)


def lists_stale(bd, kind):
    """The best row at slot s, a skipped candidate at s + stride (same wave and position, one step later), far rows elsewhere."""
    w, g = GEOM[bd.kernel]
    st = w * g
    R = 2 * st + 7
    cand = []
    for j in range(4):
        s = slot_of(bd.kernel, j % w, 0, 3)
        skipped = PAD if kind == "pad" else (N if j % 2 == 0 else 0xFFFFFFFE)
        far = bd.sep[j][len(bd.sep[j]) // 2:][-(R - 2):]          # the farther half of the pool only
        cand.append(build_list(R, {s: bd.sep[j][0], s + st: skipped}, _shuffled_fill(far, R - 2, _rs(bd.name, "stale", j))))
    return FINITE_Q, np.stack(cand)


def lists_sizes(bd, R):
    cand = []
    for j in range(4):
        rs = _rs(bd.name, "sizes", j, R)
        row = rs.permutation(rs.permutation(bd.sep[j][:300])[:R])
        if j == 2:                                              # a quarter of the slots skipped: K = 64 exceeds the valid candidates sooner
            row[1::8] = PAD
            row[5::8] = N + 1
        cand.append(row)
    return FINITE_Q, np.stack(cand)


def lists_edges(bd, kind):
    if kind == "first-and-last":                                # rows 0 and n - 1 among far rows
        R = 100
        cand = []
        for j in range(4):
            far = bd.sep[j][-(R - 2):]
            cand.append(build_list(R, {(13 * j + 5) % 90: 0, R - 1 - j: N - 1}, _shuffled_fill(far, R - 2, _rs(bd.name, "edges", j))))
        return FINITE_Q, np.stack(cand)
    R = 1 if kind == "last-alone" else stride_of(bd.kernel) + 1   # "last-everywhere": one id in every slot stays R separate entries
    return FINITE_Q, np.full((4, R), N - 1, dtype=np.uint32)


def lists_sentinel(bd, special, R):
    """Ordinary rows mixed with the +-65504 rows and a few copies, for the four finite queries and one special query."""
    qsel = FINITE_Q + [special]
    cand = []
    for j in range(5):
        rs = _rs(bd.name, "sentinel", j, R)
        placed = {3: HUGE_IDS[0], R - 2: HUGE_IDS[1], 7: DUP_IDS[9], 20: DUP_IDS[2], 11: PAD, 12: N}
        cand.append(build_list(R, placed, rs.permutation(bd.sep[j % 4][:R - len(placed)])))
    return qsel, np.stack(cand)


def finite_cases(bd):
    """Every (family, case, queries, cand, K) whose distances are all finite: what the GPU tests run, enumerated for the CPU checks."""
    for group in GROUPS:
        for desc in (False, True):
            for K in TIES_K:
                yield ("ties", f"{group}-{'desc' if desc else 'asc'}-K{K}", *lists_ties(bd, desc, group), K)
        yield ("ties", f"{group}-straddle", *lists_straddle(bd, group), 10)
    for K in (10, 64):
        yield ("arrival", f"falling-K{K}", *lists_falling(bd), K)
        yield ("arrival", f"rising-K{K}", *lists_rising(bd), K)
    yield ("arrival", "confined", *lists_confined(bd), 10)
    for K in (3, 10):
        yield ("arrival", f"last-step-K{K}", *lists_last_step(bd, K), K)
    for kind in ("pad", "beyond"):
        yield ("stale", kind, *lists_stale(bd, kind), 3)
    for R in SIZES_R:
        for K in SIZES_K:
            yield ("sizes", f"R{R}-K{K}", *lists_sizes(bd, R), K)
    for kind in ("first-and-last", "last-alone", "last-everywhere"):
        yield ("edges", kind, *lists_edges(bd, kind), 3)
    for R, K in SENTINEL_SHAPES:                                # the finite queries of the sentinel batches
        qsel, cand = lists_sentinel(bd, Q_BIG, R)
        yield ("sentinel", f"finite-rows-R{R}-K{K}", qsel[:4], cand[:4], K)


# ----------------------------------------------------------------------------- the fp64 reference (numpy only)
def valid_of(row):
    row = np.asarray(row, dtype=np.uint32)
    return row[(row != PAD) & (row.astype(np.uint64) < N)]


def rank_fp64(D, row, K):
    """The K smallest valid candidates of one list by (fp64 distance, id), repeated ids as separate entries."""
    v = valid_of(row)
    o = np.lexsort((v, D[v]))[:K]
    return v[o], D[v][o]


def boundary_near_tie(D, row, K, gamma):
    """True when a candidate among the K best and one outside them are closer than the bound without being exactly equal: the
    only situation in which the tie exemption could apply."""
    v = valid_of(row)
    if len(v) <= K:
        return False
    d = np.sort(D[v])
    a, b = d[:K][:, None], d[K:][None, :]
    return bool(((b - a <= gamma * (a + b)) & (b != a)).any())


def check_fp64(bd, key, qsel, cand, K, ids, dist, strict=True):
    """Returns how many rows needed the tie exemption.  strict=False: a list whose fp32 distances are all equal by construction."""
    exempt = 0
    for r, qi in enumerate(qsel):
        D = bd.D[qi]
        want, _ = rank_fp64(D, cand[r], K)
        m = len(want)
        got, gd = ids[r, :m], dist[r, :m]
        assert (got != PAD).all() and (ids[r, m:] == PAD).all(), f"{key} row {r}: padding before a valid entry or a missing entry: {ids[r]}"
        assert (dist[r, m:].view(np.uint32) == PAD_DIST_BITS).all(), f"{key} row {r}: padding distance is not 1e30"
        assert set(got.tolist()) <= set(valid_of(cand[r]).tolist()), f"{key} row {r}: an id that is no valid candidate"
        d64 = D[got]
        assert (np.abs(gd.astype(np.float64) - d64) <= bd.gamma * d64).all(), f"{key} row {r}: distance off by more than gamma * dist"
        assert (np.diff(gd) >= 0).all() and (got[1:][np.diff(gd) == 0] >= got[:-1][np.diff(gd) == 0]).all(), \
            f"{key} row {r}: not ascending by (distance, id): {got} {gd}"
        extra = sorted((Counter(got.tolist()) - Counter(want.tolist())).elements(), key=lambda i: (D[i], i))
        missing = sorted((Counter(want.tolist()) - Counter(got.tolist())).elements(), key=lambda i: (D[i], i))
        for e, w in zip(extra, missing):
            assert (D[e] != D[w] or not strict) and abs(D[e] - D[w]) <= bd.gamma * (D[e] + D[w]), \
                f"{key} row {r}: returned id {e} (fp64 {D[e]!r}) instead of {w} ({D[w]!r}): further apart than the fp32 bound"
        exempt += bool(extra)
    return exempt


# ----------------------------------------------------------------------------- CPU checks of the generators (no GPU)
def test_slot_geometry_matches_the_kernel_bodies():
    """GEOM restates what the bodies do: v1 / v2 walk `r0 = wave * 64; r0 += 256`, v3 `s0 = wave * ROWS; s0 += WAVES * ROWS`."""
    head = open(os.path.join(CSRC, "kernels_refine.h")).read()
    assert len(re.findall(r"for \(uint32_t r0 = wave \* 64u; r0 < R; r0 \+= 256u\)", head)) == 2       # v1 and v2
    assert GEOM["v1"] == (4, 64) and GEOM["v2"] == (4, 64)
    assert re.search(r"for \(uint32_t s0 = wave \* REFINE3_ROWS; s0 < R; s0 \+= REFINE3_WAVES \* REFINE3_ROWS\)", head)
    m = re.search(r"constexpr int REFINE3_WAVES = (\d+), REFINE3_ROWS = (\d+);", head)
    assert m and GEOM["v3"] == (int(m.group(1)), int(m.group(2)))
    for k, (w, g) in GEOM.items():
        assert stride_of(k) in SIZES_R and stride_of(k) - 1 in SIZES_R and stride_of(k) + 1 in SIZES_R
        assert g in SIZES_R and g - 1 in SIZES_R and g + 1 in SIZES_R
        for s in (0, g - 1, g, w * g - 1, w * g, 5 * w * g + 2 * g + 3):
            assert slot_of(k, *where_of(k, s)[:2], where_of(k, s)[2]) == s


@pytest.mark.parametrize("kernel", sorted(GEOM))
def test_scatter_puts_neighbouring_ties_in_different_waves_and_steps(kernel):
    for R, count in ((4 * stride_of(kernel), 64), (4 * stride_of(kernel), 60), (2 * stride_of(kernel) + 5, 20)):
        slots = scatter_slots(kernel, count, R)
        assert len(set(slots)) == count and max(slots) < (R // stride_of(kernel)) * stride_of(kernel)
        where = [where_of(kernel, s) for s in slots]
        for a, b in zip(where, where[1:]):
            assert a[0] != b[0] and a[1] != b[1], (kernel, R, a, b)
        assert len({w[0] for w in where}) == GEOM[kernel][0]            # every wave holds some of the ties
    bd = get_build("v3-256" if kernel == "v3" else "v1-64")
    if bd.kernel == kernel:
        for desc in (False, True):
            for group, gids in GROUPS.items():
                for row in lists_ties(bd, desc, group)[1]:
                    at = {int(i): s for s, i in enumerate(row) if i in set(gids.tolist())}
                    assert len(at) == len(gids)
                    seq = [where_of(kernel, at[int(i)]) for i in np.sort(gids)]
                    assert all(a[0] != b[0] and a[1] != b[1] for a, b in zip(seq, seq[1:]))


@pytest.mark.parametrize("name", BUILD_NAMES)
def test_planted_rows_and_lists_are_what_the_cases_claim(name):
    bd = get_build(name)
    D, st = bd.D, stride_of(bd.kernel)
    assert (bd.base[DUP_IDS] == bd.base[DUP_IDS[0]]).all() and (D[:, DUP_IDS] == D[:, DUP_IDS[:1]]).all()
    assert (D[Q_ON_DUP, DUP_IDS] == 0.0).all()
    assert len({r.tobytes() for r in bd.base[PM_IDS]}) == 2 and (D[Q_PM, PM_IDS] == D[Q_PM, PM_IDS[0]]).all()   # rows differ, distances equal
    assert set(np.argsort(D[Q_EDGES])[:2].tolist()) == {0, N - 1} and D[Q_EDGES, 0] < D[Q_EDGES, N - 1]
    assert (D[Q_BIG] >= 1e30).all() and (D[Q_BIG] < 3e38).all() and (D[Q_OVERFLOW] > 3.5e38).all()
    assert all(len(s) >= 300 for s in bd.sep)
    for j, qi in enumerate(FINITE_Q):
        d = D[qi][bd.sep[j]]
        assert (np.diff(d) > 2 * bd.gamma * (d[1:] + d[:-1])).all()
    for j, row in enumerate(lists_falling(bd)[1]):
        assert (np.diff(D[FINITE_Q[j]][row]) < 0).all()
    for j, row in enumerate(lists_rising(bd)[1]):
        assert (np.diff(D[FINITE_Q[j]][row]) > 0).all()
    for j, row in enumerate(lists_confined(bd)[1]):
        best, _ = rank_fp64(D[FINITE_Q[j]], row, 10)
        assert {where_of(bd.kernel, int(np.flatnonzero(row == i)[0]))[0] for i in best} == {j % GEOM[bd.kernel][0]}
    for K in (3, 10):
        _, cand = lists_last_step(bd, K)
        assert cand.shape[1] % st == K + 2
        for j, row in enumerate(cand):
            best, _ = rank_fp64(D[FINITE_Q[j]], row, K)
            assert all(int(np.flatnonzero(row == i)[0]) >= st for i in best)
    for kind in ("pad", "beyond"):
        for j, row in enumerate(lists_stale(bd, kind)[1]):
            s = int(np.flatnonzero(row == bd.sep[j][0])[0])
            assert row[s + st] == PAD if kind == "pad" else row[s + st] >= N
            assert where_of(bd.kernel, s)[0] == where_of(bd.kernel, s + st)[0] and where_of(bd.kernel, s)[2] == where_of(bd.kernel, s + st)[2]
            assert rank_fp64(D[FINITE_Q[j]], row, 2)[1][1] > 1.02 * D[FINITE_Q[j]][bd.sep[j][0]]       # every other slot is far away
    assert set(np.argsort(D[Q_PM])[:16].tolist()) == set(PM_IDS.tolist())                      # the tie group of distinct rows: the 16 best of query 2
    for group, gids in GROUPS.items():
        _, cand = lists_straddle(bd, group)
        for j, row in enumerate(cand):
            if group == "plusminus" and FINITE_Q[j] != Q_PM:
                continue
            best, bdist = rank_fp64(D[FINITE_Q[j]], row, 10)
            assert bdist[9] == D[FINITE_Q[j]][gids[0]] and np.array_equal(row[-4:], np.sort(gids)[:4][::-1])
            assert set(np.sort(gids)[:4].tolist()) <= set(best.tolist()) and len(set(gids.tolist()) - set(best.tolist())) >= 6


@pytest.mark.parametrize("name", BUILD_NAMES)
def test_fp64_ranking_agrees_with_the_oracles_double_path(oracle, name):
    """oracle.refine(mode=1) accumulates in double like the reference's CPU refine and rounds to fp32 at the end; on these lists
    (ordinary rows separated by far more than an fp32 ulp, planted groups exactly equal) it must rank as plain numpy fp64 does."""
    bd = get_build(name)
    for family, case, qsel, cand, K in finite_cases(bd):
        oid, odist = oracle.refine(bd.base, bd.dt, bd.queries[qsel], cand, K, mode=1)
        for r, qi in enumerate(qsel):
            want, wd = rank_fp64(bd.D[qi], cand[r], K)
            got = oid[r, :len(want)]
            assert sorted(got.tolist()) == sorted(want.tolist()) and (oid[r, len(want):] == PAD).all(), (name, family, case, r)
            D, diff = bd.D[qi], got != want          # mode 1 ranks AFTER its one rounding to fp32: the +-65504 rows may swap inside it
            assert (np.abs(D[got[diff]] - D[want[diff]]) <= 2.0 ** -23 * D[want[diff]]).all(), (name, family, case, r)
            assert (np.abs(odist[r, :len(want)] - wd) <= 2.0 ** -23 * wd).all(), (name, family, case, r)   # one fp32 rounding of a double sum


def test_exemption_cap_holds_on_the_reference_alone():
    """On fp64 alone: at most 5 % of the (query, case) pairs have two unequal candidates within the bound on either side of the
    K-th place (exactly equal planted groups aside, whose order the id decides)."""
    pairs = near = 0
    for name in BUILD_NAMES:
        bd = get_build(name)
        for family, case, qsel, cand, K in finite_cases(bd):
            for r, qi in enumerate(qsel):
                pairs += 1
                near += boundary_near_tie(bd.D[qi], cand[r], K, bd.gamma)
    assert pairs > 1000 and near <= 0.05 * pairs, (near, pairs)


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ctx():
    c = nvdb_amd.HipContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=BUILD_NAMES)
def build(request, ctx):
    bd = get_build(request.param)
    ctx.upload_corpus(bd.base, bd.dt)
    ctx.set_option("refine_v2", bd.v2)
    try:
        yield bd
    finally:
        ctx.set_option("refine_v2", 2)


def assert_padding(key, ids, dist):
    pad = ids == PAD
    assert (dist.view(np.uint32)[pad] == PAD_DIST_BITS).all(), f"{key}: padding distance is not 1e30"
    assert (pad[:, 1:] >= pad[:, :-1]).all(), f"{key}: padding before a valid entry"


def run_counted(ctx, oracle, bd, family, case, qsel, cand, K):
    """One finite case with all its assertions; returns ids, distances and how many rows needed the tie exemption."""
    key = (family, case)
    q = bd.queries[qsel]
    ids, dist = ctx.refine_l2_topk(q, cand, K)
    oid, odist = oracle.refine(bd.base, bd.dt, q, cand, K, mode=0)
    assert np.array_equal(ids, oid), f"{bd.name} {key}: ids differ from the oracle\n{ids}\n{oid}"
    assert np.array_equal(dist.view(np.uint32), odist.view(np.uint32)), f"{bd.name} {key}: distance bits differ from the oracle"
    assert_padding(key, ids, dist)
    return ids, dist, check_fp64(bd, key, qsel, cand, K, ids, dist)


def run_finite(*a):
    return run_counted(*a)[:2]


@gpu
def test_build_launches_the_expected_kernel(ctx, build):
    """threads / nwarps / shmem_bytes of the timing struct name the kernel that ran: v3 3 waves and its row slots, v2 4 waves and
    128 KB of chunk buffers, v1 4 waves and only the merge lists."""
    qsel, cand = lists_sizes(build, 64)
    _, _, t = ctx.refine_l2_topk(build.queries[qsel], cand, 3, want_timing=True)
    want = {"v3": (192, 3, 3 * V3_SLOT_BYTES.get(build.d, 0)), "v2": (256, 4, 4 * 2 * 64 * 256), "v1": (256, 4, 4 * 64 * 8 + 16)}[build.kernel]
    assert (t.threads, t.nwarps, t.shmem_bytes) == want, (build.name, t.threads, t.nwarps, t.shmem_bytes)


def _tied_rows(group):
    """(row of the batch whose query is nearest to the group, rows in which the whole group has ONE distance)"""
    return (1, range(4)) if group == "copies" else (2, [2])


@gpu
@pytest.mark.parametrize("K", TIES_K)
@pytest.mark.parametrize("group", list(GROUPS))
def test_ties_across_waves_smaller_id_wins_in_either_list_order(ctx, oracle, build, group, K):
    gids = np.sort(GROUPS[group])
    out = []
    for desc in (False, True):
        qsel, cand = lists_ties(build, desc, group)
        out.append(run_finite(ctx, oracle, build, "ties", f"{group}-{'desc' if desc else 'asc'}-K{K}", qsel, cand, K))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32)), \
        "the order of the tied ids in the list changed the result"
    ids, dist = out[0]
    on, tied_rows = _tied_rows(group)
    m = min(K, len(gids))
    assert np.array_equal(ids[on, :m], gids[:m])                        # the group is the nearest of that query: its smallest ids, ascending
    assert (dist[on, :m].view(np.uint32) == dist[on, 0].view(np.uint32)).all()   # one distance, also across the two row contents
    for r in tied_rows:
        tied = ids[r][np.isin(ids[r], gids)]
        assert np.array_equal(tied, gids[:len(tied)])                   # whatever made it is the smallest ids, smallest first


@gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_tie_group_straddling_the_kth_place_winners_arrive_last(ctx, oracle, build, group):
    gids = np.sort(GROUPS[group])
    qsel, cand = lists_straddle(build, group)
    ids, _ = run_finite(ctx, oracle, build, "ties", f"{group}-straddle", qsel, cand, 10)
    for r in _tied_rows(group)[1]:
        tied = ids[r][np.isin(ids[r], gids)]
        assert 4 <= len(tied) < len(gids) and np.array_equal(tied, gids[:len(tied)]) and ids[r, 9] in gids


@gpu
@pytest.mark.parametrize("order", ["falling", "rising"])
def test_arrival_in_distance_order(ctx, oracle, build, order):
    qsel, cand = (lists_falling if order == "falling" else lists_rising)(build)
    for K in (10, 64):
        ids, _ = run_finite(ctx, oracle, build, "arrival", f"{order}-K{K}", qsel, cand, K)
        assert np.array_equal(ids, cand[:, -K:][:, ::-1] if order == "falling" else cand[:, :K])


@gpu
def test_k_best_confined_to_one_waves_slots(ctx, oracle, build):
    qsel, cand = lists_confined(build)
    run_finite(ctx, oracle, build, "arrival", "confined", qsel, cand, 10)


@gpu
@pytest.mark.parametrize("K", [3, 10])
def test_k_best_in_the_final_partial_step(ctx, oracle, build, K):
    qsel, cand = lists_last_step(build, K)
    run_finite(ctx, oracle, build, "arrival", f"last-step-K{K}", qsel, cand, K)


@gpu
@pytest.mark.parametrize("kind", ["pad", "beyond"])
def test_skipped_slot_behind_the_best_row_does_not_repeat_it(ctx, oracle, build, kind):
    """v3 issues no load for a skipped candidate: its LDS slot still holds the best row from the step before."""
    qsel, cand = lists_stale(build, kind)
    ids, dist = run_finite(ctx, oracle, build, "stale", kind, qsel, cand, 3)
    for r in range(4):
        best = build.sep[r][0]
        assert ids[r, 0] == best and (ids[r] == best).sum() == 1 and dist[r, 1] > dist[r, 0]


@gpu
@pytest.mark.parametrize("R", SIZES_R)
def test_sizes_at_the_step_boundaries(ctx, oracle, build, R):
    qsel, cand = lists_sizes(build, R)
    for K in SIZES_K:
        run_finite(ctx, oracle, build, "sizes", f"R{R}-K{K}", qsel, cand, K)


@gpu
@pytest.mark.parametrize("kind", ["first-and-last", "last-alone", "last-everywhere"])
def test_first_and_last_row_of_the_allocation(ctx, oracle, build, kind):
    qsel, cand = lists_edges(build, kind)
    ids, dist = run_finite(ctx, oracle, build, "edges", kind, qsel, cand, 3)
    if kind == "first-and-last":
        assert ids[3, 0] == 0 and ids[3, 1] == N - 1                    # the two closest rows of query 3
    elif kind == "last-alone":
        assert (ids[:, 0] == N - 1).all() and (ids[:, 1:] == PAD).all()
    else:
        assert (ids == N - 1).all() and (dist == dist[:, :1]).all()


@gpu
@pytest.mark.parametrize("special", ["big", "overflow", "inf"])
def test_valid_candidates_at_or_beyond_the_padding_distance(ctx, oracle, build, special):
    """A query with one element of 1.2e15 (every distance ~1.44e30, finite), of 3e19 (the square overflows: +inf) or of +inf.
    The reference keeps such a candidate while its list is not full (topk_unsorted_push fills first, cuda_refine.cu:260-266) and
    drops it afterwards (`dist >= max_val`, :267); it never drops a valid id for looking like padding (only id 0xFFFFFFFF is
    skipped in the merge, :472).  Its final selection sort (:479-488) orders by distance alone, so with fewer valid candidates
    than K it would write the unused 1e30 / 0xFFFFFFFF entries AHEAD of a kept candidate beyond 1e30.  This project and the
    oracle keep valid entries first -- (distance asc, id asc), then padding -- so the id tells the two apart; that is what is
    pinned here.  The four ordinary queries of the batch get the full finite checks."""
    sq = {"big": Q_BIG, "overflow": Q_OVERFLOW, "inf": Q_INF}[special]
    for R, K in SENTINEL_SHAPES:
        key = ("sentinel", f"{special}-R{R}-K{K}")
        qsel, cand = lists_sentinel(build, sq, R)
        q = build.queries[qsel]
        ids, dist = ctx.refine_l2_topk(q, cand, K)
        oid, odist = oracle.refine(build.base, build.dt, q, cand, K, mode=0)
        assert np.array_equal(ids, oid), f"{build.name} {key}: ids differ from the oracle\n{ids[4]}\n{oid[4]}"
        assert np.array_equal(dist.view(np.uint32), odist.view(np.uint32)), f"{build.name} {key}: distance bits differ"
        assert_padding(key, ids, dist)
        check_fp64(build, key, qsel[:4], cand[:4], K, ids[:4], dist[:4])
        m = min(K, len(valid_of(cand[4])))
        assert np.array_equal(ids[4, :m], np.sort(valid_of(cand[4]))[:m]) and (ids[4, m:] == PAD).all()   # all distances equal: by id
        if special == "big":      # fp32 cannot tell the rows apart (ulp(1.2e15) > 65504): an exactly equal group in fp32, within gamma in fp64
            assert (dist[4, :m] == dist[4, 0]).all() and 1e30 < dist[4, 0] < 2e30
            check_fp64(build, key, [Q_BIG], cand[4:], K, ids[4:], dist[4:], strict=False)
        else:
            assert np.isposinf(dist[4, :m]).all()


@gpu
def test_nan_query_leaves_the_rest_of_the_batch_exact(ctx, oracle, build):
    """One NaN element makes every distance of that query NaN.  The reference's behaviour is then ambiguous: `dist >= max_val`
    (cuda_refine.cu:267) is false for NaN, so a NaN replaces the current worst entry whenever the list is full, and the rescan
    for the new worst (`d[i] > max_val`, :272-278) never moves off entry 0 once that holds a NaN -- which candidates survive
    depends on the thread each one fell to.  The oracle keeps the first K in list order, the kernels the first K of each wave.
    Asserted is what holds either way: no fault, every other query of the batch bit-exact, and every id returned for the NaN
    query is a valid candidate or padding, padding last."""
    for R, K in SENTINEL_SHAPES:
        key = ("sentinel", f"nan-R{R}-K{K}")
        qsel, cand = lists_sentinel(build, Q_NAN, R)
        q = build.queries[qsel]
        ids, dist = ctx.refine_l2_topk(q, cand, K)
        oid, odist = oracle.refine(build.base, build.dt, q[:4], cand[:4], K, mode=0)
        assert np.array_equal(ids[:4], oid) and np.array_equal(dist[:4].view(np.uint32), odist.view(np.uint32)), f"{build.name} {key}"
        check_fp64(build, key, qsel[:4], cand[:4], K, ids[:4], dist[:4])
        got = ids[4]
        assert set(got[got != PAD].tolist()) <= set(valid_of(cand[4]).tolist())
        assert ((got == PAD)[1:] >= (got == PAD)[:-1]).all() and (dist[4].view(np.uint32)[got == PAD] == PAD_DIST_BITS).all()


def _dev_call(ctx, torch, stream, q, cand, K, want_dist=True, Qn=None, Rn=None, fill=0x5A):
    """nvdb_hip_refine_l2_topk_dev on torch-resident buffers and a non-default torch stream; outputs pre-filled with `fill` bytes."""
    dev = torch.device("cuda", 0)
    Q, R = cand.shape
    with torch.cuda.stream(stream):
        t_q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
        t_c = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.uint32).view(np.int32)).to(dev)
        t_i = torch.full((Q, max(K, 1)), fill * 0x01010101 - (1 << 32) * (fill >= 0x80), dtype=torch.int32, device=dev)
        t_d = torch.from_numpy(np.full((Q, max(K, 1)), fill * 0x01010101, dtype=np.uint32).view(np.float32)).to(dev)
        ctx.refine_l2_topk_dev(t_q.data_ptr(), t_c.data_ptr(), Q if Qn is None else Qn, R if Rn is None else Rn, K, t_i.data_ptr(),
                               t_d.data_ptr() if want_dist else None, stream.cuda_stream)
    stream.synchronize()
    return t_i.cpu().numpy().view(np.uint32), t_d.cpu().numpy()


@gpu
def test_device_entry_point_is_byte_identical_to_the_host_entry(ctx, build):
    """Resident queries, candidates and outputs on the caller's stream (what the host layer's cuda_l2_topk_batch sits on): the tie
    lists (both groups, both orders, straddling) and the size lists, then out_dist == null, then Q, R or K == 0 (NVDB_OK, outputs untouched)."""
    import torch
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    cases = [(lists_ties(build, desc, group), K) for group in GROUPS for desc in (False, True) for K in TIES_K]
    cases += [(lists_straddle(build, group), 10) for group in GROUPS]
    cases += [(lists_sizes(build, R), K) for R in SIZES_R for K in SIZES_K]
    for (qsel, cand), K in cases:
        q = build.queries[qsel]
        hi, hd = ctx.refine_l2_topk(q, cand, K)
        di, dd = _dev_call(ctx, torch, stream, q, cand, K)
        assert di.tobytes() == hi.tobytes() and dd.tobytes() == hd.tobytes(), (build.name, cand.shape, K)
    qsel, cand = lists_ties(build, True)
    q = build.queries[qsel]
    hi, _ = ctx.refine_l2_topk(q, cand, 10)
    di, dd = _dev_call(ctx, torch, stream, q, cand, 10, want_dist=False)
    assert di.tobytes() == hi.tobytes() and (dd.view(np.uint32) == 0x5A5A5A5A).all()          # ids as before, no distance written
    for Qn, Rn, K in ((0, None, 10), (None, 0, 10), (None, None, 0)):
        di, dd = _dev_call(ctx, torch, stream, q, cand, K, Qn=Qn, Rn=Rn)                       # raises unless NVDB_OK
        assert (di == 0x5A5A5A5A).all() and (dd.view(np.uint32) == 0x5A5A5A5A).all(), (Qn, Rn, K)


@gpu
def test_exemption_cap_on_what_the_gpu_returns(ctx, oracle, build):
    """Every finite case of this build once more, with all its assertions: at most 5 % of the (query, case) pairs may need the
    tie exemption."""
    pairs = exempt = 0
    for family, case, qsel, cand, K in finite_cases(build):
        exempt += run_counted(ctx, oracle, build, family, case, qsel, cand, K)[2]
        pairs += len(qsel)
    assert pairs >= 200 and exempt <= 0.05 * pairs, (build.name, exempt, pairs)
