"""Adversarial corpora for the MFMA filters' error bounds: plain numpy, fp64 and integers, no GPU, no library.

Every fast route keeps a row only while its FILTER value stays inside a band under a bar: `tau - 2 E_q` (top-k), `radius - E_q`
(range search, masked flat route, the int8 shadow's exact bar), and the int8 two-stage kernels multiply the lo plane only where
`128 H scale >= T - qdelta`.  Random data uses a few per cent of those bands.  `build(family, dim)` plants, around ONE query,

  * a VICTIM row: the exact k-th best, whose filter value understates its score by as much as the geometry allows,
  * k + 8 DECOY rows: exact scores strictly below the victim's, filter values that overstate,
  * k - 1 TOP rows well above both, and random FILLER rows (norm 0.5 .. 0.8) far below,

and restates the filter's documented arithmetic to say where every planted row's filter value lands ("model filter") and what
bound the library grants ("model E_q").  Geometry ("split support"): the columns are two halves A and B; the victim lives on A,
the decoys on B, and whatever is rounded (the query's elements, the rows' elements) is rounded towards zero on A and away from
zero on B by almost half a step.  Cauchy-Schwarz at |A| = dim / 2 then gives an error of 1 / sqrt(2) of the bound's worst case.

Families (canonical row ids: victim 0, decoys 1 .. k + 8, tops k + 9 .. 2k + 7, fillers behind):
  F16   fp16 corpus, fp16 filter.  Prescaled query elements sit 2^-7 under (A) / over (B) the midpoint of two adjacent halves
        just above 2^14; rows are +-2^-4 on their half.  Error per row 2^-11 / sqrt(2) of ||q|| max||x||.
  F32   fp32 corpus through its fp16 shadow: the same query, and the ROWS' elements a few fp32 ulps under / over a half midpoint.
  I8Q   int8 corpus: q_i = s_q (t_i +- 0.499), |t_i| around 200 (the fp32 product q_i / s_q then still rounds as planned: the
        builder checks it), one anchor column at t = 16256 that pins s_q; rows +-127 on their half, decoys with a smaller scale.
  I8LO  int8 corpus, the two-stage test: a query that IS its quantisation (no filter error at all) with lo = -64 on every
        column but the anchor and hi planes that sum to zero; the victim is -127 on those columns, so <hi, x> = 0 and its whole
        value is the lo plane's -- Cauchy-Schwarz equality for qdelta.  Decoys: the same row at smaller scales.
  SH8   fp16 corpus filtered through its int8 shadow: the victim's elements are (63 + 15/32) row scales (the closest an fp16
        value of that size comes to a half step: residual 0.469 instead of 0.5), the decoys' (62 + 17/32); the query is exactly
        representable, because its quantisation is 1 % of this bound.  The victim holds the corpus' largest residual AND norm.

REACHED SHARES, asserted by tests/test_filter_bound_cpu.py from this model alone (never from a GPU run):
  `share_topk`  = (best decoy's model filter - victim's model filter) / (2 model E_q)
  `share_range` = (victim's exact score - victim's model filter) / model E_q          (radius = the victim's exact score)
  I8LO          = (bar - 128 H scale) / qdelta with bar = victim's value - 2 E_q (top-k) or - E_q (range): the part of qdelta in use.

  family   derived                                     model gives (every dim)      why less
  F16      2^-11 / sqrt(2) / 7.5e-4 = 0.460            0.448 .. 0.452 (range 0.453) the decoys' deficit, mantissas up to 3 % over 1.0, the 1.0001 factors
  I8Q      0.499 / (0.5005 * 1.001 * sqrt(2)) = 0.704  0.688 .. 0.695 (0.691 .. 0.697) the anchor column: 1e-5 ||q|| in E_q, |A| = dim/2 - 1
  I8LO     1 - 2 E_q / qdelta = 0.984                  0.984 (top-k) 0.992 (range)  E_q / qdelta = 0.5005 / 64; Cauchy-Schwarz itself is tight
  SH8      1 / sqrt(2) = 0.707                         0.693 (0.692)                the query's own 1 % of E_q is not attacked; 1.001 * 1.0001^2
  F32      2 * 2^-11 / sqrt(2) / 12.4e-4 = 0.557       0.549 (0.551)                as F16
Every one is within 5 % of the derived value, which is what the CPU module asserts; none had to be lowered.  The first-stage test of
I8LO compares with the bar a row meets WHEN IT STREAMS, so only placement 1 (decoys in the bootstrap, victim in the last tile, tiles in
storage order) puts qdelta at its edge; the bands under tau are tested by the selects after every chunk, whatever the order.
"""
import numpy as np

K = 10
N = 65541                      # 2^16 + 5: no multiple of a tile (16 / 32 / 64 rows), and the smallest size at which the planner no longer
                               # widens the bootstrap to save a chunk, so every build runs a bootstrap (d > 768: an exact first chunk) and >= 2 filter chunks
N_DECOY = K + 8
N_TOP = K - 1
N_PLANTED = 1 + N_DECOY + N_TOP
VICTIM = 0
DECOYS = list(range(1, 1 + N_DECOY))
TOPS = list(range(1 + N_DECOY, N_PLANTED))
FILTER_REL_F16 = 7.5e-4
F32_SHADOW_REL, F32_SHADOW_ABS = 4.9e-4, 3.0e-8
FILLER_NORM = {"F16": 0.8, "F32": 0.8, "I8Q": 0.5, "I8LO": 0.5, "SH8": 0.6}   # SH8: so that no filler's quantisation residual reaches the victim's

# the shares derived in the docstring's table, and what a test may lose to the discreteness of the representable values
DERIVED = {
    "F16": 2.0 ** -11 / np.sqrt(2.0) / FILTER_REL_F16,
    "F32": 2.0 * 2.0 ** -11 / np.sqrt(2.0) / (FILTER_REL_F16 + F32_SHADOW_REL),
    "I8Q": 0.499 / (0.5005 * 1.001 * np.sqrt(2.0)),
    "I8LO": 1.0 - 2.0 * 0.5005 / 64.0,
    "SH8": 1.0 / np.sqrt(2.0),
}
SLACK = 0.05
FAMILIES = ("F16", "I8Q", "I8LO", "SH8", "F32")
DTYPE_OF = {"F16": "f16", "F32": "f32", "I8Q": "i8", "I8LO": "i8", "SH8": "f16"}


class Case:
    """What build() returns.  rows: [N, dim] float16 / float32 / int8; scales: [N] float32 (int8) or None; query: [dim] float32;
    exact: [N] fp64 scores of the query; expected: ids of the k best by (score desc, id asc); model_filter: [N_PLANTED] fp64;
    E: model E_q; qdelta: model lo-plane allowance (int8) or None; budget: the terms of E and what the victim uses of each."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def err_victim(self):
        return self.exact[VICTIM] - self.model_filter[VICTIM]

    @property
    def best_decoy(self):
        return max(DECOYS, key=lambda r: self.model_filter[r])


# ------------------------------------------------------------------------------------------------ the documented arithmetic
def f32(x):
    return np.asarray(x, dtype=np.float32)


def prescale_exponent(q):
    """prep_q16_kernel: 2^e with max|q| 2^e in [2^14, 2^15)."""
    _, ex = np.frexp(np.float32(np.max(np.abs(q))))
    return 15 - int(ex)


def q16_of(q):
    """The scaled half copy of a query (values as fp64) and e: the product by a power of two is exact, the cast rounds to nearest even."""
    e = prescale_exponent(q)
    return f32(np.ldexp(f32(q), e)).astype(np.float16).astype(np.float64), e


def model_filter_f16(q, rows16):
    """sum half(q_i 2^e) x_i 2^-e; rows16: values the fp16 filter streams (float16).  Exact in fp64 (22 + 11 bits per product)."""
    qh, e = q16_of(q)
    return np.ldexp(rows16.astype(np.float64) @ qh, -e)


def model_E_f16(q, max_norm, fp32_corpus, dim):
    nrm = np.sqrt(np.sum(q.astype(np.float64) ** 2)) * 1.0001
    rel = FILTER_REL_F16 + (F32_SHADOW_REL if fp32_corpus else 0.0)
    return rel * nrm * max_norm + (F32_SHADOW_ABS * np.sqrt(dim) * nrm if fp32_corpus else 0.0)


def quantise_query(q):
    """prep_q8_kernel with lo_bits = 7, in its own fp32 steps: s_q = max|q| / 16256, t = rint(q * (1 / s_q)), hi = (t + 64) >> 7."""
    sq = np.float32(np.max(np.abs(q))) / np.float32(16256.0)
    isq = np.float32(1.0) / sq
    t = np.clip(np.rint(f32(q) * isq), -16256, 16256).astype(np.int64)
    hi = (t + 64) >> 7
    lo = t - (hi << 7)
    assert np.sum(np.abs(hi)) <= 65500 - len(q), "the hi plane's L1 norm would make prep_q8_kernel quantise more coarsely"
    return float(sq), t, hi, lo


def model_E_i8(q, sq, filter_max_norm, resid_max=0.0):
    """prep_q8_kernel's ebound and its two parts (query quantisation + fp32 chains, corpus residual)."""
    nrm = np.sqrt(np.sum(q.astype(np.float64) ** 2)) * 1.0001
    quant = (0.5005 * np.sqrt(len(q)) * sq + 1.0e-5 * nrm) * filter_max_norm * 1.001
    resid = nrm * resid_max * 1.001
    return quant + resid, quant, resid


def shadow_q8(rows):
    """shadow_q8_kernel (the reference quantiser's rule, apps/nvdb_quantize_i8.cpp:71-80) in fp32 steps: scale = max|x| / 127,
    rint(x * (1 / scale)) clamped to +-127 -> (int values, scales, residual norm per row)."""
    x = f32(rows)
    if len(x) > CHUNK:
        parts = [shadow_q8(rows[lo:lo + CHUNK]) for lo in range(0, len(rows), CHUNK)]
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    mx = np.max(np.abs(x), axis=1)
    scale = np.where(mx > 0, mx / np.float32(127.0), np.float32(1.0)).astype(np.float32)
    inv = (np.float32(1.0) / scale).astype(np.float32)
    qv = np.clip(np.rint(x * inv[:, None]), -127, 127)
    d = x.astype(np.float64) - qv.astype(np.float64) * scale.astype(np.float64)[:, None]
    return qv.astype(np.int8), scale, np.sqrt(np.sum(d * d, axis=1))


# ------------------------------------------------------------------------------------------------ pieces shared by the families
CHUNK = 8192


def values64(rows, scales, lo=0, hi=None):
    """Rows [lo, hi) as the fp64 values the exact score multiplies (int8: times the row scale)."""
    v = rows[lo:hi].astype(np.float64)
    return v if scales is None else v * scales[lo:hi].astype(np.float64)[:, None]


def _chunked(fn, n):
    return np.concatenate([fn(lo, min(lo + CHUNK, n)) for lo in range(0, n, CHUNK)])


def norms64(rows, scales=None):
    return _chunked(lambda lo, hi: np.sqrt(np.sum(values64(rows, scales, lo, hi) ** 2, axis=1)), len(rows))


def scores64(rows, scales, q):
    q64 = q.astype(np.float64)
    return _chunked(lambda lo, hi: values64(rows, scales, lo, hi) @ q64, len(rows))


def _fillers(rs, n, dim, norm, zero_col0=False):
    g = np.random.default_rng(rs.randint(1 << 30)).standard_normal((n, dim), dtype=np.float32)
    g *= (norm / np.sqrt(np.sum(g.astype(np.float64) ** 2, axis=1)))[:, None].astype(np.float32)
    if zero_col0:
        g[:, 0] = 0.0
    return g


def _quantise_rows(g):
    """int8 rows of fp64 rows by the reference's rule (numpy twin; only used for the filler rows)."""
    scale = f32(np.max(np.abs(g), axis=1).astype(np.float64) / 127.0)
    return np.clip(np.rint(g / scale[:, None]), -127, 127).astype(np.int8), scale


def _mirrored(rs, h, lo, hi):
    """h random integers in [lo, hi) and a shuffled copy: two halves with the same multiset."""
    a = rs.randint(lo, hi, size=h)
    return a, rs.permutation(a)


def _finish(family, dim, rows, scales, query, norms, model_filter, E, **extra):
    exact = scores64(rows, scales, query)
    order = np.lexsort((np.arange(len(exact)), -exact))
    c = Case(family=family, dim=dim, dtype=DTYPE_OF[family], rows=rows, scales=scales, query=query, exact=exact,
             expected=order[:K].copy(), order=order, model_filter=np.asarray(model_filter[:N_PLANTED], dtype=np.float64), E=float(E),
             norms=norms, qdelta=None, **extra)
    if family == "I8LO":
        c.qdelta = extra["budget"]["lo_plane_allowance"]
        h128 = extra["budget"]["victim_hi_part"]
        c.share_topk = (c.model_filter[VICTIM] - 2.0 * c.E - h128) / c.qdelta
        c.share_range = (c.exact[VICTIM] - c.E - h128) / c.qdelta
    else:
        c.share_topk = (c.model_filter[c.best_decoy] - c.model_filter[VICTIM]) / (2.0 * c.E)
        c.share_range = (c.exact[VICTIM] - c.model_filter[VICTIM]) / c.E
    return c


# ------------------------------------------------------------------------------------------------ F16 / F32
def _f16_query(rs, dim):
    """Prescaled elements 2^14 + 16 m + 8 -+ 2^-7 (ulp of a half there: 16), times 2^-19: ||q|| ~ 0.87 at d = 768."""
    h = dim // 2
    ma, mb = _mirrored(rs, h, 0, 32)
    sign = rs.choice([-1.0, 1.0], size=dim)
    v = np.concatenate([16384.0 + 16.0 * ma + 8.0 - 2.0 ** -7, 16384.0 + 16.0 * mb + 8.0 + 2.0 ** -7])
    q = f32(np.ldexp(sign * v, -19))
    assert np.array_equal(q.astype(np.float64), np.ldexp(sign * v, -19))
    return q, sign, h


def _build_f16(dim, seed, fp32_corpus):
    rs = np.random.RandomState(seed)
    q, sign, h = _f16_query(rs, dim)
    c = 2.0 ** -4                                            # ||victim|| = 2^-4 sqrt(dim / 2) = 1.22 at d = 768
    if fp32_corpus:
        # rows a few fp32 ulps under (victim) / over (decoys) the midpoint c (1 + 2^-11) of the halves c and c (1 + 2^-10);
        # a decoy's lowered elements sit just over the midpoint c (1 - 2^-12) of the halves under c
        mid, low = np.float32(c * (1 + 2.0 ** -11)), np.float32(c * (1 - 2.0 ** -12))
        v_el, d_el, d_low = np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1)), np.nextafter(low, np.float32(1))
        dt = np.float32
    else:
        v_el = d_el = np.float16(c)
        d_low = np.nextafter(np.float16(c), np.float16(0))   # the half under 2^-4
        dt = np.float16
    rows = np.zeros((N, dim), dtype=dt)
    rows[VICTIM, :h] = (sign[:h] * dt(v_el)).astype(dt)
    for j, r in enumerate(DECOYS):
        el = np.full(dim - h, d_el, dtype=dt)
        el[rs.choice(dim - h, 4 * (j + 1), replace=False)] = d_low
        rows[r, h:] = (sign[h:] * el).astype(dt)
    for j, r in enumerate(TOPS):                             # aligned with the whole query: 0.55 .. 0.67 of c on every column
        rows[r] = (sign * np.float16(c * (0.55 + 0.015 * j))).astype(dt)
    rows[N_PLANTED:] = _fillers(rs, N - N_PLANTED, dim, FILLER_NORM["F16"]).astype(np.float16).astype(dt)
    norms = norms64(rows)
    max_norm = float(np.max(norms)) * 1.0001
    streamed = rows[:N_PLANTED].astype(np.float16)           # shadow_f16_kernel: round to nearest even
    mf = model_filter_f16(q, streamed)
    E = model_E_f16(q, max_norm, fp32_corpus, dim)
    qh, e = q16_of(q)
    x_v = rows[VICTIM].astype(np.float64)
    budget = dict(query_rounding=float(np.ldexp(np.sum((np.ldexp(q.astype(np.float64), e) - qh) * x_v), -e)),
                  row_rounding=float(np.sum(q.astype(np.float64) * (x_v - streamed[VICTIM].astype(np.float64)))),
                  accumulation_allowance=4.6e-5 / FILTER_REL_F16, residual=0.0, lo_plane=0.0)
    return _finish("F32" if fp32_corpus else "F16", dim, rows, None, q, norms, mf, E, budget=budget, max_norm=max_norm)


# ------------------------------------------------------------------------------------------------ I8Q / I8LO
def _build_i8q(dim, seed):
    rs = np.random.RandomState(seed)
    h = dim // 2
    na = h - 1                                               # column 0: the anchor; A = [1, h), B = [h, dim - 1): |A| = |B|
    ta, tb = _mirrored(rs, na, 150, 250)
    sq = 2.0 ** -14
    sign = rs.choice([-1, 1], size=dim)
    t = np.zeros(dim, dtype=np.int64)
    t[0], t[1:h], t[h:dim - 1], t[dim - 1] = 16256, ta, tb + 1, 200
    t *= sign
    off = np.zeros(dim)
    off[1:h], off[h:] = 0.499, -0.499                        # |q| = s_q (|t| + 0.499) on A: t understates; B: overstates
    q = f32(sq * (t + sign * off))
    got_sq, got_t, hi, lo = quantise_query(q)
    assert got_sq == sq and np.array_equal(got_t, t), "the planned quantisation is not what the fp32 steps give"
    rows = np.zeros((N, dim), dtype=np.int8)
    scales = np.zeros(N, dtype=np.float32)
    s_v = np.float32(1.25 / (127.0 * np.sqrt(na)))
    rows[VICTIM, 1:h] = 127 * sign[1:h]
    scales[VICTIM] = s_v
    for j, r in enumerate(DECOYS):                           # sum_B |q| exceeds sum_A |q| by 0.002 |A| s_q = 1e-5 of it: the scale makes up for it
        rows[r, h:dim - 1] = 127 * sign[h:dim - 1]
        scales[r] = np.float32(float(s_v) * (1.0 - 2.0e-5 - 1.0e-5 * (j + 1)))
    for j, r in enumerate(TOPS):
        rows[r] = 8 * sign
        rows[r, 0] = 127 * sign[0]
        scales[r] = np.float32(1.25 * (0.45 + 0.05 * j) / np.sqrt(127.0 ** 2 + 64.0 * (dim - 1)))
    rows[N_PLANTED:], scales[N_PLANTED:] = _quantise_rows(_fillers(rs, N - N_PLANTED, dim, FILLER_NORM["I8Q"], zero_col0=True))
    norms = norms64(rows, scales)
    max_norm = float(np.max(norms)) * 1.0001
    mf = (rows[:N_PLANTED].astype(np.int64) @ t).astype(np.float64) * scales[:N_PLANTED].astype(np.float64) * sq
    E, quant, _ = model_E_i8(q, sq, max_norm)
    budget = dict(query_rounding=float(np.sum((q.astype(np.float64) - sq * t) * values64(rows, scales, VICTIM, VICTIM + 1)[0])), query_rounding_allowance=quant,
                  residual=0.0, lo_plane=float(np.sum(lo * rows[VICTIM].astype(np.int64))) * float(s_v) * sq,
                  lo_plane_allowance=float(np.sqrt(np.sum(lo * lo))) * max_norm * 1.0001 * sq)
    return _finish("I8Q", dim, rows, scales, q, norms, mf, E, budget=budget, max_norm=max_norm)


def _build_i8lo(dim, seed):
    rs = np.random.RandomState(seed)
    sq = 2.0 ** -14
    m = dim - 1
    hi_plane = np.zeros(m, dtype=np.int64)
    hi_plane[:m // 2], hi_plane[m // 2:2 * (m // 2)] = 3, -3  # sums to zero (an odd column keeps hi = 0)
    hi_plane = rs.permutation(hi_plane)
    t = np.concatenate([[16256], 128 * hi_plane - 64])        # lo = -64 on every column but the anchor (t = 127 * 128: lo = 0)
    q = f32(sq * t)
    got_sq, got_t, hi, lo = quantise_query(q)
    assert got_sq == sq and np.array_equal(got_t, t) and np.all(lo[1:] == -64) and lo[0] == 0 and np.sum(hi[1:]) == 0
    rows = np.zeros((N, dim), dtype=np.int8)
    scales = np.zeros(N, dtype=np.float32)
    s_v = np.float32(1.25 / (127.0 * np.sqrt(m)))
    for j, r in enumerate([VICTIM] + DECOYS):                 # the decoys: the victim's row at smaller scales, all inside the band
        rows[r, 1:] = -127
        scales[r] = np.float32(float(s_v) * (1.0 - 2.0e-4 * j))
    sg = np.sign(t).astype(np.int64)
    for j, r in enumerate(TOPS):
        rows[r] = 8 * sg
        rows[r, 0] = 127
        scales[r] = np.float32(1.25 * (0.45 + 0.05 * j) / np.sqrt(127.0 ** 2 + 64.0 * m))
    rows[N_PLANTED:], scales[N_PLANTED:] = _quantise_rows(_fillers(rs, N - N_PLANTED, dim, FILLER_NORM["I8Q"], zero_col0=True))
    norms = norms64(rows, scales)
    max_norm = float(np.max(norms)) * 1.0001
    mf = (rows[:N_PLANTED].astype(np.int64) @ t).astype(np.float64) * scales[:N_PLANTED].astype(np.float64) * sq
    E, quant, _ = model_E_i8(q, sq, max_norm)
    H = int(np.sum(hi * rows[VICTIM].astype(np.int64)))
    budget = dict(query_rounding=0.0, query_rounding_allowance=quant, residual=0.0,
                  victim_hi_part=128.0 * H * float(s_v) * sq,
                  lo_plane=float(np.sum(lo * rows[VICTIM].astype(np.int64))) * float(s_v) * sq,
                  lo_plane_allowance=float(np.sqrt(np.sum(lo * lo))) * max_norm * 1.0001 * sq)
    return _finish("I8LO", dim, rows, scales, q, norms, mf, E, budget=budget, max_norm=max_norm)


# ------------------------------------------------------------------------------------------------ SH8
def _build_sh8(dim, seed):
    rs = np.random.RandomState(seed)
    h = dim // 2 + 1                                          # A = [1, h): dim / 2 columns, B = [h, dim): one fewer, so the victim's residual is the largest
    na, nb = h - 1, dim - h                                   # column 0: anchor of the query AND of every planted row's scale
    sq, rscale = 2.0 ** -18, 2.0 ** -10
    v_el, d_el = 2031, 2001                                   # in 1/32 row scales: 63 + 15/32 (rounds to 63), 62 + 17/32 (rounds to 63)
    t_b = 8000
    t_a = (t_b * nb * d_el) // (na * v_el) + 1                # the victim's score just above an unlowered decoy's
    sign = rs.choice([-1, 1], size=dim)
    t = np.concatenate([[16256], np.full(na, t_a), np.full(nb, t_b)]) * sign
    q = f32(sq * t)
    got_sq, got_t, _, _ = quantise_query(q)
    assert got_sq == sq and np.array_equal(got_t, t)
    rows = np.zeros((N, dim), dtype=np.float16)
    rows[VICTIM, 0] = 127 * rscale * sign[0]
    rows[VICTIM, 1:h] = sign[1:h] * (v_el / 32.0 * rscale)
    for j, r in enumerate(DECOYS):
        el = np.full(nb, d_el, dtype=np.float64)
        el[rs.choice(nb, j, replace=False)] -= 32.0           # one row scale less: same residual, a lower score
        rows[r, 0] = 127 * rscale * sign[0]
        rows[r, h:] = sign[h:] * (el / 32.0 * rscale)
    for j, r in enumerate(TOPS):                              # one magnitude on every column: no residual
        rows[r] = sign * np.float16(0.033 + 0.001 * j)
    rows[N_PLANTED:] = _fillers(rs, N - N_PLANTED, dim, FILLER_NORM["SH8"]).astype(np.float16)
    x_v = rows[VICTIM].astype(np.float64)
    assert np.array_equal(x_v[1:h], sign[1:h] * (v_el / 32.0 * rscale)), "not fp16 values"
    qv, scale, resid = shadow_q8(rows)
    fmn = float(np.max(norms64(qv, scale))) * 1.0001
    resid_max = float(np.max(resid)) * 1.0001
    mf = (qv[:N_PLANTED].astype(np.int64) @ t).astype(np.float64) * scale[:N_PLANTED].astype(np.float64) * sq
    E, quant, res = model_E_i8(q, sq, fmn, resid_max)
    budget = dict(query_rounding=0.0, query_rounding_allowance=quant, residual=float(np.sum(q.astype(np.float64) * (x_v - values64(qv, scale, VICTIM, VICTIM + 1)[0]))),
                  residual_allowance=res, lo_plane=0.0)
    norms = norms64(rows)
    return _finish("SH8", dim, rows, None, q, norms, mf, E, budget=budget, resid=resid, resid_max=resid_max, filter_max_norm=fmn,
                   max_norm=float(np.max(norms)) * 1.0001)


_CACHE = {}


def build(family, dim):
    """The case of (family, dim); built once per process."""
    key = (family, dim)
    if key not in _CACHE:
        seed = 7000 + 131 * FAMILIES.index(family) + dim
        if family in ("F16", "F32"):
            _CACHE[key] = _build_f16(dim, seed, family == "F32")
        elif family == "I8Q":
            _CACHE[key] = _build_i8q(dim, seed)
        elif family == "I8LO":
            _CACHE[key] = _build_i8lo(dim, seed)
        elif family == "SH8":
            _CACHE[key] = _build_sh8(dim, seed)
        else:
            raise ValueError(family)
    return _CACHE[key]


def drop(family, dim):
    _CACHE.pop((family, dim), None)


# every (family, dim) the GPU module runs: one per distinct filter kernel build (nvdb_launch_f16.cpp / nvdb_launch_i8.cpp)
CASES = [("F16", 768), ("F16", 384), ("F16", 600), ("F16", 1536),
         ("I8Q", 768), ("I8Q", 384), ("I8Q", 1536),
         ("I8LO", 768), ("I8LO", 384), ("I8LO", 1536),
         ("SH8", 768), ("F32", 768)]


def bound_pct(family, dim):
    """The shrunk bound of the teeth runs: 80 % of the share the case reaches, so the case must fail under it."""
    return int(np.floor(80.0 * build(family, dim).share_topk))


# ------------------------------------------------------------------------------------------------ placements
def placement(kind):
    """pos[canonical id] = row of the uploaded corpus.
    0: victim in row 0, decoys in the last rows (the last chunk when tiles stream in storage order), tops in the middle;
    1: victim in row N - 1 (the partial last tile), decoys and tops one per 32-row tile at the front (the bootstrap prefix);
    2: victim and decoys in ONE 32-row tile in the middle of the corpus."""
    pos = np.full(N, -1, dtype=np.int64)
    if kind == 0:
        pos[VICTIM] = 0
        pos[DECOYS] = N - 2 - 37 * np.arange(N_DECOY)
        pos[TOPS] = 5000 + 41 * np.arange(N_TOP)
    elif kind == 1:
        pos[VICTIM] = N - 1
        pos[DECOYS] = 33 * (1 + np.arange(N_DECOY))
        pos[TOPS] = 1000 + 33 * np.arange(N_TOP)
    else:
        pos[VICTIM] = 32768 + 5
        pos[DECOYS] = 32768 + 6 + np.arange(N_DECOY)
        pos[TOPS] = 50000 + 41 * np.arange(N_TOP)
    free = np.ones(N, dtype=bool)
    free[pos[:N_PLANTED]] = False
    pos[N_PLANTED:] = np.flatnonzero(free)
    assert len(np.unique(pos)) == N
    return pos


def permuted(a, pos):
    """a (rows, scales, a score vector ...) indexed by canonical id -> indexed by uploaded row."""
    out = np.empty_like(a)
    out[pos] = a
    return out
