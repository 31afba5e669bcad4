// masked_plan.h -- the arithmetic of the masked flat top-k on the MFMA filter route (nvdb_masked_flat.cpp, DESIGN.md section 4
// "Row masks"): when the route is taken, how many live rows the bootstrap prefix of a plane must hold (L), where that prefix ends
// (P), and how the prefix is cut into work items.  Pure functions of (n, k, cap, live counts) and of the batch shape; no HIP in
// them, so that the sanitizer build of tests/masked_plan_check.cpp compiles the very code the entry point and the prefix-rank
// kernel (kernels_masked_topk.h) run.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NVDB_MP_FN __host__ __device__ inline
#else
#define NVDB_MP_FN inline
#endif

namespace nvdbhip {

constexpr uint32_t MP_TILE_ROWS = 64;            // a prefix ends on a multiple of this many rows, or at n
constexpr uint32_t MP_FLOOR_MULT = 4;            // L >= 4 k: the bar comes from a sample that holds a few multiples of k
constexpr uint64_t MP_AUTO_MIN_ROWS = 1ull << 18;   // the automatic rule's own floor (below it one filter launch is the whole stream)
constexpr uint32_t MP_MAX_SEGMENTS = 256;        // work items a query group's prefix is cut into, at most
constexpr uint32_t MP_SEG_ROWS = 2048;           // ... and none of them shorter than this on average (PART_SEG_ROWS)

// smallest r with r * r >= k
NVDB_MP_FN uint32_t mp_sqrt_ceil(uint32_t k) {
  uint32_t r = 0;
  while (static_cast<uint64_t>(r) * r < k) ++r;
  return r;
}

// With the bar at the k-th best of L live rows, about (rows / L) * G of the rows the filter streams score above it, G the k-th
// arrival of a unit-rate Poisson process (mean k, deviation sqrt(k)) -- `rows`, not the plane's live count: the filter knows no
// masks, a dead row above the bar takes a list entry until the keep step drops it, and a list overflows on what it holds BEFORE that
// step.  G stays below k + 6 sqrt(k) + 8 but for a share of < 1e-6 of the queries at every k <= 64 (k = 1: e^-15; k = 10: 4e-8;
// k = 64: seven deviations).
NVDB_MP_FN uint32_t mp_units(uint32_t k) { return k + 6u * mp_sqrt_ceil(k) + 8u; }

// L: live rows the bootstrap prefix must hold so that (rows / L) * mp_units(k) <= cap, and at least MP_FLOOR_MULT * k.  A plane
// with fewer live rows than that has the whole corpus as its prefix.  64-bit throughout (rows < 2^32, units < 2^7).
NVDB_MP_FN uint64_t mp_boot_live(uint32_t k, uint32_t cap, uint64_t rows) {
  const uint64_t c = cap ? cap : 1u;
  const uint64_t need = (rows * mp_units(k) + c - 1) / c;
  const uint64_t floor_l = static_cast<uint64_t>(MP_FLOOR_MULT) * k;
  return need > floor_l ? need : floor_l;
}

// A plane with fewer than MP_FLOOR_MULT * k live rows gives no bar worth a stream: its k-th best live score sits among the bulk of
// the corpus' scores and every list would overflow.  Its prefix is the corpus (L >= MP_FLOOR_MULT * k > live), so the bootstrap has
// seen every live row and its answer is final.
NVDB_MP_FN bool mp_boot_final(uint32_t k, uint64_t live) { return live < static_cast<uint64_t>(MP_FLOOR_MULT) * k; }

// the prefix that ends with 64-row tile `tile` (the first whose running live count reaches L): a multiple of 64, or n
NVDB_MP_FN uint64_t mp_prefix_end(uint64_t n, uint64_t tile) {
  const uint64_t e = (tile + 1) * MP_TILE_ROWS;
  return e < n ? e : n;
}

// a plane without a mask: every row is live, the prefix is L rounded up to whole tiles
NVDB_MP_FN uint64_t mp_prefix_unmasked(uint64_t n, uint32_t k, uint32_t cap) {
  const uint64_t L = mp_boot_live(k, cap, n);
  if (L >= n) return n;
  return mp_prefix_end(n, (L - 1) / MP_TILE_ROWS);
}

// P of a plane (W = ceil(n / 32) words, tail bits 0): the smallest multiple of 64 -- or n -- whose prefix holds L live rows; n
// where the plane holds fewer.  The host restatement of the prefix-rank kernel.
inline uint64_t mp_prefix_rows(const uint32_t* plane, uint64_t n, uint32_t k, uint32_t cap) {
  const uint64_t W = (n + 31) / 32;
  uint64_t live = 0;
  for (uint64_t w = 0; w < W; ++w) live += static_cast<uint64_t>(__builtin_popcount(plane[w]));
  const uint64_t L = mp_boot_live(k, cap, n);
  if (live < L) return n;
  uint64_t run = 0;
  for (uint64_t t = 0; t * MP_TILE_ROWS < n; ++t) {
    run += static_cast<uint64_t>(__builtin_popcount(plane[2 * t]));
    if (2 * t + 1 < W) run += static_cast<uint64_t>(__builtin_popcount(plane[2 * t + 1]));
    if (run >= L) return mp_prefix_end(n, t);
  }
  return n;
}

// rows [lo, hi) of segment s of S over a prefix of P rows, cut at tile boundaries; lo == hi: the prefix has fewer tiles than segments
NVDB_MP_FN void mp_segment(uint64_t P, uint32_t s, uint32_t S, uint32_t* lo, uint32_t* hi) {
  const uint64_t T = (P + MP_TILE_ROWS - 1) / MP_TILE_ROWS;
  const uint64_t a = T * s / S * MP_TILE_ROWS, b = T * (s + 1) / S * MP_TILE_ROWS;
  *lo = static_cast<uint32_t>(a < P ? a : P);
  *hi = static_cast<uint32_t>(b < P ? b : P);
}

// segments per query group: enough work items to fill the device four times over, none shorter than MP_SEG_ROWS were the prefix
// the whole corpus, at most MP_MAX_SEGMENTS
inline uint32_t mp_segments(uint64_t n, uint32_t groups, uint32_t num_cu) {
  const uint64_t by_rows = (n + MP_SEG_ROWS - 1) / MP_SEG_ROWS;
  uint64_t s = (4ull * num_cu) / (groups ? groups : 1u);
  if (s > by_rows) s = by_rows;
  if (s > MP_MAX_SEGMENTS) s = MP_MAX_SEGMENTS;
  return s ? static_cast<uint32_t>(s) : 1u;
}

// The automatic route (option path = 0) of one sub-batch of nq queries: the range search's rule (plan_range) and a floor of
// MP_AUTO_MIN_ROWS rows.  Below the floor the route's fixed steps (prefix rank, bootstrap, bar, verdict read-back) stand against a
// scan of microseconds.
// (mp_filter_pays, below, is the rule's second half)
inline bool mp_auto_filter(bool filter_supported, uint32_t nq, int64_t min_filter_batch, uint64_t n, int64_t chunk0) {
  if (!filter_supported || static_cast<int64_t>(nq) < min_filter_batch) return false;
  if (chunk0 > 0 && n < 4ull * static_cast<uint64_t>(chunk0)) return false;
  return n >= MP_AUTO_MIN_ROWS;
}

// ... and, behind it, what the two routes cost in units of one group's scan of the whole corpus (thousandths): the scan walks the
// corpus once per query group; the filter route streams it once -- MP_STREAM_MILLI, measured: fp16 d = 768, 10M rows, a stream with
// its fixed steps takes 0.65 of a 16-query group's scan -- and walks each plane's prefix, about n * L / live_m rows, once per group
// of that plane.  groups[i] / live[i]: query groups and (estimated) live rows of the sub-batch's i-th distinct plane.  A thin plane
// on a batch of one or two groups stays on the scan: its prefix is most of the corpus.
constexpr uint64_t MP_STREAM_MILLI = 650;
inline bool mp_filter_pays(uint64_t n, uint32_t k, uint32_t cap, uint32_t nplanes, const uint32_t* groups, const uint64_t* live) {
  const uint64_t L = mp_boot_live(k, cap, n);
  uint64_t scan = 0, filter = MP_STREAM_MILLI;
  for (uint32_t i = 0; i < nplanes; ++i) {
    const uint64_t share = live[i] > L ? (1000u * L + live[i] - 1) / live[i] : 1000u;    // P / n, at most 1
    scan += 1000ull * groups[i];
    filter += share * groups[i];
  }
  return filter < scan;
}

}  // namespace nvdbhip
