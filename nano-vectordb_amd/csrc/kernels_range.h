// kernels_range.h -- exact range search: every row whose reference-order score reaches a per-query radius
// (nvdb_hip_range_search; orchestration in nvdb_range.cpp, DESIGN.md section 4 "range search").
//
// Filter route (the MFMA filter kernels as they are, streamed once at FIXED thresholds):
//   range_thr_kernel      thr[q] = radius[q] - E_q (a row with exact score >= radius has filter score >= radius - E_q);
//                         queries without a usable threshold are flagged and given +inf
//   (filter launches, rescore launch: the flat search's kernels)
//   range_keep_kernel     one workgroup per query over its re-scored list: drop what misses the radius, order the rest
//                         (score desc, id asc) in LDS, write it back as the query's slab with its count (range_keep_body<MASKED>:
//                         also behind range_keep_masked_kernel of kernels_range_parts.h)
//   range_pack_kernel     slabs -> the packed id / score arrays at the offsets of the exclusive scan (done on the host
//                         over the downloaded counts), ids made global
// Exact route (any dtype / dim; the queries the filter route flagged): the any-k path's score matrix, then
//   range_count_kernel    per query, the scores >= radius
//   range_collect_kernel  their key64_of keys into the query's slab (padded to a power of two with key 0)
//   (bitonic_lds_kernel / bitonic_global_step_kernel of kernels_largek.h sort the slabs)
//   range_emit_kernel     ids and the scores' original bits from the sorted keys, straight into the packed arrays
// Membership is the C comparison score >= radius everywhere: a NaN score or a NaN radius never passes, +0.0 == -0.0.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_largek.h"
#include "range_plan.h"               // RangeDesc

namespace nvdbhip {

// grid = ceil(nq_pad / 256), block = 256.  overflow[q] arrives from the prep launch (1: a non-finite query element).
static __global__ __launch_bounds__(256) void range_thr_kernel(const float* __restrict__ radius, const float* __restrict__ ebound, float* __restrict__ thr,
                                                               uint32_t* __restrict__ overflow, uint32_t nq, uint32_t nq_pad) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= nq_pad) return;
  float t = __builtin_huge_valf();
  if (q < nq) {
    const float r = radius[q], eb = ebound[q];
    // the kernels compare filter * s_q with thr * s_q: 2^-20 relative covers the rounding of the subtraction, of that
    // product (s_q is not a power of two for int8 queries) and of the filter value's own scaling, each <= 2^-24
    float d = r - eb;
    d = d - 9.5367431640625e-7f * __builtin_fabsf(d);
    const bool ok = overflow[q] == 0u && eb >= 0.f && __builtin_fabsf(r) < __builtin_huge_valf() && __builtin_fabsf(d) < __builtin_huge_valf();
    if (ok) t = d;
    else overflow[q] = 1u;           // answered by the exact route; +inf: the filter files nothing for it
  }
  thr[q] = t;
}

// The keep step of one query's re-scored list (one workgroup of 256): drop what misses the radius -- MASKED: and what is dead in
// the query's plane (mask_of[q]; 0xFFFFFFFF: none; planes = [nmasks][W] words over the n local rows) --, order the rest in LDS,
// write it back with its count.  Flagged queries (overflow[q]) keep nothing.
template <bool MASKED>
__device__ __forceinline__ void range_keep_body(Cand* __restrict__ cand, const uint32_t* __restrict__ cnt, uint32_t cap, const float* __restrict__ radius,
                                                const uint32_t* __restrict__ overflow, uint32_t* __restrict__ kept,
                                                const uint32_t* __restrict__ mask_of, const uint32_t* __restrict__ planes, uint32_t W, uint32_t n) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  Cand* e = reinterpret_cast<Cand*>(smem_raw);
  __shared__ uint32_t s_wave[4];
  const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t m = cnt[q];
  if (m > cap) m = cap;
  if (overflow[q] != 0u) m = 0;
  const float r = radius[q];
  [[maybe_unused]] uint32_t mq = 0xFFFFFFFFu;
  [[maybe_unused]] const uint32_t* plane = nullptr;
  if constexpr (MASKED) {
    mq = mask_of[q];
    plane = planes + static_cast<uint64_t>(mq == 0xFFFFFFFFu ? 0u : mq) * W;
  }
  Cand* mine = cand + static_cast<uint64_t>(q) * cap;
  // compaction into LDS: a ballot per wave, the waves' totals through LDS, no atomics
  uint32_t keep = 0;                                                 // uniform: entries in LDS so far
  for (uint32_t base = 0; base < m; base += 256) {
    const uint32_t i = base + tid;
    Cand c = Cand{0.f, 0u};
    if (i < m) c = mine[i];
    bool pass = i < m && c.score >= r;
    if constexpr (MASKED)
      if (pass && mq != 0xFFFFFFFFu) pass = c.row < n && ((plane[c.row >> 5] >> (c.row & 31u)) & 1u) != 0u;
    const unsigned long long bal = __ballot(pass);
    if (lane == 0) s_wave[wave] = static_cast<uint32_t>(__builtin_popcountll(bal));
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) { const uint32_t v = s_wave[w]; before += w < wave ? v : 0u; total += v; }
    if (pass) e[keep + before + static_cast<uint32_t>(__builtin_popcountll(bal & ((1ull << lane) - 1ull)))] = c;
    keep += total;
    __syncthreads();
  }
  if (tid == 0) kept[q] = keep;
  if (keep == 0) return;
  uint32_t K2 = 1;
  while (K2 < keep) K2 <<= 1;
  for (uint32_t i = keep + tid; i < K2; i += 256) e[i] = Cand{NEG_INF, 0xFFFFFFFFu};    // behind every kept entry (their scores reach a finite radius)
  __syncthreads();
  for (uint32_t size = 2; size <= K2; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t i = tid; i < (K2 >> 1); i += 256) {
        const uint32_t a = 2 * i - (i & (stride - 1)), b = a + stride;
        const bool desc = ((a & size) == 0);
        const Cand ea = e[a], eb = e[b];
        if (better(eb.score, eb.row, ea.score, ea.row) == desc) { e[a] = eb; e[b] = ea; }
      }
      __syncthreads();
    }
  for (uint32_t i = tid; i < keep; i += 256) mine[i] = e[i];
}

// grid = nq, block = 256, dynamic LDS = (cap rounded up to a power of two) * 8 bytes.  The list holds exact scores (the
// rescore launch ran).  The masked search's twin is range_keep_masked_kernel (kernels_range_parts.h).
static __global__ __launch_bounds__(256) void range_keep_kernel(Cand* __restrict__ cand, const uint32_t* __restrict__ cnt, uint32_t cap,
                                                                const float* __restrict__ radius, const uint32_t* __restrict__ overflow,
                                                                uint32_t* __restrict__ kept) {
  range_keep_body<false>(cand, cnt, cap, radius, overflow, kept, nullptr, nullptr, 0u, 0u);
}

// grid = (ceil(max count / 512), nq), block = 256: two entries per thread, 16-byte accesses (slabs and, for even offsets,
// the packed ids are 16-byte aligned; an odd offset shifts the pairs by one entry).
static __global__ __launch_bounds__(256) void range_pack_kernel(const Cand* __restrict__ cand, uint32_t cap, const uint32_t* __restrict__ kept,
                                                                const unsigned long long* __restrict__ out_off, uint64_t row_base,
                                                                unsigned long long* __restrict__ out_ids, float* __restrict__ out_scores) {
  const uint32_t q = blockIdx.y;
  const uint32_t m = kept[q];
  const uint32_t j = (blockIdx.x * 256u + threadIdx.x) * 2u;
  if (j >= m) return;
  const Cand* mine = cand + static_cast<uint64_t>(q) * cap;
  const unsigned long long o = out_off[q] + j;
  if (j + 1 < m) {
    const uint4 v = *reinterpret_cast<const uint4*>(mine + j);        // two Cand
    if ((o & 1ull) == 0) {
      *reinterpret_cast<ulonglong2*>(out_ids + o) = ulonglong2{row_base + v.y, row_base + v.w};
      *reinterpret_cast<uint2*>(out_scores + o) = uint2{v.x, v.z};
    } else {
      out_ids[o] = row_base + v.y; out_ids[o + 1] = row_base + v.w;
      out_scores[o] = __builtin_bit_cast(float, v.x); out_scores[o + 1] = __builtin_bit_cast(float, v.z);
    }
  } else {
    const Cand c = mine[j];
    out_ids[o] = row_base + c.row;
    out_scores[o] = c.score;
  }
}

// compact batch of the flagged queries: grid = number of them, block = 256
static __global__ __launch_bounds__(256) void range_gather_kernel(const float* __restrict__ q32, const float* __restrict__ radius, const uint32_t* __restrict__ idx,
                                                                  uint32_t dim, float* __restrict__ out_q, float* __restrict__ out_radius) {
  const uint32_t src = idx[blockIdx.x];
  for (uint32_t i = threadIdx.x; i < dim; i += 256) out_q[static_cast<uint64_t>(blockIdx.x) * dim + i] = q32[static_cast<uint64_t>(src) * dim + i];
  if (threadIdx.x == 0) out_radius[blockIdx.x] = radius[src];
}

// the four scores a lane holds of one 16-byte load that reach the radius, as a 4-bit mask (rows >= n never do)
__device__ __forceinline__ uint32_t range_pass4(const float4 v, uint64_t i, uint32_t n, float r) {
  return (i < n && v.x >= r ? 1u : 0u) | (i + 1 < n && v.y >= r ? 2u : 0u) | (i + 2 < n && v.z >= r ? 4u : 0u) | (i + 3 < n && v.w >= r ? 8u : 0u);
}

// grid = (G, nq), block = 256.  The score rows are 256-byte aligned (ld % 64 == 0): whole 16-byte loads, the last one masked.
static __global__ __launch_bounds__(256) void range_count_kernel(const float* __restrict__ scores, uint64_t ld, uint32_t n, const float* __restrict__ radius,
                                                                 uint32_t* __restrict__ count) {
  const uint32_t q = blockIdx.y;
  const float r = radius[q];
  const float* s = scores + static_cast<uint64_t>(q) * ld;
  uint32_t mine = 0;
  for (uint64_t i = (static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x) * 4u; i < n; i += static_cast<uint64_t>(gridDim.x) * 1024u)
    mine += static_cast<uint32_t>(__builtin_popcount(range_pass4(*reinterpret_cast<const float4*>(s + i), i, n, r)));
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(&count[q], mine);
}

// grid = (G, queries of the pass), block = 256.  A wave appends with ONE atomic per step: ballots give every passing
// score its place behind the slot the atomic returned.  taken[] starts at zero; slots [cnt, K2) become key 0.
static __global__ __launch_bounds__(256) void range_collect_kernel(const float* __restrict__ scores, uint64_t ld, uint32_t n, const float* __restrict__ radius,
                                                                   const RangeDesc* __restrict__ desc, uint32_t* __restrict__ taken,
                                                                   unsigned long long* __restrict__ slab) {
  const RangeDesc d = desc[blockIdx.y];
  const float r = radius[d.q];
  const float* s = scores + static_cast<uint64_t>(d.q) * ld;
  unsigned long long* mine = slab + d.slab_off;
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * 1024u;
  const uint64_t first = static_cast<uint64_t>(blockIdx.x) * 1024u + (threadIdx.x & ~63u) * 4u;   // the wave's first row of a step (uniform)
  for (uint64_t w0 = first; w0 < n; w0 += step) {
    const uint64_t i = w0 + lane * 4u;
    float4 v = float4{0.f, 0.f, 0.f, 0.f};
    if (i < n) v = *reinterpret_cast<const float4*>(s + i);
    const uint32_t pm = range_pass4(v, i, n, r);
    const unsigned long long b0 = __ballot(pm & 1u), b1 = __ballot(pm & 2u), b2 = __ballot(pm & 4u), b3 = __ballot(pm & 8u);
    const uint32_t c0 = static_cast<uint32_t>(__builtin_popcountll(b0)), c1 = static_cast<uint32_t>(__builtin_popcountll(b1)),
                   c2 = static_cast<uint32_t>(__builtin_popcountll(b2)), c3 = static_cast<uint32_t>(__builtin_popcountll(b3));
    const uint32_t total = c0 + c1 + c2 + c3;
    if (total == 0) continue;
    uint32_t slot = 0;
    if (lane == 0) slot = atomicAdd(&taken[blockIdx.y], total);
    slot = readlane_u(slot, 0);
    const uint32_t row = static_cast<uint32_t>(i);
    if (pm & 1u) { const uint32_t p = slot + static_cast<uint32_t>(__builtin_popcountll(b0 & below)); if (p < d.cnt) mine[p] = key64_of(v.x, row); }
    if (pm & 2u) { const uint32_t p = slot + c0 + static_cast<uint32_t>(__builtin_popcountll(b1 & below)); if (p < d.cnt) mine[p] = key64_of(v.y, row + 1); }
    if (pm & 4u) { const uint32_t p = slot + c0 + c1 + static_cast<uint32_t>(__builtin_popcountll(b2 & below)); if (p < d.cnt) mine[p] = key64_of(v.z, row + 2); }
    if (pm & 8u) { const uint32_t p = slot + c0 + c1 + c2 + static_cast<uint32_t>(__builtin_popcountll(b3 & below)); if (p < d.cnt) mine[p] = key64_of(v.w, row + 3); }
  }
  if (blockIdx.x == 0) for (uint32_t j = d.cnt + threadIdx.x; j < d.K2; j += 256) mine[j] = 0ull;
}

// grid = (ceil(max count / 256), queries of the pass), block = 256: as emit_kernel, at the query's place in the packed arrays
static __global__ __launch_bounds__(256) void range_emit_kernel(const unsigned long long* __restrict__ slab, const RangeDesc* __restrict__ desc,
                                                                const float* __restrict__ scores, uint64_t ld, uint32_t n, uint64_t row_base,
                                                                unsigned long long* __restrict__ out_ids, float* __restrict__ out_scores) {
  const RangeDesc d = desc[blockIdx.y];
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= d.cnt) return;
  const uint32_t row = ~static_cast<uint32_t>(slab[d.slab_off + j]);
  out_ids[d.out_off + j] = row_base + row;
  out_scores[d.out_off + j] = scores[static_cast<uint64_t>(d.q) * ld + (row < n ? row : n - 1u)];     // (every key is a row < n: the read stays inside the matrix whatever the slab holds)
}

}  // namespace nvdbhip
