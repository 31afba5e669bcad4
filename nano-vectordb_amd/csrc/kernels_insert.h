// kernels_insert.h -- gfx950 kernels of the in-place insertion (nvdb_hip_insert_rows; orchestration in nvdb_insert.cpp, the plan in
// insert_plan.h, DESIGN.md section 4 "Insertion").  New rows join the end of their partition, so old row r of partition p goes to
// r + shift[p]; a row's partition is found by a binary search in the OLD offsets (empty partitions never win it).
//   insert_spread_kernel    one workgroup per 64-row tile of a slab of OLD positions: the tile's rows to their new positions (in the
//                           array itself where the slab plan says sources and destinations do not overlap, else read from the bounce
//                           buffer; on the growth path from the old buffer into the new one).  LaneT is the widest vector the row
//                           length guarantees: 16 / 8 / 4 / 2 / 1 bytes, as compact_move_kernel; the 4-byte build with one lane per row
//                           moves the scale arrays.  All element offsets are 64-bit.
//   insert_scatter_kernel   one workgroup per 64 staged new rows (or their staged shadow rows / scales): row i to position pos[i]
//   insert_planes_kernel    a thread per (new word, plane): 32 new positions map to old positions (their bit) or to "new row = live";
//                           whole words are written, tail bits 0 (the word stride changes, so never in place)
// No kernel reads a byte that the same launch writes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_compact.h"   // CompactLane16 / CompactLane8

namespace nvdbhip {

constexpr uint32_t INSERT_MOVE_THREADS = 256;

// the last p < nparts with off[p] <= pos (insert_plan.h ins_list)
__device__ __forceinline__ uint32_t insert_list(const uint64_t* __restrict__ off, uint32_t nparts, uint64_t pos) {
  uint32_t lo = 0, hi = nparts;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (off[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

// L rows that stand side by side at src (unit offset of the first: src_unit0) go to rows s_dst[0 .. L) of dst; upr = LaneT units per row.
// Unit u = tid, tid + 256, ... of the L * upr units: row j = u / upr, unit w = u % upr, kept by addition; four loads before their stores
template <typename LaneT>
__device__ __forceinline__ void insert_move_rows(const LaneT* src, uint64_t src_unit0, LaneT* dst, const uint64_t* s_dst, uint32_t L, uint32_t upr) {
  const uint32_t tid = threadIdx.x;
  uint32_t j = tid / upr, w = tid % upr;
  const uint32_t qs = INSERT_MOVE_THREADS / upr, rs = INSERT_MOVE_THREADS % upr;
  while (j < L) {
    LaneT v[4];
    uint64_t d[4];
    bool ok[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
      ok[u] = j < L;
      if (ok[u]) {
        v[u] = src[src_unit0 + static_cast<uint64_t>(j) * upr + w];
        d[u] = s_dst[j] * upr + w;
      }
      j += qs; w += rs;
      if (w >= upr) { w -= upr; ++j; }
    }
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) if (ok[u]) dst[d[u]] = v[u];
  }
}

// grid = ceil((s1 - s0) / 64), block = 256.  Old rows [s0, s1); src[0] is old row src_row0 (0: src is the array; s0: the bounce buffer).
// off: the OLD offsets (nparts + 1), shift: per partition
template <typename LaneT>
static __global__ __launch_bounds__(INSERT_MOVE_THREADS) void insert_spread_kernel(const LaneT* src, uint64_t src_row0, LaneT* dst,
                                                                                  const uint64_t* __restrict__ off, const uint64_t* __restrict__ shift,
                                                                                  uint32_t nparts, uint64_t s0, uint64_t s1, uint32_t upr) {
  __shared__ uint64_t s_dst[64];
  const uint64_t r0 = s0 + (static_cast<uint64_t>(blockIdx.x) << 6);
  const uint32_t L = static_cast<uint32_t>(s1 - r0 < 64u ? s1 - r0 : 64u);
  if (threadIdx.x < L) {
    const uint64_t r = r0 + threadIdx.x;
    s_dst[threadIdx.x] = r + shift[insert_list(off, nparts, r)];
  }
  __syncthreads();
  insert_move_rows<LaneT>(src, (r0 - src_row0) * upr, dst, s_dst, L, upr);
}

// grid = ceil(m / 64), block = 256.  staged: m rows side by side; pos[i]: the row of dst that staged row i becomes
template <typename LaneT>
static __global__ __launch_bounds__(INSERT_MOVE_THREADS) void insert_scatter_kernel(const LaneT* __restrict__ staged, LaneT* __restrict__ dst,
                                                                                   const uint32_t* __restrict__ pos, uint64_t m, uint32_t upr) {
  __shared__ uint64_t s_dst[64];
  const uint64_t i0 = static_cast<uint64_t>(blockIdx.x) << 6;
  const uint32_t L = static_cast<uint32_t>(m - i0 < 64u ? m - i0 : 64u);
  if (threadIdx.x < L) s_dst[threadIdx.x] = pos[i0 + threadIdx.x];
  __syncthreads();
  insert_move_rows<LaneT>(staged, i0 * upr, dst, s_dst, L, upr);
}

// grid = (ceil(W2 / 256), nmasks), block = 256.  planes: [nmasks][W] words over the n old rows, fresh: [nmasks][W2] over the n_new new
// ones.  New position j of partition p: the old row off_old[p] + (j - off_new[p]) while that is below off_old[p + 1], else a new row
static __global__ __launch_bounds__(256) void insert_planes_kernel(const uint32_t* __restrict__ planes, uint32_t W, uint32_t* __restrict__ fresh, uint32_t W2,
                                                                   const uint64_t* __restrict__ off_old, const uint64_t* __restrict__ off_new, uint32_t nparts,
                                                                   uint64_t n_new) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= W2) return;
  const uint32_t* __restrict__ plane = planes + static_cast<uint64_t>(blockIdx.y) * W;
  const uint64_t j0 = static_cast<uint64_t>(w) << 5;
  uint32_t p = insert_list(off_new, nparts, j0);
  uint32_t out = 0;
  for (uint32_t b = 0; b < 32u && j0 + b < n_new; ++b) {
    const uint64_t j = j0 + b;
    while (j >= off_new[p + 1]) ++p;               // (j < n_new = off_new[nparts]: p stays below nparts)
    const uint64_t old = off_old[p] + (j - off_new[p]);
    const uint32_t bit = old < off_old[p + 1] ? (plane[old >> 5] >> (old & 31u)) & 1u : 1u;
    out |= bit << b;
  }
  fresh[static_cast<uint64_t>(blockIdx.y) * W2 + w] = out;
}

}  // namespace nvdbhip
