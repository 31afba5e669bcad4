// kernels_range_parts.h -- gfx950 kernels of the range search on the probe path (nvdb_hip_range_search_partitions / _ivf / _masked;
// orchestration in nvdb_range_parts.cpp, DESIGN.md section 4 "range search" and "row masks").
//
//  * range_parts_kernel    : part_walk (kernels_partitions.h: the probe search's work items, tile loop, staging and mask words)
//                            with the append sink (PartAppendSink) in place of the top-k lists.  A range search has no k: a
//                            wave that owns its queries only APPENDS.  Per wave and query the radius, the slab's first entry and
//                            the entries written so far sit in scalar registers; per tile pass = valid && live && score >= radius,
//                            a ballot gives every passing lane its place behind the entries so far, and the lane writes
//                            Cand{score, row} there.  An (item, query) slab holds as many entries as the segment has rows (the
//                            host placed it), so nothing can overflow: no atomics, no counters in memory.  At the end the wave
//                            pads the rest of each slab with {-inf, 0xFFFFFFFF}.
//                            Inside a query's block (cbeg[q] .. cbeg[q + 1]) the non-padding entries ascend with the row: the
//                            host lays the slabs out by ascending partition and segment, a wave walks its tiles in order, a
//                            ballot keeps the lane order.  A position inside the block is therefore a valid id tie-break.
//  * rparts_count_kernel   : per query, the non-padding entries of its block.
//  * rparts_collect_kernel : their keys key64_of(score, position inside the block) into the query's slab (padded to a power of
//                            two with key 0); bitonic_lds_kernel / bitonic_global_step_kernel of kernels_largek.h sort the slabs.
//  * rparts_emit_kernel    : from the sorted keys back to the block entry at each position, for the score's original bits
//                            (score_key folds -0.0 into +0.0) and the row; global ids straight into the packed arrays.
//  * range_keep_masked_kernel : range_keep_kernel (range_keep_body<MASKED>, kernels_range.h) that also requires the row's bit in
//                            the query's plane -- the keep step of the masked flat range search's filter route.
// Membership is the C comparison score >= radius: a NaN score or a NaN radius never passes, +0.0 == -0.0.
#pragma once
#include "kernels_partitions.h"
#include "kernels_range.h"

namespace nvdbhip {

// The append sink of part_walk (kernels_partitions.h).  Per owned query, all wave-uniform (scalar registers): the radius, the
// first entry of the (item, query) slab and the entries written so far.
struct PartAppendSink {
  struct PerQuery { float rad; uint32_t dbase, ng; };
  const uint32_t* __restrict__ dst;
  const float* __restrict__ radius;
  Cand* __restrict__ cand;
  unsigned long long below;                                                // the lanes before this one
  __device__ __forceinline__ void open(PerQuery& p, uint32_t qi, uint32_t dslot) const {
    p.rad = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, radius[qi])));
    p.dbase = __builtin_amdgcn_readfirstlane(dst[dslot]);
    p.ng = 0u;
  }
  __device__ __forceinline__ void row(PerQuery& p, bool pass, float sc, uint32_t row, int) const {
    pass = pass && sc >= p.rad;
    const unsigned long long bal = __ballot(pass);
    // every row of the segment is offered once: ng + (passing lanes below) < segment rows = the slab's length
    if (pass) cand[static_cast<uint64_t>(p.dbase) + p.ng + static_cast<uint32_t>(__builtin_popcountll(bal & below))] = Cand{sc, row};
    p.ng += static_cast<uint32_t>(__builtin_popcountll(bal));
  }
  // the rest of the slab (it holds as many entries as the segment has rows) is padding
  __device__ __forceinline__ void close(const PerQuery& p, uint32_t seg, uint32_t, int lane) const {
    for (uint32_t j = p.ng + static_cast<uint32_t>(lane); j < seg; j += 64u) cand[static_cast<uint64_t>(p.dbase) + j] = Cand{NEG_INF, 0xFFFFFFFFu};
  }
};

template <int DT, int QW, bool ALIGNED, bool STAGED, bool MASKED>
__global__ __launch_bounds__(PART_THREADS) void range_parts_kernel(
    const void* __restrict__ rows, const float* __restrict__ scales, uint32_t dim, const PartItem* __restrict__ items,
    const uint32_t* __restrict__ qidx, const uint32_t* __restrict__ dst, const float* __restrict__ q32, const float* __restrict__ radius,
    Cand* __restrict__ cand, PartMask mk) {
  const PartAppendSink sink{dst, radius, cand, (1ull << (threadIdx.x & 63u)) - 1ull};
  part_walk<DT, QW, ALIGNED, STAGED, MASKED>(rows, scales, dim, items, qidx, q32, mk, sink);
}

// grid = queries of the launch set, block = 256: count[q] = the non-padding entries of cand[cbeg[q] .. cbeg[q + 1])
static __global__ __launch_bounds__(256) void rparts_count_kernel(const Cand* __restrict__ cand, const uint32_t* __restrict__ cbeg, uint32_t* __restrict__ count) {
  __shared__ uint32_t s_wave[4];
  const uint32_t q = blockIdx.x;
  const uint64_t lo = cbeg[q], hi = cbeg[q + 1];
  uint32_t mine = 0;
  for (uint64_t i = lo + threadIdx.x; i < hi; i += 256u) mine += cand[i].row != 0xFFFFFFFFu ? 1u : 0u;
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) count[q] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// grid = (G, queries of the pass), block = 256; desc[].q = the query's number inside the launch set.  As range_collect_kernel:
// a wave appends with one atomic per step.  taken[] starts at zero; slots [cnt, K2) become key 0.
static __global__ __launch_bounds__(256) void rparts_collect_kernel(const Cand* __restrict__ cand, const uint32_t* __restrict__ cbeg,
                                                                    const RangeDesc* __restrict__ desc, uint32_t* __restrict__ taken,
                                                                    unsigned long long* __restrict__ slab) {
  const RangeDesc d = desc[blockIdx.y];
  const uint64_t lo = cbeg[d.q];
  const uint32_t len = cbeg[d.q + 1] - cbeg[d.q];
  unsigned long long* mine = slab + d.slab_off;
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * 256u;
  const uint64_t first = static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u);        // the wave's first position of a step (uniform)
  for (uint64_t w0 = first; w0 < len; w0 += step) {
    const uint64_t i = w0 + lane;
    Cand e = Cand{NEG_INF, 0xFFFFFFFFu};
    if (i < len) e = cand[lo + i];
    const bool pass = e.row != 0xFFFFFFFFu;
    const unsigned long long bal = __ballot(pass);
    const uint32_t total = static_cast<uint32_t>(__builtin_popcountll(bal));
    if (total == 0) continue;
    uint32_t slot = 0;
    if (lane == 0) slot = atomicAdd(&taken[blockIdx.y], total);
    slot = readlane_u(slot, 0);
    if (pass) {
      const uint32_t p = slot + static_cast<uint32_t>(__builtin_popcountll(bal & below));
      if (p < d.cnt) mine[p] = key64_of(e.score, static_cast<uint32_t>(i));
    }
  }
  if (blockIdx.x == 0) for (uint32_t j = d.cnt + threadIdx.x; j < d.K2; j += 256) mine[j] = 0ull;
}

// grid = (ceil(max count / 256), queries of the pass), block = 256
static __global__ __launch_bounds__(256) void rparts_emit_kernel(const unsigned long long* __restrict__ slab, const RangeDesc* __restrict__ desc,
                                                                 const Cand* __restrict__ cand, const uint32_t* __restrict__ cbeg, uint64_t row_base,
                                                                 unsigned long long* __restrict__ out_ids, float* __restrict__ out_scores) {
  const RangeDesc d = desc[blockIdx.y];
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= d.cnt) return;
  const uint32_t len = cbeg[d.q + 1] - cbeg[d.q];                          // (>= cnt >= 1)
  const uint32_t pos = ~static_cast<uint32_t>(slab[d.slab_off + j]);
  const Cand e = cand[static_cast<uint64_t>(cbeg[d.q]) + (pos < len ? pos : len - 1u)];   // (every key is a position < len: the read stays inside the block whatever the slab holds)
  out_ids[d.out_off + j] = row_base + e.row;
  out_scores[d.out_off + j] = e.score;
}

// range_keep_kernel for a masked search: grid = nq, block = 256, dynamic LDS = (cap rounded up to a power of two) * 8 bytes.
// mask_of[q] = the query's plane (0xFFFFFFFF: none), planes = [nmasks][W] words over the LOCAL rows the lists hold.  A dead row
// above the filter's threshold has only occupied a list entry; it is dropped here.
static __global__ __launch_bounds__(256) void range_keep_masked_kernel(Cand* __restrict__ cand, const uint32_t* __restrict__ cnt, uint32_t cap,
                                                                       const float* __restrict__ radius, const uint32_t* __restrict__ overflow,
                                                                       uint32_t* __restrict__ kept, const uint32_t* __restrict__ mask_of,
                                                                       const uint32_t* __restrict__ planes, uint32_t W, uint32_t n) {
  range_keep_body<true>(cand, cnt, cap, radius, overflow, kept, mask_of, planes, W, n);
}

}  // namespace nvdbhip
