// kernels_range_parts.h -- gfx950 kernels of the range search on the probe path (nvdb_hip_range_search_partitions / _ivf / _masked;
// orchestration in nvdb_range_parts.cpp, DESIGN.md section 4 "range search" and "row masks").
//
//  * range_parts_kernel    : scan_parts_kernel's work items, tile loop, staging and mask words (kernels_partitions.h) with the
//                            top-k lists taken out.  A range search has no k: a wave that owns its queries only APPENDS.  Per wave
//                            and query the radius, the slab's first entry and the entries written so far sit in scalar registers;
//                            per tile pass = valid && live && score >= radius, a ballot gives every passing lane its place behind
//                            the entries so far, and the lane writes Cand{score, row} there.  An (item, query) slab holds as many
//                            entries as the segment has rows (the host placed it), so nothing can overflow: no atomics, no
//                            counters in memory.  At the end the wave pads the rest of each slab with {-inf, 0xFFFFFFFF}.
//                            Inside a query's block (cbeg[q] .. cbeg[q + 1]) the non-padding entries ascend with the row: the
//                            host lays the slabs out by ascending partition and segment, a wave walks its tiles in order, a
//                            ballot keeps the lane order.  A position inside the block is therefore a valid id tie-break.
//  * rparts_count_kernel   : per query, the non-padding entries of its block.
//  * rparts_collect_kernel : their keys key64_of(score, position inside the block) into the query's slab (padded to a power of
//                            two with key 0); bitonic_lds_kernel / bitonic_global_step_kernel of kernels_largek.h sort the slabs.
//  * rparts_emit_kernel    : from the sorted keys back to the block entry at each position, for the score's original bits
//                            (score_key folds -0.0 into +0.0) and the row; global ids straight into the packed arrays.
//  * range_keep_masked_kernel : range_keep_kernel (kernels_range.h) that also requires the row's bit in the query's plane -- the
//                            keep step of the masked flat range search's filter route.
// Membership is the C comparison score >= radius: a NaN score or a NaN radius never passes, +0.0 == -0.0.
#pragma once
#include "kernels_partitions.h"
#include "kernels_range.h"

namespace nvdbhip {

template <int DT, int QW, bool ALIGNED, bool STAGED, bool MASKED>
__global__ __launch_bounds__(PART_THREADS) void range_parts_kernel(
    const void* __restrict__ rows, const float* __restrict__ scales, uint32_t dim, const PartItem* __restrict__ items,
    const uint32_t* __restrict__ qidx, const uint32_t* __restrict__ dst, const float* __restrict__ q32, const float* __restrict__ radius,
    Cand* __restrict__ cand, PartMask mk) {
  constexpr uint32_t BPE = (DT == DT_F32) ? 4 : (DT == DT_F16 ? 2 : 1);
  constexpr uint32_t QG = PART_WAVES * QW;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const PartItem it = items[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  const int lane = tid & 63;
  const uint32_t wave = tid >> 6;
  const uint32_t qstride = (dim + 3u) & ~3u;
  float* q_lds = reinterpret_cast<float*>(smem_raw);                     // [QG][qstride]
  char* tile = smem_raw + static_cast<size_t>(QG) * qstride * 4;         // STAGED: [64][pitch]

  // gather the group's queries by index; slots beyond the group repeat its first query (scored, never kept)
  for (uint32_t g = 0; g < QG; ++g) {
    const uint32_t qi = qidx[it.qoff + (g < it.nqg ? g : 0u)];
    const float* src = q32 + static_cast<uint64_t>(qi) * dim;
    for (uint32_t j = tid; j < qstride; j += PART_THREADS) q_lds[g * qstride + j] = (j < dim) ? src[j] : 0.f;
  }

  const uint32_t row_bytes = dim * BPE;
  const uint32_t pitch = part_pitch(row_bytes), cpr = row_bytes >> 4;     // (STAGED) 16-byte chunks per row
  const uint32_t r_step = PART_THREADS / (cpr ? cpr : 1u), ch_step = PART_THREADS % (cpr ? cpr : 1u);
  uint4 pre[PART_MAX_CHUNKS];
  // (macros, not lambdas, as in scan_parts_kernel: behind a closure the array stayed in scratch memory)
#define NVDB_RPART_FETCH(T)                                                                                                    \
  {                                                                                                                            \
    const uint32_t nrows_ = (it.row_hi - (T) < PART_TILE_ROWS) ? it.row_hi - (T) : PART_TILE_ROWS;                             \
    const uint32_t nch_ = nrows_ * cpr;                                                                                        \
    const uint4* src_ = reinterpret_cast<const uint4*>(static_cast<const char*>(rows) + static_cast<uint64_t>(T) * row_bytes); \
    _Pragma("unroll") for (uint32_t i_ = 0; i_ < PART_MAX_CHUNKS; ++i_) {                                                      \
      const uint32_t c_ = tid + PART_THREADS * i_;                                                                             \
      pre[i_] = (c_ < nch_) ? src_[c_] : uint4{0u, 0u, 0u, 0u};                                                                \
    }                                                                                                                          \
  }
#define NVDB_RPART_STASH(T)                                                                                                    \
  {                                                                                                                            \
    const uint32_t nrows_ = (it.row_hi - (T) < PART_TILE_ROWS) ? it.row_hi - (T) : PART_TILE_ROWS;                             \
    const uint32_t nch_ = nrows_ * cpr;                                                                                        \
    uint32_t r_ = tid / cpr, ch_ = tid % cpr;                                                                                  \
    _Pragma("unroll") for (uint32_t i_ = 0; i_ < PART_MAX_CHUNKS; ++i_) {                                                      \
      const uint32_t c_ = tid + PART_THREADS * i_;                                                                             \
      if (c_ < nch_) *reinterpret_cast<uint4*>(tile + r_ * pitch + ch_ * 16u) = pre[i_];                                       \
      r_ += r_step; ch_ += ch_step;                                                                                            \
      if (ch_ >= cpr) { ch_ -= cpr; ++r_; }                                                                                    \
    }                                                                                                                          \
  }
  const bool wave_live = wave * QW < it.nqg;                               // this wave owns at least one query of the group
  // this wave's queries, all wave-uniform (scalar registers): radius, first entry of the (item, query) slab, entries written so
  // far, MASKED: mask number.  Slots beyond the group repeat its first query's; nothing is ever written for them.
  float rad[QW];
  uint32_t dbase[QW], ng[QW];
  [[maybe_unused]] uint32_t mid[QW], wcur = 0u;
#pragma unroll
  for (int g = 0; g < QW; ++g) {
    const uint32_t gi = wave * QW + g, gc = gi < it.nqg ? gi : 0u;
    const uint32_t qi = qidx[it.qoff + gc];
    rad[g] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, radius[qi])));
    dbase[g] = __builtin_amdgcn_readfirstlane(dst[it.doff + gc]);
    ng[g] = 0u;
    if constexpr (MASKED) mid[g] = __builtin_amdgcn_readfirstlane(mk.mask_of[qi]);
  }
  if constexpr (MASKED) {
    if (wave_live) wcur = part_mask_words<QW>(mk, mid, it.row_lo, it.row_hi, lane);
  }
  if constexpr (STAGED) { NVDB_RPART_FETCH(it.row_lo) NVDB_RPART_STASH(it.row_lo) }
  __syncthreads();

  const float* qptr = q_lds + wave * QW * qstride;
  const unsigned long long below = (1ull << lane) - 1ull;

  for (uint32_t t_lo = it.row_lo; t_lo < it.row_hi; t_lo += PART_TILE_ROWS) {
    const bool more = t_lo + PART_TILE_ROWS < it.row_hi;
    if constexpr (STAGED) { if (more) NVDB_RPART_FETCH(t_lo + PART_TILE_ROWS) }
    if (wave_live) {
      const uint32_t row = t_lo + lane;
      const bool valid = row < it.row_hi;
      const uint32_t rrow = valid ? row : (it.row_hi - 1);
      [[maybe_unused]] uint32_t wnext = 0u;
      uint32_t live = 0xFFFFFFFFu;                                         // bit g: this lane's row may belong to query g
      if constexpr (MASKED) {
        if (more) wnext = part_mask_words<QW>(mk, mid, t_lo + PART_TILE_ROWS, it.row_hi, lane);   // in flight while this tile is scored
        live = 0u;
        const int j = static_cast<int>((rrow >> 5) - (t_lo >> 5));         // which of the tile's words holds this lane's row: 0 .. 2
#pragma unroll
        for (int g = 0; g < QW; ++g) {
          const uint32_t w = static_cast<uint32_t>(__shfl(static_cast<int>(wcur), 4 * g + j));
          if (valid && wave * QW + g < it.nqg) live |= ((w >> (rrow & 31u)) & 1u) << g;
        }
      }
      if (!MASKED || __any(live != 0u)) {                                  // (uniform over the wave) a tile without a live row: no scores
        const float scale = (DT == DT_I8) ? scales[rrow] : 1.f;
        float sc[QW];
        if constexpr (STAGED) exact_scores<DT, QW, ALIGNED>(tile + static_cast<uint32_t>(lane) * pitch, qptr, qstride, dim, scale, sc);
        else exact_scores<DT, QW, ALIGNED>(row_ptr<DT>(rows, rrow, dim), qptr, qstride, dim, scale, sc);
#pragma unroll
        for (int g = 0; g < QW; ++g) {
          const bool pass = valid && wave * QW + g < it.nqg && ((live >> g) & 1u) && sc[g] >= rad[g];
          const unsigned long long bal = __ballot(pass);
          // every row of the segment is offered once: ng[g] + (passing lanes below) < segment rows = the slab's length
          if (pass) cand[static_cast<uint64_t>(dbase[g]) + ng[g] + static_cast<uint32_t>(__builtin_popcountll(bal & below))] = Cand{sc[g], row};
          ng[g] += static_cast<uint32_t>(__builtin_popcountll(bal));
        }
      }
      if constexpr (MASKED) wcur = wnext;
    }
    if constexpr (STAGED) {
      if (more) {                                                          // (uniform over the workgroup)
        __syncthreads();                                                   // every wave has read this tile
        NVDB_RPART_STASH(t_lo + PART_TILE_ROWS)
        __syncthreads();
      }
    }
  }

  const uint32_t seg = it.row_hi - it.row_lo;                              // entries of this (item, query) slab
#pragma unroll
  for (int g = 0; g < QW; ++g) {
    if (wave * QW + g < it.nqg)
      for (uint32_t j = ng[g] + static_cast<uint32_t>(lane); j < seg; j += 64u) cand[static_cast<uint64_t>(dbase[g]) + j] = Cand{NEG_INF, 0xFFFFFFFFu};
  }
}

#undef NVDB_RPART_FETCH
#undef NVDB_RPART_STASH

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
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  Cand* e = reinterpret_cast<Cand*>(smem_raw);
  __shared__ uint32_t s_wave[4];
  const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t m = cnt[q];
  if (m > cap) m = cap;
  if (overflow[q] != 0u) m = 0;
  const float r = radius[q];
  const uint32_t mq = mask_of[q];
  const uint32_t* plane = planes + static_cast<uint64_t>(mq == 0xFFFFFFFFu ? 0u : mq) * W;
  Cand* mine = cand + static_cast<uint64_t>(q) * cap;
  uint32_t keep = 0;                                                 // uniform: entries in LDS so far
  for (uint32_t base = 0; base < m; base += 256) {
    const uint32_t i = base + tid;
    Cand c = Cand{0.f, 0u};
    if (i < m) c = mine[i];
    bool pass = i < m && c.score >= r;
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
  for (uint32_t i = keep + tid; i < K2; i += 256) e[i] = Cand{NEG_INF, 0xFFFFFFFFu};
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

}  // namespace nvdbhip
