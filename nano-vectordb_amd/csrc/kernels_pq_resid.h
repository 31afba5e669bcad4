// kernels_pq_resid.h -- gfx950 kernels of the RESIDUAL PQ shadow (nvdb_hip_pq_build_residual / _train_residual / _reconstruct and the
// searches over such a shadow; orchestration in nvdb_pq.cpp, shapes in pq_plan.h, DESIGN.md section 4 "PQ candidate scan",
// paragraph "Residual codes").  A row is quantised as its residual to the centroid of its list, the score gets the centroid's
// share back as one base term per (probed partition, query); the per-query tables stay list-independent (pq_lut_kernel):
//   list(r)     = the p with off[p] <= r < off[p + 1] (an empty partition owns no row)
//   e[r][t]     = x[r][t] - c[list(r)][t] -- one fp32 subtraction of the row as an f32 query and the centroid's bits
//   code[r][m]  = pq_encode_kernel's rule (kernels_pq.h) applied to e
//   b(q, p)     = q . c[p] in fp32: lane l of a wave adds the elements t = l, l + 64, l + 128, .. in that order, one fma each,
//                 from 0; the 64 partial sums then meet in a butterfly, acc += shfl_xor(acc, s) for s = 32, 16, 8, 4, 2, 1
//   s(q, r)     = b(q, list(r)) + sum_m L[q][m][code[r][m]] -- the non-residual sum's bits, then ONE fp32 addition
//   y[r][t]     = c[list(r)][t] + cb[m][code[r][m]][t - m dsub], m = t / dsub (a non-residual shadow: the codeword alone)
// The kernels of kernels_pq.h and kernels_pq_train.h are not touched: what these share with them is RESTATED, so that the existing
// builds keep their code objects.
//
//  * pq_resid_encode_kernel<DT, DMAX> : once per build.  pq_encode_kernel's tile (256 rows x four sub-quantisers), LDS codeword
//                                       image and broadcast loop.  A lane first finds list(r) by an upper-bound search over the
//                                       u32 offsets (12 steps at 4096 lists; neighbouring lanes read the same words) -- per
//                                       LANE: a tile may span any number of lists --, then forms its DMAX residual elements in
//                                       the registers the non-residual build keeps the sub-vector in: the loop over j holds the
//                                       same state, plus the list number across the four sub-quantisers.  No scratch at DMAX 32.
//  * pq_resid_gather_kernel<DT>       : the trainer's gather with the centroid subtracted: X[i][t] = e[row(i)][t].  One wave per
//                                       training row (the list is searched once per row, wave-uniform), lanes stride over t.
//  * pq_base_kernel                   : once per search sub-batch, between the tables and the scan.  grid = partitions, block = 4
//                                       waves.  pstart ([nparts + 1], the work list's counting sort, behind the any-k plan's words
//                                       in the image) says which entries of qidx probe partition p; a workgroup without any leaves
//                                       at once.  The centroid is staged in LDS once; wave w takes the partition's queries w, w + 4,
//                                       ..: lanes stride over t (the query from global memory, coalesced; the centroid from LDS,
//                                       conflict-free), then the butterfly above.  base[i] belongs to qidx[i]: a work item finds
//                                       its queries' terms at base[it.qoff + g].
//  * pq_scan_resid_kernel<G, W16>     : pq_scan_kernel with the item's nqg base terms in registers, added at the sink after the
//                                       loop over m.
//  * pq_reconstruct_kernel            : rows [row0, row0 + nrows) -> y.  One wave per row, lanes stride over t.
#pragma once
#include "kernels_pq.h"

namespace nvdbhip {

constexpr uint32_t PQ_BASE_THREADS = 256;

// list(r): off[0] = 0 <= r < off[nparts] (the caller sees to that).  Invariant: off[lo] <= r < off[hi]
__device__ __forceinline__ uint32_t pq_list_of(const uint32_t* __restrict__ off, uint32_t nparts, uint32_t r) {
  uint32_t lo = 0u, hi = nparts;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// off: [nparts + 1] u32; cent: [nparts][dim] f32; the rest as pq_encode_kernel
template <int DT, int DMAX>
__global__ __launch_bounds__(PQ_ENC_THREADS) void pq_resid_encode_kernel(const void* __restrict__ rows, const float* __restrict__ scales, uint64_t n, uint32_t dim,
                                                                         uint32_t M, uint32_t dsub, const float* __restrict__ cb,
                                                                         const uint32_t* __restrict__ off, uint32_t nparts, const float* __restrict__ cent,
                                                                         uint8_t* __restrict__ codes) {
  constexpr uint32_t BPE = (DT == DT_F32) ? 4 : (DT == DT_F16 ? 2 : 1);
  __shared__ __attribute__((aligned(16))) float cw[PQ_KSUB * DMAX];
  const uint32_t tid = threadIdx.x;
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * PQ_ENC_THREADS + tid;
  const bool valid = r < n;
  const char* rowp = static_cast<const char*>(rows) + (valid ? r : 0ull) * dim * BPE;
  const float* __restrict__ cp = cent + static_cast<size_t>(pq_list_of(off, nparts, valid ? static_cast<uint32_t>(r) : 0u)) * dim;
  float scale = 1.f;
  if constexpr (DT == DT_I8) scale = valid ? scales[r] : 0.f;
  uint32_t packed = 0u;
#pragma unroll 1
  for (uint32_t mm = 0; mm < 4u; ++mm) {
    const uint32_t m = blockIdx.y * 4u + mm;
    const float* __restrict__ src = cb + static_cast<size_t>(m) * PQ_KSUB * dsub;
    __syncthreads();                                                   // (the previous sub-quantiser's codewords are read no more)
    for (uint32_t e = tid; e < PQ_KSUB * DMAX; e += PQ_ENC_THREADS) {
      const uint32_t j = e / DMAX, t = e % DMAX;
      cw[e] = t < dsub ? src[j * dsub + t] : 0.f;
    }
    __syncthreads();
    float x[DMAX];
#pragma unroll
    for (int t = 0; t < DMAX; ++t) {
      x[t] = 0.f;
      if (valid && static_cast<uint32_t>(t) < dsub) {
        float v = load1<DT>(rowp, m * dsub + t);
        if constexpr (DT == DT_I8) v *= scale;
        x[t] = v - cp[m * dsub + t];
      }
    }
    // pq_encode_kernel's loop, restated: fp32, t ascending, one fma per element, < while j ascends
    float best = __builtin_huge_valf();
    uint32_t bj = 0u;
#pragma unroll 2
    for (uint32_t j = 0; j < PQ_KSUB; ++j) {
      float d = 0.f;
#pragma unroll
      for (int t = 0; t < DMAX; ++t) {
        const float diff = x[t] - cw[j * DMAX + t];
        d = __builtin_fmaf(diff, diff, d);
      }
      if (d < best) { best = d; bj = j; }
    }
    packed |= bj << (8u * mm);
  }
  if (valid) *reinterpret_cast<uint32_t*>(codes + r * M + blockIdx.y * 4u) = packed;
}

// idx: u32 corpus rows of the training set, or nullptr: rows 0 .. m; X: [m][dim] f32
template <int DT>
__global__ __launch_bounds__(256) void pq_resid_gather_kernel(const void* __restrict__ rows, const float* __restrict__ scales, uint32_t dim,
                                                              const uint32_t* __restrict__ idx, uint64_t m, const uint32_t* __restrict__ off, uint32_t nparts,
                                                              const float* __restrict__ cent, float* __restrict__ X) {
  constexpr uint32_t BPE = (DT == DT_F32) ? 4 : (DT == DT_F16 ? 2 : 1);
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6); i < m; i += static_cast<uint64_t>(gridDim.x) * 4u) {
    const uint32_t row = idx ? idx[i] : static_cast<uint32_t>(i);
    const char* rowp = static_cast<const char*>(rows) + static_cast<uint64_t>(row) * dim * BPE;
    const float* __restrict__ cp = cent + static_cast<size_t>(pq_list_of(off, nparts, row)) * dim;
    float scale = 1.f;
    if constexpr (DT == DT_I8) scale = scales[row];
    for (uint32_t t = lane; t < dim; t += 64u) {
      float v = load1<DT>(rowp, t);
      if constexpr (DT == DT_I8) v *= scale;
      X[i * dim + t] = v - cp[t];
    }
  }
}

// q32: the sub-batch's queries [b][dim]; pstart: [gridDim.x + 1]; qidx / base: one entry per (probed partition, query) pair
static __global__ __launch_bounds__(PQ_BASE_THREADS) void pq_base_kernel(const float* __restrict__ q32, uint32_t dim, const float* __restrict__ cent,
                                                                         const uint32_t* __restrict__ pstart, const uint32_t* __restrict__ qidx,
                                                                         float* __restrict__ base) {
  __shared__ __attribute__((aligned(16))) float cs[PQ_M_MAX * PQ_DSUB_MAX];       // (dim = M dsub)
  const uint32_t p = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t beg = pstart[p], end = pstart[p + 1];
  if (beg == end) return;                                              // (the whole workgroup: no query probes p)
  for (uint32_t t = tid; t < dim; t += PQ_BASE_THREADS) cs[t] = cent[static_cast<size_t>(p) * dim + t];
  __syncthreads();
  for (uint32_t i = beg + wave; i < end; i += PQ_BASE_THREADS / 64u) {
    const float* __restrict__ q = q32 + static_cast<size_t>(qidx[i]) * dim;
    float acc = 0.f;
    for (uint32_t t = lane; t < dim; t += 64u) acc = __builtin_fmaf(q[t], cs[t], acc);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
    if (lane == 0u) base[i] = acc;
  }
}

// pq_scan_tiles (kernels_pq.h) restated with the base terms: base[it.qoff + g] is b(query g of the group, the item's partition); L2 / hn as there
template <int NG, bool W16, bool L2 = false>
__device__ __forceinline__ void pq_scan_resid_tiles(const uint8_t* __restrict__ codes, uint32_t M, const PartItem& it, const uint32_t* __restrict__ dst,
                                                    const float* __restrict__ base, const char* lut, Cand* __restrict__ cand, uint32_t wave, uint32_t lane,
                                                    const float* __restrict__ hn = nullptr) {
  using Piece = typename PqPiece<W16>::T;
  constexpr uint32_t PB = sizeof(Piece);
  const uint32_t np = M / PB, qstride = M * (PQ_KSUB * 4);
  const uint32_t lo = it.row_lo, hi = it.row_hi, ntiles = (hi - lo + 63u) / 64u;
  uint32_t dbase[NG];
  float bterm[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const bool live = static_cast<uint32_t>(g) < it.nqg;
    dbase[g] = live ? dst[it.doff + g] : 0u;
    bterm[g] = live ? base[it.qoff + g] : 0.f;
  }
  auto load = [&](uint32_t row, uint32_t p) { return *reinterpret_cast<const Piece*>(codes + static_cast<uint64_t>(row) * M + p * PB); };
  Piece nxt{};
  [[maybe_unused]] float hnxt = 0.f;
  if (wave < ntiles && lo + wave * 64u + lane < hi) nxt = load(lo + wave * 64u + lane, 0u);
  if constexpr (L2) { if (wave < ntiles && lo + wave * 64u + lane < hi) hnxt = hn[lo + wave * 64u + lane]; }
  for (uint32_t tile = wave; tile < ntiles; tile += PART_WAVES) {
    const uint32_t row = lo + tile * 64u + lane;
    const bool valid = row < hi;                                       // (a lane beyond the segment looks code 0 up and stores nothing)
    Piece cur = nxt;
    nxt = Piece{};
    [[maybe_unused]] const float hrow = hnxt;
    if (tile + PART_WAVES < ntiles && row + 64u * PART_WAVES < hi) nxt = load(row + 64u * PART_WAVES, 0u);
    if constexpr (L2) { if (tile + PART_WAVES < ntiles && row + 64u * PART_WAVES < hi) hnxt = hn[row + 64u * PART_WAVES]; }
    float acc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = 0.f;
#pragma unroll 1
    for (uint32_t p = 0; p < np; ++p) {
      const Piece pc = cur;
      if (valid && p + 1u < np) cur = load(row, p + 1u);
      const char* lutm = lut + p * (PB * PQ_KSUB * 4);
      if constexpr (W16) {
        pq_lookup4<NG>(pc.x, lutm, qstride, acc);
        pq_lookup4<NG>(pc.y, lutm + 4 * (PQ_KSUB * 4), qstride, acc);
        pq_lookup4<NG>(pc.z, lutm + 8 * (PQ_KSUB * 4), qstride, acc);
        pq_lookup4<NG>(pc.w, lutm + 12 * (PQ_KSUB * 4), qstride, acc);
      } else {
        pq_lookup4<NG>(pc, lutm, qstride, acc);
      }
    }
    if (valid) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
        if (static_cast<uint32_t>(g) < it.nqg) {
          float sc = bterm[g] + acc[g];                                // (the one addition the residual form adds)
          if constexpr (L2) sc = sc - hrow;                            // z = s - h
          cand[static_cast<uint64_t>(dbase[g]) + (row - lo)] = sc == sc ? Cand{sc, row} : Cand{NEG_INF, 0xFFFFFFFFu};
        }
    }
  }
}

// pq_scan_kernel's arguments and base: [pairs of the work list] f32 (pq_base_kernel)
template <int G, bool W16>
__global__ __launch_bounds__(PQ_SCAN_THREADS) void pq_scan_resid_kernel(const uint8_t* __restrict__ codes, uint32_t M, const PartItem* __restrict__ items,
                                                                        const uint32_t* __restrict__ qidx, const uint32_t* __restrict__ dst,
                                                                        const float* __restrict__ base, const float* __restrict__ lut, Cand* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) char pq_lds[];
  PartItem it = items[blockIdx.x];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t nqg = it.nqg < static_cast<uint32_t>(G) ? it.nqg : static_cast<uint32_t>(G);   // (the host built groups of at most G)
  it.nqg = nqg;
  const uint32_t n4 = M * (PQ_KSUB / 4u);                              // 16-byte pieces of one query's tables
  for (uint32_t g = 0; g < nqg; ++g) {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(lut + static_cast<size_t>(qidx[it.qoff + g]) * M * PQ_KSUB);
    float4* to = reinterpret_cast<float4*>(pq_lds + static_cast<size_t>(g) * M * (PQ_KSUB * 4));
    for (uint32_t i = tid; i < n4; i += PQ_SCAN_THREADS) to[i] = src[i];
  }
  __syncthreads();
  if constexpr (G >= 8) { if (nqg > 4u) { pq_scan_resid_tiles<8, W16>(codes, M, it, dst, base, pq_lds, cand, wave, lane); return; } }
  if constexpr (G >= 4) { if (nqg > 2u) { pq_scan_resid_tiles<4, W16>(codes, M, it, dst, base, pq_lds, cand, wave, lane); return; } }
  if constexpr (G >= 2) { if (nqg > 1u) { pq_scan_resid_tiles<2, W16>(codes, M, it, dst, base, pq_lds, cand, wave, lane); return; } }
  pq_scan_resid_tiles<1, W16>(codes, M, it, dst, base, pq_lds, cand, wave, lane);
}

// y: [nrows][dim] f32 of rows row0 ..; off / cent: the residual shadow's (cent == nullptr: a non-residual shadow, the codeword alone)
static __global__ __launch_bounds__(256) void pq_reconstruct_kernel(const uint8_t* __restrict__ codes, uint32_t M, uint32_t dsub, const float* __restrict__ cb,
                                                                    const uint32_t* __restrict__ off, uint32_t nparts, const float* __restrict__ cent,
                                                                    uint32_t row0, uint32_t nrows, float* __restrict__ y) {
  const uint32_t lane = threadIdx.x & 63u, dim = M * dsub;
  for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < nrows; i += gridDim.x * 4u) {
    const uint32_t row = row0 + i;
    const float* __restrict__ cp = cent ? cent + static_cast<size_t>(pq_list_of(off, nparts, row)) * dim : nullptr;
    const uint8_t* __restrict__ code = codes + static_cast<uint64_t>(row) * M;
    for (uint32_t t = lane; t < dim; t += 64u) {
      const uint32_t m = t / dsub;
      const float w = cb[(static_cast<size_t>(m) * PQ_KSUB + code[m]) * dsub + (t - m * dsub)];
      y[static_cast<size_t>(i) * dim + t] = cp ? cp[t] + w : w;
    }
  }
}

}  // namespace nvdbhip
