// kernels_pq_l2.h -- gfx950 kernels of the PQ scan under the squared-L2 METRIC (nvdb_hip_pq_set_metric / _pq_norms and every PQ
// search while the metric is 1; orchestration in nvdb_pq.cpp, sizes in pq_plan.h, DESIGN.md section 4 "PQ candidate scan",
// paragraph "L2 metric").  For every kind of shadow |q - xhat_r|^2 = |q|^2 - 2 q.xhat_r + |xhat_r|^2, and q.xhat_r is what the
// dot-product scan already computes, base term included: L2 ADC is that scan plus ONE f32 per row.  The arithmetic, fixed:
//   xhat[r][t]  = the bits nvdb_hip_pq_reconstruct returns for row r
//   n[r]        = sum_t xhat[r][t]^2 -- fp32, t ascending from 0, acc = fma(x, x, acc), the accumulator from 0
//   h[r]        = 0.5f * n[r]
//   z(q, r)     = s(q, r) - h[r], one fp32 subtraction of the dot metric's score bits; a NaN z is no candidate, -inf is one
//   qq[q]       = |q|^2 of the UNROTATED query by the base term's rule (kernels_pq_resid.h): 64 partial sums over t = l, l + 64, ..,
//                 one fma each, from 0; then the six-round butterfly
//   dist(q, r)  = fma(-2, z, qq[q]); padding +inf
//
//  * pq_norms_kernel<BITS, RESID> : once per nvdb_hip_pq_set_metric, shadows WITHOUT a rotation; no slab, no f32 rows in HBM.
//                                 grid = tiles of PQ_NORM_TILE = 1024 rows, block = 256, lane = row, PQ_NORM_ROWS_PER_LANE = 4 rows
//                                 and accumulators per lane (rows tile + j * 256 + tid: a wave's 64 rows are contiguous bytes).
//                                 The workgroup walks ALL sub-quantisers in ascending m -- a row's chain is one chain --; the
//                                 codewords of the current m (4-bit: of eight sub-quantisers at a time) sit in LDS at an odd
//                                 stride of pq_norm_stride(dsub) floats, a lane reads its own codes a dword at a time.  RESID:
//                                 the lane finds its rows' lists once (pq_list_of) and adds the centroid element by
//                                 reconstruct's rule, one fp32 addition; neighbouring lanes mostly share the list.
//  * pq_rownorm_kernel            : rotated shadows.  xhat needs the full transpose product, so nvdb_hip_pq_set_metric runs the
//                                 device part of nvdb_hip_pq_reconstruct slab by slab and this kernel over each f32 slab: a
//                                 workgroup owns 256 rows, columns come in chunks of PQ_ROWNORM_COLS through an LDS tile
//                                 (loads: 128 contiguous bytes per row and half wave), lane = row walks its row in LDS at the odd
//                                 stride PQ_ROWNORM_LD; the chain is t ascending across chunks, padding columns are not walked.
//  * pq_scan_l2_kernel<G, W16, RESID>, pq4_scan_l2_kernel<G, W16, RESID> : the L2 builds of the four scans: the prologues of
//                                 pq_scan_kernel / pq_scan_resid_kernel / pq4_scan_kernel restated, the tile loops THEIRS with the
//                                 L2 flag set (kernels_pq.h): a lane loads h[row] with the first piece of its row's codes -- 256
//                                 contiguous bytes per wave, in flight with the next tile's code prefetch --, holds it across the
//                                 loop over m and files Cand{z, row} (a NaN z as {-inf, 0xFFFFFFFF}).  The dot builds keep
//                                 their names, arguments and code.
//  * pq_qnorm_kernel              : once per sub-batch beside the tables: a wave per query, the butterfly rule.
//  * pq_l2_emit_kernel            : the select's [b][out_k] scores z -> distances, padding -> +inf, on the device before the copy
//                                 back.  Not launched on the fused-refine path.
#pragma once
#include "kernels_pq4.h"

namespace nvdbhip {

// codes: [n][M] (BITS 8) or [n][M / 2] (4); cb: [M][256 or 16][dsub]; off / nparts / cent: RESID only; hn: [n]
template <int BITS, bool RESID>
__global__ __launch_bounds__(PQ_NORM_THREADS) void pq_norms_kernel(const uint8_t* __restrict__ codes, uint32_t n, uint32_t M, uint32_t dsub,
                                                                   const float* __restrict__ cb, const uint32_t* __restrict__ off, uint32_t nparts,
                                                                   const float* __restrict__ cent, float* __restrict__ hn) {
  constexpr uint32_t KSUB = BITS == 4 ? PQ4_KSUB : PQ_KSUB;
  constexpr uint32_t SQ = BITS == 4 ? 8u : 1u;                          // sub-quantisers per staging
  constexpr uint32_t NSQ = 32u / BITS;                                  // sub-quantisers per dword of codes
  constexpr int R = PQ_NORM_ROWS_PER_LANE;
  __shared__ __attribute__((aligned(16))) float cw[SQ * KSUB * (PQ_DSUB_MAX + 1)];
  const uint32_t tid = threadIdx.x, stride = pq_norm_stride(dsub), rb = M * BITS / 8u, dim = M * dsub;
  uint32_t row[R];
  bool valid[R];
  float acc[R];
  const uint8_t* codep[R];
  [[maybe_unused]] const float* cp[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    row[j] = blockIdx.x * PQ_NORM_TILE + static_cast<uint32_t>(j) * PQ_NORM_THREADS + tid;
    valid[j] = row[j] < n;
    acc[j] = 0.f;
    codep[j] = codes + static_cast<uint64_t>(valid[j] ? row[j] : 0u) * rb;
    if constexpr (RESID) cp[j] = cent + static_cast<size_t>(pq_list_of(off, nparts, valid[j] ? row[j] : 0u)) * dim;
  }
#pragma unroll 1
  for (uint32_t m0 = 0; m0 < M; m0 += NSQ) {
    uint32_t w[R];
#pragma unroll
    for (int j = 0; j < R; ++j) w[j] = *reinterpret_cast<const uint32_t*>(codep[j] + m0 * BITS / 8u);
#pragma unroll 1
    for (uint32_t mm = 0; mm < NSQ; ++mm) {
      if (mm % SQ == 0u) {
        const float* __restrict__ src = cb + static_cast<size_t>(m0 + mm) * KSUB * dsub;
        __syncthreads();                                               // (the previous codewords are read no more)
        for (uint32_t e = tid; e < SQ * KSUB * dsub; e += PQ_NORM_THREADS) cw[(e / dsub) * stride + e % dsub] = src[e];
        __syncthreads();
      }
      const uint32_t e0 = (m0 + mm) * dsub;
      const float* c[R];
#pragma unroll
      for (int j = 0; j < R; ++j) c[j] = cw + ((mm % SQ) * KSUB + ((w[j] >> (BITS * mm)) & (KSUB - 1u))) * stride;
      for (uint32_t t = 0; t < dsub; ++t) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
          float x = c[j][t];
          if constexpr (RESID) x = cp[j][e0 + t] + x;
          acc[j] = __builtin_fmaf(x, x, acc[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < R; ++j)
    if (valid[j]) hn[row[j]] = 0.5f * acc[j];
}

// Y: [nrows][dim] f32 (a slab of reconstructed rows); hn: the slab's first entry of h
static __global__ __launch_bounds__(PQ_NORM_THREADS) void pq_rownorm_kernel(const float* __restrict__ Y, uint32_t nrows, uint32_t dim, float* __restrict__ hn) {
  __shared__ __attribute__((aligned(16))) float tile[PQ_NORM_THREADS * PQ_ROWNORM_LD];
  const uint32_t tid = threadIdx.x, r0 = blockIdx.x * PQ_NORM_THREADS;
  float acc = 0.f;
#pragma unroll 1
  for (uint32_t c0 = 0; c0 < dim; c0 += PQ_ROWNORM_COLS) {
    __syncthreads();                                                   // (the previous chunk is read no more)
    for (uint32_t e = tid; e < PQ_NORM_THREADS * PQ_ROWNORM_COLS; e += PQ_NORM_THREADS) {
      const uint32_t lr = e / PQ_ROWNORM_COLS, lc = e % PQ_ROWNORM_COLS;
      tile[lr * PQ_ROWNORM_LD + lc] = (r0 + lr < nrows && c0 + lc < dim) ? Y[static_cast<size_t>(r0 + lr) * dim + c0 + lc] : 0.f;
    }
    __syncthreads();
    const uint32_t w = dim - c0 < PQ_ROWNORM_COLS ? dim - c0 : PQ_ROWNORM_COLS;
    const float* __restrict__ mine = tile + tid * PQ_ROWNORM_LD;
    for (uint32_t t = 0; t < w; ++t) acc = __builtin_fmaf(mine[t], mine[t], acc);
  }
  if (r0 + tid < nrows) hn[r0 + tid] = 0.5f * acc;
}

// pq_scan_kernel's and pq_scan_resid_kernel's arguments (base: RESID only) and hn: [n] f32
template <int G, bool W16, bool RESID>
__global__ __launch_bounds__(PQ_SCAN_THREADS) void pq_scan_l2_kernel(const uint8_t* __restrict__ codes, uint32_t M, const PartItem* __restrict__ items,
                                                                     const uint32_t* __restrict__ qidx, const uint32_t* __restrict__ dst,
                                                                     const float* __restrict__ base, const float* __restrict__ lut,
                                                                     const float* __restrict__ hn, Cand* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) char pq_l2_lds[];
  PartItem it = items[blockIdx.x];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t nqg = it.nqg < static_cast<uint32_t>(G) ? it.nqg : static_cast<uint32_t>(G);   // (the host built groups of at most G)
  it.nqg = nqg;
  const uint32_t n4 = M * (PQ_KSUB / 4u);                              // 16-byte pieces of one query's tables
  for (uint32_t g = 0; g < nqg; ++g) {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(lut + static_cast<size_t>(qidx[it.qoff + g]) * M * PQ_KSUB);
    float4* to = reinterpret_cast<float4*>(pq_l2_lds + static_cast<size_t>(g) * M * (PQ_KSUB * 4));
    for (uint32_t i = tid; i < n4; i += PQ_SCAN_THREADS) to[i] = src[i];
  }
  __syncthreads();
  auto tiles = [&](auto ng) {
    constexpr int NG = decltype(ng)::value;
    if constexpr (RESID) pq_scan_resid_tiles<NG, W16, true>(codes, M, it, dst, base, pq_l2_lds, cand, wave, lane, hn);
    else pq_scan_tiles<NG, W16, true>(codes, M, it, dst, pq_l2_lds, cand, wave, lane, hn);
  };
  if constexpr (G >= 8) { if (nqg > 4u) { tiles(std::integral_constant<int, 8>{}); return; } }
  if constexpr (G >= 4) { if (nqg > 2u) { tiles(std::integral_constant<int, 4>{}); return; } }
  if constexpr (G >= 2) { if (nqg > 1u) { tiles(std::integral_constant<int, 2>{}); return; } }
  tiles(std::integral_constant<int, 1>{});
}

// pq4_scan_kernel's arguments and hn: [n] f32
template <int G, bool W16, bool RESID>
__global__ __launch_bounds__(PQ_SCAN_THREADS) void pq4_scan_l2_kernel(const uint8_t* __restrict__ codes, uint32_t M, const PartItem* __restrict__ items,
                                                                      const uint32_t* __restrict__ qidx, const uint32_t* __restrict__ dst,
                                                                      const float* __restrict__ base, const float* __restrict__ lut,
                                                                      const float* __restrict__ hn, Cand* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) char pq4_l2_lds[];
  PartItem it = items[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  const uint32_t nqg = it.nqg < static_cast<uint32_t>(G) ? it.nqg : static_cast<uint32_t>(G);   // (the host built groups of at most G)
  it.nqg = nqg;
  if constexpr (G >= 32) { if (nqg > 16u) { pq4_scan_item<32, W16, RESID, true>(codes, M, it, qidx, dst, base, lut, pq4_l2_lds, cand, tid, hn); return; } }
  if constexpr (G >= 16) { if (nqg > 8u) { pq4_scan_item<16, W16, RESID, true>(codes, M, it, qidx, dst, base, lut, pq4_l2_lds, cand, tid, hn); return; } }
  if (nqg > 4u) { pq4_scan_item<8, W16, RESID, true>(codes, M, it, qidx, dst, base, lut, pq4_l2_lds, cand, tid, hn); return; }
  if (nqg > 2u) { pq4_scan_item<4, W16, RESID, true>(codes, M, it, qidx, dst, base, lut, pq4_l2_lds, cand, tid, hn); return; }
  if (nqg > 1u) { pq4_scan_item<2, W16, RESID, true>(codes, M, it, qidx, dst, base, lut, pq4_l2_lds, cand, tid, hn); return; }
  pq4_scan_item<1, W16, RESID, true>(codes, M, it, qidx, dst, base, lut, pq4_l2_lds, cand, tid, hn);
}

// q32: the sub-batch's UNROTATED queries [b][dim]; qq: [b].  Four waves per workgroup, a wave per query
static __global__ __launch_bounds__(256) void pq_qnorm_kernel(const float* __restrict__ q32, uint32_t dim, uint32_t b, float* __restrict__ qq) {
  const uint32_t lane = threadIdx.x & 63u, q = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (q >= b) return;                                                  // (the whole wave)
  const float* __restrict__ qp = q32 + static_cast<size_t>(q) * dim;
  float acc = 0.f;
  for (uint32_t t = lane; t < dim; t += 64u) acc = __builtin_fmaf(qp[t], qp[t], acc);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
  if (lane == 0u) qq[q] = acc;
}

// ids / scores: the select's [b][out_k] device output (padding ~0 / -inf); scores: z -> fma(-2, z, qq[query]), padding -> +inf
static __global__ __launch_bounds__(256) void pq_l2_emit_kernel(const unsigned long long* __restrict__ ids, float* __restrict__ scores, uint64_t count,
                                                                uint32_t out_k, const float* __restrict__ qq) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  if (i >= count) return;
  scores[i] = ids[i] == ~0ull ? __builtin_huge_valf() : __builtin_fmaf(-2.f, scores[i], qq[i / out_k]);
}

}  // namespace nvdbhip
