// kernels_pq_train.h -- gfx950 kernels of the PQ codebook trainer (nvdb_hip_pq_train; orchestration in nvdb_pq.cpp, constants in
// pq_plan.h, DESIGN.md section 4 "PQ candidate scan", paragraph "Training").  Lloyd's iteration per sub-quantiser with the
// arithmetic fixed in include/nvdb_hip.h: the assignment is pq_encode_kernel's (kernels_pq.h) bit for bit -- the distance loop is
// RESTATED here, the encode kernel is not touched --, the update an fp64 sum in ascending training-row order.  No atomics.
//
//  * pq_train_gather_kernel<DT>   : once per call.  The training rows as f32 queries, X[m][dim] (load1 and, for int8, one
//                                   multiplication by the row's scale: the encode kernel's own conversion).
//  * pq_train_start_kernel        : once per call with a NULL init: codeword j of sub-quantiser mq = sub-vector mq of X[pick[mq][j]].
//  * pq_train_step_kernel<DMAX>   : THE hot kernel, once per iteration.  grid = (chunks of PQ_TRAIN_CHUNK rows, M), block = 256.
//                                   Dynamic LDS: the sub-quantiser's 256 codewords at a stride of DMAX floats, zero beyond dsub (as
//                                   in the encode); the current 256-row tile's sub-vectors TRANSPOSED, xs[t][row] (a lane writes
//                                   its own column: no bank conflict); the tile's 256 code bytes; one fp64 per wave.
//                                   Per 256-row tile of the chunk, two phases that turn the block's roles round:
//                                     1. lane = row.  Sub-vector in DMAX registers, the broadcast loop over j (a wave-uniform LDS
//                                        address per codeword), code and sub-vector to LDS, the winning distance into a fixed
//                                        butterfly over the wave's 64 lanes in fp64.
//                                     2. thread = codeword j.  It walks the tile's codes in row order as dword broadcast reads and,
//                                        for each row whose code is j, adds that row's sub-vector from LDS into acc[DMAX] fp64
//                                        registers and bumps its count.  A row matches exactly one of the 256 threads: the
//                                        divergent add runs once per row in one wave, the other three skip it (execz).
//                                   acc and count live across the chunk's tiles; at the end thread j writes
//                                   partial[chunk][mq][j][0 .. dsub), count[chunk][mq][j], thread 0 the chunk's distance sum (per
//                                   tile ((w0 + w1) + (w2 + w3)), the tiles added in tile order).
//  * pq_train_finish_kernel       : once per iteration.  grid = M, block = 256: thread j adds its codeword's partials and counts in
//                                   chunk order, divides in fp64, rounds once, writes the codeword -- or leaves it (no members, a
//                                   non-finite sum); thread 0 adds the chunks' distance sums in chunk order.
#pragma once
#include "kernels_exact.h"
#include "pq_plan.h"

namespace nvdbhip {

constexpr uint32_t PQ_TRAIN_THREADS = 256;
static_assert(PQ_TRAIN_CHUNK % PQ_TRAIN_THREADS == 0 && PQ_TRAIN_CHUNK <= 4096, "a chunk is whole tiles, at most 4096 rows");

// idx: u32 corpus rows of the training set, or nullptr: rows 0 .. m
template <int DT>
__global__ __launch_bounds__(256) void pq_train_gather_kernel(const void* __restrict__ rows, const float* __restrict__ scales, uint32_t dim,
                                                              const uint32_t* __restrict__ idx, uint64_t m, float* __restrict__ X) {
  constexpr uint32_t BPE = (DT == DT_F32) ? 4 : (DT == DT_F16 ? 2 : 1);
  const uint64_t total = m * dim;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<uint64_t>(gridDim.x) * 256) {
    const uint64_t r = i / dim;
    const uint32_t col = static_cast<uint32_t>(i - r * dim);
    const uint64_t row = idx ? idx[r] : r;
    float x = load1<DT>(static_cast<const char*>(rows) + row * dim * BPE, col);
    if constexpr (DT == DT_I8) x *= scales[row];
    X[i] = x;
  }
}

// pick: [M][256] training rows; cb[mq][j][t] = X[pick[mq][j]][mq dsub + t]
static __global__ __launch_bounds__(256) void pq_train_start_kernel(const float* __restrict__ X, uint32_t dim, uint32_t dsub,
                                                                    const uint32_t* __restrict__ pick, float* __restrict__ cb) {
  const uint32_t mq = blockIdx.x, j = threadIdx.x;
  const float* __restrict__ src = X + static_cast<size_t>(pick[mq * PQ_KSUB + j]) * dim + mq * dsub;
  float* dst = cb + (static_cast<size_t>(mq) * PQ_KSUB + j) * dsub;
  for (uint32_t t = 0; t < dsub; ++t) dst[t] = src[t];
}

// X: [m][dim] f32; cb: [M][256][dsub]; partial: [chunks][M][256][dsub] f64; count: [chunks][M][256]; dist: [chunks][M] f64
template <int DMAX>
__global__ __launch_bounds__(PQ_TRAIN_THREADS) void pq_train_step_kernel(const float* __restrict__ X, uint64_t m, uint32_t dim, uint32_t dsub,
                                                                         const float* __restrict__ cb, double* __restrict__ partial,
                                                                         uint32_t* __restrict__ count, double* __restrict__ dist) {
  extern __shared__ __attribute__((aligned(16))) char pqt_lds[];
  float* cw = reinterpret_cast<float*>(pqt_lds);                       // [256][DMAX]
  float* xs = cw + PQ_KSUB * DMAX;                                     // [DMAX][256]
  double* wsum = reinterpret_cast<double*>(xs + DMAX * PQ_TRAIN_THREADS);   // [4]
  uint32_t* code_w = reinterpret_cast<uint32_t*>(wsum + 4);            // 256 bytes
  uint8_t* code_b = reinterpret_cast<uint8_t*>(code_w);

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t M = gridDim.y, mq = blockIdx.y;
  const uint64_t row_lo = static_cast<uint64_t>(blockIdx.x) * PQ_TRAIN_CHUNK;
  const uint64_t row_hi = row_lo + PQ_TRAIN_CHUNK < m ? row_lo + PQ_TRAIN_CHUNK : m;
  const float* __restrict__ src = cb + static_cast<size_t>(mq) * PQ_KSUB * dsub;
  for (uint32_t e = tid; e < PQ_KSUB * DMAX; e += PQ_TRAIN_THREADS) {
    const uint32_t j = e / DMAX, t = e % DMAX;
    cw[e] = t < dsub ? src[j * dsub + t] : 0.f;
  }
  __syncthreads();

  double acc[DMAX];
#pragma unroll
  for (int t = 0; t < DMAX; ++t) acc[t] = 0.0;
  uint32_t cnt = 0u;
  double dsum = 0.0;                                                   // (thread 0's)
#pragma unroll 1
  for (uint64_t r0 = row_lo; r0 < row_hi; r0 += PQ_TRAIN_THREADS) {
    const uint32_t nv = static_cast<uint32_t>(row_hi - r0 < PQ_TRAIN_THREADS ? row_hi - r0 : PQ_TRAIN_THREADS);
    // ---- phase 1: lane = row
    const bool valid = tid < nv;
    const float* __restrict__ xp = X + (r0 + (valid ? tid : 0u)) * dim + mq * dsub;
    float x[DMAX];
    if (dsub % 4u == 0u) {                                             // (dim = M dsub, M % 4 == 0: every sub-vector starts on 16 bytes)
#pragma unroll
      for (int t = 0; t < DMAX; t += 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid && static_cast<uint32_t>(t) < dsub) v = *reinterpret_cast<const float4*>(xp + t);
        x[t] = v.x; x[t + 1] = v.y; x[t + 2] = v.z; x[t + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int t = 0; t < DMAX; ++t) x[t] = (valid && static_cast<uint32_t>(t) < dsub) ? xp[t] : 0.f;
    }
    // the encode kernel's loop, restated: fp32, t ascending, one fma per element, < while j ascends
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
    if (valid) {
      code_b[tid] = static_cast<uint8_t>(bj);
#pragma unroll
      for (int t = 0; t < DMAX; ++t) xs[t * PQ_TRAIN_THREADS + tid] = x[t];
    }
    // a row no codeword wins (every distance NaN or +inf) has code 0 and adds nothing to the distance sum
    double dw = (valid && best < __builtin_huge_valf()) ? static_cast<double>(best) : 0.0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dw += __shfl_xor(dw, off, 64);
    if (lane == 0u) wsum[wave] = dw;
    __syncthreads();
    // ---- phase 2: thread = codeword
    if (tid == 0u) dsum += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
#pragma unroll 1
    for (uint32_t r4 = 0; r4 < nv; r4 += 4u) {
      const uint32_t w = code_w[r4 >> 2];
#pragma unroll
      for (uint32_t b = 0; b < 4u; ++b) {
        if (r4 + b < nv && ((w >> (8u * b)) & 255u) == tid) {
#pragma unroll
          for (int t = 0; t < DMAX; ++t) acc[t] += static_cast<double>(xs[t * PQ_TRAIN_THREADS + r4 + b]);
          ++cnt;
        }
      }
    }
    __syncthreads();                                                   // (the next tile overwrites codes, sub-vectors and wave sums)
  }
  const size_t slot = (static_cast<size_t>(blockIdx.x) * M + mq) * PQ_KSUB + tid;
  double* out = partial + slot * dsub;
#pragma unroll
  for (int t = 0; t < DMAX; ++t)
    if (static_cast<uint32_t>(t) < dsub) out[t] = acc[t];
  count[slot] = cnt;
  if (tid == 0u) dist[static_cast<size_t>(blockIdx.x) * M + mq] = dsum;
}

// err: this iteration's [M] distance sums.  The chunks' sums of a codeword are left in chunk 0's slot.
static __global__ __launch_bounds__(PQ_TRAIN_THREADS) void pq_train_finish_kernel(double* __restrict__ partial, const uint32_t* __restrict__ count,
                                                                                  const double* __restrict__ dist, uint32_t chunks, uint32_t dsub,
                                                                                  float* __restrict__ cb, double* __restrict__ err) {
  const uint32_t M = gridDim.x, mq = blockIdx.x, j = threadIdx.x;
  const size_t slot0 = static_cast<size_t>(mq) * PQ_KSUB + j, step = static_cast<size_t>(M) * PQ_KSUB;
  uint64_t members = 0;
  for (uint32_t ch = 0; ch < chunks; ++ch) members += count[slot0 + ch * step];
  double* sum = partial + slot0 * dsub;
  bool finite = true;
  for (uint32_t t = 0; t < dsub; ++t) {
    double s = sum[t];
    for (uint32_t ch = 1; ch < chunks; ++ch) s += partial[(slot0 + ch * step) * dsub + t];
    sum[t] = s;
    finite = finite && (s - s == 0.0);
  }
  if (members && finite) {
    float* c = cb + slot0 * dsub;
    for (uint32_t t = 0; t < dsub; ++t) c[t] = static_cast<float>(sum[t] / static_cast<double>(members));
  }
  if (j == 0u) {
    double e = 0.0;
    for (uint32_t ch = 0; ch < chunks; ++ch) e += dist[static_cast<size_t>(ch) * M + mq];
    err[mq] = e;
  }
}

}  // namespace nvdbhip
