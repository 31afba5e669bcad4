// kernels_pq4_train.h -- gfx950 kernels of the 16-CODEWORD PQ codebook trainer (nvdb_hip_pq4_train; orchestration in nvdb_pq.cpp,
// sizes in pq_plan.h, DESIGN.md section 4 "PQ candidate scan", paragraphs "Training" and "4-bit codes").  nvdb_hip_pq_train's
// arithmetic with 16 in place of 256: the assignment is pq4_encode_kernel's (kernels_pq4.h) bit for bit -- the distance loop is
// RESTATED here, neither the encode nor the 8-bit trainer's kernels are touched --, the update an fp64 sum in ascending
// training-row order.  No atomics.  The gather, the residual gather and the rotation are the 8-bit trainer's launches.
//
// WHY its own kernel: pq_train_step_kernel is "thread = codeword" over 256 of them and a workgroup per (chunk, sub-quantiser).  With
// 16 codewords that leaves 240 of 256 threads idle in the sum phase, and a lane reads dsub * 4 bytes of its row per workgroup: 32
// bytes of every 128-byte line at dsub 8.
//
//  * pq4_train_start_kernel       : once per call with a NULL init: thread = (sub-quantiser mq, codeword j) over a [M][16] pick;
//                                   codeword j of sub-quantiser mq = sub-vector mq of X[pick[mq][j]].
//  * pq4_train_step_kernel<DMAX>  : THE hot kernel, once per iteration.  grid = (chunks of PQ_TRAIN_CHUNK rows, M / SQ), block = 256.
//                                   A workgroup owns SQ = pq4_train_sq(DMAX) CONSECUTIVE sub-quantisers of its chunk, E = SQ * DMAX
//                                   <= 64 f32 elements of a row: at dsub 8 a lane reads 256 contiguous bytes, two whole lines.
//                                   Dynamic LDS (pq4_train_lds): the fp64 wave sums [4][SQ]; the SQ x 16 codewords at a stride of
//                                   DMAX floats, zero beyond dsub; one dword of packed codes per row of the tile; the tile's
//                                   sub-vectors xs[row][E] at the ODD row stride E + 1.  Per 256-row tile two phases:
//                                     1. lane = row.  Per sub-quantiser of the group: the sub-vector in DMAX registers, the
//                                        broadcast loop over 16 codewords (a wave-uniform LDS address), the nibble into the row's
//                                        dword, the sub-vector to xs (lanes a row apart: E + 1 dwords, odd -> no two lanes of a wave
//                                        in one bank whichever power of two the bank count is), the winning distance into a fixed
//                                        fp64 butterfly over the wave's 64 lanes.
//                                     2. thread = (column e of E, group g of 256 / E codeword groups).  It owns the NA = 16 E / 256
//                                        codewords g NA .. g NA + NA of column e's sub-quantiser: NA fp64 sums in registers (four at
//                                        E = 64, two at E = 32) -- all SQ x 16 x DMAX sums of the workgroup spread over all 256
//                                        threads.  It walks the tile's rows in ascending order: the row's code dword (a broadcast),
//                                        its sub-quantiser's nibble, xs[row][e] (consecutive lanes, consecutive dwords), and into
//                                        each of its NA sums the value or +0.0 (a select, no branch).  A sum that starts at +0.0
//                                        never becomes -0.0, so adding +0.0 leaves its bits: the result is the sequential sum over
//                                        the codeword's members.  The threads of column t == 0 of a sub-vector keep the counts.
//                                   Sums and counts live across the chunk's tiles; at the end the workgroup writes
//                                   partial[chunk][mq][16][dsub], count[chunk][mq][16] and, threads 0 .. SQ, dist[chunk][mq] (per
//                                   tile ((w0 + w1) + (w2 + w3)), the tiles added in tile order).
//  * pq4_train_finish_kernel      : once per iteration.  thread = (sub-quantiser, codeword): adds the codeword's partials and counts
//                                   in chunk order, divides in fp64, rounds once, writes the codeword -- or leaves it (no members, a
//                                   non-finite sum); the thread of codeword 0 adds the chunks' distance sums in chunk order.
#pragma once
#include "kernels_pq_train.h"

namespace nvdbhip {

// pick: [M][16] training rows; cb[mq][j][t] = X[pick[mq][j]][mq dsub + t]
static __global__ __launch_bounds__(256) void pq4_train_start_kernel(const float* __restrict__ X, uint32_t dim, uint32_t M, uint32_t dsub,
                                                                     const uint32_t* __restrict__ pick, float* __restrict__ cb) {
  const uint32_t slot = blockIdx.x * 256u + threadIdx.x;               // (mq, j) = (slot / 16, slot % 16)
  if (slot >= M * PQ4_KSUB) return;
  const float* __restrict__ src = X + static_cast<size_t>(pick[slot]) * dim + (slot / PQ4_KSUB) * dsub;
  float* dst = cb + static_cast<size_t>(slot) * dsub;
  for (uint32_t t = 0; t < dsub; ++t) dst[t] = src[t];
}

// X: [m][dim] f32; cb: [M][16][dsub]; partial: [chunks][M][16][dsub] f64; count: [chunks][M][16]; dist: [chunks][M] f64
template <int DMAX>
__global__ __launch_bounds__(PQ_TRAIN_THREADS) void pq4_train_step_kernel(const float* __restrict__ X, uint64_t m, uint32_t dim, uint32_t M, uint32_t dsub,
                                                                          const float* __restrict__ cb, double* __restrict__ partial,
                                                                          uint32_t* __restrict__ count, double* __restrict__ dist) {
  constexpr uint32_t SQ = pq4_train_sq(DMAX), E = SQ * DMAX, XS = pq4_train_stride(DMAX);
  constexpr uint32_t NG = PQ_TRAIN_THREADS / E, NA = PQ4_KSUB / NG;    // codeword groups per column, codewords per thread
  static_assert(E <= 64 && PQ_TRAIN_THREADS % E == 0 && PQ4_KSUB % NG == 0 && XS % 2 == 1 && SQ <= 8, "the phase-2 split");
  extern __shared__ __attribute__((aligned(16))) char pq4t_lds[];
  double* wsum = reinterpret_cast<double*>(pq4t_lds);                  // [4][SQ]
  float* cw = reinterpret_cast<float*>(wsum + 4 * SQ);                 // [SQ][16][DMAX]
  uint32_t* code = reinterpret_cast<uint32_t*>(cw + SQ * PQ4_KSUB * DMAX);   // [256]: nibble mm = the row's code under sub-quantiser mq0 + mm
  float* xs = reinterpret_cast<float*>(code + PQ_TRAIN_THREADS);       // [256][XS]

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t mq0 = blockIdx.y * SQ;
  const uint64_t row_lo = static_cast<uint64_t>(blockIdx.x) * PQ_TRAIN_CHUNK;
  const uint64_t row_hi = row_lo + PQ_TRAIN_CHUNK < m ? row_lo + PQ_TRAIN_CHUNK : m;
  const float* __restrict__ src = cb + static_cast<size_t>(mq0) * PQ4_KSUB * dsub;
  for (uint32_t i = tid; i < SQ * PQ4_KSUB * DMAX; i += PQ_TRAIN_THREADS) {
    const uint32_t mj = i / DMAX, t = i % DMAX;                        // mj: (sub-quantiser of the group, codeword)
    cw[i] = t < dsub ? src[mj * dsub + t] : 0.f;
  }
  __syncthreads();

  // phase 2's place: column e2 of the group's elements, codewords j0 .. j0 + NA of sub-quantiser mq0 + e2 / DMAX
  const uint32_t e2 = tid % E, j0 = (tid / E) * NA, shift2 = 4u * (e2 / DMAX);
  double acc[NA];
  uint32_t cnt[NA];
#pragma unroll
  for (uint32_t a = 0; a < NA; ++a) { acc[a] = 0.0; cnt[a] = 0u; }
  double dsum = 0.0;                                                   // (threads 0 .. SQ: one sub-quantiser's each)
#pragma unroll 1
  for (uint64_t r0 = row_lo; r0 < row_hi; r0 += PQ_TRAIN_THREADS) {
    const uint32_t nv = static_cast<uint32_t>(row_hi - r0 < PQ_TRAIN_THREADS ? row_hi - r0 : PQ_TRAIN_THREADS);
    // ---- phase 1: lane = row
    const bool valid = tid < nv;
    const float* __restrict__ xp = X + (r0 + (valid ? tid : 0u)) * dim + mq0 * dsub;
    uint32_t packed = 0u;
#pragma unroll 1
    for (uint32_t mm = 0; mm < SQ; ++mm) {
      // a lane beyond the tile reads row r0's elements and leaves nothing behind: no load hangs on a per-lane condition
      float x[DMAX];
      if (dsub % 4u == 0u) {                                           // (dim = M dsub: every sub-vector starts on 16 bytes)
#pragma unroll
        for (int t = 0; t < DMAX; t += 4) {
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (static_cast<uint32_t>(t) < dsub) v = *reinterpret_cast<const float4*>(xp + mm * dsub + t);
          x[t] = v.x; x[t + 1] = v.y; x[t + 2] = v.z; x[t + 3] = v.w;
        }
      } else {
        // the odd shapes go through the lane's own xs slot, element by element in a rolled loop: DMAX conditions on t < dsub
        // held at once cost more scalar registers than there are
        float* mine = xs + tid * XS + mm * DMAX;
#pragma unroll 1
        for (uint32_t t = 0; t < static_cast<uint32_t>(DMAX); ++t) mine[t] = t < dsub ? xp[mm * dsub + t] : 0.f;
#pragma unroll
        for (int t = 0; t < DMAX; ++t) x[t] = mine[t];
      }
      // pq4_encode_kernel's loop, restated: fp32, t ascending, one fma per element, < while j ascends
      const float* __restrict__ cwm = cw + mm * (PQ4_KSUB * DMAX);
      float best = __builtin_huge_valf();
      uint32_t bj = 0u;
#pragma unroll 4
      for (uint32_t j = 0; j < PQ4_KSUB; ++j) {
        float d = 0.f;
#pragma unroll
        for (int t = 0; t < DMAX; ++t) {
          const float diff = x[t] - cwm[j * DMAX + t];
          d = __builtin_fmaf(diff, diff, d);
        }
        if (d < best) { best = d; bj = j; }
      }
      packed |= bj << (4u * mm);
      if (valid) {
#pragma unroll
        for (int t = 0; t < DMAX; ++t) xs[tid * XS + mm * DMAX + t] = x[t];
      }
      // a row no codeword wins (every distance NaN or +inf) has code 0 and adds nothing to the distance sum
      double dw = (valid && best < __builtin_huge_valf()) ? static_cast<double>(best) : 0.0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) dw += __shfl_xor(dw, off, 64);
      if (lane == 0u) wsum[wave * SQ + mm] = dw;
    }
    if (valid) code[tid] = packed;
    __syncthreads();
    // ---- phase 2: thread = (column, codeword group)
    if (tid < SQ) dsum += (wsum[tid] + wsum[SQ + tid]) + (wsum[2 * SQ + tid] + wsum[3 * SQ + tid]);
#pragma unroll 4
    for (uint32_t r = 0; r < nv; ++r) {
      const uint32_t j = ((code[r] >> shift2) & 15u) - j0;             // (the thread's a where j < NA; wraps high otherwise)
      const double xv = static_cast<double>(xs[r * XS + e2]);
#pragma unroll
      for (uint32_t a = 0; a < NA; ++a) {
        const bool mine = j == a;
        acc[a] += mine ? xv : 0.0;
        cnt[a] += mine ? 1u : 0u;
      }
    }
    __syncthreads();                                                   // (the next tile overwrites codes, sub-vectors and wave sums)
  }
  const uint32_t mq = mq0 + e2 / DMAX, t2 = e2 % DMAX;
  const size_t slot = (static_cast<size_t>(blockIdx.x) * M + mq) * PQ4_KSUB + j0;
#pragma unroll
  for (uint32_t a = 0; a < NA; ++a) {
    if (t2 < dsub) partial[(slot + a) * dsub + t2] = acc[a];
    if (t2 == 0u) count[slot + a] = cnt[a];
  }
  if (tid < SQ) dist[static_cast<size_t>(blockIdx.x) * M + mq0 + tid] = dsum;
}

// err: this iteration's [M] distance sums.  The chunks' sums of a codeword are left in chunk 0's slot.
static __global__ __launch_bounds__(256) void pq4_train_finish_kernel(double* __restrict__ partial, const uint32_t* __restrict__ count,
                                                                      const double* __restrict__ dist, uint32_t chunks, uint32_t M, uint32_t dsub,
                                                                      float* __restrict__ cb, double* __restrict__ err) {
  const size_t slot0 = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x, step = static_cast<size_t>(M) * PQ4_KSUB;   // (mq, j) = (slot0 / 16, slot0 % 16)
  if (slot0 >= step) return;
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
  if (slot0 % PQ4_KSUB == 0u) {
    const uint32_t mq = static_cast<uint32_t>(slot0 / PQ4_KSUB);
    double e = 0.0;
    for (uint32_t ch = 0; ch < chunks; ++ch) e += dist[static_cast<size_t>(ch) * M + mq];
    err[mq] = e;
  }
}

}  // namespace nvdbhip
