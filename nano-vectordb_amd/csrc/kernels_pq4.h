// kernels_pq4.h -- gfx950 kernels of the 4-BIT PQ shadow (nvdb_hip_pq4_build and every PQ call over such a shadow; orchestration
// in nvdb_pq.cpp, shapes in pq_plan.h, DESIGN.md section 4 "PQ candidate scan", paragraph "4-bit codes").
//
// Product quantisation with M sub-quantisers of 16 codewords, two codes to a byte; everything else is kernels_pq.h's arithmetic:
//   code[r][m]  < 16, by pq_encode_kernel's rule (fp32 sum of squared differences, t ascending, one fma per element; < while j
//                 ascends; a NaN or +inf distance never wins, a row without a winner gets 0), of the row, its residual
//                 (kernels_pq_resid.h) or a rotated f32 slab (kernels_pq_rotate.h)
//   byte i of row r = code[r][2 i] | code[r][2 i + 1] << 4; a row is M / 2 bytes, the array [n][M / 2]
//   L[q][m][j]  = sum_t q[m dsub + t] * cb[m][j][t], j < 16 -- fp32, t ascending, one fma per element
//   s(q, r)     = sum_m L[q][m][code[r][m]] -- fp32, m ascending, from 0 (+ the base term, one fp32 addition, residual shadows)
// What these kernels share with kernels_pq.h and kernels_pq_resid.h is RESTATED; pq_base_kernel, pq_rotate_kernel and
// pq_narrow_ids_kernel are used as they are.
//
// WHY 16 codewords: a table row is 16 consecutive dwords.  However the 64 lanes of a wave choose among them they touch at most 16
// distinct addresses in 16 different banks, and equal addresses broadcast: the gather cannot conflict, where pq_scan_kernel's
// (256 entries, 1 KB per row) spends 65 % of its LDS cycles on conflicts.  And one query's tables are 64 M bytes, not M KB: a
// workgroup holds 8 to 32 queries' tables, so a list's codes are re-read that many times less.
//
//  * pq4_encode_kernel<DT, DMAX, RESID> : once per build.  grid = 256-row tiles, block = 256, lane = row.  The workgroup walks
//                                 the row in STEPS of eight sub-quantisers: their 8 x 16 codewords go to LDS (stride DMAX, zero
//                                 beyond dsub; 16 KB at DMAX 32), the lane scores its eight sub-vectors one after the other -- the
//                                 codeword address is wave-uniform: a broadcast -- and leaves ONE dword of packed codes per step.
//                                 With a j loop of 16 the row stream is what the kernel costs, so a lane takes its sub-vector in
//                                 16-byte loads where a sub-vector is whole pieces (dsub == DMAX, rows 16-byte aligned) and
//                                 walks its row front to back across the steps: every 128-byte line is fetched once and its rest
//                                 found in cache by the same lane's next loads.  RESID: the lane's list by pq_list_of, the
//                                 centroid's elements subtracted as the sub-vector is formed.
//  * pq4_lut_kernel             : once per search sub-batch.  grid = (M / 16 rounded up, queries), block = 256: thread e takes
//                                 entry (m, j) = (e / 16, e % 16) -- a wave reads 64 dsub contiguous floats of the codebook --,
//                                 the query's 16 sub-vectors come from LDS.  Writes [q][M][16] f32, query-major: which queries
//                                 share a workgroup is known only per work item, so the scan interleaves as it copies.
//  * pq4_scan_kernel<G, W16, RESID> : THE hot kernel.  pq_scan_kernel's work items (groups of at most G = pq4_group(M) queries),
//                                 slabs and sink; lane = row, the 8 waves on different 64-row tiles.  The item's NG tables (its
//                                 queries rounded up to 1, 2, 4, 8, 16 or 32: a compile-time count chosen per item) sit in LDS
//                                 INTERLEAVED query-minor: entry (m, j) of four queries is one 16-byte slot, the 16 slots of a
//                                 table row 256 contiguous bytes, quads of queries M * 256 bytes apart.  A nibble then costs one
//                                 ds_read_b128 and four adds per quad; groups of one and two queries use dword and 8-byte
//                                 slots.  The adds of one query stay in ascending m.  Codes: 16-byte pieces (W16: M / 2 % 16 ==
//                                 0) or dwords, the next piece and the next tile's first piece in flight.  The NG slab offsets
//                                 and base terms sit behind the tables in LDS and are read at the sink (a broadcast): held in
//                                 scalar registers across the tile loop, 2 x 32 of them spill.
//  * pq4_reconstruct_kernel     : pq_reconstruct_kernel over nibbles.
#pragma once
#include "kernels_pq_resid.h"

namespace nvdbhip {

// the lane's sub-vector of sub-quantiser m (elements e0 = m dsub .. + dsub of its row) as f32, zero beyond dsub; vec: whole
// 16-byte pieces at 16-byte aligned addresses (wave-uniform)
template <int DT, int DMAX>
__device__ __forceinline__ void pq4_load_sub(const char* __restrict__ rowp, uint32_t e0, uint32_t dsub, bool vec, bool valid, float (&x)[DMAX]) {
  constexpr uint32_t BPE = (DT == DT_F32) ? 4 : (DT == DT_F16 ? 2 : 1);
  constexpr int NV = DMAX * BPE / 16;                                  // 16-byte pieces of a full sub-vector
  if constexpr (NV > 0) {
    if (vec) {
      const uint4* __restrict__ p = reinterpret_cast<const uint4*>(rowp + static_cast<size_t>(e0) * BPE);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const uint4 w = valid ? p[v] : uint4{0u, 0u, 0u, 0u};
        const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if constexpr (DT == DT_F32) {
            x[v * 4 + k] = __builtin_bit_cast(float, d[k]);
          } else if constexpr (DT == DT_F16) {
            x[v * 8 + 2 * k] = half_bits_to_float(d[k] & 0xFFFFu);
            x[v * 8 + 2 * k + 1] = half_bits_to_float(d[k] >> 16);
          } else {
#pragma unroll
            for (int b = 0; b < 4; ++b) x[v * 16 + 4 * k + b] = static_cast<float>(static_cast<signed char>((d[k] >> (8 * b)) & 255u));
          }
        }
      }
      return;
    }
  }
#pragma unroll
  for (int t = 0; t < DMAX; ++t) x[t] = (valid && static_cast<uint32_t>(t) < dsub) ? load1<DT>(rowp, e0 + t) : 0.f;
}

// rows / scales / n: the corpus or a slab of rotated f32 rows; codes: [n][M / 2]; off / nparts / cent: RESID only
template <int DT, int DMAX, bool RESID>
__global__ __launch_bounds__(PQ_ENC_THREADS) void pq4_encode_kernel(const void* __restrict__ rows, const float* __restrict__ scales, uint64_t n, uint32_t dim,
                                                                    uint32_t M, uint32_t dsub, const float* __restrict__ cb, const uint32_t* __restrict__ off,
                                                                    uint32_t nparts, const float* __restrict__ cent, uint8_t* __restrict__ codes) {
  constexpr uint32_t BPE = (DT == DT_F32) ? 4 : (DT == DT_F16 ? 2 : 1);
  __shared__ __attribute__((aligned(16))) float cw[PQ4_ENC_SQ * PQ4_KSUB * DMAX];
  const uint32_t tid = threadIdx.x;
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * PQ_ENC_THREADS + tid;
  const bool valid = r < n;
  const char* rowp = static_cast<const char*>(rows) + (valid ? r : 0ull) * dim * BPE;
  const bool vec = dsub == static_cast<uint32_t>(DMAX) && (dim * BPE) % 16u == 0u && reinterpret_cast<uintptr_t>(rows) % 16u == 0u;
  const float* __restrict__ cp = nullptr;
  if constexpr (RESID) cp = cent + static_cast<size_t>(pq_list_of(off, nparts, valid ? static_cast<uint32_t>(r) : 0u)) * dim;
  float scale = 1.f;
  if constexpr (DT == DT_I8) scale = valid ? scales[r] : 0.f;
  uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(codes + (valid ? r : 0ull) * (M / 2u));
#pragma unroll 1
  for (uint32_t m0 = 0; m0 < M; m0 += PQ4_ENC_SQ) {
    const float* __restrict__ src = cb + static_cast<size_t>(m0) * PQ4_KSUB * dsub;
    __syncthreads();                                                   // (the previous step's codewords are read no more)
    for (uint32_t e = tid; e < PQ4_ENC_SQ * PQ4_KSUB * DMAX; e += PQ_ENC_THREADS) {
      const uint32_t mj = e / DMAX, t = e % DMAX;                      // mj: (sub-quantiser of the step, codeword)
      cw[e] = t < dsub ? src[mj * dsub + t] : 0.f;
    }
    __syncthreads();
    uint32_t packed = 0u;
#pragma unroll 1
    for (uint32_t mm = 0; mm < PQ4_ENC_SQ; ++mm) {
      const uint32_t e0 = (m0 + mm) * dsub;
      float x[DMAX];
      pq4_load_sub<DT, DMAX>(rowp, e0, dsub, vec, valid, x);
#pragma unroll
      for (int t = 0; t < DMAX; ++t) {
        if (valid && static_cast<uint32_t>(t) < dsub) {
          if constexpr (DT == DT_I8) x[t] *= scale;
          if constexpr (RESID) x[t] = x[t] - cp[e0 + t];
        }
      }
      // pq_encode_kernel's loop, restated: fp32, t ascending, one fma per element, < while j ascends
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
    }
    if (valid) out[m0 / PQ4_ENC_SQ] = packed;
  }
}

// q32: [queries][dim] f32 (rotated where the shadow is); lut: [queries][M][16] f32
static __global__ __launch_bounds__(256) void pq4_lut_kernel(const float* __restrict__ q32, uint32_t dim, uint32_t M, uint32_t dsub, const float* __restrict__ cb,
                                                             float* __restrict__ lut) {
  __shared__ __attribute__((aligned(16))) float qs[16 * PQ_DSUB_MAX];
  const uint32_t tid = threadIdx.x, m0 = blockIdx.x * 16u, q = blockIdx.y;
  const uint32_t nel = (M - m0 < 16u ? M - m0 : 16u) * dsub;           // the block's sub-vectors, contiguous in the query
  for (uint32_t e = tid; e < nel; e += 256u) qs[e] = q32[static_cast<size_t>(q) * dim + m0 * dsub + e];
  __syncthreads();
  const uint32_t e = blockIdx.x * 256u + tid;                          // (m, j) = (e / 16, e % 16)
  if (e >= M * PQ4_KSUB) return;
  const float* __restrict__ c = cb + static_cast<size_t>(e) * dsub;
  const float* __restrict__ qv = qs + (tid / PQ4_KSUB) * dsub;
  float acc = 0.f;
  if (dsub % 4u == 0u) {
    for (uint32_t t = 0; t < dsub; t += 4u) {
      const float4 v = *reinterpret_cast<const float4*>(c + t);
      acc = __builtin_fmaf(qv[t], v.x, acc);
      acc = __builtin_fmaf(qv[t + 1], v.y, acc);
      acc = __builtin_fmaf(qv[t + 2], v.z, acc);
      acc = __builtin_fmaf(qv[t + 3], v.w, acc);
    }
  } else {
    for (uint32_t t = 0; t < dsub; ++t) acc = __builtin_fmaf(qv[t], c[t], acc);
  }
  lut[static_cast<size_t>(q) * M * PQ4_KSUB + e] = acc;
}

// a slot of the LDS image: entry (m, j) of W = 1, 2 or 4 queries
template <int W> struct Pq4Slot { using T = float; };
template <> struct Pq4Slot<2> { using T = float2; };
template <> struct Pq4Slot<4> { using T = float4; };

// one dword of a row's codes (eight nibbles: sub-quantisers m .. m + 7) against the NG tables of the image; lutm: row m of the
// first slot group, sstride: bytes between slot groups.  Per query the adds run in ascending m.
template <int NG>
__device__ __forceinline__ void pq4_lookup8(uint32_t w, const char* lutm, uint32_t sstride, float (&acc)[NG]) {
  constexpr int W = NG >= 4 ? 4 : NG, NS = NG / W;
  using Slot = typename Pq4Slot<W>::T;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const char* at = lutm + b * (PQ4_KSUB * W * 4) + (((w >> (4 * b)) & 15u) * (W * 4u));
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const Slot v = *reinterpret_cast<const Slot*>(at + s * sstride);
      if constexpr (W == 1) {
        acc[s] += v;
      } else if constexpr (W == 2) {
        acc[2 * s] += v.x; acc[2 * s + 1] += v.y;
      } else {
        acc[4 * s] += v.x; acc[4 * s + 1] += v.y; acc[4 * s + 2] += v.z; acc[4 * s + 3] += v.w;
      }
    }
  }
}

// one work item of at most NG queries: its tables into the image [NG / W][M][16][W] (queries beyond nqg: zeros), behind them the
// queries' slab offsets [NG] u32 and base terms [NG] f32; then the tile loop of pq_scan_tiles over rows of M / 2 bytes (L2 / hn as there)
template <int NG, bool W16, bool RESID, bool L2 = false>
__device__ __forceinline__ void pq4_scan_item(const uint8_t* __restrict__ codes, uint32_t M, const PartItem& it, const uint32_t* __restrict__ qidx,
                                              const uint32_t* __restrict__ dst, const float* __restrict__ base, const float* __restrict__ lut,
                                              char* lds, Cand* __restrict__ cand, uint32_t tid, const float* __restrict__ hn = nullptr) {
  constexpr int W = NG >= 4 ? 4 : NG, NS = NG / W;
  using Slot = typename Pq4Slot<W>::T;
  using Piece = typename PqPiece<W16>::T;
  constexpr uint32_t PB = sizeof(Piece);
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t nent = M * PQ4_KSUB, sstride = nent * (W * 4u);
#pragma unroll 1
  for (int s = 0; s < NS; ++s) {
    const float* src[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const uint32_t g = static_cast<uint32_t>(s * W + w);
      src[w] = g < it.nqg ? lut + static_cast<size_t>(qidx[it.qoff + g]) * nent : nullptr;
    }
    Slot* to = reinterpret_cast<Slot*>(lds + static_cast<size_t>(s) * sstride);
    for (uint32_t e = tid; e < nent; e += PQ_SCAN_THREADS) {
      float v[W];
#pragma unroll
      for (int w = 0; w < W; ++w) v[w] = src[w] ? src[w][e] : 0.f;
      if constexpr (W == 1) to[e] = v[0];
      else if constexpr (W == 2) to[e] = float2{v[0], v[1]};
      else to[e] = float4{v[0], v[1], v[2], v[3]};
    }
  }
  uint32_t* side = reinterpret_cast<uint32_t*>(lds + static_cast<size_t>(NS) * sstride);
  if (tid < static_cast<uint32_t>(NG)) {
    const bool live = tid < it.nqg;
    side[tid] = live ? dst[it.doff + tid] : 0u;
    float b = 0.f;
    if constexpr (RESID) b = live ? base[it.qoff + tid] : 0.f;
    reinterpret_cast<float*>(side)[NG + tid] = b;
  }
  __syncthreads();

  const uint32_t rb = M / 2u, np = rb / PB;
  const uint32_t lo = it.row_lo, hi = it.row_hi, ntiles = (hi - lo + 63u) / 64u;
  auto load = [&](uint32_t row, uint32_t p) { return *reinterpret_cast<const Piece*>(codes + static_cast<uint64_t>(row) * rb + p * PB); };
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
      const char* lutm = lds + p * (2u * PB * PQ4_KSUB * W * 4u);       // a piece holds 2 PB sub-quantisers
      if constexpr (W16) {
        pq4_lookup8<NG>(pc.x, lutm, sstride, acc);
        pq4_lookup8<NG>(pc.y, lutm + 8 * (PQ4_KSUB * W * 4), sstride, acc);
        pq4_lookup8<NG>(pc.z, lutm + 16 * (PQ4_KSUB * W * 4), sstride, acc);
        pq4_lookup8<NG>(pc.w, lutm + 24 * (PQ4_KSUB * W * 4), sstride, acc);
      } else {
        pq4_lookup8<NG>(pc, lutm, sstride, acc);
      }
    }
    uint32_t opaque = 0u;
    asm volatile("" : "+v"(opaque));                                   // (per tile: keeps the reads below inside the loop, out of 2 NG registers)
    const uint32_t* sd = side + opaque;
    if (valid) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
        if (static_cast<uint32_t>(g) < it.nqg) {
          float sc = acc[g];
          if constexpr (RESID) sc = reinterpret_cast<const float*>(sd)[NG + g] + acc[g];   // (the one addition the residual form adds)
          if constexpr (L2) sc = sc - hrow;                                                 // z = s - h
          cand[static_cast<uint64_t>(sd[g]) + (row - lo)] = sc == sc ? Cand{sc, row} : Cand{NEG_INF, 0xFFFFFFFFu};
        }
    }
  }
}

// codes: [n][M / 2]; lut: [queries of the sub-batch][M][16] f32; items / qidx / dst / cand as pq_scan_kernel; base: RESID only,
// [pairs of the work list] f32 (pq_base_kernel); dynamic LDS: pq4_scan_lds(M, G)
template <int G, bool W16, bool RESID>
__global__ __launch_bounds__(PQ_SCAN_THREADS) void pq4_scan_kernel(const uint8_t* __restrict__ codes, uint32_t M, const PartItem* __restrict__ items,
                                                                   const uint32_t* __restrict__ qidx, const uint32_t* __restrict__ dst,
                                                                   const float* __restrict__ base, const float* __restrict__ lut, Cand* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) char pq4_lds[];
  PartItem it = items[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  const uint32_t nqg = it.nqg < static_cast<uint32_t>(G) ? it.nqg : static_cast<uint32_t>(G);   // (the host built groups of at most G)
  it.nqg = nqg;
  if constexpr (G >= 32) { if (nqg > 16u) { pq4_scan_item<32, W16, RESID>(codes, M, it, qidx, dst, base, lut, pq4_lds, cand, tid); return; } }
  if constexpr (G >= 16) { if (nqg > 8u) { pq4_scan_item<16, W16, RESID>(codes, M, it, qidx, dst, base, lut, pq4_lds, cand, tid); return; } }
  if (nqg > 4u) { pq4_scan_item<8, W16, RESID>(codes, M, it, qidx, dst, base, lut, pq4_lds, cand, tid); return; }
  if (nqg > 2u) { pq4_scan_item<4, W16, RESID>(codes, M, it, qidx, dst, base, lut, pq4_lds, cand, tid); return; }
  if (nqg > 1u) { pq4_scan_item<2, W16, RESID>(codes, M, it, qidx, dst, base, lut, pq4_lds, cand, tid); return; }
  pq4_scan_item<1, W16, RESID>(codes, M, it, qidx, dst, base, lut, pq4_lds, cand, tid);
}

// pq_reconstruct_kernel over nibbles: cb is [M][16][dsub]
static __global__ __launch_bounds__(256) void pq4_reconstruct_kernel(const uint8_t* __restrict__ codes, uint32_t M, uint32_t dsub, const float* __restrict__ cb,
                                                                     const uint32_t* __restrict__ off, uint32_t nparts, const float* __restrict__ cent,
                                                                     uint32_t row0, uint32_t nrows, float* __restrict__ y) {
  const uint32_t lane = threadIdx.x & 63u, dim = M * dsub;
  for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < nrows; i += gridDim.x * 4u) {
    const uint32_t row = row0 + i;
    const float* __restrict__ cp = cent ? cent + static_cast<size_t>(pq_list_of(off, nparts, row)) * dim : nullptr;
    const uint8_t* __restrict__ code = codes + static_cast<uint64_t>(row) * (M / 2u);
    for (uint32_t t = lane; t < dim; t += 64u) {
      const uint32_t m = t / dsub, j = (code[m >> 1] >> (4u * (m & 1u))) & 15u;
      const float w = cb[(static_cast<size_t>(m) * PQ4_KSUB + j) * dsub + (t - m * dsub)];
      y[static_cast<size_t>(i) * dim + t] = cp ? cp[t] + w : w;
    }
  }
}

}  // namespace nvdbhip
