// kernels_pq.h -- gfx950 kernels of the PQ candidate scan (nvdb_hip_pq_build / nvdb_hip_pq_search_* / nvdb_hip_pq_refine_ivf;
// orchestration in nvdb_pq.cpp, shapes in pq_plan.h, DESIGN.md section 4 "PQ candidate scan").
//
// Product quantisation with M sub-quantisers of 256 codewords, one byte each, NON-residual, scored by dot-product ADC:
//   dsub = dim / M; sub-vector m of a row = elements [m dsub, (m + 1) dsub) of the row as an f32 query
//   code[r][m]  = the j that minimises d(j) = sum_t (x[t] - cb[m][j][t])^2 -- fp32, t ascending, one fma per element; compared
//                 with < while j ascends (ties: the lowest j; a NaN or +inf distance never wins: such a row gets code 0)
//   L[q][m][j]  = sum_t q[m dsub + t] * cb[m][j][t] -- fp32, t ascending, one fma per element
//   s(q, r)     = sum_m L[q][m][code[r][m]] -- fp32, m ascending, from 0; a NaN score is no candidate
//
//  * pq_encode_kernel<DT, DMAX> : once per build.  grid = (256-row tiles, M / 4), block = 256: a workgroup takes 256 rows and four
//                                 sub-quantisers.  The 256 codewords of one sub-quantiser sit in LDS at a stride of DMAX floats,
//                                 zero beyond dsub; one lane = one row, its sub-vector in DMAX registers, zero beyond dsub (a
//                                 padded element adds fma(0, 0, d) = d: the sum is that of the dsub elements).  The loop over j
//                                 reads the codeword at a wave-uniform address: a broadcast, no bank conflict.  The four codes
//                                 leave as one dword of the row-major [n][M] array.
//  * pq_lut_kernel              : once per search sub-batch.  grid = (M / 4, queries), block = 256: thread j takes codeword j of
//                                 four sub-quantisers -- a wave reads 64 dsub contiguous floats of the codebook, every line in
//                                 full --, the query's four sub-vectors come from LDS (broadcast).
//  * pq_scan_kernel<G, W16>     : THE hot kernel.  grid = work items of the probe path (PartItem, parts_worklist.h) built with
//                                 groups of at most G queries, block = 8 waves, dynamic LDS = G M KB.  The tables of the item's
//                                 nqg <= G queries are copied into LDS once; then the 8 waves take DIFFERENT 64-row tiles of the
//                                 segment (wave w: tiles w, w + 8, ..) and every wave scores its tile against ALL queries of the
//                                 group -- the per-query state (M KB) is large and shared, the per-row state (M bytes) is tiny
//                                 and private, the reverse of part_walk.  A lane reads its row's codes straight from global
//                                 memory (a wave's 64 rows are 64 M contiguous bytes), in 16-byte pieces (W16: M % 16 == 0) or
//                                 dwords, the next piece and the next tile's first piece in flight while this one is looked
//                                 up; a dword of codes costs four ds_read_b32 per query into acc[NG].  NG = the item's queries
//                                 rounded up to a power of two (a compile-time count: a remainder group of one query does not
//                                 pay for eight).  Sink: the (item, query) slab has one entry per row of the segment (slot cap
//                                 0xFFFFFFFF); the lane writes Cand{score, row} -- a NaN score as {-inf, 0xFFFFFFFF} -- at
//                                 position row - row_lo: 512 contiguous bytes per wave and query, positions ascending with the
//                                 row by construction, no ballot, no atomic, no padding pass.
//  * pq_narrow_ids_kernel       : the select's global ids back to the u32 local rows the refine takes (padding 0xFFFFFFFF).
#pragma once
#include "kernels_exact.h"
#include "parts_worklist.h"
#include "pq_plan.h"

namespace nvdbhip {

constexpr uint32_t PQ_ENC_THREADS = 256;
constexpr uint32_t PQ_SCAN_THREADS = 64 * PART_WAVES;

template <int DT, int DMAX>
__global__ __launch_bounds__(PQ_ENC_THREADS) void pq_encode_kernel(const void* __restrict__ rows, const float* __restrict__ scales, uint64_t n, uint32_t dim,
                                                                   uint32_t M, uint32_t dsub, const float* __restrict__ cb, uint8_t* __restrict__ codes) {
  constexpr uint32_t BPE = (DT == DT_F32) ? 4 : (DT == DT_F16 ? 2 : 1);
  __shared__ __attribute__((aligned(16))) float cw[PQ_KSUB * DMAX];
  const uint32_t tid = threadIdx.x;
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * PQ_ENC_THREADS + tid;
  const bool valid = r < n;
  const char* rowp = static_cast<const char*>(rows) + (valid ? r : 0ull) * dim * BPE;
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
        x[t] = load1<DT>(rowp, m * dsub + t);
        if constexpr (DT == DT_I8) x[t] *= scale;
      }
    }
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

__global__ __launch_bounds__(256) void pq_lut_kernel(const float* __restrict__ q32, uint32_t dim, uint32_t M, uint32_t dsub, const float* __restrict__ cb,
                                                     float* __restrict__ lut) {
  __shared__ __attribute__((aligned(16))) float qs[4 * PQ_DSUB_MAX];
  const uint32_t tid = threadIdx.x, m0 = blockIdx.x * 4u, q = blockIdx.y;
  for (uint32_t e = tid; e < 4u * dsub; e += 256u) qs[e] = q32[static_cast<size_t>(q) * dim + m0 * dsub + e];
  __syncthreads();
#pragma unroll 1
  for (uint32_t mm = 0; mm < 4u; ++mm) {
    const float* __restrict__ c = cb + (static_cast<size_t>(m0 + mm) * PQ_KSUB + tid) * dsub;
    const float* __restrict__ qv = qs + mm * dsub;
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
    lut[(static_cast<size_t>(q) * M + m0 + mm) * PQ_KSUB + tid] = acc;
  }
}

// one dword of a row's codes (sub-quantisers m .. m + 3) against the NG tables in LDS; lutm: table 0's row m, qstride: bytes per query
template <int NG>
__device__ __forceinline__ void pq_lookup4(uint32_t w, const char* lutm, uint32_t qstride, float (&acc)[NG]) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const char* at = lutm + b * (PQ_KSUB * 4) + (((w >> (8 * b)) & 255u) << 2);
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] += *reinterpret_cast<const float*>(at + g * qstride);
  }
}

template <bool W16> struct PqPiece { using T = uint32_t; };
template <> struct PqPiece<true> { using T = uint4; };

// the tile loop of one wave for an item of at most NG queries (its tables are in LDS).  L2 (kernels_pq_l2.h; false: no instruction
// of it): hn[row], half the squared norm of the row's reconstruction, rides with the first piece of the row's codes and leaves the
// score at the sink, one fp32 subtraction
template <int NG, bool W16, bool L2 = false>
__device__ __forceinline__ void pq_scan_tiles(const uint8_t* __restrict__ codes, uint32_t M, const PartItem& it, const uint32_t* __restrict__ dst,
                                              const char* lut, Cand* __restrict__ cand, uint32_t wave, uint32_t lane, const float* __restrict__ hn = nullptr) {
  using Piece = typename PqPiece<W16>::T;
  constexpr uint32_t PB = sizeof(Piece);
  const uint32_t np = M / PB, qstride = M * (PQ_KSUB * 4);
  const uint32_t lo = it.row_lo, hi = it.row_hi, ntiles = (hi - lo + 63u) / 64u;
  uint32_t dbase[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) dbase[g] = static_cast<uint32_t>(g) < it.nqg ? dst[it.doff + g] : 0u;
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
          if constexpr (L2) acc[g] = acc[g] - hrow;                    // z = s - h
          cand[static_cast<uint64_t>(dbase[g]) + (row - lo)] = acc[g] == acc[g] ? Cand{acc[g], row} : Cand{NEG_INF, 0xFFFFFFFFu};
        }
    }
  }
}

// lut: [queries of the sub-batch][M][256] f32; qidx / dst: the work list's (qidx[it.qoff + g]: query g of the item's group inside
// the sub-batch, dst[it.doff + g]: the first entry of its slab, which holds row_hi - row_lo entries)
template <int G, bool W16>
__global__ __launch_bounds__(PQ_SCAN_THREADS) void pq_scan_kernel(const uint8_t* __restrict__ codes, uint32_t M, const PartItem* __restrict__ items,
                                                                  const uint32_t* __restrict__ qidx, const uint32_t* __restrict__ dst,
                                                                  const float* __restrict__ lut, Cand* __restrict__ cand) {
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
  // (a table beyond nqg is read where nqg is no power of two -- whatever the LDS holds, inside the G tables -- and never stored)
  if constexpr (G >= 8) { if (nqg > 4u) { pq_scan_tiles<8, W16>(codes, M, it, dst, pq_lds, cand, wave, lane); return; } }
  if constexpr (G >= 4) { if (nqg > 2u) { pq_scan_tiles<4, W16>(codes, M, it, dst, pq_lds, cand, wave, lane); return; } }
  if constexpr (G >= 2) { if (nqg > 1u) { pq_scan_tiles<2, W16>(codes, M, it, dst, pq_lds, cand, wave, lane); return; } }
  pq_scan_tiles<1, W16>(codes, M, it, dst, pq_lds, cand, wave, lane);
}

// ids: the select's [count] global ids (row_base + local row, padding ~0) -> u32 local rows, padding 0xFFFFFFFF
static __global__ __launch_bounds__(256) void pq_narrow_ids_kernel(const unsigned long long* __restrict__ ids, uint64_t count, uint64_t row_base,
                                                                   uint32_t* __restrict__ out) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  if (i >= count) return;
  const unsigned long long id = ids[i];
  out[i] = id == ~0ull ? 0xFFFFFFFFu : static_cast<uint32_t>(id - row_base);
}

}  // namespace nvdbhip
