// kernels_ivf.h -- the kernels behind the IVF-Flat build (nvdb_ivf.cpp): resident rows as f32 queries for the assignment, the
// fp64 member sums of the k-means update, and the permuting copy that puts the corpus into list order.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_exact.h"

namespace nvdbhip {

// elements of one 16-byte load
template <int DT> __host__ __device__ constexpr uint32_t ivf_epv() { return DT == DT_F32 ? 4u : (DT == DT_F16 ? 8u : 16u); }

// "the row as an f32 query": f32 as it is, f16 widened exactly, int8 float(x) * scale rounded once
template <int DT>
__device__ __forceinline__ float ivf_elem(const void* __restrict__ rowp, uint32_t i, float scale) {
  const float x = load1<DT>(rowp, i);
  if constexpr (DT == DT_I8) return __fmul_rn(x, scale);
  else return x;
}

// out[r][0..dim) = row (idx ? idx[r] : row0 + r) as f32, r < count.  VEC: 16-byte loads (dim a multiple of ivf_epv<DT>(), rows
// 16-byte aligned), one load and its float4 stores per thread and step; else one element per thread and step.
template <int DT, bool VEC>
__global__ __launch_bounds__(256) void rows_to_f32_kernel(const void* __restrict__ rows, const float* __restrict__ scales, uint32_t dim,
                                                          uint64_t row0, const uint32_t* __restrict__ idx, uint32_t count,
                                                          float* __restrict__ out) {
  constexpr uint32_t E = VEC ? ivf_epv<DT>() : 1u;
  const uint32_t vpr = dim / E;
  const size_t total = static_cast<size_t>(count) * vpr;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<size_t>(gridDim.x) * 256) {
    const size_t r = i / vpr;
    const uint32_t v = static_cast<uint32_t>(i - r * vpr);
    const uint64_t row = idx ? idx[r] : row0 + r;
    const void* rp = row_ptr<DT>(rows, row, dim);
    float scale = 1.f;
    if constexpr (DT == DT_I8) scale = scales[row];
    float* o = out + r * dim + static_cast<size_t>(v) * E;
    if constexpr (!VEC) {
      o[0] = ivf_elem<DT>(rp, v, scale);
    } else {
      const uint4 w = static_cast<const uint4*>(rp)[v];
      const uint32_t u[4] = {w.x, w.y, w.z, w.w};
      float f[E];
      if constexpr (DT == DT_F32) {
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = __builtin_bit_cast(float, u[j]);
      } else if constexpr (DT == DT_F16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { f[2 * j] = half_bits_to_float(u[j] & 0xFFFFu); f[2 * j + 1] = half_bits_to_float(u[j] >> 16); }
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) f[j] = __fmul_rn(static_cast<float>(static_cast<signed char>((u[j >> 2] >> (8 * (j & 3))) & 0xFFu)), scale);
      }
#pragma unroll
      for (uint32_t j = 0; j < E; j += 4) *reinterpret_cast<float4*>(o + j) = make_float4(f[j], f[j + 1], f[j + 2], f[j + 3]);
    }
  }
}

// the flat search's u64 ids of the best centroid, narrowed; an id that names no centroid (padding after a non-finite row) -> 0
static __global__ __launch_bounds__(256) void narrow_ids_kernel(const unsigned long long* __restrict__ ids, uint32_t count, uint32_t nparts,
                                                                uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < count) out[i] = ids[i] < nparts ? static_cast<uint32_t>(ids[i]) : 0u;
}

// ------------------------------------------------------------------------------------------------
// k-means update.  members: the training rows in list order (by centroid, ascending row inside one); a centroid's list is cut
// into chunks of at most IVF_SUM_CHUNK_ROWS rows (chunks[c] = {first, end} positions in members).  One workgroup per chunk sums
// its rows per column in fp64, in list order, into partial[c][dim]; centroid_finish_kernel adds a centroid's chunks in chunk
// order.  No atomics anywhere: the same input gives the same bits.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t IVF_SUM_CHUNK_ROWS = 512;

// VEC: four consecutive columns per thread (dim a multiple of 4, rows 16-byte aligned): 16 / 8 / 4-byte loads for f32 / f16 / int8
template <int DT, bool VEC>
__global__ __launch_bounds__(256) void centroid_sum_kernel(const void* __restrict__ rows, const float* __restrict__ scales, uint32_t dim,
                                                           const uint32_t* __restrict__ members, const uint2* __restrict__ chunks,
                                                           double* __restrict__ partial) {
  constexpr uint32_t W = VEC ? 4u : 1u;
  const uint2 ch = chunks[blockIdx.x];
  double* out = partial + static_cast<size_t>(blockIdx.x) * dim;
  for (uint32_t c0 = threadIdx.x * W; c0 < dim; c0 += 256 * W) {
    double acc[W];
#pragma unroll
    for (uint32_t j = 0; j < W; ++j) acc[j] = 0.0;
#pragma unroll 4
    for (uint32_t m = ch.x; m < ch.y; ++m) {
      const uint32_t row = members[m];
      const void* rp = row_ptr<DT>(rows, row, dim);
      float scale = 1.f;
      if constexpr (DT == DT_I8) scale = scales[row];
      if constexpr (!VEC) {
        acc[0] += static_cast<double>(ivf_elem<DT>(rp, c0, scale));
      } else if constexpr (DT == DT_F32) {
        const float4 x = *reinterpret_cast<const float4*>(static_cast<const float*>(rp) + c0);
        acc[0] += static_cast<double>(x.x); acc[1] += static_cast<double>(x.y); acc[2] += static_cast<double>(x.z); acc[3] += static_cast<double>(x.w);
      } else if constexpr (DT == DT_F16) {
        const uint2 x = *reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(rp) + c0);
        acc[0] += static_cast<double>(half_bits_to_float(x.x & 0xFFFFu)); acc[1] += static_cast<double>(half_bits_to_float(x.x >> 16));
        acc[2] += static_cast<double>(half_bits_to_float(x.y & 0xFFFFu)); acc[3] += static_cast<double>(half_bits_to_float(x.y >> 16));
      } else {
        const uint32_t x = *reinterpret_cast<const uint32_t*>(static_cast<const signed char*>(rp) + c0);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += static_cast<double>(__fmul_rn(static_cast<float>(static_cast<signed char>((x >> (8 * j)) & 0xFFu)), scale));
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < W; ++j) out[c0 + j] = acc[j];
  }
}

// One workgroup per centroid p: sum = its chunks [chunk_first[p], chunk_first[p + 1]) added in chunk order (left in the first
// chunk's slot), norm = sqrt(sum of squares) in fp64 (per thread in column order, then a fixed tree over the 256 threads),
// cen[p] = sum / norm rounded once to f32.  No members, or a zero or non-finite norm: cen[p] stays as it is.
static __global__ __launch_bounds__(256) void centroid_finish_kernel(double* __restrict__ partial, const uint32_t* __restrict__ chunk_first, uint32_t dim,
                                                                     float* __restrict__ cen) {
  __shared__ double red[256];
  const uint32_t p = blockIdx.x, c_lo = chunk_first[p], c_hi = chunk_first[p + 1];
  double* sum = partial + static_cast<size_t>(c_lo) * dim;
  double ss = 0.0;
  if (c_hi > c_lo) {
    for (uint32_t c = threadIdx.x; c < dim; c += 256) {
      double s = sum[c];
      for (uint32_t ch = c_lo + 1; ch < c_hi; ++ch) s += partial[static_cast<size_t>(ch) * dim + c];
      sum[c] = s;
      ss += s * s;
    }
  }
  red[threadIdx.x] = ss;
  __syncthreads();
  for (uint32_t w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const double norm = sqrt(red[0]);
  if (!(c_hi > c_lo) || !(norm > 0.0) || !(norm < 1.0e300)) return;
  for (uint32_t c = threadIdx.x; c < dim; c += 256) cen[static_cast<size_t>(p) * dim + c] = static_cast<float>(sum[c] / norm);
}

// ------------------------------------------------------------------------------------------------
// dst row j = src row perm[j], j < n (and the int8 scales with them).  LaneT = uint4 where row_bytes is a multiple of 16 and both
// buffers are 16-byte aligned, unsigned char elsewhere; lpr = lanes per row.  A workgroup takes IVF_GATHER_ROWS destination rows
// per step, four per wave: 64 consecutive lanes of a row per load and store, no index arithmetic beyond the row bases.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t IVF_GATHER_ROWS = 16;

template <typename LaneT>
__global__ __launch_bounds__(256) void gather_rows_kernel(const LaneT* __restrict__ src, const float* __restrict__ src_scales,
                                                          const uint32_t* __restrict__ perm, uint64_t n, uint32_t lpr,
                                                          LaneT* __restrict__ dst, float* __restrict__ dst_scales) {
  const uint64_t groups = (n + IVF_GATHER_ROWS - 1) / IVF_GATHER_ROWS;
  for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const uint64_t j0 = g * IVF_GATHER_ROWS;
    const uint32_t nr = static_cast<uint32_t>(n - j0 < IVF_GATHER_ROWS ? n - j0 : IVF_GATHER_ROWS);
    // wave w copies rows w, w + 4, w + 8, w + 12 of the group side by side: four loads in flight per lane, wave-uniform row bases
    const LaneT* s[4];
    LaneT* d[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
      const uint32_t r = (threadIdx.x >> 6) + 4 * u;
      const bool have = r < nr;
      s[u] = src + static_cast<uint64_t>(perm[j0 + (have ? r : 0u)]) * lpr;
      d[u] = have ? dst + (j0 + r) * lpr : nullptr;
    }
    for (uint32_t l = threadIdx.x & 63u; l < lpr; l += 64) {
      LaneT v[4];
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) if (d[u]) v[u] = s[u][l];
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) if (d[u]) d[u][l] = v[u];
    }
    if (src_scales && threadIdx.x < nr) dst_scales[j0 + threadIdx.x] = src_scales[perm[j0 + threadIdx.x]];
  }
}

}  // namespace nvdbhip
