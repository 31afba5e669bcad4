// kernels_pq_rotate.h -- the gfx950 kernel of PQ shadows under a caller's OPQ rotation (nvdb_hip_pq_build_opq / _train_opq /
// _rotated_rows / _rotate, the searches and nvdb_hip_pq_reconstruct over such a shadow; orchestration in nvdb_pq.cpp, tile and
// slab sizes in pq_plan.h, DESIGN.md section 4 "PQ candidate scan", paragraph "OPQ rotations").  The one dense matrix product
// of the PQ path:
//   Y[r][i] = sum_t A[i][t] * e[r][t] -- fp32, t ascending from 0, one fused multiply-add per element, accumulator from 0
// on the fp32 matrix cores.  v_mfma_f32_16x16x4_f32 folds the four products of a K-step into the accumulator one after the
// other by fused multiply-adds (kernels_exact_mfma.h rests on the same fact), so ONE accumulator tile fed K-steps in ascending t
// is that chain bit for bit -- as long as K is never split: not across waves, not across lanes, not across launches.  Hence
// every output element lives in one accumulator register of one lane from t = 0 to t = dim - 1, whatever the tile it falls in.
//
//  * pq_rotate_kernel<DT, RESID> : grid = row tiles x column panels (the panel varies fastest: neighbouring workgroups share
//        their rows in L2, and the matrix -- 2.4 MB at dim 768 -- stays there), block = 8 waves.  A workgroup owns
//        PQ_ROT_TR = 256 rows x PQ_ROT_TC = 128 output columns; wave w owns the 64 x 64 block (w / 2, w % 2) of it: 4 x 4
//        accumulator tiles of 16 x 16, 64 registers, held across ALL K slices.
//        K slices of PQ_ROT_KS = 16 elements of both operands go through LDS, double-buffered: while the waves run the 64
//        MFMAs of slice s out of image s % 2, the loads of slice s + 1 are in flight into registers (raw bytes: the
//        conversion waits until they are stored), and land in image (s + 1) % 2 behind the MFMAs; one barrier per slice.
//        A thread moves groups of four consecutive t -- one K-step --: two of the row tile (8 bytes of fp16, 4 of int8, 16
//        of fp32 each; dim % 4 == 0 keeps every group aligned and wholly inside or outside the row) and one of the matrix
//        panel.  The row tile becomes f32 ONCE, on the way into LDS: fp16 widened, int8 float(x) * scale rounded once;
//        RESID subtracts the centroid of the row's list there (the list found once per thread and row, by
//        kernels_pq_resid.h's search), one fp32 subtraction.
//        LDS image: element (row, t0 + 4 s + kq) sits at row * 20 + kq * 4 + s floats: the lane (row = lane % 16,
//        kq = lane / 16) of an MFMA reads its operand of ALL four K-steps of the slice with one ds_read_b128, 8 reads for
//        64 MFMAs; the row stride of 20 floats spreads the 64 dword stores of a wave over 64 banks.
//        Tails are masked, never another arithmetic: rows beyond nrows, matrix rows (output columns) beyond dim and K
//        beyond dim are ZERO operands -- fma(0, 0, acc) = acc, and an accumulator that started at +0 is never -0 -- and
//        outputs beyond nrows or dim are not stored.  A wave whose whole block lies beyond them skips its MFMAs.
//        A NaN or infinity in a row reaches that row's outputs only, one in a matrix row that column only: an MFMA output
//        (i, j) reads row i of one operand and column j of the other, nothing else.
//        The f32 non-residual build also serves the queries, the trainer's gathered sample and -- with the transposed matrix --
//        reconstruction.
//  * pq_rotate_add_cent_kernel   : reconstruction under a residual rotated shadow: x[r][t] += c[list(r)][t], one fp32 addition.
#pragma once
#include "kernels_exact_mfma.h"
#include "kernels_pq_resid.h"

namespace nvdbhip {

constexpr uint32_t PQ_ROT_THREADS = 512;
constexpr uint32_t PQ_ROT_LD = PQ_ROT_KS + 4;                          // floats between two rows of an LDS image
static_assert(PQ_ROT_KS == 16 && PQ_ROT_TR == 256 && PQ_ROT_TC == 128, "the thread -> group maps below: 4 groups per row and slice, 2 + 1 groups per thread");
static_assert((2 * (PQ_ROT_TR + PQ_ROT_TC) * PQ_ROT_LD) * 4 <= 64 * 1024, "both images of both operands in static LDS");

template <int DT> struct PqRotRaw;                                     // four consecutive elements of a row as loaded
template <> struct PqRotRaw<DT_F16> { using T = uint2; };
template <> struct PqRotRaw<DT_I8> { using T = uint32_t; };
template <> struct PqRotRaw<DT_F32> { using T = float4; };

template <int DT>
__device__ __forceinline__ float4 pq_rot_to_f32(const typename PqRotRaw<DT>::T& r, float scale) {
  if constexpr (DT == DT_F16) {
    return make_float4(half_bits_to_float(r.x & 0xFFFFu), half_bits_to_float(r.x >> 16), half_bits_to_float(r.y & 0xFFFFu), half_bits_to_float(r.y >> 16));
  } else if constexpr (DT == DT_I8) {
    float4 v;
    v.x = static_cast<float>(static_cast<int>(r << 24) >> 24) * scale;
    v.y = static_cast<float>(static_cast<int>(r << 16) >> 24) * scale;
    v.z = static_cast<float>(static_cast<int>(r << 8) >> 24) * scale;
    v.w = static_cast<float>(static_cast<int>(r) >> 24) * scale;
    return v;
  } else {
    return r;
  }
}

// one K-step (t .. t + 3 of one row) into an image: element kq goes to [row][kq][step]
__device__ __forceinline__ void pq_rot_put(float* img, uint32_t row, uint32_t step, const float4& v) {
  float* at = img + row * PQ_ROT_LD + step;
  at[0] = v.x; at[4] = v.y; at[8] = v.z; at[12] = v.w;
}

// rows: the corpus (or any [..][dim] array of DT); the tile's rows are row0 .. row0 + nrows of it, Y: [nrows][dim] f32.
// A: [dim][dim] f32, row i = output column i.  off / nparts / cent: the residual shadow's (RESID only; lists are those of the
// absolute rows row0 + i, which fit 32 bits: nvdb_hip_set_partitions)
template <int DT, bool RESID>
__global__ __launch_bounds__(PQ_ROT_THREADS) void pq_rotate_kernel(const void* __restrict__ rows, const float* __restrict__ scales, uint64_t row0, uint32_t nrows,
                                                                   uint32_t dim, const float* __restrict__ A, const uint32_t* __restrict__ off, uint32_t nparts,
                                                                   const float* __restrict__ cent, float* __restrict__ Y) {
  constexpr uint32_t BPE = (DT == DT_F32) ? 4 : (DT == DT_F16 ? 2 : 1);
  using Raw = typename PqRotRaw<DT>::T;
  __shared__ __attribute__((aligned(16))) float es[2][PQ_ROT_TR * PQ_ROT_LD];
  __shared__ __attribute__((aligned(16))) float as[2][PQ_ROT_TC * PQ_ROT_LD];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, l16 = lane & 15u, kq = lane >> 4;
  const uint32_t npanels = (dim + PQ_ROT_TC - 1) / PQ_ROT_TC;
  const uint32_t r0 = (blockIdx.x / npanels) * PQ_ROT_TR, c0 = (blockIdx.x % npanels) * PQ_ROT_TC;
  const uint32_t nslices = (dim + PQ_ROT_KS - 1) / PQ_ROT_KS;

  // this thread's groups: K-step `step` of tile rows erow and erow + 128, and of panel row erow
  const uint32_t step = tid & 3u, erow = tid >> 2;
  const char* rowp[2];
  const float* centp[2];
  float scale[2];
  bool rvalid[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t lr = r0 + erow + 128u * j;
    rvalid[j] = lr < nrows;
    const uint64_t r = row0 + (rvalid[j] ? lr : 0u);
    rowp[j] = static_cast<const char*>(rows) + r * dim * BPE;
    scale[j] = 1.f;
    if constexpr (DT == DT_I8) scale[j] = rvalid[j] ? scales[r] : 0.f;
    centp[j] = nullptr;
    if constexpr (RESID) centp[j] = cent + static_cast<size_t>(pq_list_of(off, nparts, static_cast<uint32_t>(r))) * dim;
  }
  const bool avalid = c0 + erow < dim;
  const float* __restrict__ ap = A + static_cast<size_t>(avalid ? c0 + erow : 0u) * dim;

  Raw raw[2];
  float4 cen[2], mat;
  auto fetch = [&](uint32_t slice) {                                   // global -> registers; beyond the row, the panel or dim: zeros
    const uint32_t t = slice * PQ_ROT_KS + 4u * step;
    const bool kin = t < dim;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      raw[j] = Raw{};
      cen[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rvalid[j] && kin) {
        raw[j] = *reinterpret_cast<const Raw*>(rowp[j] + static_cast<size_t>(t) * BPE);
        if constexpr (RESID) cen[j] = *reinterpret_cast<const float4*>(centp[j] + t);
      }
    }
    mat = make_float4(0.f, 0.f, 0.f, 0.f);
    if (avalid && kin) mat = *reinterpret_cast<const float4*>(ap + t);
  };
  auto land = [&](uint32_t img) {                                      // registers -> LDS, the row tile converted (and the centroid subtracted) once
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float4 v = pq_rot_to_f32<DT>(raw[j], scale[j]);
      if constexpr (RESID) { v.x -= cen[j].x; v.y -= cen[j].y; v.z -= cen[j].z; v.w -= cen[j].w; }
      pq_rot_put(es[img], erow + 128u * j, step, v);
    }
    pq_rot_put(as[img], erow, step, mat);
  };

  const uint32_t wr = wave >> 1, wc = wave & 1u;                       // this wave's 64 x 64 block of the tile
  const bool live = r0 + wr * 64u < nrows && c0 + wc * 64u < dim;
  floatx4_t acc[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = floatx4_t{0.f, 0.f, 0.f, 0.f};

  fetch(0u);
  land(0u);
  __syncthreads();
#pragma unroll 1
  for (uint32_t slice = 0; slice < nslices; ++slice) {
    const uint32_t img = slice & 1u;
    const bool more = slice + 1u < nslices;
    if (more) fetch(slice + 1u);
    if (live) {
      floatx4_t a[4], b[4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) a[rt] = *reinterpret_cast<const floatx4_t*>(&es[img][(wr * 64u + rt * 16u + l16) * PQ_ROT_LD + kq * 4u]);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) b[ct] = *reinterpret_cast<const floatx4_t*>(&as[img][(wc * 64u + ct * 16u + l16) * PQ_ROT_LD + kq * 4u]);
#pragma unroll
      for (int s = 0; s < 4; ++s)                                      // K-steps in ascending t: the chain order
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][s], b[ct][s], acc[rt][ct], 0, 0, 0);
    }
    if (more) land(img ^ 1u);                                          // (image img ^ 1 was last read before the previous barrier)
    __syncthreads();
  }

  if (!live) return;
  // D: this lane holds rows 4 * kq + v, v = 0 .. 3, of column l16 of every accumulator tile
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const uint32_t r = r0 + wr * 64u + rt * 16u + 4u * kq + v;
      if (r >= nrows) continue;
      float* __restrict__ yp = Y + static_cast<uint64_t>(r) * dim;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const uint32_t col = c0 + wc * 64u + ct * 16u + l16;
        if (col < dim) yp[col] = acc[rt][ct][v];
      }
    }
}

// x: [nrows][dim] f32 of the absolute rows row0 ..; x[i][t] += c[list(row0 + i)][t].  One wave per row, lanes stride over t
static __global__ __launch_bounds__(256) void pq_rotate_add_cent_kernel(float* __restrict__ x, uint32_t row0, uint32_t nrows, uint32_t dim,
                                                                        const uint32_t* __restrict__ off, uint32_t nparts, const float* __restrict__ cent) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < nrows; i += gridDim.x * 4u) {
    const float* __restrict__ cp = cent + static_cast<size_t>(pq_list_of(off, nparts, row0 + i)) * dim;
    float* __restrict__ xp = x + static_cast<size_t>(i) * dim;
    for (uint32_t t = lane; t < dim; t += 64u) xp[t] = cp[t] + xp[t];
  }
}

}  // namespace nvdbhip
