// nvdb_launch_f16.cpp -- launch helpers of the fp16 MFMA filter kernels (kernels_filter.h): which build streams which shape, its LDS
// attribute, its rendezvous counters, its survivor logs; the bootstrap build; query prep.
#include "nvdb_ctx.h"

namespace nvdbhip {

nvdb_status launch_prep_q16(nvdb_hip_ctx* c, hipStream_t s, const float* dev_q, uint32_t nq, uint32_t nq_pad, const PrepInit& pinit) {
  // fp32 corpus: the shadow adds 2^-11 relative (normal halves) and <= 2^-25 absolute per element (subnormal halves)
  prep_q16_kernel<<<nq_pad, 256, 0, s>>>(dev_q, nq, c->dim, c->fdim, prep_norm(c, c->max_norm), c->dtype == NVDB_DTYPE_F32 ? FILTER_REL_F16 + 4.9e-4f : FILTER_REL_F16,
                                         c->dtype == NVDB_DTYPE_F32 ? 3.0e-8f * std::sqrt(static_cast<float>(c->dim)) : 0.f, static_cast<uint32_t*>(c->overflow.p),
                                         static_cast<_Float16*>(c->q16.p),
                                         static_cast<float*>(c->qscale.p), static_cast<float*>(c->qinv.p),
                                         static_cast<float*>(c->ebound.p), static_cast<float*>(c->slack.p), pinit);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

// dims up to 768: batches <= 128 on filter_f16_kernel (32x32x16, 32 queries per wave), larger ones on the 16x16x32 build with 64
// queries per wave -- with siblings to keep in step its SYNC build, on 8 waves of 32 queries unless option waves8 = 0
template <int DIM, int NB>
nvdb_status launch_filter_dim(nvdb_hip_ctx* c, FilterRun& run, RowRange rows) {
  constexpr uint32_t TROWS = f16_m16_tile_rows(DIM);     // tile of the m16 build
  constexpr int MBK = TROWS / 16;                         // ... in 16-row blocks
  static_assert(f16_m16_qpb(2, 8) == f16_filter_qpb(DIM, 2) && f16_m16_qpb(4, 4) == f16_filter_qpb(DIM, 2), "m16 builds: queries per workgroup");
  // both builds of a dim are launched with the larger of their two carve-ups (they differ up to d=384)
  constexpr size_t lds = std::max(filter_f16_lds_bytes<DIM>(), filter_f16_m16_lds_bytes<DIM, MBK>());
#ifdef NVDB_HIP_DEV
  const bool m16 = f16_m16_build(c, NB);                 // developer build: option mfma16 = 0 selects the 32x32x16 build for batches > 128 (A/B only)
  constexpr bool HAS_WIDE32 = true;
#else
  const bool m16 = (NB == 2);
  constexpr bool HAS_WIDE32 = (NB == 1);                 // the product instantiates filter_f16_kernel for batches <= 128 (and as the bootstrap build) only
#endif
  const uint32_t nwg = filter_grid(c, run.QT);
  if (!m16) {
    if constexpr (HAS_WIDE32) return launch_filter_f16_kernel(c, run, rows, filter_f16_kernel<DIM, NB>, nwg, FilterGeom{256, lds, 4, true}, &c->hitlog, FILTER_ROWS, 0u);
    return fail(c, NVDB_ERR_INTERNAL, "fp16 filter kernel: no build for this batch");
  }
  nvdb_status st;
  SyncArgs sy;
  if ((st = sibling_sync_args(c, run, nwg, sy))) return st;
  if constexpr (DIM <= 768)
    if (sy.prog && c->opt_waves8)
      return launch_filter_f16_kernel(c, run, rows, filter_f16_m16_kernel<DIM, 4, true, false, MBK, 2, 8>, nwg, FilterGeom{512, lds, 8, true}, &c->hitlog, TROWS,
                                      sy.prog, sy.mask, sy.lead);
  return launch_filter_f16_kernel(c, run, rows, sy.prog ? filter_f16_m16_kernel<DIM, 6, true, false, MBK> : filter_f16_m16_kernel<DIM, 6, false, false, MBK>, nwg,
                                  FilterGeom{256, lds, 4, true}, &c->hitlog, TROWS, sy.prog, sy.mask, sy.lead);
}

// dims 2048 / 2560 / 3072: K-split build, 16-row tiles in two half-K stages, 16 queries per wave, 64 per workgroup
template <int DIM>
nvdb_status launch_filter_k2_dim(nvdb_hip_ctx* c, FilterRun& run, RowRange rows) {
  static_assert(f16_filter_qpb(DIM, 1) == 4 * 16, "K-split build: 4 waves x 16 queries");
  const uint32_t nwg = filter_grid(c, run.QT);
  nvdb_status st;
  SyncArgs sy;
  if ((st = sibling_sync_args(c, run, nwg, sy))) return st;
  return launch_filter_f16_kernel(c, run, rows, sy.prog ? filter_f16_k2_kernel<DIM, true> : filter_f16_k2_kernel<DIM, false>, nwg,
                                  FilterGeom{256, filter_f16_k2_lds_bytes<DIM>(), 4, true}, &c->hitlog, 16, sy.prog, sy.mask, sy.lead);
}

// dims 896 .. 1536: 16-row tiles, 32 queries per wave (MB = 1, NQB = 2), 128 queries per workgroup; with siblings to keep in
// step and a tile's DIM / 32 pieces splitting over 8 waves (DIM % 256 == 0), two waves per SIMD: 8 waves x 16 queries
// (DIM/8 <= 192 registers of fragments per wave) unless option waves8 = 0
template <int DIM>
nvdb_status launch_filter_k_dim(nvdb_hip_ctx* c, FilterRun& run, RowRange rows) {
  constexpr size_t lds = filter_f16_m16_lds_bytes<DIM, 1>();
  static_assert(f16_m16_qpb(1, 8) == f16_filter_qpb(DIM, 1) && f16_m16_qpb(2, 4) == f16_filter_qpb(DIM, 1), "16-row-tile builds: queries per workgroup");
  const uint32_t nwg = filter_grid(c, run.QT);
  nvdb_status st;
  SyncArgs sy;
  if ((st = sibling_sync_args(c, run, nwg, sy))) return st;
  if constexpr (DIM % 256 == 0)
    if (sy.prog && c->opt_waves8)
      return launch_filter_f16_kernel(c, run, rows, filter_f16_m16_kernel<DIM, 4, true, false, 1, 1, 8>, nwg, FilterGeom{512, lds, 8, true}, &c->hitlog, 16, sy.prog,
                                      sy.mask, sy.lead);
  return launch_filter_f16_kernel(c, run, rows, sy.prog ? filter_f16_m16_kernel<DIM, 6, true, false, 1, 2> : filter_f16_m16_kernel<DIM, 6, false, false, 1, 2>, nwg,
                                  FilterGeom{256, lds, 4, true}, &c->hitlog, 16, sy.prog, sy.mask, sy.lead);
}

// threshold bootstrap on the matrix cores (fp16): best (score,row) of every 32-row tile of rows [0,n0) per query
// -> cand[q][tile]; the caller then runs select(mode 2) to turn the k-th largest tile maximum into thr[q].
template <int DIM, int NB>
nvdb_status launch_boot_dim(nvdb_hip_ctx* c, FilterRun& run, RowRange rows) {
  return launch_filter_f16_kernel(c, run, rows, filter_f16_kernel<DIM, NB, true>, filter_grid(c, run.QT), FilterGeom{256, filter_f16_lds_bytes<DIM>(), 0, false}, &c->cand,
                                  FILTER_ROWS, run.cap);
}

nvdb_status launch_boot_f16(nvdb_hip_ctx* c, FilterRun& run, uint32_t n0) {
  const uint32_t nb = filter_nb(c, run.kind, run.nq);
  nvdb_status st;
  if (dispatch_dim(F16Dims{}, c->fdim, st, [&](auto D) { return nb == 1 ? launch_boot_dim<decltype(D)::value, 1>(c, run, {0, n0}) : launch_boot_dim<decltype(D)::value, 2>(c, run, {0, n0}); })) return st;
  return fail(c, NVDB_ERR_UNSUPPORTED, "boot kernel: unsupported dim");
}

nvdb_status launch_filter_f16(nvdb_hip_ctx* c, FilterRun& run, RowRange rows) {
  const uint32_t nb = filter_nb(c, run.kind, run.nq);
  nvdb_status st;
  if (dispatch_dim(F16DimsK2{}, c->fdim, st, [&](auto D) { return launch_filter_k2_dim<decltype(D)::value>(c, run, rows); })) return st;
  if (dispatch_dim(F16Dims16{}, c->fdim, st, [&](auto D) { return launch_filter_k_dim<decltype(D)::value>(c, run, rows); })) return st;
  if (dispatch_dim(F16Dims{}, c->fdim, st, [&](auto D) { return nb == 1 ? launch_filter_dim<decltype(D)::value, 1>(c, run, rows) : launch_filter_dim<decltype(D)::value, 2>(c, run, rows); })) return st;
  return fail(c, NVDB_ERR_UNSUPPORTED, "filter kernel: unsupported dim");
}

}  // namespace nvdbhip
