// nvdb_launch_i8.cpp -- launch helpers of the int8 MFMA filter kernels (kernels_filter.h: two-stage / bootstrap builds;
// kernels_filter_i8s.h: the 16x16x64 logged build); query prep (two int8 planes).
#include "nvdb_ctx.h"
#include "kernels_filter_i8s.h"

namespace nvdbhip {

nvdb_status launch_prep_q8(nvdb_hip_ctx* c, hipStream_t s, const float* dev_q, uint32_t nq, uint32_t nq_pad, const PrepInit& pinit) {
  // (filter_max_norm: row norms of what the int8 kernels stream -- the corpus itself, or the int8 filter shadow of an fp16 / fp32 corpus,
  //  whose quantisation residual resid_max joins the error bound)
  prep_q8_kernel<<<nq_pad, 256, 0, s>>>(dev_q, nq, c->dim, c->fdim, prep_norm(c, c->filter_max_norm), c->q8shadow ? prep_norm(c, c->resid_max) : 0.f, static_cast<signed char*>(c->q16.p),
                                        static_cast<signed char*>(c->q16.p) + static_cast<size_t>(nq_pad) * c->fdim,
                                        static_cast<float*>(c->qscale.p), static_cast<float*>(c->qinv.p),
                                        static_cast<float*>(c->ebound.p), static_cast<float*>(c->slack.p), static_cast<float*>(c->qdelta.p),
                                        static_cast<uint32_t*>(c->overflow.p), static_cast<uint32_t>(c->opt_i8_lo_bits), pinit);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

#ifdef NVDB_HIP_DEV   // the two-plane int8 kernel (option i8_wide = 0): the reference build the two-stage kernels are compared with
template <int DIM>
nvdb_status launch_filter_i8_dim(nvdb_hip_ctx* c, FilterRun& run, RowRange rows) {
  const uint32_t nwg = filter_grid(c, run.QT);
  nvdb_status st;
  SyncArgs sy;
  if ((st = sibling_sync_args(c, run, nwg, sy))) return st;
  return launch_filter_i8_kernel(c, run, rows, run.QT, sy.prog ? filter_i8_kernel<DIM, false, 6, true> : filter_i8_kernel<DIM>, nwg, FilterGeom{256, filter_i8_lds_bytes<DIM>(), 4, true},
                                 static_cast<size_t>(run.nq_pad) * DIM, &c->hitlog, scatter_args(c, run, FILTER_ROWS), 0u, sy.prog, sy.mask, sy.lead);
}
#endif  // NVDB_HIP_DEV

// the builds of the two-stage kernel; SYNC is the last choice made (both instantiations of a build have one type)
template <int DIM, int NB, int MB> auto i8w_build(bool sync) { return sync ? filter_i8w_kernel<DIM, NB, 6, true, MB> : filter_i8w_kernel<DIM, NB, 6, false, MB>; }
template <int DIM, int WPB, bool DEFER> auto i8p_build(bool sync) { return sync ? filter_i8p_kernel<DIM, true, false, 6, WPB, DEFER> : filter_i8p_kernel<DIM, false, false, 6, WPB, DEFER>; }
template <int DIM, int WPB> auto i8s_build(bool sync) { return sync ? filter_i8s_kernel<DIM, true, false, 6, WPB> : filter_i8s_kernel<DIM, false, false, 6, WPB>; }
template <int DIM, int WPB> auto i8c_build(bool sync) { return sync ? shadow_i8c_kernel<DIM, true, 6, WPB> : shadow_i8c_kernel<DIM, false, 6, WPB>; }   // one common scale (shadow_scale_plan.h)

// int8, dims up to 768, 64-row tiles: which build streams which batch.  The product library holds
//   batches <= 128 (NB = 1)  filter_i8w_kernel at 32 queries per wave; d = 512 / 768 and more than 8 queries (d = 384: more than 64): the
//                            16x16x64 logged build on 8 (d = 384: 4) waves, waves without queries only load
//   batches > 128 (NB = 2)   d >= 384: the 16x16x64 logged build (filter_i8s_kernel), at d = 768 on 8 waves of 32 queries (option i8_dense8;
//                            d = 384 / 512 / 640 on 4 of 64); d = 256: the 32x32x32 logged build (filter_i8p_kernel)
//   option i8_defer, signed / huge row scales: the pipelined build with the in-loop second stage (filter_i8p_kernel, DEFER)
// and the developer library every build at every batch (options i8_pipe, i8_waves8, i8_mfma16, i8_small8).
template <int DIM, int NB>
nvdb_status launch_filter_i8w_dim(nvdb_hip_ctx* c, FilterRun& run, RowRange rows) {
  constexpr uint32_t TROWS = i8w_tile_rows(DIM);
  static_assert(TROWS == I8W_TILE_ROWS, "the builds of dims <= 768 stream two 32-row blocks per tile");
  if ((rows.hi - rows.lo) % TROWS) return fail(c, NVDB_ERR_INTERNAL, "int8 two-stage kernel: row range is not a multiple of its 64-row tile");
  const bool pipe = i8_pipelined(c, run.kind, NB);       // (developer build: i8_pipe = 0 runs filter_i8w_kernel at 64 queries per wave, i8_waves8 = 1 the 8-wave pipelined build)
  const bool defer = i8_stage2_in_loop(c), logs = i8_logs_survivors(c, run.kind, NB);
#ifdef NVDB_HIP_DEV
  const bool w8 = pipe && c->opt_i8_waves8 && DIM != 384;
  constexpr bool HAS_I8W = true, HAS_I8P32 = true, DEV_I8S8_512 = true;
#else
  constexpr bool DEV_I8S8_512 = false;
  constexpr bool w8 = false;
  constexpr bool HAS_I8W = (NB == 1);                    // the product runs filter_i8w_kernel for batches <= 128 only
  constexpr bool HAS_I8P32 = (DIM < 384);                // ... and the 32x32x32 logged build only where the 16x16x64 build does not exist
#endif
  const uint32_t nwg = filter_grid(c, run.QT);
  nvdb_status st;
  SyncArgs sy;
  if ((st = sibling_sync_args(c, run, nwg, sy))) return st;
  const bool sync = sy.prog != nullptr;
  // (every build's survivor log is sized for 8 waves per workgroup)
  auto launch = [&](auto kern, uint32_t waves, size_t lds) {
    return launch_filter_i8w_kernel(c, run, rows, kern, nwg, FilterGeom{64 * waves, lds, 8, true}, static_cast<size_t>(run.nq_pad) * DIM, TROWS, sy);
  };
  // batches <= 128 at d = 512 / 768: the 16x16x64 logged build on 8 waves of 32 queries (waves without queries only load): its first-stage
  // test rides in the MFMA shadow, so four busy waves stay inside the tile time the HBM stream allows (+6.5 % at batch 128,
  // +2.4 % at 64 over filter_i8w_kernel<768, 1>, profiles/r03_i8_small_batch_ab.txt); signed / huge scales keep the in-loop build.
  // One query tile has no siblings: the SYNC = false instantiation alone.
  if constexpr (NB == 1 && (DIM == 768 || DIM == 512))
    if (c->opt_i8_small8 && !defer && run.QT == 1 && run.nq > 8)   // (a handful of queries: equal within noise, the old kernel stays)
      return launch(filter_i8s_kernel<DIM, false, false, 6, 8>, 8, filter_i8s_lds_bytes<DIM, 8>());
  if constexpr (NB == 1 && DIM == 384)               // d = 384 has no 8-wave schedule: 64 < batch <= 128 on the 4-wave build, two waves without queries (+4 % at 128; equal at 64)
    if (c->opt_i8_small8 && !defer && run.QT == 1 && run.nq > 64)
      return launch(filter_i8s_kernel<DIM, false, false, 6, 4>, 4, filter_i8s_lds_bytes<DIM, 4>());
  if (logs && c->opt_i8_mfma16) {
    // d = 768: on 8 waves of 32 queries, two per SIMD (option i8_dense8).  A flagged block runs rare_log, serial work during which a lone wave's
    // MFMA pipe idles; with two waves per SIMD the partner's MFMAs fill it.  Per launch of the N = 10M ladder the 8-wave build wins 10 / 10 / 5 %
    // where many blocks are flagged and is equal on the last, sparse chunk -- but a 4-wave launch that FOLLOWS 8-wave ones ran 5 % slower than
    // after 4-wave ones, so a search does not mix them (profiles/r07_step0_waves_per_launch.txt, r07_ab_dense8.txt)
    // a shadow written under one common scale (shadow_scale_plan.h): shadow_i8c_kernel, whose first-stage test compares raw accumulator bits --
    // same log, same survivors (d = 768, both wave counts; option shadow_common_scale = 0 set AFTER the load keeps the per-row build on it)
    const bool common = run.kind == FILTER_SHADOW8 && c->q8shadow && c->shadow_cs.common && c->opt_shadow_common_scale != 0;
    if constexpr (DIM == 768) {
      if (common) {
        if (w8 || c->opt_i8_dense8) return launch(i8c_build<DIM, 8>(sync), 8, filter_i8s_lds_bytes<DIM, 8>());
        return launch(i8c_build<DIM, 4>(sync), 4, filter_i8s_lds_bytes<DIM, 4>());
      }
    }
    (void)common;
    if constexpr (DIM == 768 || (DEV_I8S8_512 && DIM == 512))      // (the developer library also holds the d = 512 build; it runs at d = 768 only)
      if ((w8 || c->opt_i8_dense8) && DIM == 768) return launch(i8s_build<DIM, 8>(sync), 8, filter_i8s_lds_bytes<DIM, 8>());
    if constexpr (DIM >= 384)
      if (!w8) return launch(i8s_build<DIM, 4>(sync), 4, filter_i8s_lds_bytes<DIM, 4>());
  }
#ifdef NVDB_HIP_DEV
  if constexpr (DIM != 384)                            // the 8-wave pipelined build: the in-loop second stage only, no d = 384 schedule
    if (w8) return launch(i8p_build<DIM, 8, true>(sync), 8, filter_i8p_lds_bytes<DIM, 8, true>());
#endif
  if (pipe && defer) return launch(i8p_build<DIM, 4, true>(sync), 4, filter_i8p_lds_bytes<DIM, 4, true>());
  if constexpr (HAS_I8P32)
    if (pipe) return launch(i8p_build<DIM, 4, false>(sync), 4, filter_i8p_lds_bytes<DIM, 4, false>());
  if constexpr (HAS_I8W)
    if (!pipe) return launch(i8w_build<DIM, NB, 2>(sync), 4, filter_i8w_lds_bytes<DIM, 2>());
  return fail(c, NVDB_ERR_INTERNAL, "int8 two-stage kernel: no build for this batch");
}

// int8, 768 < dim <= 1536: the two-stage kernel on 32-row tiles with one 32-query block per wave (128 queries per workgroup);
// the reference takes any dim (src/simd_dot.cpp:160-213)
template <int DIM>
nvdb_status launch_filter_i8w_big_dim(nvdb_hip_ctx* c, FilterRun& run, RowRange rows) {
  constexpr uint32_t TROWS = i8w_tile_rows(DIM);
  static_assert(TROWS == FILTER_ROWS, "the builds of dims > 768 stream one 32-row block per tile");
  if ((rows.hi - rows.lo) % TROWS) return fail(c, NVDB_ERR_INTERNAL, "int8 kernel: row range is not a multiple of its 32-row tile");
  const uint32_t nwg = filter_grid(c, run.QT);
  nvdb_status st;
  SyncArgs sy;
  if ((st = sibling_sync_args(c, run, nwg, sy))) return st;
  return launch_filter_i8w_kernel(c, run, rows, i8w_build<DIM, 1, 1>(sy.prog != nullptr), nwg, FilterGeom{256, filter_i8w_lds_bytes<DIM, 1>(), 4, true},
                                  static_cast<size_t>(run.nq_pad) * DIM, TROWS, sy);
}

// the boot build is the 128-queries-per-workgroup two-plane kernel: QT counts ITS query tiles, nb per tile of the run (same padded batch)
template <int DIM>
nvdb_status launch_boot_i8_dim(nvdb_hip_ctx* c, FilterRun& run, RowRange rows) {
  const uint32_t QT = run.nq_pad / 128u;
  return launch_filter_i8_kernel(c, run, rows, QT, filter_i8_kernel<DIM, true>, filter_grid(c, QT), FilterGeom{256, filter_i8_lds_bytes<DIM>(), 0, false},
                                 static_cast<size_t>(run.nq_pad) * DIM, &c->cand, scatter_args(c, run, FILTER_ROWS), run.cap, static_cast<uint32_t*>(nullptr), 0u, 0u);
}

nvdb_status launch_boot_i8(nvdb_hip_ctx* c, FilterRun& run, uint32_t n0) {
  nvdb_status st;
  if (dispatch_dim(I8Dims{}, c->fdim, st, [&](auto D) { return launch_boot_i8_dim<decltype(D)::value>(c, run, RowRange{0, n0}); })) return st;
  return fail(c, NVDB_ERR_UNSUPPORTED, "int8 boot kernel: unsupported dim");
}

nvdb_status launch_filter_i8(nvdb_hip_ctx* c, FilterRun& run, RowRange rows) {
  const uint32_t nb = filter_nb(c, run.kind, run.nq);
  nvdb_status st;
  if (dispatch_dim(I8DimsBig{}, c->fdim, st, [&](auto D) { return launch_filter_i8w_big_dim<decltype(D)::value>(c, run, rows); })) return st;
  if (i8_two_stage(c, run.kind) && dispatch_dim(I8Dims{}, c->fdim, st, [&](auto D) {
        return nb == 2 ? launch_filter_i8w_dim<decltype(D)::value, 2>(c, run, rows) : launch_filter_i8w_dim<decltype(D)::value, 1>(c, run, rows);
      })) return st;
#ifdef NVDB_HIP_DEV
  if (dispatch_dim(I8Dims{}, c->fdim, st, [&](auto D) { return launch_filter_i8_dim<decltype(D)::value>(c, run, rows); })) return st;
#endif
  return fail(c, NVDB_ERR_UNSUPPORTED, "int8 filter kernel: unsupported dim");
}

}  // namespace nvdbhip
