/*
 * nvdb_hip_dev.h -- developer entry points of libnvdb_hip_dev.so (csrc/nvdb_debug.cpp; the library built with -DNVDB_HIP_DEV).
 *
 * NOT part of the drop-in surface: the product library libnvdb_hip.so exports none of these and contains none of the
 * stamped kernel builds behind them.  The dev library is a superset of the
 * product library (same C ABI, include/nvdb_hip.h); tools_dev/ and one CPU test load it explicitly.
 */
#ifndef NVDB_HIP_DEV_H
#define NVDB_HIP_DEV_H

#include "nvdb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Developer aid: the clock the chip holds inside the production fp16 d=768 filter kernel.  Launches a diagnostic
 * build (identical code + one s_memtime / s_memrealtime stamp pair around the tile loop of every workgroup; thresholds +inf)
 * on the resident corpus with the query workspace of the previous search (128 < nq <= its padded batch), back to
 * back for `seconds`, then reports out4 = { ms per launch (last 8), median, min, max over workgroups of
 * delta(s_memtime) / delta(s_memrealtime) x 100 MHz in GHz, mean and max over workgroups of the tile loop's duration in us, then per XCD label (blockIdx % 8) the mean duration and its spread } (22 floats).
 * variant: 0 = the 4-wave loop, 20 = the 8-wave production loop; any other number is NVDB_ERR_INVALID (the timing-only
 * ablation builds 1, 5, 15, 16, 17 were retired: profiles/README.md). */
nvdb_status nvdb_hip_debug_clock(nvdb_hip_ctx* ctx, int variant, uint32_t nq, float seconds, float* out4);

/* The tile range [lo, hi) the device's XCD-balanced partition (kernels_filter.h stream_tile_range) gives each of n_streams
 * row streams over n_tiles tiles, evaluated ON the device with weights8 (8 floats; NULL = the context's current, adapted
 * weights, which are also returned in weights_out8 if that is non-NULL).  tests/test_gpu_parity.py checks that the ranges tile
 * [0, n_tiles) exactly for any weights. */
nvdb_status nvdb_hip_debug_tile_ranges(nvdb_hip_ctx* ctx, uint32_t n_tiles, uint32_t n_streams, const float* weights8, uint32_t* out_lo,
                                       uint32_t* out_hi, float* weights_out8);

/* Developer aid (host only, no GPU): the physical tile the filter kernels stream for logical tile g of a corpus of n_tiles
 * tiles -- a bijection of [0, n_tiles) (identity below 64 tiles).  tests/test_cabi_cpu.py checks that property. */
uint32_t nvdb_permuted_tile(uint32_t g, uint32_t n_tiles);

/* The same for the int8 two-stage kernels (int8 d=768 corpus, nq > 128; the thresholds the last search ended with): stamped builds of
 * 0 = filter_i8w_kernel<768,2>, 10 = the software-pipelined build with the in-loop second stage (filter_i8p_kernel, DEFER),
 * 20 = filter_i8p_kernel with first-stage survivors logged, 30 = the 16x16x64 build (filter_i8s_kernel), 35 = that build on 8 waves;
 * any other number is NVDB_ERR_INVALID (the timing-only ablation builds were retired: profiles/README.md).  out[0..3] as above, out[4], out[5] = rare-path
 * entries and lo-plane MFMA blocks per launch, out[6], out[7] = mean and longest tile-loop duration of a workgroup in us (out must hold 8 floats).
 * Developer option "debug_rows" (nvdb_hip_set_option, this build only): the launches cover rows [0, debug_rows) instead of the corpus. */
nvdb_status nvdb_hip_debug_clock_i8(nvdb_hip_ctx* ctx, int variant, uint32_t nq, float seconds, float* out4);

/* What one flat search of nq queries for the k best would do on a corpus of the given shape -- the plan the search entry
 * points compute before their first launch (csrc/nvdb_plan.h), for a context described by plain numbers.  Needs NO device.
 * The options are applied through nvdb_hip_set_option itself, so ranges and developer-only keys behave as in a real context. */
typedef struct nvdb_hip_plan_shape {
  uint64_t n;
  uint32_t dim, fdim, dtype;                  /* fdim: the dim the filter kernels run at (== dim without a padded shadow) */
  uint32_t owned, has_shadow16, has_shadow8, q8shadow, i8_scales_signed;
  uint32_t num_cu, cap_hint;
  uint32_t shadow_demoted;                    /* the int8 filter shadow has overflowed on this corpus before (the retry ladder's flag) */
  uint32_t load_rule;                         /* 1: whether the corpus has an int8 filter shadow is decided as at load time, from the options */
  uint64_t free_hbm;                          /* ... "q8_shadow", "q8_auto_min_rows", "q8_auto_max_mb" and this many bytes of free HBM */
} nvdb_hip_plan_shape;

typedef struct nvdb_hip_plan_option { const char* key; int64_t value; } nvdb_hip_plan_option;

#define NVDB_PLAN_MAX_CHUNKS 64
typedef struct nvdb_hip_plan {
  uint32_t route;                             /* 1 exact, 2 filter, 3 any-k: nvdb_hip_scan_stats.path of the search */
  uint32_t prep, prep_inits, k_wide;          /* prep: the filter flow's prep launch runs (also ahead of an any-k search the bootstrap rules sent there) */
  uint32_t k_eff, cap, QPB, QT, nq_pad, prog_words;
  uint32_t head;                              /* exact route: rows of the prescan (0: one scan) */
  uint32_t padded, perm_on;
  uint32_t boot;                              /* filter route: 0 MFMA bootstrap, 1 exact chunk [0, r0), 2 any-k machinery seeding the lists from [0, r0) */
  uint32_t tile_rows, n_al, growth, boot_tiles, boot_rows, r0, tail_exact;
  uint32_t helper_tile_rows;                  /* what the launchers' shared helper says a tile of this shape holds */
  uint32_t n_chunks;                          /* filter route: the filter launches, [chunk_lo[i], chunk_hi[i]) */
  uint32_t chunk_lo[NVDB_PLAN_MAX_CHUNKS], chunk_hi[NVDB_PLAN_MAX_CHUNKS];
  uint32_t stat_chunks;                       /* nvdb_hip_scan_stats.chunks / .rows_scanned the search will report (any-k: for a batch */
  uint64_t stat_rows_scanned;                 /* whose score matrix fits the HBM budget in one piece -- only the device knows) */
  uint32_t filter_shadow;                     /* filter route: 1 = the launches stream the int8 shadow of an fp16 / fp32 corpus, 0 = the corpus' own dtype's kernels */
} nvdb_hip_plan;

/* err (may be NULL): err_len bytes for the message of a status != NVDB_OK -- a rejected option, an unsupported shape
 * (the search's own message), more than NVDB_PLAN_MAX_CHUNKS chunks. */
nvdb_status nvdb_hip_debug_plan(const nvdb_hip_plan_shape* shape, const nvdb_hip_plan_option* opts, uint32_t n_opts, uint32_t nq, uint32_t k,
                                int force_path, uint32_t cap_override, nvdb_hip_plan* out, char* err, size_t err_len);

#ifdef __cplusplus
}
#endif
#endif /* NVDB_HIP_DEV_H */
