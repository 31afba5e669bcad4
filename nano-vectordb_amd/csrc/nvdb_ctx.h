// nvdb_ctx.h -- internal to libnvdb_hip.so: the context behind the C ABI (include/nvdb_hip.h), the small host helpers every
// translation unit uses, and the declarations of what one unit calls in another.  Not installed, not part of the boundary.
//
//   nvdb_corpus.cpp        create / destroy, corpus upload / adopt / generate (+ shadow copies, row-norm pass), options, statistics
//   nvdb_plan.h            what one flat search will do (plan_search): route, list capacity, query tiling, bootstrap, chunk boundaries -- decided
//                          before anything is enqueued, from a CONST context, no HIP call; the filter choice (filter_kind) travels in the plan, then in the flow's FilterRun
//   nvdb_search.cpp        one flat search: plan -> prologue (begin_filter_run, the range search's too) -> launches (search_core); entry points, self-checks, retry ladder
//   nvdb_range.cpp         range search (every row whose score reaches a per-query radius): plan, filter route, exact route, packing (kernels_range.h)
//   nvdb_range_parts.cpp   range search on the probe path: the partition range scan, its per-query tail, the probe / IVF / masked entry points
//                          (kernels_range_parts.h, range_plan.h; nvdb_range.h and nvdb_parts.h are what it shares with its two neighbours)
//   nvdb_launch_f16.cpp    launch helpers of the fp16 MFMA filter kernels (kernels_filter.h), query prep for them
//   nvdb_launch_i8.cpp     ... of the int8 kernels (kernels_filter.h, kernels_filter_i8s.h)
//   nvdb_launch_exact.cpp  ... of the exact fp32-order kernels, select / rescore / merge, the any-k path (kernels_exact*.h, kernels_largek.h)
//   nvdb_refine.cpp        exact-L2 refine (kernels_refine.h)
//   nvdb_partitions.cpp    partitioned probe search: partition table, coarse quantiser, the pass driver of every partition scan (nvdb_parts.h: work list ->
//                          image -> copies -> launches by class), the top-k argument check; row masks and the masked searches (kernels_partitions.h, row_mask.h)
//   parts_worklist.h       the work list itself and its image's layout, plain C++ with no HIP call (as nvdb_plan.h, range_plan.h, parts_anyk_plan.h, masked_plan.h)
//   nvdb_parts_anyk.cpp    the probe search for any k: per sub-batch one pass at radius -inf, select, long slabs (kernels_parts_anyk.h, parts_anyk_plan.h)
//   nvdb_masked_flat.cpp   the masked flat top-k on the MFMA filter route: prefix rank, bootstrap bar, the range search's filter pass, top-k of the kept
//                          lists (kernels_masked_topk.h, masked_plan.h)
//   nvdb_compact.cpp       in-place compaction of tombstoned rows: rank, slab walk (direct / bounce), planes, partition table (kernels_compact.h, compact_plan.h);
//                          nvdb_hip_compact_rows here, nvdb_hip_ivf_compact beside the index in nvdb_ivf.cpp
//   nvdb_insert.cpp        insertion at the ends of partitions, in place or into grown buffers: plan, descending slab walk (direct / bounce), scatter of the
//                          staged rows and their shadows, planes, table (kernels_insert.h, insert_plan.h, nvdb_insert.h); nvdb_hip_reserve_rows and
//                          nvdb_hip_insert_rows here, nvdb_hip_ivf_add_rows beside the index in nvdb_ivf.cpp
//   nvdb_ivf.cpp           IVF-Flat build: row assignment, spherical k-means, list layout, the reordered index and its searches (the context's, ids mapped
//                          back by ivf_map_ids) (kernels_ivf.h, ivf_layout.h)
//   nvdb_debug.cpp         developer entry points (libnvdb_hip_dev.so only)
//   nvdb_group.cpp         device group, layered on the public ABI (does not include this header)
// There is NO CPU fallback anywhere in these files: without a working HIP device every entry point that computes returns
// NVDB_ERR_HIP.
#pragma once
// the library is built with -fvisibility=hidden: only what the public headers declare is exported
#pragma GCC visibility push(default)
#include "../../include/nvdb_hip.h"
#ifdef NVDB_HIP_DEV
#include "../../include/nvdb_hip_dev.h"
#endif
#pragma GCC visibility pop

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "kernels_exact.h"       // Cand, FinalSelect
#include "kernels_filter.h"      // Hit, ScatterArgs, PrepInit, tile constants
#include "nvdb_common.h"
#include "shadow_scale_plan.h"

using namespace nvdbhip;

namespace nvdbhip {

constexpr uint32_t SELECT_MAX_CAP = 8192;     // 64 KB of LDS in select_kernel
constexpr uint32_t WAVE_KMAX = 64;            // k the wavefront-resident top-k lists hold (entry j in lane j)
constexpr uint32_t FILTER_KMAX = 1024;        // k the filter path's 8192-entry lists (and its bootstrap over 8k tile maxima) hold
constexpr float FILTER_REL_F16 = 7.5e-4f;     // |filter - reference| <= REL * ||q|| * max||x||   (DESIGN.md "error bound")
constexpr uint32_t PROG_SLOTS = 16;           // filter launches per search whose rendezvous counters the init kernel pre-clears
constexpr uint32_t F16_FILTER_MAX_DIM = 3072;
constexpr uint32_t I8W_TILE_ROWS = 64;        // rows per tile of the int8 two-stage kernel (two 32-row blocks)
constexpr uint32_t PAD_ROWS = 64;             // zero rows every library-owned corpus / shadow is padded with: the largest tile
constexpr uint32_t I8_FILTER_MAX_DIM = 1536;

// what a search's filter launches stream: nothing (exact / any-k route), fp16 rows (the corpus or its fp16 shadow), the int8 shadow of an fp16 / fp32 corpus, an int8 corpus
enum FilterKind : uint32_t { FILTER_NONE = 0, FILTER_F16 = 1, FILTER_SHADOW8 = 2, FILTER_I8 = 3 };
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

struct PartState;                             // nvdb_partitions.cpp: partition table, centroids and workspace of the probe search

}  // namespace nvdbhip

struct nvdb_hip_ctx {
  int device = 0;
  int num_cu = 256;
  hipStream_t stream = nullptr;
  std::string err;

  // resident corpus
  void* rows = nullptr;
  float* scales = nullptr;
  bool owned = false;
  uint64_t n = 0;
  uint64_t cap_rows = 0;                           // rows the OWNED arrays (rows, scales, shadows) have room for, their padding aside: n after a load, more after
                                                   // nvdb_hip_reserve_rows / a grown nvdb_hip_insert_rows; a compaction keeps it
  uint32_t dim = 0, dtype = 0;
  uint64_t row_base = 0;
  float max_norm = 0.f;
  bool i8_scales_signed = false;                   // int8 corpus with a negative or NaN row scale: the in-loop second-stage build (no biased accumulators)
  signed char* shadow8 = nullptr;                  // int8 corpus with a dim the kernels are not instantiated for: rows zero-padded to fdim; or (q8shadow) the int8 FILTER shadow of an fp16 / fp32 corpus
  bool q8shadow = false;                           // fp16 / fp32 corpus with a resident int8 FILTER shadow (option q8_shadow): the int8 MFMA kernels can stream shadow8, every survivor is re-scored from the original rows
  bool shadow_demoted = false;                     // the shadow's lists or wave logs overflowed on this corpus (host API's retry ladder): searches start on the fp16 filter, in the spirit of cap_hint; a reload clears it
  float filter_max_norm = 0.f;                     // max row norm of what the int8 filter streams (== max_norm for an int8 corpus; the shadow's for q8shadow -- max_norm stays the fp16 filter's)
  float resid_max = 0.f;                           // q8shadow: largest ||x - scale * x_q|| over the rows -- the corpus side of the filter's error bound
  ShadowScaleFact shadow_cs;                       // q8shadow: is the shadow written under ONE scale (shadow_scale_plan.h)?  common: the flat search runs the bits-domain first stage
  int64_t opt_shadow_common_scale = -1;            // set before the corpus is loaded: 0 = the shadow keeps the reference's per-row scales, otherwise automatic (one common scale where shadow_cs_keep allows it)
  int64_t opt_q8_shadow = -1;                      // set before the corpus is loaded: 1 = build the int8 filter shadow for fp16 / fp32 corpora whose dim the int8 kernels take, 0 = never (set later: also stop
                                                   // streaming a resident one where the fp16 filter stands beside it), -1 = automatic (q8_shadow_wanted below)
  int64_t opt_q8_auto_min_rows = 1 << 20;          // automatic shadow: corpora with at least this many rows (smaller ones are latency-bound: today's chain) ...
  int64_t opt_q8_auto_max_mb = 16384;              // ... whose shadow takes at most this much HBM (and at most a quarter of what is free once the corpus is resident)
  float* shadow8_scales = nullptr;                 // ... and its scales in a buffer padded to whole tiles
  _Float16* shadow16 = nullptr;                    // fp16 copy streamed by the MFMA filter (fp32 corpus and/or padded dim)
  uint32_t fdim = 0;                               // dim the filter kernels run at (>= dim; == dim without padding)
  DevBuf qdelta;                                   // int8: per query, what the lo plane can add to a filter value
  int64_t opt_i8_wide = 1;
  int64_t opt_i8_waves8 = 0;                       // developer library: EVERY int8 build of a batch > 128 on 8 waves of 32 queries (two per SIMD) instead of 4 of 64, with the ladder of the
                                                   // unlogged builds; off.  The product's 8-wave build is option i8_dense8
  int64_t opt_i8_dense8 = 1;                       // int8 filter, d = 768, batches > 128: the 16x16x64 logged build on 8 waves of 32 queries -- while one wave of a SIMD logs first-stage
                                                   // survivors the other's MFMAs keep the pipe busy: +2.4-4.0 % on the int8 shadow, +1.2-2.4 % on an int8 corpus (profiles/r07_ab_dense8.txt); 0: 4 waves of 64
  int64_t opt_i8_defer = 0;                        // pipelined build: 1 = second stage inside the tile loop (deferred v_dot4 slots), 0 = log the first stage's survivors, finish them after the stream
  int64_t opt_i8_mfma16 = 1;                       // int8 batches > 128, d = 512 / 768: the pipelined build on v_mfma_i32_16x16x64_i8 (kernels_filter_i8s.h): +7.3 % (profiles/r03_i8_mfma16_ab.txt); 0 (developer build): the 32x32x32 build
  int64_t opt_i8_pipe = 1;                         // int8 batches > 128: software-pipelined build (stage-1 test in the shadow of the other row block's MFMAs)
  int64_t opt_waves8 = 1;                          // d=768: 8-wave workgroups (two waves per SIMD, 32 queries each) for the fp16 m16 kernel: +2.3 % (0: four waves x 64 queries)
  void* pinned = nullptr;                           // pinned host staging of small calls: status words, results, queries
  void* pinned_dev = nullptr;                       // ... as the device addresses it (hipHostGetDevicePointer)
  size_t pinned_bytes = 0;
  int64_t opt_tile_permute = 1;
  uint32_t cap_hint = 0;                            // this corpus has needed the longest candidate lists before: start with them
  bool stats_lazy = false;                          // stats.candidates not read back yet (nvdb_hip_get_stats does it)
  std::vector<hipEvent_t> kl_pool;                  // recycled events of collected launches
  int64_t opt_time_launches = 0;                   // host API with a timing struct: 1 = also attach start / stop events to every filter launch (stats.filter_kernel_ms); costs ~0.1 ms per launch-rich pass
  int64_t opt_exact_lds = 1;                       // exact MFMA kernels: full groups of 64 queries stage their row tiles through LDS once per workgroup: 1 = for fp32 rows (101 vs 75 TFLOP/s; fp16 / int8 rows are faster register-direct: 86 vs 77), 2 = always, 0 = never
  int64_t opt_exact_img = 1;                       // exact MFMA kernels, fp16 / int8 rows, full groups of 64 queries: tile converted once per workgroup into an fp32 LDS image (exact_mfma_img_kernel); 0: register-direct / raw-staged builds
  int64_t opt_exact_wgs = 1;                       // exact MFMA SCAN kernels: workgroups per CU in all (one is resident at a time).  1 = a single round: every workgroup pays the start-up of its
                                                   // top-k lists (the first ~150 tiles of a stream take the insertion path) once, and the grid (wgs * CUs / query groups, rounded DOWN) never leaves
                                                   // a partly filled last round -- 2, the value of round 3, cost 5-30 % (profiles/r04_exact_wgs_sweep.txt: 128 queries 67 -> 90 TFLOP/s)
  int64_t opt_exact_prescan = 1;                   // path 1, more than 8 queries, >= 1M rows: scan the first 1/64 of the rows on its own and start the rest with its exact k-th best scores as the bar
  int64_t opt_exact_mfma = 1;                      // exact fp32-order scores on the fp32 matrix cores where the shape allows (kernels_exact_mfma.h); 0: VALU kernels only
  int64_t opt_rescore8 = 2;                        // rescore kernel: 0 lane per candidate, 1 eight lanes per candidate, 2 = 1 + rows staged through LDS

  // grow-only workspace
  DevBuf q32, q16, qscale, qinv, ebound, slack, thr, cnt, overflow, cand, out_ids, out_scores, misc, hitlog, prog;
  DevBuf hostblock;                                // host API, <= 1024 queries: [status words (= misc, aliased) | ids | scores] in one allocation, one D2H copy
  DevBuf tickets;                                  // FUSE_TICKETS words, zeroed by the search's prep launch: "last workgroup" ticket of the fused rescore + final select
  int64_t opt_fuse = 1;                            // 1: init folded into the prep launch, the final select into the rescore launch; 0: separate launches
  int64_t opt_shadow_exact_thr = 1;                // searches that stream the int8 shadow, k <= 64: thresholds one error bound under an EXACT k-th best score (the selects re-score their best 2k entries); 0: two bounds under the k-th list score
  int64_t opt_zero_copy = 1;                       // host API, small calls: queries read from / results written to pinned host memory by the kernels themselves (no H2D / D2H copy enqueued)
  bool status_by_kernel = false;                   // last search_core: its final kernel wrote the status words to the caller's pinned block
  size_t q32_dirty = 0;                            // bytes of q32 (from its start) that may hold old queries: beyond them the buffer is zero
  DevBuf rq, rcand, rout_ids, rout_dist;           // refine
  DevBuf rdbg;                                     // refine phase stamps: 3 x uint64 per sampled query (option refine_dbg_q)
  DevBuf xcdw;                                     // XCD balance: 8 speed weights + 16 accumulators (kernels_filter.h ScatterArgs::xcdw)
  int64_t opt_xcd_balance = 1;
  int64_t opt_i8_lo_bits = 7;                      // int8: bits of a quantised query's lo plane (ScatterArgs::lo_bits)
  int64_t opt_boot_tiles = 0;                      // threshold bootstrap over this many 32-row tile maxima (0: max(64, 8k))
  int64_t opt_i8_small8 = 1;                       // int8 d = 512 / 768, batches <= 128: 1 = the 8-wave 16x16x64 logged build, 0 = filter_i8w_kernel<768, 1> (developer library)
  int64_t dbg_rows = 0;                            // developer build: rows the stamped launches of nvdb_hip_debug_clock_i8 cover (0: the corpus)
  int64_t dbg_bound_pct = 100;                     // developer build: per cent of max_norm / filter_max_norm / resid_max the query prep is handed (tests/test_gpu_filter_bound.py: a case must fail under a short bound)
  DevBuf lk_scores, lk_sel, lk_hist, lk_state;     // any-k path (kernels_largek.h): score matrix of a query sub-batch, selected keys, radix state
  int64_t opt_refine_pinned = 0;                   // refine host call: stage queries / candidates / results through pinned host buffers (reference CUDA_PINNED)
  int64_t opt_refine_dbg_q = 0;                    // refine host call with a timing struct: the first min(this, Q) queries run the STAMP build of the same kernel template (reference CUDA_DBG_TIMING / CUDA_DBG_Q); 0 = off
  void* rpinned = nullptr;                         // ... [queries | candidates | out ids | out dist]
  size_t rpinned_bytes = 0;
  int64_t opt_largek_budget_mb = 8192;             // HBM the any-k path may use for its score matrix
  // range search (nvdb_range.cpp): the last call's packed results stay here for nvdb_hip_range_results
  DevBuf rg_radius, rg_kept, rg_off, rg_idx, rg_q, rg_desc, rg_taken, rg_slab;   // radii, list / score counts, pack offsets, flagged queries (numbers, compact batch), exact-route passes
  DevBuf rg_pcnt, rg_maskof;                       // partition range scan: per-query entry counts; masked flat range search: mask_of on the device
  DevBuf rg_ids, rg_scores;                        // packed global ids / scores of the last range search (grow-only)
  uint64_t range_total = 0;                        // ... their entries
  bool range_valid = false;                        // ... and whether nvdb_hip_range_results may hand them out (false: none yet, over budget, corpus changed)
  int64_t opt_range_max_mb = 4096;                 // packed results (12 bytes per entry) a range search may hold

  // options
  int64_t opt_path = 0, opt_chunk0 = 512, opt_cap = 0, opt_min_filter_batch = 1, opt_growth = 0;   // opt_growth 0 = automatic

  // state of the last search
  nvdb_hip_scan_stats stats{};
  uint32_t last_nq = 0, last_cap = 0;
  bool last_filter = false;
  FilterKind last_filter_kind = FILTER_NONE;       // what its filter launches streamed
  bool last_perm = false;                          // ... in permuted tile order (of the last search that filtered: nvdb_hip_debug_clock_i8 streams the same way)
  std::vector<hipEvent_t> ev_pool;
  std::vector<std::pair<int, int>> ev_filter;      // (start,stop) event indices of filter launches (last search)
  // kernel-time accounting across searches ("time_kernels" option): one entry per dominant-kernel launch
  struct KLaunch { hipEvent_t e0, e1; double flops, bytes; };
  std::vector<KLaunch> klaunch;
  int64_t opt_time_kernels = 0;
  int64_t opt_sync_every = 4, opt_sync_lead = 4;   // rendezvous period (power of two, tiles) and allowed lead
  int64_t opt_sibling_sync = 1;                    // 1: co-streaming workgroups rendezvous every 8 tiles (L2 sharing)
  int64_t opt_f32_shadow = 1;                      // 1: fp32 corpora get an fp16 shadow copy for the MFMA filter
  int64_t opt_mfma_boot = 1;                       // 1: threshold bootstrap on the matrix cores (fp16 corpora)
  int64_t opt_refine_v2 = 2;                       // refine kernel: 0 lane per row, 1 column chunks through LDS, 2 whole rows through LDS (fp16 d = 256/384/512/768; else 1)
  int64_t opt_mfma16 = 1;                          // 1: use the 16x16x32 MFMA build for 256-query tiles
  std::set<const void*> lds_attr_set;              // kernels whose dynamic-LDS limit was raised on this device
  nvdbhip::PartState* parts = nullptr;             // partitioned probe search (created by nvdb_hip_set_partitions, or by the first masked flat search)
  DevBuf row_masks, mask_rows;                     // row masks (nvdb_hip_set_row_masks): [nmasks][ceil(n / 32)] words; staging of nvdb_hip_update_row_mask's row list
  uint32_t nmasks = 0;                             // ... planes resident (0: none; any corpus load drops them, the buffer stays)
  std::vector<uint64_t> mask_live;                 // ... and their live rows as the host knows them: counted when the planes are set, moved by the length of every
                                                   // update's row list (an ESTIMATE -- a list may name a row twice or a row already in that state); read by the masked
                                                   // flat search's automatic route only, never by a result; exact after nvdb_hip_compact_rows
  // compaction (nvdb_compact.cpp): grow-only workspace -- tile ranks, their block sums / bases, one slab of the widest array, the map, the planes' live counts --
  // and the spare the repacked planes are written to before it is swapped with row_masks
  DevBuf cp_rank, cp_sums, cp_bounce, cp_map, cp_live, row_masks_alt;
  int64_t opt_compact_slab_rows = 65536;           // rows per slab of the walk (a multiple of 64; compact_plan.h): profiles/compact_bench_10M.txt; the insertion's walk too
  // insertion (nvdb_insert.cpp): grow-only workspace -- [old offsets | shifts | new offsets], the new rows' positions; the staged rows live for one call only
  DevBuf ins_meta, ins_pos;
  int64_t opt_insert_growth_pct = 50;              // an insertion that outgrows cap_rows reallocates to max(n + m, cap_rows * (100 + this) / 100) rows; 0: exactly n + m
};

#define HIPCHK(ctx, call)                                                                        \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
      return NVDB_ERR_HIP;                                                                       \
    }                                                                                            \
  } while (0)

namespace nvdbhip {

inline nvdb_status fail(nvdb_hip_ctx* c, nvdb_status s, const std::string& msg) {
  c->err = msg;
  return s;
}

inline nvdb_status ensure(nvdb_hip_ctx* c, DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return NVDB_OK;
  if (b.p) { HIPCHK(c, hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
  size_t want = std::max<size_t>(bytes, 256);
  HIPCHK(c, hipMalloc(&b.p, want));
  b.bytes = want;
  return NVDB_OK;
}

inline size_t bpe_of(uint32_t dtype) { return dtype == NVDB_DTYPE_F32 ? 4 : (dtype == NVDB_DTYPE_F16 ? 2 : (dtype == NVDB_DTYPE_I8 ? 1 : 0)); }

inline bool aligned_rows(uint32_t dtype, uint32_t dim) {
  if (dtype == NVDB_DTYPE_F32) return dim % 4 == 0;
  return dim % 8 == 0;    // f16: 16-byte groups of 8; int8: 8-byte groups of 8
}

// dims the fp16 MFMA kernels are instantiated for: multiples of 128 up to 768 (64 queries per wave: their fragments fill
// 384 registers at 768), up to 1536 on the 16-row-tile build (32 queries per wave), 2048 / 2560 / 3072 on the K-split build
// (16 queries per wave, a tile streamed as two half-K stages); int8 rows: every multiple of 128 bytes from 256 (swz_chunk's
// two families), beyond 768 on 32-row tiles.  The launchers dispatch from these lists and the predicates are read off them.
template <int... D> struct DimList {};
using F16Dims = DimList<768, 640, 512, 384, 256, 128>;
using F16Dims16 = DimList<896, 1024, 1152, 1280, 1408, 1536>;
using F16DimsK2 = DimList<2048, 2560, 3072>;
using I8Dims = DimList<768, 640, 512, 384, 256>;
using I8DimsBig = DimList<896, 1024, 1152, 1280, 1408, 1536>;
// the exact fp32-MFMA kernels (kernels_exact_mfma.h): dim % 32 == 0 (no scalar tail), 16 queries x dim floats in registers
using ExactMfmaDims = DimList<768, 640, 512, 384, 256, 128>;
// fp16 dims of the whole-row refine kernel (kernels_refine.h, v3): rows of 512 bytes to 1 KB, or of 1536 bytes
using Refine3Dims = DimList<768, 512, 384, 256>;

// st = f(std::integral_constant<int, D>) for the D of the list that equals dim; false: the list does not hold dim
template <int... D, typename F>
bool dispatch_dim(DimList<D...>, uint32_t dim, nvdb_status& st, F&& f) {
  return ((dim == static_cast<uint32_t>(D) && ((st = f(std::integral_constant<int, D>{})), true)) || ...);
}
template <int... D> bool has_dim(DimList<D...>, uint32_t dim) { return ((dim == static_cast<uint32_t>(D)) || ...); }
// st = f(std::integral_constant<int, DT_*>) for the corpus dtype (anything that is neither fp32 nor fp16 is int8, as in every launcher)
template <typename F>
void dispatch_dtype(uint32_t dtype, nvdb_status& st, F&& f) {
  if (dtype == NVDB_DTYPE_F32) st = f(std::integral_constant<int, DT_F32>{});
  else if (dtype == NVDB_DTYPE_F16) st = f(std::integral_constant<int, DT_F16>{});
  else st = f(std::integral_constant<int, DT_I8>{});
}

inline bool f16_filter_dim(uint32_t dim) { return has_dim(F16Dims{}, dim) || has_dim(F16Dims16{}, dim) || has_dim(F16DimsK2{}, dim); }
inline bool i8_filter_dim(uint32_t dim) { return has_dim(I8Dims{}, dim) || has_dim(I8DimsBig{}, dim); }

// what the int8 MFMA kernels stream: an int8 corpus (its zero-padded copy, where the dim needed one), or the int8 filter shadow of an fp16 / fp32 corpus
inline const signed char* filter_rows_i8(const nvdb_hip_ctx* c) { return c->shadow8 ? c->shadow8 : static_cast<const signed char*>(c->rows); }
inline const float* filter_scales_i8(const nvdb_hip_ctx* c) { return c->shadow8 ? c->shadow8_scales : c->scales; }
// what the fp16 MFMA kernels stream: the corpus itself, or the fp16 shadow of an fp32 corpus
inline const _Float16* filter_rows_f16(const nvdb_hip_ctx* c) {
  return c->shadow16 ? c->shadow16 : static_cast<const _Float16*>(c->rows);
}

// a shadow context whose corpus the fp16 filter streams as it is (every int8 dim is an fp16 dim too): both filters are available
inline bool f16_beside_shadow(const nvdb_hip_ctx* c) { return c->q8shadow && c->dtype == NVDB_DTYPE_F16 && f16_filter_dim(c->dim); }
// which of the two a search starts on: the shadow, unless it was switched off after the load or has overflowed on this corpus
inline bool shadow_preferred(const nvdb_hip_ctx* c) { return c->q8shadow && !(f16_beside_shadow(c) && (c->opt_q8_shadow == 0 || c->shadow_demoted)); }
// THE filter choice.  The planners call it once and carry the value in their plan: every shape helper below and every launcher takes it from there
inline FilterKind filter_kind(const nvdb_hip_ctx* c) { return c->dtype == NVDB_DTYPE_I8 ? FILTER_I8 : shadow_preferred(c) ? FILTER_SHADOW8 : FILTER_F16; }
constexpr bool filter_is_i8(FilterKind kind) { return kind == FILTER_I8 || kind == FILTER_SHADOW8; }
// HBM the int8 filter shadow of a corpus takes: a byte per element and a scale per row (padding aside)
inline uint64_t q8_shadow_bytes(uint64_t n, uint32_t dim) { return n * (static_cast<uint64_t>(dim) + 4u); }
// Does a corpus get the shadow when it becomes resident?  free_hbm: what hipMemGetInfo reports free with the corpus resident.
// 1: wherever the int8 kernels take the dim.  Automatic: fp16 corpora only (the fp16 filter streams the corpus itself, so the
// fallback costs no second copy), large enough to be throughput-bound, within the HBM budget.
inline bool q8_shadow_wanted(const nvdb_hip_ctx* c, uint64_t free_hbm) {
  if (c->opt_q8_shadow == 0 || c->dtype == NVDB_DTYPE_I8 || !i8_filter_dim(c->dim)) return false;
  if (c->opt_q8_shadow > 0) return true;
  const uint64_t bytes = q8_shadow_bytes(c->n, c->dim);
  return c->dtype == NVDB_DTYPE_F16 && f16_filter_dim(c->dim) && c->n >= static_cast<uint64_t>(c->opt_q8_auto_min_rows) &&
         bytes <= (static_cast<uint64_t>(c->opt_q8_auto_max_mb) << 20) && bytes <= free_hbm / 4;
}
inline bool filter_supported(const nvdb_hip_ctx* c) {
  if (c->q8shadow) return true;
  if (c->dtype == NVDB_DTYPE_F16) return f16_filter_dim(c->dim) || c->shadow16 != nullptr;
  if (c->dtype == NVDB_DTYPE_F32) return c->shadow16 != nullptr;
  if (c->dtype == NVDB_DTYPE_I8) return i8_filter_dim(c->dim) || c->shadow8 != nullptr;
  return false;
}

// int8: the two-stage kernel (hi plane resident, lo plane on demand); option i8_wide = 0 selects the two-plane kernel
inline bool i8_two_stage(const nvdb_hip_ctx* c, FilterKind kind) { return filter_is_i8(kind) && c->opt_i8_wide; }

// NB = 32-query blocks per wave: 1 for nq <= 128 (HBM-bound regime) and for the two-plane int8 kernel, else 2
inline uint32_t filter_nb(const nvdb_hip_ctx* c, FilterKind kind, uint32_t nq) {
  if (filter_is_i8(kind) && (!i8_two_stage(c, kind) || c->fdim > 768)) return 1u;   // two-plane kernel; dims > 768: 32 queries per wave
  if (!filter_is_i8(kind) && c->fdim > 768) return 1u;       // 16-row-tile build: 128 queries per workgroup
  return nq <= 128 ? 1u : 2u;
}

// ---- shape facts of the filter builds: written here once, used by the launchers (nvdb_launch_f16.cpp, nvdb_launch_i8.cpp)
// AND by plan_search (nvdb_plan.h), which sizes the query tiles and aligns the chunk boundaries with them ----
// a corpus this library allocated (a shadow copy always is) is zero-padded to whole tiles
// (as far as the filter that streams this search goes: the fp16 filter beside an int8 shadow reads the corpus itself)
inline bool corpus_padded(const nvdb_hip_ctx* c, FilterKind kind) { return c->owned || c->shadow16 != nullptr || (c->shadow8 != nullptr && filter_is_i8(kind)); }
// fp16, dims <= 768: batches > 128 (NB == 2) run the 16x16x32 build (developer library: unless option mfma16 = 0) ...
inline bool f16_m16_build(const nvdb_hip_ctx* c, uint32_t nb) { return nb == 2 && c->opt_mfma16; }
// ... whose tiles are MB 16-row blocks: 64-row tiles up to d = 384, 32-row tiles beyond
constexpr uint32_t f16_m16_tile_rows(uint32_t dim) { return dim <= 384 ? 64u : 32u; }
// the int8 two-stage kernel: 64-row tiles (two 32-row blocks) up to d = 768, 32-row tiles beyond
constexpr uint32_t i8w_tile_rows(uint32_t dim) { return dim <= 768 ? I8W_TILE_ROWS : FILTER_ROWS; }
// rows per tile of the build that streams this batch, as far as chunk boundaries care (the 16-row-tile fp16 builds of
// dims > 768 take any multiple of 32)
inline uint32_t filter_tile_rows(const nvdb_hip_ctx* c, FilterKind kind, uint32_t nq) {
  if (filter_is_i8(kind)) return i8_two_stage(c, kind) ? i8w_tile_rows(c->fdim) : FILTER_ROWS;
  return (c->fdim <= 768 && f16_m16_build(c, filter_nb(c, kind, nq))) ? f16_m16_tile_rows(c->fdim) : FILTER_ROWS;
}
// queries per workgroup: fp16 64 on the K-split build (dims > 1536), 128 on the 16-row-tile build (768 < dim <= 1536), else and
// for every int8 build 128 per 32-query block of a wave
constexpr uint32_t f16_filter_qpb(uint32_t dim, uint32_t nb) { return dim > 1536 ? 64u : dim > 768 ? 128u : 128u * nb; }
constexpr uint32_t f16_m16_qpb(uint32_t nqb, uint32_t wpb) { return 16u * nqb * wpb; }   // filter_f16_m16_kernel<.., NQB, WPB>: WPB waves x NQB 16-query blocks
inline uint32_t filter_qpb(const nvdb_hip_ctx* c, FilterKind kind, uint32_t nq) { return filter_is_i8(kind) ? 128u * filter_nb(c, kind, nq) : f16_filter_qpb(c->fdim, filter_nb(c, kind, nq)); }
// int8 two-stage, dims <= 768: batches > 128 run a software-pipelined build (developer library: unless option i8_pipe = 0), which
// logs the first stage's survivors and finishes them after the stream unless the second stage has to stay in the tile loop
inline bool i8_pipelined(const nvdb_hip_ctx* c, FilterKind kind, uint32_t nb) { return i8_two_stage(c, kind) && nb == 2 && c->opt_i8_pipe; }
inline bool i8_stage2_in_loop(const nvdb_hip_ctx* c) { return c->opt_i8_defer != 0 || c->i8_scales_signed; }
inline bool i8_logs_survivors(const nvdb_hip_ctx* c, FilterKind kind, uint32_t nb) { return i8_pipelined(c, kind, nb) && !i8_stage2_in_loop(c); }

inline hipEvent_t get_event(nvdb_hip_ctx* c, size_t idx) {
  while (c->ev_pool.size() <= idx) { hipEvent_t e; (void)hipEventCreate(&e); c->ev_pool.push_back(e); }
  return c->ev_pool[idx];
}

// ---- a filter flow: what the plans of both (SearchPlan, nvdb_plan.h; RangePlan, nvdb_range.h) share -- all that begin_filter_run reads
struct FilterPlan {
  FilterKind kind = FILTER_NONE;        // filter_kind(c) when the plan was made: the shapes below are that filter's
  bool filter = false, perm_on = false;    // filter launches follow the prologue; ... streaming tiles in permuted order
  bool prep = false, prep_inits = false;   // the prep launch runs; ... and does the per-search resets itself (option fuse), else init_search_kernel
  uint32_t cap = 0, QPB = 0, QT = 0, nq_pad = 0, prog_words = 0;
};
// ... and the flow as its launchers see it: built once by begin_filter_run, handed to every launch helper with the rows of that launch
struct FilterRun {
  hipStream_t s; FilterKind kind; bool perm;   // perm: tiles in permuted order (else identity)
  uint32_t nq, QT, nq_pad, cap; const float* thr;
  uint32_t prog_slot = 0;               // next free region of the rendezvous counters (next_prog_region)
  hipEvent_t e0 = nullptr, e1 = nullptr;   // the next timed filter launch takes them (hipExtLaunchKernelGGL: its own start / stop timestamps, no extra packets)
};
struct RowRange { uint32_t lo, hi; };
// ---- defined in one translation unit, called from another ----------------------------------------------------------
// nvdb_launch_exact.cpp
nvdb_status launch_init_search(nvdb_hip_ctx* c, hipStream_t s, uint32_t nq_pad, uint32_t prog_words);
nvdb_status launch_scan_exact(nvdb_hip_ctx* c, hipStream_t s, uint32_t row_lo, uint32_t row_hi, const float* q32, uint32_t nq, uint32_t k,
                              const float* thr, uint32_t cap, uint32_t reserve);
// q32 != nullptr (modes 0 and 2, a search that streams the int8 shadow): the bar is exact -- the select re-scores its best 2k entries
// from the corpus' own rows (c->rows, c->dtype, c->dim) against these queries and sets thr = k-th exact score - c->ebound (kernels_exact.h)
nvdb_status launch_select(nvdb_hip_ctx* c, hipStream_t s, uint32_t nq, uint32_t cap, uint32_t k, const float* slack, int mode, uint64_t* out_ids,
                          float* out_scores, uint32_t out_k, const float* q32 = nullptr);
nvdb_status launch_rescore(nvdb_hip_ctx* c, hipStream_t s, const float* q32, uint32_t nq, uint32_t cap, FinalSelect fs = FinalSelect{}, bool* fused = nullptr);
nvdb_status search_largek(nvdb_hip_ctx* c, hipStream_t s, const float* dev_q, uint32_t nq, uint32_t k, uint64_t* dev_out_ids, float* dev_out_scores,
                          uint32_t n_rows = 0, Cand* seed_cand = nullptr, uint32_t* seed_cnt = nullptr, uint32_t seed_cap = 0);
// what the any-k path and the range search's exact route share: queries per score-matrix sub-batch (QB) and per workgroup (QG) within
// largek_budget_mb, the [queries][ld] score matrix of the first n rows, the descending sort of `lists` key lists of K2 (power of two) entries
nvdb_status score_matrix_batch(nvdb_hip_ctx* c, uint32_t nq, size_t per_query_bytes, size_t held_bytes, uint32_t& QB, uint32_t& QG);
nvdb_status launch_score_matrix(nvdb_hip_ctx* c, hipStream_t s, const float* q32, uint32_t nq, float* scores, uint64_t ld, uint32_t n, uint32_t QG, bool mfma_ok);
nvdb_status launch_sort_keys(nvdb_hip_ctx* c, hipStream_t s, unsigned long long* keys, uint32_t K2, uint32_t lists);
// nvdb_launch_f16.cpp / nvdb_launch_i8.cpp
// a corpus norm as the query prep kernels get it: the developer library scales it by option debug_bound_pct (100: unchanged, x * 1.0f)
inline float prep_norm(const nvdb_hip_ctx* c, float v) {
#ifdef NVDB_HIP_DEV
  return v * (static_cast<float>(c->dbg_bound_pct) / 100.f);
#else
  (void)c;
  return v;
#endif
}
nvdb_status launch_prep_q16(nvdb_hip_ctx* c, hipStream_t s, const float* dev_q, uint32_t nq, uint32_t nq_pad, const PrepInit& pinit);
nvdb_status launch_prep_q8(nvdb_hip_ctx* c, hipStream_t s, const float* dev_q, uint32_t nq, uint32_t nq_pad, const PrepInit& pinit);
nvdb_status launch_filter_f16(nvdb_hip_ctx* c, FilterRun& run, RowRange rows);
nvdb_status launch_filter_i8(nvdb_hip_ctx* c, FilterRun& run, RowRange rows);
nvdb_status launch_boot_f16(nvdb_hip_ctx* c, FilterRun& run, uint32_t n0);      // tile maxima of rows [0, n0)
nvdb_status launch_boot_i8(nvdb_hip_ctx* c, FilterRun& run, uint32_t n0);
// nvdb_corpus.cpp
nvdb_status corpus_alloc_padded(nvdb_hip_ctx* c, uint64_t n, uint32_t dim, uint32_t dtype, void** rows, float** scales);
nvdb_status corpus_take_ownership(nvdb_hip_ctx* c, void* dev_rows, float* dev_scales, uint64_t n, uint32_t dim, uint32_t dtype, uint64_t global_row_base);
void corpus_drop(nvdb_hip_ctx* c);       // the context forgets its corpus, shadows, partition table and planes (what a load does before it loads)
// the load's own pass over the resident rows again (nvdb_hip_insert_rows, where a new row forbids a resident shadow): the shadows are freed, then norms, flags
// and whatever shadow a load of these rows would build -- with room for cap_rows rows; table, planes, options and what the context has learnt stay
nvdb_status corpus_rederive(nvdb_hip_ctx* c);
// nvdb_partitions.cpp
void parts_drop(nvdb_hip_ctx* c);        // the corpus changes: forget the partition table and the centroids (the workspace stays)
void parts_destroy(nvdb_hip_ctx* c);     // ... and free the workspace
// nvdb_search.cpp
nvdb_status ensure_q32(nvdb_hip_ctx* c, hipStream_t s, size_t qbytes);          // the host API's query buffer: qbytes + 8 rows; a new buffer starts all zero
nvdb_status zero_q32_pad(nvdb_hip_ctx* c, hipStream_t s, size_t qbytes);        // ... and the 8 rows behind this call's queries read as zeros
// prologue of search_core (whatever its route) and range_filter_pass: workspace (+ extra: a per-query word array), last filter state, init or prep, the run value
nvdb_status begin_filter_run(nvdb_hip_ctx* c, hipStream_t s, const FilterPlan& p, const float* dev_q, const float* host_q, uint32_t nq, DevBuf* extra, FilterRun& run);
nvdb_status launch_boot(nvdb_hip_ctx* c, FilterRun& run, uint32_t n0);
nvdb_status launch_filter(nvdb_hip_ctx* c, FilterRun& run, RowRange rows);
nvdb_status next_prog_region(nvdb_hip_ctx* c, FilterRun& run, uint32_t nwg, uint32_t** out);
ScatterArgs scatter_args(nvdb_hip_ctx* c, const FilterRun& run, uint32_t trows = 0);
float filter_events_ms(const nvdb_hip_ctx* c);                                 // sum over the last search's timed filter launches (ev_filter)
nvdb_status sum_candidates(nvdb_hip_ctx* c, unsigned long long* total);         // list lengths the last thresholding select left, each capped at last_cap

// ---- launching a filter kernel (nvdb_launch_f16.cpp, nvdb_launch_i8.cpp, nvdb_debug.cpp) ----------------------------
// the dynamic-LDS limit of a kernel, raised once per kernel and device
inline nvdb_status raise_lds_limit(nvdb_hip_ctx* c, const void* fn, size_t bytes) {
  if (c->lds_attr_set.count(fn)) return NVDB_OK;
  HIPCHK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
  c->lds_attr_set.insert(fn);
  return NVDB_OK;
}

// workgroups of a filter launch: one per CU, rounded down to whole groups of QT (the QT query tiles of a row stream)
inline uint32_t filter_grid(const nvdb_hip_ctx* c, uint32_t QT) {
  const uint32_t nwg = (static_cast<uint32_t>(c->num_cu) / QT) * QT;
  return nwg ? nwg : QT;
}

// xcd_aware_grid(QT, nwg) (kernels_filter.h: the predicate the kernels place themselves by): the XCD-aware mapping is active.
// Only then, and with siblings to keep in step, does the rendezvous apply
inline bool sibling_sync_grid(const nvdb_hip_ctx* c, uint32_t QT, uint32_t nwg) { return c->opt_sibling_sync && QT > 1 && QT <= 8 && xcd_aware_grid(QT, nwg); }

// rendezvous arguments of a filter kernel: counters (unused / not-yet-started slots read 0xFFFFFFFF = "far ahead"),
// period mask, allowed lead; prog == nullptr: the SYNC = false build runs
struct SyncArgs { uint32_t* prog = nullptr; uint32_t mask = 0, lead = 0; };
inline nvdb_status sibling_sync_args(nvdb_hip_ctx* c, FilterRun& run, uint32_t nwg, SyncArgs& out) {
  out = SyncArgs{};
  if (!sibling_sync_grid(c, run.QT, nwg)) return NVDB_OK;
  out.mask = static_cast<uint32_t>(c->opt_sync_every - 1);
  out.lead = static_cast<uint32_t>(c->opt_sync_lead);
  return next_prog_region(c, run, nwg, &out.prog);
}

// one filter launch as one kernel build wants it; log_waves: waves per workgroup the survivor log is sized for (0: the
// build writes no log); timed: the run's launch events attach (hipExtLaunchKernelGGL)
struct FilterGeom { uint32_t block; size_t lds; uint32_t log_waves; bool timed; };

// A DevBuf* in a kernel's argument list stands for the Hit* it holds at launch time: the survivor log may move when
// launch_filter_kernel grows it, after the caller has evaluated the arguments.
template <typename T> inline T launch_arg(T a) { return a; }
inline Hit* launch_arg(DevBuf* b) { return static_cast<Hit*>(b->p); }

template <typename... KA, typename... A>
nvdb_status launch_filter_kernel(nvdb_hip_ctx* c, FilterRun& run, void (*kern)(KA...), uint32_t nwg, const FilterGeom& g, A... args) {
  nvdb_status st;
  if ((st = raise_lds_limit(c, reinterpret_cast<const void*>(kern), g.lds))) return st;
  if (g.log_waves && (st = ensure(c, c->hitlog, static_cast<size_t>(nwg) * g.log_waves * FILTER_LOGCAP * sizeof(Hit)))) return st;
  if (g.timed) hipExtLaunchKernelGGL(kern, dim3(nwg), dim3(g.block), g.lds, run.s, std::exchange(run.e0, nullptr), std::exchange(run.e1, nullptr), 0, launch_arg(args)...);
  else kern<<<nwg, g.block, g.lds, run.s>>>(launch_arg(args)...);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

// the arguments every fp16 build starts with (rows, range, queries, thresholds, log, scatter arguments); rest: what one
// build adds (the rendezvous arguments, or filter_f16_kernel's aux word)
template <typename... KA, typename... Rest>
nvdb_status launch_filter_f16_kernel(nvdb_hip_ctx* c, FilterRun& run, RowRange rows, void (*kern)(KA...), uint32_t nwg, const FilterGeom& g, DevBuf* log,
                                     uint32_t trows, Rest... rest) {
  if (trows && (rows.hi - rows.lo) % trows) return fail(c, NVDB_ERR_INTERNAL, "fp16 filter kernel: row range is not a multiple of its tile");
  return launch_filter_kernel(c, run, kern, nwg, g, filter_rows_f16(c), rows.lo, rows.hi, static_cast<const _Float16*>(c->q16.p), run.nq, run.QT, run.thr,
                              static_cast<const float*>(c->qscale.p), static_cast<const float*>(c->qinv.p), log, scatter_args(c, run, trows), rest...);
}

// ... every int8 build (rows, scales, range, the two query planes -- the lo plane qlo_off bytes behind the hi plane --, thresholds; QT: of THIS build)
template <typename... KA, typename... Rest>
nvdb_status launch_filter_i8_kernel(nvdb_hip_ctx* c, FilterRun& run, RowRange rows, uint32_t QT, void (*kern)(KA...), uint32_t nwg, const FilterGeom& g, size_t qlo_off, Rest... rest) {
  const signed char* qhi = static_cast<const signed char*>(c->q16.p);
  return launch_filter_kernel(c, run, kern, nwg, g, filter_rows_i8(c), filter_scales_i8(c), rows.lo, rows.hi, qhi, qhi + qlo_off, run.nq, QT, run.thr,
                              static_cast<const float*>(c->qscale.p), static_cast<const float*>(c->qinv.p), rest...);
}
// ... and what the two-stage builds (filter_i8w / i8p / i8s_kernel) add: qdelta, log, scatter arguments, rendezvous, stage counts (misc[4], [5]: tiles past stage 0 / stage 1)
template <typename... KA>
nvdb_status launch_filter_i8w_kernel(nvdb_hip_ctx* c, FilterRun& run, RowRange rows, void (*kern)(KA...), uint32_t nwg, const FilterGeom& g, size_t qlo_off,
                                     uint32_t trows, const SyncArgs& sy) {
  return launch_filter_i8_kernel(c, run, rows, run.QT, kern, nwg, g, qlo_off, static_cast<const float*>(c->qdelta.p), &c->hitlog, scatter_args(c, run, trows),
                                 sy.prog, sy.mask, sy.lead, static_cast<uint32_t*>(c->misc.p) + 4);
}

}  // namespace nvdbhip
