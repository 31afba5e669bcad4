// nvdb_plan.h -- everything one flat search decides before its first launch (DESIGN.md "pipeline"): route, list capacity,
// which filter streams, query tiling, bootstrap, chunk boundaries.  plan_search is pure integer arithmetic over corpus facts
// and options: no HIP call and a const context, so tests/test_search_plan_cpu.py pins it without a device (nvdb_hip_debug_plan).
// Which filter streams is chosen once (filter_kind, nvdb_ctx.h) and carried in the plan: the shape facts plan_search shares with
// the launchers (tile rows, queries per workgroup, which int8 build logs; nvdb_ctx.h) take it as an argument, here and there.
#pragma once
#include "nvdb_ctx.h"

namespace nvdbhip {

enum Route : uint32_t { ROUTE_EXACT = 1, ROUTE_FILTER = 2, ROUTE_ANYK = 3 };   // the values of nvdb_hip_scan_stats::path
// how the filter route gets its first thresholds: tile maxima on the matrix cores (entries discarded, rows streamed again),
// rows [0, r0) on the exact kernel, or (64 < k) the k best of rows [0, r0) from the any-k machinery seeding the lists
enum Boot : uint32_t { BOOT_MFMA = 0, BOOT_EXACT_CHUNK = 1, BOOT_ANYK_SEEDED = 2 };

// filter == (route == ROUTE_FILTER); prep without filter: the any-k route when only the bootstrap rules sent a 64 < k search there (its fused init does the per-search resets)
struct SearchPlan : FilterPlan {
  const char* error = nullptr;          // message of the NVDB_ERR_UNSUPPORTED plan_search returned
  Route route = ROUTE_EXACT;
  bool k_wide = false;                  // k beyond the wavefront lists' 64 entries
  uint32_t k_eff = 0;
  uint32_t head = 0;                    // exact route: rows of the prescan (0: one scan)
  // filter route
  bool padded = false;
  Boot boot = BOOT_MFMA;
  uint32_t tile_rows = 0, n_al = 0, growth = 0, boot_tiles = 0, boot_rows = 0;
  uint32_t r0 = 0;                      // rows the exact / seeded bootstrap covers; the chunks tile [r0, n_al)
  uint64_t size0 = 0;                   // rows of the first chunk; every later one covers (growth - 1) x the rows before it
  bool tail_exact = false;              // ragged tail [n_al, n) of an adopted corpus on the exact kernel
};

// end of the chunk that starts at row r
inline uint32_t chunk_end(const SearchPlan& p, uint32_t r) {
  const uint64_t size = r == p.r0 ? p.size0 : static_cast<uint64_t>(r) * (p.growth - 1);
  return static_cast<uint32_t>(std::min<uint64_t>(p.n_al, r + size));
}

inline nvdb_status plan_search(const nvdb_hip_ctx& ctx, uint32_t nq, uint32_t k, int force_path, uint32_t cap_override, SearchPlan& p) {
  const nvdb_hip_ctx* c = &ctx;
  p = SearchPlan{};
  // (a shadow context: the shadow unless it was switched off or has overflowed on this corpus); tiles, queries per workgroup, growth, bootstrap below are that filter's
  const FilterKind kind = p.kind = filter_kind(c);
  const uint32_t n = static_cast<uint32_t>(c->n);
  const uint32_t k_eff = p.k_eff = static_cast<uint32_t>(std::min<uint64_t>(k, c->n));
  int path = force_path ? force_path : static_cast<int>(c->opt_path);
  if (path == 0) path = (filter_supported(c) && nq >= c->opt_min_filter_batch && c->n >= 4ull * c->opt_chunk0) ? 2 : 1;
  if (path == 2 && !filter_supported(c)) {
    p.error = "MFMA filter path needs an fp16/fp32 corpus with dim <= 3072 or an int8 corpus with dim <= 1536";
    return NVDB_ERR_UNSUPPORTED;
  }
  uint32_t cap = cap_override ? cap_override : c->opt_cap > 0 ? static_cast<uint32_t>(c->opt_cap) : std::max<uint32_t>(c->cap_hint, nq <= 64 ? SELECT_MAX_CAP : 2048u);
  cap = std::min(cap, SELECT_MAX_CAP);
  if (cap < 4 * k_eff) cap = std::min<uint32_t>(SELECT_MAX_CAP, 4 * k_eff);
  // 64 < k <= 1024 on the filter path (its kernels do not depend on k; the lists do): the longest lists, a bootstrap over
  // 8k tile maxima and chunks small enough that k * (growth - 1) new survivors + the k kept ones + the error band fit.
  // Anything else beyond the wavefront lists' 64 entries takes the any-k path.
  const bool k_wide = p.k_wide = k_eff > WAVE_KMAX;
  // dims whose kernels have no MFMA bootstrap build (768 < dim): an EXACT bootstrap over the first 8k tiles' rows on the any-k
  // machinery (score matrix of the sample -> radix select -> the k best seed the lists), then the filter streams the rest
  const bool wide_exact_boot = k_wide && path == 2 && force_path != 1 && k_eff <= FILTER_KMAX && c->fdim > 768 &&
                               c->n >= 4ull * FILTER_ROWS * 8 * k_eff;
  const bool wide_on_filter = wide_exact_boot || (k_wide && path == 2 && force_path != 1 && k_eff <= FILTER_KMAX && c->opt_mfma_boot &&
                              c->fdim <= 768 && c->n >= 2ull * FILTER_ROWS * 8 * k_eff);
  if (wide_on_filter) cap = SELECT_MAX_CAP;
  p.cap = cap;
  p.QPB = filter_qpb(c, kind, nq);
  p.QT = (nq + p.QPB - 1) / p.QPB;
  p.nq_pad = p.QT * p.QPB;
  // one region of sibling-rendezvous counters per filter launch of this search, all reset by the init kernel
  p.prog_words = PROG_SLOTS * static_cast<uint32_t>(c->num_cu) * 8u;
  // The filter path's prep launch does the per-search resets itself (and, for the host API's small calls, reads the queries
  // straight from pinned host memory); the exact and any-k paths have no prep launch: init_search_kernel, queries copied.
  p.prep = path == 2 && !(k_wide && !wide_on_filter);
  p.prep_inits = c->opt_fuse && p.prep;
  if (k_wide && !wide_on_filter) { p.route = ROUTE_ANYK; return NVDB_OK; }   // (scores -> radix select -> sort)
  if (path == 1) {
    // Two launches on big corpora: every workgroup of the scan starts with empty top-k lists, and until a list has warmed up
    // nearly every tile takes the serial insertion path (~0.65 ms per round at 64 queries: profiles/r04_exact_wgs_sweep.txt).  So the
    // first 1/64 of the rows is scanned on its own, a select turns it into the exact k-th best score per query (slack 0: the k best
    // stay in the list), and the scan of the other 63/64 starts with that bar: a row reaches a list only if it beats it.  Same lists,
    // same final select, same results.  (Only where the MFMA scan runs: more than 8 queries; the VALU kernel's lists warm up per wave.)
    p.head = (c->opt_exact_prescan && nq > 8 && n >= (1u << 20)) ? std::max<uint32_t>(1u << 15, (n >> 6) & ~255u) : 0u;
    return NVDB_OK;
  }
  // ---- the filter route ----
  // Whole tiles: the padded rows of a corpus this library allocated are dropped when the wave files its survivors; for an
  // adopted corpus the ragged tail goes to the exact kernel.  Chunk boundaries are whole tiles of the streaming kernel.
  p.padded = corpus_padded(c, kind);
  const uint32_t tile_rows = p.tile_rows = filter_tile_rows(c, kind, nq);
  const uint32_t n_al = p.n_al = p.padded ? (n + tile_rows - 1) / tile_rows * tile_rows : n / tile_rows * tile_rows;
  // chunk i covers (growth-1) x the rows seen before it.  fp16: 8 (flat between 4 and 8).  int8 batches > 128: 3 --
  // tighter thresholds earlier mean fewer tiles for which the two-stage kernel needs the lo plane, and a tile costs
  // what its slowest wave costs (profiles/r01d_i8_growth_sweep.txt)
  // (with the first-stage survivors finished after the stream a flagged value costs little: 6 and a 1024-tile bootstrap on big
  // corpora, profiles/r02_i8_boot_growth_sweep.txt; the in-loop second stage wants 3)
  const bool i8_big = i8_two_stage(c, kind) && nq > 128 && c->fdim <= 768;
  const bool i8_log = i8_big && i8_logs_survivors(c, kind, filter_nb(c, kind, nq)) && !c->opt_i8_waves8 && c->n >= 64ull * FILTER_ROWS * 1024;
  uint64_t growth = c->opt_growth > 0 ? static_cast<uint64_t>(c->opt_growth) : (i8_log ? 6u : i8_big ? 3u : 8u);
  if (k_wide) growth = std::max<uint64_t>(2, std::min<uint64_t>(growth, cap / (3ull * k_eff)));     // k * (growth - 1) + k + band <= cap
  p.growth = static_cast<uint32_t>(growth);
  // T tile maxima with T >= 8k: their k-th largest is then close to the k-th best of the 32*T rows (with T == k it
  // would be the smallest tile maximum, a uselessly weak threshold)
  uint32_t boot_tiles = std::max<uint32_t>(64u, 8u * k_eff);
  if (c->opt_boot_tiles > 0) boot_tiles = std::max<uint32_t>(boot_tiles, std::min<uint32_t>(static_cast<uint32_t>(c->opt_boot_tiles), cap));
  else if (i8_log && !k_wide) boot_tiles = std::max<uint32_t>(boot_tiles, std::min<uint32_t>(1024u, cap));
  else if (!k_wide) {
    // A bootstrap of up to 256 tiles that saves a whole chunk (a filter launch + its select, ~12 us) pays for itself; a larger
    // bootstrap that saves none does not (profiles/r04_boot_tiles_sweep.txt: 500K rows 3 -> 2 chunks -9 us, 2.9M rows 4 -> 3 chunks
    // -14..-28 us; 1M / 10M rows, where 256 tiles save nothing: +0.5..2 %).  So: the smallest bootstrap <= 256 tiles with which the
    // chunks (each `growth` x the rows before it) reach the corpus one launch earlier.
    uint64_t reach = static_cast<uint64_t>(FILTER_ROWS) * boot_tiles, per = 1;
    uint32_t J = 0;
    while (reach < n) { reach *= growth; per *= growth; ++J; }
    if (J >= 2) {
      per /= growth;                                                             // growth^(J-1)
      uint64_t need = (static_cast<uint64_t>(n) + per * FILTER_ROWS - 1) / (per * FILTER_ROWS);
      need = (need + 3) & ~3ull;                                                 // chunk boundaries stay multiples of the 64-row tiles whatever the growth
      if (need > boot_tiles && need <= 256 && need <= cap) boot_tiles = static_cast<uint32_t>(need);
    }
  }
  p.boot_tiles = boot_tiles;
  p.boot_rows = FILTER_ROWS * boot_tiles;
  const bool mfma_boot = c->opt_mfma_boot && n >= p.boot_rows && boot_tiles >= k_eff && boot_tiles <= cap &&
                         c->fdim <= 768;    // no bootstrap build of the 16-row-tile fp16 kernel / the 32-query int8 kernel: exact bootstrap chunk
  // 64 < k on the filter path needs the MFMA bootstrap (the exact bootstrap chunk's wavefront lists hold 64 entries) or the
  // seeded one; e.g. option boot_tiles larger than the corpus: the any-k path takes the search instead, after the prep launch
  if (k_wide && !mfma_boot && !wide_exact_boot) { p.route = ROUTE_ANYK; return NVDB_OK; }
  p.route = ROUTE_FILTER; p.filter = true;
  p.boot = mfma_boot ? BOOT_MFMA : k_wide ? BOOT_ANYK_SEEDED : BOOT_EXACT_CHUNK;
  // permuted tile order needs the bootstrap whose entries are discarded (the exact bootstrap chunk keeps rows [0, r0))
  p.perm_on = c->opt_tile_permute && mfma_boot;
  if (mfma_boot) p.size0 = static_cast<uint64_t>(p.boot_rows) * growth;
  else {
    // bootstrap chunk [0, r0): a whole number of the streaming kernel's tiles
    p.r0 = std::min<uint32_t>(n_al, (static_cast<uint32_t>(k_wide ? FILTER_ROWS * 8u * k_eff : c->opt_chunk0) + tile_rows - 1) / tile_rows * tile_rows);
    if (p.r0 > n) p.r0 = n / tile_rows * tile_rows;
    p.size0 = static_cast<uint64_t>(p.r0) * (growth - 1);
  }
  p.tail_exact = n_al < n;
  return NVDB_OK;
}

}  // namespace nvdbhip
