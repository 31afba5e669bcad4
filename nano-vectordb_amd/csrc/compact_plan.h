// compact_plan.h -- the host arithmetic of the in-place compaction (nvdb_compact.cpp, DESIGN.md section 4 "Compaction"): the rank
// of a row (live rows below it), where the walk starts, how the corpus is cut into slabs and which of them may be moved directly,
// the partition table and an index's permutation after the move.  Plain C++ with no HIP call in it, so that the sanitizer build
// of tests/compact_plan_check.cpp compiles the very code the entry points run (as masked_plan.h, parts_worklist.h).
//
// A plane over n rows is rm_words(n) words (row_mask.h), its tail bits 0.  tile_rank has ceil(n / 64) + 1 entries: tile_rank[t] =
// live rows below row 64 t, the last entry the plane's live count.  The move is stable, so the live rows of source rows [s0, s1)
// land in [rank(s0), rank(s1)), at or below where they were.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace nvdbhip {

constexpr uint32_t CP_TILE_ROWS = 64;
constexpr uint64_t CP_SLAB_ROWS_MAX = 1ull << 24;      // a slab is one launch of one workgroup per tile

inline bool cp_slab_rows_valid(int64_t v) { return v >= CP_TILE_ROWS && static_cast<uint64_t>(v) <= CP_SLAB_ROWS_MAX && v % CP_TILE_ROWS == 0; }

inline uint64_t cp_tiles(uint64_t n) { return (n + CP_TILE_ROWS - 1) / CP_TILE_ROWS; }

inline bool cp_live(const uint32_t* plane, uint64_t r) { return (plane[r >> 5] >> (r & 31u)) & 1u; }

// the reference of the device's rank kernels: tile_rank[0 .. cp_tiles(n)], written completely
inline void cp_tile_ranks(const uint32_t* plane, uint64_t n, uint32_t* tile_rank) {
  const uint64_t W = (n + 31) / 32, T = cp_tiles(n);
  uint32_t run = 0;
  for (uint64_t t = 0; t < T; ++t) {
    tile_rank[t] = run;
    run += static_cast<uint32_t>(__builtin_popcount(plane[2 * t]));
    if (2 * t + 1 < W) run += static_cast<uint32_t>(__builtin_popcount(plane[2 * t + 1]));
  }
  tile_rank[T] = run;
}

// live rows below row r, r <= n
inline uint64_t cp_rank(const uint32_t* plane, const uint32_t* tile_rank, uint64_t n, uint64_t r) {
  if (r >= n) return tile_rank[cp_tiles(n)];
  uint64_t run = tile_rank[r / CP_TILE_ROWS];
  const uint64_t w0 = (r / CP_TILE_ROWS) * 2, w = r >> 5;
  if (w > w0) run += static_cast<uint64_t>(__builtin_popcount(plane[w0]));
  if (r & 31u) run += static_cast<uint64_t>(__builtin_popcount(plane[w] & ((1u << (r & 31u)) - 1u)));
  return run;
}

// the first dead row; n: every row is live
inline uint64_t cp_first_dead(const uint32_t* plane, uint64_t n) {
  const uint64_t W = (n + 31) / 32;
  for (uint64_t w = 0; w < W; ++w) {
    const uint32_t dead = ~plane[w];
    if (!dead) continue;
    const uint64_t r = w * 32 + static_cast<uint64_t>(__builtin_ctz(dead));
    return r < n ? r : n;                            // (the tail bits of the last word are 0 without naming a row)
  }
  return n;
}

// One slab: source rows [s0, s1) whose live rows land in [d0, d1).  direct: d1 <= s0 -- one launch may read the slab and write
// its destination, they do not overlap.  Otherwise the slab is gathered into the bounce buffer and copied from there.
struct CpSlab { uint64_t s0, s1, d0, d1; bool direct; };

// The walk: ascending slabs from the first dead row (everything before it stays where it is).  The first slab starts AT that row,
// every later one on a multiple of slab_rows above its tile, so that all starts but the first are whole tiles; slabs without a
// live row are left out.  slab_rows: a multiple of 64.
inline void cp_plan(const uint32_t* plane, const uint32_t* tile_rank, uint64_t n, uint64_t slab_rows, std::vector<CpSlab>& out) {
  out.clear();
  const uint64_t first = cp_first_dead(plane, n);
  if (first >= n) return;
  const uint64_t origin = first / CP_TILE_ROWS * CP_TILE_ROWS;
  for (uint64_t s0 = first, i = 1; s0 < n; ++i) {
    const uint64_t s1 = std::min(n, origin + i * slab_rows);
    const uint64_t d0 = cp_rank(plane, tile_rank, n, s0), d1 = cp_rank(plane, tile_rank, n, s1);
    if (d1 > d0) out.push_back(CpSlab{s0, s1, d0, d1, d1 <= s0});
    s0 = s1;
  }
}

// the partition table after the move: offsets'[p] = live rows below offsets[p] (in place is fine)
inline void cp_offsets(const uint32_t* plane, const uint32_t* tile_rank, uint64_t n, const uint64_t* offsets, uint64_t count, uint64_t* out) {
  for (uint64_t p = 0; p < count; ++p) out[p] = cp_rank(plane, tile_rank, n, offsets[p]);
}

// the same from the map alone (old_rows[j] = old row of new row j, ascending): entries below offsets[p]
inline void cp_offsets_from_map(const uint32_t* old_rows, uint64_t n_new, const uint64_t* offsets, uint64_t count, uint64_t* out) {
  for (uint64_t p = 0; p < count; ++p)
    out[p] = offsets[p] > 0xFFFFFFFFull ? n_new
                                         : static_cast<uint64_t>(std::lower_bound(old_rows, old_rows + n_new, static_cast<uint32_t>(offsets[p])) - old_rows);
}

// an index's permutation after the move, in place: perm[j] = perm[old_rows[j]], j < n_new.  old_rows[j] >= j and ascending, so an
// entry is read before the walk overwrites it
inline void cp_perm(uint32_t* perm, const uint32_t* old_rows, uint64_t n_new) {
  for (uint64_t j = 0; j < n_new; ++j) perm[j] = perm[old_rows[j]];
}

// inv[perm[j]] = j over the n_new positions that are left, 0xFFFFFFFF for a source row without a position; inv: n_src entries.
// false (inv partly written): an entry of perm is >= n_src or named twice
inline bool cp_inverse(const uint32_t* perm, uint64_t n_new, uint64_t n_src, uint32_t* inv) {
  for (uint64_t r = 0; r < n_src; ++r) inv[r] = 0xFFFFFFFFu;
  for (uint64_t j = 0; j < n_new; ++j) {
    if (perm[j] >= n_src || inv[perm[j]] != 0xFFFFFFFFu) return false;
    inv[perm[j]] = static_cast<uint32_t>(j);
  }
  return true;
}

}  // namespace nvdbhip
