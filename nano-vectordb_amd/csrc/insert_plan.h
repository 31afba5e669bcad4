// insert_plan.h -- the host arithmetic of the in-place insertion (nvdb_insert.cpp, DESIGN.md section 4 "Insertion"): how many new rows
// every partition receives and by how much its old rows shift, the new partition table, where every new row lands, how the rows that
// move are cut into DESCENDING slabs and which of them may be moved directly, an index's permutation after the move, the capacity
// rule.  Plain C++ with no HIP call in it, so that the sanitizer build of tests/insert_plan_check.cpp compiles the very code the entry
// points run (as compact_plan.h, masked_plan.h, parts_worklist.h).
//
// The move is the compaction's, turned round: new rows join the END of their partition, so old row r of partition p becomes
// r + shift[p], shift[p] = new rows in partitions < p -- an order-preserving map whose shifts never decrease with the row.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace nvdbhip {

constexpr uint32_t INS_TILE_ROWS = 64;

inline bool ins_growth_pct_valid(int64_t v) { return v >= 0 && v <= 400; }

// rows the owned arrays get when n + m no longer fits capacity `cap`: max(n + m, cap * (100 + pct) / 100), never beyond what a
// corpus may hold (unless n + m itself asks for it: the caller has checked that)
inline uint64_t ins_capacity(uint64_t n, uint64_t m, uint64_t cap, uint64_t pct) {
  const uint64_t grown = std::min<uint64_t>(cap * (100 + pct) / 100, 0xFFFFFFF0ull);
  return std::max(n + m, grown);
}

// The table the plan works on is never empty: a corpus without one is a single partition [0, n).
struct InsPlan {
  std::vector<uint64_t> off_old, off_new;          // nparts + 1 each
  std::vector<uint64_t> cnt, shift;                // nparts each: new rows of the partition, new rows in the partitions before it
  uint64_t n = 0, m = 0;
  uint64_t lo = 0;                                 // the first old row that moves (the end of the first partition that receives rows); n: none
};

// part_of == nullptr: every new row joins the last partition.  false: an entry of part_of is >= nparts (nothing of `out` is to be used).
// out_new_rows (optional, m entries): the new local row of inserted row i -- rows that name the same partition keep the order of i
inline bool ins_plan(const uint64_t* offsets, uint32_t nparts, const uint32_t* part_of, uint64_t m, InsPlan& out, uint64_t* out_new_rows) {
  out.off_old.assign(offsets, offsets + nparts + 1);
  out.cnt.assign(nparts, 0);
  out.shift.assign(nparts, 0);
  out.off_new.assign(static_cast<size_t>(nparts) + 1, 0);
  out.n = offsets[nparts];
  out.m = m;
  if (part_of) {
    for (uint64_t i = 0; i < m; ++i) {
      if (part_of[i] >= nparts) return false;
      ++out.cnt[part_of[i]];
    }
  } else {
    out.cnt[nparts - 1] = m;
  }
  uint64_t run = 0;
  out.lo = out.n;
  for (uint32_t p = 0; p < nparts; ++p) {
    out.shift[p] = run;
    out.off_new[p] = offsets[p] + run;
    if (out.cnt[p] && out.lo == out.n && run == 0) out.lo = offsets[p + 1];
    run += out.cnt[p];
  }
  out.off_new[nparts] = out.n + run;
  if (out_new_rows) {
    // the first free position of every partition's gap: behind its old rows
    std::vector<uint64_t> next(nparts);
    for (uint32_t p = 0; p < nparts; ++p) next[p] = out.off_new[p + 1] - out.cnt[p];
    for (uint64_t i = 0; i < m; ++i) out_new_rows[i] = next[part_of ? part_of[i] : nparts - 1]++;
  }
  return true;
}

// the partition of old row pos < n: the last p with off_old[p] <= pos (empty partitions are skipped by construction)
inline uint32_t ins_list(const uint64_t* off, uint32_t nparts, uint64_t pos) {
  uint32_t lo = 0, hi = nparts;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}
inline uint64_t ins_shift_at(const InsPlan& pl, uint64_t pos) {
  return pl.shift[ins_list(pl.off_old.data(), static_cast<uint32_t>(pl.cnt.size()), pos)];
}

// One slab: old rows [s0, s1), every one of which goes to its row + shift.  direct: s0 + (the smallest shift of the slab, that of
// s0) >= s1 -- one launch may read the slab and write its destinations, they do not overlap.  Otherwise the slab is copied into the
// bounce buffer and spread from there.
struct InsSlab { uint64_t s0, s1; bool direct; };

// The walk: DESCENDING slabs of at most slab_rows rows from the last row down to pl.lo (rows below it stay where they are).
// Destinations lie above sources and slabs descend, so no row is overwritten before it has been read.
inline void ins_slabs(const InsPlan& pl, uint64_t slab_rows, std::vector<InsSlab>& out) {
  out.clear();
  for (uint64_t s1 = pl.n; s1 > pl.lo;) {
    const uint64_t s0 = s1 - pl.lo > slab_rows ? s1 - slab_rows : pl.lo;
    out.push_back(InsSlab{s0, s1, s0 + ins_shift_at(pl, s0) >= s1});
    s1 = s0;
  }
}

// An index's permutation after the move: perm'[j + shift] = perm[j] for the old positions, perm'[new_rows[i]] = first_id + i;
// perm comes with its old n entries and leaves with n + m.  inv (an index's inverse, first_id entries, or empty: not built) is
// extended and rewritten the same way
inline void ins_perm(std::vector<uint32_t>& perm, std::vector<uint32_t>& inv, const InsPlan& pl, const uint64_t* new_rows, uint64_t first_id) {
  const uint32_t nparts = static_cast<uint32_t>(pl.cnt.size());
  perm.resize(pl.n + pl.m);
  for (uint32_t p = nparts; p-- > 0;) {            // descending: an entry is read before the walk overwrites it
    if (!pl.shift[p]) break;                       // (shifts never decrease with p: everything below stays)
    for (uint64_t j = pl.off_old[p + 1]; j-- > pl.off_old[p];) perm[j + pl.shift[p]] = perm[j];
  }
  for (uint64_t i = 0; i < pl.m; ++i) perm[new_rows[i]] = static_cast<uint32_t>(first_id + i);
  if (!inv.empty()) {
    inv.resize(first_id + pl.m);
    for (uint64_t r = 0; r < inv.size(); ++r) inv[r] = 0xFFFFFFFFu;
    for (uint64_t j = 0; j < perm.size(); ++j) inv[perm[j]] = static_cast<uint32_t>(j);
  }
}

}  // namespace nvdbhip
