// compact_plan_check.cpp -- the host arithmetic of the in-place compaction (nano-vectordb_amd/csrc/compact_plan.h, the code the
// entry points run) against naive loops, with exactly sized heap buffers: built with -fsanitize=address,undefined by
// tests/test_cabi_compact_cpu.py.  The slab walk is SIMULATED on an array of row numbers: a direct slab is moved in the worst
// order a launch could take (descending), a bounced slab goes through a buffer of one slab; the result must be what moving the
// live rows one at a time gives, and a direct slab's destination must end at or before its start.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "compact_plan.h"

using namespace nvdbhip;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static uint32_t state = 2463534242u;
static uint32_t next() { state = state * 1664525u + 1013904223u; return state >> 8; }

static const char* PLANE_NAMES[] = {"all live", "row 0 dead", "last row dead", "one dead per tile", "alternating", "dead block over three slabs",
                                    "random 50 %", "random 1 % live"};

static std::vector<bool> make_live(int kind, uint64_t n, uint64_t slab) {
  std::vector<bool> live(n, true);
  switch (kind) {
    case 0: break;
    case 1: live[0] = false; break;
    case 2: live[n - 1] = false; break;
    case 3: for (uint64_t t = 0; t * 64 < n; ++t) live[std::min(n - 1, t * 64 + next() % 64)] = false; break;
    case 4: for (uint64_t r = 0; r < n; ++r) live[r] = r % 2 == 0; break;
    case 5: for (uint64_t r = n / 4; r < std::min(n, n / 4 + 2 * slab + 7); ++r) live[r] = false; break;   // (touches three slabs where n has them)
    case 6: for (uint64_t r = 0; r < n; ++r) live[r] = next() % 2 == 0; break;
    default: for (uint64_t r = 0; r < n; ++r) live[r] = next() % 100 == 0; break;
  }
  return live;
}

static void check_case(int kind, uint64_t n, uint64_t slab) {
  const std::vector<bool> live = make_live(kind, n, slab);
  const uint64_t W = (n + 31) / 32, T = cp_tiles(n);
  uint32_t* plane = new uint32_t[W];                 // exactly W words, tail bits 0
  std::fill(plane, plane + W, 0u);
  for (uint64_t r = 0; r < n; ++r) if (live[r]) plane[r >> 5] |= 1u << (r & 31u);
  uint32_t* rank = new uint32_t[T + 1];              // exactly T + 1 entries
  cp_tile_ranks(plane, n, rank);

  // ranks, first dead row, the map of moving rows one at a time
  std::vector<uint32_t> old_rows;
  uint64_t first_dead = n;
  for (uint64_t r = 0; r <= n; ++r) {
    CHECK(cp_rank(plane, rank, n, r) == old_rows.size());
    if (r < n) {
      CHECK(cp_live(plane, r) == live[r]);
      if (live[r]) old_rows.push_back(static_cast<uint32_t>(r));
      else if (first_dead == n) first_dead = r;
    }
  }
  const uint64_t n_new = old_rows.size();
  CHECK(rank[T] == n_new);
  CHECK(cp_first_dead(plane, n) == first_dead);

  // the slab walk
  CHECK(cp_slab_rows_valid(static_cast<int64_t>(slab)));
  std::vector<CpSlab> slabs;
  cp_plan(plane, rank, n, slab, slabs);
  uint32_t* rows = new uint32_t[n];                  // the corpus: rows[i] = the row that stands at position i
  std::iota(rows, rows + n, 0u);
  uint32_t* bounce = new uint32_t[slab];             // one slab
  uint64_t prev_end = first_dead, moved = first_dead;
  for (const CpSlab& sl : slabs) {
    CHECK(sl.s0 >= prev_end && sl.s0 < sl.s1 && sl.s1 <= n && sl.s1 - sl.s0 <= slab);
    CHECK(sl.s0 == first_dead || sl.s0 % 64 == 0);   // every start but the walk's own is a whole tile
    CHECK(sl.d0 == moved && sl.d1 > sl.d0 && sl.d1 - sl.d0 <= sl.s1 - sl.s0 && sl.d0 <= sl.s0);
    for (uint64_t r = prev_end; r < sl.s0; ++r) CHECK(!live[r]);   // (what lies between two slabs is dead)
    CHECK(sl.direct == (sl.d1 <= sl.s0));
    std::vector<uint64_t> src;
    for (uint64_t r = sl.s0; r < sl.s1; ++r) if (live[r]) src.push_back(r);
    CHECK(src.size() == sl.d1 - sl.d0);
    if (sl.direct) {
      CHECK(sl.d1 <= sl.s0);                         // the invariant: destination range ends at or before the slab's start
      for (uint64_t i = src.size(); i-- > 0;) rows[sl.d0 + i] = rows[src[i]];
    } else {
      for (uint64_t i = 0; i < src.size(); ++i) bounce[i] = rows[src[i]];
      for (uint64_t i = src.size(); i-- > 0;) rows[sl.d0 + i] = bounce[i];
    }
    moved = sl.d1;
    prev_end = sl.s1;
  }
  for (uint64_t r = prev_end; r < n; ++r) CHECK(!live[r]);
  CHECK(first_dead == n ? slabs.empty() : moved == n_new);
  for (uint64_t j = 0; j < n_new; ++j) CHECK(rows[j] == old_rows[j]);

  // the partition table: random non-decreasing offsets from 0 to n, and two empty partitions
  std::vector<uint64_t> off{0, 0};
  for (int p = 0; p < 9; ++p) off.push_back(next() % (n + 1));
  off.push_back(n); off.push_back(n);
  std::sort(off.begin(), off.end());
  uint64_t* got = new uint64_t[off.size()];
  uint64_t* got_map = new uint64_t[off.size()];
  cp_offsets(plane, rank, n, off.data(), off.size(), got);
  cp_offsets_from_map(old_rows.data(), n_new, off.data(), off.size(), got_map);
  for (size_t p = 0; p < off.size(); ++p) {
    uint64_t want = 0;
    for (uint64_t r = 0; r < off[p]; ++r) want += live[r] ? 1u : 0u;
    CHECK(got[p] == want && got_map[p] == want);
  }

  // an index's permutation: in place, then its inverse over the source rows
  uint32_t* perm = new uint32_t[n];
  std::iota(perm, perm + n, 0u);
  for (uint64_t i = n; i > 1; --i) std::swap(perm[i - 1], perm[next() % i]);
  std::vector<uint32_t> want_perm(n_new);
  for (uint64_t j = 0; j < n_new; ++j) want_perm[j] = perm[old_rows[j]];
  uint32_t* map = new uint32_t[n_new ? n_new : 1];
  std::copy(old_rows.begin(), old_rows.end(), map);
  cp_perm(perm, map, n_new);
  for (uint64_t j = 0; j < n_new; ++j) CHECK(perm[j] == want_perm[j]);
  uint32_t* inv = new uint32_t[n];
  CHECK(cp_inverse(perm, n_new, n, inv));
  uint64_t placed = 0;
  for (uint64_t r = 0; r < n; ++r)
    if (inv[r] != 0xFFFFFFFFu) { CHECK(inv[r] < n_new && perm[inv[r]] == r); ++placed; }
  CHECK(placed == n_new);
  if (n_new >= 2) { perm[1] = perm[0]; CHECK(!cp_inverse(perm, n_new, n, inv)); }   // a row named twice

  std::printf("n=%llu slab=%llu %s: %llu live, %zu slabs checked\n", static_cast<unsigned long long>(n), static_cast<unsigned long long>(slab),
              PLANE_NAMES[kind], static_cast<unsigned long long>(n_new), slabs.size());
  delete[] plane; delete[] rank; delete[] rows; delete[] bounce; delete[] got; delete[] got_map; delete[] perm; delete[] map; delete[] inv;
}

int main() {
  for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 4097ull})
    for (uint64_t slab : {64ull, 4096ull})
      for (int kind = 0; kind < 8; ++kind) check_case(kind, n, slab);
  CHECK(!cp_slab_rows_valid(0) && !cp_slab_rows_valid(63) && !cp_slab_rows_valid(100) && !cp_slab_rows_valid((1ll << 24) + 64) && cp_slab_rows_valid(1ll << 24));
  std::printf(failures ? "%d FAILURES\n" : "OK\n", failures);
  return failures ? 1 : 0;
}
