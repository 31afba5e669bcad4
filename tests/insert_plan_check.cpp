// insert_plan_check.cpp -- the host arithmetic of the in-place insertion (nano-vectordb_amd/csrc/insert_plan.h, the code the entry
// points run) against a naive model, with exactly sized heap buffers: built with -fsanitize=address,undefined by
// tests/test_cabi_insert_cpu.py.  The model: old rows (tagged with their partition) followed by the new rows (tagged with
// part_of), put into the new order by std::stable_sort on the partition.  The slab walk is SIMULATED on an array of row numbers: a
// direct slab must write at or beyond its own end and is moved in the worst order a launch could take (ascending), a bounced slab
// goes through a buffer of one slab; the result must be the model's order.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "insert_plan.h"

using namespace nvdbhip;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static uint32_t state = 2463534242u;
static uint32_t next() { state = state * 1664525u + 1013904223u; return state >> 8; }

static const char* PATTERN_NAMES[] = {"one row at the end, no part_of", "one row into partition 0", "one row into partition 1", "one row into every partition",
                                      "all rows into partition 0", "65 rows into one middle partition", "random part_of", "all rows into the last partition",
                                      "a shift beyond a slab"};
constexpr int NPATTERNS = 9;

// a table over n rows with empty partitions at the start, in the middle and at the end
static std::vector<uint64_t> make_table(uint64_t n, bool single) {
  if (single) return {0, n};
  std::vector<uint64_t> off{0, 0};
  for (int p = 0; p < 7; ++p) off.push_back(next() % (n + 1));
  off.push_back(off[3]);                             // (an empty partition in the middle once sorted)
  off.push_back(n); off.push_back(n);
  std::sort(off.begin(), off.end());
  return off;
}

static void check_case(int pattern, uint64_t n, uint64_t slab, bool single) {
  const std::vector<uint64_t> off = make_table(n, single);
  const uint32_t nparts = static_cast<uint32_t>(off.size() - 1);
  std::vector<uint32_t> part_of;
  bool null_part_of = false;
  switch (pattern) {
    case 0: part_of.assign(1, nparts - 1); null_part_of = true; break;
    case 1: part_of.assign(1, 0); break;
    case 2: part_of.assign(1, std::min(1u, nparts - 1)); break;
    case 3: for (uint32_t p = 0; p < nparts; ++p) part_of.push_back(p); break;
    case 4: part_of.assign(100, 0); break;
    case 5: part_of.assign(65, nparts / 2); break;
    case 6: for (int i = 0; i < 333; ++i) part_of.push_back(next() % nparts); break;
    case 7: part_of.assign(70, nparts - 1); break;
    default: part_of.assign(2 * slab + 5, std::min(1u, nparts - 1)); break;
  }
  const uint64_t m = part_of.size();
  uint32_t* po = new uint32_t[m];                    // exactly m entries
  std::copy(part_of.begin(), part_of.end(), po);
  uint64_t* new_rows = new uint64_t[m];
  InsPlan pl;
  CHECK(ins_plan(off.data(), nparts, null_part_of ? nullptr : po, m, pl, new_rows));
  CHECK(pl.n == n && pl.m == m && pl.cnt.size() == nparts && pl.shift.size() == nparts && pl.off_new.size() == nparts + 1u);

  // the model
  struct Ent { uint32_t part; uint64_t id; };        // id: old row, or n + i for new row i
  std::vector<Ent> model;
  for (uint64_t r = 0; r < n; ++r) {
    uint32_t p = 0;
    while (!(off[p] <= r && r < off[p + 1])) ++p;
    CHECK(ins_list(off.data(), nparts, r) == p);
    model.push_back(Ent{p, r});
  }
  for (uint64_t i = 0; i < m; ++i) model.push_back(Ent{po[i], n + i});
  std::stable_sort(model.begin(), model.end(), [](const Ent& a, const Ent& b) { return a.part < b.part; });
  std::vector<uint64_t> where(n + m);
  for (uint64_t j = 0; j < n + m; ++j) where[model[j].id] = j;
  for (uint64_t i = 0; i < m; ++i) CHECK(new_rows[i] == where[n + i]);
  for (uint64_t r = 0; r < n; ++r) CHECK(r + ins_shift_at(pl, r) == where[r]);
  for (uint32_t p = 0; p <= nparts; ++p) {
    uint64_t below = 0;
    for (const Ent& e : model) below += e.part < p ? 1u : 0u;
    CHECK(pl.off_new[p] == below);
  }
  uint64_t first_moved = n;
  for (uint64_t r = 0; r < n; ++r) if (where[r] != r) { first_moved = r; break; }
  CHECK(pl.lo <= first_moved);                       // nothing below lo moves
  for (uint64_t r = 0; r < pl.lo; ++r) CHECK(where[r] == r);

  // the walk, in place in an array of exactly n + m rows
  std::vector<InsSlab> slabs;
  ins_slabs(pl, slab, slabs);
  uint64_t* rows = new uint64_t[n + m];
  std::iota(rows, rows + n, 0ull);
  std::fill(rows + n, rows + n + m, ~0ull);
  uint64_t* bounce = new uint64_t[slab];             // one slab
  uint64_t top = n;
  for (const InsSlab& sl : slabs) {
    CHECK(sl.s1 == top && sl.s0 < sl.s1 && sl.s1 - sl.s0 <= slab && sl.s0 >= pl.lo);
    const uint64_t shift_min = ins_shift_at(pl, sl.s0);
    CHECK(sl.direct == (sl.s0 + shift_min >= sl.s1));
    if (sl.direct) {
      for (uint64_t r = sl.s0; r < sl.s1; ++r) {     // ascending: an overlap would overwrite a row before it is read
        CHECK(r + ins_shift_at(pl, r) >= sl.s1);
        rows[r + ins_shift_at(pl, r)] = rows[r];
      }
    } else {
      for (uint64_t r = sl.s0; r < sl.s1; ++r) bounce[r - sl.s0] = rows[r];
      for (uint64_t r = sl.s0; r < sl.s1; ++r) rows[r + ins_shift_at(pl, r)] = bounce[r - sl.s0];
    }
    top = sl.s0;
  }
  CHECK(top == pl.lo || (slabs.empty() && pl.lo == n));
  for (uint64_t i = 0; i < m; ++i) rows[new_rows[i]] = n + i;
  for (uint64_t j = 0; j < n + m; ++j) CHECK(rows[j] == model[j].id);

  // an index's permutation and its inverse
  std::vector<uint32_t> perm(n), inv;
  std::iota(perm.begin(), perm.end(), 0u);
  for (uint64_t i = n; i > 1; --i) std::swap(perm[i - 1], perm[next() % i]);
  const std::vector<uint32_t> perm0 = perm;
  if (pattern % 2) { inv.resize(n); for (uint64_t j = 0; j < n; ++j) inv[perm[j]] = static_cast<uint32_t>(j); }
  perm.shrink_to_fit();
  ins_perm(perm, inv, pl, new_rows, n);
  CHECK(perm.size() == n + m);
  for (uint64_t j = 0; j < n + m; ++j) CHECK(perm[j] == (model[j].id < n ? perm0[model[j].id] : static_cast<uint32_t>(model[j].id)));
  if (pattern % 2) {
    CHECK(inv.size() == n + m);
    for (uint64_t j = 0; j < n + m; ++j) CHECK(inv[perm[j]] == j);
  } else {
    CHECK(inv.empty());
  }

  // an entry of part_of beyond the table
  po[m - 1] = nparts;
  InsPlan bad;
  CHECK(!ins_plan(off.data(), nparts, po, m, bad, nullptr));

  std::printf("n=%llu slab=%llu %s, %u partitions: %llu new rows, %zu slabs checked\n", static_cast<unsigned long long>(n), static_cast<unsigned long long>(slab),
              PATTERN_NAMES[pattern], nparts, static_cast<unsigned long long>(m), slabs.size());
  delete[] po; delete[] new_rows; delete[] rows; delete[] bounce;
}

int main() {
  for (uint64_t n : {1ull, 31ull, 32ull, 33ull, 63ull, 64ull, 65ull, 4097ull})
    for (uint64_t slab : {64ull, 4096ull})
      for (int pattern = 0; pattern < NPATTERNS; ++pattern) {
        check_case(pattern, n, slab, false);
        check_case(pattern, n, slab, true);
      }
  // the capacity rule
  CHECK(ins_capacity(100, 1, 100, 50) == 150 && ins_capacity(100, 1, 100, 0) == 101 && ins_capacity(100, 100, 100, 50) == 200);
  CHECK(ins_capacity(10, 1, 100, 400) == 500 && ins_capacity(4000000000ull, 1, 4000000000ull, 50) == 0xFFFFFFF0ull);
  CHECK(ins_growth_pct_valid(0) && ins_growth_pct_valid(400) && !ins_growth_pct_valid(-1) && !ins_growth_pct_valid(401));
  std::printf(failures ? "%d FAILURES\n" : "OK\n", failures);
  return failures ? 1 : 0;
}
