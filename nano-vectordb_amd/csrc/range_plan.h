// range_plan.h -- the host-side arithmetic of the range searches: where the partition range scan (nvdb_range_parts.cpp) cuts a
// batch into query sub-batches under the candidate-block budget, and what the downloaded per-query counts become on both the
// probe path and the flat search's exact route (range_tail, nvdb_range.h) -- offsets / lims, the power-of-two key slabs, the runs
// of slabs that are collected, sorted and emitted together, and a run's descriptors.  Plain C++ with no HIP in it, so that the
// sanitizer build of tests/range_plan_check.cpp compiles the very code the entry points run.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace nvdbhip {

// a launch set's candidate blocks hold fewer entries than this: positions inside them are 32-bit, 0xFFFFFFFF is never one
constexpr uint64_t RP_MAX_ENTRIES = 0xFFFFFFFFull;
// the longest slab (a count rounded up to a power of two) whose length still fits 32 bits
constexpr uint64_t RP_MAX_SLAB = 1ull << 31;

// block[q] = candidate entries query q's block takes (the rows of its probed union).  Returns the end q1 of the sub-batch that
// starts at q0: the longest run of consecutive queries whose blocks together stay within budget_entries and below RP_MAX_ENTRIES;
// a single query is taken whatever the budget says (its block cannot be cut).  q1 == q0 (no progress): q0 >= nq, or query q0's
// block alone reaches RP_MAX_ENTRIES.
inline uint32_t rp_cut(const uint64_t* block, uint32_t nq, uint32_t q0, uint64_t budget_entries) {
  uint64_t sum = 0;
  uint32_t q = q0;
  while (q < nq) {
    if (block[q] >= RP_MAX_ENTRIES - sum) break;                     // (sum < RP_MAX_ENTRIES: no wrap)
    if (q > q0 && sum + block[q] > budget_entries) break;
    sum += block[q];
    ++q;
  }
  return q;
}

// off[q] = base + the counts before q; lims (optional, nq entries: the caller's out_lims + 1) = base + the counts up to and
// including q.  Returns base + every count.
inline uint64_t rp_scan(const uint64_t* cnt, uint32_t nq, uint64_t base, uint64_t* off, uint64_t* lims) {
  uint64_t run = base;
  for (uint32_t q = 0; q < nq; ++q) {
    if (off) off[q] = run;
    run += cnt[q];
    if (lims) lims[q] = run;
  }
  return run;
}

// slab length of a count: the smallest power of two >= max(cnt, 2) (the sort network needs one pair); 0 for cnt == 0
inline uint64_t rp_slab_len(uint64_t cnt) {
  if (cnt == 0) return 0;
  uint64_t K2 = 2;
  while (K2 < cnt) K2 <<= 1;
  return K2;
}

// one query's slab inside a run: its first key, its length, the query (number inside the sub-batch) and its count
struct RpSlab {
  uint64_t slab_off, K2;
  uint32_t q, cnt;
};

// The slabs of the queries with cnt[i] > 0, ordered by length (stable: equal lengths by query), slabs of one length side by side
// so that one sort launch serves a whole class; cut into runs that hold at most slab_max keys (a single slab is taken whatever
// slab_max says) and at most max_slabs slabs (>= 1: a run's slabs are one grid dimension of its launches).  run_end[r] = one past the last slab of run r; slab_off restarts at 0 in every run.
// false (nothing usable written): a count whose slab would exceed RP_MAX_SLAB.
inline bool rp_slab_runs(const uint32_t* cnt, uint32_t nq, uint64_t slab_max, uint32_t max_slabs, std::vector<RpSlab>& slabs, std::vector<uint32_t>& run_end) {
  slabs.clear();
  run_end.clear();
  for (uint32_t i = 0; i < nq; ++i) {
    if (!cnt[i]) continue;
    const uint64_t K2 = rp_slab_len(cnt[i]);
    if (K2 > RP_MAX_SLAB) return false;
    slabs.push_back(RpSlab{0ull, K2, i, cnt[i]});
  }
  std::stable_sort(slabs.begin(), slabs.end(), [](const RpSlab& a, const RpSlab& b) { return a.K2 < b.K2; });
  uint64_t keys = 0;
  for (size_t i = 0; i < slabs.size(); ++i) {
    const size_t run_begin = run_end.empty() ? 0 : run_end.back();
    if (i > run_begin && (keys + slabs[i].K2 > slab_max || i - run_begin >= max_slabs)) {
      run_end.push_back(static_cast<uint32_t>(i));
      keys = 0;
    }
    slabs[i].slab_off = keys;
    keys += slabs[i].K2;
  }
  if (!slabs.empty()) run_end.push_back(static_cast<uint32_t>(slabs.size()));
  return true;
}

// one query's share of a run's collect / sort / emit launches, as the kernels read it
struct RangeDesc {
  unsigned long long slab_off;       // first key of the query's slab (entries; the slabs of one K2 class are adjacent)
  unsigned long long out_off;        // first entry of the query in the packed arrays
  uint32_t q;                        // the query's number inside the sub-batch (row of the score matrix / candidate block)
  uint32_t cnt;                      // entries that reach the radius
  uint32_t K2;                       // slab length: cnt rounded up to a power of two (>= 2)
  uint32_t pad;
};

// The descriptors of the run slabs[r0 .. r1) of rp_slab_runs; out_off[q] = query q's first entry in the packed arrays.  Returns
// the run's keys (its last slab's end).
inline uint64_t rp_run_descs(const std::vector<RpSlab>& slabs, size_t r0, size_t r1, const uint64_t* out_off, std::vector<RangeDesc>& run) {
  run.clear();
  for (size_t i = r0; i < r1; ++i) run.push_back(RangeDesc{slabs[i].slab_off, out_off[slabs[i].q], slabs[i].q, slabs[i].cnt, static_cast<uint32_t>(slabs[i].K2), 0u});
  return r1 > r0 ? slabs[r1 - 1].slab_off + slabs[r1 - 1].K2 : 0;
}

}  // namespace nvdbhip
