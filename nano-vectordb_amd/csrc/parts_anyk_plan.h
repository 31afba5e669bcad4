// parts_anyk_plan.h -- the host-side arithmetic of the probe search for any k (nvdb_parts_anyk.cpp) beyond range_plan.h: the slab a
// query's selected keys take and whether it is sorted in LDS or in global memory, where a batch is cut into query sub-batches, and
// a sub-batch's plan -- the width of its device output rows, the LDS the select kernel needs, the key slabs of the long lists.
// Plain C++ with no HIP in it (pa_slab_len is constexpr, so the select kernel evaluates the very same function): the sanitizer
// build of tests/parts_anyk_plan_check.cpp compiles the code the entry points run.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "range_plan.h"

namespace nvdbhip {

// the longest slab the select kernel sorts in LDS (64 KB of keys beside the histogram); longer ones are sorted in global memory
constexpr uint32_t PA_LDS_KEYS = 8192;

// Slab length of a query with a candidate block of len entries: the smallest power of two >= max(min(k, len), 2); 0 for an empty
// block.  The host knows len (the rows of the probed union) but, under a mask, not how many entries are live: both sides size
// and route the slab by len.
constexpr uint64_t pa_slab_len(uint32_t k, uint32_t len) {
  const uint32_t want = k < len ? k : len;
  if (want == 0) return 0;
  uint64_t K2 = 2;
  while (K2 < want) K2 <<= 1;
  return K2;
}
constexpr bool pa_slab_is_long(uint64_t K2) { return K2 > PA_LDS_KEYS; }

// rp_cut for the top-k: the sub-batch q0 .. q1 whose candidate blocks stay within budget_entries and below RP_MAX_ENTRIES, whose
// long slabs together hold at most budget_entries keys, and whose device output -- (q1 - q0) rows of min(k, longest block)
// entries -- holds at most budget_entries entries.  A single query is taken whatever the budget says.  q1 == q0: q0 >= nq, or
// query q0's block alone reaches RP_MAX_ENTRIES.
inline uint32_t pa_cut(const uint64_t* block, uint32_t nq, uint32_t q0, uint32_t k, uint64_t budget_entries) {
  uint64_t sum = 0, slabs = 0, widest = 0;
  uint32_t q = q0;
  while (q < nq) {
    if (block[q] >= RP_MAX_ENTRIES - sum) break;                     // (sum < RP_MAX_ENTRIES: no wrap; block[q] fits 32 bits)
    const uint64_t K2 = pa_slab_len(k, static_cast<uint32_t>(block[q]));
    const uint64_t long_keys = pa_slab_is_long(K2) ? K2 : 0;
    const uint64_t w = std::max<uint64_t>(widest, std::min<uint64_t>(k, block[q]));
    if (q > q0 && (sum + block[q] > budget_entries || slabs + long_keys > budget_entries || static_cast<uint64_t>(q - q0 + 1) * w > budget_entries)) break;
    sum += block[q];
    slabs += long_keys;
    widest = w;
    ++q;
  }
  return q;
}

// one long list as the emit kernel reads it (32-bit words only: the list rides in the work list's image)
struct PaLong {
  uint32_t off_lo, off_hi;           // first key of the query's slab
  uint32_t q;                        // the query's number inside the sub-batch
  uint32_t K2;
};

constexpr uint32_t PA_NO_SLAB = 0xFFFFFFFFu;

// a sub-batch of b queries
struct PaPlan {
  uint32_t out_k = 1;                // entries per row of the device output: min(k, longest block), at least 1
  uint32_t lds_keys = 2;             // the longest slab sorted in LDS
  uint64_t slab_keys = 0;            // keys of all long slabs
  std::vector<uint32_t> slab_off;    // [b][2]: (lo, hi) of the query's first key; (PA_NO_SLAB, PA_NO_SLAB): sorted in LDS
  std::vector<PaLong> longs;         // ordered by K2 (equal lengths side by side: one sort launch per length), then by query
};

// false (the plan is unusable): a slab longer than RP_MAX_SLAB (more than 2^31 results for one query)
inline bool pa_plan(const uint64_t* block, uint32_t b, uint32_t k, PaPlan& p) {
  p = PaPlan{};
  p.slab_off.assign(static_cast<size_t>(b) * 2, PA_NO_SLAB);
  std::vector<uint32_t> cnt(b, 0u);                                  // what rp_slab_runs sizes a slab by; 0: no slab in global memory
  uint64_t widest = 0;
  for (uint32_t i = 0; i < b; ++i) {
    const uint32_t len = static_cast<uint32_t>(block[i]);
    widest = std::max<uint64_t>(widest, std::min<uint32_t>(k, len));
    const uint64_t K2 = pa_slab_len(k, len);
    if (pa_slab_is_long(K2)) cnt[i] = std::min<uint32_t>(k, len);
    else p.lds_keys = std::max(p.lds_keys, static_cast<uint32_t>(K2));
  }
  p.out_k = static_cast<uint32_t>(std::max<uint64_t>(widest, 1));
  std::vector<RpSlab> slabs;
  std::vector<uint32_t> run_end;
  if (!rp_slab_runs(cnt.data(), b, ~0ull, 0xFFFFFFFFu, slabs, run_end)) return false;     // (no limits: one run)
  for (const RpSlab& s : slabs) {
    p.slab_off[static_cast<size_t>(s.q) * 2] = static_cast<uint32_t>(s.slab_off);
    p.slab_off[static_cast<size_t>(s.q) * 2 + 1] = static_cast<uint32_t>(s.slab_off >> 32);
    p.longs.push_back(PaLong{static_cast<uint32_t>(s.slab_off), static_cast<uint32_t>(s.slab_off >> 32), s.q, static_cast<uint32_t>(s.K2)});
    p.slab_keys = s.slab_off + s.K2;
  }
  return true;
}

}  // namespace nvdbhip
