// range_plan_check.cpp -- the host-side arithmetic of the range searches (nano-vectordb_amd/csrc/range_plan.h, the code the
// library's entry points run) against naive loops, with exactly sized heap buffers: built with -fsanitize=address,undefined by
// tests/test_cabi_range_parts_cpu.py, a read past a count list or a write past an offset array stops the program.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "range_plan.h"

using namespace nvdbhip;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// the slab of one count: a power of two, >= 2, >= cnt, and the smallest such
static void check_slab(uint32_t cnt) {
  const uint64_t K2 = rp_slab_len(cnt);
  if (cnt == 0) CHECK(K2 == 0);
  else {
    CHECK(K2 >= 2 && K2 >= cnt && (K2 & (K2 - 1)) == 0);
    CHECK(K2 == 2 || K2 / 2 < cnt);
  }
  // one query: its run, its offsets
  uint32_t* c = new uint32_t[1]{cnt};
  std::vector<RpSlab> slabs;
  std::vector<uint32_t> run_end;
  CHECK(rp_slab_runs(c, 1, 1, 1, slabs, run_end));
  CHECK(slabs.size() == (cnt ? 1u : 0u) && run_end.size() == slabs.size());
  if (cnt) CHECK(slabs[0].slab_off == 0 && slabs[0].K2 == K2 && slabs[0].q == 0 && slabs[0].cnt == cnt && run_end[0] == 1);
  delete[] c;
  std::printf("slab cnt=%u checked\n", cnt);
}

// counts -> offsets / lims, classes and runs
static void check_counts() {
  const uint32_t nq = 7;
  uint64_t* cnt = new uint64_t[nq]{0, 1, 8192, 8193, 0, 3, 8192};
  uint64_t* off = new uint64_t[nq];
  uint64_t* lims = new uint64_t[nq + 1];
  lims[0] = 100;
  const uint64_t total = rp_scan(cnt, nq, 100, off, lims + 1);
  uint64_t run = 100;
  for (uint32_t q = 0; q < nq; ++q) { CHECK(off[q] == run); run += cnt[q]; CHECK(lims[q + 1] == run); }
  CHECK(total == run && total == 100 + 1 + 8192 + 8193 + 3 + 8192);
  CHECK(rp_scan(cnt, nq, 0, nullptr, nullptr) == total - 100);
  CHECK(rp_scan(nullptr, 0, 5, nullptr, nullptr) == 5);

  uint32_t* c32 = new uint32_t[nq];
  for (uint32_t q = 0; q < nq; ++q) c32[q] = static_cast<uint32_t>(cnt[q]);
  std::vector<RpSlab> slabs;
  std::vector<uint32_t> run_end;
  // room for everything: one run, ordered by class, equal classes by query, offsets a running sum
  CHECK(rp_slab_runs(c32, nq, 1ull << 40, 1u << 20, slabs, run_end));
  CHECK(slabs.size() == 5 && run_end.size() == 1 && run_end[0] == 5);
  const uint32_t want_q[5] = {1, 5, 2, 6, 3};
  const uint64_t want_k[5] = {2, 4, 8192, 8192, 16384};
  uint64_t at = 0;
  for (size_t i = 0; i < slabs.size(); ++i) {
    CHECK(slabs[i].q == want_q[i] && slabs[i].K2 == want_k[i] && slabs[i].cnt == c32[want_q[i]] && slabs[i].slab_off == at);
    at += slabs[i].K2;
  }
  // 8192 keys per run: {2, 4}, {8192}, {8192}, {16384 alone, over the limit}
  CHECK(rp_slab_runs(c32, nq, 8192, 1u << 20, slabs, run_end));
  CHECK(run_end.size() == 4 && run_end[0] == 2 && run_end[1] == 3 && run_end[2] == 4 && run_end[3] == 5);
  CHECK(slabs[0].slab_off == 0 && slabs[1].slab_off == 2 && slabs[2].slab_off == 0 && slabs[3].slab_off == 0 && slabs[4].slab_off == 0);
  // at most two slabs per run
  CHECK(rp_slab_runs(c32, nq, 1ull << 40, 2, slabs, run_end));
  CHECK(run_end.size() == 3 && run_end[0] == 2 && run_end[1] == 4 && run_end[2] == 5 && slabs[3].slab_off == 8192 && slabs[4].slab_off == 0);
  // ... and the descriptors of those runs: every slab once, its query's offset, the run's keys
  {
    std::vector<RangeDesc> run;
    size_t r0 = 0, seen = 0;
    const uint64_t want_keys[3] = {2 + 4, 8192 + 8192, 16384};
    for (size_t r = 0; r < run_end.size(); ++r) {
      const size_t r1 = run_end[r];
      CHECK(rp_run_descs(slabs, r0, r1, off, run) == want_keys[r] && run.size() == r1 - r0);
      for (size_t i = 0; i < run.size(); ++i, ++seen) {
        const RangeDesc& d = run[i];
        CHECK(d.q == want_q[seen] && d.cnt == c32[d.q] && d.K2 == want_k[seen] && d.out_off == off[d.q] && d.pad == 0);
        CHECK(d.slab_off == (i ? run[i - 1].slab_off + run[i - 1].K2 : 0));
      }
      r0 = r1;
    }
    CHECK(seen == 5);
    CHECK(rp_run_descs(slabs, 2, 2, off, run) == 0 && run.empty());      // an empty run
  }
  // a count beyond 2^31 has no slab
  c32[0] = 0x80000001u;
  CHECK(!rp_slab_runs(c32, nq, 1ull << 40, 2, slabs, run_end));
  c32[0] = 0x80000000u;
  CHECK(rp_slab_runs(c32, nq, 1ull << 40, 1u << 20, slabs, run_end) && slabs.back().K2 == RP_MAX_SLAB);
  // no counts at all
  CHECK(rp_slab_runs(nullptr, 0, 8, 8, slabs, run_end) && slabs.empty() && run_end.empty());
  delete[] cnt; delete[] off; delete[] lims; delete[] c32;
  std::printf("counts checked\n");
}

// the cut against a naive restatement: every sub-batch is the longest admissible run of consecutive queries
static void check_cut(const std::vector<uint64_t>& blocks, uint64_t budget, const std::vector<uint32_t>& want_ends, const char* what) {
  const uint32_t nq = static_cast<uint32_t>(blocks.size());
  uint64_t* b = new uint64_t[nq];                    // exactly nq entries
  for (uint32_t q = 0; q < nq; ++q) b[q] = blocks[q];
  std::vector<uint32_t> ends;
  for (uint32_t q0 = 0; q0 < nq;) {
    const uint32_t q1 = rp_cut(b, nq, q0, budget);
    if (q1 == q0) break;
    uint64_t sum = 0;
    for (uint32_t q = q0; q < q1; ++q) sum += b[q];
    CHECK(sum < RP_MAX_ENTRIES);
    CHECK(q1 == q0 + 1 || sum <= budget);
    if (q1 < nq) CHECK(sum + b[q1] > budget || sum + b[q1] >= RP_MAX_ENTRIES);   // one more query would not have fitted
    ends.push_back(q1);
    q0 = q1;
  }
  CHECK(ends == want_ends);
  CHECK(rp_cut(b, nq, nq, budget) == nq);
  delete[] b;
  std::printf("cut %s checked\n", what);
}

int main() {
  for (uint32_t cnt : {0u, 1u, 8192u, 8193u}) check_slab(cnt);
  check_counts();
  check_cut({5, 5, 5, 5}, 100, {4}, "all in one");
  check_cut({5, 5, 5, 5}, 10, {2, 4}, "pairs");
  check_cut({20000, 20000, 20000}, 131072 / 8, {1, 2, 3}, "one query per sub-batch");      // a 1 MB budget of 8-byte entries against 20000-row unions
  check_cut({0, 0, 7, 0, 9, 0}, 7, {4, 5, 6}, "empty blocks");                          // (behind a block that is over the budget by itself nothing rides along)
  check_cut({0xC0000000ull, 0x3FFFFFFEull, 1, 0x7FFFFFFFull, 0x7FFFFFFFull, 1}, ~0ull, {2, 4, 6}, "2^32 entries");   // 2^32 - 2 fits, 2^32 - 1 does not
  check_cut({5, 0xFFFFFFFFull, 5}, ~0ull, {1}, "a block that cannot be placed");            // no progress at query 1: the caller reports it
  check_cut({}, 10, {}, "no queries");
  std::printf(failures ? "FAILED\n" : "OK\n");
  return failures ? 1 : 0;
}
