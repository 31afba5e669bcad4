// ivf_layout_check.cpp -- the inverted-list layout behind nvdb_ivf_layout_host (nano-vectordb_amd/csrc/ivf_layout.h, the code the
// library's entry point runs) against std::stable_sort, with exactly sized heap buffers: built with -fsanitize=address,undefined
// by tests/test_cabi_ivf_cpu.py, a write past an output or a read past the assignment stops the program.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "ivf_layout.h"

using nvdbhip::ivf_layout;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static void check_case(const char* name, const std::vector<uint32_t>& assign, uint32_t nparts) {
  const uint64_t n = assign.size();
  // heap copies of exactly n / nparts + 1 entries (a one-entry block stands in for an empty array: the pointer must not be null)
  uint32_t* a = new uint32_t[n ? n : 1];
  std::copy(assign.begin(), assign.end(), a);
  uint64_t* offsets = new uint64_t[nparts + 1];
  uint32_t* perm = new uint32_t[n ? n : 1];
  std::fill(offsets, offsets + nparts + 1, 77u);
  CHECK(ivf_layout(a, n, nparts, offsets, perm));
  std::vector<uint32_t> want(n);
  std::iota(want.begin(), want.end(), 0u);
  std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) { return assign[x] < assign[y]; });
  CHECK(std::equal(want.begin(), want.end(), perm));
  std::vector<uint64_t> count(nparts + 1, 0);
  for (uint32_t p : assign) ++count[p + 1];
  for (uint32_t p = 0; p < nparts; ++p) count[p + 1] += count[p];
  CHECK(std::equal(count.begin(), count.end(), offsets));
  CHECK(offsets[0] == 0 && offsets[nparts] == n);
  std::printf("%s: n=%llu nparts=%u checked\n", name, static_cast<unsigned long long>(n), nparts);
  delete[] a; delete[] offsets; delete[] perm;
}

int main() {
  uint32_t state = 12345u;
  auto next = [&]() { state = state * 1664525u + 1013904223u; return state >> 8; };
  std::vector<uint32_t> v(10000);
  for (auto& x : v) x = next() % 37u;
  check_case("random", v, 37);
  check_case("one partition", std::vector<uint32_t>(500, 3u), 7);
  for (auto& x : v) x = 2u + next() % 5u;                                // partitions 0, 1 and 7 .. 9 stay empty
  check_case("empty at both ends", v, 10);
  check_case("no rows", std::vector<uint32_t>(), 5);

  // an entry == nparts, null pointers, too many rows: refused with the outputs untouched
  std::vector<uint32_t> bad = {0, 1, 2, 3, 1};
  std::vector<uint64_t> off(4, 99u);
  std::vector<uint32_t> perm(5, 99u);
  CHECK(!ivf_layout(bad.data(), bad.size(), 3, off.data(), perm.data()));
  CHECK(std::count(off.begin(), off.end(), 99u) == 4 && std::count(perm.begin(), perm.end(), 99u) == 5);
  bad[3] = 2;
  CHECK(!ivf_layout(nullptr, bad.size(), 3, off.data(), perm.data()));
  CHECK(!ivf_layout(bad.data(), bad.size(), 3, nullptr, perm.data()));
  CHECK(!ivf_layout(bad.data(), bad.size(), 3, off.data(), nullptr));
  CHECK(!ivf_layout(bad.data(), 0xFFFFFF01ull, 3, off.data(), perm.data()));
  CHECK(std::count(off.begin(), off.end(), 99u) == 4 && std::count(perm.begin(), perm.end(), 99u) == 5);
  CHECK(ivf_layout(bad.data(), bad.size(), 3, off.data(), perm.data()));
  CHECK((perm == std::vector<uint32_t>{0, 1, 4, 2, 3}) && (off == std::vector<uint64_t>{0, 1, 3, 5}));

  std::printf(failures ? "FAILED\n" : "OK\n");
  return failures ? 1 : 0;
}
