// row_mask_check.cpp -- the host-side bit work of the row masks (nano-vectordb_amd/csrc/row_mask.h, the code the library's entry
// points run) against naive loops, with exactly sized heap buffers: built with -fsanitize=address,undefined by
// tests/test_cabi_row_masks_cpu.py, a write past a plane or a read past a row list stops the program.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "row_mask.h"

using namespace nvdbhip;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static uint32_t state = 12345u;
static uint32_t next() { state = state * 1664525u + 1013904223u; return state >> 8; }

static bool bit(const uint32_t* plane, uint64_t r) { return (plane[r >> 5] >> (r & 31u)) & 1u; }

static void check_tail(uint64_t n) {
  const uint64_t W = rm_words(n);
  CHECK(W == (n + 31) / 32);
  uint32_t* plane = new uint32_t[W];                 // exactly W words
  std::fill(plane, plane + W, 0xFFFFFFFFu);
  rm_clear_tail(plane, n);
  for (uint64_t r = 0; r < W * 32; ++r) CHECK(bit(plane, r) == (r < n));
  for (uint64_t w = 0; w < W; ++w) plane[w] = next() * 2654435761u;
  std::vector<uint32_t> before(plane, plane + W);
  rm_clear_tail(plane, n);
  for (uint64_t r = 0; r < W * 32; ++r) CHECK(bit(plane, r) == (r < n && bit(before.data(), r)));
  std::printf("tail n=%llu checked\n", static_cast<unsigned long long>(n));
  delete[] plane;
}

static void check_permute(uint64_t n) {
  const uint64_t W = rm_words(n);
  uint32_t* perm = new uint32_t[n];
  std::iota(perm, perm + n, 0u);
  for (uint64_t i = n; i > 1; --i) std::swap(perm[i - 1], perm[next() % i]);
  uint32_t* src = new uint32_t[W];
  for (uint64_t w = 0; w < W; ++w) src[w] = next() * 2654435761u;
  rm_clear_tail(src, n);
  uint32_t* dst = new uint32_t[W];
  std::fill(dst, dst + W, 0xFFFFFFFFu);             // must be overwritten completely
  rm_permute(src, perm, n, dst);
  for (uint64_t j = 0; j < n; ++j) CHECK(bit(dst, j) == bit(src, perm[j]));
  for (uint64_t r = n; r < W * 32; ++r) CHECK(!bit(dst, r));
  uint32_t* inv = new uint32_t[n];
  CHECK(rm_inverse(perm, n, inv));
  for (uint64_t j = 0; j < n; ++j) CHECK(inv[perm[j]] == j);
  // round trip: permuting the permuted plane through the inverse gives the source plane back
  uint32_t* back = new uint32_t[W];
  rm_permute(dst, inv, n, back);
  CHECK(std::equal(src, src + W, back));
  if (n >= 2) {                                      // a row named twice is no permutation
    perm[0] = perm[1];
    CHECK(!rm_inverse(perm, n, inv));
    perm[0] = static_cast<uint32_t>(n);              // ... nor is a row >= n
    CHECK(!rm_inverse(perm, n, inv));
  }
  std::printf("permute n=%llu checked\n", static_cast<unsigned long long>(n));
  delete[] perm; delete[] src; delete[] dst; delete[] inv; delete[] back;
}

int main() {
  for (uint64_t n : {1, 31, 32, 33, 64, 65}) check_tail(n);
  for (uint64_t n : {1, 31, 32, 33, 64, 65, 10007}) check_permute(n);

  // row lists: duplicates are legal, a row == n is not; an empty list is fine with a null pointer
  const uint64_t n = 65;
  uint64_t* rows = new uint64_t[4]{0, 64, 64, 31};
  CHECK(rm_rows_valid(rows, 4, n));
  rows[2] = 65;
  CHECK(!rm_rows_valid(rows, 4, n));
  CHECK(rm_rows_valid(rows, 2, n));
  rows[0] = ~0ull;
  CHECK(!rm_rows_valid(rows, 1, n));
  CHECK(rm_rows_valid(nullptr, 0, n));
  delete[] rows;
  // mask numbers: < nmasks or the "no mask" number; no masks resident: never valid; null: plane 0 for every query
  uint32_t* mo = new uint32_t[3]{0, 2, ROW_MASK_NONE};
  CHECK(rm_mask_of_valid(mo, 3, 3));
  CHECK(!rm_mask_of_valid(mo, 3, 2));
  CHECK(rm_mask_of_valid(mo, 1, 1));
  CHECK(!rm_mask_of_valid(mo, 3, 0));
  CHECK(rm_mask_of_valid(nullptr, 3, 1));
  CHECK(!rm_mask_of_valid(nullptr, 3, 0));
  delete[] mo;
  std::printf("lists checked\n");

  std::printf(failures ? "FAILED\n" : "OK\n");
  return failures ? 1 : 0;
}
