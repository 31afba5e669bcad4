// row_mask.h -- the host-side bit work of the row masks (nvdb_hip_set_row_masks and friends, include/nvdb_hip.h): plain C++ with
// no HIP in it, so that the sanitizer build of tests/row_mask_check.cpp compiles the very code the entry points run.
// A plane over n rows is W = rm_words(n) uint32 words; row r is live iff bit r & 31 of word r >> 5 is 1.
#pragma once
#include <cstdint>

namespace nvdbhip {

constexpr uint64_t ROW_MASK_MAX_ROWS = 0xFFFFFF00ull;   // what nvdb_hip_set_partitions takes
constexpr uint32_t ROW_MASK_NONE = 0xFFFFFFFFu;         // a mask_of entry: no mask, every row live

inline uint64_t rm_words(uint64_t n) { return (n + 31) / 32; }

// bits at positions >= n of the plane's last word become 0
inline void rm_clear_tail(uint32_t* plane, uint64_t n) {
  if (n % 32) plane[n / 32] &= (1u << (n % 32)) - 1u;
}

// dst bit j = src bit perm[j], j < n (perm[j] < n); dst: rm_words(n) words, written completely, its tail bits 0
inline void rm_permute(const uint32_t* src, const uint32_t* perm, uint64_t n, uint32_t* dst) {
  for (uint64_t w = 0; w < rm_words(n); ++w) dst[w] = 0;
  for (uint64_t j = 0; j < n; ++j) {
    const uint32_t r = perm[j];
    dst[j >> 5] |= ((src[r >> 5] >> (r & 31u)) & 1u) << (j & 31u);
  }
}

// inv[perm[j]] = j; false (inv partly written): perm is no permutation of 0 .. n - 1
inline bool rm_inverse(const uint32_t* perm, uint64_t n, uint32_t* inv) {
  for (uint64_t j = 0; j < n; ++j) inv[j] = 0xFFFFFFFFu;
  for (uint64_t j = 0; j < n; ++j) {
    if (perm[j] >= n || inv[perm[j]] != 0xFFFFFFFFu) return false;
    inv[perm[j]] = static_cast<uint32_t>(j);
  }
  return true;
}

// every listed row is a row of the corpus (duplicates are legal)
inline bool rm_rows_valid(const uint64_t* rows, uint64_t nrows, uint64_t n) {
  for (uint64_t i = 0; i < nrows; ++i)
    if (rows[i] >= n) return false;
  return true;
}

// every query names a resident plane or ROW_MASK_NONE; mask_of == nullptr: every query uses plane 0
inline bool rm_mask_of_valid(const uint32_t* mask_of, uint32_t nq, uint32_t nmasks) {
  if (nmasks == 0) return false;
  if (!mask_of) return true;
  for (uint32_t q = 0; q < nq; ++q)
    if (mask_of[q] != ROW_MASK_NONE && mask_of[q] >= nmasks) return false;
  return true;
}

}  // namespace nvdbhip
