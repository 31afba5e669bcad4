// ivf_layout.h -- the inverted-list layout of an assignment: a stable counting sort, plain C++ with no HIP in it, so that the
// sanitizer build of tests/ivf_layout_check.cpp compiles the very code nvdb_ivf_layout_host (nvdb_ivf.cpp) runs.
#pragma once
#include <cstdint>
#include <vector>

namespace nvdbhip {

constexpr uint64_t IVF_MAX_ROWS = 0xFFFFFF00ull;   // what nvdb_hip_set_partitions takes

// offsets[p] = first list position of partition p (nparts + 1 entries), perm[j] = the original row at position j: positions are
// ordered by partition, then by original row.  false (nothing written): a null pointer, n > IVF_MAX_ROWS, an entry >= nparts.
inline bool ivf_layout(const uint32_t* assign, uint64_t n, uint32_t nparts, uint64_t* offsets, uint32_t* perm) {
  if (!assign || !offsets || !perm || n > IVF_MAX_ROWS) return false;
  std::vector<uint64_t> next(static_cast<size_t>(nparts) + 1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    if (assign[i] >= nparts) return false;
    ++next[assign[i] + 1];
  }
  for (uint32_t p = 0; p < nparts; ++p) next[p + 1] += next[p];
  for (uint32_t p = 0; p <= nparts; ++p) offsets[p] = next[p];
  for (uint64_t i = 0; i < n; ++i) perm[next[assign[i]]++] = static_cast<uint32_t>(i);
  return true;
}

}  // namespace nvdbhip
