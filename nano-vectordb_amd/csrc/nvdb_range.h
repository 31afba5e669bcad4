// nvdb_range.h -- what the flat range search (nvdb_range.cpp) and the range search on the probe path (nvdb_range_parts.cpp) share:
// the packed result arrays of a call and their budget, and the partition range scan as the flat masked search calls it.  Internal.
#pragma once
#include "nvdb_parts.h"
#include "kernels_range.h"

namespace nvdbhip {

constexpr uint32_t RANGE_STAT_FILTER = 5, RANGE_STAT_EXACT = 6, RANGE_STAT_PARTS = 7;     // nvdb_hip_scan_stats::path

// grow a packed result array, keeping what it holds
inline nvdb_status grow_keep(nvdb_hip_ctx* c, hipStream_t s, DevBuf& b, size_t bytes, size_t limit_bytes) {
  if (b.p && b.bytes >= bytes) return NVDB_OK;
  const size_t want = std::max<size_t>(std::max(bytes, std::min(bytes + bytes / 2, limit_bytes)), static_cast<size_t>(1) << 20);
  void* np = nullptr;
  HIPCHK(c, hipMalloc(&np, want));
  if (b.p) {
    HIPCHK(c, hipMemcpyAsync(np, b.p, b.bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipFree(b.p));
  }
  b.p = np; b.bytes = want;
  return NVDB_OK;
}

// the packed arrays of one call: how far they are filled, and whether the call still packs (false: over budget, counting only)
struct RangeOut {
  uint64_t budget_entries = 0;
  bool pack = true;
};

// room for `end` entries; false: the budget is exceeded (from here on the call only counts), or *st
inline bool reserve_packed(nvdb_hip_ctx* c, hipStream_t s, RangeOut& out, uint64_t end, nvdb_status* st) {
  *st = NVDB_OK;
  if (!out.pack) return false;
  if (end > out.budget_entries) { out.pack = false; return false; }
  if ((*st = grow_keep(c, s, c->rg_ids, static_cast<size_t>(end) * 8, static_cast<size_t>(out.budget_entries) * 8))) return false;
  if ((*st = grow_keep(c, s, c->rg_scores, static_cast<size_t>(end) * 4, static_cast<size_t>(out.budget_entries) * 4))) return false;
  return true;
}

template <typename T>
inline nvdb_status upload(nvdb_hip_ctx* c, hipStream_t s, DevBuf& b, const std::vector<T>& v) {
  if (nvdb_status st = ensure(c, b, v.size() * sizeof(T))) return st;
  HIPCHK(c, hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipStreamSynchronize(s));       // (the vector may go away; earlier kernels that read the buffer have finished)
  return NVDB_OK;
}

// ---- the partition range scan (nvdb_range_parts.cpp) over the table off[0 .. nparts]: nr queries (host memory) with their radii and
// probe rows; msel != nullptr: masked (validated by the caller).  qmap[i] = query i's number inside the caller's sub-batch
// (ascending; nullptr: i).  Fills cnt[qmap[i]] and, while the call packs, emits query i's slice at base + (sum of cnt[] before
// qmap[i]) -- as range_exact does: the counts of every earlier query of the sub-batch are known by then.  Adds its launches, rows
// and entries to c->stats.  The batch is cut into consecutive query sub-batches under largek_budget_mb here.
nvdb_status range_parts_core(nvdb_hip_ctx* c, hipStream_t s, const char* who, const uint64_t* off, uint32_t nparts, const float* queries, const float* radius,
                             uint32_t nr, const uint32_t* probe, uint32_t nprobe, const MaskSel* msel, const uint32_t* qmap, std::vector<uint64_t>& cnt,
                             uint64_t base, RangeOut& out);

// nvdb_hip_range_search and nvdb_hip_range_search_masked (msel != nullptr; nvdb_range.cpp)
nvdb_status range_search_flat(nvdb_hip_ctx* c, const char* who, const float* queries, uint32_t nq, const float* radius, const MaskSel* msel, uint64_t* out_lims,
                              nvdb_hip_timing* timing);

}  // namespace nvdbhip
