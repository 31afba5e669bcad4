// nvdb_range.h -- what the flat range search (nvdb_range.cpp) and the range search on the probe path (nvdb_range_parts.cpp) share:
// the packed result arrays of a call and their budget, the tail that turns downloaded counts into sorted, emitted slices
// (range_tail), and the partition range scan as the flat masked search calls it (range_parts_core: per sub-batch one parts_pass
// of nvdb_parts.h, the count, the tail).  Internal.
#pragma once
#include "nvdb_parts.h"
#include "kernels_range.h"
#include "range_plan.h"

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

constexpr uint32_t RUN_MAX_SLABS = 32768;          // a run's slabs are the y dimension of its collect / sort / emit grids

// The tail both range routes share, from "the counts of a sub-batch are on the host" to "emit launched": hc[i] = query i's
// count (i < b), out_off[i] = its first entry in the packed arrays (room reserved by the caller).  The slabs and their runs are
// range_plan.h's (at most slab_max keys and RUN_MAX_SLABS slabs per run); per run the descriptors are uploaded, taken[] is
// zeroed, collect(run, desc, taken, slab) launches the caller's collect kernel (grid y = run.size()), every length class is
// sorted, emit(run, max_cnt, desc, slab) launches the caller's emit kernel.  run: the descriptors on the host; desc: on the device.
template <class Collect, class Emit>
nvdb_status range_tail(nvdb_hip_ctx* c, hipStream_t s, const char* who, const uint32_t* hc, uint32_t b, const uint64_t* out_off, uint64_t slab_max,
                       Collect&& collect, Emit&& emit) {
  std::vector<RpSlab> slabs;
  std::vector<uint32_t> run_end;
  std::vector<RangeDesc> run;
  nvdb_status st;
  if (!rp_slab_runs(hc, b, slab_max, RUN_MAX_SLABS, slabs, run_end)) return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 results for one query");
  size_t r0 = 0;
  for (const uint32_t r1 : run_end) {
    const uint64_t keys = rp_run_descs(slabs, r0, r1, out_off, run);
    const uint32_t nrun = static_cast<uint32_t>(run.size());
    uint32_t max_cnt = 0;
    for (const RangeDesc& d : run) max_cnt = std::max(max_cnt, d.cnt);
    if ((st = ensure(c, c->rg_slab, static_cast<size_t>(keys) * 8))) return st;
    if ((st = ensure(c, c->rg_taken, static_cast<size_t>(nrun) * 4))) return st;
    if ((st = upload(c, s, c->rg_desc, run))) return st;
    const RangeDesc* desc = static_cast<const RangeDesc*>(c->rg_desc.p);
    unsigned long long* slab = static_cast<unsigned long long*>(c->rg_slab.p);
    uint32_t* taken = static_cast<uint32_t*>(c->rg_taken.p);
    HIPCHK(c, hipMemsetAsync(taken, 0, static_cast<size_t>(nrun) * 4, s));
    collect(run, desc, taken, slab);
    HIPCHK(c, hipGetLastError());
    for (uint32_t a = 0; a < nrun;) {                 // slabs of one length side by side: one sort launch per length
      uint32_t e = a;
      while (e < nrun && run[e].K2 == run[a].K2) ++e;
      if ((st = launch_sort_keys(c, s, slab + run[a].slab_off, run[a].K2, e - a))) return st;
      a = e;
    }
    emit(run, max_cnt, desc, slab);
    HIPCHK(c, hipGetLastError());
    r0 = r1;
  }
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

// one launch of range_parts_kernel's build for this corpus (qw queries per wave) over the items of `a`; radius: per query of the
// launch set, on the device (the probe search for any k, nvdb_parts_anyk.cpp, passes -inf throughout)
nvdb_status launch_range_parts(nvdb_hip_ctx* c, hipStream_t s, uint32_t qw, bool staged, const float* radius, const ScanArgs& a);

// ---- the flat range search's plan and filter pass (nvdb_range.cpp), as the masked flat top-k (nvdb_masked_flat.cpp) calls them
// FilterPlan (nvdb_ctx.h): kind, cap, query tiling, prep_inits, perm_on; filter (== prep): the filter route serves this sub-batch (else: the exact route alone)
struct RangePlan : FilterPlan {
  const char* error = nullptr;
  bool tail_exact = false;
  uint32_t tile_rows = 0, n_al = 0;
  uint32_t launch_rows = 0;             // rows per filter launch
};
// the route and shapes of one sub-batch of nq queries; p.error: why a forced route is refused
nvdb_status plan_range(const nvdb_hip_ctx& ctx, uint32_t nq, RangePlan& p);

// what the host reads of one filter pass
struct FilterVerdict {
  std::vector<uint32_t> kept, overflow, listcnt;
  uint32_t misc[8] = {0};
};
// filter route of one sub-batch: everything up to the ordered slabs in c->cand and their counts in c->rg_kept, then the verdict's
// read-back (synchronises the stream).  dmask_of != nullptr: the keep step also requires the row's bit in the query's plane
nvdb_status range_filter_pass(nvdb_hip_ctx* c, hipStream_t s, const RangePlan& p, const float* dq, const float* dradius, uint32_t nq, const uint32_t* dmask_of,
                              FilterVerdict& v);

// nvdb_hip_range_search and nvdb_hip_range_search_masked (msel != nullptr; nvdb_range.cpp)
nvdb_status range_search_flat(nvdb_hip_ctx* c, const char* who, const float* queries, uint32_t nq, const float* radius, const MaskSel* msel, uint64_t* out_lims,
                              nvdb_hip_timing* timing);

}  // namespace nvdbhip
