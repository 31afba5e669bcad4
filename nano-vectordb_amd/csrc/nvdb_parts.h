// nvdb_parts.h -- what the probe search (nvdb_partitions.cpp) and the partition range scan (nvdb_range_parts.cpp) share: the
// state behind nvdb_hip_ctx::parts, the kernel build a corpus takes and the dispatch to it (parts_dispatch), the host-side work list
// and its pinned image.  Internal.
#pragma once
#include <type_traits>

#include "nvdb_ctx.h"
#include "kernels_partitions.h"
#include "row_mask.h"

namespace nvdbhip {

struct PartState {
  std::vector<uint64_t> offsets;                   // nparts + 1; empty: no table
  nvdb_hip_ctx* coarse = nullptr;                  // child context that holds the centroids as an f32 corpus (same device)
  bool have_centroids = false;
  // grow-only workspace
  DevBuf meta, cand, q, out_ids, out_scores, out_counts;
  void* pin = nullptr;                             // pinned staging of the work list
  size_t pin_bytes = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // host scratch, reused across calls
  std::vector<uint32_t> uniq, ucount, pcount, pstart, cursor, qidx, dst, cbeg, psum, probe_tmp;
  std::vector<uint64_t> coarse_ids, rows_union;
  std::vector<float> coarse_scores;
  std::vector<PartItem> items[3];
};

constexpr size_t PART_LDS_LIMIT = 160 * 1024;

inline size_t parts_lds(uint32_t dim, uint32_t row_bytes, uint32_t qw, bool staged) {
  const size_t qstride = (dim + 3u) & ~3u;
  return PART_WAVES * qw * qstride * 4 + (staged ? static_cast<size_t>(PART_TILE_ROWS) * part_pitch(row_bytes) : 0);
}

// how a masked search differs from its twin: mask_of as the caller gave it (nullptr: plane 0 for every query; validated by the caller)
struct MaskSel { const uint32_t* mask_of; };

// a masked call's mask_of against the resident planes (before anything is launched)
inline nvdb_status mask_args(nvdb_hip_ctx* c, const uint32_t* mask_of, uint32_t nq, const char* who) {
  if (c->nmasks == 0) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": no row masks (nvdb_hip_set_row_masks)");
  if (!rm_mask_of_valid(mask_of, nq, c->nmasks)) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": mask_of entry names a mask >= nmasks");
  return NVDB_OK;
}

// the kernel build of the resident corpus: rows staged through LDS where they are whole 16-byte chunks and a tile fits beside
// the queries; qw_max = the most queries per wave the LDS has room for (0: not even one -- the dim is too large)
struct PartBuild { uint32_t qw_max = 0; bool staged = false; };
PartBuild parts_build(const nvdb_hip_ctx* c);

// what a launch of either scan passes besides the corpus: nitems work items, the work list's arrays, the queries, the candidate
// buffer; mk.mask_of != nullptr: the MASKED build
struct ScanArgs {
  const PartItem* items; uint32_t nitems; const uint32_t* qidx; const uint32_t* dst; const float* q32; Cand* cand; PartMask mk;
};

// The one place a launch's build -- dtype x QW x {staged, direct aligned, direct unaligned} x masked -- becomes compile-time
// constants: launch(DT, QW, ALIGNED, STAGED, MASKED) receives them as std::integral_constant values and instantiates its kernel.
template <class F>
nvdb_status parts_dispatch(const nvdb_hip_ctx* c, uint32_t qw, bool staged, bool masked, F&& launch) {
  auto with_mask = [&](auto dt, auto w, auto al, auto st) {
    return masked ? launch(dt, w, al, st, std::true_type{}) : launch(dt, w, al, st, std::false_type{});
  };
  auto with_rows = [&](auto dt, auto w) {
    if (staged) return with_mask(dt, w, std::true_type{}, std::true_type{});
    if (aligned_rows(c->dtype, c->dim)) return with_mask(dt, w, std::true_type{}, std::false_type{});
    return with_mask(dt, w, std::false_type{}, std::false_type{});
  };
  auto with_qw = [&](auto dt) {
    if (qw == 4) return with_rows(dt, std::integral_constant<int, 4>{});
    if (qw == 2) return with_rows(dt, std::integral_constant<int, 2>{});
    return with_rows(dt, std::integral_constant<int, 1>{});
  };
  if (c->dtype == NVDB_DTYPE_F32) return with_qw(std::integral_constant<int, DT_F32>{});
  if (c->dtype == NVDB_DTYPE_F16) return with_qw(std::integral_constant<int, DT_F16>{});
  return with_qw(std::integral_constant<int, DT_I8>{});
}

// ... and what every build's launch does alike: the LDS it takes (raised above 64 KB where needed), the grid, the error check.
// args: the kernel's arguments behind (rows, scales, dim)
template <class K, class... A>
nvdb_status parts_launch(nvdb_hip_ctx* c, hipStream_t s, K kernel, uint32_t qw, bool staged, uint32_t nitems, A... args) {
  const size_t lds = parts_lds(c->dim, c->dim * static_cast<uint32_t>(bpe_of(c->dtype)), qw, staged);
  if (lds > 64 * 1024)
    if (nvdb_status st = raise_lds_limit(c, reinterpret_cast<const void*>(kernel), PART_LDS_LIMIT)) return st;
  kernel<<<nitems, PART_THREADS, lds, s>>>(c->rows, c->scales, c->dim, args...);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

// The probe table of a call, checked and de-duplicated, into the PartState's host scratch (uniq / ucount): 0xFFFFFFFF slots dropped,
// a partition named twice counted once, an entry >= nparts -> NVDB_ERR_INVALID.  rows_union (optional, nq entries): the rows of
// every query's probed union.
nvdb_status parts_probes(nvdb_hip_ctx* c, const char* who, const uint64_t* off, uint32_t nparts, uint32_t nq, const uint32_t* probe, uint32_t nprobe,
                         uint64_t* rows_union);

// The work list of queries q0 .. q0 + nq of that table (numbered from 0 inside the list; nvdb_partitions.cpp describes it): the
// counting sort by partition, query groups of at most qg_max queries, segments of at most PART_SEG_ROWS rows, classes by group
// size.  slot_cap: an (item, query) gets min(slot_cap, segment rows) candidate slots (the top-k search: k; the range scan: no cap).
struct PartList { uint32_t npairs = 0; uint64_t total = 0, rows_read = 0; size_t nitems = 0; };
nvdb_status parts_worklist(nvdb_hip_ctx* c, const char* who, const uint64_t* off, uint32_t nparts, uint32_t q0, uint32_t nq, uint32_t nprobe,
                           uint32_t qg_max, uint32_t slot_cap, PartList& wl);

// The pinned image of the work list [items | qidx | dst | cbeg | masked: mask_of | extra] and the device workspace it is copied
// to (meta, grown here; the copy itself is the caller's: hipMemcpyAsync(ps->meta.p, ps->pin, image.bytes)).
struct PartImage {
  size_t bytes = 0;
  const PartItem* items = nullptr;                 // device addresses
  const uint32_t *qidx = nullptr, *dst = nullptr, *cbeg = nullptr, *extra = nullptr;
  PartMask mk{nullptr, nullptr, 0u};
};
nvdb_status parts_stage(nvdb_hip_ctx* c, const PartList& wl, uint32_t nq, const MaskSel* msel, const uint32_t* extra, uint32_t extra_words, PartImage& im);

// nvdb_hip_ctx::parts, created where a call needs the workspace only (no table is set, a table that is set stays as it is)
PartState* parts_workspace(nvdb_hip_ctx* c);

// the coarse step of the IVF forms: the np = min(nprobe, nparts) best centroids of every query into ps->probe_tmp ([nq][np]);
// out_probe (optional) keeps the caller's row length.  timing (optional): receives the coarse search's h2d / kernel / d2h.
nvdb_status parts_coarse(nvdb_hip_ctx* c, const char* who, const float* queries, uint32_t nq, uint32_t nprobe, uint32_t* out_probe, nvdb_hip_timing* timing,
                         uint32_t& np);

// one launch of scan_parts_kernel's build for this corpus (qw queries per wave) over the items of `a`
nvdb_status launch_scan_parts(nvdb_hip_ctx* c, hipStream_t s, uint32_t qw, bool staged, uint32_t k, const ScanArgs& a);

// The probe search proper over the table off[0 .. nparts]: the caller has validated the context, nq > 0 and 0 < k <= 64.
// msel != nullptr: the masked search (the caller has checked mask_of against the resident planes).  Replaces c->stats (path 4).
nvdb_status parts_search(nvdb_hip_ctx* c, const uint64_t* off, uint32_t nparts, const float* queries, uint32_t nq, uint32_t k, const uint32_t* probe,
                         uint32_t nprobe, const MaskSel* msel, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nvdb_hip_timing* timing);

// nvdb_hip_search_batch_masked behind its argument checks (nvdb_masked_flat.cpp): the MFMA filter route where the plan takes it
nvdb_status masked_flat_search(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t k, const uint32_t* mask_of, uint64_t* out_ids, float* out_scores,
                               uint32_t* out_counts, nvdb_hip_timing* timing);

// the context holds a corpus and a partition table
nvdb_status parts_args(nvdb_hip_ctx* c, const char* who);

}  // namespace nvdbhip
