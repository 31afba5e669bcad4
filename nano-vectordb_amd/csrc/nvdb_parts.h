// nvdb_parts.h -- what the drivers of the probe path share (nvdb_partitions.cpp holds the definitions; the users are the probe
// search there, the partition range scan nvdb_range_parts.cpp, the probe search for any k nvdb_parts_anyk.cpp and the masked flat
// bootstrap nvdb_masked_flat.cpp): the state behind nvdb_hip_ctx::parts, the kernel build a corpus takes and the dispatch to it
// (parts_dispatch), one pass's set-up (parts_pass: work list, workspace, pinned image, copies), the launches of a pass by class
// (parts_scan_classes), the bracket of a call that runs several passes (parts_call_begin / parts_call_end) and the argument
// checks of the top-k entry points (parts_topk_args).  The work list itself is plain C++: parts_worklist.h.  Internal.
#pragma once
#include <functional>
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
  PartScratch list;                                // the work list of the current pass (parts_worklist.h)
  std::vector<uint32_t> probe_tmp;
  std::vector<uint64_t> coarse_ids, rows_union;
  std::vector<float> coarse_scores;
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

// pw_probes (parts_worklist.h) into the PartState's scratch; an entry >= nparts -> NVDB_ERR_INVALID.  rows_union (optional, nq
// entries): the rows of every query's probed union.
nvdb_status parts_probes(nvdb_hip_ctx* c, const char* who, const uint64_t* off, uint32_t nparts, uint32_t nq, const uint32_t* probe, uint32_t nprobe,
                         uint64_t* rows_union);

// The image of a work list on the device (meta): [items | qidx | dst | cbeg | masked: mask_of | extra], as device addresses.
struct PartImage {
  size_t bytes = 0;
  const PartItem* items = nullptr;
  const uint32_t *qidx = nullptr, *dst = nullptr, *cbeg = nullptr, *extra = nullptr;
  PartMask mk{nullptr, nullptr, 0u};
};

// One pass: queries q0 .. q0 + b of a batch whose probe table parts_probes has taken, over the table off[0 .. nparts].
struct PartPass {
  // what the caller sets
  const uint64_t* off = nullptr;
  uint32_t nparts = 0, q0 = 0, b = 0, nprobe = 0;
  uint32_t slot_cap = 0;                           // an (item, query) gets min(slot_cap, segment rows) candidate slots
  const MaskSel* msel = nullptr;                   // the BATCH's (nullptr: unmasked): the pass takes mask_of + q0
  const float* queries = nullptr;                  // the BATCH's, host memory: rows q0 .. go to ps->q; nullptr: they are on the device already
  const uint32_t* extra = nullptr;                 // words behind the work list in the image (the hook may set them)
  uint32_t extra_words = 0;
  bool skip_empty = false;                         // a list without candidate slots: return after building it (wl.total == 0), nothing staged
  bool time_copies = false;                        // record ps->ev[0] / ev[1] around the two copies
  // what parts_pass leaves
  PartList wl;
  PartImage im;
};

// The set-up of a pass on stream s: build the work list (qg_max = PART_WAVES * pb.qw_max), run `between` (optional: what a caller
// does between list and image -- grow buffers of its own, rewrite items, set p.extra), grow cand and q, stage the pinned image,
// enqueue its copy to meta and, where p.queries is given, the queries' copy to ps->q.
using PartPassHook = std::function<nvdb_status(PartPass&)>;
nvdb_status parts_pass(nvdb_hip_ctx* c, hipStream_t s, const char* who, const PartBuild& pb, PartPass& p, const PartPassHook& between = nullptr);

// The launches of a staged pass: the three classes of group size, widest first (the longest items start early), class cl on the
// QW = min(pb.qw_max, 1 << cl) build.  launch(qw, ScanArgs) -> nvdb_status is launch_scan_parts or launch_range_parts with the
// caller's k or radius; q32: the pass's queries on the device.  Adds the launches made to `launches`.
template <class Launch>
nvdb_status parts_scan_classes(nvdb_hip_ctx* c, const PartBuild& pb, const PartImage& im, const float* q32, uint32_t& launches, Launch&& launch) {
  const PartState* ps = c->parts;
  const PartItem* it = im.items;
  for (int cl = 2; cl >= 0; --cl) {
    const uint32_t n_cl = static_cast<uint32_t>(ps->list.items[cl].size());
    if (!n_cl) continue;
    const ScanArgs a{it, n_cl, im.qidx, im.dst, q32, static_cast<Cand*>(ps->cand.p), im.mk};
    if (nvdb_status st = launch(std::min<uint32_t>(pb.qw_max, 1u << cl), a)) return st;
    it += n_cl;
    ++launches;
  }
  return NVDB_OK;
}

// The bracket of a call that runs its passes between two events on c->stream (the range scan, the any-k search).  begin: sets
// the device, records event 60, replaces c->stats by an empty record of `path`, clears what nvdb_hip_search_check reads (it
// describes flat searches).  end: records event 62, synchronises, adds the span to timing->kernel_ms (the passes' copies ride
// inside: they alternate with the launches) and fills total_ms / threads / nwarps / shmem_bytes.
nvdb_status parts_call_begin(nvdb_hip_ctx* c, uint32_t path);
nvdb_status parts_call_end(nvdb_hip_ctx* c, nvdb_hip_timing* timing);

// entries from .. k of nq output rows become "no entry" (~0, -inf); counts (optional, nq entries) become 0
void pad_rows(uint32_t nq, uint32_t k, uint32_t from, uint64_t* out_ids, float* out_scores, uint32_t* counts = nullptr);

// What the top-k entry points of the probe path check alike, in one order (an earlier failure wins): corpus and table, ivf:
// centroids, timing zeroed, nq == 0 || k == 0 answered, k <= kmax (kmax = 0: any k), null pointers, masked: mask_of, nprobe == 0
// answered with padding, !ivf: null probe table.  *done: the call is answered (an error, or nothing to search).
nvdb_status parts_topk_args(nvdb_hip_ctx* c, const char* who, bool ivf, uint32_t kmax, const float* queries, uint32_t nq, uint32_t k, const uint32_t* probe,
                            uint32_t nprobe, const MaskSel* msel, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nvdb_hip_timing* timing, bool* done);

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
