// nvdb_parts_anyk.cpp -- the probe search for any k (DESIGN.md section 4 "probe search, any k"): the exact top-k of every query's
// probed union, live rows only under a mask, for k beyond the wavefront-resident lists of nvdb_hip_search_partitions.  k <= 64 IS
// that call.  Otherwise, per sub-batch of queries:
//   pass          parts_pass (nvdb_parts.h) with uncapped slots, as the range scan: an (item, query) slab holds as many entries as its segment has rows;
//                 between list and image: the sub-batch's plan (pa_plan), its words behind the work list, the device output grown
//   scan          parts_scan_classes: range_parts_kernel with every radius -inf appends Cand{score, row} of every live row and pads the slabs (kernels_range_parts.h)
//   select        parts_anyk_select_kernel: count, radix select of the k-th key, collect, and for slabs that fit the LDS sort + emit (kernels_parts_anyk.h)
//   long slabs    bitonic_global_step_kernel launches per slab length, parts_anyk_emit_kernel
//   copy          the sub-batch's rows of the device output into the caller's arrays
// The host cuts a batch into consecutive query sub-batches with pa_cut (parts_anyk_plan.h): candidate blocks within half of
// largek_budget_mb, the long slabs within the other half; the caller never sees the cut.
// Entry points: nvdb_hip_search_partitions_anyk / nvdb_hip_search_ivf_anyk (nvdb_hip_ivf_search_anyk, nvdb_ivf.cpp, maps the ids).
#include "nvdb_range.h"
#include "kernels_parts_anyk.h"

namespace nvdbhip {

namespace {

constexpr uint32_t PARTS_STAT_ANYK = 8;                              // nvdb_hip_scan_stats::path

// the search proper for k > 64: the arguments are validated, nq > 0 and nprobe > 0
nvdb_status parts_anyk_search(nvdb_hip_ctx* c, const char* who, const float* queries, uint32_t nq, uint32_t k, const uint32_t* probe, uint32_t nprobe,
                              const MaskSel* msel, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nvdb_hip_timing* timing) {
  PartState* ps = c->parts;
  const uint64_t* off = ps->offsets.data();
  const uint32_t nparts = static_cast<uint32_t>(ps->offsets.size() - 1);
  const PartBuild pb = parts_build(c);
  if (!pb.qw_max) return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": dim too large for the query staging");
  nvdb_status st;
  // every query's block: the rows of its probed union (and the probe table's check, before anything is launched)
  std::vector<uint64_t> block(nq, 0);
  if ((st = parts_probes(c, who, off, nparts, nq, probe, nprobe, block.data()))) return st;

  if ((st = parts_call_begin(c, PARTS_STAT_ANYK))) return st;
  hipStream_t s = c->stream;

  const uint64_t budget_entries = (static_cast<uint64_t>(c->opt_largek_budget_mb) << 20) / (2 * sizeof(Cand));
  std::vector<uint32_t> extra, hcnt, hraw;
  PaPlan plan;
  for (uint32_t q0 = 0; q0 < nq;) {
    const uint32_t q1 = pa_cut(block.data(), nq, q0, k, budget_entries);
    if (q1 == q0) return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": one query's probed union holds 2^32 rows or more");
    const uint32_t b = q1 - q0;
    uint64_t* ids0 = out_ids + static_cast<size_t>(q0) * k;
    float* sc0 = out_scores + static_cast<size_t>(q0) * k;
    uint32_t nlong = 0;
    size_t out_entries = 0;
    PartPass p;
    p.off = off; p.nparts = nparts; p.q0 = q0; p.b = b; p.nprobe = nprobe; p.slot_cap = 0xFFFFFFFFu;
    p.msel = msel; p.queries = queries;
    p.skip_empty = true;
    st = parts_pass(c, s, who, pb, p, [&](PartPass& pp) -> nvdb_status {
      if (!pa_plan(block.data() + q0, b, k, plan)) return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 results for one query");
      nlong = static_cast<uint32_t>(plan.longs.size());
      // behind the work list in the pinned image: [radius (-inf) b | slab_off 2 b | long lists 4 nlong]
      extra.assign(static_cast<size_t>(b) * 3 + static_cast<size_t>(nlong) * 4, 0xFF800000u);
      std::copy(plan.slab_off.begin(), plan.slab_off.end(), extra.begin() + b);
      if (nlong) std::memcpy(extra.data() + static_cast<size_t>(b) * 3, plan.longs.data(), static_cast<size_t>(nlong) * sizeof(PaLong));
      pp.extra = extra.data(); pp.extra_words = static_cast<uint32_t>(extra.size());
      out_entries = static_cast<size_t>(b) * plan.out_k;
      nvdb_status e;
      if ((e = ensure(c, ps->out_ids, out_entries * 8))) return e;
      if ((e = ensure(c, ps->out_scores, out_entries * 4))) return e;
      if ((e = ensure(c, ps->out_counts, static_cast<size_t>(b) * 4))) return e;
      if ((e = ensure(c, c->rg_pcnt, static_cast<size_t>(b) * 4))) return e;
      return ensure(c, c->rg_slab, static_cast<size_t>(plan.slab_keys) * 8);
    });
    if (st) return st;
    const PartList& wl = p.wl;
    const PartImage& im = p.im;
    if (!wl.total) {                                                   // no row in any union of the sub-batch
      pad_rows(b, k, 0, ids0, sc0, out_counts ? out_counts + q0 : nullptr);
      q0 = q1;
      continue;
    }
    const float* d_radius = reinterpret_cast<const float*>(im.extra);
    const uint32_t* d_slab_off = im.extra + b;
    const PaLong* d_longs = reinterpret_cast<const PaLong*>(im.extra + static_cast<size_t>(b) * 3);
    const Cand* cand = static_cast<const Cand*>(ps->cand.p);
    unsigned long long* d_ids = static_cast<unsigned long long*>(ps->out_ids.p);
    float* d_scores = static_cast<float*>(ps->out_scores.p);
    uint32_t* d_counts = static_cast<uint32_t*>(ps->out_counts.p);
    unsigned long long* slab = static_cast<unsigned long long*>(c->rg_slab.p);
    uint32_t launches = 0;
    if ((st = parts_scan_classes(c, pb, im, static_cast<const float*>(ps->q.p), launches,
                                 [&](uint32_t qw, const ScanArgs& a) { return launch_range_parts(c, s, qw, pb.staged, d_radius, a); })))
      return st;
    c->stats.chunks += launches;
    const size_t lds = PA_LDS_HEAD + static_cast<size_t>(plan.lds_keys) * 8;
    if (lds > 64 * 1024)
      if ((st = raise_lds_limit(c, reinterpret_cast<const void*>(parts_anyk_select_kernel), PA_LDS_HEAD + static_cast<size_t>(PA_LDS_KEYS) * 8))) return st;
    parts_anyk_select_kernel<<<b, PA_THREADS, lds, s>>>(cand, im.cbeg, k, plan.out_k, c->row_base, d_slab_off, slab, d_ids, d_scores, d_counts,
                                                        static_cast<uint32_t*>(c->rg_pcnt.p));
    HIPCHK(c, hipGetLastError());
    for (uint32_t a = 0; a < nlong;) {                                 // slabs of one length side by side: one sort per length
      uint32_t z = a;
      while (z < nlong && plan.longs[z].K2 == plan.longs[a].K2) ++z;
      const uint64_t first = (static_cast<uint64_t>(plan.longs[a].off_hi) << 32) | plan.longs[a].off_lo;
      if ((st = launch_sort_keys(c, s, slab + first, plan.longs[a].K2, z - a))) return st;
      a = z;
    }
    for (uint32_t a = 0; a < nlong; a += 32768u) {                     // (the lists are one grid dimension of the launch)
      const uint32_t n_l = std::min<uint32_t>(32768u, nlong - a);
      parts_anyk_emit_kernel<<<dim3((plan.out_k + 255u) / 256u, n_l), 256, 0, s>>>(slab, d_longs + a, cand, im.cbeg, d_counts, plan.out_k, c->row_base, d_ids, d_scores);
      HIPCHK(c, hipGetLastError());
    }
    // the sub-batch's rows into the caller's arrays; what lies beyond the device rows' width is padding
    if (plan.out_k == k) {
      HIPCHK(c, hipMemcpyAsync(ids0, d_ids, out_entries * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipMemcpyAsync(sc0, d_scores, out_entries * 4, hipMemcpyDeviceToHost, s));
    } else {
      HIPCHK(c, hipMemcpy2DAsync(ids0, static_cast<size_t>(k) * 8, d_ids, static_cast<size_t>(plan.out_k) * 8, static_cast<size_t>(plan.out_k) * 8, b, hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipMemcpy2DAsync(sc0, static_cast<size_t>(k) * 4, d_scores, static_cast<size_t>(plan.out_k) * 4, static_cast<size_t>(plan.out_k) * 4, b, hipMemcpyDeviceToHost, s));
    }
    hcnt.resize(b);
    hraw.resize(b);
    HIPCHK(c, hipMemcpyAsync(hcnt.data(), d_counts, static_cast<size_t>(b) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(hraw.data(), c->rg_pcnt.p, static_cast<size_t>(b) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));                // (the next sub-batch rewrites the blocks, the image and the device output)
    pad_rows(b, k, plan.out_k, ids0, sc0);
    if (out_counts) std::copy(hcnt.begin(), hcnt.end(), out_counts + q0);
    for (uint32_t i = 0; i < b; ++i) c->stats.candidates += hraw[i];
    c->stats.rows_scanned += wl.rows_read;
    q0 = q1;
  }
  if ((st = parts_call_end(c, timing))) return st;
  if (timing) timing->K = k;
  return NVDB_OK;
}

}  // namespace
}  // namespace nvdbhip

extern "C" {

nvdb_status nvdb_hip_search_partitions_anyk(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t k, const uint32_t* probe, uint32_t nprobe,
                                            const uint32_t* mask_of, int masked, uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                            nvdb_hip_timing* timing) {
  if (k <= WAVE_KMAX)                                                  // the wavefront-resident lists answer it: the twin, bit for bit
    return masked ? nvdb_hip_search_partitions_masked(c, queries, nq, k, probe, nprobe, mask_of, out_ids, out_scores, out_counts, timing)
                  : nvdb_hip_search_partitions(c, queries, nq, k, probe, nprobe, out_ids, out_scores, out_counts, timing);
  const char* who = "search_partitions_anyk";
  const MaskSel msel{mask_of};
  bool done;
  const nvdb_status st = parts_topk_args(c, who, false, 0, queries, nq, k, probe, nprobe, masked ? &msel : nullptr, out_ids, out_scores, out_counts, timing, &done);
  if (st || done) return st;
  return parts_anyk_search(c, who, queries, nq, k, probe, nprobe, masked ? &msel : nullptr, out_ids, out_scores, out_counts, timing);
}

nvdb_status nvdb_hip_search_ivf_anyk(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe, const uint32_t* mask_of, int masked,
                                     uint64_t* out_ids, float* out_scores, uint32_t* out_counts, uint32_t* out_probe, nvdb_hip_timing* timing) {
  if (k <= WAVE_KMAX)
    return masked ? nvdb_hip_search_ivf_masked(c, queries, nq, k, nprobe, mask_of, out_ids, out_scores, out_counts, out_probe, timing)
                  : nvdb_hip_search_ivf(c, queries, nq, k, nprobe, out_ids, out_scores, out_counts, out_probe, timing);
  const char* who = "search_ivf_anyk";
  const MaskSel msel{mask_of};
  bool done;
  nvdb_status st = parts_topk_args(c, who, true, 0, queries, nq, k, nullptr, nprobe, masked ? &msel : nullptr, out_ids, out_scores, out_counts, timing, &done);
  if (st || done) return st;
  uint32_t np = 0;
  if ((st = parts_coarse(c, who, queries, nq, nprobe, out_probe, timing, np))) return st;
  return parts_anyk_search(c, who, queries, nq, k, c->parts->probe_tmp.data(), np, masked ? &msel : nullptr, out_ids, out_scores, out_counts, timing);
}

}  // extern "C"
