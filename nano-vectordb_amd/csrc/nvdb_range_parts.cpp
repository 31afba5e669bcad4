// nvdb_range_parts.cpp -- range search on the probe path (DESIGN.md section 4 "range search"): every row of a query's probed
// partitions that is live in its mask and whose reference-order score reaches its radius.  Per sub-batch of queries:
//   pass          parts_pass (nvdb_parts.h) with uncapped slots -- an (item, query) slab holds as many entries as its segment has rows -- and the
//                 sub-batch's radii behind the work list in the image
//   scan          parts_scan_classes: range_parts_kernel appends Cand{score, row} to the slabs and pads them (kernels_range_parts.h)
//   tail          count per query -> host: exclusive scan -> range_tail (nvdb_range.h): slab runs, collect keys (score, position), sort, emit
// The host cuts a batch into consecutive query sub-batches whose candidate blocks stay within half of largek_budget_mb (the other
// half is the key slabs') and below 2^32 entries (rp_cut); packed results are appended in query order, so the caller never sees the cut.
// Entry points: nvdb_hip_range_search_partitions / nvdb_hip_range_search_ivf; nvdb_hip_range_search_masked (nvdb_range.cpp) sends
// what its filter route cannot answer here, the corpus as one implicit partition.
#include "nvdb_range.h"
#include "kernels_range_parts.h"

namespace nvdbhip {

nvdb_status launch_range_parts(nvdb_hip_ctx* c, hipStream_t s, uint32_t qw, bool staged, const float* radius, const ScanArgs& a) {
  return parts_dispatch(c, qw, staged, a.mk.mask_of != nullptr, [&](auto dt, auto w, auto al, auto st, auto mk) {
    return parts_launch(c, s, range_parts_kernel<dt(), w(), al(), st(), mk()>, w(), st(), a.nitems, a.items, a.qidx, a.dst, a.q32, radius, a.cand, a.mk);
  });
}

nvdb_status range_parts_core(nvdb_hip_ctx* c, hipStream_t s, const char* who, const uint64_t* off, uint32_t nparts, const float* queries, const float* radius,
                             uint32_t nr, const uint32_t* probe, uint32_t nprobe, const MaskSel* msel, const uint32_t* qmap, std::vector<uint64_t>& cnt,
                             uint64_t base, RangeOut& out) {
  PartState* ps = c->parts;
  const PartBuild pb = parts_build(c);
  if (!pb.qw_max) return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": dim too large for the query staging");
  nvdb_status st;

  // every query's block: the rows of its probed union (and the probe table's check, before anything is launched)
  std::vector<uint64_t> block(nr, 0);
  if ((st = parts_probes(c, who, off, nparts, nr, probe, nprobe, block.data()))) return st;
  // largek_budget_mb bounds what a launch set holds: half of it for the candidate blocks, half for the key slabs of a run (a single
  // query's block, or a single slab, is taken whatever the budget says: neither can be cut)
  const uint64_t budget_entries = (static_cast<uint64_t>(c->opt_largek_budget_mb) << 20) / (2 * sizeof(Cand));
  const uint64_t slab_max = budget_entries;
  auto qnum = [&](uint32_t i) { return qmap ? qmap[i] : i; };
  uint32_t pos = 0;                                  // cnt[0 .. pos) are summed in `before`
  uint64_t before = 0;
  std::vector<uint32_t> hc;
  std::vector<uint64_t> out_off;
  for (uint32_t q0 = 0; q0 < nr;) {
    const uint32_t q1 = rp_cut(block.data(), nr, q0, budget_entries);
    if (q1 == q0) return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": one query's probed union holds 2^32 rows or more");
    const uint32_t b = q1 - q0;
    PartPass p;
    p.off = off; p.nparts = nparts; p.q0 = q0; p.b = b; p.nprobe = nprobe; p.slot_cap = 0xFFFFFFFFu;
    p.msel = msel; p.queries = queries;
    p.extra = reinterpret_cast<const uint32_t*>(radius + q0); p.extra_words = b;
    p.skip_empty = true;
    if ((st = parts_pass(c, s, who, pb, p, [&](PartPass&) { return ensure(c, c->rg_pcnt, static_cast<size_t>(b) * 4); }))) return st;
    const PartList& wl = p.wl;
    const PartImage& im = p.im;
    hc.assign(b, 0u);
    if (wl.total) {
      uint32_t launches = 0;
      if ((st = parts_scan_classes(c, pb, im, static_cast<const float*>(ps->q.p), launches, [&](uint32_t qw, const ScanArgs& a) {
            return launch_range_parts(c, s, qw, pb.staged, reinterpret_cast<const float*>(im.extra), a);
          })))
        return st;
      c->stats.chunks += launches;
      rparts_count_kernel<<<b, 256, 0, s>>>(static_cast<const Cand*>(ps->cand.p), im.cbeg, static_cast<uint32_t*>(c->rg_pcnt.p));
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(hc.data(), c->rg_pcnt.p, static_cast<size_t>(b) * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipStreamSynchronize(s));            // (also: the pinned image and the host vectors are free for the next sub-batch)
      c->stats.rows_scanned += wl.rows_read;
    }
    // the slices' places in the packed arrays: behind every earlier query of the caller's sub-batch
    out_off.assign(b, 0);
    for (uint32_t i = 0; i < b; ++i) {
      const uint32_t qn = qnum(q0 + i);
      cnt[qn] = hc[i];
      c->stats.candidates += hc[i];
      while (pos < qn) before += cnt[pos++];
      out_off[i] = base + before;
    }
    while (pos <= qnum(q1 - 1)) before += cnt[pos++];
    q0 = q1;
    if (!wl.total) continue;
    if (!reserve_packed(c, s, out, base + before, &st)) { if (st) return st; continue; }
    const Cand* cand = static_cast<const Cand*>(ps->cand.p);
    st = range_tail(c, s, who, hc.data(), b, out_off.data(), slab_max,
        [&](const std::vector<RangeDesc>& run, const RangeDesc* desc, uint32_t* taken, unsigned long long* slab) {
          const uint32_t nrun = static_cast<uint32_t>(run.size());
          uint32_t max_len = 0;                          // the longest block of the run
          for (const RangeDesc& d : run) max_len = std::max(max_len, ps->list.cbeg[d.q + 1] - ps->list.cbeg[d.q]);
          const uint32_t G = std::max<uint32_t>(1, std::min<uint32_t>((max_len + 1023u) / 1024u, (8u * static_cast<uint32_t>(c->num_cu) + nrun - 1) / nrun));
          rparts_collect_kernel<<<dim3(G, nrun), 256, 0, s>>>(cand, im.cbeg, desc, taken, slab);
        },
        [&](const std::vector<RangeDesc>& run, uint32_t max_cnt, const RangeDesc* desc, const unsigned long long* slab) {
          rparts_emit_kernel<<<dim3((max_cnt + 255u) / 256u, static_cast<uint32_t>(run.size())), 256, 0, s>>>(
              slab, desc, cand, im.cbeg, c->row_base, static_cast<unsigned long long*>(c->rg_ids.p), static_cast<float*>(c->rg_scores.p));
        });
    if (st) return st;
    HIPCHK(c, hipStreamSynchronize(s));              // the next sub-batch rewrites the blocks, the image and the descriptors
  }
  return NVDB_OK;
}

namespace {

// the probe forms' driver: the arguments are validated, nq > 0 and nprobe > 0
nvdb_status range_parts_search(nvdb_hip_ctx* c, const char* who, const float* queries, uint32_t nq, const float* radius, const uint32_t* probe, uint32_t nprobe,
                               const MaskSel* msel, uint64_t* out_lims, nvdb_hip_timing* timing) {
  PartState* ps = c->parts;
  if (nvdb_status st = parts_call_begin(c, RANGE_STAT_PARTS)) return st;
  hipStream_t s = c->stream;
  RangeOut out;
  out.budget_entries = (static_cast<uint64_t>(c->opt_range_max_mb) << 20) / 12;
  std::vector<uint64_t> cnt(nq, 0);
  if (nvdb_status st = range_parts_core(c, s, who, ps->offsets.data(), static_cast<uint32_t>(ps->offsets.size() - 1), queries, radius, nq, probe, nprobe, msel, nullptr,
                                        cnt, 0, out))
    return st;
  const uint64_t total = rp_scan(cnt.data(), nq, 0, nullptr, out_lims + 1);
  if (nvdb_status st = parts_call_end(c, timing)) return st;
  if (!out.pack)
    return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string(total) + " results (" + std::to_string((total * 12 + (1u << 20) - 1) >> 20) +
                                            " MB packed) exceed option range_max_mb = " + std::to_string(c->opt_range_max_mb) + "; out_lims is complete");
  c->range_total = total;
  c->range_valid = true;
  return NVDB_OK;
}

// what the two probe forms check alike; *done: the call is answered (an error, or a batch without queries / probes)
nvdb_status range_parts_args(nvdb_hip_ctx* c, const char* who, bool ivf, const float* queries, uint32_t nq, const float* radius, uint32_t nprobe,
                             const MaskSel* msel, uint64_t* out_lims, nvdb_hip_timing* timing, bool* done) {
  *done = true;
  if (!c) return NVDB_ERR_INVALID;
  if (!out_lims || (nq > 0 && (!queries || !radius)))
    return fail(c, NVDB_ERR_INVALID, !out_lims ? std::string(who) + ": null out_lims" : queries ? std::string(who) + ": null radius" : "Null query");
  if (nvdb_status st = parts_args(c, who)) return st;
  if (ivf && !c->parts->have_centroids) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": no centroids (nvdb_hip_set_centroids)");
  if (msel && nq > 0)
    if (nvdb_status st = mask_args(c, msel->mask_of, nq, who)) return st;
  if (timing) std::memset(timing, 0, sizeof(*timing));
  out_lims[0] = 0;
  c->range_valid = false;                                            // a new range search of any kind replaces the held result
  c->range_total = 0;
  if (nq == 0 || nprobe == 0) {
    for (uint32_t q = 0; q < nq; ++q) out_lims[q + 1] = 0;
    c->range_valid = true;
    return NVDB_OK;
  }
  *done = false;
  return NVDB_OK;
}

}  // namespace
}  // namespace nvdbhip

extern "C" {

nvdb_status nvdb_hip_range_search_partitions(nvdb_hip_ctx* c, const float* queries, uint32_t nq, const float* radius, const uint32_t* probe, uint32_t nprobe,
                                             const uint32_t* mask_of, int masked, uint64_t* out_lims, nvdb_hip_timing* timing) {
  const char* who = "range_search_partitions";
  const MaskSel msel{mask_of};
  bool done;
  nvdb_status st = range_parts_args(c, who, false, queries, nq, radius, nprobe, masked ? &msel : nullptr, out_lims, timing, &done);
  if (st || done) return st;
  if (!probe) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": null probe table");
  return range_parts_search(c, who, queries, nq, radius, probe, nprobe, masked ? &msel : nullptr, out_lims, timing);
}

nvdb_status nvdb_hip_range_search_ivf(nvdb_hip_ctx* c, const float* queries, uint32_t nq, const float* radius, uint32_t nprobe, const uint32_t* mask_of, int masked,
                                      uint64_t* out_lims, uint32_t* out_probe, nvdb_hip_timing* timing) {
  const char* who = "range_search_ivf";
  const MaskSel msel{mask_of};
  bool done;
  nvdb_status st = range_parts_args(c, who, true, queries, nq, radius, nprobe, masked ? &msel : nullptr, out_lims, timing, &done);
  if (st || done) return st;
  uint32_t np = 0;
  if ((st = parts_coarse(c, who, queries, nq, nprobe, out_probe, timing, np))) return st;
  return range_parts_search(c, who, queries, nq, radius, c->parts->probe_tmp.data(), np, masked ? &msel : nullptr, out_lims, timing);
}

}  // extern "C"
