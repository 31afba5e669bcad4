// nvdb_masked_flat.cpp -- the masked flat top-k (nvdb_hip_search_batch_masked) on the MFMA filter route (DESIGN.md section 4 "Row
// masks").  The flat search's running thresholds come from the k-th best filter score of ALL rows, so a dead row above the bar would
// push live rows out; this route makes its bar from live rows only and then streams the corpus once at FIXED thresholds, as the
// range search does.  Per sub-batch of <= 1024 queries, all on the context's stream, no host synchronisation before the verdict:
//   1. prefix rank   per distinct plane of the sub-batch, the prefix [0, P) that holds L live rows (masked_plan.h; P = n where the
//                    plane holds fewer) and the bootstrap's work items over it (masked_prefix_rank_kernel)
//   2. bootstrap     the exact masked top-k over [0, P): the masked partition scan, every plane a partition of its own (queries of
//                    different planes never share a group), then select_parts_kernel -- into the output staging.  The pass is
//                    parts_pass / parts_scan_classes (nvdb_parts.h) with the queries on the device already; its hook turns the
//                    placeholder segments into what the prefix-rank kernel fills in
//   3. bar           radius = the k-th bootstrap score; fewer than k live rows in [0, n), or a plane with too few for a bar
//                    (mp_boot_final): NaN -- the bootstrap's answer is final, the query files nothing in the filter pass
//   4. main pass     range_filter_pass (nvdb_range.cpp) at radius = bar under the queries' planes: every live row whose exact score
//                    reaches the bar, ordered (score desc, row asc); ties at the bar are all kept
//   5. top-k         the first k of every kept list over the bootstrap's answer (masked_topk_from_kept_kernel)
//   6. flagged       list overflow, non-finite query or bar, wave-log overflow, violated bound: those queries alone, as a compact
//                    batch, on the masked partition scan over the whole corpus
// Option path = 1, and the automatic rule below MP_AUTO_MIN_ROWS rows, is the partition scan alone: the call as it was before this route.
#include "nvdb_range.h"
#include "kernels_masked_topk.h"

namespace nvdbhip {

namespace {

// does this sub-batch take the filter route?  (path = 2 without a filter was refused before anything was enqueued)
// mask: the sub-batch's planes (resolved)
bool sub_filters(const nvdb_hip_ctx* c, uint32_t b, uint32_t k, const uint32_t* mask) {
  if (c->opt_path == 1) return false;
  if (c->opt_path == 2) return true;
  if (!mp_auto_filter(filter_supported(c), b, c->opt_min_filter_batch, c->n, c->opt_chunk0)) return false;
  const PartBuild pb = parts_build(c);
  if (!pb.qw_max) return false;
  // query groups and (estimated) live rows per distinct plane: what the two routes would walk
  const uint32_t qg_max = PART_WAVES * pb.qw_max;
  std::vector<uint32_t> count(static_cast<size_t>(c->nmasks) + 1, 0u), groups;
  std::vector<uint64_t> live;
  for (uint32_t q = 0; q < b; ++q) ++count[mask[q] == ROW_MASK_NONE ? c->nmasks : mask[q]];
  for (uint32_t m = 0; m <= c->nmasks; ++m) {
    if (!count[m]) continue;
    groups.push_back((count[m] + qg_max - 1) / qg_max);
    live.push_back(m < c->mask_live.size() && m < c->nmasks ? c->mask_live[m] : c->n);
  }
  const uint32_t cap = c->opt_cap > 0 ? std::max<uint32_t>(2u, std::min<uint32_t>(static_cast<uint32_t>(c->opt_cap), SELECT_MAX_CAP)) : SELECT_MAX_CAP;   // (plan_range's)
  return mp_filter_pays(c->n, k, cap, static_cast<uint32_t>(groups.size()), groups.data(), live.data());
}

void add_stats(nvdb_hip_scan_stats& into, const nvdb_hip_scan_stats& s) {
  into.chunks += s.chunks;
  into.rows_scanned += s.rows_scanned;
  into.candidates += s.candidates;
}

// host scratch of one call
struct MaskedScratch {
  std::vector<uint32_t> slot_mask, slot_count, lut, extra, bootcnt, prefix, flagged, fl_m, fl_cnt;
  std::vector<uint64_t> off, fl_ids;
  std::vector<float> fl_q, fl_sc;
  FilterVerdict v;
};

// the masked partition scan over the whole corpus for nf queries in host memory (the call as it was before the filter route);
// its statistics are ADDED to *acc where given (parts_search replaces c->stats)
nvdb_status scan_whole(nvdb_hip_ctx* c, const float* queries, uint32_t nf, uint32_t k, const uint32_t* mask_of, uint64_t* out_ids, float* out_scores,
                       uint32_t* out_counts, nvdb_hip_timing* timing, nvdb_hip_scan_stats* acc) {
  const uint64_t whole[2] = {0, c->n};
  c->parts->probe_tmp.assign(nf, 0u);
  const MaskSel msel{mask_of};
  const nvdb_hip_scan_stats keep = c->stats;
  const nvdb_status st = parts_search(c, whole, 1, queries, nf, k, c->parts->probe_tmp.data(), 1, &msel, out_ids, out_scores, out_counts, timing);
  if (acc) {
    const nvdb_hip_scan_stats mine = c->stats;
    c->stats = keep;
    if (!st) add_stats(*acc, mine);
  }
  return st;
}

// one sub-batch of b queries on the filter route.  queries / mask: host (mask resolved: NULL -> plane 0); dq / dmask: the same on the device
nvdb_status filter_sub(nvdb_hip_ctx* c, hipStream_t s, const RangePlan& p, const float* queries, const uint32_t* mask, const float* dq, const uint32_t* dmask,
                       uint32_t b, uint32_t k, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, uint32_t& violations, MaskedScratch& sc) {
  PartState* ps = c->parts;
  nvdb_status st;
  const uint32_t n = static_cast<uint32_t>(c->n);
  const PartBuild pb = parts_build(c);
  if (!pb.qw_max) return fail(c, NVDB_ERR_UNSUPPORTED, "search_batch_masked: dim too large for the query staging");
  const uint32_t qg_max = PART_WAVES * pb.qw_max;

  // 1. the distinct planes of the sub-batch ("no mask" among them) as the partitions of the bootstrap's work list
  sc.lut.assign(static_cast<size_t>(c->nmasks) + 1, 0xFFFFFFFFu);
  sc.slot_mask.clear();
  sc.slot_count.clear();
  ps->probe_tmp.resize(b);
  for (uint32_t q = 0; q < b; ++q) {
    const uint32_t li = mask[q] == ROW_MASK_NONE ? c->nmasks : mask[q];
    if (sc.lut[li] == 0xFFFFFFFFu) { sc.lut[li] = static_cast<uint32_t>(sc.slot_mask.size()); sc.slot_mask.push_back(mask[q]); sc.slot_count.push_back(0u); }
    ps->probe_tmp[q] = sc.lut[li];
    ++sc.slot_count[sc.lut[li]];
  }
  const uint32_t nslots = static_cast<uint32_t>(sc.slot_mask.size());
  uint32_t groups = 0;
  for (uint32_t j = 0; j < nslots; ++j) groups += (sc.slot_count[j] + qg_max - 1) / qg_max;
  const uint32_t nseg = mp_segments(c->n, groups, static_cast<uint32_t>(c->num_cu));
  // every slot a partition of nseg * PART_SEG_ROWS placeholder rows: the list builder cuts it into nseg segments, whose rows
  // the prefix-rank kernel sets (nslots <= 1025, nseg <= 256: the placeholders stay far below 2^32)
  const uint64_t span = static_cast<uint64_t>(nseg) * PART_SEG_ROWS;
  sc.off.resize(static_cast<size_t>(nslots) + 1);
  for (uint32_t j = 0; j <= nslots; ++j) sc.off[j] = j * span;
  if ((st = parts_probes(c, "search_batch_masked", sc.off.data(), nslots, b, ps->probe_tmp.data(), 1, nullptr))) return st;
  sc.extra.resize(static_cast<size_t>(nslots) * 2 + b);               // [slot table | every query's slot]
  for (uint32_t j = 0; j < nslots; ++j) { sc.extra[2 * j] = sc.slot_mask[j]; sc.extra[2 * j + 1] = nseg; }
  for (uint32_t q = 0; q < b; ++q) sc.extra[2 * static_cast<size_t>(nslots) + q] = ps->probe_tmp[q];
  const size_t ob_ids = static_cast<size_t>(b) * k * 8, ob_sc = static_cast<size_t>(b) * k * 4;
  const MaskSel msel{mask};
  PartPass pass;
  pass.off = sc.off.data(); pass.nparts = nslots; pass.q0 = 0; pass.b = b; pass.nprobe = 1; pass.slot_cap = k;
  pass.msel = &msel;                                                    // (queries: nullptr -- dq holds them)
  pass.extra = sc.extra.data(); pass.extra_words = static_cast<uint32_t>(sc.extra.size());
  st = parts_pass(c, s, "search_batch_masked", pb, pass, [&](PartPass&) -> nvdb_status {
    for (auto& items : ps->list.items)                                  // a placeholder segment becomes (segment number, nseg, slot + 1)
      for (PartItem& it : items) {
        const uint32_t slot = static_cast<uint32_t>(it.row_lo / span);
        it.row_lo = static_cast<uint32_t>((it.row_lo - slot * span) / PART_SEG_ROWS);
        it.row_hi = nseg;
        it.pad = slot + 1u;
      }
    nvdb_status e;
    if ((e = ensure(c, ps->out_ids, ob_ids))) return e;
    if ((e = ensure(c, ps->out_scores, ob_sc))) return e;
    if ((e = ensure(c, ps->out_counts, static_cast<size_t>(b) * 4))) return e;
    if ((e = ensure(c, c->rg_radius, static_cast<size_t>(b) * 4))) return e;
    return ensure(c, c->rg_idx, static_cast<size_t>(nslots) * 8);       // [prefix | final] per slot
  });
  if (st) return st;
  const PartList& wl = pass.wl;
  const PartImage& im = pass.im;
  // a slot of a segment shorter than k is written in part: what is not written reads as "no entry" (row 0xFFFFFFFF)
  HIPCHK(c, hipMemsetAsync(ps->cand.p, 0xFF, std::max<uint64_t>(wl.total, 1) * sizeof(Cand), s));
  const uint32_t nitems = static_cast<uint32_t>(wl.nitems);
  unsigned long long* d_ids = static_cast<unsigned long long*>(ps->out_ids.p);
  float* d_sc = static_cast<float*>(ps->out_scores.p);
  uint32_t* d_cnt = static_cast<uint32_t*>(ps->out_counts.p);
  float* d_radius = static_cast<float*>(c->rg_radius.p);
  masked_prefix_rank_kernel<<<nslots, MASKED_RANK_THREADS, 0, s>>>(static_cast<const uint32_t*>(c->row_masks.p), static_cast<uint32_t>(rm_words(c->n)), n, k, p.cap,
                                                                   reinterpret_cast<const MaskedSlot*>(im.extra), const_cast<PartItem*>(im.items), nitems,
                                                                   static_cast<uint32_t*>(c->rg_idx.p), static_cast<uint32_t*>(c->rg_idx.p) + nslots);
  HIPCHK(c, hipGetLastError());

  // 2. bootstrap: the masked scan over the prefixes, the select into the output staging
  uint32_t launches = 0;
  if ((st = parts_scan_classes(c, pb, im, dq, launches, [&](uint32_t qw, const ScanArgs& a) { return launch_scan_parts(c, s, qw, pb.staged, k, a); }))) return st;
  select_parts_kernel<<<b, 64, 0, s>>>(static_cast<const Cand*>(ps->cand.p), im.cbeg, k, c->row_base, d_ids, d_sc, d_cnt);
  HIPCHK(c, hipGetLastError());
  // 3. bar
  const uint32_t* d_slot_of = im.extra + 2 * static_cast<size_t>(nslots);
  masked_bar_kernel<<<(b + 255u) / 256u, 256, 0, s>>>(d_sc, d_cnt, d_slot_of, static_cast<const uint32_t*>(c->rg_idx.p) + nslots, k, b, d_radius);
  HIPCHK(c, hipGetLastError());
  sc.bootcnt.resize(b);
  sc.prefix.resize(static_cast<size_t>(nslots) * 2);
  HIPCHK(c, hipMemcpyAsync(sc.bootcnt.data(), d_cnt, static_cast<size_t>(b) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(sc.prefix.data(), c->rg_idx.p, static_cast<size_t>(nslots) * 8, hipMemcpyDeviceToHost, s));

  // 4. main pass (reads the verdict back: the one synchronisation)
  FilterVerdict& v = sc.v;
  if ((st = range_filter_pass(c, s, p, dq, d_radius, b, dmask, v))) return st;
  c->stats.chunks += launches;
  for (uint32_t j = 0; j < nslots; ++j) c->stats.rows_scanned += static_cast<uint64_t>(sc.prefix[j]) * ((sc.slot_count[j] + qg_max - 1) / qg_max);
  for (uint32_t q = 0; q < b; ++q) c->stats.candidates += std::min(v.listcnt[q], p.cap);
  c->stats.bound_violations += v.misc[0];
  violations += v.misc[0];
  sc.flagged.clear();
  const bool all = (v.misc[0] | v.misc[1]) != 0;        // a violated bound: nothing of this pass is trusted; a wave's log overflowed: which queries lost entries is unknown
  for (uint32_t q = 0; q < b; ++q) {
    if (sc.bootcnt[q] < k || sc.prefix[nslots + sc.extra[2 * static_cast<size_t>(nslots) + q]]) continue;   // answered by the bootstrap
    if (all || v.overflow[q] || v.kept[q] < k) sc.flagged.push_back(q);
  }
  c->stats.overflow_queries += all ? (v.misc[1] ? b : 0u) : static_cast<uint32_t>(sc.flagged.size());

  // 5. top-k out of the kept lists
  if (!all) {
    masked_topk_from_kept_kernel<<<b, 64, 0, s>>>(static_cast<const Cand*>(c->cand.p), p.cap, static_cast<const uint32_t*>(c->rg_kept.p),
                                                  static_cast<const uint32_t*>(c->overflow.p), k, c->row_base, d_ids, d_sc, d_cnt);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(out_ids, d_ids, ob_ids, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(out_scores, d_sc, ob_sc, hipMemcpyDeviceToHost, s));
  if (out_counts) HIPCHK(c, hipMemcpyAsync(out_counts, d_cnt, static_cast<size_t>(b) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));

  // 6. the flagged queries alone, a compact batch on the scan
  if (!sc.flagged.empty()) {
    const uint32_t nf = static_cast<uint32_t>(sc.flagged.size());
    sc.fl_q.resize(static_cast<size_t>(nf) * c->dim);
    sc.fl_m.resize(nf);
    sc.fl_ids.resize(static_cast<size_t>(nf) * k);
    sc.fl_sc.resize(static_cast<size_t>(nf) * k);
    sc.fl_cnt.resize(nf);
    for (uint32_t i = 0; i < nf; ++i) {
      std::memcpy(sc.fl_q.data() + static_cast<size_t>(i) * c->dim, queries + static_cast<size_t>(sc.flagged[i]) * c->dim, static_cast<size_t>(c->dim) * 4);
      sc.fl_m[i] = mask[sc.flagged[i]];
    }
    if ((st = scan_whole(c, sc.fl_q.data(), nf, k, sc.fl_m.data(), sc.fl_ids.data(), sc.fl_sc.data(), sc.fl_cnt.data(), nullptr, &c->stats))) return st;
    for (uint32_t i = 0; i < nf; ++i) {
      const size_t d = static_cast<size_t>(sc.flagged[i]) * k, f = static_cast<size_t>(i) * k;
      std::memcpy(out_ids + d, sc.fl_ids.data() + f, static_cast<size_t>(k) * 8);
      std::memcpy(out_scores + d, sc.fl_sc.data() + f, static_cast<size_t>(k) * 4);
      if (out_counts) out_counts[sc.flagged[i]] = sc.fl_cnt[i];
    }
  }
  return NVDB_OK;
}

}  // namespace

nvdb_status masked_flat_search(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t k, const uint32_t* mask_of, uint64_t* out_ids, float* out_scores,
                               uint32_t* out_counts, nvdb_hip_timing* timing) {
  nvdb_status st;
  if (c->opt_path == 2) {                                             // (an unsupported forced route fails before anything is enqueued)
    RangePlan p;
    if ((st = plan_range(*c, std::min<uint32_t>(nq, 1024u), p))) return fail(c, st, p.error);
  }
  std::vector<uint32_t> mask_host(nq, 0u);                            // every query's plane, NULL resolved to plane 0
  if (mask_of) std::copy(mask_of, mask_of + nq, mask_host.begin());
  bool any = false;
  for (uint32_t q0 = 0; q0 < nq; q0 += 1024) any = any || sub_filters(c, std::min<uint32_t>(1024u, nq - q0), k, mask_host.data() + q0);
  if (!any) return scan_whole(c, queries, nq, k, mask_of, out_ids, out_scores, out_counts, timing, nullptr);

  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t qbytes = static_cast<size_t>(nq) * c->dim * 4;
  if ((st = ensure_q32(c, s, qbytes))) return st;
  const hipEvent_t e[3] = {get_event(c, 60), get_event(c, 61), get_event(c, 62)};
  HIPCHK(c, hipEventRecord(e[0], s));
  if ((st = zero_q32_pad(c, s, qbytes))) return st;
  HIPCHK(c, hipMemcpyAsync(c->q32.p, queries, qbytes, hipMemcpyHostToDevice, s));
  if ((st = upload(c, s, c->rg_maskof, mask_host))) return st;
  HIPCHK(c, hipEventRecord(e[1], s));

  c->stats = nvdb_hip_scan_stats{};
  c->stats.path = 2;
  c->stats_lazy = false;
  c->last_nq = 0; c->last_cap = 0; c->last_filter = false;             // (nvdb_hip_search_check describes unmasked flat searches)
  uint32_t violations = 0;
  MaskedScratch sc;
  nvdb_hip_timing scan_t;
  std::memset(&scan_t, 0, sizeof(scan_t));
  for (uint32_t q0 = 0; q0 < nq; q0 += 1024) {
    const uint32_t b = std::min<uint32_t>(1024u, nq - q0);
    const float* hq = queries + static_cast<size_t>(q0) * c->dim;
    uint64_t* oi = out_ids + static_cast<size_t>(q0) * k;
    float* os = out_scores + static_cast<size_t>(q0) * k;
    uint32_t* oc = out_counts ? out_counts + q0 : nullptr;
    RangePlan p;                                                      // (the last sub-batch may be smaller: its own route and tiling)
    if (sub_filters(c, b, k, mask_host.data() + q0)) {
      if ((st = plan_range(*c, b, p))) return fail(c, st, p.error);
    }
    if (p.filter) {
      st = filter_sub(c, s, p, hq, mask_host.data() + q0, static_cast<const float*>(c->q32.p) + static_cast<size_t>(q0) * c->dim,
                      static_cast<const uint32_t*>(c->rg_maskof.p) + q0, b, k, oi, os, oc, violations, sc);
    } else {
      st = scan_whole(c, hq, b, k, mask_host.data() + q0, oi, os, oc, timing ? &scan_t : nullptr, &c->stats);
    }
    if (st) return st;
  }
  HIPCHK(c, hipEventRecord(e[2], s));
  HIPCHK(c, hipStreamSynchronize(s));
  c->stats.path = 2;
  c->stats_lazy = false;
  c->last_filter = false;
  if (timing) {
    (void)hipEventElapsedTime(&timing->h2d_ms, e[0], e[1]);
    (void)hipEventElapsedTime(&timing->kernel_ms, e[1], e[2]);
    timing->total_ms = timing->h2d_ms + timing->kernel_ms;
    timing->threads = PART_THREADS; timing->nwarps = PART_WAVES; timing->K = k;
  }
  if (violations) return fail(c, NVDB_ERR_INTERNAL, "filter error bound violated; results were recomputed on the partition scan");
  return NVDB_OK;
}

}  // namespace nvdbhip
