// nvdb_range.cpp -- exact range search (DESIGN.md section 4 "range search"): every row whose reference-order score reaches a
// per-query radius, as variable-length slices (lims) over packed device arrays.  Per sub-batch of <= 1024 queries:
//   filter route  prep -> thresholds radius - E_q -> the MFMA filter over the whole corpus at those FIXED thresholds (no bootstrap, no
//                 select, no chunk schedule) -> rescore -> keep / order (range_keep_kernel) -> pack
//   exact route   score matrix of a query sub-batch (the any-k path's) -> count -> range_tail (nvdb_range.h): collect, sort, emit; serves every dtype / dim,
//                 option path = 1, and the queries the filter route could not answer (flagged: non-finite query or radius, list overflow;
//                 all of them after a wave-log overflow or a bound violation)
// nvdb_hip_range_search_masked is the same call under a row-mask plane per query: on the filter route only the keep step differs
// (range_keep_masked_kernel; thresholds are fixed, so a dead row costs a list entry and nothing else), and what the exact route would
// answer goes to the partition range scan of nvdb_range_parts.cpp instead, the corpus as one implicit partition.
// The exclusive scan of the per-query counts runs on the HOST over the downloaded counts: the call is synchronous and has to bring the
// counts down for out_lims anyway, and the packed arrays are sized from them before anything is written.
#include "nvdb_range.h"
#include "kernels_range_parts.h"

namespace nvdbhip {

// Pure arithmetic over corpus facts and options, like plan_search (and like it, it chooses the filter kind once and carries it in the plan).
nvdb_status plan_range(const nvdb_hip_ctx& ctx, uint32_t nq, RangePlan& p) {
  const nvdb_hip_ctx* c = &ctx;
  p = RangePlan{};
  const FilterKind kind = p.kind = filter_kind(c);
  int path = static_cast<int>(c->opt_path);
  if (path == 0) path = (filter_supported(c) && nq >= c->opt_min_filter_batch && c->n >= 4ull * c->opt_chunk0) ? 2 : 1;
  if (path == 2 && !filter_supported(c)) {
    p.error = "MFMA filter path needs an fp16/fp32 corpus with dim <= 3072 or an int8 corpus with dim <= 1536";
    return NVDB_ERR_UNSUPPORTED;
  }
  if (path != 2) return NVDB_OK;
  p.filter = p.prep = true;
  // The longest lists the keep kernel orders in LDS: how many rows reach a radius is the caller's choice, not a property of the corpus
  // (even: the pack kernel moves two entries per 16-byte access)
  p.cap = c->opt_cap > 0 ? std::min<uint32_t>(static_cast<uint32_t>(c->opt_cap), SELECT_MAX_CAP) : SELECT_MAX_CAP;
  p.cap = std::max<uint32_t>(2u, (p.cap + 1u) & ~1u);
  p.QPB = filter_qpb(c, kind, nq);
  p.QT = (nq + p.QPB - 1) / p.QPB;
  p.nq_pad = p.QT * p.QPB;
  p.prog_words = PROG_SLOTS * static_cast<uint32_t>(c->num_cu) * 8u;
  p.prep_inits = c->opt_fuse != 0;
  const uint32_t n = static_cast<uint32_t>(c->n);
  p.tile_rows = filter_tile_rows(c, kind, nq);
  p.n_al = corpus_padded(c, kind) ? (n + p.tile_rows - 1) / p.tile_rows * p.tile_rows : n / p.tile_rows * p.tile_rows;
  p.tail_exact = p.n_al < n;
  // Launches.  A wave logs at most FILTER_LOGCAP survivors per launch, and a range search has no thresholds that tighten from chunk to
  // chunk: what bounds the pressure on a log is the number of launches alone.  Four launches give every wave 4 x 4096 entries -- with
  // one wave per SIMD that is 16M entries per sub-batch, twice what its 1024 full lists hold, so the lists overflow (a per-query
  // fallback) before the logs do (a whole-sub-batch fallback) -- and cost three launch boundaries of ~10 us against a stream of
  // milliseconds.  Below 256K rows the stream itself is that short: one launch.
  const uint32_t pieces = p.n_al >= (1u << 18) ? 4u : 1u;
  p.launch_rows = std::max<uint32_t>(64u, ((p.n_al + pieces - 1) / pieces + 63u) & ~63u);
  // permuted tile order spreads a clustered corpus' survivors over the waves' logs; only where the streaming kernel's tile is the
  // plan's tile (dims <= 768), as for the flat search
  p.perm_on = c->opt_tile_permute && c->fdim <= 768;
  return NVDB_OK;
}

namespace {

// ---- exact route: ne queries at dev_q / dev_radius; qmap[i] = query i's number inside its sub-batch (ascending).  Fills cnt[qmap[i]]
// and, while the call packs, emits query i's slice at base + (sum of cnt[] before qmap[i]) -- the counts of every earlier query of the
// sub-batch are known by then: the filter route's came first, the exact route's arrive in order.
nvdb_status range_exact(nvdb_hip_ctx* c, hipStream_t s, const float* dev_q, const float* dev_radius, uint32_t ne, const std::vector<uint32_t>& qmap,
                        std::vector<uint64_t>& cnt, uint64_t base, RangeOut& out) {
  const uint32_t n = static_cast<uint32_t>(c->n);
  const uint64_t ld = (static_cast<uint64_t>(n) + 63u) & ~63ull;
  uint32_t QB = 0, QG = 0;
  nvdb_status st;
  if ((st = score_matrix_batch(c, ne, ld * 4, c->lk_scores.bytes, QB, QG))) return st;
  if ((st = ensure(c, c->lk_scores, static_cast<size_t>(QB) * ld * 4))) return st;
  if ((st = ensure(c, c->rg_taken, static_cast<size_t>(QB) * 4))) return st;
  float* scores = static_cast<float*>(c->lk_scores.p);
  // keys a run may hold in slabs: a quarter of the score matrix' budget, or one query's slab
  const uint64_t slab_max = (static_cast<uint64_t>(c->opt_largek_budget_mb) << 20) / 32;
  std::vector<uint32_t> hc;
  std::vector<uint64_t> pre, out_off;
  for (uint32_t g0 = 0; g0 < ne; g0 += QB) {
    const uint32_t b = std::min(QB, ne - g0);
    const float* rad = dev_radius + g0;
    if ((st = launch_score_matrix(c, s, dev_q + static_cast<size_t>(g0) * c->dim, b, scores, ld, n, QG, true))) return st;
    uint32_t* taken = static_cast<uint32_t*>(c->rg_taken.p);
    HIPCHK(c, hipMemsetAsync(taken, 0, static_cast<size_t>(b) * 4, s));
    const uint32_t G = std::max<uint32_t>(1, std::min<uint32_t>((n + 1023u) / 1024u, (8u * static_cast<uint32_t>(c->num_cu) + b - 1) / b));
    range_count_kernel<<<dim3(G, b), 256, 0, s>>>(scores, ld, n, rad, taken);
    HIPCHK(c, hipGetLastError());
    hc.resize(b);
    HIPCHK(c, hipMemcpyAsync(hc.data(), taken, static_cast<size_t>(b) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    c->stats.chunks++;
    c->stats.rows_scanned += c->n;
    for (uint32_t i = 0; i < b; ++i) cnt[qmap[g0 + i]] = hc[i];
    const uint32_t last = qmap[g0 + b - 1];
    pre.assign(static_cast<size_t>(last) + 2, 0);
    for (uint32_t j = 0; j <= last; ++j) pre[j + 1] = pre[j] + cnt[j];
    if (!reserve_packed(c, s, out, base + pre[last + 1], &st)) { if (st) return st; continue; }
    out_off.resize(b);
    for (uint32_t i = 0; i < b; ++i) out_off[i] = base + pre[qmap[g0 + i]];
    st = range_tail(c, s, "range_search", hc.data(), b, out_off.data(), slab_max,
        [&](const std::vector<RangeDesc>& run, const RangeDesc* desc, uint32_t* taken, unsigned long long* slab) {
          const uint32_t nr = static_cast<uint32_t>(run.size());
          const uint32_t Gr = std::max<uint32_t>(1, std::min<uint32_t>((n + 1023u) / 1024u, (8u * static_cast<uint32_t>(c->num_cu) + nr - 1) / nr));
          range_collect_kernel<<<dim3(Gr, nr), 256, 0, s>>>(scores, ld, n, rad, desc, taken, slab);
        },
        [&](const std::vector<RangeDesc>& run, uint32_t max_cnt, const RangeDesc* desc, const unsigned long long* slab) {
          range_emit_kernel<<<dim3((max_cnt + 255u) / 256u, static_cast<uint32_t>(run.size())), 256, 0, s>>>(
              slab, desc, scores, ld, n, c->row_base, static_cast<unsigned long long*>(c->rg_ids.p), static_cast<float*>(c->rg_scores.p));
        });
    if (st) return st;
  }
  return NVDB_OK;
}

}  // namespace

// ---- filter route of one sub-batch: everything up to the ordered slabs in c->cand and their counts in c->rg_kept
// dmask_of != nullptr: the masked search -- the keep step also requires the row's bit in the query's plane (everything before it is the unmasked pass)
nvdb_status range_filter_pass(nvdb_hip_ctx* c, hipStream_t s, const RangePlan& p, const float* dq, const float* dradius, uint32_t nq, const uint32_t* dmask_of,
                              FilterVerdict& v) {
  nvdb_status st;
  const uint32_t n = static_cast<uint32_t>(c->n), cap = p.cap, QT = p.QT;
  FilterRun run;
  if ((st = begin_filter_run(c, s, p, dq, nullptr, nq, &c->rg_kept, run))) return st;
  range_thr_kernel<<<(p.nq_pad + 255) / 256, 256, 0, s>>>(dradius, static_cast<const float*>(c->ebound.p), static_cast<float*>(c->thr.p),
                                                          static_cast<uint32_t*>(c->overflow.p), nq, p.nq_pad);
  HIPCHK(c, hipGetLastError());
  for (uint32_t r = 0; r < p.n_al;) {
    const uint32_t hi = static_cast<uint32_t>(std::min<uint64_t>(p.n_al, static_cast<uint64_t>(r) + p.launch_rows));
    if ((st = launch_filter(c, run, {r, hi}))) return st;
    c->stats.chunks++;
    c->stats.rows_scanned += static_cast<uint64_t>(hi - r) * QT;
    r = hi;
  }
  // ragged tail of an adopted corpus: exact scores against the same thresholds (fewer rows than the wavefront lists hold)
  if (p.tail_exact) {
    if ((st = launch_scan_exact(c, s, p.n_al, n, dq, nq, WAVE_KMAX, static_cast<const float*>(c->thr.p), cap, 0))) return st;
    c->stats.rows_scanned += static_cast<uint64_t>(n - p.n_al) * QT;
  }
  if ((st = launch_rescore(c, s, dq, nq, cap))) return st;          // exact scores into the lists, |filter - exact| <= E_q checked
  uint32_t cap2 = 1;
  while (cap2 < cap) cap2 <<= 1;
  if (dmask_of) {
    if ((st = raise_lds_limit(c, reinterpret_cast<const void*>(range_keep_masked_kernel), SELECT_MAX_CAP * sizeof(Cand)))) return st;
    range_keep_masked_kernel<<<nq, 256, cap2 * sizeof(Cand), s>>>(static_cast<Cand*>(c->cand.p), static_cast<const uint32_t*>(c->cnt.p), cap, dradius,
                                                                  static_cast<const uint32_t*>(c->overflow.p), static_cast<uint32_t*>(c->rg_kept.p), dmask_of,
                                                                  static_cast<const uint32_t*>(c->row_masks.p), static_cast<uint32_t>(rm_words(c->n)), n);
  } else {
    if ((st = raise_lds_limit(c, reinterpret_cast<const void*>(range_keep_kernel), SELECT_MAX_CAP * sizeof(Cand)))) return st;
    range_keep_kernel<<<nq, 256, cap2 * sizeof(Cand), s>>>(static_cast<Cand*>(c->cand.p), static_cast<const uint32_t*>(c->cnt.p), cap, dradius,
                                                           static_cast<const uint32_t*>(c->overflow.p), static_cast<uint32_t*>(c->rg_kept.p));
  }
  HIPCHK(c, hipGetLastError());
  v.kept.resize(nq); v.overflow.resize(nq); v.listcnt.resize(nq);
  HIPCHK(c, hipMemcpyAsync(v.misc, c->misc.p, 32, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(v.kept.data(), c->rg_kept.p, static_cast<size_t>(nq) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(v.overflow.data(), c->overflow.p, static_cast<size_t>(nq) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(v.listcnt.data(), c->cnt.p, static_cast<size_t>(nq) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return NVDB_OK;
}

nvdb_status range_search_flat(nvdb_hip_ctx* c, const char* who, const float* queries, uint32_t nq, const float* radius, const MaskSel* msel, uint64_t* out_lims,
                              nvdb_hip_timing* timing) {
  if (!c) return NVDB_ERR_INVALID;
  if (!out_lims || (nq > 0 && (!queries || !radius)))
    return fail(c, NVDB_ERR_INVALID, !out_lims ? std::string(who) + ": null out_lims" : queries ? std::string(who) + ": null radius" : "Null query");
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (msel && nq > 0)                                               // (before anything is written or launched)
    if (nvdb_status ms = mask_args(c, msel->mask_of, nq, who)) return ms;
  if (timing) std::memset(timing, 0, sizeof(*timing));
  out_lims[0] = 0;
  c->range_valid = false;
  c->range_total = 0;
  if (nq == 0) { c->range_valid = true; return NVDB_OK; }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  nvdb_status st;
  {
    RangePlan p;                                                    // (an unsupported forced route fails before anything is enqueued)
    if ((st = plan_range(*c, std::min<uint32_t>(nq, 1024u), p))) return fail(c, st, p.error);
  }
  const size_t qbytes = static_cast<size_t>(nq) * c->dim * 4;
  if ((st = ensure_q32(c, s, qbytes))) return st;
  if ((st = ensure(c, c->rg_radius, static_cast<size_t>(nq) * 4))) return st;
  if ((st = ensure(c, c->rg_off, 1024 * 8))) return st;
  const hipEvent_t e[3] = {get_event(c, 60), get_event(c, 61), get_event(c, 62)};
  HIPCHK(c, hipEventRecord(e[0], s));
  if ((st = zero_q32_pad(c, s, qbytes))) return st;
  HIPCHK(c, hipMemcpyAsync(c->q32.p, queries, qbytes, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->rg_radius.p, radius, static_cast<size_t>(nq) * 4, hipMemcpyHostToDevice, s));
  std::vector<uint32_t> mask_host;                                  // masked: every query's plane, NULL resolved to plane 0
  if (msel) {
    mask_host.assign(nq, 0u);
    if (msel->mask_of) std::copy(msel->mask_of, msel->mask_of + nq, mask_host.begin());
    if ((st = upload(c, s, c->rg_maskof, mask_host))) return st;
  }
  HIPCHK(c, hipEventRecord(e[1], s));

  c->stats = nvdb_hip_scan_stats{};
  c->stats.path = msel ? RANGE_STAT_PARTS : RANGE_STAT_EXACT;
  c->stats_lazy = false;
  c->last_nq = 0; c->last_cap = 0; c->last_filter = false;           // (nvdb_hip_search_check describes flat searches)
  c->last_filter_kind = FILTER_NONE;
  bool any_filter = false;
  RangeOut out;
  out.budget_entries = (static_cast<uint64_t>(c->opt_range_max_mb) << 20) / 12;
  uint64_t total = 0;
  uint32_t violations = 0;
  FilterVerdict v;
  std::vector<uint64_t> cnt, off;
  std::vector<uint32_t> flagged, fl_m, fl_probe;
  std::vector<float> fl_q, fl_r;
  for (uint32_t q0 = 0; q0 < nq; q0 += 1024) {
    const uint32_t b = std::min<uint32_t>(1024u, nq - q0);
    const float* dq = static_cast<const float*>(c->q32.p) + static_cast<size_t>(q0) * c->dim;
    const float* dr = static_cast<const float*>(c->rg_radius.p) + q0;
    cnt.assign(b, 0);
    flagged.clear();
    bool slabs = false;                                             // the filter route left slabs to pack
    RangePlan ps;                                                   // (the last sub-batch may be smaller: its own route and tiling)
    if ((st = plan_range(*c, b, ps))) return fail(c, st, ps.error);
    if (ps.filter) {
      any_filter = true;
      if ((st = range_filter_pass(c, s, ps, dq, dr, b, msel ? static_cast<const uint32_t*>(c->rg_maskof.p) + q0 : nullptr, v))) return st;
      for (uint32_t q = 0; q < b; ++q) c->stats.candidates += std::min(v.listcnt[q], ps.cap);
      c->stats.bound_violations += v.misc[0];
      violations += v.misc[0];
      if (v.misc[0] | v.misc[1]) {
        // a violated bound: nothing of this pass is trusted; a wave's log overflowed: which queries lost entries is unknown
        if (v.misc[1]) c->stats.overflow_queries += b;
        for (uint32_t q = 0; q < b; ++q) flagged.push_back(q);
      } else {
        for (uint32_t q = 0; q < b; ++q) {
          if (v.overflow[q]) flagged.push_back(q);
          else { cnt[q] = v.kept[q]; slabs = slabs || v.kept[q] != 0; }
        }
        c->stats.overflow_queries += static_cast<uint32_t>(flagged.size());
      }
      if (!msel && !flagged.empty() && flagged.size() < b) {
        // the flagged queries as a compact batch (64 zero rows behind it: the exact kernels load whole query groups)
        const size_t qb = flagged.size() * static_cast<size_t>(c->dim) * 4, padb = 64 * static_cast<size_t>(c->dim) * 4;
        if ((st = ensure(c, c->rg_q, qb + padb + flagged.size() * 4 + 256))) return st;
        if ((st = upload(c, s, c->rg_idx, flagged))) return st;
        float* gq = static_cast<float*>(c->rg_q.p);
        float* gr = reinterpret_cast<float*>(static_cast<char*>(c->rg_q.p) + ((qb + padb + 255) & ~static_cast<size_t>(255)));
        HIPCHK(c, hipMemsetAsync(static_cast<char*>(c->rg_q.p) + qb, 0, padb, s));
        range_gather_kernel<<<static_cast<uint32_t>(flagged.size()), 256, 0, s>>>(dq, dr, static_cast<const uint32_t*>(c->rg_idx.p), c->dim, gq, gr);
        HIPCHK(c, hipGetLastError());
        dq = gq; dr = gr;
      }
    } else {
      for (uint32_t q = 0; q < b; ++q) flagged.push_back(q);
    }
    if (!flagged.empty() && msel) {
      // masked: the flagged queries on the partition range scan, the corpus as one implicit partition that each of them probes
      const uint32_t nf = static_cast<uint32_t>(flagged.size());
      fl_q.resize(static_cast<size_t>(nf) * c->dim);
      fl_r.resize(nf);
      fl_m.resize(nf);
      for (uint32_t i = 0; i < nf; ++i) {
        const size_t src = static_cast<size_t>(q0) + flagged[i];
        std::memcpy(fl_q.data() + static_cast<size_t>(i) * c->dim, queries + src * c->dim, static_cast<size_t>(c->dim) * 4);
        fl_r[i] = radius[src];
        fl_m[i] = mask_host[src];
      }
      fl_probe.assign(nf, 0u);
      const uint64_t whole[2] = {0, c->n};
      const MaskSel fsel{fl_m.data()};
      parts_workspace(c);
      if ((st = range_parts_core(c, s, who, whole, 1, fl_q.data(), fl_r.data(), nf, fl_probe.data(), 1, &fsel, flagged.data(), cnt, total, out))) return st;
    } else if (!flagged.empty() && (st = range_exact(c, s, dq, dr, static_cast<uint32_t>(flagged.size()), flagged, cnt, total, out))) return st;
    off.assign(b, 0);
    uint64_t run = total;
    uint32_t max_kept = 0;
    for (uint32_t q = 0; q < b; ++q) {
      off[q] = run;
      run += cnt[q];
      out_lims[q0 + q + 1] = run;
      if (slabs && !v.overflow[q]) max_kept = std::max(max_kept, v.kept[q]);
    }
    if (slabs && reserve_packed(c, s, out, run, &st)) {
      if ((st = upload(c, s, c->rg_off, off))) return st;
      // (flagged queries pack nothing: range_keep_kernel left their counts at 0)
      range_pack_kernel<<<dim3((max_kept + 511u) / 512u, b), 256, 0, s>>>(static_cast<const Cand*>(c->cand.p), ps.cap, static_cast<const uint32_t*>(c->rg_kept.p),
                                                                                  static_cast<const unsigned long long*>(c->rg_off.p), c->row_base,
                                                                                  static_cast<unsigned long long*>(c->rg_ids.p), static_cast<float*>(c->rg_scores.p));
      HIPCHK(c, hipGetLastError());
    }
    if (st) return st;
    total = run;
  }
  HIPCHK(c, hipEventRecord(e[2], s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (any_filter) c->stats.path = RANGE_STAT_FILTER;
  if (timing) {
    (void)hipEventElapsedTime(&timing->h2d_ms, e[0], e[1]);
    (void)hipEventElapsedTime(&timing->kernel_ms, e[1], e[2]);
    timing->total_ms = timing->h2d_ms + timing->kernel_ms;
    timing->threads = 256; timing->nwarps = 4;
  }
  if (!out.pack)
    return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string(total) + " results (" + std::to_string((total * 12 + (1u << 20) - 1) >> 20) +
                                            " MB packed) exceed option range_max_mb = " + std::to_string(c->opt_range_max_mb) + "; out_lims is complete");
  c->range_total = total;
  c->range_valid = true;
  if (violations) return fail(c, NVDB_ERR_INTERNAL, msel ? "filter error bound violated; results were recomputed on the partition range scan"
                                                         : "filter error bound violated; results were recomputed on the exact route");
  return NVDB_OK;
}

}  // namespace nvdbhip

extern "C" {

nvdb_status nvdb_hip_range_search(nvdb_hip_ctx* c, const float* queries, uint32_t nq, const float* radius, uint64_t* out_lims, nvdb_hip_timing* timing) {
  return range_search_flat(c, "range_search", queries, nq, radius, nullptr, out_lims, timing);
}

nvdb_status nvdb_hip_range_search_masked(nvdb_hip_ctx* c, const float* queries, uint32_t nq, const float* radius, const uint32_t* mask_of, uint64_t* out_lims,
                                         nvdb_hip_timing* timing) {
  const MaskSel msel{mask_of};
  return range_search_flat(c, "range_search_masked", queries, nq, radius, &msel, out_lims, timing);
}

nvdb_status nvdb_hip_range_results(nvdb_hip_ctx* c, uint64_t* out_ids, float* out_scores) {
  if (!c) return NVDB_ERR_INVALID;
  if (!out_ids || !out_scores) return fail(c, NVDB_ERR_INVALID, "range_results: null output");
  if (!c->range_valid) return fail(c, NVDB_ERR_INVALID, "range_results: no range search whose results are held (none yet, over range_max_mb, or the corpus changed)");
  if (c->range_total == 0) return NVDB_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(out_ids, c->rg_ids.p, static_cast<size_t>(c->range_total) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out_scores, c->rg_scores.p, static_cast<size_t>(c->range_total) * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NVDB_OK;
}

}  // extern "C"
