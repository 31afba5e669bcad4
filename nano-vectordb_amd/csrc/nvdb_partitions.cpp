// nvdb_partitions.cpp -- partitioned probe search: the partition table and the optional coarse quantiser of a context, the
// pass driver every user of the partition scans shares (nvdb_parts.h), the launches of kernels_partitions.h, and the entry points nvdb_hip_set_partitions / set_centroids /
// search_partitions / search_ivf, the row masks (nvdb_hip_set_row_masks / update_row_mask / get_row_masks) and the masked
// searches (include/nvdb_hip.h).
//
// Work list (built per pass from the probe table, all on the host, in plain C++: parts_worklist.h):
//   1. every query's probes are de-duplicated; a counting sort by partition gives, per probed partition, the ascending list of
//      the queries that probe it (qidx);
//   2. that list is cut into groups of at most PART_WAVES * QW queries, the partition into balanced segments of at most PART_SEG_ROWS
//      rows; one work item = (segment, group): a partition probed by 8 queries is read once per segment, not 8 times;
//   3. every (item, query) gets a slot of min(k, segment rows) candidates inside the query's block of the candidate buffer
//      (dst); the blocks are laid out by a prefix sum (cbeg), so the capacity is exact and nothing can overflow.
// Items are sorted by group size into classes (<= 8, <= 16, <= 32 queries) that run the QW = 1, 2, 4 builds of the kernel (the
// widest one the LDS has room for): a remainder group of three queries does not pay for sixteen.
// One pass = parts_pass (work list -> cand / q grown -> pinned image -> the image's and the queries' copies) and
// parts_scan_classes (the three classes' launches, widest first); parts_search below, the partition range scan
// (nvdb_range_parts.cpp) and the probe search for any k (nvdb_parts_anyk.cpp), whose slots hold a segment's row count instead of
// min(k, rows), and the masked flat bootstrap (nvdb_masked_flat.cpp) add only what is theirs.  parts_call_begin / _end bracket
// the calls that run several passes; parts_topk_args is the one argument check of the six top-k entry points.
// A masked search is the same work list with every query's mask number appended to the pinned image; the MASKED builds of the
// scan test a row's bit before they offer it, and the select kernel writes the counts the host can no longer derive.  The
// masked flat search runs the corpus as one implicit partition that every query probes -- or, where its plan says so, rides the MFMA
// filter kernels (nvdb_masked_flat.cpp), which calls back into this scan for its bootstrap and for flagged queries.
#include "nvdb_parts.h"

namespace nvdbhip {

void parts_drop(nvdb_hip_ctx* c) {
  PartState* ps = c->parts;
  if (!ps) return;
  ps->offsets.clear();
  ps->have_centroids = false;
  if (ps->coarse) { nvdb_hip_destroy(ps->coarse); ps->coarse = nullptr; }
}

void parts_destroy(nvdb_hip_ctx* c) {
  PartState* ps = c->parts;
  if (!ps) return;
  parts_drop(c);
  for (DevBuf* b : {&ps->meta, &ps->cand, &ps->q, &ps->out_ids, &ps->out_scores, &ps->out_counts}) if (b->p) (void)hipFree(b->p);
  if (ps->pin) (void)hipHostFree(ps->pin);
  for (hipEvent_t e : ps->ev) if (e) (void)hipEventDestroy(e);
  delete ps;
  c->parts = nullptr;
}

nvdb_status launch_scan_parts(nvdb_hip_ctx* c, hipStream_t s, uint32_t qw, bool staged, uint32_t k, const ScanArgs& a) {
  return parts_dispatch(c, qw, staged, a.mk.mask_of != nullptr, [&](auto dt, auto w, auto al, auto st, auto mk) {
    return parts_launch(c, s, scan_parts_kernel<dt(), w(), al(), st(), mk()>, w(), st(), a.nitems, a.items, a.qidx, a.dst, a.q32, k, a.cand, a.mk);
  });
}

nvdb_status parts_args(nvdb_hip_ctx* c, const char* who) {
  if (!c) return NVDB_ERR_INVALID;
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (!c->parts || c->parts->offsets.empty()) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": no partition table (nvdb_hip_set_partitions)");
  return NVDB_OK;
}

PartState* parts_workspace(nvdb_hip_ctx* c) {
  if (!c->parts) c->parts = new PartState();
  return c->parts;
}

PartBuild parts_build(const nvdb_hip_ctx* c) {
  const uint32_t row_bytes = c->dim * static_cast<uint32_t>(bpe_of(c->dtype));
  const bool can_stage = row_bytes % 16 == 0 && row_bytes <= PART_STAGE_MAX_ROW_BYTES && reinterpret_cast<uintptr_t>(c->rows) % 16 == 0;
  PartBuild b;
  for (int pass = 0; pass < 2 && !b.qw_max; ++pass) {
    if (pass == 0 && !can_stage) continue;
    for (uint32_t qw : {4u, 2u, 1u})
      if (parts_lds(c->dim, row_bytes, qw, pass == 0) <= PART_LDS_LIMIT) { b.qw_max = qw; b.staged = pass == 0; break; }
  }
  return b;
}

nvdb_status parts_probes(nvdb_hip_ctx* c, const char* who, const uint64_t* off, uint32_t nparts, uint32_t nq, const uint32_t* probe, uint32_t nprobe,
                         uint64_t* rows_union) {
  if (const char* why = pw_probes(c->parts->list, off, nparts, nq, probe, nprobe, rows_union)) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": " + why);
  return NVDB_OK;
}

namespace {

// the HIP side of a work list's image: meta, the pinned buffer and the events grown / created, the image written (pw_write_image),
// its parts as device addresses.  msel: the pass's own (nullptr: unmasked)
nvdb_status parts_stage(nvdb_hip_ctx* c, const PartList& wl, uint32_t nq, const MaskSel* msel, const uint32_t* extra, uint32_t extra_words, PartImage& im) {
  PartState* ps = c->parts;
  const PartLayout l = pw_layout(ps->list, wl, nq, msel != nullptr, extra_words);
  const size_t meta_bytes = l.words * 4;
  if (nvdb_status st = ensure(c, ps->meta, meta_bytes)) return st;
  if (ps->pin_bytes < meta_bytes) {
    if (ps->pin) (void)hipHostFree(ps->pin);
    ps->pin = nullptr; ps->pin_bytes = 0;
    HIPCHK(c, hipHostMalloc(&ps->pin, meta_bytes + meta_bytes / 2, hipHostMallocDefault));
    ps->pin_bytes = meta_bytes + meta_bytes / 2;
  }
  for (hipEvent_t& e : ps->ev) if (!e) HIPCHK(c, hipEventCreate(&e));
  pw_write_image(ps->list, l, msel ? msel->mask_of : nullptr, extra, static_cast<uint32_t*>(ps->pin));
  const uint32_t* dmeta = static_cast<const uint32_t*>(ps->meta.p);
  im.bytes = meta_bytes;
  im.items = reinterpret_cast<const PartItem*>(dmeta + l.items);
  im.qidx = dmeta + l.qidx;
  im.dst = dmeta + l.dst;
  im.cbeg = dmeta + l.cbeg;
  im.extra = dmeta + l.extra;
  im.mk = msel ? PartMask{dmeta + l.mask_of, static_cast<const uint32_t*>(c->row_masks.p), static_cast<uint32_t>(rm_words(c->n))}
               : PartMask{nullptr, nullptr, 0u};
  return NVDB_OK;
}

}  // namespace

nvdb_status parts_pass(nvdb_hip_ctx* c, hipStream_t s, const char* who, const PartBuild& pb, PartPass& p, const PartPassHook& between) {
  PartState* ps = c->parts;
  nvdb_status st;
  if (const char* why = pw_worklist(ps->list, p.off, p.nparts, p.q0, p.b, p.nprobe, PART_WAVES * pb.qw_max, p.slot_cap, p.wl))
    return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": " + why);
  if (p.skip_empty && !p.wl.total) return NVDB_OK;
  if (between && (st = between(p))) return st;
  // device workspace (grow-only) and the pinned image of the work list
  const size_t qbytes = static_cast<size_t>(p.b) * c->dim * 4;
  if ((st = ensure(c, ps->cand, std::max<size_t>(p.wl.total, 1) * sizeof(Cand)))) return st;
  if (p.queries && (st = ensure(c, ps->q, qbytes))) return st;
  const MaskSel sub{p.msel && p.msel->mask_of ? p.msel->mask_of + p.q0 : nullptr};   // the one place a batch's mask_of becomes a pass's
  if ((st = parts_stage(c, p.wl, p.b, p.msel ? &sub : nullptr, p.extra, p.extra_words, p.im))) return st;
  if (p.time_copies) HIPCHK(c, hipEventRecord(ps->ev[0], s));
  HIPCHK(c, hipMemcpyAsync(ps->meta.p, ps->pin, p.im.bytes, hipMemcpyHostToDevice, s));
  if (p.queries) HIPCHK(c, hipMemcpyAsync(ps->q.p, p.queries + static_cast<size_t>(p.q0) * c->dim, qbytes, hipMemcpyHostToDevice, s));
  if (p.time_copies) HIPCHK(c, hipEventRecord(ps->ev[1], s));
  return NVDB_OK;
}

nvdb_status parts_call_begin(nvdb_hip_ctx* c, uint32_t path) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventRecord(get_event(c, 60), c->stream));
  c->stats = nvdb_hip_scan_stats{};
  c->stats.path = path;
  c->stats_lazy = false;
  c->last_nq = 0; c->last_cap = 0; c->last_filter = false;           // (nvdb_hip_search_check describes flat searches)
  c->last_filter_kind = FILTER_NONE;
  return NVDB_OK;
}

nvdb_status parts_call_end(nvdb_hip_ctx* c, nvdb_hip_timing* timing) {
  HIPCHK(c, hipEventRecord(get_event(c, 62), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (timing) {
    const PartBuild pb = parts_build(c);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, get_event(c, 60), get_event(c, 62));
    timing->kernel_ms += ms;
    timing->total_ms = timing->h2d_ms + timing->kernel_ms + timing->d2h_ms;
    timing->threads = PART_THREADS; timing->nwarps = PART_WAVES;
    timing->shmem_bytes = parts_lds(c->dim, c->dim * static_cast<uint32_t>(bpe_of(c->dtype)), pb.qw_max, pb.staged);
  }
  return NVDB_OK;
}

nvdb_status parts_coarse(nvdb_hip_ctx* c, const char* who, const float* queries, uint32_t nq, uint32_t nprobe, uint32_t* out_probe, nvdb_hip_timing* timing,
                         uint32_t& np) {
  PartState* ps = c->parts;
  nvdb_status st;
  const uint32_t nparts = static_cast<uint32_t>(ps->offsets.size() - 1);
  np = std::min(nprobe, nparts);                                           // the clamp; out_probe keeps the caller's row length
  // coarse step: the flat search over the centroids (its order: score desc, partition number asc)
  ps->coarse_ids.resize(static_cast<size_t>(nq) * np);
  ps->coarse_scores.resize(static_cast<size_t>(nq) * np);
  nvdb_hip_timing ct;
  if ((st = nvdb_hip_search_batch(ps->coarse, queries, nq, np, ps->coarse_ids.data(), ps->coarse_scores.data(), nullptr, timing ? &ct : nullptr)))
    return fail(c, st, std::string(who) + " (coarse step): " + nvdb_hip_last_error(ps->coarse));
  ps->probe_tmp.resize(static_cast<size_t>(nq) * np);
  for (size_t i = 0; i < ps->probe_tmp.size(); ++i) ps->probe_tmp[i] = static_cast<uint32_t>(ps->coarse_ids[i]);
  if (out_probe)
    for (uint32_t q = 0; q < nq; ++q)
      for (uint32_t j = 0; j < nprobe; ++j) out_probe[static_cast<size_t>(q) * nprobe + j] = j < np ? ps->probe_tmp[static_cast<size_t>(q) * np + j] : 0xFFFFFFFFu;
  if (timing) { timing->h2d_ms = ct.h2d_ms; timing->kernel_ms = ct.kernel_ms; timing->d2h_ms = ct.d2h_ms; }
  return NVDB_OK;
}

// the search proper over the table off[0 .. nparts]; the caller has validated the context, nq > 0 and 0 < k <= 64.
// msel != nullptr: the masked search (the caller has checked mask_of against the resident planes)
nvdb_status parts_search(nvdb_hip_ctx* c, const uint64_t* off, uint32_t nparts, const float* queries, uint32_t nq, uint32_t k, const uint32_t* probe,
                         uint32_t nprobe, const MaskSel* msel, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nvdb_hip_timing* timing) {
  PartState* ps = c->parts;
  const uint32_t row_bytes = c->dim * static_cast<uint32_t>(bpe_of(c->dtype));
  const PartBuild pb = parts_build(c);
  if (!pb.qw_max) return fail(c, NVDB_ERR_UNSUPPORTED, "search_partitions: dim too large for the query staging");
  nvdb_status st;
  const bool host_counts = out_counts && !msel;                          // (masked: the select kernel counts)
  if (host_counts) ps->rows_union.resize(nq);
  if ((st = parts_probes(c, "search_partitions", off, nparts, nq, probe, nprobe, host_counts ? ps->rows_union.data() : nullptr))) return st;

  const size_t ob_ids = static_cast<size_t>(nq) * k * 8, ob_sc = static_cast<size_t>(nq) * k * 4;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  PartPass p;
  p.off = off; p.nparts = nparts; p.q0 = 0; p.b = nq; p.nprobe = nprobe; p.slot_cap = k;
  p.msel = msel; p.queries = queries;
  p.time_copies = timing != nullptr;
  st = parts_pass(c, s, "search_partitions", pb, p, [&](PartPass&) -> nvdb_status {
    if (host_counts)
      for (uint32_t q = 0; q < nq; ++q) out_counts[q] = static_cast<uint32_t>(std::min<uint64_t>(k, ps->rows_union[q]));
    if (nvdb_status e = ensure(c, ps->out_ids, ob_ids)) return e;
    if (nvdb_status e = ensure(c, ps->out_scores, ob_sc)) return e;
    return msel ? ensure(c, ps->out_counts, static_cast<size_t>(nq) * 4) : NVDB_OK;
  });
  if (st) return st;
  uint32_t* d_counts = msel ? static_cast<uint32_t*>(ps->out_counts.p) : nullptr;
  uint32_t launches = 0;
  if ((st = parts_scan_classes(c, pb, p.im, static_cast<const float*>(ps->q.p), launches,
                               [&](uint32_t qw, const ScanArgs& a) { return launch_scan_parts(c, s, qw, pb.staged, k, a); })))
    return st;
  select_parts_kernel<<<nq, 64, 0, s>>>(static_cast<const Cand*>(ps->cand.p), p.im.cbeg, k, c->row_base,
                                         static_cast<unsigned long long*>(ps->out_ids.p), static_cast<float*>(ps->out_scores.p), d_counts);
  HIPCHK(c, hipGetLastError());
  if (timing) HIPCHK(c, hipEventRecord(ps->ev[2], s));
  HIPCHK(c, hipMemcpyAsync(out_ids, ps->out_ids.p, ob_ids, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(out_scores, ps->out_scores.p, ob_sc, hipMemcpyDeviceToHost, s));
  if (d_counts && out_counts) HIPCHK(c, hipMemcpyAsync(out_counts, d_counts, static_cast<size_t>(nq) * 4, hipMemcpyDeviceToHost, s));
  if (timing) HIPCHK(c, hipEventRecord(ps->ev[3], s));
  HIPCHK(c, hipStreamSynchronize(s));

  c->stats = nvdb_hip_scan_stats{};
  c->stats.path = 4;
  c->stats.chunks = launches;
  c->stats.rows_scanned = p.wl.rows_read;
  c->stats.candidates = p.wl.total;
  c->stats_lazy = false;
  c->last_filter = false;
  if (timing) {
    float h2d = 0.f, ker = 0.f, d2h = 0.f;
    (void)hipEventElapsedTime(&h2d, ps->ev[0], ps->ev[1]);
    (void)hipEventElapsedTime(&ker, ps->ev[1], ps->ev[2]);
    (void)hipEventElapsedTime(&d2h, ps->ev[2], ps->ev[3]);
    timing->h2d_ms += h2d; timing->kernel_ms += ker; timing->d2h_ms += d2h;
    timing->total_ms = timing->h2d_ms + timing->kernel_ms + timing->d2h_ms;
    timing->threads = PART_THREADS; timing->nwarps = PART_WAVES; timing->K = k;
    timing->shmem_bytes = parts_lds(c->dim, row_bytes, pb.qw_max, pb.staged);
  }
  return NVDB_OK;
}

void pad_rows(uint32_t nq, uint32_t k, uint32_t from, uint64_t* out_ids, float* out_scores, uint32_t* counts) {
  for (uint32_t q = 0; q < nq; ++q)
    for (uint32_t j = from; j < k; ++j) { out_ids[static_cast<size_t>(q) * k + j] = ~0ull; out_scores[static_cast<size_t>(q) * k + j] = NEG_INF; }
  if (counts) std::fill(counts, counts + nq, 0u);
}

nvdb_status parts_topk_args(nvdb_hip_ctx* c, const char* who, bool ivf, uint32_t kmax, const float* queries, uint32_t nq, uint32_t k, const uint32_t* probe,
                            uint32_t nprobe, const MaskSel* msel, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nvdb_hip_timing* timing, bool* done) {
  *done = true;
  nvdb_status st = parts_args(c, who);
  if (st) return st;
  if (ivf && !c->parts->have_centroids) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": no centroids (nvdb_hip_set_centroids)");
  if (timing) std::memset(timing, 0, sizeof(*timing));
  if (nq == 0 || k == 0) return NVDB_OK;
  if (kmax && k > kmax) return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": k <= " + std::to_string(kmax) + " (wavefront-resident lists)");
  if (!queries || !out_ids || !out_scores) return fail(c, NVDB_ERR_INVALID, queries ? "null output" : "Null query");
  if (msel && (st = mask_args(c, msel->mask_of, nq, who))) return st;
  if (nprobe == 0) { pad_rows(nq, k, 0, out_ids, out_scores, out_counts); return NVDB_OK; }
  if (!ivf && !probe) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": null probe table");
  *done = false;
  return NVDB_OK;
}

namespace {

// nvdb_hip_search_partitions and its masked twin (msel != nullptr)
nvdb_status search_partitions_any(nvdb_hip_ctx* c, const char* who, const float* queries, uint32_t nq, uint32_t k, const uint32_t* probe, uint32_t nprobe,
                                  const MaskSel* msel, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nvdb_hip_timing* timing) {
  bool done;
  const nvdb_status st = parts_topk_args(c, who, false, WAVE_KMAX, queries, nq, k, probe, nprobe, msel, out_ids, out_scores, out_counts, timing, &done);
  if (st || done) return st;
  PartState* ps = c->parts;
  return parts_search(c, ps->offsets.data(), static_cast<uint32_t>(ps->offsets.size() - 1), queries, nq, k, probe, nprobe, msel, out_ids, out_scores,
                      out_counts, timing);
}

// nvdb_hip_search_ivf and its masked twin: the coarse step knows no masks
nvdb_status search_ivf_any(nvdb_hip_ctx* c, const char* who, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe, const MaskSel* msel,
                           uint64_t* out_ids, float* out_scores, uint32_t* out_counts, uint32_t* out_probe, nvdb_hip_timing* timing) {
  bool done;
  nvdb_status st = parts_topk_args(c, who, true, WAVE_KMAX, queries, nq, k, nullptr, nprobe, msel, out_ids, out_scores, out_counts, timing, &done);
  if (st || done) return st;
  PartState* ps = c->parts;
  uint32_t np = 0;
  if ((st = parts_coarse(c, who, queries, nq, nprobe, out_probe, timing, np))) return st;
  const uint32_t nparts = static_cast<uint32_t>(ps->offsets.size() - 1);
  return parts_search(c, ps->offsets.data(), nparts, queries, nq, k, ps->probe_tmp.data(), np, msel, out_ids, out_scores, out_counts, timing);
}

}  // namespace
}  // namespace nvdbhip

extern "C" {

nvdb_status nvdb_hip_set_partitions(nvdb_hip_ctx* c, const uint64_t* offsets, uint32_t nparts) {
  if (!c) return NVDB_ERR_INVALID;
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (!offsets || nparts == 0 || nparts == 0xFFFFFFFFu) return fail(c, NVDB_ERR_INVALID, "set_partitions: null table or no partitions");
  if (c->n > 0xFFFFFF00ull) return fail(c, NVDB_ERR_UNSUPPORTED, "set_partitions: corpus shard too large");
  if (offsets[0] != 0 || offsets[nparts] != c->n) return fail(c, NVDB_ERR_INVALID, "set_partitions: offsets[0] must be 0 and offsets[nparts] the row count");
  for (uint32_t p = 0; p < nparts; ++p)
    if (offsets[p + 1] < offsets[p]) return fail(c, NVDB_ERR_INVALID, "set_partitions: offsets must be non-decreasing");
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->parts) c->parts = new PartState();
  parts_drop(c);                                   // a new table: the old centroids no longer describe it
  c->parts->offsets.assign(offsets, offsets + nparts + 1);
  return NVDB_OK;
}

nvdb_status nvdb_hip_set_centroids(nvdb_hip_ctx* c, const float* centroids) {
  nvdb_status st = parts_args(c, "set_centroids");
  if (st) return st;
  if (!centroids) return fail(c, NVDB_ERR_INVALID, "set_centroids: null centroids");
  PartState* ps = c->parts;
  ps->have_centroids = false;
  if (!ps->coarse) {
    if ((st = nvdb_hip_create(c->device, &ps->coarse))) return fail(c, st, std::string("set_centroids: ") + nvdb_hip_last_error(nullptr));
  }
  const uint32_t nparts = static_cast<uint32_t>(ps->offsets.size() - 1);
  if ((st = nvdb_hip_upload_corpus(ps->coarse, centroids, nullptr, nparts, c->dim, NVDB_DTYPE_F32, 0)))
    return fail(c, st, std::string("set_centroids: ") + nvdb_hip_last_error(ps->coarse));
  ps->have_centroids = true;
  return NVDB_OK;
}

nvdb_status nvdb_hip_search_partitions(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t k, const uint32_t* probe,
                                       uint32_t nprobe, uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                       nvdb_hip_timing* timing) {
  return search_partitions_any(c, "search_partitions", queries, nq, k, probe, nprobe, nullptr, out_ids, out_scores, out_counts, timing);
}

nvdb_status nvdb_hip_search_ivf(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe, uint64_t* out_ids,
                                float* out_scores, uint32_t* out_counts, uint32_t* out_probe, nvdb_hip_timing* timing) {
  return search_ivf_any(c, "search_ivf", queries, nq, k, nprobe, nullptr, out_ids, out_scores, out_counts, out_probe, timing);
}

// ---- row masks ------------------------------------------------------------------------------------------------------

nvdb_status nvdb_hip_set_row_masks(nvdb_hip_ctx* c, const uint32_t* bits, uint32_t nmasks) {
  if (!c) return NVDB_ERR_INVALID;
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (c->n > ROW_MASK_MAX_ROWS) return fail(c, NVDB_ERR_UNSUPPORTED, "set_row_masks: corpus shard too large");
  if (nmasks == 0xFFFFFFFFu) return fail(c, NVDB_ERR_INVALID, "set_row_masks: 0xFFFFFFFF masks (the number that means no mask)");
  if (nmasks == 0) { c->nmasks = 0; return NVDB_OK; }
  const uint64_t W = rm_words(c->n);
  const size_t words = static_cast<size_t>(nmasks) * W;
  std::vector<uint32_t> planes;                    // the caller's planes with their tail bits cleared (no planes given: all ones)
  if (bits) planes.assign(bits, bits + words);
  else planes.assign(words, 0xFFFFFFFFu);
  for (uint32_t m = 0; m < nmasks; ++m) rm_clear_tail(planes.data() + static_cast<size_t>(m) * W, c->n);
  c->mask_live.assign(nmasks, 0);
  for (uint32_t m = 0; m < nmasks; ++m)
    for (uint64_t w = 0; w < W; ++w) c->mask_live[m] += static_cast<uint64_t>(__builtin_popcount(planes[static_cast<size_t>(m) * W + w]));
  HIPCHK(c, hipSetDevice(c->device));
  c->nmasks = 0;                                   // (a failure below leaves no masks, not half of the new ones)
  if (nvdb_status st = ensure(c, c->row_masks, words * 4)) return st;
  HIPCHK(c, hipMemcpyAsync(c->row_masks.p, planes.data(), words * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->nmasks = nmasks;
  return NVDB_OK;
}

nvdb_status nvdb_hip_update_row_mask(nvdb_hip_ctx* c, uint32_t mask, const uint64_t* rows, uint64_t nrows, int live) {
  if (!c) return NVDB_ERR_INVALID;
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (mask >= c->nmasks) return fail(c, NVDB_ERR_INVALID, "update_row_mask: mask >= nmasks (nvdb_hip_set_row_masks)");
  if (nrows == 0) return NVDB_OK;
  if (!rows) return fail(c, NVDB_ERR_INVALID, "update_row_mask: null row list");
  if (!rm_rows_valid(rows, nrows, c->n)) return fail(c, NVDB_ERR_INVALID, "update_row_mask: a listed row is >= the row count");
  if (nrows > (1ull << 31)) return fail(c, NVDB_ERR_UNSUPPORTED, "update_row_mask: row list too long (split it)");
  std::vector<uint32_t> r32(rows, rows + nrows);   // (n <= 0xFFFFFF00: a local row fits 32 bits)
  HIPCHK(c, hipSetDevice(c->device));
  if (nvdb_status st = ensure(c, c->mask_rows, nrows * 4)) return st;
  HIPCHK(c, hipMemcpyAsync(c->mask_rows.p, r32.data(), nrows * 4, hipMemcpyHostToDevice, c->stream));
  uint32_t* plane = static_cast<uint32_t*>(c->row_masks.p) + static_cast<size_t>(mask) * rm_words(c->n);
  update_row_mask_kernel<<<static_cast<unsigned>((nrows + 255) / 256), 256, 0, c->stream>>>(plane, static_cast<const uint32_t*>(c->mask_rows.p), nrows, live != 0);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (mask < c->mask_live.size()) {
    uint64_t& est = c->mask_live[mask];
    est = live ? std::min<uint64_t>(c->n, est + nrows) : (est > nrows ? est - nrows : 0);
  }
  return NVDB_OK;
}

nvdb_status nvdb_hip_get_row_masks(nvdb_hip_ctx* c, uint32_t* nmasks, uint64_t* words_per_mask, uint32_t* bits_out) {
  if (!c) return NVDB_ERR_INVALID;
  if (nmasks) *nmasks = c->nmasks;
  if (words_per_mask) *words_per_mask = c->nmasks ? rm_words(c->n) : 0;
  if (bits_out && c->nmasks) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(bits_out, c->row_masks.p, static_cast<size_t>(c->nmasks) * rm_words(c->n) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return NVDB_OK;
}

// ---- masked searches ------------------------------------------------------------------------------------------------

nvdb_status nvdb_hip_search_partitions_masked(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t k, const uint32_t* probe,
                                              uint32_t nprobe, const uint32_t* mask_of, uint64_t* out_ids, float* out_scores,
                                              uint32_t* out_counts, nvdb_hip_timing* timing) {
  const MaskSel msel{mask_of};
  return search_partitions_any(c, "search_partitions_masked", queries, nq, k, probe, nprobe, &msel, out_ids, out_scores, out_counts, timing);
}

nvdb_status nvdb_hip_search_ivf_masked(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe, const uint32_t* mask_of,
                                       uint64_t* out_ids, float* out_scores, uint32_t* out_counts, uint32_t* out_probe,
                                       nvdb_hip_timing* timing) {
  const MaskSel msel{mask_of};
  return search_ivf_any(c, "search_ivf_masked", queries, nq, k, nprobe, &msel, out_ids, out_scores, out_counts, out_probe, timing);
}

nvdb_status nvdb_hip_search_batch_masked(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t k, const uint32_t* mask_of,
                                         uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nvdb_hip_timing* timing) {
  if (!c) return NVDB_ERR_INVALID;
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (timing) std::memset(timing, 0, sizeof(*timing));
  if (nq == 0 || k == 0) return NVDB_OK;
  if (k > WAVE_KMAX) return fail(c, NVDB_ERR_UNSUPPORTED, "search_batch_masked: k <= 64 (wavefront-resident lists)");
  if (!queries || !out_ids || !out_scores) return fail(c, NVDB_ERR_INVALID, queries ? "null output" : "Null query");
  if (nvdb_status st = mask_args(c, mask_of, nq, "search_batch_masked")) return st;
  parts_workspace(c);                              // the workspace only: no table is set, a table that is set stays as it is
  return masked_flat_search(c, queries, nq, k, mask_of, out_ids, out_scores, out_counts, timing);
}

}  // extern "C"
