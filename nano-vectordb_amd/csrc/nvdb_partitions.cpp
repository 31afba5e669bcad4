// nvdb_partitions.cpp -- partitioned probe search: the partition table and the optional coarse quantiser of a context, the
// host-side work list, the launches of kernels_partitions.h, and the entry points nvdb_hip_set_partitions / set_centroids /
// search_partitions / search_ivf, the row masks (nvdb_hip_set_row_masks / update_row_mask / get_row_masks) and the masked
// searches (include/nvdb_hip.h).
//
// Work list (built per call from the probe table, all on the host):
//   1. every query's probes are de-duplicated; a counting sort by partition gives, per probed partition, the ascending list of
//      the queries that probe it (qidx);
//   2. that list is cut into groups of at most PART_WAVES * QW queries, the partition into balanced segments of at most PART_SEG_ROWS
//      rows; one work item = (segment, group): a partition probed by 8 queries is read once per segment, not 8 times;
//   3. every (item, query) gets a slot of min(k, segment rows) candidates inside the query's block of the candidate buffer
//      (dst); the blocks are laid out by a prefix sum (cbeg), so the capacity is exact and nothing can overflow.
// Items are sorted by group size into classes (<= 8, <= 16, <= 32 queries) that run the QW = 1, 2, 4 builds of the kernel (the
// widest one the LDS has room for): a remainder group of three queries does not pay for sixteen.
// The list builder, its pinned image and the dispatch to a kernel build (parts_worklist / parts_stage / parts_dispatch,
// nvdb_parts.h) are shared with the partition range scan (nvdb_range_parts.cpp), whose slots hold a segment's row count instead
// of min(k, rows).
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
  PartState* ps = c->parts;
  ps->uniq.resize(static_cast<size_t>(nq) * nprobe);
  ps->ucount.assign(nq, 0);
  for (uint32_t q = 0; q < nq; ++q) {
    uint32_t* u = ps->uniq.data() + static_cast<size_t>(q) * nprobe;
    uint32_t m = 0;
    for (uint32_t j = 0; j < nprobe; ++j) {
      const uint32_t p = probe[static_cast<size_t>(q) * nprobe + j];
      if (p == 0xFFFFFFFFu) continue;
      if (p >= nparts) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": probe entry names a partition >= nparts");
      u[m++] = p;
    }
    std::sort(u, u + m);
    m = static_cast<uint32_t>(std::unique(u, u + m) - u);
    ps->ucount[q] = m;
    if (rows_union) {
      uint64_t rows = 0;
      for (uint32_t j = 0; j < m; ++j) rows += off[u[j] + 1] - off[u[j]];
      rows_union[q] = rows;
    }
  }
  return NVDB_OK;
}

nvdb_status parts_worklist(nvdb_hip_ctx* c, const char* who, const uint64_t* off, uint32_t nparts, uint32_t q0, uint32_t nq, uint32_t nprobe,
                           uint32_t qg_max, uint32_t slot_cap, PartList& wl) {
  PartState* ps = c->parts;
  // 1. the de-duplicated probes of queries q0 .. q0 + nq (parts_probes): per-partition query counts
  const uint32_t* uniq = ps->uniq.data() + static_cast<size_t>(q0) * nprobe;
  const uint32_t* ucount = ps->ucount.data() + q0;
  ps->pcount.assign(nparts, 0);
  for (uint32_t q = 0; q < nq; ++q)
    for (uint32_t j = 0; j < ucount[q]; ++j) ++ps->pcount[uniq[static_cast<size_t>(q) * nprobe + j]];
  // 2. counting sort: the queries of every partition, ascending
  ps->pstart.assign(nparts + 1, 0);
  for (uint32_t p = 0; p < nparts; ++p) ps->pstart[p + 1] = ps->pstart[p] + ps->pcount[p];
  const uint32_t npairs = ps->pstart[nparts];
  ps->qidx.resize(npairs);
  ps->cursor.assign(ps->pstart.begin(), ps->pstart.end() - 1);
  for (uint32_t q = 0; q < nq; ++q) {
    const uint32_t* u = uniq + static_cast<size_t>(q) * nprobe;
    for (uint32_t j = 0; j < ucount[q]; ++j) ps->qidx[ps->cursor[u[j]]++] = q;
  }
  // 3. candidate slots a probe of partition p costs a query; the queries' blocks
  auto nseg_of = [](uint64_t size) { return static_cast<uint32_t>((size + PART_SEG_ROWS - 1) / PART_SEG_ROWS); };
  ps->psum.assign(nparts, 0);
  for (uint32_t p = 0; p < nparts; ++p) {
    const uint64_t size = off[p + 1] - off[p];
    if (!ps->pcount[p] || !size) continue;
    const uint32_t nseg = nseg_of(size);
    uint64_t sum = 0;
    for (uint32_t sg = 0; sg < nseg; ++sg) sum += std::min<uint64_t>(slot_cap, size * (sg + 1) / nseg - size * sg / nseg);
    ps->psum[p] = static_cast<uint32_t>(sum);
  }
  ps->cbeg.assign(nq + 1, 0);
  uint64_t total = 0;
  for (uint32_t q = 0; q < nq; ++q) {
    const uint32_t* u = uniq + static_cast<size_t>(q) * nprobe;
    for (uint32_t j = 0; j < ucount[q]; ++j) total += ps->psum[u[j]];
    if (total >= 0xFFFFFFFFull) return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 candidate slots in one call (split the batch)");
    ps->cbeg[q + 1] = static_cast<uint32_t>(total);
  }
  // 4. work items, by class of group size
  for (auto& v : ps->items) v.clear();
  ps->dst.clear();
  ps->cursor.assign(ps->cbeg.begin(), ps->cbeg.end() - 1);
  uint64_t rows_read = 0;
  for (uint32_t p = 0; p < nparts; ++p) {
    const uint64_t size = off[p + 1] - off[p];
    const uint32_t cnt = ps->pcount[p];
    if (!cnt || !size) continue;
    const uint32_t nseg = nseg_of(size);
    for (uint32_t g0 = 0; g0 < cnt; g0 += qg_max) {
      const uint32_t nqg = std::min(qg_max, cnt - g0);
      const int cl = nqg <= PART_WAVES ? 0 : (nqg <= 2 * PART_WAVES ? 1 : 2);
      for (uint32_t sg = 0; sg < nseg; ++sg) {
        const uint32_t lo = static_cast<uint32_t>(off[p] + size * sg / nseg), hi = static_cast<uint32_t>(off[p] + size * (sg + 1) / nseg);
        ps->items[cl].push_back(PartItem{lo, hi, ps->pstart[p] + g0, static_cast<uint32_t>(ps->dst.size()), nqg, 0u});
        const uint32_t slot = std::min<uint32_t>(slot_cap, hi - lo);
        for (uint32_t g = 0; g < nqg; ++g) { uint32_t& cur = ps->cursor[ps->qidx[ps->pstart[p] + g0 + g]]; ps->dst.push_back(cur); cur += slot; }
        rows_read += hi - lo;
      }
    }
  }
  wl.npairs = npairs;
  wl.total = total;
  wl.rows_read = rows_read;
  wl.nitems = ps->items[0].size() + ps->items[1].size() + ps->items[2].size();
  return NVDB_OK;
}

nvdb_status parts_stage(nvdb_hip_ctx* c, const PartList& wl, uint32_t nq, const MaskSel* msel, const uint32_t* extra, uint32_t extra_words, PartImage& im) {
  PartState* ps = c->parts;
  const size_t w_items = wl.nitems * (sizeof(PartItem) / 4), w_qidx = wl.npairs, w_dst = ps->dst.size(), w_cbeg = nq + 1, w_mask = msel ? nq : 0;
  const size_t meta_bytes = (w_items + w_qidx + w_dst + w_cbeg + w_mask + extra_words) * 4;
  if (nvdb_status st = ensure(c, ps->meta, meta_bytes)) return st;
  if (ps->pin_bytes < meta_bytes) {
    if (ps->pin) (void)hipHostFree(ps->pin);
    ps->pin = nullptr; ps->pin_bytes = 0;
    HIPCHK(c, hipHostMalloc(&ps->pin, meta_bytes + meta_bytes / 2, hipHostMallocDefault));
    ps->pin_bytes = meta_bytes + meta_bytes / 2;
  }
  for (hipEvent_t& e : ps->ev) if (!e) HIPCHK(c, hipEventCreate(&e));
  uint32_t* w = static_cast<uint32_t*>(ps->pin);
  for (int cl = 2; cl >= 0; --cl) {                                     // the widest groups first: the longest items start early
    if (!ps->items[cl].empty()) std::memcpy(w, ps->items[cl].data(), ps->items[cl].size() * sizeof(PartItem));
    w += ps->items[cl].size() * (sizeof(PartItem) / 4);
  }
  if (w_qidx) std::memcpy(w, ps->qidx.data(), w_qidx * 4);
  w += w_qidx;
  if (w_dst) std::memcpy(w, ps->dst.data(), w_dst * 4);
  w += w_dst;
  std::memcpy(w, ps->cbeg.data(), w_cbeg * 4);
  w += w_cbeg;
  for (uint32_t q = 0; q < w_mask; ++q) w[q] = msel->mask_of ? msel->mask_of[q] : 0u;
  w += w_mask;
  if (extra_words) std::memcpy(w, extra, static_cast<size_t>(extra_words) * 4);
  uint32_t* dmeta = static_cast<uint32_t*>(ps->meta.p);
  im.bytes = meta_bytes;
  im.items = reinterpret_cast<const PartItem*>(dmeta);
  im.qidx = dmeta + w_items;
  im.dst = im.qidx + w_qidx;
  im.cbeg = im.dst + w_dst;
  im.extra = im.cbeg + w_cbeg + w_mask;
  im.mk = msel ? PartMask{im.cbeg + w_cbeg, static_cast<const uint32_t*>(c->row_masks.p), static_cast<uint32_t>(rm_words(c->n))}
               : PartMask{nullptr, nullptr, 0u};
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
  const uint32_t qw_max = pb.qw_max;
  const bool staged = pb.staged;
  if (!qw_max) return fail(c, NVDB_ERR_UNSUPPORTED, "search_partitions: dim too large for the query staging");
  nvdb_status st;
  const bool host_counts = out_counts && !msel;                          // (masked: the select kernel counts)
  if (host_counts) ps->rows_union.resize(nq);
  if ((st = parts_probes(c, "search_partitions", off, nparts, nq, probe, nprobe, host_counts ? ps->rows_union.data() : nullptr))) return st;
  PartList wl;
  if ((st = parts_worklist(c, "search_partitions", off, nparts, 0, nq, nprobe, PART_WAVES * qw_max, k, wl))) return st;
  if (host_counts)
    for (uint32_t q = 0; q < nq; ++q) out_counts[q] = static_cast<uint32_t>(std::min<uint64_t>(k, ps->rows_union[q]));
  const uint64_t total = wl.total, rows_read = wl.rows_read;

  // device workspace (grow-only) and the pinned image of the work list: [items | qidx | dst | cbeg | masked: mask_of]
  const size_t qbytes = static_cast<size_t>(nq) * c->dim * 4, ob_ids = static_cast<size_t>(nq) * k * 8, ob_sc = static_cast<size_t>(nq) * k * 4;
  HIPCHK(c, hipSetDevice(c->device));
  if ((st = ensure(c, ps->cand, std::max<size_t>(total, 1) * sizeof(Cand)))) return st;
  if ((st = ensure(c, ps->q, qbytes))) return st;
  if ((st = ensure(c, ps->out_ids, ob_ids))) return st;
  if ((st = ensure(c, ps->out_scores, ob_sc))) return st;
  if (msel && (st = ensure(c, ps->out_counts, static_cast<size_t>(nq) * 4))) return st;
  PartImage im;
  if ((st = parts_stage(c, wl, nq, msel, nullptr, 0, im))) return st;
  hipStream_t s = c->stream;
  const PartItem* d_items = im.items;
  const uint32_t *d_qidx = im.qidx, *d_dst = im.dst, *d_cbeg = im.cbeg;
  const PartMask mk = im.mk;
  uint32_t* d_counts = msel ? static_cast<uint32_t*>(ps->out_counts.p) : nullptr;
  if (timing) HIPCHK(c, hipEventRecord(ps->ev[0], s));
  HIPCHK(c, hipMemcpyAsync(ps->meta.p, ps->pin, im.bytes, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(ps->q.p, queries, qbytes, hipMemcpyHostToDevice, s));
  if (timing) HIPCHK(c, hipEventRecord(ps->ev[1], s));
  uint32_t launches = 0;
  {
    const PartItem* it = d_items;
    for (int cl = 2; cl >= 0; --cl) {
      const uint32_t n_cl = static_cast<uint32_t>(ps->items[cl].size());
      if (!n_cl) continue;
      const uint32_t qw = std::min<uint32_t>(qw_max, 1u << cl);
      const ScanArgs a{it, n_cl, d_qidx, d_dst, static_cast<const float*>(ps->q.p), static_cast<Cand*>(ps->cand.p), mk};
      if ((st = launch_scan_parts(c, s, qw, staged, k, a))) return st;
      it += n_cl;
      ++launches;
    }
  }
  select_parts_kernel<<<nq, 64, 0, s>>>(static_cast<const Cand*>(ps->cand.p), d_cbeg, k, c->row_base,
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
  c->stats.rows_scanned = rows_read;
  c->stats.candidates = total;
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
    timing->shmem_bytes = parts_lds(c->dim, row_bytes, qw_max, staged);
  }
  return NVDB_OK;
}

namespace {

void pad_outputs(uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
  for (size_t i = 0; i < static_cast<size_t>(nq) * k; ++i) { out_ids[i] = ~0ull; out_scores[i] = NEG_INF; }
  if (out_counts) for (uint32_t q = 0; q < nq; ++q) out_counts[q] = 0;
}

// nvdb_hip_search_partitions and its masked twin (msel != nullptr)
nvdb_status search_partitions_any(nvdb_hip_ctx* c, const char* who, const float* queries, uint32_t nq, uint32_t k, const uint32_t* probe, uint32_t nprobe,
                                  const MaskSel* msel, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nvdb_hip_timing* timing) {
  nvdb_status st = parts_args(c, who);
  if (st) return st;
  if (timing) std::memset(timing, 0, sizeof(*timing));
  if (nq == 0 || k == 0) return NVDB_OK;
  if (k > WAVE_KMAX) return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": k <= 64 (wavefront-resident lists)");
  if (!queries || !out_ids || !out_scores) return fail(c, NVDB_ERR_INVALID, queries ? "null output" : "Null query");
  if (msel && (st = mask_args(c, msel->mask_of, nq, who))) return st;
  if (nprobe == 0) { pad_outputs(nq, k, out_ids, out_scores, out_counts); return NVDB_OK; }
  if (!probe) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": null probe table");
  PartState* ps = c->parts;
  return parts_search(c, ps->offsets.data(), static_cast<uint32_t>(ps->offsets.size() - 1), queries, nq, k, probe, nprobe, msel, out_ids, out_scores,
                      out_counts, timing);
}

// nvdb_hip_search_ivf and its masked twin: the coarse step knows no masks
nvdb_status search_ivf_any(nvdb_hip_ctx* c, const char* who, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe, const MaskSel* msel,
                           uint64_t* out_ids, float* out_scores, uint32_t* out_counts, uint32_t* out_probe, nvdb_hip_timing* timing) {
  nvdb_status st = parts_args(c, who);
  if (st) return st;
  PartState* ps = c->parts;
  if (!ps->have_centroids) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": no centroids (nvdb_hip_set_centroids)");
  if (timing) std::memset(timing, 0, sizeof(*timing));
  if (nq == 0 || k == 0) return NVDB_OK;
  if (k > WAVE_KMAX) return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": k <= 64 (wavefront-resident lists)");
  if (!queries || !out_ids || !out_scores) return fail(c, NVDB_ERR_INVALID, queries ? "null output" : "Null query");
  if (msel && (st = mask_args(c, msel->mask_of, nq, who))) return st;
  if (nprobe == 0) { pad_outputs(nq, k, out_ids, out_scores, out_counts); return NVDB_OK; }
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
