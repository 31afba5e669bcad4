// nvdb_search.cpp -- orchestration of one flat search (DESIGN.md "pipeline") and the search entry points of the C ABI:
//   path 1 (exact):   init -> exact scan over the whole corpus -> select(final)
//   path 2 (filter):  prep (+ init) -> bootstrap (+ select) -> { filter launch on a chunk (+ select) }* with growing chunks
//                     -> rescore in the reference's fp32 order + final select
//   path 3 (any k):   score matrix of a query sub-batch -> radix select -> sort
// No kernel is defined or launched from this file: the launch helpers live in nvdb_launch_*.cpp.
#include "nvdb_plan.h"

namespace nvdbhip {

// The host API's result block: the 64 bytes of status words (c->misc points INTO the block from then on), ids, scores -- one
// allocation, so that one copy brings down everything a search's caller waits for.  Growing it carries the status words
// (the sticky ones outlive a search) over to the new allocation.
nvdb_status ensure_hostblock(nvdb_hip_ctx* c, size_t out_bytes) {
  const size_t need = 64 + out_bytes;
  if (c->hostblock.p && c->hostblock.bytes >= need) return NVDB_OK;
  HIPCHK(c, hipDeviceSynchronize());
  void* np = nullptr;
  const size_t want = std::max<size_t>(need + need / 2, static_cast<size_t>(1) << 20);
  HIPCHK(c, hipMalloc(&np, want));
  if (c->misc.p) HIPCHK(c, hipMemcpy(np, c->misc.p, 64, hipMemcpyDeviceToDevice));
  else HIPCHK(c, hipMemset(np, 0, 64));
  if (c->hostblock.p) HIPCHK(c, hipFree(c->hostblock.p));
  else if (c->misc.p) HIPCHK(c, hipFree(c->misc.p));
  c->hostblock.p = np; c->hostblock.bytes = want;
  c->misc.p = np; c->misc.bytes = 64;
  return NVDB_OK;
}

// The host API's query buffer.  The 8 query rows after a batch must read as zeros (the exact kernel loads query groups of 8).  The
// buffer is zero beyond q32_dirty (zeroed when allocated, only ever written through [0, qbytes) of some call): a memset is enqueued
// only when an earlier, larger batch left queries where this call's padding lies.
nvdb_status ensure_q32(nvdb_hip_ctx* c, hipStream_t s, size_t qbytes) {
  const size_t before = c->q32.p ? c->q32.bytes : 0;
  if (nvdb_status st = ensure(c, c->q32, qbytes + 8 * static_cast<size_t>(c->dim) * 4)) return st;
  if (c->q32.bytes != before) { HIPCHK(c, hipMemsetAsync(c->q32.p, 0, c->q32.bytes, s)); c->q32_dirty = 0; }   // a new buffer starts all zero
  return NVDB_OK;
}
nvdb_status zero_q32_pad(nvdb_hip_ctx* c, hipStream_t s, size_t qbytes) {
  const size_t pad_bytes = 8 * static_cast<size_t>(c->dim) * 4;
  if (c->q32_dirty > qbytes) HIPCHK(c, hipMemsetAsync(static_cast<char*>(c->q32.p) + qbytes, 0, std::min(pad_bytes, c->q32_dirty - qbytes), s));
  c->q32_dirty = std::max(c->q32_dirty, qbytes);
  return NVDB_OK;
}

// rendezvous counters for the next filter launch: a region the init kernel already cleared, or (past PROG_SLOTS
// launches in one search) a region cleared here
nvdb_status next_prog_region(nvdb_hip_ctx* c, FilterRun& run, uint32_t nwg, uint32_t** out) {
  const size_t region_words = static_cast<size_t>(c->num_cu) * 8;
  if (nwg * 8u > region_words) return fail(c, NVDB_ERR_INTERNAL, "rendezvous region too small for this grid");
  uint32_t* base = static_cast<uint32_t*>(c->prog.p) + static_cast<size_t>(run.prog_slot % PROG_SLOTS) * region_words;
  if (run.prog_slot >= PROG_SLOTS) HIPCHK(c, hipMemsetAsync(base, 0xFF, region_words * 4, run.s));
  ++run.prog_slot;
  *out = base;
  return NVDB_OK;
}

// trows = rows per tile of the kernel being launched (0: identity tile order).  With the permutation on, logical tile g
// of the corpus' T = ceil-or-floor(n / trows) tiles is streamed from physical tile perm_tile(g) (kernels_filter.h).
ScatterArgs scatter_args(nvdb_hip_ctx* c, const FilterRun& run, uint32_t trows) {
  ScatterArgs a{static_cast<Cand*>(c->cand.p), static_cast<uint32_t*>(c->cnt.p), static_cast<uint32_t*>(c->overflow.p),
                static_cast<uint32_t*>(c->misc.p) + 1, run.cap, static_cast<uint32_t>(c->n), 1u, 0u, 0u,
                c->opt_xcd_balance ? static_cast<float*>(c->xcdw.p) : nullptr, static_cast<uint32_t>(c->opt_i8_lo_bits)};
  if (trows && run.perm) {
    const uint32_t n = static_cast<uint32_t>(c->n);
    a.perm_T = corpus_padded(c, run.kind) ? (n + trows - 1) / trows : n / trows;
    perm_params(a.perm_T, a.perm_mul, a.perm_mask);
  }
  return a;
}

nvdb_status launch_boot(nvdb_hip_ctx* c, FilterRun& run, uint32_t n0) { return filter_is_i8(run.kind) ? launch_boot_i8(c, run, n0) : launch_boot_f16(c, run, n0); }
nvdb_status launch_filter(nvdb_hip_ctx* c, FilterRun& run, RowRange rows) { return filter_is_i8(run.kind) ? launch_filter_i8(c, run, rows) : launch_filter_f16(c, run, rows); }

nvdb_status begin_filter_run(nvdb_hip_ctx* c, hipStream_t s, const FilterPlan& p, const float* dev_q, const float* host_q, uint32_t nq, DevBuf* extra, FilterRun& run) {
  nvdb_status st;
  const size_t per_q = static_cast<size_t>(p.nq_pad) * 4;
  const struct { DevBuf& buf; size_t bytes; bool filter_flow; } workspace[] = {
      {c->thr, per_q, false}, {c->cnt, per_q, false}, {c->overflow, per_q, false}, {c->cand, static_cast<size_t>(nq) * p.cap * sizeof(Cand), false},
      {c->misc, 64, false}, {c->prog, static_cast<size_t>(p.prog_words) * 4, false}, {c->tickets, FUSE_TICKETS * 4, false},
      {c->q16, static_cast<size_t>(p.nq_pad) * c->fdim * 2, true}, {c->qscale, per_q, true}, {c->qinv, per_q, true},
      {c->ebound, per_q, true}, {c->slack, per_q, true}, {c->qdelta, per_q, true}};
  for (const auto& w : workspace)
    if ((p.prep || !w.filter_flow) && (st = ensure(c, w.buf, w.bytes))) return st;
  if (extra && (st = ensure(c, *extra, per_q))) return st;
  // what the last search's filter launches did, from the plan (the rest of "the last search" is the caller's to record)
  c->ev_filter.clear();
  c->last_filter_kind = p.filter ? p.kind : FILTER_NONE;
  if (p.filter) c->last_perm = p.perm_on;
  run = FilterRun{s, p.kind, p.perm_on, nq, p.QT, p.nq_pad, p.cap, static_cast<const float*>(c->thr.p)};
  // per-search resets and queries: the prep launch does both itself (option fuse), else init_search_kernel and a copy (one query tile: no siblings, no counters to reset)
  const uint32_t prog_words = p.QT > 1 ? p.prog_words : 0u;
  if (host_q && !p.prep_inits) { HIPCHK(c, hipMemcpyAsync(const_cast<float*>(dev_q), host_q, static_cast<size_t>(nq) * c->dim * 4, hipMemcpyDefault, s)); host_q = nullptr; }   // (host_q is the pinned block as the device addresses it)
  if (!p.prep_inits && (st = launch_init_search(c, s, p.nq_pad, prog_words))) return st;
  if (!p.prep) return NVDB_OK;
  PrepInit pinit{nullptr, nullptr, nullptr, nullptr, 0u, nullptr, nullptr, nullptr};
  if (p.prep_inits) pinit = PrepInit{static_cast<uint32_t*>(c->cnt.p), static_cast<float*>(c->thr.p), static_cast<uint32_t*>(c->misc.p), static_cast<uint32_t*>(c->prog.p),
                                     prog_words, static_cast<uint32_t*>(c->tickets.p), host_q, const_cast<float*>(dev_q)};   // (the copy is written only where host_q is read)
  return filter_is_i8(p.kind) ? launch_prep_q8(c, s, dev_q, nq, p.nq_pad, pinit) : launch_prep_q16(c, s, dev_q, nq, p.nq_pad, pinit);
}

// Enqueue one whole search of nq (<= 2048) queries resident at dev_q: plan (nvdb_plan.h), workspace, launches.  No host synchronisation.
// host_q != nullptr (host API, small calls): the queries are still in pinned host memory at host_q and `dev_q` is the device
// buffer they belong in -- the filter path's prep launch reads them over PCIe and fills dev_q itself, every other path gets a
// copy enqueued here.  status_out != nullptr: pinned host memory for the 8 status words; c->status_by_kernel tells the caller
// whether the search's last kernel wrote them (else it copies misc itself).
nvdb_status search_core(nvdb_hip_ctx* c, hipStream_t s, const float* dev_q, uint32_t nq, uint32_t k, uint64_t* dev_out_ids,
                        float* dev_out_scores, int force_path, bool time_filter, uint32_t cap_override = 0, bool sticky = true,
                        const float* host_q = nullptr, uint32_t* status_out = nullptr) {
  c->status_by_kernel = false;
  SearchPlan p;
  nvdb_status st = plan_search(*c, nq, k, force_path, cap_override, p);
  if (st) return fail(c, st, p.error);
  const int final_mode = sticky ? 1 : 3;          // select_kernel: 3 = final select without folding into the sticky self-check words
  const uint32_t n = static_cast<uint32_t>(c->n), k_eff = p.k_eff, cap = p.cap, QT = p.QT;
  // workspace, per-search resets, queries, prep; then the rest of the state of "the last search", all of it from the plan
  FilterRun run;
  if ((st = begin_filter_run(c, s, p, dev_q, host_q, nq, nullptr, run))) return st;
  c->stats = nvdb_hip_scan_stats{};
  c->stats.path = p.route;
  c->last_nq = nq; c->last_cap = cap; c->last_filter = p.filter;
  const float* slack = static_cast<const float*>(c->slack.p);

  if (p.route == ROUTE_ANYK) return search_largek(c, s, dev_q, nq, k, dev_out_ids, dev_out_scores);
  if (p.route == ROUTE_EXACT) {
    // prescan (plan_search): rows [0, head) alone, their exact k-th best score is the bar the rest of the scan starts with
    if (p.head && (st = launch_scan_exact(c, s, 0, p.head, dev_q, nq, k_eff, nullptr, cap, 0))) return st;
    if (p.head && (st = launch_select(c, s, nq, cap, k_eff, nullptr, 0, nullptr, nullptr, 0))) return st;
    if ((st = launch_scan_exact(c, s, p.head, n, dev_q, nq, k_eff, p.head ? run.thr : nullptr, cap, p.head ? k_eff : 0))) return st;
    c->stats.chunks = p.head ? 2 : 1;
    c->stats.rows_scanned = c->n;
    return launch_select(c, s, nq, cap, k_eff, nullptr, final_mode, dev_out_ids, dev_out_scores, k);
  }

  // ---- the filter route: bootstrap + select, { chunk + select }*, tail, rescore + final select ----
  // MFMA bootstrap: thresholds from the k-th largest of the tile maxima of rows [0, boot_rows); those rows are scanned again by
  // the normal build, so the select discards the bootstrap's entries (mode 2: out_k = list length)
  if (p.boot == BOOT_MFMA) st = launch_boot(c, run, p.boot_rows);
  else if (p.boot == BOOT_ANYK_SEEDED) st = search_largek(c, s, dev_q, nq, k_eff, nullptr, nullptr, p.r0, static_cast<Cand*>(c->cand.p), static_cast<uint32_t*>(c->cnt.p), cap);
  else st = launch_scan_exact(c, s, 0, p.r0, dev_q, nq, k_eff, nullptr, cap, 0);
  if (st) return st;
  // The int8 shadow's band is its widest term (||q|| x the largest quantisation residual of any row) counted twice under a list
  // score; the thresholding selects of such a search put ONE bound under an exact k-th best score instead (select_body, ExactBar)
  const float* xthr_q = (p.kind == FILTER_SHADOW8 && k_eff <= WAVE_KMAX && c->opt_shadow_exact_thr) ? dev_q : nullptr;
  if ((st = launch_select(c, s, nq, cap, k_eff, slack, p.boot == BOOT_MFMA ? 2 : 0, nullptr, nullptr, p.boot == BOOT_MFMA ? p.boot_tiles : 0, xthr_q))) return st;
  size_t ev = 0;
  for (uint32_t r = p.r0; r < p.n_al;) {
    const uint32_t hi = chunk_end(p, r);
    nvdb_hip_ctx::KLaunch kl{nullptr, nullptr, 0.0, 0.0};
    const bool acct = c->opt_time_kernels && c->klaunch.size() < 8192;
    if (acct) {
      // the kernel's own start/stop timestamps (events attached to the launch itself: no barrier packets, no gaps)
      for (hipEvent_t* e : {&kl.e0, &kl.e1}) {
        if (!c->kl_pool.empty()) { *e = c->kl_pool.back(); c->kl_pool.pop_back(); }
        else HIPCHK(c, hipEventCreate(e));
      }
      kl.flops = 2.0 * nq * static_cast<double>(std::min(hi, n) - r) * c->dim;   // algorithmic: real queries, real rows
      kl.bytes = static_cast<double>(std::min(hi, n) - r) * (filter_is_i8(run.kind) ? c->fdim + 4.0 : c->fdim * 2.0);   // rows streamed once
      run.e0 = kl.e0; run.e1 = kl.e1;
    } else if (time_filter) {
      run.e0 = get_event(c, ev); run.e1 = get_event(c, ev + 1);
    }
    if (time_filter && acct) { HIPCHK(c, hipEventRecord(get_event(c, ev), s)); }
    if ((st = launch_filter(c, run, {r, hi}))) return st;
    if (time_filter && acct) { HIPCHK(c, hipEventRecord(get_event(c, ev + 1), s)); }
    if (time_filter) { c->ev_filter.emplace_back(ev, ev + 1); ev += 2; }
    if (acct) c->klaunch.push_back(kl);
    if ((st = launch_select(c, s, nq, cap, k_eff, slack, 0, nullptr, nullptr, 0, xthr_q))) return st;
    c->stats.chunks++;
    c->stats.rows_scanned += static_cast<uint64_t>(hi - r) * QT;
    r = hi;
  }
  // ragged tail of an adopted corpus: exact scores, pruned by the current thresholds
  // (fewer than one tile of rows per workgroup: the wavefront lists' 64 entries keep every row that clears the threshold)
  if (p.tail_exact && (st = launch_scan_exact(c, s, p.n_al, n, dev_q, nq, std::min(k_eff, WAVE_KMAX), run.thr, cap, 0))) return st;
  if (p.tail_exact) c->stats.rows_scanned += static_cast<uint64_t>(n - p.n_al) * QT;
  // the final select rides in the rescore launch (one workgroup per query in both); its last workgroup folds the self-check words
  FinalSelect fs{};
  if (c->opt_fuse)
    fs = FinalSelect{final_mode, k_eff, k, c->row_base, reinterpret_cast<unsigned long long*>(dev_out_ids), dev_out_scores, static_cast<float*>(c->thr.p),
                     static_cast<uint32_t*>(c->overflow.p), static_cast<uint32_t*>(c->misc.p) + 6,
                     p.prep_inits ? static_cast<uint32_t*>(c->tickets.p) + (FUSE_TICKETS - 1) : nullptr, p.prep_inits ? status_out : nullptr};
  if (fs.mode == 1 && fs.ticket == nullptr) fs.mode = 0;          // (the sticky fold needs the ticket: separate select launch)
  bool fused = false;
  if ((st = launch_rescore(c, s, dev_q, nq, cap, fs, &fused))) return st;
  if (fused) { c->status_by_kernel = fs.status_out != nullptr; return NVDB_OK; }
  return launch_select(c, s, nq, cap, k_eff, nullptr, final_mode, dev_out_ids, dev_out_scores, k);
}

float filter_events_ms(const nvdb_hip_ctx* c) {
  float total = 0.f;
  for (auto& pr : c->ev_filter) { float ms = 0.f; if (hipEventElapsedTime(&ms, c->ev_pool[pr.first], c->ev_pool[pr.second]) == hipSuccess) total += ms; }
  return total;
}

// candidates that reached the rescore = the list lengths left by the last thresholding select (the final select
// does not touch them); summed here rather than by 1024 same-address atomics in the rescore kernel
nvdb_status sum_candidates(nvdb_hip_ctx* c, unsigned long long* total) {
  *total = 0;
  if (!c->last_nq) return NVDB_OK;
  std::vector<uint32_t> cn(c->last_nq);
  HIPCHK(c, hipMemcpy(cn.data(), c->cnt.p, c->last_nq * 4, hipMemcpyDeviceToHost));
  for (uint32_t v : cn) *total += std::min(v, c->last_cap);
  return NVDB_OK;
}

// a query with a NaN / infinite element is flagged like a list overflow by the prep launch, with a negative error bound
static nvdb_status any_non_finite_query(nvdb_hip_ctx* c, uint32_t nq, bool* any) {
  std::vector<float> eb(nq);
  HIPCHK(c, hipMemcpy(eb.data(), c->ebound.p, static_cast<size_t>(nq) * 4, hipMemcpyDeviceToHost));
  *any = std::any_of(eb.begin(), eb.end(), [](float v) { return v < 0.f; });
  return NVDB_OK;
}

// One sub-batch (<= 1024 queries) of the host API: search, and when the self-check tripped (rare) redo it.  The ladder after a filter
// attempt whose lists or wave logs overflowed:
//   rung 1a  (the attempt streamed the int8 shadow and the fp16 filter stands beside it) the fp16 filter at the same list capacity --
//            the shadow's band is the widest (||q|| x the largest quantisation residual of ANY row), so a corpus that quantises badly
//            overflows there alone; the context is marked shadow_demoted and later searches start on the fp16 filter
//   rung 1b  the filter with the longest candidate lists the select kernel can sort (near-duplicate-heavy corpora: thousands of rows
//            inside the filter's error band of the k-th score; re-scoring them is cheap, only the list was too short)
//   rung 2   if that is still not enough, the bound itself was violated, or a query is not finite: the always-correct exact path.
// (The queries are in the device buffer by then: the retries read them there.)  verdict(rung) waits for the attempt and says
// NVDB_ERR_INTERNAL when its self-check tripped; at rung 0 it leaves the exact counts in c->stats (search_check_impl).
// *part: the statistics of the FIRST attempt, the ones that are reported; *kind: what its filter launches streamed.
template <typename Verdict>
static nvdb_status search_sub_batch(nvdb_hip_ctx* c, hipStream_t s, const float* dq, uint32_t nq, uint32_t k, uint64_t* oi, float* os, bool time_filter,
                                    const float* host_q, uint32_t* st_out, Verdict&& verdict, nvdb_hip_scan_stats* part, FilterKind* kind, bool* tripped = nullptr) {
  nvdb_status st;
  if ((st = search_core(c, s, dq, nq, k, oi, os, 0, time_filter, 0, false, host_q, st_out))) return st;
  *kind = c->last_filter_kind;
  nvdb_status chk = verdict(0);
  *part = c->stats;
  if (tripped) *tripped = chk == NVDB_ERR_INTERNAL;
  if (chk != NVDB_ERR_INTERNAL) return chk;
  const uint32_t cap0 = c->last_cap;
  bool retry_filter = part->path == 2 && !part->bound_violations;
  if (retry_filter && c->last_filter_kind == FILTER_SHADOW8 && f16_beside_shadow(c)) {
    bool non_finite = false;
    if ((st = any_non_finite_query(c, nq, &non_finite))) return st;
    if (non_finite) retry_filter = false;
    else {
      c->shadow_demoted = true;                            // (plan_search now picks the fp16 filter, here and in later searches)
      if ((st = search_core(c, s, dq, nq, k, oi, os, 2, false, cap0, false, nullptr, st_out))) return st;
      if ((chk = verdict(1)) != NVDB_OK && chk != NVDB_ERR_INTERNAL) return chk;
    }
  }
  if (chk != NVDB_OK && retry_filter && cap0 < SELECT_MAX_CAP) {
    if ((st = search_core(c, s, dq, nq, k, oi, os, 2, false, SELECT_MAX_CAP, false, nullptr, st_out))) return st;
    if ((chk = verdict(1)) == NVDB_OK) c->cap_hint = SELECT_MAX_CAP;
    else if (chk != NVDB_ERR_INTERNAL) return chk;
  }
  if (chk != NVDB_OK) {
    if ((st = search_core(c, s, dq, nq, k, oi, os, 1, false, 0, false, nullptr, st_out))) return st;
    if ((chk = verdict(2)) != NVDB_OK && chk != NVDB_ERR_INTERNAL) return chk;
  }
  c->stats = *part;
  return NVDB_OK;
}

// (shmem_bytes: the dynamic LDS of the 32x32 filter builds, filter_f16_lds_bytes / filter_i8_lds_bytes at the corpus' dim -- what
// the ABI's callers have always been told; kind: what the reported attempt's filter launches streamed)
static void fill_timing(const nvdb_hip_ctx* c, nvdb_hip_timing* t, const hipEvent_t (&e)[4], uint32_t k, uint32_t path, FilterKind kind) {
  (void)hipEventElapsedTime(&t->h2d_ms, e[0], e[1]);
  (void)hipEventElapsedTime(&t->kernel_ms, e[1], e[2]);
  (void)hipEventElapsedTime(&t->d2h_ms, e[2], e[3]);
  t->total_ms = t->h2d_ms + t->kernel_ms + t->d2h_ms;
  t->threads = 256; t->nwarps = 4; t->K = k;
  t->shmem_bytes = path != 2 ? 0 : filter_is_i8(kind) ? static_cast<size_t>(FILTER_STAGES_I8) * (FILTER_ROWS * c->fdim + 4096) : static_cast<size_t>(FILTER_STAGES) * FILTER_ROWS * c->fdim * 2;
}

}  // namespace nvdbhip

extern "C" {

static nvdb_status search_args(nvdb_hip_ctx* c, const void* q, uint32_t nq, uint32_t k, const void* oi, const void* os) {
  if (!c) return NVDB_ERR_INVALID;
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (nq > 0 && k > 0 && (!q || !oi || !os)) return fail(c, NVDB_ERR_INVALID, q ? "null output" : "Null query");
  return NVDB_OK;
}

nvdb_status nvdb_hip_search_batch_dev(nvdb_hip_ctx* c, const float* dev_q, uint32_t nq, uint32_t k, uint64_t* dev_out_ids,
                                      float* dev_out_scores, void* hip_stream) {
  nvdb_status st = search_args(c, dev_q, nq, k, dev_out_ids, dev_out_scores);
  if (st) return st;
  if (nq == 0 || k == 0) return NVDB_OK;
  if (nq > 2048) return fail(c, NVDB_ERR_UNSUPPORTED, "search_batch_dev: at most 2048 queries per call");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
  return search_core(c, s, dev_q, nq, k, dev_out_ids, dev_out_scores, 0, false);
}

// own_only: the host API's view of ITS OWN last search (misc[0], [1], per-query flags); the sticky words that device-API
// searches left for the caller's next nvdb_hip_search_check are neither read into the verdict nor cleared
static nvdb_status search_check_impl(nvdb_hip_ctx* c, nvdb_hip_scan_stats* stats, bool own_only) {
  if (!c) return NVDB_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  // caller has synchronised its stream; read the self-check words
  std::vector<uint32_t> ovf(c->last_nq);
  uint32_t misc[16] = {0};
  if (c->last_nq) HIPCHK(c, hipMemcpy(ovf.data(), c->overflow.p, c->last_nq * 4, hipMemcpyDeviceToHost));
  if (c->misc.p) {
    HIPCHK(c, hipMemcpy(misc, c->misc.p, 64, hipMemcpyDeviceToHost));
    if (own_only) misc[12] = misc[13] = misc[14] = 0;
    const uint32_t zero[3] = {0, 0, 0};             // sticky words (select_kernel): what ANY search since the last check found
    if (misc[12] | misc[13] | misc[14]) HIPCHK(c, hipMemcpy(static_cast<uint32_t*>(c->misc.p) + 12, zero, 12, hipMemcpyHostToDevice));
  }
  c->stats.sticky_overflow = (misc[12] | misc[14]) ? 1u : 0u;
  c->stats.sticky_violations = misc[13];
  c->stats.i8_stage1_tiles = misc[4]; c->stats.i8_stage2_blocks = misc[5];
  uint32_t nov = 0;
  for (uint32_t v : ovf) nov += v ? 1u : 0u;
  if (std::getenv("NVDB_DEBUG_OVERFLOW") && (nov || misc[1])) {
    std::vector<uint32_t> cn(c->last_nq);
    (void)hipMemcpy(cn.data(), c->cnt.p, c->last_nq * 4, hipMemcpyDeviceToHost);
    std::fprintf(stderr, "[nvdb debug] log_overflow=%u list flags:", misc[1]);
    for (uint32_t q = 0; q < c->last_nq; ++q) if (ovf[q]) std::fprintf(stderr, " q%u(cnt=%u)", q, cn[q]);
    std::fprintf(stderr, "\n");
  }
  if (misc[1]) nov = c->last_nq;                 // a wave's survivor log overflowed: which queries lost entries is unknown
  c->stats.overflow_queries = nov;
  c->stats.bound_violations = misc[0];
  unsigned long long tot = 0;
  if (c->last_filter) { if (nvdb_status st = sum_candidates(c, &tot)) return st; }
  c->stats.candidates = tot;
  c->stats.filter_kernel_ms = filter_events_ms(c);
  if (stats) *stats = c->stats;
  if (misc[0]) return fail(c, NVDB_ERR_INTERNAL, "filter error bound violated (bound_violations > 0)");
  if (nov) return fail(c, NVDB_ERR_INTERNAL, "candidate list overflow: re-run these queries with option path=1");
  if (misc[13]) return fail(c, NVDB_ERR_INTERNAL, "filter error bound violated in an earlier search since the last check");
  if (misc[12] | misc[14]) return fail(c, NVDB_ERR_INTERNAL, "candidate list overflow in an earlier search since the last check");
  return NVDB_OK;
}

nvdb_status nvdb_hip_search_check(nvdb_hip_ctx* c, nvdb_hip_scan_stats* stats) { return search_check_impl(c, stats, false); }

nvdb_status nvdb_hip_search_batch(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_ids,
                                  float* out_scores, uint32_t* out_k_eff, nvdb_hip_timing* timing) {
  nvdb_status st = search_args(c, queries, nq, k, out_ids, out_scores);
  if (st) return st;
  if (timing) std::memset(timing, 0, sizeof(*timing));
  if (out_k_eff) *out_k_eff = static_cast<uint32_t>(std::min<uint64_t>(k, c->n));
  if (nq == 0 || k == 0) return NVDB_OK;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t qbytes = static_cast<size_t>(nq) * c->dim * 4;
  if ((st = ensure_q32(c, s, qbytes))) return st;
  if (nq <= 1024) { if ((st = ensure_hostblock(c, static_cast<size_t>(nq) * k * 12))) return st; }
  else {
    if ((st = ensure(c, c->out_ids, static_cast<size_t>(nq) * k * 8))) return st;
    if ((st = ensure(c, c->out_scores, static_cast<size_t>(nq) * k * 4))) return st;
  }
  const hipEvent_t e[4] = {get_event(c, 60), get_event(c, 61), get_event(c, 62), get_event(c, 63)};
  c->stats_lazy = false;
  const bool time_filter = timing != nullptr && c->opt_time_launches;
  auto zero_pad = [&]() -> nvdb_status { return zero_q32_pad(c, s, qbytes); };
  nvdb_hip_scan_stats total{};
  FilterKind kind = FILTER_NONE;
  if (nq <= 1024) {
    // One sub-batch: everything the host needs comes back in ONE synchronisation through pinned staging -- the
    // self-check words (32 B), ids and scores -- instead of five small pageable copies of ~20 us each (a third of
    // a single-query search at N = 1M).  Small query blocks go up through the same staging buffer.
    // Small calls (zero_copy, round 4) enqueue NO copy at all: the prep launch reads the queries from the pinned block over
    // PCIe (and leaves the device copy the later kernels read), the final launch writes ids, scores and -- its last workgroup --
    // the status words into the pinned block; the host only synchronises.  Two blit launches + their gaps less per search.
    const size_t ob_ids = static_cast<size_t>(nq) * k * 8, ob_sc = static_cast<size_t>(nq) * k * 4;
    const size_t q_stage = qbytes <= 64 * 1024 ? qbytes : 0;
    const bool stage_out = ob_ids + ob_sc <= (static_cast<size_t>(16) << 20);     // very large k: results go straight to the caller's buffers
    const bool zc_in = c->opt_zero_copy && q_stage != 0;
    const bool zc_out = c->opt_zero_copy && stage_out && ob_ids + ob_sc <= 64 * 1024;
    const size_t need = 64 + (stage_out ? ob_ids + ob_sc : 0) + q_stage;
    if (c->pinned_bytes < need) {
      if (c->pinned) (void)hipHostFree(c->pinned);
      c->pinned = nullptr; c->pinned_bytes = 0; c->pinned_dev = nullptr;
      HIPCHK(c, hipHostMalloc(&c->pinned, need + need / 2, hipHostMallocDefault));
      c->pinned_bytes = need + need / 2;
      HIPCHK(c, hipHostGetDevicePointer(&c->pinned_dev, c->pinned, 0));
    }
    char* pin = static_cast<char*>(c->pinned);
    char* pin_d = static_cast<char*>(c->pinned_dev);                              // the same block as the kernels address it
    uint32_t* pin_status = reinterpret_cast<uint32_t*>(pin);
    const size_t off_ids = 64, off_sc = off_ids + (stage_out ? ob_ids : 0), off_q = off_sc + (stage_out ? ob_sc : 0);
    char* pin_ids = pin + off_ids; char* pin_sc = pin + off_sc; char* pin_q = pin + off_q;
    if (timing) HIPCHK(c, hipEventRecord(e[0], s));
    if ((st = zero_pad())) return st;
    const float* host_q = nullptr;                                                 // non-null: search_core brings the queries down itself
    if (q_stage) {
      std::memcpy(pin_q, queries, qbytes);
      if (zc_in) host_q = reinterpret_cast<const float*>(pin_d + off_q);
      else HIPCHK(c, hipMemcpyAsync(c->q32.p, pin_q, qbytes, hipMemcpyHostToDevice, s));
    } else HIPCHK(c, hipMemcpyAsync(c->q32.p, queries, qbytes, hipMemcpyHostToDevice, s));
    if (timing) HIPCHK(c, hipEventRecord(e[1], s));
    const float* dq = static_cast<const float*>(c->q32.p);
    uint64_t* oi = zc_out ? reinterpret_cast<uint64_t*>(pin_d + off_ids) : reinterpret_cast<uint64_t*>(static_cast<char*>(c->hostblock.p) + 64);
    float* os = zc_out ? reinterpret_cast<float*>(pin_d + off_sc) : reinterpret_cast<float*>(static_cast<char*>(c->hostblock.p) + 64 + ob_ids);
    uint32_t* st_out = zc_out ? reinterpret_cast<uint32_t*>(pin_d) : nullptr;
    // the verdict comes down with the results: the pinned status words
    auto verdict = [&](int rung) -> nvdb_status {
      if (rung == 0 && timing) HIPCHK(c, hipEventRecord(e[2], s));
      if (zc_out) {
        // ids and scores were written into the pinned block by the final kernel; the status words too when that kernel was the
        // fused rescore + select (else: 32 bytes copied here)
        if (!c->status_by_kernel) HIPCHK(c, hipMemcpyAsync(pin_status, c->misc.p, 32, hipMemcpyDeviceToHost, s));
      } else if (stage_out) {
        // status words, ids and scores are adjacent on the device (ensure_hostblock) and in the staging buffer: ONE copy
        HIPCHK(c, hipMemcpyAsync(pin, c->hostblock.p, 64 + ob_ids + ob_sc, hipMemcpyDeviceToHost, s));
      } else {
        HIPCHK(c, hipMemcpyAsync(pin_status, c->misc.p, 32, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(out_ids, oi, ob_ids, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(out_scores, os, ob_sc, hipMemcpyDeviceToHost, s));
      }
      if (timing) HIPCHK(c, hipEventRecord(e[3], s));
      HIPCHK(c, hipStreamSynchronize(s));
      if (!(pin_status[0] | pin_status[1] | pin_status[6])) return NVDB_OK;
      // tripped; the first attempt's exact counts for the statistics
      return (rung == 0 && search_check_impl(c, nullptr, true) == NVDB_ERR_HIP) ? NVDB_ERR_HIP : NVDB_ERR_INTERNAL;
    };
    bool tripped = false;
    if ((st = search_sub_batch(c, s, dq, nq, k, oi, os, time_filter, host_q, st_out, verdict, &total, &kind, &tripped))) return st;
    if (!tripped) {
      total.i8_stage1_tiles = pin_status[4]; total.i8_stage2_blocks = pin_status[5];
      total.filter_kernel_ms = filter_events_ms(c);
      c->stats = total;
      c->stats_lazy = c->last_filter;                 // candidates: read back on demand
    }
    if (stage_out) {
      std::memcpy(out_ids, pin_ids, ob_ids);
      std::memcpy(out_scores, pin_sc, ob_sc);
    }
  } else {
    if ((st = zero_pad())) return st;
    HIPCHK(c, hipEventRecord(e[0], s));
    HIPCHK(c, hipMemcpyAsync(c->q32.p, queries, qbytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(e[1], s));
    auto verdict = [&](int rung) -> nvdb_status {     // (nothing reads the verdict of the exact path)
      HIPCHK(c, hipStreamSynchronize(s));
      return rung < 2 ? search_check_impl(c, nullptr, true) : NVDB_OK;
    };
    for (uint32_t q0 = 0; q0 < nq; q0 += 1024) {
      const float* dq = static_cast<const float*>(c->q32.p) + static_cast<size_t>(q0) * c->dim;
      uint64_t* oi = static_cast<uint64_t*>(c->out_ids.p) + static_cast<size_t>(q0) * k;
      float* os = static_cast<float*>(c->out_scores.p) + static_cast<size_t>(q0) * k;
      nvdb_hip_scan_stats part{};
      if ((st = search_sub_batch(c, s, dq, std::min<uint32_t>(1024, nq - q0), k, oi, os, time_filter, nullptr, nullptr, verdict, &part, &kind))) return st;
      total.path = std::max(total.path, part.path);
      total.chunks += part.chunks; total.rows_scanned += part.rows_scanned; total.candidates += part.candidates;
      total.overflow_queries += part.overflow_queries; total.bound_violations += part.bound_violations;
      total.i8_stage1_tiles += part.i8_stage1_tiles; total.i8_stage2_blocks += part.i8_stage2_blocks;
      total.filter_kernel_ms += part.filter_kernel_ms;
    }
    HIPCHK(c, hipEventRecord(e[2], s));
    HIPCHK(c, hipMemcpyAsync(out_ids, c->out_ids.p, static_cast<size_t>(nq) * k * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(out_scores, c->out_scores.p, static_cast<size_t>(nq) * k * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipEventRecord(e[3], s));
    HIPCHK(c, hipStreamSynchronize(s));
    c->stats = total;
  }
  if (timing) fill_timing(c, timing, e, k, total.path, kind);
  if (total.bound_violations) return fail(c, NVDB_ERR_INTERNAL, "filter error bound violated; results were recomputed on the exact path");
  return NVDB_OK;
}

nvdb_status nvdb_hip_collect_kernel_times(nvdb_hip_ctx* c, uint32_t* launches, double* total_ms, double* total_flops,
                                          double* total_bytes) {
  if (!c) return NVDB_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  double ms = 0, fl = 0, by = 0;
  uint32_t cnt = 0;
  for (auto& k : c->klaunch) {
    float t = 0.f;
    HIPCHK(c, hipEventSynchronize(k.e1));
    HIPCHK(c, hipEventElapsedTime(&t, k.e0, k.e1));
    ms += t; fl += k.flops; by += k.bytes; ++cnt;
    c->kl_pool.push_back(k.e0); c->kl_pool.push_back(k.e1);
  }
  c->klaunch.clear();
  if (launches) *launches = cnt;
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = fl;
  if (total_bytes) *total_bytes = by;
  return NVDB_OK;
}

}  // extern "C"
