// nvdb_refine.cpp -- exact-L2 refine rerank (reference src/cuda_refine.cu:839-1173; kernels: kernels_refine.h).
#include "nvdb_ctx.h"
#include "kernels_refine.h"

// ---- refine -----------------------------------------------------------------------------------------
static nvdb_status refine_args(nvdb_hip_ctx* c, const void* q, const void* cand, uint32_t K, const void* out_ids) {
  if (!c) return NVDB_ERR_INVALID;
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (c->dtype != NVDB_DTYPE_F16 && c->dtype != NVDB_DTYPE_F32)
    return fail(c, NVDB_ERR_UNSUPPORTED, "refine supports base dtype fp16/fp32 only");
  if (K > NVDB_HIP_REFINE_KMAX) return fail(c, NVDB_ERR_INVALID, "refine: K not supported (K<=64)");
  if (!q || !cand || !out_ids) return fail(c, NVDB_ERR_INVALID, "refine: null pointer");
  return NVDB_OK;
}

// the kernel build of one refine call and how it is launched.  lds: its dynamic LDS.  takes_dim: v1 / v2 take the row length as
// their third argument, v3 has it as a template parameter and takes none (an ignored argument would move its kernarg offsets)
struct RefineChoice { const void* fn; uint32_t threads, waves; size_t lds; bool takes_dim; };
// ... and what the timing struct reports of it
struct RefineLaunch { uint32_t threads = 0, nwarps = 0; size_t lds = 0; };

template <typename... A> static const void* kernel_ptr(void (*k)(A...)) { return reinterpret_cast<const void*>(k); }

// STAMP: the stamped build of the same template (same arithmetic, same results; option refine_dbg_q)
template <bool STAMP>
static RefineChoice choose_refine(const nvdb_hip_ctx* c) {
  const bool f16 = c->dtype == NVDB_DTYPE_F16, al = aligned_rows(c->dtype, c->dim);
  RefineChoice k{};
  nvdb_status st = NVDB_OK;
  // v3 (whole rows per request, four lanes per row): fp16 rows of 512 / 768 / 1024 / 1536 bytes
  if (c->opt_refine_v2 >= 2 && f16 && dispatch_dim(Refine3Dims{}, c->dim, st, [&](auto D) {
        constexpr int DIM = decltype(D)::value;
        k = {kernel_ptr(refine_l2_rows_kernel<DIM, STAMP>), 64 * REFINE3_WAVES, REFINE3_WAVES, static_cast<size_t>(REFINE3_WAVES) * refine3_slot_bytes<DIM>(), false};
        return NVDB_OK;
      }))
    return k;
  // v2 (coalesced gather through LDS): whole 16-byte steps only (f16: dim % 8 == 0, f32: dim % 4 == 0)
  if (al && c->opt_refine_v2 && static_cast<uint64_t>(c->dim) * bpe_of(c->dtype) >= 256)
    return {kernel_ptr(f16 ? refine_l2_lds_kernel<DT_F16, STAMP> : refine_l2_lds_kernel<DT_F32, STAMP>), 256, 4, 4 * 2 * 64 * 256, true};
  if (f16) return {kernel_ptr(al ? refine_l2_kernel<DT_F16, true, STAMP> : refine_l2_kernel<DT_F16, false, STAMP>), 256, 4, 0, true};
  return {kernel_ptr(al ? refine_l2_kernel<DT_F32, true, STAMP> : refine_l2_kernel<DT_F32, false, STAMP>), 256, 4, 0, true};
}

// dbg != nullptr: wave 0 of the first dbg_q workgroups writes its phase cycles to dbg[3q ..]
static nvdb_status launch_refine(nvdb_hip_ctx* c, hipStream_t s, const float* dq, const uint32_t* dc, uint32_t Q, uint32_t R,
                                 uint32_t K, uint32_t* doi, float* dod, uint64_t* dbg = nullptr, uint32_t dbg_q = 0,
                                 RefineLaunch* launched = nullptr) {
  const RefineChoice k = dbg ? choose_refine<true>(c) : choose_refine<false>(c);
  if (launched) *launched = {k.threads, k.waves, k.lds ? k.lds : refine_merge_bytes(k.waves)};   // v1 has the merge lists only
  nvdb_status st;
  if (k.lds && (st = raise_lds_limit(c, k.fn, k.lds))) return st;
  std::vector<void*> args = {&c->rows, &c->n};
  if (k.takes_dim) args.push_back(&c->dim);
  args.insert(args.end(), {&dq, &dc, &R, &K, &doi, &dod, &dbg, &dbg_q});
  HIPCHK(c, hipLaunchKernel(k.fn, dim3(Q), dim3(k.threads), args.data(), k.lds, s));
  return NVDB_OK;
}

extern "C" {

nvdb_status nvdb_hip_refine_l2_topk_dev(nvdb_hip_ctx* c, const float* dq, const uint32_t* dc, uint32_t Q, uint32_t R, uint32_t K,
                                        uint32_t* doi, float* dod, void* hip_stream) {
  if (c && (K == 0 || Q == 0 || R == 0)) return NVDB_OK;
  nvdb_status st = refine_args(c, dq, dc, K, doi);
  if (st) return st;
  HIPCHK(c, hipSetDevice(c->device));
  return launch_refine(c, hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream, dq, dc, Q, R, K, doi, dod);
}

nvdb_status nvdb_hip_refine_l2_topk(nvdb_hip_ctx* c, const float* queries, const uint32_t* cand_ids, uint32_t Q, uint32_t R,
                                    uint32_t K, uint32_t* out_ids, float* out_dist, nvdb_hip_timing* timing) {
  if (timing) std::memset(timing, 0, sizeof(*timing));
  if (c && (K == 0 || Q == 0 || R == 0)) return NVDB_OK;       // cuda_refine.cu:853-857
  nvdb_status st = refine_args(c, queries, cand_ids, K, out_ids);
  if (st) return st;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t qb = static_cast<size_t>(Q) * c->dim * 4, cb = static_cast<size_t>(Q) * R * 4, ob = static_cast<size_t>(Q) * K * 4;
  if ((st = ensure(c, c->rq, qb))) return st;
  if ((st = ensure(c, c->rcand, cb))) return st;
  if ((st = ensure(c, c->rout_ids, ob))) return st;
  if ((st = ensure(c, c->rout_dist, ob))) return st;
  // phase stamps (reference CUDA_DBG_TIMING / CUDA_DBG_Q, cuda_refine.cu:863-872): only with a timing struct to report them in
  const uint32_t dbg_q = (timing && c->opt_refine_dbg_q > 0) ? static_cast<uint32_t>(std::min<int64_t>(c->opt_refine_dbg_q, Q)) : 0u;
  const size_t dbgb = static_cast<size_t>(dbg_q) * 3 * sizeof(uint64_t);
  if (dbg_q) {
    if ((st = ensure(c, c->rdbg, dbgb))) return st;
    HIPCHK(c, hipMemsetAsync(c->rdbg.p, 0, dbgb, s));
  }
  hipEvent_t e0 = get_event(c, 56), e1 = get_event(c, 57), e2 = get_event(c, 58), e3 = get_event(c, 59);
  // optional pinned staging (reference: CUDA_PINNED, src/cuda_refine.cu:875, 902-914): inputs are packed into pinned host
  // buffers BEFORE the timed region, the asynchronous copies then run at the link's rate instead of through the runtime's
  // pageable bounce buffers; results come back into pinned memory and are copied out after the synchronisation.
  const void* h_q = queries;
  const void* h_c = cand_ids;
  void* h_oi = out_ids;
  void* h_od = out_dist;
  if (c->opt_refine_pinned) {
    const size_t need = qb + cb + 2 * ob;
    if (c->rpinned_bytes < need) {
      if (c->rpinned) (void)hipHostFree(c->rpinned);
      c->rpinned = nullptr; c->rpinned_bytes = 0;
      HIPCHK(c, hipHostMalloc(&c->rpinned, need, hipHostMallocDefault));
      c->rpinned_bytes = need;
    }
    char* pin = static_cast<char*>(c->rpinned);
    std::memcpy(pin, queries, qb);
    std::memcpy(pin + qb, cand_ids, cb);
    h_q = pin; h_c = pin + qb; h_oi = pin + qb + cb; h_od = pin + qb + cb + ob;
  }
  HIPCHK(c, hipEventRecord(e0, s));
  HIPCHK(c, hipMemcpyAsync(c->rq.p, h_q, qb, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->rcand.p, h_c, cb, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipEventRecord(e1, s));
  RefineLaunch launched;
  if ((st = launch_refine(c, s, static_cast<const float*>(c->rq.p), static_cast<const uint32_t*>(c->rcand.p), Q, R, K,
                          static_cast<uint32_t*>(c->rout_ids.p), out_dist ? static_cast<float*>(c->rout_dist.p) : nullptr,
                          dbg_q ? static_cast<uint64_t*>(c->rdbg.p) : nullptr, dbg_q, &launched)))
    return st;
  HIPCHK(c, hipEventRecord(e2, s));
  HIPCHK(c, hipMemcpyAsync(h_oi, c->rout_ids.p, ob, hipMemcpyDeviceToHost, s));
  if (out_dist) HIPCHK(c, hipMemcpyAsync(h_od, c->rout_dist.p, ob, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipEventRecord(e3, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (c->opt_refine_pinned) {
    std::memcpy(out_ids, h_oi, ob);
    if (out_dist) std::memcpy(out_dist, h_od, ob);
  }
  if (timing) {
    (void)hipEventElapsedTime(&timing->h2d_ms, e0, e1);
    (void)hipEventElapsedTime(&timing->kernel_ms, e1, e2);
    (void)hipEventElapsedTime(&timing->d2h_ms, e2, e3);
    timing->total_ms = timing->h2d_ms + timing->kernel_ms + timing->d2h_ms;
    timing->threads = launched.threads; timing->nwarps = launched.nwarps; timing->K = K; timing->R = R;
    timing->shmem_bytes = launched.lds;
  }
  if (dbg_q) {                                   // after the events: h2d / kernel / d2h keep their meaning (cuda_refine.cu:1116-1144)
    std::vector<uint64_t> h(static_cast<size_t>(dbg_q) * 3);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->rdbg.p, dbgb, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    double sum[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = 0; i < dbg_q; ++i)
      for (int p = 0; p < 3; ++p) sum[p] += static_cast<double>(h[static_cast<size_t>(i) * 3 + p]);
    timing->dbg_q = dbg_q;
    timing->dbg_dist_cycles_avg = sum[0] / dbg_q;
    timing->dbg_write_cycles_avg = sum[1] / dbg_q;
    timing->dbg_merge_cycles_avg = sum[2] / dbg_q;
    const double tot = timing->dbg_dist_cycles_avg + timing->dbg_write_cycles_avg + timing->dbg_merge_cycles_avg;
    timing->dbg_dist_pct = tot > 0.0 ? timing->dbg_dist_cycles_avg / tot : 0.0;     // fractions, like the reference's *_pct
    timing->dbg_write_pct = tot > 0.0 ? timing->dbg_write_cycles_avg / tot : 0.0;
    timing->dbg_merge_pct = tot > 0.0 ? timing->dbg_merge_cycles_avg / tot : 0.0;
  }
  return NVDB_OK;
}

}  // extern "C"
