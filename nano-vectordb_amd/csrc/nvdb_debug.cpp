// nvdb_debug.cpp -- developer entry points (include/nvdb_hip_dev.h): stamped builds of the filter kernels, the device's
// tile partition function, the plan of a search for a shape given as plain numbers (no device).  Compiled into libnvdb_hip_dev.so only; the product library does not contain this file's code.
#ifdef NVDB_HIP_DEV
#include "nvdb_plan.h"
#include "kernels_filter_i8s.h"

namespace {
__global__ void fill_u32_kernel(uint32_t* p, uint32_t v, size_t n) {
  size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// What the two clock entry points share.  `launch` enqueues one stamped launch; they run back to back in bursts of CLOCK_BURST (the
// rendezvous counters, the first prog_bytes of c->prog, reset ahead of each) until `seconds` have passed, and the last burst is timed
// (`before_timed` is enqueued ahead of it).  Then the stamp pairs every workgroup's wave 0 left behind the counters are read back.
constexpr uint32_t CLOCK_BURST = 8;
struct ClockStats {
  float ms = 0.f;                                  // per launch of the timed burst
  float ghz[3] = {0.f, 0.f, 0.f};                  // median, min, max over the workgroups that stamped: delta(s_memtime) / delta(s_memrealtime) x 100 MHz
  std::vector<double> us;                          // the tile loop's duration per workgroup (realtime ticks at 100 MHz; 0: no stamp)
  uint32_t stamped = 0;
  double sum_us = 0.0, max_us = 0.0;               // over the workgroups that stamped
};
template <typename Launch, typename BeforeTimed>
nvdb_status clock_bursts(nvdb_hip_ctx* c, uint32_t nwg, size_t prog_bytes, float seconds, Launch launch, BeforeTimed before_timed, ClockStats& out) {
  hipEvent_t e0, e1;
  HIPCHK(c, hipEventCreate(&e0)); HIPCHK(c, hipEventCreate(&e1));
  // a workgroup without tiles (a corpus of fewer tiles than row streams) leaves no stamp: its pair reads 0, not what the buffer held
  HIPCHK(c, hipMemsetAsync(static_cast<char*>(c->prog.p) + prog_bytes, 0, static_cast<size_t>(nwg) * 16, c->stream));
  const auto t_start = std::chrono::steady_clock::now();
  for (;;) {
    const bool last = std::chrono::duration<float>(std::chrono::steady_clock::now() - t_start).count() >= seconds;
    if (last) { if (nvdb_status st = before_timed()) return st; HIPCHK(c, hipEventRecord(e0, c->stream)); }
    for (uint32_t r = 0; r < CLOCK_BURST; ++r) {
      HIPCHK(c, hipMemsetAsync(c->prog.p, 0xFF, prog_bytes, c->stream));
      if (nvdb_status st = launch()) return st;
    }
    if (last) break;
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  HIPCHK(c, hipEventRecord(e1, c->stream));
  HIPCHK(c, hipEventSynchronize(e1));
  HIPCHK(c, hipEventElapsedTime(&out.ms, e0, e1));
  out.ms /= static_cast<float>(CLOCK_BURST);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  std::vector<uint64_t> stamps(static_cast<size_t>(nwg) * 2);
  HIPCHK(c, hipMemcpy(stamps.data(), static_cast<const char*>(c->prog.p) + prog_bytes, stamps.size() * 8, hipMemcpyDeviceToHost));
  std::vector<float> ghz;
  out.us.assign(nwg, 0.0);
  for (uint32_t w = 0; w < nwg; ++w) {
    if (!stamps[2 * w + 1]) continue;
    ghz.push_back(static_cast<float>(static_cast<double>(stamps[2 * w]) / static_cast<double>(stamps[2 * w + 1]) * 0.1));
    out.us[w] = static_cast<double>(stamps[2 * w + 1]) * 0.01;
    out.sum_us += out.us[w]; out.max_us = std::max(out.max_us, out.us[w]); ++out.stamped;
  }
  std::sort(ghz.begin(), ghz.end());
  if (!ghz.empty()) { out.ghz[0] = ghz[ghz.size() / 2]; out.ghz[1] = ghz.front(); out.ghz[2] = ghz.back(); }
  return NVDB_OK;
}
}  // namespace

extern "C" {

nvdb_status nvdb_hip_debug_clock(nvdb_hip_ctx* c, int variant, uint32_t nq, float seconds, float* out4) {
  if (!c || !out4) return NVDB_ERR_INVALID;
  if (variant != 0 && variant != 20) return fail(c, NVDB_ERR_INVALID, "debug: unknown variant");
  if (!c->rows || c->dtype != NVDB_DTYPE_F16 || c->dim != 768 || !c->q16.p) return fail(c, NVDB_ERR_UNSUPPORTED, "debug: run a path-2 search on an fp16 d=768 corpus first");
  if (nq <= 128 || nq > (c->last_nq + 255u) / 256u * 256u) return fail(c, NVDB_ERR_UNSUPPORTED, "debug: 128 < nq <= the last search's padded batch");
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t QT = (nq + 255) / 256, nq_pad = QT * 256;
  const uint32_t nwg = filter_grid(c, QT);
  if (!xcd_aware_grid(QT, nwg)) return fail(c, NVDB_ERR_UNSUPPORTED, "debug: batch does not map onto the XCD-aware grid");
  DevBuf inf;                                      // thresholds +inf: no survivors, the streaming / MFMA machinery alone
  nvdb_status st = ensure(c, inf, nq_pad * 4);
  if (st) return st;
  fill_u32_kernel<<<(nq_pad + 255) / 256, 256, 0, c->stream>>>(static_cast<uint32_t*>(inf.p), 0x7F800000u, nq_pad);
  const size_t prog_bytes = static_cast<size_t>(nwg) * 8 * 4, stamp_bytes = static_cast<size_t>(nwg) * 16;
  if ((st = ensure(c, c->prog, prog_bytes + stamp_bytes))) return st;
  const uint32_t n_al = static_cast<uint32_t>(c->n / FILTER_ROWS * FILTER_ROWS);
  FilterRun run{c->stream, FILTER_F16, false, nq, QT, nq_pad, c->last_cap, static_cast<const float*>(inf.p)};
  // 0: the 4-wave build; 20: the 8-wave production build (two waves per SIMD, 32 queries each); tiles in identity order
  const auto kern = variant == 0 ? filter_f16_m16_kernel<768, 6, true, true> : filter_f16_m16_kernel<768, 4, true, true, 2, 2, 8>;
  const uint32_t waves = variant == 0 ? 4 : 8;
  ClockStats cs;
  st = clock_bursts(c, nwg, prog_bytes, seconds, [&] {
    return launch_filter_f16_kernel(c, run, {0, n_al}, kern, nwg, FilterGeom{64 * waves, filter_f16_m16_lds_bytes<768>(), waves, false}, &c->hitlog, 0,
                                    static_cast<uint32_t*>(c->prog.p), static_cast<uint32_t>(c->opt_sync_every - 1), static_cast<uint32_t>(c->opt_sync_lead));
  }, [] { return NVDB_OK; }, cs);
  (void)hipFree(inf.p);
  if (st) return st;
  out4[0] = cs.ms; out4[1] = cs.ghz[0]; out4[2] = cs.ghz[1]; out4[3] = cs.ghz[2];
  // how long the workgroups' tile loops ran: mean and max -- the launch ends with the slowest
  out4[4] = static_cast<float>(cs.sum_us / nwg);
  out4[5] = static_cast<float>(cs.max_us);
  // per XCD label (blockIdx % 8): mean duration, and the spread inside the label (max - min)
  for (uint32_t x = 0; x < 8; ++x) {
    double sx = 0.0, mn = 1e30, mxv = 0.0; uint32_t cnt = 0;
    for (uint32_t w = x; w < nwg; w += 8) { sx += cs.us[w]; mn = std::min(mn, cs.us[w]); mxv = std::max(mxv, cs.us[w]); ++cnt; }
    out4[6 + 2 * x] = cnt ? static_cast<float>(sx / cnt) : 0.f;
    out4[7 + 2 * x] = cnt ? static_cast<float>(mxv - mn) : 0.f;
  }
  return NVDB_OK;
}

nvdb_status nvdb_hip_debug_clock_i8(nvdb_hip_ctx* c, int variant, uint32_t nq, float seconds, float* out4) {
  if (!c || !out4) return NVDB_ERR_INVALID;
  // the stamped builds (the log sized for 8 waves per workgroup, as the product's launches)
  using Kern = decltype(&filter_i8w_kernel<768, 2, 6, true, 2, true>);
  Kern kern; uint32_t waves = 4; size_t lds;
  switch (variant) {
    case 0: kern = filter_i8w_kernel<768, 2, 6, true, 2, true>; lds = filter_i8w_lds_bytes<768, 2>(); break;
    case 10: kern = filter_i8p_kernel<768, true, true, 6, 4, true>; lds = filter_i8p_lds_bytes<768, 4, true>(); break;    // the software-pipelined build with the in-loop second stage
    case 20: kern = filter_i8p_kernel<768, true, true, 6, 4, false>; lds = filter_i8p_lds_bytes<768, 4, false>(); break;  // ... first-stage survivors logged, finished after the stream
    case 30: kern = filter_i8s_kernel<768, true, true, 6, 4>; lds = filter_i8s_lds_bytes<768, 4>(); break;                // the 16x16x64 build (kernels_filter_i8s.h)
    case 35: kern = filter_i8s_kernel<768, true, true, 6, 8>; lds = filter_i8s_lds_bytes<768, 8>(); waves = 8; break;     // ... on 8 waves
    default: return fail(c, NVDB_ERR_INVALID, "debug: unknown variant");
  }
  if (!c->rows || c->dtype != NVDB_DTYPE_I8 || c->dim != 768 || !c->q16.p || !c->opt_i8_wide) return fail(c, NVDB_ERR_UNSUPPORTED, "debug: run a path-2 search on an int8 d=768 corpus first");
  if (nq <= 128 || nq > (c->last_nq + 255u) / 256u * 256u) return fail(c, NVDB_ERR_UNSUPPORTED, "debug: 128 < nq <= the last search's padded batch");
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t QT = (nq + 255) / 256, nq_pad = QT * 256;
  const uint32_t nwg = filter_grid(c, QT);
  if (!xcd_aware_grid(QT, nwg)) return fail(c, NVDB_ERR_UNSUPPORTED, "debug: batch does not map onto the XCD-aware grid");
  // thresholds: the ones the last search ended with (realistic stage-1 / stage-2 rates for the production variant)
  const size_t prog_bytes = static_cast<size_t>(nwg) * 8 * 4, stamp_bytes = static_cast<size_t>(nwg) * 16;
  nvdb_status st;
  if ((st = ensure(c, c->prog, std::max(prog_bytes + stamp_bytes, static_cast<size_t>(PROG_SLOTS) * c->num_cu * 8 * 4)))) return st;
  const uint64_t n_dbg = c->dbg_rows > 0 ? std::min<uint64_t>(c->n, static_cast<uint64_t>(c->dbg_rows)) : c->n;
  const uint32_t n_al = static_cast<uint32_t>(n_dbg / I8W_TILE_ROWS * I8W_TILE_ROWS);
  FilterRun run{c->stream, FILTER_I8, c->last_perm /* ... and its tile order */, nq, QT, nq_pad, c->last_cap, static_cast<const float*>(c->thr.p)};
  const SyncArgs sy{static_cast<uint32_t*>(c->prog.p), static_cast<uint32_t>(c->opt_sync_every - 1), static_cast<uint32_t>(c->opt_sync_lead)};
  uint32_t* counts_dev = static_cast<uint32_t*>(c->misc.p) + 4;   // rare-path entries / lo-plane MFMA blocks: of the timed burst only
  ClockStats cs;
  st = clock_bursts(c, nwg, prog_bytes, seconds, [&] {
    return launch_filter_i8w_kernel(c, run, {0, n_al}, kern, nwg, FilterGeom{64 * waves, lds, 8, false}, static_cast<size_t>(nq_pad) * 768, I8W_TILE_ROWS, sy);
  }, [&]() -> nvdb_status { HIPCHK(c, hipMemsetAsync(counts_dev, 0, 8, c->stream)); return NVDB_OK; }, cs);
  if (st) return st;
  out4[0] = cs.ms; out4[1] = cs.ghz[0]; out4[2] = cs.ghz[1]; out4[3] = cs.ghz[2];
  uint32_t counts[2] = {0, 0};
  HIPCHK(c, hipMemcpy(counts, counts_dev, 8, hipMemcpyDeviceToHost));
  out4[4] = static_cast<float>(counts[0]) / CLOCK_BURST;
  out4[5] = static_cast<float>(counts[1]) / CLOCK_BURST;
  out4[6] = cs.stamped ? static_cast<float>(cs.sum_us / cs.stamped) : 0.f;   // the tile loop alone, per workgroup that stamped
  out4[7] = static_cast<float>(cs.max_us);
  return NVDB_OK;
}

// the device's own stream_tile_range for every stream of a launch, with the weights given (or the context's current ones)
__global__ void tile_ranges_kernel(uint32_t T, uint32_t S, const float* w, uint32_t* lo, uint32_t* hi) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) stream_tile_range(T, S, s, true, w, lo[s], hi[s]);
}

nvdb_status nvdb_hip_debug_tile_ranges(nvdb_hip_ctx* c, uint32_t n_tiles, uint32_t n_streams, const float* weights8, uint32_t* out_lo, uint32_t* out_hi,
                                       float* weights_out8) {
  if (!c || !n_streams || !out_lo || !out_hi) return c ? fail(c, NVDB_ERR_INVALID, "bad argument") : NVDB_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf buf;
  nvdb_status st;
  if ((st = ensure(c, buf, static_cast<size_t>(n_streams) * 8 + 32))) return st;
  uint32_t* lo = static_cast<uint32_t*>(buf.p);
  uint32_t* hi = lo + n_streams;
  float* w = reinterpret_cast<float*>(hi + n_streams);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (weights8) HIPCHK(c, hipMemcpy(w, weights8, 32, hipMemcpyHostToDevice));
  else HIPCHK(c, hipMemcpy(w, c->xcdw.p, 32, hipMemcpyDeviceToDevice));
  tile_ranges_kernel<<<(n_streams + 255) / 256, 256, 0, c->stream>>>(n_tiles, n_streams, w, lo, hi);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out_lo, lo, static_cast<size_t>(n_streams) * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(out_hi, hi, static_cast<size_t>(n_streams) * 4, hipMemcpyDeviceToHost));
  if (weights_out8) HIPCHK(c, hipMemcpy(weights_out8, w, 32, hipMemcpyDeviceToHost));
  HIPCHK(c, hipFree(buf.p));
  return NVDB_OK;
}

// plan_search on a detached context: nothing here touches a device
nvdb_status nvdb_hip_debug_plan(const nvdb_hip_plan_shape* shape, const nvdb_hip_plan_option* opts, uint32_t n_opts, uint32_t nq, uint32_t k,
                                int force_path, uint32_t cap_override, nvdb_hip_plan* out, char* err, size_t err_len) {
  if (!shape || !out || (n_opts && !opts) || !nq || !k || !shape->n) return NVDB_ERR_INVALID;
  static _Float16 shadow16;                        // (the plan only asks whether a shadow exists)
  static signed char shadow8;
  nvdb_hip_ctx c;
  c.n = shape->n; c.dim = shape->dim; c.fdim = shape->fdim; c.dtype = shape->dtype;
  c.owned = shape->owned != 0; c.q8shadow = shape->q8shadow != 0; c.i8_scales_signed = shape->i8_scales_signed != 0;
  if (shape->has_shadow16) c.shadow16 = &shadow16;
  if (shape->has_shadow8) c.shadow8 = &shadow8;
  c.num_cu = static_cast<int>(shape->num_cu); c.cap_hint = shape->cap_hint;
  c.shadow_demoted = shape->shadow_demoted != 0;
  auto failed = [&](nvdb_status st, const char* msg) { if (err && err_len) std::snprintf(err, err_len, "%s", msg); return st; };
  for (uint32_t i = 0; i < n_opts; ++i)
    if (nvdb_status st = nvdb_hip_set_option(&c, opts[i].key, opts[i].value)) return failed(st, c.err.c_str());
  // load_rule: the corpus got its int8 filter shadow by the rule a load applies (q8_shadow_wanted, the options above, free_hbm bytes free)
  if (shape->load_rule && q8_shadow_wanted(&c, shape->free_hbm)) { c.shadow8 = &shadow8; c.q8shadow = true; }
  SearchPlan p;
  if (nvdb_status st = plan_search(c, nq, k, force_path, cap_override, p)) return failed(st, p.error);
  *out = nvdb_hip_plan{};
  out->filter_shadow = p.filter && p.kind == FILTER_SHADOW8;
  out->route = p.route; out->prep = p.prep; out->prep_inits = p.prep_inits; out->k_wide = p.k_wide;
  out->k_eff = p.k_eff; out->cap = p.cap; out->QPB = p.QPB; out->QT = p.QT; out->nq_pad = p.nq_pad; out->prog_words = p.prog_words;
  out->head = p.head;
  out->stat_chunks = p.route == ROUTE_EXACT && p.head ? 2 : 1;
  out->stat_rows_scanned = c.n;
  if (p.route != ROUTE_FILTER) return NVDB_OK;
  out->padded = p.padded; out->perm_on = p.perm_on; out->boot = p.boot;
  out->tile_rows = p.tile_rows; out->n_al = p.n_al; out->growth = p.growth; out->boot_tiles = p.boot_tiles; out->boot_rows = p.boot_rows;
  out->r0 = p.r0; out->tail_exact = p.tail_exact;
  out->helper_tile_rows = filter_tile_rows(&c, p.kind, nq);
  out->stat_rows_scanned = p.tail_exact ? (c.n - p.n_al) * p.QT : 0;
  for (uint32_t r = p.r0; r < p.n_al; r = chunk_end(p, r)) {
    if (out->n_chunks == NVDB_PLAN_MAX_CHUNKS) return failed(NVDB_ERR_INTERNAL, "plan: more than NVDB_PLAN_MAX_CHUNKS chunks");
    out->chunk_lo[out->n_chunks] = r; out->chunk_hi[out->n_chunks++] = chunk_end(p, r);
    out->stat_rows_scanned += static_cast<uint64_t>(chunk_end(p, r) - r) * p.QT;
  }
  out->stat_chunks = out->n_chunks;
  return NVDB_OK;
}
}  // extern "C"
#endif  // NVDB_HIP_DEV
