// nvdb_ivf.cpp -- from a resident corpus to an IVF-Flat index: nvdb_hip_assign_rows (every row's best centroid),
// nvdb_hip_train_centroids (spherical k-means), nvdb_ivf_layout_host (the inverted lists of an assignment) and nvdb_hip_ivf_*
// (the corpus copied into list order, searched by nvdb_hip_search_ivf, answered in original ids)  (include/nvdb_hip.h).
//
// The assignment is the flat search turned round: the centroids are the f32 corpus of a child context (as nvdb_hip_set_centroids
// holds them), the resident rows are the queries.  rows_to_f32_kernel writes a batch of rows as f32 queries, the child's device
// API ranks it with k = 1 on the caller's stream, narrow_ids_kernel keeps the u32 part; a batch whose self-check trips goes
// through the child's host API, which retries by itself -- the device group's pattern (nvdb_group.cpp).
#include "nvdb_ctx.h"
#include "compact_plan.h"
#include "insert_plan.h"
#include "nvdb_insert.h"
#include "nvdb_parts.h"
#include "ivf_layout.h"
#include "row_mask.h"
#include "kernels_ivf.h"

namespace nvdbhip {
namespace {

constexpr uint32_t ASSIGN_BATCH = 1024;

std::string g_ivf_build_err;

struct DevMem {                                    // a device allocation that lives as long as its scope
  void* p = nullptr;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { if (p) (void)hipFree(p); }
  template <typename T> T* as() const { return static_cast<T*>(p); }
};
nvdb_status dev_alloc(nvdb_hip_ctx* c, DevMem& m, size_t bytes) {
  HIPCHK(c, hipMalloc(&m.p, std::max<size_t>(bytes, 256)));
  return NVDB_OK;
}

struct Coarse {                                    // the child context that holds the centroids
  nvdb_hip_ctx* ctx = nullptr;
  Coarse() = default;
  Coarse(const Coarse&) = delete;
  Coarse& operator=(const Coarse&) = delete;
  ~Coarse() { if (ctx) nvdb_hip_destroy(ctx); }
};
nvdb_status coarse_load(nvdb_hip_ctx* c, Coarse& co, const float* centroids, uint32_t nparts, const char* who) {
  nvdb_status st;
  if (!co.ctx && (st = nvdb_hip_create(c->device, &co.ctx))) return fail(c, st, std::string(who) + ": " + nvdb_hip_last_error(nullptr));
  if ((st = nvdb_hip_upload_corpus(co.ctx, centroids, nullptr, nparts, c->dim, NVDB_DTYPE_F32, 0)))
    return fail(c, st, std::string(who) + " (centroids): " + nvdb_hip_last_error(co.ctx));
  return NVDB_OK;
}

// elapsed time of a stretch of one stream, for the NVDB_IVF_DEBUG report
struct StreamTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t s = nullptr;
  explicit StreamTimer(bool on, hipStream_t stream) : s(stream) { if (on && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) e0 = nullptr; }
  StreamTimer(const StreamTimer&) = delete;
  StreamTimer& operator=(const StreamTimer&) = delete;
  ~StreamTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  void start() { if (e0) (void)hipEventRecord(e0, s); }
  float stop() {                                   // ms; synchronises on the stop event
    float ms = 0.f;
    if (e0 && hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess) (void)hipEventElapsedTime(&ms, e0, e1);
    return ms;
  }
};
bool ivf_debug() { return std::getenv("NVDB_IVF_DEBUG") != nullptr; }

// rows of the resident corpus: [row0, row0 + count), or dev_idx[0 .. count) (u32 row numbers in HBM); rows != nullptr: of these
// device rows (and scales) in the corpus' dtype and dim instead -- the staged rows of nvdb_hip_ivf_add_rows
struct RowSel { uint64_t row0; const uint32_t* dev_idx; uint64_t count; const void* rows = nullptr; const float* scales = nullptr; };

template <int DT>
nvdb_status launch_rows_to_f32_dt(nvdb_hip_ctx* c, hipStream_t s, const void* rows, const float* scales, uint64_t row0, const uint32_t* idx, uint32_t count, float* out) {
  const bool vec = c->dim % ivf_epv<DT>() == 0 && reinterpret_cast<uintptr_t>(rows) % 16 == 0;
  const size_t total = static_cast<size_t>(count) * (vec ? c->dim / ivf_epv<DT>() : c->dim);
  const unsigned grid = static_cast<unsigned>(std::min<size_t>((total + 255) / 256, 65536));
  if (vec) rows_to_f32_kernel<DT, true><<<grid, 256, 0, s>>>(rows, scales, c->dim, row0, idx, count, out);
  else rows_to_f32_kernel<DT, false><<<grid, 256, 0, s>>>(rows, scales, c->dim, row0, idx, count, out);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}
// rows [first, first + count) of the selection as f32 [count][dim] at `out`
nvdb_status launch_rows_to_f32(nvdb_hip_ctx* c, hipStream_t s, const RowSel& sel, uint64_t first, uint32_t count, float* out) {
  const uint32_t* idx = sel.dev_idx ? sel.dev_idx + first : nullptr;
  const uint64_t row0 = sel.row0 + first;
  const void* rows = sel.rows ? sel.rows : c->rows;
  const float* scales = sel.rows ? sel.scales : c->scales;
  if (c->dtype == NVDB_DTYPE_F32) return launch_rows_to_f32_dt<DT_F32>(c, s, rows, scales, row0, idx, count, out);
  if (c->dtype == NVDB_DTYPE_F16) return launch_rows_to_f32_dt<DT_F16>(c, s, rows, scales, row0, idx, count, out);
  return launch_rows_to_f32_dt<DT_I8>(c, s, rows, scales, row0, idx, count, out);
}

// out_assign[i] (host) = best centroid of row i of the selection; the centroids are resident in `child`
nvdb_status assign_core(nvdb_hip_ctx* c, nvdb_hip_ctx* child, uint32_t nparts, const RowSel& sel, uint32_t* out_assign, const char* who) {
  if (sel.count == 0) return NVDB_OK;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t qrow = static_cast<size_t>(c->dim) * 4;
  DevMem q, ids, sc, asg;
  nvdb_status st;
  if ((st = dev_alloc(c, q, (ASSIGN_BATCH + 8) * qrow))) return st;          // + the 8 zero rows the exact kernel reads after a batch
  if ((st = dev_alloc(c, ids, ASSIGN_BATCH * 8))) return st;
  if ((st = dev_alloc(c, sc, ASSIGN_BATCH * 4))) return st;
  if ((st = dev_alloc(c, asg, sel.count * 4))) return st;
  struct Redo { uint64_t first; std::vector<uint64_t> ids; };
  std::vector<Redo> redo;
  std::vector<float> hq, hsc;
  for (uint64_t first = 0; first < sel.count; first += ASSIGN_BATCH) {
    const uint32_t nb = static_cast<uint32_t>(std::min<uint64_t>(ASSIGN_BATCH, sel.count - first));
    if ((st = launch_rows_to_f32(c, s, sel, first, nb, q.as<float>()))) return st;
    HIPCHK(c, hipMemsetAsync(q.as<char>() + nb * qrow, 0, 8 * qrow, s));
    if ((st = nvdb_hip_search_batch_dev(child, q.as<float>(), nb, 1, ids.as<uint64_t>(), sc.as<float>(), s)))
      return fail(c, st, std::string(who) + " (assignment): " + nvdb_hip_last_error(child));
    narrow_ids_kernel<<<(nb + 255) / 256, 256, 0, s>>>(ids.as<unsigned long long>(), nb, nparts, asg.as<uint32_t>() + first);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    const nvdb_status chk = nvdb_hip_search_check(child, nullptr);
    if (chk == NVDB_OK) continue;
    if (chk != NVDB_ERR_INTERNAL) return fail(c, chk, std::string(who) + " (assignment): " + nvdb_hip_last_error(child));
    // the self-check tripped (list overflow, non-finite row): this batch again through the host API, which retries by itself
    hq.resize(static_cast<size_t>(nb) * c->dim);
    hsc.resize(nb);
    Redo r{first, std::vector<uint64_t>(nb)};
    HIPCHK(c, hipMemcpy(hq.data(), q.p, nb * qrow, hipMemcpyDeviceToHost));
    st = nvdb_hip_search_batch(child, hq.data(), nb, 1, r.ids.data(), hsc.data(), nullptr, nullptr);
    if (st && st != NVDB_ERR_INTERNAL)               // (NVDB_ERR_INTERNAL there: recomputed on the exact path, the results stand)
      return fail(c, st, std::string(who) + " (assignment, host retry): " + nvdb_hip_last_error(child));
    redo.push_back(std::move(r));
  }
  HIPCHK(c, hipMemcpy(out_assign, asg.p, sel.count * 4, hipMemcpyDeviceToHost));
  for (const Redo& r : redo)
    for (size_t i = 0; i < r.ids.size(); ++i) out_assign[r.first + i] = r.ids[i] < nparts ? static_cast<uint32_t>(r.ids[i]) : 0u;
  return NVDB_OK;
}

nvdb_status ivf_args(nvdb_hip_ctx* c, uint32_t nparts, const char* who) {
  if (!c) return NVDB_ERR_INVALID;
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (nparts == 0 || nparts == 0xFFFFFFFFu) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": nparts must be in [1, 2^32 - 2]");
  return NVDB_OK;
}

// the draw behind a NULL `init` (include/nvdb_hip.h states the rule): attempt t for centroid j
uint64_t train_draw(uint64_t seed, uint32_t j, uint32_t t, uint64_t m) {
  const uint32_t key = synth_row_key(seed, (static_cast<uint64_t>(t) << 32) | j);
  return ((static_cast<uint64_t>(mix32(key ^ 0x9E3779B9u)) << 32) | mix32(key + 0x85EBCA6Bu)) % m;
}

template <int DT>
nvdb_status launch_centroid_sum_dt(nvdb_hip_ctx* c, hipStream_t s, const uint32_t* members, const uint2* chunks, uint32_t nchunks, double* partial) {
  const bool vec = c->dim % 4 == 0 && reinterpret_cast<uintptr_t>(c->rows) % 16 == 0;
  if (vec) centroid_sum_kernel<DT, true><<<nchunks, 256, 0, s>>>(c->rows, c->scales, c->dim, members, chunks, partial);
  else centroid_sum_kernel<DT, false><<<nchunks, 256, 0, s>>>(c->rows, c->scales, c->dim, members, chunks, partial);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}
nvdb_status launch_centroid_sum(nvdb_hip_ctx* c, hipStream_t s, const uint32_t* members, const uint2* chunks, uint32_t nchunks, double* partial) {
  if (c->dtype == NVDB_DTYPE_F32) return launch_centroid_sum_dt<DT_F32>(c, s, members, chunks, nchunks, partial);
  if (c->dtype == NVDB_DTYPE_F16) return launch_centroid_sum_dt<DT_F16>(c, s, members, chunks, nchunks, partial);
  return launch_centroid_sum_dt<DT_I8>(c, s, members, chunks, nchunks, partial);
}

nvdb_status launch_gather_rows(nvdb_hip_ctx* c, hipStream_t s, const nvdb_hip_ctx* src, const uint32_t* perm, void* dst, float* dst_scales) {
  const size_t row_bytes = static_cast<size_t>(src->dim) * bpe_of(src->dtype);
  const bool vec = row_bytes % 16 == 0 && reinterpret_cast<uintptr_t>(src->rows) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
  const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((src->n + IVF_GATHER_ROWS - 1) / IVF_GATHER_ROWS, static_cast<uint64_t>(c->num_cu) * 32));
  if (vec) gather_rows_kernel<uint4><<<grid, 256, 0, s>>>(static_cast<const uint4*>(src->rows), src->scales, perm, src->n, static_cast<uint32_t>(row_bytes / 16),
                                                          static_cast<uint4*>(dst), dst_scales);
  else gather_rows_kernel<unsigned char><<<grid, 256, 0, s>>>(static_cast<const unsigned char*>(src->rows), src->scales, perm, src->n, static_cast<uint32_t>(row_bytes),
                                                              static_cast<unsigned char*>(dst), dst_scales);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

}  // namespace
}  // namespace nvdbhip

struct nvdb_hip_ivf {
  nvdb_hip_ctx* ctx = nullptr;                     // the list-ordered copy with its partition table and centroids; row_base 0
  std::vector<uint32_t> perm;                      // perm[position] = row of the source corpus
  std::vector<uint32_t> inv;                       // inv[row of the source corpus] = position; built by the first nvdb_hip_ivf_update_row_mask
  std::vector<uint64_t> offsets;                   // nparts + 1
  uint64_t src_row_base = 0;
  uint64_t src_n = 0;                              // rows of the source corpus (perm.size() until nvdb_hip_ivf_compact removes rows)
  std::string err;
};

namespace {

// positions in the list-ordered copy -> ids of the source corpus, in place; what is no position ("no entry", ~0) stays.  The
// order stays: equal scores stand by (list, original row)
void ivf_map_ids(const nvdb_hip_ivf* ix, uint64_t* ids, uint64_t count) {
  const uint32_t* perm = ix->perm.data();
  const uint64_t n = ix->perm.size();
  for (uint64_t i = 0; i < count; ++i)
    if (ids[i] < n) ids[i] = ix->src_row_base + perm[ids[i]];
}

// a call forwarded to the index's context: its status, and on failure its error text
nvdb_status ivf_forward(nvdb_hip_ivf* ix, nvdb_status st) {
  if (st) ix->err = nvdb_hip_last_error(ix->ctx);
  return st;
}

}  // namespace

extern "C" {

nvdb_status nvdb_ivf_layout_host(const uint32_t* assign, uint64_t n, uint32_t nparts, uint64_t* out_offsets, uint32_t* out_perm) {
  return ivf_layout(assign, n, nparts, out_offsets, out_perm) ? NVDB_OK : NVDB_ERR_INVALID;
}

nvdb_status nvdb_hip_assign_rows(nvdb_hip_ctx* c, const float* centroids, uint32_t nparts, uint64_t row0, uint64_t nrows, uint32_t* out_assign) {
  nvdb_status st = ivf_args(c, nparts, "assign_rows");
  if (st) return st;
  if (!centroids) return fail(c, NVDB_ERR_INVALID, "assign_rows: null centroids");
  if (row0 > c->n || nrows > c->n - row0) return fail(c, NVDB_ERR_INVALID, "assign_rows: row range out of bounds");
  if (nrows == 0) return NVDB_OK;
  if (!out_assign) return fail(c, NVDB_ERR_INVALID, "assign_rows: null output");
  Coarse co;
  if ((st = coarse_load(c, co, centroids, nparts, "assign_rows"))) return st;
  return assign_core(c, co.ctx, nparts, RowSel{row0, nullptr, nrows}, out_assign, "assign_rows");
}

nvdb_status nvdb_hip_train_centroids(nvdb_hip_ctx* c, uint32_t nparts, uint32_t iters, uint64_t seed, uint64_t max_train_rows,
                                     const float* init, float* out_centroids) {
  nvdb_status st = ivf_args(c, nparts, "train_centroids");
  if (st) return st;
  if (!out_centroids) return fail(c, NVDB_ERR_INVALID, "train_centroids: null output");
  const uint64_t n = c->n, m = (max_train_rows == 0 || max_train_rows >= n) ? n : max_train_rows;
  if (nparts > m) return fail(c, NVDB_ERR_INVALID, "train_centroids: more centroids than training rows");
  if (m > IVF_MAX_ROWS) return fail(c, NVDB_ERR_UNSUPPORTED, "train_centroids: training set too large (max_train_rows)");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const uint32_t dim = c->dim;
  const size_t cen_count = static_cast<size_t>(nparts) * dim;

  // the training set: every row, or rows floor(i * n / m) (n < 2^32, m < 2^32: the product fits)
  std::vector<uint32_t> train_rows;
  DevMem d_train;
  if (m < n) {
    train_rows.resize(m);
    for (uint64_t i = 0; i < m; ++i) train_rows[i] = static_cast<uint32_t>(i * n / m);
    if ((st = dev_alloc(c, d_train, m * 4))) return st;
    HIPCHK(c, hipMemcpy(d_train.p, train_rows.data(), m * 4, hipMemcpyHostToDevice));
  }
  const RowSel train{0, m < n ? d_train.as<uint32_t>() : nullptr, m};
  auto corpus_row = [&](uint64_t t) { return m < n ? train_rows[t] : static_cast<uint32_t>(t); };

  std::vector<float> cen(cen_count);
  DevMem d_cen;
  if ((st = dev_alloc(c, d_cen, cen_count * 4))) return st;
  if (init) std::memcpy(cen.data(), init, cen_count * 4);
  else {
    // nparts distinct training rows (train_draw; a row already taken is drawn again, after 64 attempts the next free one is taken)
    std::vector<bool> taken(m, false);
    std::vector<uint32_t> pick(nparts);
    for (uint32_t j = 0; j < nparts; ++j) {
      uint64_t t = train_draw(seed, j, 0, m);
      for (uint32_t a = 1; taken[t] && a < 64; ++a) t = train_draw(seed, j, a, m);
      while (taken[t]) t = t + 1 < m ? t + 1 : 0;
      taken[t] = true;
      pick[j] = corpus_row(t);
    }
    DevMem d_pick;
    if ((st = dev_alloc(c, d_pick, static_cast<size_t>(nparts) * 4))) return st;
    HIPCHK(c, hipMemcpyAsync(d_pick.p, pick.data(), static_cast<size_t>(nparts) * 4, hipMemcpyHostToDevice, s));
    if ((st = launch_rows_to_f32(c, s, RowSel{0, d_pick.as<uint32_t>(), nparts}, 0, nparts, d_cen.as<float>()))) return st;
    HIPCHK(c, hipMemcpyAsync(cen.data(), d_cen.p, cen_count * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (uint32_t j = 0; j < nparts; ++j) {       // unit length, in fp64, one rounding to f32 (an all-zero row stays as it is)
      float* v = cen.data() + static_cast<size_t>(j) * dim;
      double ss = 0.0;
      for (uint32_t k = 0; k < dim; ++k) ss += static_cast<double>(v[k]) * v[k];
      const double norm = std::sqrt(ss);
      if (!(norm > 0.0) || !std::isfinite(norm)) continue;
      for (uint32_t k = 0; k < dim; ++k) v[k] = static_cast<float>(static_cast<double>(v[k]) / norm);
    }
  }

  if (iters) {
    Coarse co;
    std::vector<uint32_t> assign(m), perm(m), members, chunk_first(static_cast<size_t>(nparts) + 1);
    std::vector<uint64_t> offsets(static_cast<size_t>(nparts) + 1);
    std::vector<uint2> chunks;
    const size_t max_chunks = m / IVF_SUM_CHUNK_ROWS + nparts;
    DevMem d_members, d_chunks, d_first, d_partial;
    if ((st = dev_alloc(c, d_members, m * 4))) return st;
    if ((st = dev_alloc(c, d_chunks, max_chunks * sizeof(uint2)))) return st;
    if ((st = dev_alloc(c, d_first, chunk_first.size() * 4))) return st;
    if ((st = dev_alloc(c, d_partial, max_chunks * dim * sizeof(double)))) return st;
    const bool dbg = ivf_debug();
    StreamTimer t_assign(dbg, s), t_update(dbg, s);
    float ms_assign = 0.f, ms_update = 0.f;
    for (uint32_t it = 0; it < iters; ++it) {
      if ((st = coarse_load(c, co, cen.data(), nparts, "train_centroids"))) return st;
      t_assign.start();
      if ((st = assign_core(c, co.ctx, nparts, train, assign.data(), "train_centroids"))) return st;
      ms_assign += t_assign.stop();
      if (!ivf_layout(assign.data(), m, nparts, offsets.data(), perm.data())) return fail(c, NVDB_ERR_INTERNAL, "train_centroids: assignment out of range");
      const uint32_t* mem = perm.data();
      if (m < n) {
        members.resize(m);
        for (uint64_t j = 0; j < m; ++j) members[j] = train_rows[perm[j]];
        mem = members.data();
      }
      chunks.clear();
      for (uint32_t p = 0; p < nparts; ++p) {
        chunk_first[p] = static_cast<uint32_t>(chunks.size());
        for (uint64_t b = offsets[p]; b < offsets[p + 1]; b += IVF_SUM_CHUNK_ROWS)
          chunks.push_back(make_uint2(static_cast<uint32_t>(b), static_cast<uint32_t>(std::min<uint64_t>(b + IVF_SUM_CHUNK_ROWS, offsets[p + 1]))));
      }
      chunk_first[nparts] = static_cast<uint32_t>(chunks.size());
      HIPCHK(c, hipMemcpyAsync(d_members.p, mem, m * 4, hipMemcpyHostToDevice, s));
      HIPCHK(c, hipMemcpyAsync(d_chunks.p, chunks.data(), chunks.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
      HIPCHK(c, hipMemcpyAsync(d_first.p, chunk_first.data(), chunk_first.size() * 4, hipMemcpyHostToDevice, s));
      HIPCHK(c, hipMemcpyAsync(d_cen.p, cen.data(), cen_count * 4, hipMemcpyHostToDevice, s));
      t_update.start();
      if ((st = launch_centroid_sum(c, s, d_members.as<uint32_t>(), d_chunks.as<uint2>(), static_cast<uint32_t>(chunks.size()), d_partial.as<double>()))) return st;
      centroid_finish_kernel<<<nparts, 256, 0, s>>>(d_partial.as<double>(), d_first.as<uint32_t>(), dim, d_cen.as<float>());
      HIPCHK(c, hipGetLastError());
      ms_update += t_update.stop();
      HIPCHK(c, hipMemcpyAsync(cen.data(), d_cen.p, cen_count * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipStreamSynchronize(s));
    }
    if (dbg) std::fprintf(stderr, "[nvdb ivf] train: %u iterations over %llu rows, %u centroids: assignment %.1f ms, member sums + normalisation %.2f ms (hipEvents)\n",
                          iters, static_cast<unsigned long long>(m), nparts, ms_assign, ms_update);
  }
  std::memcpy(out_centroids, cen.data(), cen_count * 4);
  return NVDB_OK;
}

nvdb_status nvdb_hip_ivf_build(nvdb_hip_ctx* src, const float* centroids, uint32_t nparts, nvdb_hip_ivf** out) {
  if (!out) return NVDB_ERR_INVALID;
  *out = nullptr;
  if (!src) { g_ivf_build_err = "ivf_build: null source context"; return NVDB_ERR_INVALID; }
  auto src_fail = [&](nvdb_status st) { g_ivf_build_err = src->err; return st; };
  nvdb_status st = ivf_args(src, nparts, "ivf_build");
  if (st) return src_fail(st);
  if (!centroids) return src_fail(fail(src, NVDB_ERR_INVALID, "ivf_build: null centroids"));
  if (src->n > IVF_MAX_ROWS) return src_fail(fail(src, NVDB_ERR_UNSUPPORTED, "ivf_build: corpus shard too large"));
  const uint64_t n = src->n;
  const bool dbg = ivf_debug();

  // 1. + 2. every row's centroid, the lists
  auto ix = new nvdb_hip_ivf();
  auto bail = [&](nvdb_status s_, const std::string& msg) { g_ivf_build_err = msg; nvdb_hip_ivf_destroy(ix); return s_; };
  std::vector<uint32_t> assign(n);
  float ms_assign = 0.f, ms_gather = 0.f;
  {
    Coarse co;
    if ((st = coarse_load(src, co, centroids, nparts, "ivf_build"))) return bail(st, src->err);
    StreamTimer t(dbg, src->stream);
    t.start();
    if ((st = assign_core(src, co.ctx, nparts, RowSel{0, nullptr, n}, assign.data(), "ivf_build"))) return bail(st, src->err);
    ms_assign = t.stop();
  }
  ix->perm.resize(n);
  ix->offsets.resize(static_cast<size_t>(nparts) + 1);
  ix->src_row_base = src->row_base;
  ix->src_n = n;
  if (!ivf_layout(assign.data(), n, nparts, ix->offsets.data(), ix->perm.data())) return bail(NVDB_ERR_INTERNAL, "ivf_build: assignment out of range");

  // 3. - 5. the list-ordered copy, owned by a fresh context on the same device
  if ((st = nvdb_hip_create(src->device, &ix->ctx))) return bail(st, std::string("ivf_build: ") + nvdb_hip_last_error(nullptr));
  nvdb_hip_ctx* c = ix->ctx;
  auto ctx_fail = [&](nvdb_status s_) { return bail(s_, "ivf_build: " + c->err); };
  c->opt_f32_shadow = src->opt_f32_shadow;          // (options that act when a corpus becomes resident)
  c->opt_shadow_common_scale = src->opt_shadow_common_scale;
  c->opt_q8_shadow = src->opt_q8_shadow > 0 ? 1 : 0;   // (the explicit option only: the automatic shadow serves the flat route, which an index's context does not run)
  void* rows = nullptr;
  float* scales = nullptr;
  {
    DevMem d_perm;
    if ((st = dev_alloc(c, d_perm, n * 4))) return ctx_fail(st);
    if ((st = corpus_alloc_padded(c, n, src->dim, src->dtype, &rows, &scales))) return ctx_fail(st);
    auto gather = [&]() -> nvdb_status {
      HIPCHK(c, hipStreamSynchronize(src->stream));
      HIPCHK(c, hipMemcpyAsync(d_perm.p, ix->perm.data(), n * 4, hipMemcpyHostToDevice, c->stream));
      StreamTimer t(dbg, c->stream);
      t.start();
      if (nvdb_status g = launch_gather_rows(c, c->stream, src, d_perm.as<uint32_t>(), rows, scales)) return g;
      ms_gather = t.stop();
      HIPCHK(c, hipStreamSynchronize(c->stream));
      return NVDB_OK;
    };
    if ((st = gather())) { (void)hipFree(rows); if (scales) (void)hipFree(scales); return ctx_fail(st); }
  }
  if ((st = corpus_take_ownership(c, rows, scales, n, src->dim, src->dtype, 0))) return ctx_fail(st);
  // 6. the partition table and the coarse quantiser
  if ((st = nvdb_hip_set_partitions(c, ix->offsets.data(), nparts))) return ctx_fail(st);
  if ((st = nvdb_hip_set_centroids(c, centroids))) return ctx_fail(st);
  if (dbg) {
    const double bytes = 2.0 * static_cast<double>(n) * src->dim * bpe_of(src->dtype);
    std::fprintf(stderr, "[nvdb ivf] build: %llu rows, %u lists: assignment %.1f ms, gather %.3f ms (%.2f TB/s read + written) (hipEvents)\n",
                 static_cast<unsigned long long>(n), nparts, ms_assign, ms_gather, ms_gather > 0.f ? bytes / (ms_gather * 1e9) : 0.0);
  }
  *out = ix;
  return NVDB_OK;
}

void nvdb_hip_ivf_destroy(nvdb_hip_ivf* ix) {
  if (!ix) return;
  if (ix->ctx) nvdb_hip_destroy(ix->ctx);
  delete ix;
}

const char* nvdb_hip_ivf_last_error(const nvdb_hip_ivf* ix) { return ix ? ix->err.c_str() : g_ivf_build_err.c_str(); }

nvdb_hip_ctx* nvdb_hip_ivf_ctx(nvdb_hip_ivf* ix) { return ix ? ix->ctx : nullptr; }

nvdb_status nvdb_hip_ivf_info(const nvdb_hip_ivf* ix, uint64_t* n, uint32_t* nparts, uint64_t* offsets_out, uint32_t* perm_out) {
  if (!ix) return NVDB_ERR_INVALID;
  if (n) *n = ix->perm.size();
  if (nparts) *nparts = static_cast<uint32_t>(ix->offsets.size() - 1);
  if (offsets_out) std::memcpy(offsets_out, ix->offsets.data(), ix->offsets.size() * sizeof(uint64_t));
  if (perm_out && !ix->perm.empty()) std::memcpy(perm_out, ix->perm.data(), ix->perm.size() * sizeof(uint32_t));
  return NVDB_OK;
}

nvdb_status nvdb_hip_ivf_search(nvdb_hip_ivf* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe, uint64_t* out_ids,
                                float* out_scores, uint32_t* out_counts, uint32_t* out_probe, nvdb_hip_timing* timing) {
  if (!ix) return NVDB_ERR_INVALID;
  if (nvdb_status st = ivf_forward(ix, nvdb_hip_search_ivf(ix->ctx, queries, nq, k, nprobe, out_ids, out_scores, out_counts, out_probe, timing))) return st;
  if (nq && k) ivf_map_ids(ix, out_ids, static_cast<uint64_t>(nq) * k);      // (nq == 0 || k == 0: nothing was written)
  return NVDB_OK;
}

nvdb_status nvdb_hip_ivf_set_row_masks(nvdb_hip_ivf* ix, const uint32_t* bits, uint32_t nmasks) {
  if (!ix) return NVDB_ERR_INVALID;
  nvdb_status st;
  if (!bits || nmasks == 0 || nmasks == 0xFFFFFFFFu) st = nvdb_hip_set_row_masks(ix->ctx, nullptr, nmasks);   // nothing to permute
  else {
    // position j of the index is live iff bit perm[j] of the caller's plane is set
    // (the caller's planes are over the source corpus' rows, the index's over the positions a compaction has left)
    const uint64_t n = ix->perm.size(), W = rm_words(n), Wsrc = rm_words(ix->src_n);
    std::vector<uint32_t> planes(static_cast<size_t>(nmasks) * W);
    for (uint32_t m = 0; m < nmasks; ++m) rm_permute(bits + static_cast<size_t>(m) * Wsrc, ix->perm.data(), n, planes.data() + static_cast<size_t>(m) * W);
    st = nvdb_hip_set_row_masks(ix->ctx, planes.data(), nmasks);
  }
  if (st) ix->err = nvdb_hip_last_error(ix->ctx);
  return st;
}

nvdb_status nvdb_hip_ivf_update_row_mask(nvdb_hip_ivf* ix, uint32_t mask, const uint64_t* rows, uint64_t nrows, int live) {
  if (!ix) return NVDB_ERR_INVALID;
  const uint64_t n = ix->src_n;                      // rows are named as the source corpus numbers them, before and after a compaction
  if (nrows && !rows) { ix->err = "ivf_update_row_mask: null row list"; return NVDB_ERR_INVALID; }
  if (!rm_rows_valid(rows, nrows, n)) { ix->err = "ivf_update_row_mask: a listed row is >= the row count"; return NVDB_ERR_INVALID; }
  if (ix->inv.empty() && nrows) {
    ix->inv.resize(n);
    if (!cp_inverse(ix->perm.data(), ix->perm.size(), n, ix->inv.data())) { ix->inv.clear(); ix->err = "ivf_update_row_mask: the index's permutation is damaged"; return NVDB_ERR_INTERNAL; }
  }
  std::vector<uint64_t> pos;
  pos.reserve(nrows);
  for (uint64_t i = 0; i < nrows; ++i)
    if (ix->inv[rows[i]] != 0xFFFFFFFFu) pos.push_back(ix->inv[rows[i]]);   // (a row that a compaction removed has no position: nothing to update)
  const nvdb_status st = nvdb_hip_update_row_mask(ix->ctx, mask, pos.data(), pos.size(), live);
  if (st) ix->err = nvdb_hip_last_error(ix->ctx);
  return st;
}

nvdb_status nvdb_hip_ivf_compact(nvdb_hip_ivf* ix, uint32_t mask, uint64_t* out_n) {
  if (!ix) return NVDB_ERR_INVALID;
  std::vector<uint32_t> old_rows(ix->perm.size());   // positions of the list-ordered copy: new position j was position old_rows[j]
  uint64_t n_new = 0;
  const nvdb_status st = nvdb_hip_compact_rows(ix->ctx, mask, &n_new, old_rows.data());
  if (st) {
    ix->err = nvdb_hip_last_error(ix->ctx);
    // A failure before the first row moved (an allocation of the workspace, say) has changed nothing: the index stays as it was.
    // Only where the context has DROPPED its corpus -- a HIP error during the move -- is this an index of no rows
    if (!ix->ctx->rows) {
      ix->perm.clear(); ix->inv.clear();
      std::fill(ix->offsets.begin(), ix->offsets.end(), 0);
    }
    return st;
  }
  if (n_new == ix->perm.size()) {                    // no row was dead: nothing moved, perm, offsets and inv stand
    if (out_n) *out_n = n_new;
    return NVDB_OK;
  }
  // lists shrink in place and stay contiguous: the entries of the map below an old offset are the live positions before that list
  cp_offsets_from_map(old_rows.data(), n_new, ix->offsets.data(), ix->offsets.size(), ix->offsets.data());
  cp_perm(ix->perm.data(), old_rows.data(), n_new);
  ix->perm.resize(n_new);
  ix->inv.clear();                                   // rebuilt by the next nvdb_hip_ivf_update_row_mask
  if (out_n) *out_n = n_new;
  return NVDB_OK;
}

nvdb_status nvdb_hip_ivf_add_rows(nvdb_hip_ivf* ix, const void* rows, const float* scales, uint64_t m, uint64_t* out_first_id, uint32_t* out_assign) {
  if (!ix) return NVDB_ERR_INVALID;
  nvdb_hip_ctx* c = ix->ctx;
  auto ctx_fail = [&](nvdb_status st) {
    ix->err = c->err;
    if (!c->rows) {                                  // the context dropped its corpus (a HIP error during the move): an index of no rows
      ix->perm.clear(); ix->inv.clear();
      std::fill(ix->offsets.begin(), ix->offsets.end(), 0);
    }
    return st;
  };
  if (m > IVF_MAX_ROWS || ix->src_n + m > IVF_MAX_ROWS) { ix->err = "ivf_add_rows: too many rows for one index"; return NVDB_ERR_UNSUPPORTED; }
  InsertStage stage;
  bool done = false;
  nvdb_status st = insert_stage(c, "ivf_add_rows", rows, scales, m, true, nullptr, stage, &done);
  if (st) return ctx_fail(st);
  if (done) {                                        // m == 0
    if (out_first_id) *out_first_id = ix->src_n;
    return NVDB_OK;
  }
  // every new row's list: nvdb_hip_assign_rows' rule, over the staged rows, against the index's own centroids
  PartState* ps = c->parts;
  if (!ps || !ps->have_centroids || !ps->coarse) return ctx_fail(fail(c, NVDB_ERR_INVALID, "ivf_add_rows: the index has no centroids"));
  const uint32_t nparts = static_cast<uint32_t>(ix->offsets.size() - 1);
  std::vector<uint32_t> assign(m);
  if ((st = assign_core(c, ps->coarse, nparts, RowSel{0, nullptr, m, stage.rows, stage.scales}, assign.data(), "ivf_add_rows"))) return ctx_fail(st);
  InsPlan pl;                                        // (the context's table is the index's: the plan of the move is the plan of perm)
  std::vector<uint64_t> new_rows(m);
  if ((st = insert_staged(c, "ivf_add_rows", stage, m, assign.data(), new_rows.data(), nullptr, &pl))) return ctx_fail(st);
  // the new rows carry the largest original ids: "ordered by partition, then original row" still holds
  ins_perm(ix->perm, ix->inv, pl, new_rows.data(), ix->src_n);
  ix->offsets = pl.off_new;
  if (out_first_id) *out_first_id = ix->src_n;
  if (out_assign) std::copy(assign.begin(), assign.end(), out_assign);
  ix->src_n += m;
  return NVDB_OK;
}

nvdb_status nvdb_hip_ivf_search_masked(nvdb_hip_ivf* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe, const uint32_t* mask_of,
                                       uint64_t* out_ids, float* out_scores, uint32_t* out_counts, uint32_t* out_probe, nvdb_hip_timing* timing) {
  if (!ix) return NVDB_ERR_INVALID;
  if (nvdb_status st = ivf_forward(ix, nvdb_hip_search_ivf_masked(ix->ctx, queries, nq, k, nprobe, mask_of, out_ids, out_scores, out_counts, out_probe, timing))) return st;
  if (nq && k) ivf_map_ids(ix, out_ids, static_cast<uint64_t>(nq) * k);
  return NVDB_OK;
}

nvdb_status nvdb_hip_ivf_search_anyk(nvdb_hip_ivf* ix, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe, const uint32_t* mask_of, int masked,
                                     uint64_t* out_ids, float* out_scores, uint32_t* out_counts, uint32_t* out_probe, nvdb_hip_timing* timing) {
  if (!ix) return NVDB_ERR_INVALID;
  if (nvdb_status st = ivf_forward(ix, nvdb_hip_search_ivf_anyk(ix->ctx, queries, nq, k, nprobe, mask_of, masked, out_ids, out_scores, out_counts, out_probe, timing))) return st;
  if (nq && k) ivf_map_ids(ix, out_ids, static_cast<uint64_t>(nq) * k);      // (the select's keys carry positions in the list-ordered copy)
  return NVDB_OK;
}

nvdb_status nvdb_hip_ivf_range_search(nvdb_hip_ivf* ix, const float* queries, uint32_t nq, const float* radius, uint32_t nprobe, const uint32_t* mask_of, int masked,
                                      uint64_t* out_lims, uint32_t* out_probe, nvdb_hip_timing* timing) {
  if (!ix) return NVDB_ERR_INVALID;
  return ivf_forward(ix, nvdb_hip_range_search_ivf(ix->ctx, queries, nq, radius, nprobe, mask_of, masked, out_lims, out_probe, timing));
}

nvdb_status nvdb_hip_ivf_range_results(nvdb_hip_ivf* ix, uint64_t* out_ids, float* out_scores) {
  if (!ix) return NVDB_ERR_INVALID;
  if (nvdb_status st = ivf_forward(ix, nvdb_hip_range_results(ix->ctx, out_ids, out_scores))) return st;
  ivf_map_ids(ix, out_ids, ix->ctx->range_total);
  return NVDB_OK;
}

}  // extern "C"
