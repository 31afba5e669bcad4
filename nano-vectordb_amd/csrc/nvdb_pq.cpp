// nvdb_pq.cpp -- the PQ candidate scan (DESIGN.md section 4 "PQ candidate scan"): the step the exact-L2 refine follows.  A context
// holds a PQ SHADOW of its resident corpus -- M byte codes per row under the caller's codebooks (nvdb_hip_pq_build: pq_encode_kernel)
// -- and answers a probe search from the codes alone: per sub-batch of queries
//   pass          parts_pass (nvdb_parts.h) with uncapped slots and groups of G = pq_group(M) queries (every item is class 0);
//                 between list and image: the any-k plan (pa_sub_plan), the tables' buffer grown
//   tables        pq_lut_kernel: L[b][M][256] from the sub-batch's queries on the device (ps->q)
//   scan          pq_scan_kernel<G, W16>: one launch over the work items; every row of a segment -> Cand{score, row} at its place in the slab
//   select        pa_sub_select: the any-k path's select, long slabs and emit, unchanged, with k = R
//   copy          the R candidates of every query into the caller's arrays (pa_sub_finish) -- or, fused (nvdb_hip_pq_refine_ivf):
//                 pq_narrow_ids_kernel, the refine's device launcher on the same stream over ps->q, and only [b][K] results copied back
// Sub-batches: pa_cut (parts_anyk_plan.h) under largek_budget_mb, and at most a quarter of that budget in tables.
// Whatever makes rows resident or moves them frees the shadow (pq_drop); the PQ calls then return NVDB_ERR_INVALID.
// The codebooks are the caller's or nvdb_hip_pq_train's (kernels_pq_train.h): the training rows gathered once as f32, the start
// filled on the device, then per iteration pq_train_step_kernel (assignment by the encode's rule and the members' fp64 sums, fused)
// and pq_train_finish_kernel (the division) with no host step in between; rows, partial sums and codebooks live inside the call, and
// the context's shadow is not touched.  nvdb_hip_pq4_train (kernels_pq4_train.h) is the same call with 16 codewords: its own start,
// step and finish kernels behind the shared gather, residual and rotation stages.
// A RESIDUAL shadow (nvdb_hip_pq_build_residual; kernels_pq_resid.h) holds the codes of x - centroid of the row's list, with its own
// device copies of the table (u32) and the centroids, and a search adds two things: pstart of the pass's work list rides behind
// the any-k plan's words in the image, pq_base_kernel writes b(q, p) = q . c[p] per (probed partition, query) pair between tables
// and scan, and pq_scan_resid_kernel adds the pair's term at the sink.  The residual trainer swaps the gather for
// pq_resid_gather_kernel and shares everything behind it.  nvdb_hip_set_partitions / _set_centroids free such a shadow.
// A shadow under an OPQ ROTATION (nvdb_hip_pq_build_opq; kernels_pq_rotate.h) holds the codes of y = A e, e the row or its residual:
// the build rotates a slab of rows into f32 scratch memory (pq_rotate_kernel<DT, RESID>), runs the f32 non-residual encode over the
// slab and moves on; the trainer rotates its gathered sample the same way, in place slab by slab; a search rotates each sub-batch's
// queries (ps->q -> pq.qrot) in front of pq_lut_kernel and nowhere else -- the coarse step, the base terms and the refine keep the
// caller's queries --; reconstruction multiplies the codewords by A^T.  No rotation: none of these launches.
// A 4-BIT shadow (nvdb_hip_pq4_build; kernels_pq4.h) holds two codes to a byte under 16 codewords per sub-quantiser: PqState::nbits
// says which of the two sets of kernels (encode, tables, scan, reconstruct) every call above launches -- groups of pq4_group(M)
// queries, which fill the work list's classes 1 and 2 as well: the items of all three are contiguous in the image and one launch
// takes them --; the pass, the base terms, the rotation, the select and the refine do not know the width.
// Under the L2 METRIC (nvdb_hip_pq_set_metric(1); kernels_pq_l2.h) the shadow also holds h[r] = |xhat_r|^2 / 2 -- pq_norms_kernel
// straight from the codes, or, under a rotation, pq_rownorm_kernel over reconstruct_slab's rows slab by slab -- and a search
// launches the L2 builds of the scans (z = s - h at the sink), pq_qnorm_kernel beside the tables and pq_l2_emit_kernel behind the
// select (z -> fma(-2, z, |q|^2), padding +inf); the fused call only takes the order.  PqState::metric dies with the shadow.
// Entry points: nvdb_hip_pq_set_metric / _metric / _norms (nvdb_hip_ivf_pq_set_metric), nvdb_hip_pq_train / _build / _info / _download_codes / _search_partitions / _search_ivf / _refine_ivf,
// nvdb_hip_pq_build_residual / _train_residual / _reconstruct / _kind and nvdb_hip_pq_build_opq / _train_opq / _rotation /
// _rotated_rows / _rotate, nvdb_hip_pq4_build / _pq4_train / _pq_bits; the index forms (nvdb_hip_ivf_pq_*, nvdb_ivf.cpp) call them on the index's context and map the ids.
#include "nvdb_parts.h"
#include "kernels_pq.h"
#include "kernels_pq_resid.h"
#include "kernels_pq_train.h"
#include "kernels_pq_rotate.h"
#include "kernels_pq4.h"
#include "kernels_pq4_train.h"
#include "kernels_pq_l2.h"
#include "ivf_layout.h"

namespace nvdbhip {

void pq_drop(nvdb_hip_ctx* c) {
  PqState* pq = c->pq;
  if (!pq) return;
  if (pq->codebooks) (void)hipFree(pq->codebooks);
  if (pq->codes) (void)hipFree(pq->codes);
  if (pq->lut.p) (void)hipFree(pq->lut.p);
  if (pq->cent) (void)hipFree(pq->cent);
  if (pq->off) (void)hipFree(pq->off);
  if (pq->base.p) (void)hipFree(pq->base.p);
  if (pq->rot) (void)hipFree(pq->rot);
  if (pq->rot_t) (void)hipFree(pq->rot_t);
  if (pq->qrot.p) (void)hipFree(pq->qrot.p);
  if (pq->half_norm) (void)hipFree(pq->half_norm);
  if (pq->qq.p) (void)hipFree(pq->qq.p);
  delete pq;
  c->pq = nullptr;
}

void pq_drop_residual(nvdb_hip_ctx* c) {
  if (c->pq && c->pq->residual) pq_drop(c);
}

namespace {

constexpr uint32_t PARTS_STAT_PQ = 9;                                // nvdb_hip_scan_stats::path

// rows / scales / n: the context's corpus, or (residual == false only) a slab of rotated f32 rows; codes: where row 0 of them goes
template <int DT>
nvdb_status launch_encode(nvdb_hip_ctx* c, hipStream_t s, const PqState& pq, bool residual, const void* rows, const float* scales, uint64_t n, uint8_t* codes) {
  const dim3 grid(static_cast<unsigned>((n + PQ_ENC_THREADS - 1) / PQ_ENC_THREADS), pq.M / 4u);
  auto go = [&](auto kernel) {
    kernel<<<grid, PQ_ENC_THREADS, 0, s>>>(rows, scales, n, c->dim, pq.M, pq.dsub, pq.codebooks, codes);
  };
  auto go_resid = [&](auto kernel) {
    kernel<<<grid, PQ_ENC_THREADS, 0, s>>>(rows, scales, n, c->dim, pq.M, pq.dsub, pq.codebooks, pq.off, pq.nparts, pq.cent, codes);
  };
  const uint32_t dmax = pq_encode_bound(pq.dsub);
  if (residual) {
    switch (dmax) {
      case 4: go_resid(pq_resid_encode_kernel<DT, 4>); break;
      case 8: go_resid(pq_resid_encode_kernel<DT, 8>); break;
      case 16: go_resid(pq_resid_encode_kernel<DT, 16>); break;
      default: go_resid(pq_resid_encode_kernel<DT, 32>); break;
    }
  } else {
    switch (dmax) {
      case 4: go(pq_encode_kernel<DT, 4>); break;
      case 8: go(pq_encode_kernel<DT, 8>); break;
      case 16: go(pq_encode_kernel<DT, 16>); break;
      default: go(pq_encode_kernel<DT, 32>); break;
    }
  }
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

// ... and of a 4-bit shadow: one kernel for both kinds
template <int DT>
nvdb_status launch_encode4(nvdb_hip_ctx* c, hipStream_t s, const PqState& pq, bool residual, const void* rows, const float* scales, uint64_t n, uint8_t* codes) {
  const unsigned grid = static_cast<unsigned>((n + PQ_ENC_THREADS - 1) / PQ_ENC_THREADS);
  auto go = [&](auto kernel) {
    kernel<<<grid, PQ_ENC_THREADS, 0, s>>>(rows, scales, n, c->dim, pq.M, pq.dsub, pq.codebooks, pq.off, pq.nparts, pq.cent, codes);
  };
  auto with_kind = [&](auto dmax) {
    if (residual) go(pq4_encode_kernel<DT, decltype(dmax)::value, true>);
    else go(pq4_encode_kernel<DT, decltype(dmax)::value, false>);
  };
  switch (pq_encode_bound(pq.dsub)) {
    case 4: with_kind(std::integral_constant<int, 4>{}); break;
    case 8: with_kind(std::integral_constant<int, 8>{}); break;
    case 16: with_kind(std::integral_constant<int, 16>{}); break;
    default: with_kind(std::integral_constant<int, 32>{}); break;
  }
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

// Y[nrows][dim] = rows row0 .. row0 + nrows of `rows` (dtype DT; minus their lists' centroids where cent is given) times mat^T
template <int DT>
nvdb_status launch_rotate(nvdb_hip_ctx* c, hipStream_t s, const void* rows, const float* scales, uint64_t row0, uint32_t nrows, const float* mat,
                          const uint32_t* off, uint32_t nparts, const float* cent, float* Y) {
  const unsigned grid = static_cast<unsigned>(pq_rotate_grid(nrows, c->dim));
  if (cent) pq_rotate_kernel<DT, true><<<grid, PQ_ROT_THREADS, 0, s>>>(rows, scales, row0, nrows, c->dim, mat, off, nparts, cent, Y);
  else pq_rotate_kernel<DT, false><<<grid, PQ_ROT_THREADS, 0, s>>>(rows, scales, row0, nrows, c->dim, mat, nullptr, 0u, nullptr, Y);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

// f32 rows already on the device (queries, a gathered sample, codewords side by side)
nvdb_status launch_rotate_f32(nvdb_hip_ctx* c, hipStream_t s, const float* X, uint32_t nrows, const float* mat, float* Y) {
  return launch_rotate<DT_F32>(c, s, X, nullptr, 0, nrows, mat, nullptr, 0u, nullptr, Y);
}

// what the residual calls need of the context: a partition table and centroids; 0: fine
nvdb_status resid_args(nvdb_hip_ctx* c, const char* who) {
  if (nvdb_status st = parts_args(c, who)) return st;
  if (!c->parts->have_centroids || !c->parts->coarse) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": no centroids (nvdb_hip_set_centroids)");
  return NVDB_OK;
}

// the context's table as the u32 words the residual kernels search (n <= 0xFFFFFF00: nvdb_hip_set_partitions)
std::vector<uint32_t> resid_offsets(const nvdb_hip_ctx* c) {
  const std::vector<uint64_t>& off = c->parts->offsets;
  return std::vector<uint32_t>(off.begin(), off.end());
}

// ---- the trainer (nvdb_hip_pq_train): device memory that lives as long as the call
struct TrainMem {
  void* p = nullptr;
  TrainMem() = default;
  TrainMem(const TrainMem&) = delete;
  TrainMem& operator=(const TrainMem&) = delete;
  ~TrainMem() { if (p) (void)hipFree(p); }
  template <typename T> T* as() const { return static_cast<T*>(p); }
};
nvdb_status train_alloc(nvdb_hip_ctx* c, TrainMem& m, size_t bytes) {
  HIPCHK(c, hipMalloc(&m.p, std::max<size_t>(bytes, 256)));
  return NVDB_OK;
}

template <int DT>
nvdb_status launch_train_gather(nvdb_hip_ctx* c, hipStream_t s, const uint32_t* idx, uint64_t m, float* X) {
  const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((m * c->dim + 255) / 256, static_cast<uint64_t>(c->num_cu) * 64));
  pq_train_gather_kernel<DT><<<grid, 256, 0, s>>>(c->rows, c->scales, c->dim, idx, m, X);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

// ... and the residual trainer's: off / cent on the device, a wave per training row
template <int DT>
nvdb_status launch_resid_gather(nvdb_hip_ctx* c, hipStream_t s, const uint32_t* idx, uint64_t m, const uint32_t* off, uint32_t nparts, const float* cent, float* X) {
  const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((m + 3) / 4, static_cast<uint64_t>(c->num_cu) * 64));
  pq_resid_gather_kernel<DT><<<grid, 256, 0, s>>>(c->rows, c->scales, c->dim, idx, m, off, nparts, cent, X);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

// one Lloyd iteration of every sub-quantiser: the fused assign-and-sum step, then the division.  err: this iteration's [M] distance sums
nvdb_status launch_train_iteration(nvdb_hip_ctx* c, hipStream_t s, const float* X, uint64_t m, uint32_t M, uint32_t dsub, float* cb, double* partial,
                                   uint32_t* count, double* dist, double* err) {
  const uint32_t chunks = static_cast<uint32_t>(pq_train_chunks(m)), dmax = pq_encode_bound(dsub);
  const size_t lds = pq_train_lds(dmax);
  auto go = [&](auto kernel) -> nvdb_status {
    if (lds > 64 * 1024)
      if (nvdb_status st = raise_lds_limit(c, reinterpret_cast<const void*>(kernel), lds)) return st;
    kernel<<<dim3(chunks, M), PQ_TRAIN_THREADS, lds, s>>>(X, m, c->dim, dsub, cb, partial, count, dist);
    HIPCHK(c, hipGetLastError());
    return NVDB_OK;
  };
  nvdb_status st;
  switch (dmax) {
    case 4: st = go(pq_train_step_kernel<4>); break;
    case 8: st = go(pq_train_step_kernel<8>); break;
    case 16: st = go(pq_train_step_kernel<16>); break;
    default: st = go(pq_train_step_kernel<32>); break;
  }
  if (st) return st;
  pq_train_finish_kernel<<<M, PQ_TRAIN_THREADS, 0, s>>>(partial, count, dist, chunks, dsub, cb, err);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

// ... of the 16-codeword trainer (nvdb_hip_pq4_train): a workgroup per (chunk, group of pq4_train_sq sub-quantisers)
nvdb_status launch_train4_iteration(nvdb_hip_ctx* c, hipStream_t s, const float* X, uint64_t m, uint32_t M, uint32_t dsub, float* cb, double* partial,
                                    uint32_t* count, double* dist, double* err) {
  const uint32_t chunks = static_cast<uint32_t>(pq_train_chunks(m)), dmax = pq_encode_bound(dsub);
  const size_t lds = pq4_train_lds(dmax);
  auto go = [&](auto kernel) -> nvdb_status {
    if (lds > 64 * 1024)
      if (nvdb_status st = raise_lds_limit(c, reinterpret_cast<const void*>(kernel), lds)) return st;
    kernel<<<dim3(chunks, M / pq4_train_sq(dmax)), PQ_TRAIN_THREADS, lds, s>>>(X, m, c->dim, M, dsub, cb, partial, count, dist);
    HIPCHK(c, hipGetLastError());
    return NVDB_OK;
  };
  nvdb_status st;
  switch (dmax) {
    case 4: st = go(pq4_train_step_kernel<4>); break;
    case 8: st = go(pq4_train_step_kernel<8>); break;
    case 16: st = go(pq4_train_step_kernel<16>); break;
    default: st = go(pq4_train_step_kernel<32>); break;
  }
  if (st) return st;
  pq4_train_finish_kernel<<<(M * PQ4_KSUB + 255u) / 256u, 256, 0, s>>>(partial, count, dist, chunks, M, dsub, cb, err);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

// the call proper, the arguments validated: cb (host, [M][256][dsub]; nbits 4: [M][16][dsub]) and err (host, [iters]) are this call's own and reach the caller on success only
// residual: the training rows are the residuals to the centroids of their lists (the caller has checked resid_args)
// rotation (host, [dim][dim], or nullptr): the gathered rows, residual or not, become A e before anything reads them
// nbits: 8, or 4 (nvdb_hip_pq4_train): the codewords per sub-quantiser, the pick, the partial sums and the iteration's kernels
nvdb_status pq_train(nvdb_hip_ctx* c, bool residual, const float* rotation, uint32_t M, uint32_t iters, uint64_t seed, uint64_t m, const float* init,
                     std::vector<float>& cb, std::vector<double>& err, uint32_t nbits) {
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const uint64_t n = c->n;
  const uint32_t dim = c->dim, dsub = dim / M, ksub = nbits == 4 ? PQ4_KSUB : PQ_KSUB;
  const size_t cb_bytes = cb.size() * 4;
  nvdb_status st = NVDB_OK;

  // the training set as f32 rows: every row, or rows floor(i * n / m) (n < 2^32, m < 2^32: the product fits)
  TrainMem d_idx, d_x, d_cb, d_off;
  if (m < n) {
    std::vector<uint32_t> idx(m);
    for (uint64_t i = 0; i < m; ++i) idx[i] = static_cast<uint32_t>(i * n / m);
    if ((st = train_alloc(c, d_idx, m * 4))) return st;
    HIPCHK(c, hipMemcpy(d_idx.p, idx.data(), m * 4, hipMemcpyHostToDevice));
  }
  if ((st = train_alloc(c, d_x, m * dim * 4)) || (st = train_alloc(c, d_cb, cb_bytes))) return st;
  if (residual) {
    // the centroids where set_centroids put them (the child context's f32 rows, this device), the table as u32 for the call
    const std::vector<uint32_t> off = resid_offsets(c);
    if ((st = train_alloc(c, d_off, off.size() * 4))) return st;
    HIPCHK(c, hipMemcpy(d_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    dispatch_dtype(c->dtype, st, [&](auto dt) {
      return launch_resid_gather<decltype(dt)::value>(c, s, d_idx.as<uint32_t>(), m, d_off.as<uint32_t>(), static_cast<uint32_t>(off.size() - 1),
                                                      static_cast<const float*>(c->parts->coarse->rows), d_x.as<float>());
    });
  } else {
    dispatch_dtype(c->dtype, st, [&](auto dt) { return launch_train_gather<decltype(dt)::value>(c, s, d_idx.as<uint32_t>(), m, d_x.as<float>()); });
  }
  if (st) return st;
  if (rotation) {
    // in place, slab by slab through scratch memory: the f32 build of the product, then the slab copied back over its rows
    const uint64_t slab = std::min<uint64_t>(m, pq_rotate_slab_rows(dim));
    TrainMem d_rot, d_y;
    if ((st = train_alloc(c, d_rot, static_cast<size_t>(dim) * dim * 4)) || (st = train_alloc(c, d_y, slab * dim * 4))) return st;
    HIPCHK(c, hipMemcpyAsync(d_rot.p, rotation, static_cast<size_t>(dim) * dim * 4, hipMemcpyHostToDevice, s));
    for (uint64_t r = 0; r < m && !st; r += slab) {
      const uint32_t nr = static_cast<uint32_t>(std::min<uint64_t>(slab, m - r));
      float* x = d_x.as<float>() + r * dim;
      if ((st = launch_rotate_f32(c, s, x, nr, d_rot.as<float>(), d_y.as<float>()))) break;
      if (hipMemcpyAsync(x, d_y.p, static_cast<size_t>(nr) * dim * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) st = fail(c, NVDB_ERR_HIP, "pq_train: copy of a rotated slab");
    }
    const hipError_t e = hipStreamSynchronize(s);                      // (before the matrix and the slab leave scope, whatever happened)
    if (!st && e != hipSuccess) st = fail(c, NVDB_ERR_HIP, std::string("pq_train: ") + hipGetErrorString(e));
    if (st) return st;
  }

  if (init) {
    HIPCHK(c, hipMemcpyAsync(d_cb.p, init, cb_bytes, hipMemcpyHostToDevice, s));
  } else {
    // per sub-quantiser 256 (16) distinct training rows, the centroid trainer's draw under the sub-quantiser's own seed
    std::vector<uint32_t> pick(static_cast<size_t>(M) * ksub);
    for (uint32_t mq = 0; mq < M; ++mq) train_pick(seed ^ (0x9E3779B97F4A7C15ull * (mq + 1)), ksub, m, pick.data() + static_cast<size_t>(mq) * ksub);
    TrainMem d_pick;
    if ((st = train_alloc(c, d_pick, pick.size() * 4))) return st;
    HIPCHK(c, hipMemcpyAsync(d_pick.p, pick.data(), pick.size() * 4, hipMemcpyHostToDevice, s));
    if (nbits == 4) pq4_train_start_kernel<<<(M * PQ4_KSUB + 255u) / 256u, 256, 0, s>>>(d_x.as<float>(), dim, M, dsub, d_pick.as<uint32_t>(), d_cb.as<float>());
    else pq_train_start_kernel<<<M, PQ_KSUB, 0, s>>>(d_x.as<float>(), dim, dsub, d_pick.as<uint32_t>(), d_cb.as<float>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));                                // (d_pick leaves scope)
  }

  std::vector<double> err_m(static_cast<size_t>(iters) * M);
  if (iters) {
    const uint64_t chunks = pq_train_chunks(m);
    TrainMem d_partial, d_count, d_dist, d_err;
    if ((st = train_alloc(c, d_partial, nbits == 4 ? pq4_train_partial_bytes(m, dim) : pq_train_partial_bytes(m, dim))) || (st = train_alloc(c, d_count, chunks * M * ksub * 4)) ||
        (st = train_alloc(c, d_dist, chunks * M * 8)) || (st = train_alloc(c, d_err, err_m.size() * 8)))
      return st;
    const auto iteration = nbits == 4 ? launch_train4_iteration : launch_train_iteration;
    for (uint32_t it = 0; it < iters; ++it)
      if ((st = iteration(c, s, d_x.as<float>(), m, M, dsub, d_cb.as<float>(), d_partial.as<double>(), d_count.as<uint32_t>(), d_dist.as<double>(),
                          d_err.as<double>() + static_cast<size_t>(it) * M)))
        break;
    if (!st) {
      HIPCHK(c, hipMemcpyAsync(err_m.data(), d_err.p, err_m.size() * 8, hipMemcpyDeviceToHost, s));
    }
    const hipError_t e = hipStreamSynchronize(s);                      // (before the partials leave scope, whatever happened)
    if (!st && e != hipSuccess) st = fail(c, NVDB_ERR_HIP, std::string("pq_train: ") + hipGetErrorString(e));
    if (st) return st;
  }
  HIPCHK(c, hipMemcpyAsync(cb.data(), d_cb.p, cb_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  // the mean winning distance per iteration: the sub-quantisers' sums added in ascending order, one division
  for (uint32_t it = 0; it < iters; ++it) {
    double e = 0.0;
    for (uint32_t mq = 0; mq < M; ++mq) e += err_m[static_cast<size_t>(it) * M + mq];
    err[it] = e / (static_cast<double>(m) * M);
  }
  return NVDB_OK;
}

// the scan's build for M: G tables in LDS, 16-byte or dword code loads
template <int G>
nvdb_status launch_scan_g(nvdb_hip_ctx* c, hipStream_t s, const PqState& pq, const PartImage& im, uint32_t nitems) {
  const size_t lds = G * pq_lut_bytes(pq.M);
  auto go = [&](auto kernel) -> nvdb_status {
    if (lds > 64 * 1024)
      if (nvdb_status st = raise_lds_limit(c, reinterpret_cast<const void*>(kernel), PART_LDS_LIMIT)) return st;
    kernel<<<nitems, PQ_SCAN_THREADS, lds, s>>>(pq.codes, pq.M, im.items, im.qidx, im.dst, static_cast<const float*>(pq.lut.p), static_cast<Cand*>(c->parts->cand.p));
    HIPCHK(c, hipGetLastError());
    return NVDB_OK;
  };
  auto go_resid = [&](auto kernel) -> nvdb_status {
    if (lds > 64 * 1024)
      if (nvdb_status st = raise_lds_limit(c, reinterpret_cast<const void*>(kernel), PART_LDS_LIMIT)) return st;
    kernel<<<nitems, PQ_SCAN_THREADS, lds, s>>>(pq.codes, pq.M, im.items, im.qidx, im.dst, static_cast<const float*>(pq.base.p),
                                                static_cast<const float*>(pq.lut.p), static_cast<Cand*>(c->parts->cand.p));
    HIPCHK(c, hipGetLastError());
    return NVDB_OK;
  };
  auto go_l2 = [&](auto kernel) -> nvdb_status {                       // the L2 builds: one signature for both kinds, h behind the tables
    if (lds > 64 * 1024)
      if (nvdb_status st = raise_lds_limit(c, reinterpret_cast<const void*>(kernel), PART_LDS_LIMIT)) return st;
    kernel<<<nitems, PQ_SCAN_THREADS, lds, s>>>(pq.codes, pq.M, im.items, im.qidx, im.dst, static_cast<const float*>(pq.base.p),
                                                static_cast<const float*>(pq.lut.p), pq.half_norm, static_cast<Cand*>(c->parts->cand.p));
    HIPCHK(c, hipGetLastError());
    return NVDB_OK;
  };
  if (pq.metric) {
    if (pq.residual) return pq_wide_codes(pq.M) ? go_l2(pq_scan_l2_kernel<G, true, true>) : go_l2(pq_scan_l2_kernel<G, false, true>);
    return pq_wide_codes(pq.M) ? go_l2(pq_scan_l2_kernel<G, true, false>) : go_l2(pq_scan_l2_kernel<G, false, false>);
  }
  if (pq.residual) return pq_wide_codes(pq.M) ? go_resid(pq_scan_resid_kernel<G, true>) : go_resid(pq_scan_resid_kernel<G, false>);
  return pq_wide_codes(pq.M) ? go(pq_scan_kernel<G, true>) : go(pq_scan_kernel<G, false>);
}

// the 4-bit scan's build for M: G interleaved tables in LDS; nitems: the items of every class (im.items: classes 2, 1, 0, contiguous)
template <int G>
nvdb_status launch_scan4_g(nvdb_hip_ctx* c, hipStream_t s, const PqState& pq, const PartImage& im, uint32_t nitems) {
  const size_t lds = pq4_scan_lds(pq.M, G);
  auto go = [&](auto kernel) -> nvdb_status {
    if (lds > 64 * 1024)
      if (nvdb_status st = raise_lds_limit(c, reinterpret_cast<const void*>(kernel), PART_LDS_LIMIT)) return st;
    kernel<<<nitems, PQ_SCAN_THREADS, lds, s>>>(pq.codes, pq.M, im.items, im.qidx, im.dst, static_cast<const float*>(pq.base.p),
                                                static_cast<const float*>(pq.lut.p), static_cast<Cand*>(c->parts->cand.p));
    HIPCHK(c, hipGetLastError());
    return NVDB_OK;
  };
  auto go_l2 = [&](auto kernel) -> nvdb_status {
    if (lds > 64 * 1024)
      if (nvdb_status st = raise_lds_limit(c, reinterpret_cast<const void*>(kernel), PART_LDS_LIMIT)) return st;
    kernel<<<nitems, PQ_SCAN_THREADS, lds, s>>>(pq.codes, pq.M, im.items, im.qidx, im.dst, static_cast<const float*>(pq.base.p),
                                                static_cast<const float*>(pq.lut.p), pq.half_norm, static_cast<Cand*>(c->parts->cand.p));
    HIPCHK(c, hipGetLastError());
    return NVDB_OK;
  };
  if (pq.metric) {
    if (pq.residual) return pq4_wide_codes(pq.M) ? go_l2(pq4_scan_l2_kernel<G, true, true>) : go_l2(pq4_scan_l2_kernel<G, false, true>);
    return pq4_wide_codes(pq.M) ? go_l2(pq4_scan_l2_kernel<G, true, false>) : go_l2(pq4_scan_l2_kernel<G, false, false>);
  }
  if (pq.residual) return pq4_wide_codes(pq.M) ? go(pq4_scan_kernel<G, true, true>) : go(pq4_scan_kernel<G, false, true>);
  return pq4_wide_codes(pq.M) ? go(pq4_scan_kernel<G, true, false>) : go(pq4_scan_kernel<G, false, false>);
}

nvdb_status launch_scan(nvdb_hip_ctx* c, hipStream_t s, const PqState& pq, const PartImage& im, uint32_t nitems) {
  if (pq.nbits == 4) {
    switch (pq4_group(pq.M)) {
      case 32: return launch_scan4_g<32>(c, s, pq, im, nitems);
      case 16: return launch_scan4_g<16>(c, s, pq, im, nitems);
      default: return launch_scan4_g<8>(c, s, pq, im, nitems);
    }
  }
  switch (pq_group(pq.M)) {
    case 8: return launch_scan_g<8>(c, s, pq, im, nitems);
    case 4: return launch_scan_g<4>(c, s, pq, im, nitems);
    case 2: return launch_scan_g<2>(c, s, pq, im, nitems);
    default: return launch_scan_g<1>(c, s, pq, im, nitems);
  }
}

// what a fused call adds to the search: K results per query by exact L2 over the R candidates (out_dist may be nullptr)
struct PqRefine { uint32_t K; uint64_t* out_ids; float* out_dist; };

// the search proper: the arguments are validated, nq > 0, R > 0 and nprobe > 0.  rf == nullptr: the R candidates go to out_ids /
// out_scores / out_counts; else they stay on the device and rf's arrays receive the refined results
nvdb_status pq_search(nvdb_hip_ctx* c, const char* who, const float* queries, uint32_t nq, uint32_t R, const uint32_t* probe, uint32_t nprobe,
                      uint64_t* out_ids, float* out_scores, uint32_t* out_counts, const PqRefine* rf, nvdb_hip_timing* timing) {
  PartState* ps = c->parts;
  PqState& pq = *c->pq;
  const uint64_t* off = ps->offsets.data();
  const uint32_t nparts = static_cast<uint32_t>(ps->offsets.size() - 1);
  const PartBuild pb = parts_build(c);                               // (the pass takes its group size from p.qg_max)
  nvdb_status st;
  std::vector<uint64_t> block(nq, 0);
  if ((st = parts_probes(c, who, off, nparts, nq, probe, nprobe, block.data()))) return st;

  if ((st = parts_call_begin(c, PARTS_STAT_PQ))) return st;
  hipStream_t s = c->stream;

  const uint64_t budget_bytes = static_cast<uint64_t>(c->opt_largek_budget_mb) << 20;
  const uint64_t budget_entries = budget_bytes / (2 * sizeof(Cand));
  const bool b4 = pq.nbits == 4;
  const bool l2_out = pq.metric != 0 && !rf;                           // the L2 metric with scores to report: |q|^2 and the emit (fused: z orders, no distance is formed)
  const float pos_inf = __builtin_huge_valf();
  const uint32_t group = b4 ? pq4_group(pq.M) : pq_group(pq.M);
  const size_t lut_bytes = b4 ? pq4_lut_bytes(pq.M) : pq_lut_bytes(pq.M);
  const uint32_t lut_batch = b4 ? pq4_lut_batch(pq.M, budget_bytes / 4) : pq_lut_batch(pq.M, budget_bytes / 4);
  PaSub sub;
  std::vector<uint32_t> h_rid;
  for (uint32_t q0 = 0; q0 < nq;) {
    const uint32_t q1 = pa_cut(block.data(), static_cast<uint32_t>(std::min<uint64_t>(nq, static_cast<uint64_t>(q0) + lut_batch)), q0, R, budget_entries);
    if (q1 == q0) return fail(c, NVDB_ERR_UNSUPPORTED, std::string(who) + ": one query's probed union holds 2^32 rows or more");
    const uint32_t b = q1 - q0;
    uint64_t* ids0 = rf ? nullptr : out_ids + static_cast<size_t>(q0) * R;
    float* sc0 = rf ? nullptr : out_scores + static_cast<size_t>(q0) * R;
    PartPass p;
    p.off = off; p.nparts = nparts; p.q0 = q0; p.b = b; p.nprobe = nprobe; p.slot_cap = 0xFFFFFFFFu;
    p.qg_max = group;
    p.queries = queries;
    p.skip_empty = true;
    size_t pstart_at = 0;                                              // residual: where pstart begins in the image's extra words
    st = parts_pass(c, s, who, pb, p, [&](PartPass& pp) -> nvdb_status {
      if (nvdb_status e = pa_sub_plan(c, who, block.data() + q0, b, R, sub, pp)) return e;
      if (pq.residual) {
        // behind the plan's words: pstart[nparts + 1] of this pass's counting sort -- which entries of qidx probe partition p
        pstart_at = sub.extra.size();
        sub.extra.insert(sub.extra.end(), ps->list.pstart.begin(), ps->list.pstart.end());
        pp.extra = sub.extra.data(); pp.extra_words = static_cast<uint32_t>(sub.extra.size());
        if (nvdb_status e = ensure(c, pq.base, static_cast<size_t>(pp.wl.npairs) * 4)) return e;
      }
      if (pq.rot)
        if (nvdb_status e = ensure(c, pq.qrot, static_cast<size_t>(b) * c->dim * 4)) return e;
      if (l2_out)
        if (nvdb_status e = ensure(c, pq.qq, static_cast<size_t>(b) * 4)) return e;
      return ensure(c, pq.lut, b * lut_bytes);
    });
    if (st) return st;
    if (!p.wl.total) {                                                 // no row in any union of the sub-batch
      if (rf) {
        std::fill(rf->out_ids + static_cast<size_t>(q0) * rf->K, rf->out_ids + static_cast<size_t>(q1) * rf->K, ~0ull);
        if (rf->out_dist) std::fill(rf->out_dist + static_cast<size_t>(q0) * rf->K, rf->out_dist + static_cast<size_t>(q1) * rf->K, 1e30f);
      } else {
        pad_rows(b, R, 0, ids0, sc0, out_counts ? out_counts + q0 : nullptr);
        if (l2_out) std::fill(sc0, sc0 + static_cast<size_t>(b) * R, pos_inf);
      }
      q0 = q1;
      continue;
    }
    // the tables' queries: the sub-batch's own, or -- a rotated shadow -- A q (the base terms and the refine below keep ps->q)
    const float* lut_q = static_cast<const float*>(ps->q.p);
    if (pq.rot) {
      if ((st = launch_rotate_f32(c, s, lut_q, b, pq.rot, static_cast<float*>(pq.qrot.p)))) return st;
      lut_q = static_cast<const float*>(pq.qrot.p);
    }
    if (b4) pq4_lut_kernel<<<dim3((pq.M + 15u) / 16u, b), 256, 0, s>>>(lut_q, c->dim, pq.M, pq.dsub, pq.codebooks, static_cast<float*>(pq.lut.p));
    else pq_lut_kernel<<<dim3(pq.M / 4u, b), 256, 0, s>>>(lut_q, c->dim, pq.M, pq.dsub, pq.codebooks, static_cast<float*>(pq.lut.p));
    HIPCHK(c, hipGetLastError());
    if (l2_out) {
      pq_qnorm_kernel<<<(b + 3u) / 4u, 256, 0, s>>>(static_cast<const float*>(ps->q.p), c->dim, b, static_cast<float*>(pq.qq.p));
      HIPCHK(c, hipGetLastError());
    }
    if (pq.residual) {
      pq_base_kernel<<<nparts, PQ_BASE_THREADS, 0, s>>>(static_cast<const float*>(ps->q.p), c->dim, pq.cent, p.im.extra + pstart_at, p.im.qidx,
                                                        static_cast<float*>(pq.base.p));
      HIPCHK(c, hipGetLastError());
    }
    if ((st = launch_scan(c, s, pq, p.im, static_cast<uint32_t>(p.wl.nitems)))) return st;
    c->stats.chunks += 1;
    if ((st = pa_sub_select(c, s, sub, p.im, b, R))) return st;
    if (l2_out) {                                                      // z -> distances where the select left them, padding -> +inf
      const uint64_t ne = static_cast<uint64_t>(b) * sub.plan.out_k;
      pq_l2_emit_kernel<<<static_cast<unsigned>((ne + 255) / 256), 256, 0, s>>>(static_cast<const unsigned long long*>(ps->out_ids.p),
                                                                               static_cast<float*>(ps->out_scores.p), ne, sub.plan.out_k,
                                                                               static_cast<const float*>(pq.qq.p));
      HIPCHK(c, hipGetLastError());
    }
    if (rf) {
      // the candidates stay on the device: [b][out_k] global ids -> u32 local rows -> the refine over this sub-batch's queries
      const uint32_t r_dev = sub.plan.out_k;
      const size_t nc = static_cast<size_t>(b) * r_dev, no = static_cast<size_t>(b) * rf->K;
      if ((st = ensure(c, c->rcand, nc * 4)) || (st = ensure(c, c->rout_ids, no * 4)) || (st = ensure(c, c->rout_dist, no * 4))) return st;
      pq_narrow_ids_kernel<<<static_cast<unsigned>((nc + 255) / 256), 256, 0, s>>>(static_cast<const unsigned long long*>(ps->out_ids.p), nc, c->row_base,
                                                                                static_cast<uint32_t*>(c->rcand.p));
      HIPCHK(c, hipGetLastError());
      if ((st = nvdb_hip_refine_l2_topk_dev(c, static_cast<const float*>(ps->q.p), static_cast<const uint32_t*>(c->rcand.p), b, r_dev, rf->K,
                                            static_cast<uint32_t*>(c->rout_ids.p), rf->out_dist ? static_cast<float*>(c->rout_dist.p) : nullptr, s)))
        return st;
      h_rid.resize(no);
      HIPCHK(c, hipMemcpyAsync(h_rid.data(), c->rout_ids.p, no * 4, hipMemcpyDeviceToHost, s));
      if (rf->out_dist) HIPCHK(c, hipMemcpyAsync(rf->out_dist + static_cast<size_t>(q0) * rf->K, c->rout_dist.p, no * 4, hipMemcpyDeviceToHost, s));
    }
    if ((st = pa_sub_finish(c, s, sub, b, R, ids0, sc0, out_counts ? out_counts + q0 : nullptr))) return st;
    for (uint32_t q = 0; l2_out && sub.plan.out_k < R && q < b; ++q)   // (the host's padding beyond the device rows' width)
      std::fill(sc0 + static_cast<size_t>(q) * R + sub.plan.out_k, sc0 + static_cast<size_t>(q + 1) * R, pos_inf);
    if (rf)
      for (size_t i = 0; i < h_rid.size(); ++i) rf->out_ids[static_cast<size_t>(q0) * rf->K + i] = h_rid[i] == 0xFFFFFFFFu ? ~0ull : c->row_base + h_rid[i];
    c->stats.rows_scanned += p.wl.rows_read;
    q0 = q1;
  }
  if ((st = parts_call_end(c, timing))) return st;
  if (timing) {
    timing->K = rf ? rf->K : R; timing->R = R;
    timing->threads = PQ_SCAN_THREADS; timing->shmem_bytes = b4 ? pq4_scan_lds(pq.M, group) : group * lut_bytes;
  }
  return NVDB_OK;
}

// what every PQ call checks first: a context, a corpus, codes
nvdb_status pq_args(nvdb_hip_ctx* c, const char* who) {
  if (!c) return NVDB_ERR_INVALID;
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (!c->pq) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": no PQ codes: nvdb_hip_pq_build");
  return NVDB_OK;
}

nvdb_status pq_search_args(nvdb_hip_ctx* c, const char* who, bool ivf, const float* queries, uint32_t nq, uint32_t R, const uint32_t* probe, uint32_t nprobe,
                           uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nvdb_hip_timing* timing, bool* done) {
  *done = true;
  if (nvdb_status st = pq_args(c, who)) return st;
  const nvdb_status st = parts_topk_args(c, who, ivf, 0, queries, nq, R, probe, nprobe, nullptr, out_ids, out_scores, out_counts, timing, done);
  if (!st && *done && c->pq->metric && nq && R && nprobe == 0) std::fill(out_scores, out_scores + static_cast<size_t>(nq) * R, __builtin_huge_valf());   // all padding: +inf under L2
  return st;
}

// nvdb_hip_pq_build / nvdb_hip_pq_build_residual: on any failure nothing has changed
// opq: the codes are cut from A e (rotation: host, [dim][dim]); else rotation is not looked at.  nbits: 8, or 4 (nvdb_hip_pq4_build)
nvdb_status pq_build(nvdb_hip_ctx* c, const char* who, bool residual, const float* codebooks, uint32_t M, bool opq = false, const float* rotation = nullptr,
                     uint32_t nbits = 8) {
  if (!c) return NVDB_ERR_INVALID;
  const std::string w = std::string(who) + ": ";
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (opq && !rotation) return fail(c, NVDB_ERR_INVALID, w + "null rotation");
  if (!codebooks) return fail(c, NVDB_ERR_INVALID, w + "null codebooks");
  bool unsupported = false;
  if (const char* why = nbits == 4 ? pq4_shape_check(c->dim, M, residual, unsupported) : pq_shape_check(c->dim, M, unsupported))
    return fail(c, unsupported ? NVDB_ERR_UNSUPPORTED : NVDB_ERR_INVALID, w + why);
  if (residual)
    if (nvdb_status st = resid_args(c, who)) return st;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  PqState fresh;
  fresh.M = M; fresh.dsub = c->dim / M;
  fresh.nbits = nbits;
  fresh.residual = residual;
  const size_t row_bytes = pq_row_bytes(M, nbits);
  const size_t cb_bytes = static_cast<size_t>(M) * (nbits == 4 ? PQ4_KSUB : PQ_KSUB) * fresh.dsub * 4;
  const size_t code_bytes = static_cast<size_t>(c->n) * row_bytes, pad_bytes = static_cast<size_t>(PAD_ROWS) * row_bytes;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&fresh.codebooks), cb_bytes);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&fresh.codes), code_bytes + pad_bytes);
  if (e == hipSuccess) e = hipMemcpyAsync(fresh.codebooks, codebooks, cb_bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(fresh.codes + code_bytes, 0, pad_bytes, s);
  if (residual) {
    // the shadow's own copies: the table as u32, the centroids from where set_centroids put them (the child context's f32 rows)
    const std::vector<uint32_t> off = resid_offsets(c);
    fresh.nparts = static_cast<uint32_t>(off.size() - 1);
    const size_t cent_bytes = static_cast<size_t>(fresh.nparts) * c->dim * 4;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&fresh.off), off.size() * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&fresh.cent), cent_bytes);
    if (e == hipSuccess) e = hipMemcpy(fresh.off, off.data(), off.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpyAsync(fresh.cent, c->parts->coarse->rows, cent_bytes, hipMemcpyDeviceToDevice, s);
  }
  TrainMem d_slab;                                                     // a rotated build's f32 rows, a slab at a time; lives as long as the call
  const uint64_t slab = std::min<uint64_t>(c->n, pq_rotate_slab_rows(c->dim));
  if (opq) {
    // the shadow's own copies of A and of A^T (transposed here, once)
    const size_t d = c->dim, rot_bytes = d * d * 4;
    std::vector<float> at(d * d);
    for (size_t i = 0; i < d; ++i)
      for (size_t t = 0; t < d; ++t) at[t * d + i] = rotation[i * d + t];
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&fresh.rot), rot_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&fresh.rot_t), rot_bytes);
    if (e == hipSuccess) e = hipMalloc(&d_slab.p, slab * d * 4);
    if (e == hipSuccess) e = hipMemcpy(fresh.rot, rotation, rot_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(fresh.rot_t, at.data(), rot_bytes, hipMemcpyHostToDevice);
  }
  nvdb_status st = NVDB_OK;
  if (e != hipSuccess) st = fail(c, NVDB_ERR_HIP, w + hipGetErrorString(e));
  if (!st && !opq)
    dispatch_dtype(c->dtype, st, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      return nbits == 4 ? launch_encode4<DT>(c, s, fresh, residual, c->rows, c->scales, c->n, fresh.codes)
                        : launch_encode<DT>(c, s, fresh, residual, c->rows, c->scales, c->n, fresh.codes);
    });
  // rotated: per slab the product into the scratch rows, then the f32 non-residual encode over them (the centroid is gone already)
  for (uint64_t r = 0; opq && !st && r < c->n; r += slab) {
    const uint32_t nr = static_cast<uint32_t>(std::min<uint64_t>(slab, c->n - r));
    dispatch_dtype(c->dtype, st, [&](auto dt) {
      return launch_rotate<decltype(dt)::value>(c, s, c->rows, c->scales, r, nr, fresh.rot, fresh.off, fresh.nparts, residual ? fresh.cent : nullptr, d_slab.as<float>());
    });
    if (!st) st = nbits == 4 ? launch_encode4<DT_F32>(c, s, fresh, false, d_slab.p, nullptr, nr, fresh.codes + r * row_bytes)
                             : launch_encode<DT_F32>(c, s, fresh, false, d_slab.p, nullptr, nr, fresh.codes + r * row_bytes);
  }
  if (!st && (e = hipStreamSynchronize(s)) != hipSuccess) st = fail(c, NVDB_ERR_HIP, w + hipGetErrorString(e));
  if (st) {                                                            // nothing changed: an earlier build stands
    if (opq) (void)hipStreamSynchronize(s);                            // (before the slab leaves scope)
    (void)hipGetLastError();
    if (fresh.codebooks) (void)hipFree(fresh.codebooks);
    if (fresh.codes) (void)hipFree(fresh.codes);
    if (fresh.off) (void)hipFree(fresh.off);
    if (fresh.cent) (void)hipFree(fresh.cent);
    if (fresh.rot) (void)hipFree(fresh.rot);
    if (fresh.rot_t) (void)hipFree(fresh.rot_t);
    return st;
  }
  pq_drop(c);
  c->pq = new PqState(fresh);
  return NVDB_OK;
}

// the device part of nvdb_hip_pq_reconstruct: rows row0 .. row0 + nr as their codes describe them, enqueued on the context's stream.
// d_y / d_x: [nr][dim] f32 (d_x: a rotated shadow's rows back in the corpus' space, else not looked at); *xhat: which of the two holds them
nvdb_status reconstruct_slab(nvdb_hip_ctx* c, const PqState& pq, uint32_t row0, uint32_t nr, float* d_y, float* d_x, const float** xhat) {
  const unsigned grid = std::min<unsigned>((nr + 3u) / 4u, static_cast<unsigned>(c->num_cu) * 64u);
  // a rotated shadow: the codewords side by side, times A^T, and only then the centroid
  const float* cent = pq.residual && !pq.rot ? pq.cent : nullptr;
  if (pq.nbits == 4) pq4_reconstruct_kernel<<<grid, 256, 0, c->stream>>>(pq.codes, pq.M, pq.dsub, pq.codebooks, pq.off, pq.nparts, cent, row0, nr, d_y);
  else pq_reconstruct_kernel<<<grid, 256, 0, c->stream>>>(pq.codes, pq.M, pq.dsub, pq.codebooks, pq.off, pq.nparts, cent, row0, nr, d_y);
  HIPCHK(c, hipGetLastError());
  *xhat = d_y;
  if (pq.rot) {
    if (nvdb_status st = launch_rotate_f32(c, c->stream, d_y, nr, pq.rot_t, d_x)) return st;
    if (pq.residual) {
      pq_rotate_add_cent_kernel<<<grid, 256, 0, c->stream>>>(d_x, row0, nr, c->dim, pq.off, pq.nparts, pq.cent);
      HIPCHK(c, hipGetLastError());
    }
    *xhat = d_x;
  }
  return NVDB_OK;
}

// nvdb_hip_pq_set_metric(1): h[r] for the shadow the context holds, into memory of its own; on any failure nothing has changed
nvdb_status pq_half_norms(nvdb_hip_ctx* c, const char* who, float** out) {
  const PqState& pq = *c->pq;
  const std::string w = std::string(who) + ": ";
  if (c->n > IVF_MAX_ROWS) return fail(c, NVDB_ERR_UNSUPPORTED, w + "corpus shard too large");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const uint32_t n = static_cast<uint32_t>(c->n);
  TrainMem d_h, d_y, d_x;                                              // d_y / d_x: a rotated shadow's slabs
  nvdb_status st = train_alloc(c, d_h, pq_norm_bytes(n));
  if (!st && !pq.rot) {
    // the codewords' squares straight from the codes: no f32 rows in HBM
    const unsigned grid = (n + PQ_NORM_TILE - 1u) / PQ_NORM_TILE;
    auto go = [&](auto kernel) { kernel<<<grid, PQ_NORM_THREADS, 0, s>>>(pq.codes, n, pq.M, pq.dsub, pq.codebooks, pq.off, pq.nparts, pq.cent, d_h.as<float>()); };
    if (pq.nbits == 4) { if (pq.residual) go(pq_norms_kernel<4, true>); else go(pq_norms_kernel<4, false>); }
    else { if (pq.residual) go(pq_norms_kernel<8, true>); else go(pq_norms_kernel<8, false>); }
    if (hipGetLastError() != hipSuccess) st = fail(c, NVDB_ERR_HIP, w + "launch of the norms kernel");
  } else if (!st) {
    // a rotation: xhat is the full transpose product -- reconstruct's device part slab by slab, the chain over each f32 slab
    const uint32_t step = static_cast<uint32_t>(std::min<uint64_t>(n, pq_reconstruct_rows(c->dim)));
    if (!(st = train_alloc(c, d_y, static_cast<size_t>(step) * c->dim * 4))) st = train_alloc(c, d_x, static_cast<size_t>(step) * c->dim * 4);
    for (uint32_t r = 0; !st && r < n; r += step) {
      const uint32_t nr = std::min<uint32_t>(step, n - r);
      const float* xhat = nullptr;
      if ((st = reconstruct_slab(c, pq, r, nr, d_y.as<float>(), d_x.as<float>(), &xhat))) break;
      pq_rownorm_kernel<<<(nr + PQ_NORM_THREADS - 1u) / PQ_NORM_THREADS, PQ_NORM_THREADS, 0, s>>>(xhat, nr, c->dim, d_h.as<float>() + r);
      if (hipGetLastError() != hipSuccess) st = fail(c, NVDB_ERR_HIP, w + "launch of the row-norm kernel");
    }
  }
  const hipError_t e = hipStreamSynchronize(s);                        // (before the slabs leave scope, whatever happened)
  if (!st && e != hipSuccess) st = fail(c, NVDB_ERR_HIP, w + hipGetErrorString(e));
  if (st) { (void)hipGetLastError(); return st; }
  *out = d_h.as<float>();
  d_h.p = nullptr;                                                     // (the shadow's from here on)
  return NVDB_OK;
}

// every training entry point behind one set of checks.  nbits: 8, or 4 (nvdb_hip_pq4_train: pq4_shape_check, 16 codewords)
nvdb_status pq_train_call(nvdb_hip_ctx* c, const char* who, bool residual, uint32_t M, uint32_t iters, uint64_t seed, uint64_t max_train_rows, const float* init,
                          float* out_codebooks, double* out_err, bool opq = false, const float* rotation = nullptr, uint32_t nbits = 8) {
  if (!c) return NVDB_ERR_INVALID;
  const std::string w = std::string(who) + ": ";
  if (opq && !rotation) return fail(c, NVDB_ERR_INVALID, w + "null rotation");
  if (!out_codebooks) return fail(c, NVDB_ERR_INVALID, w + "null output");
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  bool unsupported = false;
  if (const char* why = nbits == 4 ? pq4_shape_check(c->dim, M, residual, unsupported) : pq_shape_check(c->dim, M, unsupported))
    return fail(c, unsupported ? NVDB_ERR_UNSUPPORTED : NVDB_ERR_INVALID, w + why);
  if (residual)
    if (nvdb_status st = resid_args(c, who)) return st;
  const uint64_t m = pq_train_rows(c->n, max_train_rows);
  if (m < (nbits == 4 ? PQ4_TRAIN_MIN_ROWS : PQ_TRAIN_MIN_ROWS)) return fail(c, NVDB_ERR_INVALID, w + (nbits == 4 ? "fewer than 16 training rows" : "fewer than 256 training rows"));
  if (m > IVF_MAX_ROWS) return fail(c, NVDB_ERR_UNSUPPORTED, w + "training set too large (max_train_rows)");
  std::vector<float> cb(static_cast<size_t>(M) * (nbits == 4 ? PQ4_KSUB : PQ_KSUB) * (c->dim / M));
  std::vector<double> err(iters);
  if (nvdb_status st = pq_train(c, residual, opq ? rotation : nullptr, M, iters, seed, m, init, cb, err, nbits)) {
    (void)hipGetLastError();
    return st;
  }
  std::memcpy(out_codebooks, cb.data(), cb.size() * 4);
  if (out_err && iters) std::memcpy(out_err, err.data(), err.size() * 8);
  return NVDB_OK;
}

}  // namespace
}  // namespace nvdbhip

extern "C" {

nvdb_status nvdb_hip_pq_build(nvdb_hip_ctx* c, const float* codebooks, uint32_t M) { return pq_build(c, "pq_build", false, codebooks, M); }

nvdb_status nvdb_hip_pq_build_residual(nvdb_hip_ctx* c, const float* codebooks, uint32_t M) { return pq_build(c, "pq_build_residual", true, codebooks, M); }

nvdb_status nvdb_hip_pq_train(nvdb_hip_ctx* c, uint32_t M, uint32_t iters, uint64_t seed, uint64_t max_train_rows, const float* init, float* out_codebooks,
                              double* out_err) {
  return pq_train_call(c, "pq_train", false, M, iters, seed, max_train_rows, init, out_codebooks, out_err);
}

nvdb_status nvdb_hip_pq_train_residual(nvdb_hip_ctx* c, uint32_t M, uint32_t iters, uint64_t seed, uint64_t max_train_rows, const float* init,
                                       float* out_codebooks, double* out_err) {
  return pq_train_call(c, "pq_train_residual", true, M, iters, seed, max_train_rows, init, out_codebooks, out_err);
}

nvdb_status nvdb_hip_pq_build_opq(nvdb_hip_ctx* c, const float* rotation, const float* codebooks, uint32_t M, uint32_t residual) {
  return pq_build(c, "pq_build_opq", residual != 0, codebooks, M, true, rotation);
}

nvdb_status nvdb_hip_pq_train_opq(nvdb_hip_ctx* c, const float* rotation, uint32_t M, uint32_t iters, uint64_t seed, uint64_t max_train_rows, const float* init,
                                  float* out_codebooks, double* out_err, uint32_t residual) {
  return pq_train_call(c, "pq_train_opq", residual != 0, M, iters, seed, max_train_rows, init, out_codebooks, out_err, true, rotation);
}

nvdb_status nvdb_hip_pq4_build(nvdb_hip_ctx* c, const float* rotation, const float* codebooks, uint32_t M, uint32_t residual) {
  return pq_build(c, "pq4_build", residual != 0, codebooks, M, rotation != nullptr, rotation, 4);
}

nvdb_status nvdb_hip_pq4_train(nvdb_hip_ctx* c, const float* rotation, uint32_t M, uint32_t iters, uint64_t seed, uint64_t max_train_rows, const float* init,
                               float* out_codebooks, double* out_err, uint32_t residual) {
  return pq_train_call(c, "pq4_train", residual != 0, M, iters, seed, max_train_rows, init, out_codebooks, out_err, rotation != nullptr, rotation, 4);
}

nvdb_status nvdb_hip_pq_bits(nvdb_hip_ctx* c, uint32_t* nbits) {
  if (!c) return NVDB_ERR_INVALID;
  if (nbits) *nbits = c->pq ? c->pq->nbits : 0u;
  return NVDB_OK;
}

nvdb_status nvdb_hip_pq_rotation(nvdb_hip_ctx* c, uint32_t* rotated, float* out) {
  if (!c) return NVDB_ERR_INVALID;
  const bool have = c->pq && c->pq->rot;
  if (rotated) *rotated = have ? 1u : 0u;
  if (have && out) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->pq->rot, static_cast<size_t>(c->dim) * c->dim * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return NVDB_OK;
}

nvdb_status nvdb_hip_pq_rotated_rows(nvdb_hip_ctx* c, uint64_t row0, uint64_t nrows, float* out) {
  if (nvdb_status st = pq_args(c, "pq_rotated_rows")) return st;
  if (!c->pq->rot) return fail(c, NVDB_ERR_INVALID, "pq_rotated_rows: the shadow has no rotation: nvdb_hip_pq_build_opq");
  if (row0 > c->n || nrows > c->n - row0) return fail(c, NVDB_ERR_INVALID, "pq_rotated_rows: row0 + nrows > n");
  if (nrows == 0) return NVDB_OK;
  if (!out) return fail(c, NVDB_ERR_INVALID, "pq_rotated_rows: null output");
  HIPCHK(c, hipSetDevice(c->device));
  const PqState& pq = *c->pq;
  const uint64_t step = std::min<uint64_t>(nrows, pq_reconstruct_rows(c->dim));
  TrainMem d_y;
  if (nvdb_status st = train_alloc(c, d_y, step * c->dim * 4)) return st;
  for (uint64_t r = 0; r < nrows; r += step) {
    const uint32_t nr = static_cast<uint32_t>(std::min<uint64_t>(step, nrows - r));
    nvdb_status st = NVDB_OK;
    dispatch_dtype(c->dtype, st, [&](auto dt) {
      return launch_rotate<decltype(dt)::value>(c, c->stream, c->rows, c->scales, row0 + r, nr, pq.rot, pq.off, pq.nparts, pq.residual ? pq.cent : nullptr, d_y.as<float>());
    });
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(out + r * c->dim, d_y.p, static_cast<size_t>(nr) * c->dim * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return NVDB_OK;
}

nvdb_status nvdb_hip_pq_rotate(nvdb_hip_ctx* c, const float* x, uint64_t n, float* out) {
  if (nvdb_status st = pq_args(c, "pq_rotate")) return st;
  if (!c->pq->rot) return fail(c, NVDB_ERR_INVALID, "pq_rotate: the shadow has no rotation: nvdb_hip_pq_build_opq");
  if (n == 0) return NVDB_OK;
  if (!x || !out) return fail(c, NVDB_ERR_INVALID, x ? "pq_rotate: null output" : "pq_rotate: null vectors");
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t step = std::min<uint64_t>(n, pq_reconstruct_rows(c->dim));
  const size_t bytes = step * c->dim * 4;
  TrainMem d_x, d_y;
  nvdb_status st;
  if ((st = train_alloc(c, d_x, bytes)) || (st = train_alloc(c, d_y, bytes))) return st;
  for (uint64_t r = 0; r < n; r += step) {
    const uint32_t nr = static_cast<uint32_t>(std::min<uint64_t>(step, n - r));
    HIPCHK(c, hipMemcpyAsync(d_x.p, x + r * c->dim, static_cast<size_t>(nr) * c->dim * 4, hipMemcpyHostToDevice, c->stream));
    if ((st = launch_rotate_f32(c, c->stream, d_x.as<float>(), nr, c->pq->rot, d_y.as<float>()))) return st;
    HIPCHK(c, hipMemcpyAsync(out + r * c->dim, d_y.p, static_cast<size_t>(nr) * c->dim * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return NVDB_OK;
}

nvdb_status nvdb_hip_pq_kind(nvdb_hip_ctx* c, uint32_t* residual) {
  if (!c) return NVDB_ERR_INVALID;
  if (residual) *residual = (c->pq && c->pq->residual) ? 1u : 0u;
  return NVDB_OK;
}

nvdb_status nvdb_hip_pq_reconstruct(nvdb_hip_ctx* c, uint64_t row0, uint64_t nrows, float* out) {
  if (nvdb_status st = pq_args(c, "pq_reconstruct")) return st;
  if (row0 > c->n || nrows > c->n - row0) return fail(c, NVDB_ERR_INVALID, "pq_reconstruct: row0 + nrows > n");
  if (nrows == 0) return NVDB_OK;
  if (!out) return fail(c, NVDB_ERR_INVALID, "pq_reconstruct: null output");
  if (c->n > IVF_MAX_ROWS) return fail(c, NVDB_ERR_UNSUPPORTED, "pq_reconstruct: corpus shard too large");
  HIPCHK(c, hipSetDevice(c->device));
  const PqState& pq = *c->pq;
  const uint64_t step = std::min<uint64_t>(nrows, pq_reconstruct_rows(c->dim));
  TrainMem d_y, d_x;                                                   // d_x: a rotated shadow's rows back in the corpus' space
  if (nvdb_status st = train_alloc(c, d_y, step * c->dim * 4)) return st;
  if (pq.rot)
    if (nvdb_status st = train_alloc(c, d_x, step * c->dim * 4)) return st;
  for (uint64_t r = 0; r < nrows; r += step) {
    const uint32_t nr = static_cast<uint32_t>(std::min<uint64_t>(step, nrows - r));
    const float* xhat = nullptr;
    if (nvdb_status st = reconstruct_slab(c, pq, static_cast<uint32_t>(row0 + r), nr, d_y.as<float>(), d_x.as<float>(), &xhat)) return st;
    HIPCHK(c, hipMemcpyAsync(out + r * c->dim, xhat, static_cast<size_t>(nr) * c->dim * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return NVDB_OK;
}

nvdb_status nvdb_hip_pq_set_metric(nvdb_hip_ctx* c, uint32_t metric) {
  if (!c) return NVDB_ERR_INVALID;
  if (metric > 1u) return fail(c, NVDB_ERR_INVALID, "pq_set_metric: metric must be 0 (dot product) or 1 (squared L2)");
  if (metric == 0u && !c->pq) return NVDB_OK;                          // (the default already)
  if (nvdb_status st = pq_args(c, "pq_set_metric")) return st;
  PqState& pq = *c->pq;
  if (metric == pq.metric) return NVDB_OK;
  if (metric == 0u) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(pq.half_norm);
    pq.half_norm = nullptr;
    pq.metric = 0u;
    return NVDB_OK;
  }
  float* h = nullptr;
  if (nvdb_status st = pq_half_norms(c, "pq_set_metric", &h)) return st;
  pq.half_norm = h;
  pq.metric = 1u;
  return NVDB_OK;
}

nvdb_status nvdb_hip_pq_metric(nvdb_hip_ctx* c, uint32_t* metric) {
  if (!c) return NVDB_ERR_INVALID;
  if (!metric) return fail(c, NVDB_ERR_INVALID, "pq_metric: null output");
  *metric = c->pq ? c->pq->metric : 0u;
  return NVDB_OK;
}

nvdb_status nvdb_hip_pq_norms(nvdb_hip_ctx* c, uint64_t row0, uint64_t nrows, float* out) {
  if (nvdb_status st = pq_args(c, "pq_norms")) return st;
  if (!c->pq->metric) return fail(c, NVDB_ERR_INVALID, "pq_norms: the metric is not squared L2: nvdb_hip_pq_set_metric");
  if (row0 > c->n || nrows > c->n - row0) return fail(c, NVDB_ERR_INVALID, "pq_norms: row0 + nrows > n");
  if (nrows == 0) return NVDB_OK;
  if (!out) return fail(c, NVDB_ERR_INVALID, "pq_norms: null output");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(out, c->pq->half_norm + row0, nrows * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (uint64_t i = 0; i < nrows; ++i) out[i] = out[i] + out[i];       // n = h + h: the halving is undone exactly (short of a subnormal n)
  return NVDB_OK;
}

nvdb_status nvdb_hip_pq_info(nvdb_hip_ctx* c, uint32_t* M, uint32_t* dsub, uint64_t* code_bytes) {
  if (!c) return NVDB_ERR_INVALID;
  const PqState* pq = c->pq;
  if (M) *M = pq ? pq->M : 0u;
  if (dsub) *dsub = pq ? pq->dsub : 0u;
  if (code_bytes) *code_bytes = pq ? c->n * pq_row_bytes(pq->M, pq->nbits) : 0ull;
  return NVDB_OK;
}

nvdb_status nvdb_hip_pq_download_codes(nvdb_hip_ctx* c, uint64_t row0, uint64_t nrows, uint8_t* out) {
  if (nvdb_status st = pq_args(c, "pq_download_codes")) return st;
  if (row0 > c->n || nrows > c->n - row0) return fail(c, NVDB_ERR_INVALID, "pq_download_codes: row0 + nrows > n");
  if (nrows == 0) return NVDB_OK;
  if (!out) return fail(c, NVDB_ERR_INVALID, "pq_download_codes: null output");
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t row_bytes = pq_row_bytes(c->pq->M, c->pq->nbits);
  HIPCHK(c, hipMemcpyAsync(out, c->pq->codes + row0 * row_bytes, nrows * row_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NVDB_OK;
}

nvdb_status nvdb_hip_pq_search_partitions(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t R, const uint32_t* probe, uint32_t nprobe,
                                          uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nvdb_hip_timing* timing) {
  const char* who = "pq_search_partitions";
  bool done;
  const nvdb_status st = pq_search_args(c, who, false, queries, nq, R, probe, nprobe, out_ids, out_scores, out_counts, timing, &done);
  if (st || done) return st;
  return pq_search(c, who, queries, nq, R, probe, nprobe, out_ids, out_scores, out_counts, nullptr, timing);
}

nvdb_status nvdb_hip_pq_search_ivf(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t R, uint32_t nprobe, uint64_t* out_ids, float* out_scores,
                                   uint32_t* out_counts, uint32_t* out_probe, nvdb_hip_timing* timing) {
  const char* who = "pq_search_ivf";
  bool done;
  nvdb_status st = pq_search_args(c, who, true, queries, nq, R, nullptr, nprobe, out_ids, out_scores, out_counts, timing, &done);
  if (st || done) return st;
  uint32_t np = 0;
  if ((st = parts_coarse(c, who, queries, nq, nprobe, out_probe, timing, np))) return st;
  return pq_search(c, who, queries, nq, R, c->parts->probe_tmp.data(), np, out_ids, out_scores, out_counts, nullptr, timing);
}

nvdb_status nvdb_hip_pq_refine_ivf(nvdb_hip_ctx* c, const float* queries, uint32_t nq, uint32_t K, uint32_t R, uint32_t nprobe, uint64_t* out_ids,
                                   float* out_dist, uint32_t* out_probe, nvdb_hip_timing* timing) {
  const char* who = "pq_refine_ivf";
  nvdb_status st = pq_args(c, who);
  if (st || (st = parts_args(c, who))) return st;
  if (!c->parts->have_centroids) return fail(c, NVDB_ERR_INVALID, std::string(who) + ": no centroids (nvdb_hip_set_centroids)");
  if (timing) std::memset(timing, 0, sizeof(*timing));
  if (nq == 0 || R == 0 || K == 0) return NVDB_OK;
  if (c->dtype != NVDB_DTYPE_F16 && c->dtype != NVDB_DTYPE_F32) return fail(c, NVDB_ERR_UNSUPPORTED, "refine supports base dtype fp16/fp32 only");
  if (K > NVDB_HIP_REFINE_KMAX) return fail(c, NVDB_ERR_INVALID, "refine: K not supported (K<=64)");
  if (!queries || !out_ids) return fail(c, NVDB_ERR_INVALID, queries ? "null output" : "Null query");
  if (nprobe == 0) {
    std::fill(out_ids, out_ids + static_cast<size_t>(nq) * K, ~0ull);
    if (out_dist) std::fill(out_dist, out_dist + static_cast<size_t>(nq) * K, 1e30f);
    return NVDB_OK;
  }
  uint32_t np = 0;
  if ((st = parts_coarse(c, who, queries, nq, nprobe, out_probe, timing, np))) return st;
  const PqRefine rf{K, out_ids, out_dist};
  return pq_search(c, who, queries, nq, R, c->parts->probe_tmp.data(), np, nullptr, nullptr, nullptr, &rf, timing);
}

}  // extern "C"
