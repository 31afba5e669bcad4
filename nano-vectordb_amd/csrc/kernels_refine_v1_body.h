// kernels_refine_v1_body.h -- body of refine v1 (lane per candidate row), included by kernels_refine.h as the body of the product kernel
// (STAMP = false) and of its stamped twin (STAMP = true, option refine_dbg_q).  Not a standalone header: the
// enclosing kernel declares STAMP, dbg_out and dbg_q.
  __shared__ float lds_d[4][64];
  __shared__ uint32_t lds_id[4][64];
  __shared__ uint32_t lds_cnt[4];
  const uint32_t q = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  [[maybe_unused]] const bool stamp = STAMP && q < dbg_q && __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0;
  [[maybe_unused]] uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
  if constexpr (STAMP) { if (stamp) t0 = refine_stamp(); }
  const float* __restrict__ qv = queries + static_cast<uint64_t>(q) * dim;
  const uint32_t* __restrict__ cq = cand + static_cast<uint64_t>(q) * R;

  WaveTopKMin tk;
  tk.d = 1e30f; tk.id = 0xFFFFFFFFu; tk.cnt = 0; tk.thr_d = 1e30f; tk.thr_id = 0xFFFFFFFFu;

  for (uint32_t r0 = wave * 64u; r0 < R; r0 += 256u) {
    const uint32_t r = r0 + lane;
    const uint32_t id = (r < R) ? cq[r] : 0xFFFFFFFFu;
    const bool valid = (id != 0xFFFFFFFFu) && (static_cast<uint64_t>(id) < n);     // cuda_refine.cu:437
    const uint32_t rid = valid ? id : 0u;
    float d;
    if constexpr (DT == DT_F16) d = l2_f16_ref_order<ALIGNED>(static_cast<const unsigned short*>(rows) + static_cast<uint64_t>(rid) * dim, qv, dim);
    else d = l2_f32_ref_order<ALIGNED>(static_cast<const float*>(rows) + static_cast<uint64_t>(rid) * dim, qv, dim);
    unsigned long long m = __ballot(valid && wmin_accepts(tk, K, d, id));
    while (m) {
      const int L = __builtin_ctzll(m);
      m &= m - 1;
      const float cd = readlane_f(d, L);
      const uint32_t cid = readlane_u(id, L);
      if (wmin_accepts(tk, K, cd, cid)) wmin_insert(tk, K, cd, cid, lane);
    }
  }
  if constexpr (STAMP) { if (stamp) t1 = refine_stamp(); }
  lds_d[wave][lane] = tk.d; lds_id[wave][lane] = tk.id;
  if (lane == 0) lds_cnt[wave] = tk.cnt;
  __syncthreads();
  if (wave != 0) return;
  if constexpr (STAMP) { if (stamp) t2 = refine_stamp(); }
  for (int w = 1; w < 4; ++w) {
    const uint32_t c = lds_cnt[w];
    for (uint32_t j = 0; j < c; ++j) {
      const float cd = lds_d[w][j];
      const uint32_t cid = lds_id[w][j];
      if (wmin_accepts(tk, K, cd, cid)) wmin_insert(tk, K, cd, cid, lane);
    }
  }
  if (static_cast<uint32_t>(lane) < K) {
    const bool have = static_cast<uint32_t>(lane) < tk.cnt;
    out_ids[static_cast<uint64_t>(q) * K + lane] = have ? tk.id : 0xFFFFFFFFu;
    if (out_dist) out_dist[static_cast<uint64_t>(q) * K + lane] = have ? tk.d : 1e30f;
  }
  if constexpr (STAMP) {
    if (stamp) {
      t3 = refine_stamp();
      if (lane == 0) refine_stamp_store(dbg_out, q, t0, t1, t2, t3);
    }
  }
