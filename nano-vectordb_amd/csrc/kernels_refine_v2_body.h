// kernels_refine_v2_body.h -- body of refine v2 (column chunks through LDS), included by kernels_refine.h as the body of the product kernel
// (STAMP = false) and of its stamped twin (STAMP = true, option refine_dbg_q).  Not a standalone header: the
// enclosing kernel declares STAMP, dbg_out and dbg_q.
  constexpr int BPE = (DT == DT_F16) ? 2 : 4;
  constexpr int CH_BYTES = 256, CH_ELEMS = CH_BYTES / BPE, BUF_BYTES = 64 * CH_BYTES;   // 16 KB per wave buffer
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float lds_d[4][64];
  __shared__ uint32_t lds_id[4][64];
  __shared__ uint32_t lds_cnt[4];
  const uint32_t q = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float* __restrict__ qv = queries + static_cast<uint64_t>(q) * dim;
  const uint32_t* __restrict__ cq = cand + static_cast<uint64_t>(q) * R;
  const uint32_t row_bytes = dim * BPE;
  const uint32_t nchunks = (row_bytes + CH_BYTES - 1) / CH_BYTES;
  char* mybuf = smem + wave * 2 * BUF_BYTES;
  const uint32_t lds_mine = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(NVDB_LPTR(mybuf)));
  const char* gbase = static_cast<const char*>(rows);
  [[maybe_unused]] const bool stamp = STAMP && q < dbg_q && wave == 0;
  [[maybe_unused]] uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
  if constexpr (STAMP) { if (stamp) t0 = refine_stamp(); }

  WaveTopKMin tk;
  tk.d = 1e30f; tk.id = 0xFFFFFFFFu; tk.cnt = 0; tk.thr_d = 1e30f; tk.thr_id = 0xFFFFFFFFu;

  const uint32_t sub = lane >> 4, pos = lane & 15;           // piece p stages rows 4p..4p+3; this lane: row 4p+sub, slot pos
  for (uint32_t r0 = wave * 64u; r0 < R; r0 += 256u) {
    const uint32_t r = r0 + lane;
    const uint32_t id = (r < R) ? cq[r] : 0xFFFFFFFFu;
    const bool valid = (id != 0xFFFFFFFFu) && (static_cast<uint64_t>(id) < n);     // cuda_refine.cu:437
    const uint32_t rid = valid ? id : 0u;                    // invalid lanes gather row 0 and are dropped below
    // row ids this lane gathers for: rows 4p+sub, p = 0..15
    uint32_t src_row_off_lo[16], src_row_off_hi[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const uint32_t rr = static_cast<uint32_t>(__shfl(static_cast<int>(rid), 4 * p + static_cast<int>(sub)));
      const uint64_t off = static_cast<uint64_t>(rr) * row_bytes;
      src_row_off_lo[p] = static_cast<uint32_t>(off); src_row_off_hi[p] = static_cast<uint32_t>(off >> 32);
    }
    auto issue_chunk = [&](uint32_t c, uint32_t buf) {
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        const uint32_t rowi = 4u * p + sub;
        uint32_t coff = c * CH_BYTES + ((pos ^ (rowi & 15u)) << 4);          // source chunk for LDS slot `pos`
        if (coff + 16 > row_bytes) coff = row_bytes - 16;                     // ragged last chunk: any in-row bytes (unused)
        const uint64_t off = ((static_cast<uint64_t>(src_row_off_hi[p]) << 32) | src_row_off_lo[p]) + coff;
        glds16_v(gbase + off, lds_mine + buf * BUF_BYTES + p * 1024);
      }
    };
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    issue_chunk(0, 0);
    for (uint32_t c = 0; c < nchunks; ++c) {
      if (c + 1 < nchunks) { issue_chunk(c + 1, (c + 1) & 1u); asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); }
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const char* rowc = mybuf + (c & 1u) * BUF_BYTES + lane * CH_BYTES;
      const uint32_t e0 = c * CH_ELEMS;
      const uint32_t ne = (dim - e0 < static_cast<uint32_t>(CH_ELEMS)) ? dim - e0 : static_cast<uint32_t>(CH_ELEMS);
      if constexpr (DT == DT_F16) {
        for (uint32_t j = 0; j * 8 < ne; ++j) {                              // 8 dims = 4 pairs per 16-byte slot
          const uint4 v = *reinterpret_cast<const uint4*>(rowc + ((j ^ (static_cast<uint32_t>(lane) & 15u)) << 4));
          const float* qq = qv + e0 + 8 * j;
          float dx, dy;
          dx = qq[0] - half_bits_to_float(v.x & 0xFFFFu); dy = qq[1] - half_bits_to_float(v.x >> 16); a0 = __builtin_fmaf(dx, dx, a0); a0 = __builtin_fmaf(dy, dy, a0);
          dx = qq[2] - half_bits_to_float(v.y & 0xFFFFu); dy = qq[3] - half_bits_to_float(v.y >> 16); a1 = __builtin_fmaf(dx, dx, a1); a1 = __builtin_fmaf(dy, dy, a1);
          dx = qq[4] - half_bits_to_float(v.z & 0xFFFFu); dy = qq[5] - half_bits_to_float(v.z >> 16); a2 = __builtin_fmaf(dx, dx, a2); a2 = __builtin_fmaf(dy, dy, a2);
          dx = qq[6] - half_bits_to_float(v.w & 0xFFFFu); dy = qq[7] - half_bits_to_float(v.w >> 16); a3 = __builtin_fmaf(dx, dx, a3); a3 = __builtin_fmaf(dy, dy, a3);
        }
      } else {
        for (uint32_t j = 0; j * 4 < ne; ++j) {                              // single accumulator, one fma per element
          const float4 v = *reinterpret_cast<const float4*>(rowc + ((j ^ (static_cast<uint32_t>(lane) & 15u)) << 4));
          const float* qq = qv + e0 + 4 * j;
          float dd;
          dd = qq[0] - v.x; a0 = __builtin_fmaf(dd, dd, a0);
          dd = qq[1] - v.y; a0 = __builtin_fmaf(dd, dd, a0);
          dd = qq[2] - v.z; a0 = __builtin_fmaf(dd, dd, a0);
          dd = qq[3] - v.w; a0 = __builtin_fmaf(dd, dd, a0);
        }
      }
    }
    const float d = (DT == DT_F16) ? (a0 + a1) + (a2 + a3) : a0;
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
