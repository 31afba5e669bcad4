// kernels_refine_v3_body.h -- body of refine v3 (whole rows through LDS, four lanes per row), included by kernels_refine.h as the body of the product kernel
// (STAMP = false) and of its stamped twin (STAMP = true, option refine_dbg_q).  Not a standalone header: the
// enclosing kernel declares STAMP, dbg_out and dbg_q.
  constexpr int RB = DIM * 2;                       // row bytes
  constexpr int LA = refine3_la<DIM>();             // lanes of piece A (16 bytes each): the whole row up to 1 KB
  constexpr int REM = RB - LA * 16;                 // 0, or 512 for 1536-byte rows: remainder, two rows per piece
  static_assert(DIM % 8 == 0 && (REM == 0 || REM == 512), "rows of up to 1 KB, or of 1536 bytes");
  constexpr int NPAIR = DIM / 8;                    // pairs per lane = 16-byte pieces per row
  constexpr int SLOT = refine3_slot_bytes<DIM>();
  constexpr int ABLOCK = LA * 16 + 16, BBLOCK = 1040;
  constexpr int BOFF = REFINE3_ROWS * ABLOCK;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float lds_d[REFINE3_WAVES][64];
  __shared__ uint32_t lds_id[REFINE3_WAVES][64];
  __shared__ uint32_t lds_cnt[REFINE3_WAVES];
  const uint32_t q = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane >> 2, c = lane & 3;
  const uint32_t* __restrict__ cq = cand + static_cast<uint64_t>(q) * R;
  char* myslot = smem + wave * SLOT;
  const uint32_t lds_mine = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(NVDB_LPTR(myslot)));
  const char* gbase = static_cast<const char*>(rows);
  [[maybe_unused]] const bool stamp = STAMP && q < dbg_q && wave == 0;
  [[maybe_unused]] uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
  if constexpr (STAMP) { if (stamp) t0 = refine_stamp(); }

  // this lane's query elements: pairs c, c + 4, c + 8, ... (two floats each), resident for the whole query
  float2 qv[NPAIR];
  {
    const float2* qp = reinterpret_cast<const float2*>(queries + static_cast<uint64_t>(q) * DIM) + c;
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) qv[i] = qp[4 * i];
  }

  WaveTopKMin tk;
  tk.d = 1e30f; tk.id = 0xFFFFFFFFu; tk.cnt = 0; tk.thr_d = 1e30f; tk.thr_id = 0xFFFFFFFFu;

  const uint32_t voffA = static_cast<uint32_t>(lane) * 16u;                                 // piece A: lane l <- bytes [16 l, 16 l + 16) of the row
  const uint32_t lane_lo = static_cast<uint32_t>(lane & 31) * 16u + LA * 16u;               // piece B: 32 lanes per row, after the A part
  const char* rdA = myslot + r * ABLOCK + c * 4;                                            // this lane's read bases
  const char* rdB = myslot + BOFF + (r & 7) * BBLOCK + (r >> 3) * 512 + c * 4;

  uint32_t idx = wave * REFINE3_ROWS + (lane & 15);
  uint32_t ids_next = (idx < R) ? cq[idx] : 0xFFFFFFFFu;
  for (uint32_t s0 = wave * REFINE3_ROWS; s0 < R; s0 += REFINE3_WAVES * REFINE3_ROWS) {
    const uint32_t ids = ids_next;                  // lanes 0..15 (and their copies in 16..63): candidate of row lane & 15
    idx += REFINE3_WAVES * REFINE3_ROWS;
    ids_next = (idx < R) ? cq[idx] : 0xFFFFFFFFu;   // next step's ids travel while this step's rows do
    // ---- issue: 16 whole rows (rows j and j + 8 together: they share the remainder piece) ----
#pragma unroll
    for (int j = 0; j < REFINE3_ROWS / 2; ++j) {
      const uint32_t sid0 = readlane_u(ids, j), sid1 = readlane_u(ids, j + 8);
      const bool ok0 = (sid0 != 0xFFFFFFFFu) && (static_cast<uint64_t>(sid0) < n);         // cuda_refine.cu:437
      const bool ok1 = (sid1 != 0xFFFFFFFFu) && (static_cast<uint64_t>(sid1) < n);
      const uint64_t off0 = static_cast<uint64_t>(ok0 ? sid0 : 0u) * RB;                   // skipped candidates: row 0, dropped below
      const uint64_t off1 = static_cast<uint64_t>(ok1 ? sid1 : 0u) * RB;
      if (lane < LA) {                               // (all 64 lanes for rows of 1 KB and more); ok0 / ok1: wave-uniform branches
        if (ok0) glds16_imm<0>(voffA, gbase + off0, lds_mine + j * ABLOCK);
        if (ok1) glds16_imm<0>(voffA, gbase + off1, lds_mine + (j + 8) * ABLOCK);
      }
      if constexpr (REM != 0) {
        const uint64_t o = (lane < 32 ? off0 : off1) + lane_lo;                            // the two rows are read by different half-waves
        if (ok0 || ok1) glds16_v(gbase + o, lds_mine + BOFF + j * BBLOCK);
      }
    }
    const uint32_t my_id = static_cast<uint32_t>(__shfl(static_cast<int>(ids), r));
    const bool valid = (my_id != 0xFFFFFFFFu) && (static_cast<uint64_t>(my_id) < n);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // ---- consume: accumulator c of row r ----
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) {
      const char* src = (i < LA) ? rdA + i * 16 : rdB + (i - LA) * 16;
      const uint32_t x = *reinterpret_cast<const uint32_t*>(src);                          // half2 pair (x[2p], x[2p+1])
      const float dx = q_minus_half_lo(x, qv[i].x);
      const float dy = q_minus_half_hi(x, qv[i].y);
      acc = __builtin_fmaf(dx, dx, acc);
      acc = __builtin_fmaf(dy, dy, acc);
    }
    const float s1 = acc + __shfl_xor(acc, 1);      // a0 + a1 | a2 + a3
    const float d = s1 + __shfl_xor(s1, 2);         // (a0 + a1) + (a2 + a3): the same bits in all four lanes
    unsigned long long m = __ballot(valid && c == 0 && wmin_accepts(tk, K, d, my_id));
    while (m) {
      const int L = __builtin_ctzll(m);
      m &= m - 1;
      const float cd = readlane_f(d, L);
      const uint32_t cid = readlane_u(my_id, L);
      if (wmin_accepts(tk, K, cd, cid)) wmin_insert(tk, K, cd, cid, lane);
    }
  }
  if constexpr (STAMP) { if (stamp) t1 = refine_stamp(); }
  lds_d[wave][lane] = tk.d; lds_id[wave][lane] = tk.id;
  if (lane == 0) lds_cnt[wave] = tk.cnt;
  __syncthreads();
  if (wave != 0) return;
  if constexpr (STAMP) { if (stamp) t2 = refine_stamp(); }
  for (int w = 1; w < REFINE3_WAVES; ++w) {
    const uint32_t cn = lds_cnt[w];
    for (uint32_t j = 0; j < cn; ++j) {
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
