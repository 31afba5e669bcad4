// kernels_masked_topk.h -- gfx950 kernels of the masked flat top-k on the MFMA filter route (nvdb_hip_search_batch_masked;
// orchestration in nvdb_masked_flat.cpp, DESIGN.md section 4 "Row masks").  The route's heavy steps are existing kernels -- the
// masked partition scan over a bootstrap prefix, the filter stream at fixed thresholds, the rescore, the masked keep step --; what
// is here joins them:
//   masked_prefix_rank_kernel   one workgroup per distinct plane of a sub-batch: the plane's live count against L (masked_plan.h),
//                               the prefix P = the smallest multiple of 64 rows (or n) that holds L live rows, and the plane's
//                               bootstrap work items cut over [0, P).  A popcount descent: the region that holds the L-th live row is
//                               split sixteen ways, one wave per part, until it fits one wave's lanes.  No atomics; the result does
//                               not depend on timing.
//   masked_bar_kernel           radius[q] = the query's k-th bootstrap score (an exact score of a live row), NaN where the
//                               bootstrap found fewer than k live rows, or the plane holds too few for a bar (mp_boot_final): then
//                               the prefix was the corpus and the bootstrap's result is final
//   masked_topk_from_kept_kernel  the first min(k, kept) entries of a query's kept list -> ids / scores / count, padded
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_partitions.h"
#include "masked_plan.h"

namespace nvdbhip {

constexpr uint32_t MASKED_RANK_THREADS = 1024;
constexpr uint32_t MASKED_RANK_WAVES = MASKED_RANK_THREADS / 64;

// one distinct plane of a sub-batch: its number (0xFFFFFFFF: no mask) and the segments each of its query groups' prefix is cut into
struct MaskedSlot { uint32_t mask, nseg; };

// live rows of 64-row tile t of a plane of W words (tail bits are 0)
__device__ __forceinline__ uint32_t masked_tile_live(const uint32_t* __restrict__ plane, uint32_t W, uint32_t t) {
  const uint32_t w = 2u * t;
  uint32_t c = static_cast<uint32_t>(__builtin_popcount(plane[w]));
  if (w + 1u < W) c += static_cast<uint32_t>(__builtin_popcount(plane[w + 1u]));
  return c;
}

// grid = distinct planes of the sub-batch, block = 1024.  items: the work list's items as the host staged them -- an item whose pad is
// slot + 1 is a TEMPLATE of that slot: row_lo = its segment number, row_hi = the segment count; this kernel turns it into rows
// (an item whose segment is empty -- a prefix of fewer tiles than segments -- becomes an idle item: one tile, no queries).
static __global__ __launch_bounds__(MASKED_RANK_THREADS) void masked_prefix_rank_kernel(
    const uint32_t* __restrict__ planes, uint32_t W, uint32_t n, uint32_t k, uint32_t cap, const MaskedSlot* __restrict__ slots,
    PartItem* __restrict__ items, uint32_t nitems, uint32_t* __restrict__ prefix_out, uint32_t* __restrict__ final_out) {
  __shared__ uint32_t s_tot[MASKED_RANK_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const MaskedSlot slot = slots[blockIdx.x];
  uint32_t P = n;                                                      // uniform over the workgroup
  uint32_t live = n;
  if (slot.mask == 0xFFFFFFFFu) {
    P = static_cast<uint32_t>(mp_prefix_unmasked(n, k, cap));
  } else {
    const uint32_t* __restrict__ plane = planes + static_cast<uint64_t>(slot.mask) * W;
    uint32_t lo = 0, len = (n + 63u) >> 6;                             // the region of tiles that holds the target-th live row
    uint32_t before = 0, target = 0;                                   // live rows in tiles [0, lo); the rank looked for (1-based)
    bool first = true, whole = false;
    while (first || len > 64u) {
      const uint32_t part = (len + MASKED_RANK_WAVES - 1u) / MASKED_RANK_WAVES, end = lo + len;
      const uint32_t my_lo = lo + wave * part;
      const uint32_t my_hi = my_lo + part < end ? my_lo + part : end;
      uint32_t sum = 0;
      for (uint32_t t = my_lo + lane; t < my_hi; t += 64u) sum += masked_tile_live(plane, W, t);
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      if (lane == 0) s_tot[wave] = sum;
      __syncthreads();
      uint32_t tot[MASKED_RANK_WAVES], all = 0;
#pragma unroll
      for (uint32_t w = 0; w < MASKED_RANK_WAVES; ++w) { tot[w] = s_tot[w]; all += tot[w]; }
      __syncthreads();                                                 // (the totals are read before the next round writes them)
      if (first) {
        const uint64_t L = mp_boot_live(k, cap, n);
        first = false;
        live = all;
        if (all < L) { whole = true; break; }                          // fewer live rows than the sample wants: the prefix is the corpus
        target = static_cast<uint32_t>(L);
      }
      // the part that holds the target: before + (totals up to and including it) >= target for the first time
      uint32_t pick = MASKED_RANK_WAVES - 1u, run = before, run_at = before;
      bool found = false;
#pragma unroll
      for (uint32_t w = 0; w < MASKED_RANK_WAVES; ++w) {
        if (!found && run + tot[w] >= target) { found = true; pick = w; run_at = run; }
        run += tot[w];
      }
      before = run_at;
      const uint32_t nlo = lo + pick * part;
      len = nlo + part < end ? part : end - nlo;
      lo = nlo;
    }
    if (!whole) {
      // the region fits a wave: a lane per tile, an inclusive scan, the first lane that reaches the target (every wave alike)
      const uint32_t t = lo + lane;
      uint32_t inc = lane < len ? masked_tile_live(plane, W, t) : 0u;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= static_cast<uint32_t>(o)) inc += up;
      }
      const unsigned long long reach = __ballot(lane < len && before + inc >= target);
      const uint32_t f = reach ? static_cast<uint32_t>(__builtin_ctzll(reach)) : (len - 1u);
      P = static_cast<uint32_t>(mp_prefix_end(n, static_cast<uint64_t>(lo) + f));
    }
  }
  if (tid == 0) {
    prefix_out[blockIdx.x] = P;
    final_out[blockIdx.x] = mp_boot_final(k, live) ? 1u : 0u;         // (then P == n: the bootstrap sees every live row)
  }
  for (uint32_t i = tid; i < nitems; i += MASKED_RANK_THREADS) {
    PartItem it = items[i];
    if (it.pad != blockIdx.x + 1u) continue;
    uint32_t a, b;
    mp_segment(P, it.row_lo, it.row_hi, &a, &b);
    if (a < b) { it.row_lo = a; it.row_hi = b; }
    else { it.row_lo = 0u; it.row_hi = n < 64u ? n : 64u; it.nqg = 0u; }
    items[i] = it;
  }
}

// grid = ceil(nq / 256), block = 256
static __global__ __launch_bounds__(256) void masked_bar_kernel(const float* __restrict__ boot_scores, const uint32_t* __restrict__ boot_counts,
                                                                const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ slot_final,
                                                                uint32_t k, uint32_t nq, float* __restrict__ radius) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= nq) return;
  const bool bar = boot_counts[q] == k && slot_final[slot_of[q]] == 0u;
  radius[q] = bar ? boot_scores[static_cast<uint64_t>(q) * k + (k - 1u)] : __builtin_nanf("");
}

// grid = nq, block = 64.  The kept lists are ordered (score desc, row asc) by the keep step.  Queries the bootstrap answered
// (their radius is NaN, so overflow[q] is set) and flagged queries (overflow[q]) keep what the bootstrap's select wrote; the host
// redoes the flagged ones.
static __global__ __launch_bounds__(64) void masked_topk_from_kept_kernel(const Cand* __restrict__ cand, uint32_t cap, const uint32_t* __restrict__ kept,
                                                                          const uint32_t* __restrict__ overflow, uint32_t k, uint64_t row_base,
                                                                          unsigned long long* __restrict__ out_ids, float* __restrict__ out_scores,
                                                                          uint32_t* __restrict__ counts) {
  const uint32_t q = blockIdx.x, lane = threadIdx.x;
  if (counts[q] < k || overflow[q] != 0u) return;
  const uint32_t have = kept[q] < cap ? kept[q] : cap;
  const uint32_t m = have < k ? have : k;
  if (lane < k) {
    Cand c = Cand{NEG_INF, 0xFFFFFFFFu};
    if (lane < m) c = cand[static_cast<uint64_t>(q) * cap + lane];
    out_ids[static_cast<uint64_t>(q) * k + lane] = lane < m ? row_base + c.row : ~0ull;
    out_scores[static_cast<uint64_t>(q) * k + lane] = lane < m ? c.score : NEG_INF;
  }
  if (lane == 0) counts[q] = m;
}

}  // namespace nvdbhip
