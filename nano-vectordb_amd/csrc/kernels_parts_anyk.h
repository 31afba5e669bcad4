// kernels_parts_anyk.h -- gfx950 kernels of the probe search for any k (nvdb_hip_search_partitions_anyk / _ivf_anyk; orchestration
// in nvdb_parts_anyk.cpp, DESIGN.md section 4 "probe search, any k").
//
// The scan is the range search's (range_parts_kernel, kernels_range_parts.h) with every radius -inf: a query's candidate block
// cand[cbeg[q] .. cbeg[q + 1]) then holds every live row of its probed union as Cand{score, row}, the non-padding entries
// ascending with the row, so that a position inside the block is a valid id tie-break.
//
//  * parts_anyk_select_kernel : one workgroup per query.  Counts the non-padding entries c (out_counts = min(k, c)); for c > k an
//                               8-bit radix select over key64_of(score, position) finds the k-th largest key -- the histogram in
//                               LDS, every pass inside the kernel, from the top byte down until the bucket of the k-th key is
//                               taken whole (keys are distinct: after the last byte at the latest); collects the keys >= that key
//                               into a slab of K2 = pa_slab_len(k, block length) entries (parts_anyk_plan.h).  K2 <= PA_LDS_KEYS:
//                               the slab is LDS, sorted there (the network of bitonic_lds_kernel) and emitted -- global ids, and
//                               the scores' original bits from the block entry at the key's position (score_key folds -0.0 into
//                               +0.0).  Longer slabs are written to global memory for bitonic_global_step_kernel (kernels_largek.h).
//  * parts_anyk_emit_kernel   : ... and emitted from there once they are sorted.
// Rows beyond a query's count are padded with id UINT64_MAX / -inf by the select kernel on both routes.
// Blocks of any length below 2^32 entries: one workgroup loops over its block (once to count, once per radix pass, once to collect).
#pragma once
#include "kernels_range_parts.h"
#include "parts_anyk_plan.h"

namespace nvdbhip {

constexpr uint32_t PA_THREADS = 256;
constexpr uint32_t PA_LDS_HEAD = 256 * 4 + 64;     // the histogram and 16 words of workgroup state in front of the key slab (a multiple of 16)

// histogram add of one wave step.  The scores of a block share their top bytes, so the first passes hit a few counters: up to
// four rounds in which the lanes that share the first remaining lane's digit add their number at once, then whoever is left
// adds alone.  Called by whole waves (in: the lane has a key of this pass).
__device__ __forceinline__ void pa_hist_add(uint32_t* hist, bool in, uint32_t digit, uint32_t lane) {
  unsigned long long left = __ballot(in);
#pragma unroll 1
  for (int round = 0; round < 4 && left; ++round) {
    const int first = __builtin_ctzll(left);
    const uint32_t d0 = readlane_u(digit, first);
    const unsigned long long same = __ballot(in && digit == d0) & left;
    if (lane == static_cast<uint32_t>(first)) atomicAdd(&hist[d0], static_cast<uint32_t>(__builtin_popcountll(same)));
    left &= ~same;
  }
  if ((left >> lane) & 1ull) atomicAdd(&hist[digit], 1u);
}

// grid = queries of the launch set, block = PA_THREADS, dynamic LDS = PA_LDS_HEAD + (the longest LDS slab of the launch set) * 8.
// out_k = entries per output row (>= min(k, c) of every query); slab_off[q][2] = (lo, hi) of the query's first key in `slab`
// (read for long slabs only); raw_counts[q] = c.
static __global__ __launch_bounds__(PA_THREADS) void parts_anyk_select_kernel(
    const Cand* __restrict__ cand, const uint32_t* __restrict__ cbeg, uint32_t k, uint32_t out_k, uint64_t row_base,
    const uint32_t* __restrict__ slab_off, unsigned long long* __restrict__ slab, unsigned long long* __restrict__ out_ids,
    float* __restrict__ out_scores, uint32_t* __restrict__ out_counts, uint32_t* __restrict__ raw_counts) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem_raw);
  uint32_t* state = hist + 256;                    // [0..3] per-wave sums, [4] digit, [5] rank left, [6] bucket size, [7] keys taken
  unsigned long long* lds_keys = reinterpret_cast<unsigned long long*>(smem_raw + PA_LDS_HEAD);
  const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint32_t len = cbeg[q + 1] - cbeg[q];
  const Cand* __restrict__ blk = cand + cbeg[q];
  unsigned long long* my_ids = out_ids + static_cast<uint64_t>(q) * out_k;
  float* my_scores = out_scores + static_cast<uint64_t>(q) * out_k;

  // 1. the non-padding entries
  uint32_t mine = 0;
  for (uint64_t i = tid; i < len; i += PA_THREADS) mine += blk[i].row != 0xFFFFFFFFu ? 1u : 0u;
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if (lane == 0) state[wave] = mine;
  if (tid == 0) state[7] = 0u;
  __syncthreads();
  const uint32_t c = state[0] + state[1] + state[2] + state[3];
  const uint32_t k_eff = c < k ? c : k;
  if (tid == 0) { out_counts[q] = k_eff; raw_counts[q] = c; }
  const uint64_t K2 = pa_slab_len(k, len);          // (k_eff <= min(k, len) <= K2)
  const bool in_lds = !pa_slab_is_long(K2);
  if (!in_lds || k_eff == 0)
    for (uint32_t j = k_eff + tid; j < out_k; j += PA_THREADS) { my_ids[j] = ~0ull; my_scores[j] = NEG_INF; }
  if (K2 == 0) return;                             // an empty block (uniform)
  __syncthreads();                                 // (state[0..3] are rewritten below)

  // 2. the k-th largest key; 0: every entry is taken
  unsigned long long kth = 0ull;
  if (c > k) {
    unsigned long long prefix = 0ull;
    uint32_t krem = k;
#pragma unroll 1
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      hist[tid] = 0u;
      __syncthreads();
      for (uint64_t w0 = wave * 64u; w0 < len; w0 += PA_THREADS) {       // (wave-uniform bounds: the ballots see whole waves)
        const uint64_t i = w0 + lane;
        bool in = false;
        uint32_t digit = 0u;
        if (i < len) {
          const Cand e = blk[i];
          if (e.row != 0xFFFFFFFFu) {
            const unsigned long long key = key64_of(e.score, static_cast<uint32_t>(i));
            in = pass == 0 || (key >> (shift + 8)) == prefix;
            digit = static_cast<uint32_t>(key >> shift) & 255u;
          }
        }
        pa_hist_add(hist, in, digit, lane);
      }
      __syncthreads();
      // thread t owns digit 255 - t: an inclusive scan over t counts the keys of this pass whose digit is >= its own
      const uint32_t v = hist[255u - tid];
      uint32_t inc = v;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= static_cast<uint32_t>(o)) inc += up;
      }
      if (lane == 63u) state[wave] = inc;
      __syncthreads();
      uint32_t above = inc - v;
      for (uint32_t w = 0; w < wave; ++w) above += state[w];
      if (above < krem && krem <= above + v) { state[4] = 255u - tid; state[5] = krem - above; state[6] = v; }   // exactly one digit (1 <= krem <= keys of the pass)
      __syncthreads();
      prefix = (prefix << 8) | state[4];
      krem = state[5];
      if (krem == state[6]) { kth = prefix << shift; break; }          // the bucket is taken whole: every key >= its smallest possible member
    }
  }

  // 3. the keys >= kth, in any order; the rest of the slab is key 0 (below every real key: ~position is never 0)
  unsigned long long* keys = lds_keys;
  if (!in_lds) keys = slab + ((static_cast<unsigned long long>(slab_off[2 * q + 1]) << 32) | slab_off[2 * q]);
  for (uint64_t w0 = wave * 64u; w0 < len; w0 += PA_THREADS) {
    const uint64_t i = w0 + lane;
    bool take = false;
    unsigned long long key = 0ull;
    if (i < len) {
      const Cand e = blk[i];
      key = key64_of(e.score, static_cast<uint32_t>(i));
      take = e.row != 0xFFFFFFFFu && key >= kth;
    }
    const unsigned long long bal = __ballot(take);
    if (bal == 0ull) continue;
    uint32_t slot = 0;
    if (lane == 0) slot = atomicAdd(&state[7], static_cast<uint32_t>(__builtin_popcountll(bal)));
    slot = readlane_u(slot, 0);
    const uint64_t p = static_cast<uint64_t>(slot) + static_cast<uint32_t>(__builtin_popcountll(bal & below));
    if (take && p < K2) keys[p] = key;
  }
  __syncthreads();
  const uint64_t taken = state[7] < K2 ? state[7] : K2;
  for (uint64_t j = taken + tid; j < K2; j += PA_THREADS) keys[j] = 0ull;
  if (!in_lds) return;                             // sorted and emitted by the launches that follow
  __syncthreads();

  // 4. sort descending in LDS, emit
  const uint32_t n2 = static_cast<uint32_t>(K2);
  for (uint32_t size = 2; size <= n2; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t i = tid; i < (n2 >> 1); i += PA_THREADS) {
        const uint32_t a = 2 * i - (i & (stride - 1)), b = a + stride;
        const bool desc = ((a & size) == 0);
        const unsigned long long ea = lds_keys[a], eb = lds_keys[b];
        if ((eb > ea) == desc) { lds_keys[a] = eb; lds_keys[b] = ea; }
      }
      __syncthreads();
    }
  for (uint32_t j = tid; j < out_k; j += PA_THREADS) {
    if (j < k_eff) {
      const uint32_t pos = ~static_cast<uint32_t>(lds_keys[j]);
      const Cand e = blk[pos < len ? pos : len - 1u];                  // (every key is a position < len: the read stays inside the block whatever the slab holds)
      my_ids[j] = row_base + e.row;
      my_scores[j] = e.score;
    } else {
      my_ids[j] = ~0ull;
      my_scores[j] = NEG_INF;
    }
  }
}

// grid = (ceil(out_k / 256), long lists), block = 256: entry j < counts[q] of a sorted long slab
static __global__ __launch_bounds__(256) void parts_anyk_emit_kernel(const unsigned long long* __restrict__ slab, const PaLong* __restrict__ longs,
                                                                     const Cand* __restrict__ cand, const uint32_t* __restrict__ cbeg,
                                                                     const uint32_t* __restrict__ counts, uint32_t out_k, uint64_t row_base,
                                                                     unsigned long long* __restrict__ out_ids, float* __restrict__ out_scores) {
  const PaLong d = longs[blockIdx.y];
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= counts[d.q] || j >= out_k) return;
  const uint32_t len = cbeg[d.q + 1] - cbeg[d.q];                          // (>= the count >= 1)
  const uint32_t pos = ~static_cast<uint32_t>(slab[((static_cast<unsigned long long>(d.off_hi) << 32) | d.off_lo) + j]);
  const Cand e = cand[static_cast<uint64_t>(cbeg[d.q]) + (pos < len ? pos : len - 1u)];
  out_ids[static_cast<uint64_t>(d.q) * out_k + j] = row_base + e.row;
  out_scores[static_cast<uint64_t>(d.q) * out_k + j] = e.score;
}

}  // namespace nvdbhip
