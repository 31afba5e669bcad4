// kernels_compact.h -- gfx950 kernels of the in-place compaction (nvdb_hip_compact_rows; orchestration in nvdb_compact.cpp, the
// slab plan in compact_plan.h, DESIGN.md section 4 "Compaction").  A 64-row tile is two words of the plane; the move is stable, so
// the destination of live row r of tile t is rank[t] + popcount(the tile's bits below r).
//   compact_tile_rank_kernel   per block of 1024 tiles: rank[t] = live rows of the block's tiles before t, sums[block] = its total
//   compact_rank_add_kernel    rank[t] += base[t / 1024] (the host's scan of the sums); rank[T] = the plane's live count
//   compact_move_kernel        one workgroup per tile of a slab: the tile's live rows, side by side, to their destination rows
//                              (in the array itself where the slab plan says the ranges do not overlap, else in the bounce buffer).
//                              LaneT is the widest vector the row length guarantees: 16 / 8 / 4 / 2 / 1 bytes; the 4-byte build with
//                              one lane per row moves the scale arrays.  All element offsets are 64-bit.
//   compact_planes_kernel      a thread per (tile, plane): the plane's bits of the tile's live rows, squeezed together, ORed into the
//                              FRESH planes at bit rank[t] (the word stride changes, so never in place); counts each plane's live rows
//   compact_map_kernel         old_rows[new row] = old row
// No kernel reads a byte that the same launch writes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace nvdbhip {

constexpr uint32_t COMPACT_RANK_THREADS = 1024;     // tiles per block of the rank kernels
constexpr uint32_t COMPACT_MOVE_THREADS = 256;
// the mover's 16- and 8-byte lanes: plain vectors (one global_load_dwordx4 / dwordx2 each, held in registers)
typedef uint32_t CompactLane16 __attribute__((ext_vector_type(4)));
typedef uint32_t CompactLane8 __attribute__((ext_vector_type(2)));

// the 64 bits of tile t of a plane of W words (tail bits are 0; the last tile may have one word only)
__device__ __forceinline__ unsigned long long compact_tile_bits(const uint32_t* __restrict__ plane, uint32_t W, uint32_t t) {
  const uint32_t w = 2u * t;
  unsigned long long m = plane[w];
  if (w + 1u < W) m |= static_cast<unsigned long long>(plane[w + 1u]) << 32;
  return m;
}
__device__ __forceinline__ unsigned long long compact_low_mask(uint32_t bits) { return bits >= 64u ? ~0ull : (1ull << bits) - 1ull; }

// grid = ceil(T / 1024), block = 1024
static __global__ __launch_bounds__(COMPACT_RANK_THREADS) void compact_tile_rank_kernel(const uint32_t* __restrict__ plane, uint32_t W, uint32_t T,
                                                                                       uint32_t* __restrict__ rank, uint32_t* __restrict__ sums) {
  __shared__ uint32_t s_tot[COMPACT_RANK_THREADS / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t t = blockIdx.x * COMPACT_RANK_THREADS + tid;
  const uint32_t c = t < T ? static_cast<uint32_t>(__builtin_popcountll(compact_tile_bits(plane, W, t))) : 0u;
  uint32_t inc = c;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(inc, o);
    if (lane >= static_cast<uint32_t>(o)) inc += up;
  }
  if (lane == 63u) s_tot[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  for (uint32_t w = 0; w < wave; ++w) before += s_tot[w];
  if (t < T) rank[t] = before + inc - c;
  if (tid == COMPACT_RANK_THREADS - 1u) sums[blockIdx.x] = before + inc;
}

// grid = ceil((T + 1) / 256), block = 256.  base: one entry per block of the kernel above, then the total
static __global__ __launch_bounds__(256) void compact_rank_add_kernel(uint32_t* __restrict__ rank, uint32_t T, const uint32_t* __restrict__ base, uint32_t nblocks) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < T) rank[t] += base[t / COMPACT_RANK_THREADS];
  else if (t == T) rank[T] = base[nblocks];
}

// grid = tiles of the slab, block = 256.  Tile t0 + blockIdx.x; rows below row_lo (the slab's start, inside tile t0 for the first slab
// of a walk only) are not this launch's.  dst_row0: the destination row that stands at dst[0] (0: dst is the array; the slab's first
// destination row: dst is the bounce buffer).  upr = LaneT units per row.
template <typename LaneT>
static __global__ __launch_bounds__(COMPACT_MOVE_THREADS) void compact_move_kernel(const LaneT* src, LaneT* dst, uint64_t dst_row0,
                                                                                  const uint32_t* __restrict__ plane, uint32_t W,
                                                                                  const uint32_t* __restrict__ rank, uint32_t t0, uint32_t row_lo,
                                                                                  uint32_t upr) {
  __shared__ uint32_t s_row[64];                                       // s_row[j] = the tile's j-th row to move
  const uint32_t tid = threadIdx.x, t = t0 + blockIdx.x;
  const uint64_t tile_row = static_cast<uint64_t>(t) << 6;
  const unsigned long long m = compact_tile_bits(plane, W, t);
  const uint32_t skip = row_lo > tile_row ? static_cast<uint32_t>(row_lo - tile_row) : 0u;
  const unsigned long long mv = m & ~compact_low_mask(skip);
  if (!mv) return;                                                     // (uniform over the workgroup)
  const uint64_t d_first = static_cast<uint64_t>(rank[t]) + static_cast<uint64_t>(__builtin_popcountll(m & compact_low_mask(skip))) - dst_row0;
  if (tid < 64u && ((mv >> tid) & 1ull)) s_row[__builtin_popcountll(mv & compact_low_mask(tid))] = tid;
  __syncthreads();
  const uint32_t L = static_cast<uint32_t>(__builtin_popcountll(mv));
  // unit u = tid, tid + 256, ... of the L * upr units the rows to move hold: row j = u / upr, unit w = u % upr, kept by addition
  uint32_t j = tid / upr, w = tid % upr;
  const uint32_t qs = COMPACT_MOVE_THREADS / upr, rs = COMPACT_MOVE_THREADS % upr;
  while (j < L) {
    LaneT v[4];
    uint64_t d[4];
    bool ok[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
      ok[u] = j < L;
      if (ok[u]) {
        v[u] = src[(tile_row + s_row[j]) * upr + w];
        d[u] = (d_first + j) * upr + w;
      }
      j += qs; w += rs;
      if (w >= upr) { w -= upr; ++j; }
    }
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) if (ok[u]) dst[d[u]] = v[u];
  }
}

// grid = (ceil(T / 256), nmasks), block = 256.  fresh: [nmasks][W2] words, all zero before the launch; live[p] += plane p's live rows
static __global__ __launch_bounds__(256) void compact_planes_kernel(const uint32_t* __restrict__ planes, uint32_t W, uint32_t T, uint32_t mask,
                                                                    const uint32_t* __restrict__ rank, uint32_t* __restrict__ fresh, uint32_t W2,
                                                                    unsigned long long* __restrict__ live) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x, p = blockIdx.y;
  uint32_t kept = 0;
  if (t < T) {
    unsigned long long m = compact_tile_bits(planes + static_cast<uint64_t>(mask) * W, W, t);
    const unsigned long long b = compact_tile_bits(planes + static_cast<uint64_t>(p) * W, W, t) & m;
    unsigned long long out = 0;                                        // bit k = the plane's bit of the tile's k-th live row
    for (uint32_t k = 0; m; ++k, m &= m - 1ull)
      if (b & (m & (0ull - m))) out |= 1ull << k;
    kept = static_cast<uint32_t>(__builtin_popcountll(out));
    if (out) {
      const uint32_t pos = rank[t], sh = pos & 31u;
      const unsigned long long lo = out << sh, hi = sh ? out >> (64u - sh) : 0ull;
      uint32_t* __restrict__ word = fresh + static_cast<uint64_t>(p) * W2 + (pos >> 5);
      const uint32_t piece[3] = {static_cast<uint32_t>(lo), static_cast<uint32_t>(lo >> 32), static_cast<uint32_t>(hi)};
#pragma unroll
      for (uint32_t i = 0; i < 3; ++i) if (piece[i]) atomicOr(word + i, piece[i]);   // (a set bit names a new row: inside the plane)
    }
  }
  for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
  if ((threadIdx.x & 63u) == 0u && kept) atomicAdd(live + p, static_cast<unsigned long long>(kept));
}

// grid = ceil(T / 4), block = 256: a wave per tile, a lane per row
static __global__ __launch_bounds__(256) void compact_map_kernel(const uint32_t* __restrict__ plane, uint32_t W, uint32_t T, const uint32_t* __restrict__ rank,
                                                                 uint32_t* __restrict__ old_rows) {
  const uint32_t lane = threadIdx.x & 63u, t = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (t >= T) return;
  const unsigned long long m = compact_tile_bits(plane, W, t);
  if ((m >> lane) & 1ull) old_rows[static_cast<uint64_t>(rank[t]) + static_cast<uint64_t>(__builtin_popcountll(m & compact_low_mask(lane)))] = (t << 6) + lane;
}

}  // namespace nvdbhip
