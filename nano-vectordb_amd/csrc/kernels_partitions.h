// kernels_partitions.h -- gfx950 kernels of the partitioned probe search (nvdb_hip_search_partitions / nvdb_hip_search_ivf).
//
//  * part_walk           : the walk over one work item = (a segment of contiguous rows, a group of <= PART_WAVES*QW queries that
//                          all probe the partition the segment belongs to), one workgroup per item.  The queries are gathered BY
//                          INDEX into LDS once; the segment is walked in tiles of 64 rows; one lane = one row (the reference
//                          order of exact_scores<> is a strict chain over the row); the waves score the SAME 64 rows, each
//                          against its own QW queries, so a wave owns its queries' results outright and nothing is merged
//                          across waves.  What happens to a scored row is a SINK's business (below).
//                          STAGED: the tile's rows are contiguous bytes -- the workgroup fetches them with coalesced 16-byte
//                          global loads (the next tile's loads are in flight, in registers, while this tile is scored), stores
//                          them into LDS at a row pitch that is an ODD number of 16-byte slots, and every lane reads its row
//                          back with conflict-free ds_read_b128.  Otherwise (rows that are no multiple of 16 bytes, or too long
//                          for the LDS) the lanes read their rows from global memory directly.
//                          MASKED: every query of the group searches under a row mask (a bit plane over the corpus, bit r = local
//                          row r is live; PartMask): a lane tests its own row's bit per owned query and a dead row is never
//                          offered.  A tile's mask words (at most three per query) are loaded one tile ahead by 4 lanes per
//                          query, so the score chain hides them, and handed to the rows' lanes by a lane permute; a wave none of
//                          whose lanes has a live row for any of its queries skips the tile's scores.
//  * scan_parts_kernel   : part_walk with the top-k sink (PartTopKSink): a wave-wide list of the k best per owned query.  Each
//                          (item, query) owns a slot of min(k, segment rows) Cand entries that the host placed: no atomics,
//                          no counters, no overflow path.  (The range scan is the same walk with an append sink:
//                          range_parts_kernel, kernels_range_parts.h.)
//  * select_parts_kernel : one wave per query reduces the query's slots to the k best by (score desc, row asc), adds the global
//                          row base and pads; given a count pointer it stores how many entries the query has (masked searches:
//                          the host cannot derive min(k, live rows) from the partition sizes).
//  * update_row_mask_kernel : one thread per listed row sets or clears the row's bit in a plane (the tombstone path).
//
// Scores: exact_scores<> of kernels_exact.h, i.e. the bits of nvdb_hip_search_batch.  Non-finite scores: no fault, no hang,
// order unspecified.
#pragma once
#include "kernels_exact.h"
#include "parts_worklist.h"   // PartItem, PART_WAVES, PART_QW_MAX, PART_SEG_ROWS: what the host-side list builder shares with the kernels

namespace nvdbhip {

constexpr uint32_t PART_TILE_ROWS = 64;        // rows per tile = lanes per wave
constexpr uint32_t PART_THREADS = 64 * PART_WAVES;
constexpr uint32_t PART_STAGE_MAX_ROW_BYTES = 1536;
constexpr uint32_t PART_MAX_CHUNKS = PART_TILE_ROWS * PART_STAGE_MAX_ROW_BYTES / 16u / PART_THREADS;   // 16-byte chunks of a tile one thread prefetches

// MASKED builds: mask_of[q] = the plane query q searches under (0xFFFFFFFF: none, every row live), planes = [nmasks][W] words,
// local row r live in plane m iff bit r & 31 of word m * W + (r >> 5).  Unmasked builds ignore it.
struct PartMask { const uint32_t* mask_of; const uint32_t* planes; uint32_t W; };

// The mask words of the tile that starts at row T, for a wave's QW queries in ONE register: lane 4 * g + j (j < 3) holds word
// (T >> 5) + j of query g's plane -- a tile of 64 rows starts anywhere, so it touches at most three words -- clamped to the
// word of the segment's last row (the index stays inside the plane).  mid[g]: query g's plane, wave-uniform (0xFFFFFFFF: none,
// the word reads as all ones).
template <int QW>
__device__ __forceinline__ uint32_t part_mask_words(const PartMask& mk, const uint32_t (&mid)[QW], uint32_t T, uint32_t row_hi, int lane) {
  asm volatile("" : "+v"(lane));   // recomputed per tile: hoisted out of the tile loop, the lane's plane address cost the f32 QW = 4 build registers it does not have
  uint32_t lmid = 0xFFFFFFFFu;
#pragma unroll
  for (int g = 0; g < QW; ++g)
    if ((lane >> 2) == g && (lane & 3) < 3) lmid = mid[g];
  const uint32_t wi = (T >> 5) + (static_cast<uint32_t>(lane) & 3u), wmax = (row_hi - 1u) >> 5;
  return lmid == 0xFFFFFFFFu ? 0xFFFFFFFFu : mk.planes[static_cast<uint64_t>(lmid) * mk.W + (wi < wmax ? wi : wmax)];
}

// LDS row pitch of a staged tile: the smallest odd multiple of 16 bytes >= row_bytes.  A ds_read_b128 is served in groups of 16
// lanes whose lane numbers cover every residue mod 16; with an odd pitch (in 16-byte slots) lane L's slot is L * pitch mod 16,
// a bijection of the residues: the 16 lanes of a group touch 16 different 16-byte slots of the 256-byte bank window.
__host__ __device__ inline uint32_t part_pitch(uint32_t row_bytes) { return ((row_bytes >> 4) | 1u) << 4; }

// The walk over one work item, shared by the probe search's scan (scan_parts_kernel, below) and the range scan
// (range_parts_kernel, kernels_range_parts.h): the query gather, the staging of the tiles, the mask words, the tile loop and the
// scores.  What happens to a scored row is the SINK's business:
//   Sink::PerQuery                    what a wave keeps per owned query: wave-uniform values or a wave-wide list (a wave owns its
//                                     queries outright)
//   sink.open(pq, qi, dslot)          once per owned query: qi = the query's number, dst[dslot] = its (item, query) slot (wave
//                                     slots beyond the group repeat the group's first query; nothing is ever kept for them)
//   sink.row(pq, pass, score, row, lane)  once per scored tile and owned query, by every lane: pass = the lane's row exists, the
//                                     query is one of the group's and the row is live in its mask
//   sink.close(pq, seg, dslot, lane)  after the last tile, for the group's queries only: seg = the segment's rows
template <int DT, int QW, bool ALIGNED, bool STAGED, bool MASKED, class Sink>
__device__ __forceinline__ void part_walk(const void* rows, const float* scales, uint32_t dim, const PartItem* items,
                                          const uint32_t* qidx, const float* q32, const PartMask& mk, const Sink& sink) {
  constexpr uint32_t BPE = (DT == DT_F32) ? 4 : (DT == DT_F16 ? 2 : 1);
  constexpr uint32_t QG = PART_WAVES * QW;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const PartItem it = items[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  const int lane = tid & 63;
  const uint32_t wave = tid >> 6;
  const uint32_t qstride = (dim + 3u) & ~3u;
  float* q_lds = reinterpret_cast<float*>(smem_raw);                     // [QG][qstride]
  char* tile = smem_raw + static_cast<size_t>(QG) * qstride * 4;         // STAGED: [64][pitch]

  // gather the group's queries by index; slots beyond the group repeat its first query (scored, never kept)
  for (uint32_t g = 0; g < QG; ++g) {
    const uint32_t qi = qidx[it.qoff + (g < it.nqg ? g : 0u)];
    const float* src = q32 + static_cast<uint64_t>(qi) * dim;
    for (uint32_t j = tid; j < qstride; j += PART_THREADS) q_lds[g * qstride + j] = (j < dim) ? src[j] : 0.f;
  }

  const uint32_t row_bytes = dim * BPE;
  const uint32_t pitch = part_pitch(row_bytes), cpr = row_bytes >> 4;     // (STAGED) 16-byte chunks per row
  // chunk c of a tile = tid + PART_THREADS * i: global address tile_base + 16 * c (the rows are contiguous), LDS row c / cpr, slot c % cpr
  const uint32_t r_step = PART_THREADS / (cpr ? cpr : 1u), ch_step = PART_THREADS % (cpr ? cpr : 1u);
  uint4 pre[PART_MAX_CHUNKS];
  // (macros, not lambdas: behind a closure the array stayed in scratch memory)
  // issue the loads of the tile that starts at row T
#define NVDB_PART_FETCH(T)                                                                                                     \
  {                                                                                                                            \
    const uint32_t nrows_ = (it.row_hi - (T) < PART_TILE_ROWS) ? it.row_hi - (T) : PART_TILE_ROWS;                             \
    const uint32_t nch_ = nrows_ * cpr;                                                                                        \
    const uint4* src_ = reinterpret_cast<const uint4*>(static_cast<const char*>(rows) + static_cast<uint64_t>(T) * row_bytes); \
    _Pragma("unroll") for (uint32_t i_ = 0; i_ < PART_MAX_CHUNKS; ++i_) {                                                      \
      const uint32_t c_ = tid + PART_THREADS * i_;                                                                             \
      pre[i_] = (c_ < nch_) ? src_[c_] : uint4{0u, 0u, 0u, 0u};                                                                \
    }                                                                                                                          \
  }
  // ... and put them into the LDS tile
#define NVDB_PART_STASH(T)                                                                                                     \
  {                                                                                                                            \
    const uint32_t nrows_ = (it.row_hi - (T) < PART_TILE_ROWS) ? it.row_hi - (T) : PART_TILE_ROWS;                             \
    const uint32_t nch_ = nrows_ * cpr;                                                                                        \
    uint32_t r_ = tid / cpr, ch_ = tid % cpr;                                                                                  \
    _Pragma("unroll") for (uint32_t i_ = 0; i_ < PART_MAX_CHUNKS; ++i_) {                                                      \
      const uint32_t c_ = tid + PART_THREADS * i_;                                                                             \
      if (c_ < nch_) *reinterpret_cast<uint4*>(tile + r_ * pitch + ch_ * 16u) = pre[i_];                                       \
      r_ += r_step; ch_ += ch_step;                                                                                            \
      if (ch_ >= cpr) { ch_ -= cpr; ++r_; }                                                                                    \
    }                                                                                                                          \
  }
  const bool wave_live = wave * QW < it.nqg;                               // this wave owns at least one query of the group
  // this wave's queries, gathered by index like the query vectors (slots beyond the group repeat its first query's): the sink's
  // per-query state and, MASKED, the mask numbers (scalar registers) and the first tile's mask words (part_mask_words)
  typename Sink::PerQuery sq[QW];
  [[maybe_unused]] uint32_t mid[QW], wcur = 0u;
#pragma unroll
  for (int g = 0; g < QW; ++g) {
    const uint32_t gi = wave * QW + g, gc = gi < it.nqg ? gi : 0u;
    const uint32_t qi = qidx[it.qoff + gc];
    sink.open(sq[g], qi, it.doff + gc);
    if constexpr (MASKED) mid[g] = __builtin_amdgcn_readfirstlane(mk.mask_of[qi]);
  }
  if constexpr (MASKED) {
    if (wave_live) wcur = part_mask_words<QW>(mk, mid, it.row_lo, it.row_hi, lane);
  }
  if constexpr (STAGED) { NVDB_PART_FETCH(it.row_lo) NVDB_PART_STASH(it.row_lo) }
  __syncthreads();

  const float* qptr = q_lds + wave * QW * qstride;
  // per tile: issue the next tile's loads, score this tile, barrier, stash, barrier
  for (uint32_t t_lo = it.row_lo; t_lo < it.row_hi; t_lo += PART_TILE_ROWS) {
    const bool more = t_lo + PART_TILE_ROWS < it.row_hi;
    if constexpr (STAGED) { if (more) NVDB_PART_FETCH(t_lo + PART_TILE_ROWS) }
    if (wave_live) {
      const uint32_t row = t_lo + lane;
      const bool valid = row < it.row_hi;
      const uint32_t rrow = valid ? row : (it.row_hi - 1);
      [[maybe_unused]] uint32_t wnext = 0u;
      uint32_t live = 0xFFFFFFFFu;                                         // bit g: this lane's row is offered to query g
      if constexpr (MASKED) {
        if (more) wnext = part_mask_words<QW>(mk, mid, t_lo + PART_TILE_ROWS, it.row_hi, lane);   // in flight while this tile is scored
        live = 0u;
        const int j = static_cast<int>((rrow >> 5) - (t_lo >> 5));         // which of the tile's words holds this lane's row: 0 .. 2
#pragma unroll
        for (int g = 0; g < QW; ++g) {
          const uint32_t w = static_cast<uint32_t>(__shfl(static_cast<int>(wcur), 4 * g + j));
          if (valid && wave * QW + g < it.nqg) live |= ((w >> (rrow & 31u)) & 1u) << g;
        }
      }
      if (!MASKED || __any(live != 0u)) {                                  // (uniform over the wave) a tile without a live row: no scores
        const float scale = (DT == DT_I8) ? scales[rrow] : 1.f;
        float sc[QW];
        if constexpr (STAGED) exact_scores<DT, QW, ALIGNED>(tile + static_cast<uint32_t>(lane) * pitch, qptr, qstride, dim, scale, sc);
        else exact_scores<DT, QW, ALIGNED>(row_ptr<DT>(rows, rrow, dim), qptr, qstride, dim, scale, sc);
#pragma unroll
        for (int g = 0; g < QW; ++g) sink.row(sq[g], valid && wave * QW + g < it.nqg && ((live >> g) & 1u), sc[g], row, lane);
      }
      if constexpr (MASKED) wcur = wnext;
    }
    if constexpr (STAGED) {
      if (more) {                                                          // (uniform over the workgroup)
        __syncthreads();                                                   // every wave has read this tile
        NVDB_PART_STASH(t_lo + PART_TILE_ROWS)
        __syncthreads();
      }
    }
  }
  const uint32_t seg = it.row_hi - it.row_lo;
#pragma unroll
  for (int g = 0; g < QW; ++g)
    if (wave * QW + g < it.nqg) sink.close(sq[g], seg, it.doff + wave * QW + g, lane);
}

#undef NVDB_PART_FETCH
#undef NVDB_PART_STASH

// The top-k sink: a wave-wide list of the k best per owned query; at the end min(k, segment rows) entries per (item, query) go
// to the slot the host placed (every row was offered, so a list that is not full is padded).
struct PartTopKSink {
  using PerQuery = WaveTopK;
  const uint32_t* __restrict__ dst;
  Cand* __restrict__ cand;
  uint32_t k;
  __device__ __forceinline__ void open(WaveTopK& tk, uint32_t, uint32_t) const { wtk_init(tk); }
  __device__ __forceinline__ void row(WaveTopK& tk, bool pass, float sc, uint32_t row, int lane) const {
    wtk_offer(tk, k, pass && wtk_accepts(tk, k, sc, row), sc, row, lane);
  }
  __device__ __forceinline__ void close(const WaveTopK& tk, uint32_t seg, uint32_t dslot, int lane) const {
    if (static_cast<uint32_t>(lane) < (seg < k ? seg : k))
      cand[static_cast<uint64_t>(dst[dslot]) + lane] = (static_cast<uint32_t>(lane) < tk.cnt) ? Cand{tk.s, tk.id} : Cand{NEG_INF, 0xFFFFFFFFu};
  }
};

template <int DT, int QW, bool ALIGNED, bool STAGED, bool MASKED>
__global__ __launch_bounds__(PART_THREADS) void scan_parts_kernel(
    const void* __restrict__ rows, const float* __restrict__ scales, uint32_t dim, const PartItem* __restrict__ items,
    const uint32_t* __restrict__ qidx, const uint32_t* __restrict__ dst, const float* __restrict__ q32, uint32_t k,
    Cand* __restrict__ cand, PartMask mk) {
  const PartTopKSink sink{dst, cand, k};
  part_walk<DT, QW, ALIGNED, STAGED, MASKED>(rows, scales, dim, items, qidx, q32, mk, sink);
}

// grid = nq, block = 64: the query's slots are cand[cbeg[q] .. cbeg[q+1])
static __global__ __launch_bounds__(64) void select_parts_kernel(
    const Cand* __restrict__ cand, const uint32_t* __restrict__ cbeg, uint32_t k, uint64_t row_base,
    unsigned long long* __restrict__ out_ids, float* __restrict__ out_scores, uint32_t* __restrict__ out_counts) {
  const uint32_t q = blockIdx.x;
  const int lane = threadIdx.x;
  const uint32_t lo = cbeg[q], hi = cbeg[q + 1];
  WaveTopK tk;
  wtk_init(tk);
  for (uint32_t base = lo; base < hi; base += 64) {
    const uint32_t i = base + lane;
    const bool have = i < hi;
    const Cand c = have ? cand[i] : Cand{NEG_INF, 0xFFFFFFFFu};
    const bool pass = have && c.row != 0xFFFFFFFFu && wtk_accepts(tk, k, c.score, c.row);
    wtk_offer(tk, k, pass, c.score, c.row, lane);
  }
  if (static_cast<uint32_t>(lane) < k) {
    const bool have = static_cast<uint32_t>(lane) < tk.cnt;
    out_ids[static_cast<uint64_t>(q) * k + lane] = have ? (row_base + tk.id) : ~0ull;
    out_scores[static_cast<uint64_t>(q) * k + lane] = have ? tk.s : NEG_INF;
  }
  if (out_counts && lane == 0) out_counts[q] = tk.cnt;
}

// grid = ceil(nrows / 256), block = 256: rows[i] < n (the host checked); several listed rows may share a word, hence the atomics
static __global__ __launch_bounds__(256) void update_row_mask_kernel(uint32_t* __restrict__ plane, const uint32_t* __restrict__ rows,
                                                                     uint64_t nrows, bool live) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= nrows) return;
  const uint32_t r = rows[i], bit = 1u << (r & 31u);
  if (live) atomicOr(plane + (r >> 5), bit);
  else atomicAnd(plane + (r >> 5), ~bit);
}

}  // namespace nvdbhip
