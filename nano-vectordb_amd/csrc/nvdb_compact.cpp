// nvdb_compact.cpp -- nvdb_hip_compact_rows (include/nvdb_hip.h, DESIGN.md section 4 "Compaction"): the rows that are dead in one
// plane leave the resident corpus, on the device, in place.
//   1. rank: per 64-row tile the live rows before it (two kernels around a host scan of one sum per 1024 tiles), read back with
//      the plane -- the host plans from them (compact_plan.h: first dead row, slabs, direct or bounce, the partition table);
//   2. planes: every resident plane squeezed through the same map into the spare buffer (swapped in at the end);
//   3. map out, where the caller wants it;
//   4. the walk: per array (rows, scales, shadows and their scales) the slabs in ascending order -- a direct slab is one launch that
//      reads the slab and writes below it, any other one launch into the bounce buffer and a copy from there, both on the
//      context's stream.  Destinations lie at or below sources and slabs ascend, so nothing is overwritten before it is read;
//   5. the padding behind the new end reads as zeros again; n, the planes, their live counts, the table follow.
// A HIP error from step 4 on leaves no half-moved corpus: the context drops it.
#include "nvdb_parts.h"
#include "compact_plan.h"
#include "kernels_compact.h"

namespace nvdbhip {
namespace {

// one per-row array of the resident corpus: row_bytes per row, `pad` bytes behind row n that must read as zeros
struct MovedArray { void* p; size_t row_bytes, pad; };

// the launch of one slab of one array: tiles [s0 / 64, ceil(s1 / 64)), the widest vector row_bytes guarantees
nvdb_status launch_move(nvdb_hip_ctx* c, hipStream_t s, const MovedArray& a, const CpSlab& sl, void* dst, uint64_t dst_row0, const uint32_t* plane,
                        uint32_t W, const uint32_t* rank) {
  const uint32_t t0 = static_cast<uint32_t>(sl.s0 / CP_TILE_ROWS), nt = static_cast<uint32_t>(cp_tiles(sl.s1)) - t0;
  const uint32_t row_lo = static_cast<uint32_t>(sl.s0);
  auto go = [&](auto lane) {
    using LaneT = decltype(lane);
    compact_move_kernel<LaneT><<<nt, COMPACT_MOVE_THREADS, 0, s>>>(static_cast<const LaneT*>(a.p), static_cast<LaneT*>(dst), dst_row0, plane, W, rank, t0,
                                                                   row_lo, static_cast<uint32_t>(a.row_bytes / sizeof(LaneT)));
  };
  if (a.row_bytes % 16 == 0) go(CompactLane16{});
  else if (a.row_bytes % 8 == 0) go(CompactLane8{});
  else if (a.row_bytes % 4 == 0) go(uint32_t{});
  else if (a.row_bytes % 2 == 0) go(uint16_t{});
  else go(uint8_t{});
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

// steps 4 and 5 for one array
nvdb_status move_array(nvdb_hip_ctx* c, hipStream_t s, const MovedArray& a, const std::vector<CpSlab>& slabs, uint64_t n_new, const uint32_t* plane, uint32_t W,
                       const uint32_t* rank) {
  for (const CpSlab& sl : slabs) {
    if (sl.direct) {
      if (nvdb_status st = launch_move(c, s, a, sl, a.p, 0, plane, W, rank)) return st;
      continue;
    }
    if (nvdb_status st = launch_move(c, s, a, sl, c->cp_bounce.p, sl.d0, plane, W, rank)) return st;
    HIPCHK(c, hipMemcpyAsync(static_cast<char*>(a.p) + sl.d0 * a.row_bytes, c->cp_bounce.p, (sl.d1 - sl.d0) * a.row_bytes, hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(c, hipMemsetAsync(static_cast<char*>(a.p) + n_new * a.row_bytes, 0, a.pad, s));
  return NVDB_OK;
}

}  // namespace
}  // namespace nvdbhip

extern "C" {

nvdb_status nvdb_hip_compact_rows(nvdb_hip_ctx* c, uint32_t mask, uint64_t* out_n, uint32_t* out_old_rows) {
  if (!c) return NVDB_ERR_INVALID;
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (!c->owned) return fail(c, NVDB_ERR_UNSUPPORTED, "compact_rows: an adopted corpus is the caller's memory (unpadded, not moved)");
  if (c->nmasks == 0) return fail(c, NVDB_ERR_INVALID, "compact_rows: no row masks (nvdb_hip_set_row_masks)");
  if (mask >= c->nmasks) return fail(c, NVDB_ERR_INVALID, "compact_rows: mask >= nmasks (nvdb_hip_set_row_masks)");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  nvdb_status st;
  const uint64_t n = c->n;                           // (planes are resident: n <= ROW_MASK_MAX_ROWS, rows and ranks fit 32 bits)
  const uint32_t W = static_cast<uint32_t>(rm_words(n)), T = static_cast<uint32_t>(cp_tiles(n));
  const uint32_t* planes = static_cast<const uint32_t*>(c->row_masks.p);
  const uint32_t* plane = planes + static_cast<size_t>(mask) * W;

  // 1. the count, then the ranks
  const uint32_t nblocks = (T + COMPACT_RANK_THREADS - 1) / COMPACT_RANK_THREADS;
  if ((st = ensure(c, c->cp_rank, (static_cast<size_t>(T) + 1) * 4))) return st;
  if ((st = ensure(c, c->cp_sums, (static_cast<size_t>(nblocks) + 1) * 4))) return st;
  uint32_t* rank = static_cast<uint32_t*>(c->cp_rank.p);
  compact_tile_rank_kernel<<<nblocks, COMPACT_RANK_THREADS, 0, s>>>(plane, W, T, rank, static_cast<uint32_t*>(c->cp_sums.p));
  HIPCHK(c, hipGetLastError());
  std::vector<uint32_t> base(static_cast<size_t>(nblocks) + 1);
  HIPCHK(c, hipMemcpyAsync(base.data(), c->cp_sums.p, static_cast<size_t>(nblocks) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  uint64_t n_new = 0;
  for (uint32_t b = 0; b < nblocks; ++b) { const uint32_t sum = base[b]; base[b] = static_cast<uint32_t>(n_new); n_new += sum; }
  base[nblocks] = static_cast<uint32_t>(n_new);
  if (n_new == 0) return fail(c, NVDB_ERR_INVALID, "compact_rows: no row is live in the plane (an empty corpus is not representable)");
  if (n_new == n) {                                  // nothing to move: the identity map
    if (out_n) *out_n = n;
    if (out_old_rows) for (uint64_t j = 0; j < n; ++j) out_old_rows[j] = static_cast<uint32_t>(j);
    return NVDB_OK;
  }
  HIPCHK(c, hipMemcpyAsync(c->cp_sums.p, base.data(), base.size() * 4, hipMemcpyHostToDevice, s));
  compact_rank_add_kernel<<<(T + 1 + 255) / 256, 256, 0, s>>>(rank, T, static_cast<const uint32_t*>(c->cp_sums.p), nblocks);
  HIPCHK(c, hipGetLastError());
  std::vector<uint32_t> h_rank(static_cast<size_t>(T) + 1), h_plane(W);
  HIPCHK(c, hipMemcpyAsync(h_rank.data(), rank, h_rank.size() * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(h_plane.data(), plane, static_cast<size_t>(W) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  std::vector<CpSlab> slabs;
  cp_plan(h_plane.data(), h_rank.data(), n, static_cast<uint64_t>(c->opt_compact_slab_rows), slabs);

  // the arrays that move, and the bounce buffer: one slab of the widest of them
  const size_t rb = static_cast<size_t>(c->dim) * bpe_of(c->dtype);
  std::vector<MovedArray> arrays;
  arrays.push_back(MovedArray{c->rows, rb, static_cast<size_t>(PAD_ROWS) * rb + 4096});
  if (c->scales) arrays.push_back(MovedArray{c->scales, 4, static_cast<size_t>(n + PAD_ROWS - n_new) * 4});
  if (c->shadow8) {
    const size_t sb = c->q8shadow ? c->dim : c->fdim;                       // (the filter shadow keeps the dim, the padded-dim shadow runs at fdim)
    const size_t n_pad = (static_cast<size_t>(n) + PAD_ROWS - 1) / PAD_ROWS * PAD_ROWS + PAD_ROWS;
    arrays.push_back(MovedArray{c->shadow8, sb, static_cast<size_t>(PAD_ROWS) * sb + 4096});
    arrays.push_back(MovedArray{c->shadow8_scales, 4, (n_pad - n_new) * 4});
  }
  if (c->shadow16) arrays.push_back(MovedArray{c->shadow16, static_cast<size_t>(c->fdim) * 2, static_cast<size_t>(PAD_ROWS) * c->fdim * 2 + 4096});
  size_t bounce = 0;
  for (const CpSlab& sl : slabs)
    if (!sl.direct)
      for (const MovedArray& a : arrays) bounce = std::max(bounce, static_cast<size_t>(sl.d1 - sl.d0) * a.row_bytes);
  if (bounce && (st = ensure(c, c->cp_bounce, bounce))) return st;

  // 2. every plane through the map, into the spare
  const uint32_t W2 = static_cast<uint32_t>(rm_words(n_new));
  const size_t fresh_bytes = static_cast<size_t>(c->nmasks) * W2 * 4;
  if ((st = ensure(c, c->row_masks_alt, fresh_bytes))) return st;
  if ((st = ensure(c, c->cp_live, static_cast<size_t>(c->nmasks) * 8))) return st;
  HIPCHK(c, hipMemsetAsync(c->row_masks_alt.p, 0, fresh_bytes, s));
  HIPCHK(c, hipMemsetAsync(c->cp_live.p, 0, static_cast<size_t>(c->nmasks) * 8, s));
  compact_planes_kernel<<<dim3((T + 255) / 256, c->nmasks), 256, 0, s>>>(planes, W, T, mask, rank, static_cast<uint32_t*>(c->row_masks_alt.p), W2,
                                                                         static_cast<unsigned long long*>(c->cp_live.p));
  HIPCHK(c, hipGetLastError());
  std::vector<uint64_t> live(c->nmasks);
  HIPCHK(c, hipMemcpyAsync(live.data(), c->cp_live.p, live.size() * 8, hipMemcpyDeviceToHost, s));

  // 3. the map
  if (out_old_rows) {
    if ((st = ensure(c, c->cp_map, static_cast<size_t>(n_new) * 4))) return st;
    compact_map_kernel<<<(T + 3) / 4, 256, 0, s>>>(plane, W, T, rank, static_cast<uint32_t*>(c->cp_map.p));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_old_rows, c->cp_map.p, static_cast<size_t>(n_new) * 4, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));                // (so far nothing of the context has changed)

  // 4. + 5. the walk; from here on a failure drops the corpus
  for (const MovedArray& a : arrays)
    if ((st = move_array(c, s, a, slabs, n_new, plane, W, rank))) break;
  if (!st && hipStreamSynchronize(s) != hipSuccess) st = fail(c, NVDB_ERR_HIP, "compact_rows: the move failed on the device");
  if (st) {
    const std::string why = c->err;
    (void)hipGetLastError();
    corpus_drop(c);
    return fail(c, NVDB_ERR_HIP, why + " (the corpus was dropped: load it again)");
  }
  if (c->parts && !c->parts->offsets.empty())
    cp_offsets(h_plane.data(), h_rank.data(), n, c->parts->offsets.data(), c->parts->offsets.size(), c->parts->offsets.data());
  std::swap(c->row_masks, c->row_masks_alt);
  c->mask_live = live;
  c->n = n_new;
  c->range_valid = false; c->range_total = 0;        // the held range results name rows by their old numbers
  if (out_n) *out_n = n_new;
  return NVDB_OK;
}

}  // extern "C"
