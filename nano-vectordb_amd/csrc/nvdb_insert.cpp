// nvdb_insert.cpp -- nvdb_hip_reserve_rows and nvdb_hip_insert_rows (include/nvdb_hip.h, DESIGN.md section 4 "Insertion"): new rows
// join the ends of partitions of the resident corpus, on the device -- the compaction's mirror image.
//   1. stage: the new rows (and scales) host -> device; the load's own kernels give their shadow rows and their share of the norm
//      bounds (row_norm_max_kernel, shadow_q8_kernel, shadow_f16_kernel, shadow_i8_kernel over the staged rows);
//   2. plan (insert_plan.h): counts and shifts per partition, the new table, every new row's position, the descending slabs;
//   3. planes: every resident plane through the map into the spare buffer (swapped in at the end), new rows live;
//   4. the walk, per array (rows, scales, shadows and their scales).  In place where n + m fits the capacity: descending slabs from
//      the last row down to the end of the first partition that receives rows -- a direct slab is one launch that reads the slab and
//      writes above it, any other is copied into the bounce buffer and spread from there.  Otherwise into freshly allocated arrays
//      (old + new resident at the peak): rows below the walk by one copy, the slabs straight to their new positions, no bounce;
//   5. the staged rows into the gaps; behind the new end the padding reads as zeros again; n, capacity, table, planes, bounds follow.
// Where a new row forbids a resident shadow (a non-finite value under the q8 shadow, |x| >= 60000 under the fp16 shadow) only the rows
// are placed and corpus_rederive runs the load's pass over all of them.  A HIP error from step 4 on leaves no half-moved corpus: the
// context drops it.
#include "nvdb_insert.h"
#include "nvdb_parts.h"
#include "insert_plan.h"
#include "kernels_corpus.h"
#include "kernels_insert.h"

namespace nvdbhip {
namespace {

enum ArrKind { ARR_ROWS, ARR_SCALES, ARR_SH8, ARR_SH8S, ARR_SH16 };

// one per-row array of the resident corpus: row_bytes per row; staged: the new rows' entries (device), fresh: its grown replacement
struct InsArray { ArrKind kind; void* p; size_t row_bytes; const void* staged; void* fresh; };

inline size_t pad_rows_up(size_t n) { return (n + PAD_ROWS - 1) / PAD_ROWS * PAD_ROWS + PAD_ROWS; }

// bytes of an array with room for `cap` rows, as a load of cap rows allocates it (corpus_alloc_padded, compute_max_norm) ...
size_t arr_bytes(const InsArray& a, size_t cap) {
  if (a.kind == ARR_SCALES) return (cap + PAD_ROWS) * 4;
  if (a.kind == ARR_SH8S) return pad_rows_up(cap) * 4;
  return cap * a.row_bytes + static_cast<size_t>(PAD_ROWS) * a.row_bytes + 4096;
}
// ... and the bytes behind row n that must read as zeros
size_t arr_tail(const InsArray& a, size_t n) {
  if (a.kind == ARR_SCALES) return static_cast<size_t>(PAD_ROWS) * 4;
  if (a.kind == ARR_SH8S) return (pad_rows_up(n) - n) * 4;
  return static_cast<size_t>(PAD_ROWS) * a.row_bytes + 4096;
}

// the owned arrays of the resident corpus; shadows: with its shadows
std::vector<InsArray> corpus_arrays(const nvdb_hip_ctx* c, bool shadows) {
  std::vector<InsArray> v;
  v.push_back(InsArray{ARR_ROWS, c->rows, static_cast<size_t>(c->dim) * bpe_of(c->dtype), nullptr, nullptr});
  if (c->scales) v.push_back(InsArray{ARR_SCALES, c->scales, 4, nullptr, nullptr});
  if (shadows && c->shadow8) {
    v.push_back(InsArray{ARR_SH8, c->shadow8, c->q8shadow ? c->dim : c->fdim, nullptr, nullptr});   // (the filter shadow keeps the dim, the padded-dim shadow runs at fdim)
    v.push_back(InsArray{ARR_SH8S, c->shadow8_scales, 4, nullptr, nullptr});
  }
  if (shadows && c->shadow16) v.push_back(InsArray{ARR_SH16, c->shadow16, static_cast<size_t>(c->fdim) * 2, nullptr, nullptr});
  return v;
}

void free_fresh(std::vector<InsArray>& arrays) {
  for (InsArray& a : arrays) if (a.fresh) { (void)hipFree(a.fresh); a.fresh = nullptr; }
}

// replacements with room for `cap` rows; a failure frees what it allocated
nvdb_status alloc_fresh(nvdb_hip_ctx* c, std::vector<InsArray>& arrays, size_t cap, const char* who) {
  for (InsArray& a : arrays) {
    const hipError_t e = hipMalloc(&a.fresh, arr_bytes(a, cap));
    if (e != hipSuccess) {
      a.fresh = nullptr;
      free_fresh(arrays);
      (void)hipGetLastError();
      return fail(c, NVDB_ERR_HIP, std::string(who) + ": allocation of the grown arrays: " + hipGetErrorString(e));
    }
  }
  return NVDB_OK;
}

// the replacements become the corpus' arrays
void adopt_fresh(nvdb_hip_ctx* c, std::vector<InsArray>& arrays, uint64_t cap) {
  for (InsArray& a : arrays) {
    (void)hipFree(a.p);
    switch (a.kind) {
      case ARR_ROWS: c->rows = a.fresh; break;
      case ARR_SCALES: c->scales = static_cast<float*>(a.fresh); break;
      case ARR_SH8: c->shadow8 = static_cast<signed char*>(a.fresh); break;
      case ARR_SH8S: c->shadow8_scales = static_cast<float*>(a.fresh); break;
      case ARR_SH16: c->shadow16 = static_cast<_Float16*>(a.fresh); break;
    }
    a.p = a.fresh; a.fresh = nullptr;
  }
  c->cap_rows = cap;
}

// f(lane): lane a value of the widest vector type row_bytes guarantees
template <class F>
void with_lane(size_t row_bytes, F&& f) {
  if (row_bytes % 16 == 0) f(CompactLane16{});
  else if (row_bytes % 8 == 0) f(CompactLane8{});
  else if (row_bytes % 4 == 0) f(uint32_t{});
  else if (row_bytes % 2 == 0) f(uint16_t{});
  else f(uint8_t{});
}

// the device image of a plan (ins_meta): [old offsets | shifts | new offsets]
struct PlanImage { const uint64_t *off_old, *shift, *off_new; uint32_t nparts; };

// old rows [sl.s0, sl.s1) of src (whose first row is old row src_row0) to their new rows of dst
nvdb_status launch_spread(nvdb_hip_ctx* c, hipStream_t s, const InsArray& a, const void* src, uint64_t src_row0, void* dst, const PlanImage& im, const InsSlab& sl) {
  const uint32_t nt = static_cast<uint32_t>((sl.s1 - sl.s0 + INS_TILE_ROWS - 1) / INS_TILE_ROWS);
  with_lane(a.row_bytes, [&](auto lane) {
    using LaneT = decltype(lane);
    insert_spread_kernel<LaneT><<<nt, INSERT_MOVE_THREADS, 0, s>>>(static_cast<const LaneT*>(src), src_row0, static_cast<LaneT*>(dst), im.off_old, im.shift, im.nparts,
                                                                    sl.s0, sl.s1, static_cast<uint32_t>(a.row_bytes / sizeof(LaneT)));
  });
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

nvdb_status launch_scatter(nvdb_hip_ctx* c, hipStream_t s, const InsArray& a, void* dst, const uint32_t* pos, uint64_t m) {
  const uint32_t nt = static_cast<uint32_t>((m + INS_TILE_ROWS - 1) / INS_TILE_ROWS);
  with_lane(a.row_bytes, [&](auto lane) {
    using LaneT = decltype(lane);
    insert_scatter_kernel<LaneT><<<nt, INSERT_MOVE_THREADS, 0, s>>>(static_cast<const LaneT*>(a.staged), static_cast<LaneT*>(dst), pos, m,
                                                                     static_cast<uint32_t>(a.row_bytes / sizeof(LaneT)));
  });
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

// steps 4 and 5 for one array.  grow: a.fresh receives every row; else the array moves in place
nvdb_status move_array(nvdb_hip_ctx* c, hipStream_t s, const InsArray& a, bool grow, const InsPlan& pl, const std::vector<InsSlab>& slabs, const PlanImage& im,
                       const uint32_t* pos) {
  char* dst = static_cast<char*>(grow ? a.fresh : a.p);
  if (grow && pl.lo) HIPCHK(c, hipMemcpyAsync(dst, a.p, pl.lo * a.row_bytes, hipMemcpyDeviceToDevice, s));   // (rows below the walk keep their numbers)
  for (const InsSlab& sl : slabs) {
    if (grow || sl.direct) {
      if (nvdb_status st = launch_spread(c, s, a, a.p, 0, dst, im, sl)) return st;
      continue;
    }
    HIPCHK(c, hipMemcpyAsync(c->cp_bounce.p, static_cast<const char*>(a.p) + sl.s0 * a.row_bytes, (sl.s1 - sl.s0) * a.row_bytes, hipMemcpyDeviceToDevice, s));
    if (nvdb_status st = launch_spread(c, s, a, c->cp_bounce.p, sl.s0, dst, im, sl)) return st;
  }
  if (nvdb_status st = launch_scatter(c, s, a, dst, pos, pl.m)) return st;
  const size_t n_new = static_cast<size_t>(pl.n + pl.m);
  HIPCHK(c, hipMemsetAsync(dst + n_new * a.row_bytes, 0, arr_tail(a, n_new), s));
  return NVDB_OK;
}

struct DevTmp {                                    // a device allocation that lives as long as its scope
  void* p = nullptr;
  DevTmp() = default;
  DevTmp(const DevTmp&) = delete;
  DevTmp& operator=(const DevTmp&) = delete;
  ~DevTmp() { if (p) (void)hipFree(p); }
};
nvdb_status tmp_alloc(nvdb_hip_ctx* c, DevTmp& t, size_t bytes) {
  HIPCHK(c, hipMalloc(&t.p, std::max<size_t>(bytes, 256)));
  return NVDB_OK;
}

// two words of the misc block after a kernel has written them
nvdb_status read_bits(nvdb_hip_ctx* c, hipStream_t s, const uint32_t* bits, uint32_t hb[2]) {
  HIPCHK(c, hipMemcpyAsync(hb, bits, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return NVDB_OK;
}
inline float as_float(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

template <int DT>
nvdb_status launch_norm(nvdb_hip_ctx* c, hipStream_t s, const void* rows, const float* scales, uint64_t m, uint32_t dim, uint32_t* bits) {
  HIPCHK(c, hipMemsetAsync(bits, 0, 8, s));
  const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((m + 3) / 4, 4096));
  row_norm_max_kernel<DT><<<grid, 256, 0, s>>>(rows, scales, m, dim, bits);
  HIPCHK(c, hipGetLastError());
  return NVDB_OK;
}

}  // namespace

nvdb_status insert_stage(nvdb_hip_ctx* c, const char* who, const void* rows, const float* scales, uint64_t m, bool needs_table, const uint32_t* part_of,
                         InsertStage& stage, bool* done) {
  *done = true;
  const std::string w(who);
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (!c->owned) return fail(c, NVDB_ERR_UNSUPPORTED, w + ": an adopted corpus is the caller's memory (unpadded, not moved)");
  if (m == 0) return NVDB_OK;
  if (!rows) return fail(c, NVDB_ERR_INVALID, w + ": null rows");
  if (c->dtype == NVDB_DTYPE_I8 && !scales) return fail(c, NVDB_ERR_INVALID, w + ": int8 corpus needs per-row scales");
  const bool table = c->parts && !c->parts->offsets.empty();
  if ((needs_table || part_of) && !table) return fail(c, NVDB_ERR_INVALID, w + ": part_of without a partition table (nvdb_hip_set_partitions)");
  if (part_of) {
    const uint64_t nparts = c->parts->offsets.size() - 1;
    for (uint64_t i = 0; i < m; ++i)
      if (part_of[i] >= nparts) return fail(c, NVDB_ERR_INVALID, w + ": an entry of part_of is >= the number of partitions");
  }
  if (m >= 0xFFFFFFF0ull - c->n) return fail(c, NVDB_ERR_UNSUPPORTED, w + ": corpus shard must hold fewer than 2^32-16 rows (shard it)");
  if ((table || c->nmasks) && c->n + m > ROW_MASK_MAX_ROWS) return fail(c, NVDB_ERR_UNSUPPORTED, w + ": too many rows for the resident partition table / row masks");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t rb = static_cast<size_t>(c->dim) * bpe_of(c->dtype);
  HIPCHK(c, hipMalloc(&stage.rows, std::max<size_t>(m * rb, 256)));
  if (c->dtype == NVDB_DTYPE_I8) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&stage.scales), std::max<size_t>(m * 4, 256)));
  HIPCHK(c, hipMemcpyAsync(stage.rows, rows, m * rb, hipMemcpyHostToDevice, c->stream));
  if (stage.scales) HIPCHK(c, hipMemcpyAsync(stage.scales, scales, m * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *done = false;
  return NVDB_OK;
}

nvdb_status insert_staged(nvdb_hip_ctx* c, const char* who, const InsertStage& stage, uint64_t m, const uint32_t* part_of, uint64_t* out_new_rows, uint64_t* out_n,
                          InsPlan* out_plan) {
  const std::string w(who);
  hipStream_t s = c->stream;
  nvdb_status st;
  const uint64_t n = c->n, n_new = n + m;
  const bool table = c->parts && !c->parts->offsets.empty();

  // 2. the plan (a corpus without a table is one partition)
  const uint64_t whole[2] = {0, n};
  const uint64_t* offsets = table ? c->parts->offsets.data() : whole;
  const uint32_t nparts = table ? static_cast<uint32_t>(c->parts->offsets.size() - 1) : 1u;
  InsPlan pl;
  std::vector<uint64_t> new_rows(m);
  if (!ins_plan(offsets, nparts, part_of, m, pl, new_rows.data())) return fail(c, NVDB_ERR_INVALID, w + ": an entry of part_of is >= the number of partitions");
  const bool grow = n_new > c->cap_rows;
  const uint64_t new_cap = grow ? ins_capacity(n, m, c->cap_rows, static_cast<uint64_t>(c->opt_insert_growth_pct)) : c->cap_rows;

  // 1. (second half) what the load's kernels say about the staged rows
  HIPCHK(c, hipSetDevice(c->device));
  if ((st = ensure(c, c->misc, 64))) return st;
  uint32_t* bits = static_cast<uint32_t*>(c->misc.p) + 8;
  uint32_t hb[2] = {0, 0};
  if (c->dtype == NVDB_DTYPE_F32) st = launch_norm<DT_F32>(c, s, stage.rows, stage.scales, m, c->dim, bits);
  else if (c->dtype == NVDB_DTYPE_F16) st = launch_norm<DT_F16>(c, s, stage.rows, stage.scales, m, c->dim, bits);
  else st = launch_norm<DT_I8>(c, s, stage.rows, stage.scales, m, c->dim, bits);
  if (st || (st = read_bits(c, s, bits, hb))) return st;
  const float new_max_norm = as_float(hb[0]);
  const bool new_signed = hb[1] != 0;
  float new_filter_norm = 0.f, new_resid = 0.f;
  bool shadow_bad = false;                           // a new row holds a value a load would not have built the resident shadow for
  DevTmp sh8, sh8s, sh16;
  ShadowScaleFact cs = c->shadow_cs;
  const void* staged_sh8s = nullptr;
  if (c->q8shadow) {
    if ((st = tmp_alloc(c, sh8, m * c->dim)) || (st = tmp_alloc(c, sh8s, m * 4))) return st;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((m + 3) / 4, 4096));
    uint32_t hb4[4] = {0, 0, 0, 0};
    auto quantise = [&](float common) -> nvdb_status {
      HIPCHK(c, hipMemsetAsync(bits, 0, 16, s));
      if (c->dtype == NVDB_DTYPE_F32) shadow_q8_kernel<float><<<grid, 256, 0, s>>>(static_cast<const float*>(stage.rows), static_cast<signed char*>(sh8.p), static_cast<float*>(sh8s.p), m, c->dim, c->dim, common, bits);
      else shadow_q8_kernel<_Float16><<<grid, 256, 0, s>>>(static_cast<const _Float16*>(stage.rows), static_cast<signed char*>(sh8.p), static_cast<float*>(sh8s.p), m, c->dim, c->dim, common, bits);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(hb4, bits, 16, hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipStreamSynchronize(s));
      return NVDB_OK;
    };
    // a shadow under one common scale takes the new rows under that scale; a new row above it has clipped: the new rows are
    // quantised again under their own scales and the fact falls (shadow_scale_plan.h) -- applied below, once the move has succeeded
    if ((st = quantise(cs.common ? cs.s_c : 0.f))) return st;
    if (cs.common && !shadow_cs_after_write(cs, as_float(hb4[2])) && (st = quantise(0.f))) return st;
    hb[0] = hb4[0]; hb[1] = hb4[1];
    new_resid = as_float(hb[0]);
    shadow_bad = hb[1] != 0;
    if (!shadow_bad) {
      if ((st = launch_norm<DT_I8>(c, s, sh8.p, static_cast<const float*>(sh8s.p), m, c->dim, bits)) || (st = read_bits(c, s, bits, hb))) return st;
      new_filter_norm = as_float(hb[0]);
    }
    staged_sh8s = sh8s.p;
  } else if (c->shadow8) {                           // the padded-dim shadow of an int8 corpus: the rows zero-padded, the corpus' own scales
    if ((st = tmp_alloc(c, sh8, m * c->fdim))) return st;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((m * c->fdim + 255) / 256, 4096));
    shadow_i8_kernel<<<grid, 256, 0, s>>>(static_cast<const signed char*>(stage.rows), static_cast<signed char*>(sh8.p), m, c->dim, c->fdim);
    HIPCHK(c, hipGetLastError());
    staged_sh8s = stage.scales;
  }
  if (c->shadow16) {
    if ((st = tmp_alloc(c, sh16, m * c->fdim * 2))) return st;
    HIPCHK(c, hipMemsetAsync(bits, 0, 8, s));
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((m * c->fdim + 255) / 256, 4096));
    if (c->dtype == NVDB_DTYPE_F32) shadow_f16_kernel<float><<<grid, 256, 0, s>>>(static_cast<const float*>(stage.rows), static_cast<_Float16*>(sh16.p), m, c->dim, c->fdim, bits);
    else shadow_f16_kernel<_Float16><<<grid, 256, 0, s>>>(static_cast<const _Float16*>(stage.rows), static_cast<_Float16*>(sh16.p), m, c->dim, c->fdim, bits);
    HIPCHK(c, hipGetLastError());
    if ((st = read_bits(c, s, bits, hb))) return st;
    if (!(as_float(hb[0]) < 60000.f)) shadow_bad = true;
  }

  // the arrays that move (the shadows only where they stay), the plan's image, the new rows' positions
  std::vector<InsArray> arrays = corpus_arrays(c, !shadow_bad);
  for (InsArray& a : arrays)
    a.staged = a.kind == ARR_ROWS ? stage.rows : a.kind == ARR_SCALES ? static_cast<const void*>(stage.scales) : a.kind == ARR_SH8 ? sh8.p : a.kind == ARR_SH8S ? staged_sh8s : sh16.p;
  std::vector<uint64_t> meta;
  meta.insert(meta.end(), pl.off_old.begin(), pl.off_old.end());
  meta.insert(meta.end(), pl.shift.begin(), pl.shift.end());
  meta.insert(meta.end(), pl.off_new.begin(), pl.off_new.end());
  std::vector<uint32_t> pos32(new_rows.begin(), new_rows.end());   // (n + m < 2^32 - 16)
  if ((st = ensure(c, c->ins_meta, meta.size() * 8)) || (st = ensure(c, c->ins_pos, m * 4))) return st;
  HIPCHK(c, hipMemcpyAsync(c->ins_meta.p, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->ins_pos.p, pos32.data(), m * 4, hipMemcpyHostToDevice, s));
  const uint64_t* d_meta = static_cast<const uint64_t*>(c->ins_meta.p);
  const PlanImage im{d_meta, d_meta + nparts + 1, d_meta + 2 * static_cast<size_t>(nparts) + 1, nparts};
  std::vector<InsSlab> slabs;
  ins_slabs(pl, static_cast<uint64_t>(c->opt_compact_slab_rows), slabs);
  if (!grow) {
    size_t bounce = 0;
    for (const InsSlab& sl : slabs)
      if (!sl.direct)
        for (const InsArray& a : arrays) bounce = std::max(bounce, static_cast<size_t>(sl.s1 - sl.s0) * a.row_bytes);
    if (bounce && (st = ensure(c, c->cp_bounce, bounce))) return st;
  }

  // 3. every plane through the map, into the spare
  const uint32_t W = static_cast<uint32_t>(rm_words(n)), W2 = static_cast<uint32_t>(rm_words(n_new));
  if (c->nmasks) {
    if ((st = ensure(c, c->row_masks_alt, static_cast<size_t>(c->nmasks) * W2 * 4))) return st;
    insert_planes_kernel<<<dim3((W2 + 255) / 256, c->nmasks), 256, 0, s>>>(static_cast<const uint32_t*>(c->row_masks.p), W, static_cast<uint32_t*>(c->row_masks_alt.p), W2,
                                                                           im.off_old, im.off_new, nparts, n_new);
    HIPCHK(c, hipGetLastError());
  }
  if (grow && (st = alloc_fresh(c, arrays, new_cap, who))) return st;
  if (hipStreamSynchronize(s) != hipSuccess) {       // (so far nothing of the context has changed)
    free_fresh(arrays);
    return fail(c, NVDB_ERR_HIP, w + ": staging failed on the device");
  }

  // 4. + 5. the walk; from here on a failure drops the corpus
  for (const InsArray& a : arrays)
    if ((st = move_array(c, s, a, grow, pl, slabs, im, static_cast<const uint32_t*>(c->ins_pos.p)))) break;
  if (!st && hipStreamSynchronize(s) != hipSuccess) st = fail(c, NVDB_ERR_HIP, w + ": the move failed on the device");
  if (!st) {
    if (grow) adopt_fresh(c, arrays, new_cap);
    c->n = n_new;
    if (shadow_bad) st = corpus_rederive(c);
  }
  if (st) {
    const std::string why = c->err;
    (void)hipGetLastError();
    free_fresh(arrays);
    corpus_drop(c);
    return fail(c, NVDB_ERR_HIP, why + " (the corpus was dropped: load it again)");
  }
  if (!shadow_bad) {
    c->max_norm = std::max(c->max_norm, new_max_norm);
    if (c->q8shadow) {
      c->filter_max_norm = std::max(c->filter_max_norm, new_filter_norm);
      c->resid_max = std::max(c->resid_max, new_resid);
      c->shadow_cs = cs;
    } else {
      c->filter_max_norm = c->max_norm;
      c->i8_scales_signed = c->i8_scales_signed || new_signed;
    }
  }
  if (table) c->parts->offsets = pl.off_new;
  if (c->nmasks) {
    std::swap(c->row_masks, c->row_masks_alt);
    for (uint64_t& live : c->mask_live) live += m;
  }
  c->range_valid = false; c->range_total = 0;        // the held range results name rows by their old numbers
  if (out_new_rows) std::copy(new_rows.begin(), new_rows.end(), out_new_rows);
  if (out_n) *out_n = n_new;
  if (out_plan) *out_plan = std::move(pl);
  return NVDB_OK;
}

}  // namespace nvdbhip

extern "C" {

nvdb_status nvdb_hip_reserve_rows(nvdb_hip_ctx* c, uint64_t rows) {
  if (!c) return NVDB_ERR_INVALID;
  if (!c->rows || c->n == 0) return fail(c, NVDB_ERR_NO_CORPUS, "Empty base");
  if (!c->owned) return fail(c, NVDB_ERR_UNSUPPORTED, "reserve_rows: an adopted corpus is the caller's memory");
  if (rows <= c->cap_rows) return NVDB_OK;
  if (rows >= 0xFFFFFFF0ull) return fail(c, NVDB_ERR_UNSUPPORTED, "reserve_rows: corpus shard must hold fewer than 2^32-16 rows (shard it)");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  std::vector<InsArray> arrays = corpus_arrays(c, true);
  if (nvdb_status st = alloc_fresh(c, arrays, rows, "reserve_rows")) return st;
  hipError_t e = hipSuccess;
  for (const InsArray& a : arrays) {                 // the rows as they stand, zeros behind them
    const size_t used = static_cast<size_t>(c->n) * a.row_bytes;
    if (e == hipSuccess) e = hipMemcpyAsync(a.fresh, a.p, used, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(static_cast<char*>(a.fresh) + used, 0, arr_tail(a, c->n), s);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {                             // the old arrays were only read: nothing changed
    free_fresh(arrays);
    (void)hipGetLastError();
    return fail(c, NVDB_ERR_HIP, std::string("reserve_rows: ") + hipGetErrorString(e));
  }
  adopt_fresh(c, arrays, rows);
  return NVDB_OK;
}

nvdb_status nvdb_hip_insert_rows(nvdb_hip_ctx* c, const void* rows, const float* scales, uint64_t m, const uint32_t* part_of, uint64_t* out_new_rows, uint64_t* out_n) {
  if (!c) return NVDB_ERR_INVALID;
  InsertStage stage;
  bool done = false;
  if (nvdb_status st = insert_stage(c, "insert_rows", rows, scales, m, false, part_of, stage, &done)) return st;
  if (done) {                                        // m == 0
    if (out_n) *out_n = c->n;
    return NVDB_OK;
  }
  return insert_staged(c, "insert_rows", stage, m, part_of, out_new_rows, out_n);
}

}  // extern "C"
