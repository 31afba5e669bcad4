// pq_plan.h -- the host-side arithmetic of the PQ candidate scan (nvdb_pq.cpp, kernels_pq.h; DESIGN.md section 4 "PQ candidate
// scan"): which shapes a PQ shadow takes, the encode kernel's compile-time sub-vector bound, how many queries' tables a scan
// workgroup holds in LDS, how its lanes load their codes, how many queries one sub-batch's tables may serve, and the trainer's
// chunk, LDS and partial-sum sizes (kernels_pq_train.h; kernels_pq4_train.h for 16 codewords).  Plain C++ with no HIP in it, like the
// other plans.
#pragma once
#include <cstddef>
#include <cstdint>

namespace nvdbhip {

constexpr uint32_t PQ_KSUB = 256;                   // codewords per sub-quantiser: one byte per code
constexpr uint32_t PQ_M_MAX = 128;                  // sub-quantisers at most: one query's tables are M KB of LDS
constexpr uint32_t PQ_DSUB_MAX = 32;                // the encode kernel's widest build: a lane holds its sub-vector in 32 registers, 256 codewords x 32 floats = 32 KB of LDS
constexpr size_t PQ_LDS_BUDGET = 156 * 1024;        // LDS the tables of a scan workgroup may take (of 160 KB)

// 0: fine; else why nvdb_hip_pq_build refuses the shape (unsupported: the arguments are valid, the build does not exist)
inline const char* pq_shape_check(uint32_t dim, uint32_t M, bool& unsupported) {
  unsupported = false;
  if (M < 4 || M % 4 != 0 || M > PQ_M_MAX) return "M must be a multiple of 4 in [4, 128]";
  if (dim == 0 || dim % M != 0) return "dim must be a multiple of M";
  if (dim / M > PQ_DSUB_MAX) { unsupported = true; return "dim / M <= 32 (the encode kernel's widest build)"; }
  return nullptr;
}

// the encode kernel's build for sub-vectors of dsub elements: the smallest bound of {4, 8, 16, 32} that holds them
constexpr uint32_t pq_encode_bound(uint32_t dsub) { return dsub <= 4 ? 4u : dsub <= 8 ? 8u : dsub <= 16 ? 16u : 32u; }

// bytes of one query's tables: [M][256] f32
constexpr size_t pq_lut_bytes(uint32_t M) { return static_cast<size_t>(M) * PQ_KSUB * 4; }

// THE LDS budget rule: queries per scan workgroup = the largest G of {8, 4, 2, 1} whose tables fit (8 up to M = 19, 4 up to 39,
// 2 up to 78, 1 up to 128)
constexpr uint32_t pq_group(uint32_t M) {
  for (uint32_t G = 8; G > 1; G >>= 1)
    if (G * pq_lut_bytes(M) <= PQ_LDS_BUDGET) return G;
  return 1;
}

// ---- the trainer (nvdb_hip_pq_train, kernels_pq_train.h)
constexpr uint32_t PQ_TRAIN_CHUNK = 4096;           // training rows per workgroup of the step kernel: the unit of the fp64 sums' order (include/nvdb_hip.h names it)
constexpr uint32_t PQ_TRAIN_MIN_ROWS = PQ_KSUB;     // a start needs 256 distinct training rows

// the training set of max_train_rows over n resident rows: every row (0 or >= n), else that many
constexpr uint64_t pq_train_rows(uint64_t n, uint64_t max_train_rows) { return (max_train_rows == 0 || max_train_rows >= n) ? n : max_train_rows; }
constexpr uint64_t pq_train_chunks(uint64_t m) { return (m + PQ_TRAIN_CHUNK - 1) / PQ_TRAIN_CHUNK; }
// the step kernel's LDS for the build DMAX: codewords [256][DMAX] f32, the tile's sub-vectors [DMAX][256] f32, four fp64 wave sums, 256 code bytes
constexpr size_t pq_train_lds(uint32_t dmax) { return 2 * static_cast<size_t>(PQ_KSUB) * dmax * 4 + 4 * 8 + 256; }
// bytes of the per-chunk fp64 partial sums
constexpr uint64_t pq_train_partial_bytes(uint64_t m, uint32_t dim) { return pq_train_chunks(m) * PQ_KSUB * dim * 8; }

// ---- the residual shadow (kernels_pq_resid.h)
// rows nvdb_hip_pq_reconstruct maps per launch: at most 64 MB of f32 output on the device, at least one row
constexpr uint64_t pq_reconstruct_rows(uint32_t dim) {
  const uint64_t r = (64ull << 20) / (static_cast<uint64_t>(dim) * 4);
  return r < 1 ? 1 : r;
}

// ---- OPQ rotations (kernels_pq_rotate.h): Y[rows][dim] = E[rows][dim] . A^T on the fp32 matrix cores
// THE tile cut: a workgroup of 8 waves owns 256 rows x 128 output columns (a wave: 64 x 64, 16 accumulator tiles), K in slices of
// 16 through LDS.  Operand traffic through L2 and LDS is n * dim^2 * 4 * (1 / 256 + 1 / 128) bytes: 277 GB at 10M x 768, against
// 737 GB at 64 x 64; the MFMA time of 2 * n * dim^2 flop at 157 TFLOP/s is 75 ms there, so the tile has to stage 3.7 TB/s over 256
// CUs to hide under it: 6 bytes per CU and clock at 2.4 GHz (64 x 64: 16), where a CU's LDS takes 128.
constexpr uint32_t PQ_ROT_TR = 256;                 // rows per workgroup tile
constexpr uint32_t PQ_ROT_TC = 128;                 // output columns per workgroup tile (a column panel of the matrix)
constexpr uint32_t PQ_ROT_KS = 16;                  // K elements per LDS slice: four MFMA K-steps

// workgroups of one launch over nrows rows: row tiles x column panels, the panel varying fastest
constexpr uint64_t pq_rotate_grid(uint64_t nrows, uint32_t dim) {
  return ((nrows + PQ_ROT_TR - 1) / PQ_ROT_TR) * ((dim + PQ_ROT_TC - 1) / PQ_ROT_TC);
}
// rows one slab of rotated f32 rows holds (the build and the trainer rotate slab by slab into scratch memory that lives inside the
// call): at most 256 MB, whole row tiles, at least one; at dim >= 4 a slab's grid stays below 2^17 workgroups
constexpr uint64_t pq_rotate_slab_rows(uint32_t dim) {
  const uint64_t r = (256ull << 20) / (static_cast<uint64_t>(dim) * 4) / PQ_ROT_TR * PQ_ROT_TR;
  return r < PQ_ROT_TR ? PQ_ROT_TR : r;
}

// a lane reads its row's codes in 16-byte pieces where a row is whole pieces, else in dwords (M % 4 == 0 always)
constexpr bool pq_wide_codes(uint32_t M) { return M % 16 == 0; }

// queries one sub-batch may hold tables for: budget_bytes of them, at least one
constexpr uint32_t pq_lut_batch(uint32_t M, uint64_t budget_bytes) {
  const uint64_t b = budget_bytes / pq_lut_bytes(M);
  return b < 1 ? 1u : b > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(b);
}

// ---- 4-bit shadows (nvdb_hip_pq4_build, kernels_pq4.h): 16 codewords per sub-quantiser, two codes to a byte
constexpr uint32_t PQ4_KSUB = 16;                   // codewords per sub-quantiser: one table row is 16 consecutive dwords
constexpr uint32_t PQ4_M_MAX = 256;                 // sub-quantisers at most: one query's tables are 64 M bytes, 16 KB here
constexpr uint32_t PQ4_ENC_SQ = 8;                  // sub-quantisers per encode step: a thread leaves one dword of packed codes
constexpr uint32_t PQ_BASE_DIM_MAX = PQ_M_MAX * PQ_DSUB_MAX;   // pq_base_kernel stages one centroid in a static array of this many floats

// 0: fine; else why nvdb_hip_pq4_build refuses the shape.  residual: the search's base terms go through pq_base_kernel as it is,
// whose centroid array bounds dim (an 8-bit shape never exceeds it; a 4-bit one can, at M > 128 with dsub 32)
inline const char* pq4_shape_check(uint32_t dim, uint32_t M, bool residual, bool& unsupported) {
  unsupported = false;
  if (M < 8 || M % 8 != 0 || M > PQ4_M_MAX) return "M must be a multiple of 8 in [8, 256] (4-bit codes)";
  if (dim == 0 || dim % M != 0) return "dim must be a multiple of M";
  if (dim / M > PQ_DSUB_MAX) { unsupported = true; return "dim / M <= 32 (the encode kernel's widest build)"; }
  if (residual && dim > PQ_BASE_DIM_MAX) { unsupported = true; return "dim <= 4096 for a residual 4-bit shadow (the base terms' centroid stage)"; }
  return nullptr;
}

// ---- the 16-codeword trainer (nvdb_hip_pq4_train, kernels_pq4_train.h): the 8-bit trainer's chunk and training-set rules
constexpr uint32_t PQ4_TRAIN_MIN_ROWS = PQ4_KSUB;   // a start needs 16 distinct training rows
// sub-quantisers a step workgroup owns for the build dmax: a row contributes at most 64 f32 elements (8, 8, 4, 2 at dmax 4, 8, 16,
// 32; M % 8 == 0 makes each divide M)
constexpr uint32_t pq4_train_sq(uint32_t dmax) { return dmax <= 8 ? 8u : 64u / dmax; }
// dwords between two rows of the tile's sub-vectors in LDS: the group's elements plus one, ODD -- phase 1 writes with lane = row,
// phase 2 reads with lane = column, and neither hits a bank twice whichever power of two the bank count is
constexpr uint32_t pq4_train_stride(uint32_t dmax) { return pq4_train_sq(dmax) * dmax + 1; }
// the step kernel's LDS for the build dmax: fp64 wave sums [4][sq], codewords [sq][16][dmax] f32, 256 code dwords, the tile's
// sub-vectors [256][stride] f32 -- at most 71936 bytes (dmax 8; 37120 at dmax 4): two workgroups in a CU's 160 KB
constexpr size_t pq4_train_lds(uint32_t dmax) {
  return 4 * static_cast<size_t>(pq4_train_sq(dmax)) * 8 + static_cast<size_t>(pq4_train_sq(dmax)) * PQ4_KSUB * dmax * 4 + 256 * 4 +
         256 * static_cast<size_t>(pq4_train_stride(dmax)) * 4;
}
static_assert(2 * pq4_train_lds(4) <= 160 * 1024 && 2 * pq4_train_lds(8) <= 160 * 1024 && 2 * pq4_train_lds(16) <= 160 * 1024 &&
                  2 * pq4_train_lds(32) <= 160 * 1024,
              "two step workgroups per CU");
// bytes of the per-chunk fp64 partial sums
constexpr uint64_t pq4_train_partial_bytes(uint64_t m, uint32_t dim) { return pq_train_chunks(m) * PQ4_KSUB * dim * 8; }

// bytes of one row's codes and of one query's tables ([M][16] f32) under either width
constexpr uint32_t pq_row_bytes(uint32_t M, uint32_t nbits) { return nbits == 4 ? M / 2 : M; }
constexpr size_t pq4_lut_bytes(uint32_t M) { return static_cast<size_t>(M) * PQ4_KSUB * 4; }

// THE group rule of the 4-bit scan: G = the largest of {32, 16, 8} whose interleaved tables (G * 64 M bytes) leave room for TWO
// workgroups per CU, i.e. fit half the LDS budget; 8 where none does (8 * 64 * 256 = 128 KB still fits one).  Why two: a wave's
// work per nibble is one ds_read_b128 and four dependent-free adds per quad, with nothing else to overlap a code load's latency
// than other waves -- 16 waves per CU (4 per SIMD) are what the 8-bit scan runs with at its best group sizes, and a second
// workgroup also covers the first one's table copy and barrier.  Why not smaller than that: every doubling of G halves the
// re-reads of a list's codes and the table stream through L2.  32 up to M = 32, 16 up to M = 72, 8 above (M = 96: 48 KB, three
// workgroups per CU).  PART_WAVES * PART_QW_MAX = 32 is the work list's widest group.
constexpr uint32_t pq4_group(uint32_t M) {
  for (uint32_t G = 32; G > 8; G >>= 1)
    if (G * pq4_lut_bytes(M) <= PQ_LDS_BUDGET / 2) return G;
  return 8;
}

// the 4-bit scan's LDS: the G tables and, behind them, G slab offsets and G base terms
constexpr size_t pq4_scan_lds(uint32_t M, uint32_t G) { return G * pq4_lut_bytes(M) + G * 8u; }

// a lane reads its row's M / 2 code bytes in 16-byte pieces where a row is whole pieces, else in dwords (M % 8 == 0 always)
constexpr bool pq4_wide_codes(uint32_t M) { return (M / 2) % 16 == 0; }

// queries one sub-batch may hold 4-bit tables for: budget_bytes of them, at least one
constexpr uint32_t pq4_lut_batch(uint32_t M, uint64_t budget_bytes) {
  const uint64_t b = budget_bytes / pq4_lut_bytes(M);
  return b < 1 ? 1u : b > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(b);
}

// ---- the L2 metric (nvdb_hip_pq_set_metric, kernels_pq_l2.h): h[r] = |xhat_r|^2 / 2, one f32 per row beside the codes
// h is allocated as the codes are -- one hipMalloc outside every budget option, a failure leaves the metric where it was --: 4
// bytes per row beside M or M / 2 of codes, 40 MB at 10M rows
constexpr uint64_t pq_norm_bytes(uint64_t n) { return n * 4; }
constexpr uint32_t PQ_NORM_THREADS = 256;
// rows a lane of pq_norms_kernel owns (so many accumulators): a tile stages the whole codebook, dim KB, through LDS, so its cost
// per row falls with the tile -- at 4 a tile is 1024 rows and the staging 0.75 KB per row at dim 768, a third of pq_encode's
// (its tiles are 256 rows); 8 would halve it again but leaves 10M rows only 1221 tiles for 256 CUs and doubles the tail
constexpr uint32_t PQ_NORM_ROWS_PER_LANE = 4;
constexpr uint32_t PQ_NORM_TILE = PQ_NORM_THREADS * PQ_NORM_ROWS_PER_LANE;
// floats between two codewords of the LDS image: ODD, so that 64 lanes on 64 different codewords hit 64 different banks
constexpr uint32_t pq_norm_stride(uint32_t dsub) { return dsub | 1u; }
// columns per LDS chunk of pq_rownorm_kernel and the floats between two of its rows (odd again: lane = row walks its row)
constexpr uint32_t PQ_ROWNORM_COLS = 32;
constexpr uint32_t PQ_ROWNORM_LD = PQ_ROWNORM_COLS + 1;

}  // namespace nvdbhip
