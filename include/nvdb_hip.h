/*
 * nvdb_hip.h -- C ABI of libnvdb_hip.so: the MI355X (gfx950) replacement for nano-vectordb's
 * flat-scan hot path and its exact-L2 refine stage.
 *
 * Plain C, plain pointers and sizes, no C++/torch types, no exceptions.  Every call returns an
 * nvdb_status (0 = OK); nvdb_hip_last_error(ctx) holds the message of the last failure.  The host
 * C++ wrappers (nano-vectordb_amd/host/include/nvdb/) translate status != 0 into
 * std::runtime_error, the reference's flat-path convention (src/flat_index.cpp:17).
 *
 * Each entry point names the reference interface it stands in for (file:line into the reference
 * tree).  INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Threading: a context is single-owner (one host thread at a time), like the reference's
 * process-global CUDA state (src/cuda_refine.cu:26-90); different contexts are independent, which
 * is how the multi-GPU path runs one context per device / per process.
 */
#ifndef NVDB_HIP_H
#define NVDB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVDB_HIP_ABI_VERSION 3

/* dtype codes == VecbinHeader::dtype (include/nvdb/vecbin_format.h:10-14) */
enum { NVDB_DTYPE_F32 = 1, NVDB_DTYPE_F16 = 2, NVDB_DTYPE_I8 = 3 };

typedef enum nvdb_status {
  NVDB_OK = 0,
  NVDB_ERR_INVALID = 1,      /* bad argument (null pointer, dim/dtype mismatch, k too large ...) */
  NVDB_ERR_HIP = 2,          /* a HIP runtime call failed (no device, out of memory ...)         */
  NVDB_ERR_UNSUPPORTED = 3,  /* shape outside what the kernels implement                          */
  NVDB_ERR_NO_CORPUS = 4,    /* search/refine before a corpus is resident ("Empty base")         */
  NVDB_ERR_INTERNAL = 5      /* a self-check failed (filter error bound violated, overflow ...)   */
} nvdb_status;

/* The flat path takes ANY k (clamped to the row count like the reference, src/flat_index.cpp:24): k <= 64 runs on
 * wavefront-resident lists / the MFMA filter, 65..1024 on the filter path where it is eligible (MFMA bootstrap, a dtype / dim
 * with a bootstrap build, >= 512*k rows), every other k > 64 on the any-k path (scores -> radix select -> sort).
 * Largest K of the refine path = the reference's NVDB_CUDA_KMAX = 64 (src/cuda_refine.cu:12-14, 858-862). */
#define NVDB_HIP_REFINE_KMAX 64

typedef struct nvdb_hip_ctx nvdb_hip_ctx;

/* Field-for-field mirror of nvdb::CudaRefineTiming (include/nvdb/cuda_refine.h:7-22); the flat
 * path fills h2d/kernel/d2h/total and leaves the rest zero.  dbg_*: the refine call's in-kernel
 * phase split (reference CUDA_DBG_TIMING, src/cuda_refine.cu:416-418, 495-500, 1116-1144), filled
 * when option "refine_dbg_q" > 0 and a timing struct is passed: the first dbg_q = min(option, Q)
 * queries run the STAMP build of the refine kernel's template, and dbg_*_cycles_avg are their average
 * shader-clock cycles (s_memtime) per phase -- dist (gather + distances + top-K insertion), write
 * (list to LDS + barrier), merge (wave 0 merges the lists, stores the result).  dbg_*_pct are
 * FRACTIONS of the three averages' sum (0 when it is 0).  Otherwise all dbg_* are zero. */
typedef struct nvdb_hip_timing {
  float h2d_ms, kernel_ms, d2h_ms, total_ms;
  uint32_t threads;
  uint32_t nwarps;          /* number of 64-lane wavefronts per workgroup */
  uint32_t K;
  uint32_t R;
  size_t shmem_bytes;       /* LDS bytes per workgroup of the dominant kernel */
  uint32_t dbg_q;
  double dbg_dist_cycles_avg, dbg_write_cycles_avg, dbg_merge_cycles_avg;
  double dbg_dist_pct, dbg_write_pct, dbg_merge_pct;
} nvdb_hip_timing;

/* What the last flat search did (for tests, bench.py and the roofline arithmetic). */
typedef struct nvdb_hip_scan_stats {
  uint32_t path;               /* 1 = exact fp32 scan, 2 = MFMA filter + exact rescore (k <= 1024), 3 = any-k (k > 64 off the filter path), 4 = partitioned probe search,
                                  5 = range search, filter route, 6 = range search, exact route, 7 = range search, partition scan, 8 = probe search, any k */
  uint32_t chunks;             /* corpus chunks (kernel launches of the dominant kernel)          */
  uint64_t rows_scanned;       /* rows x query-tiles streamed by the dominant kernel              */
  uint64_t candidates;         /* (query,row) pairs that reached the exact rescore                */
  uint32_t overflow_queries;   /* queries whose candidate list overflowed (re-run on path 1)      */
  uint32_t bound_violations;   /* |filter - exact| > bound seen by the rescore (must be 0)        */
  float    filter_kernel_ms;   /* sum of hipEvent times of the dominant kernel's launches (host API with a timing struct and option "time_launches" = 1; else 0) */
  float    other_kernel_ms;    /* prep + select + rescore + merge                                  */
  uint32_t i8_stage1_tiles;    /* int8 two-stage kernel: (wave, tile) pairs that went past the hi-plane quick test */
  uint32_t i8_stage2_blocks;   /* ... 32-query blocks for which the lo plane was multiplied after all           */
  uint32_t sticky_overflow;    /* nvdb_hip_search_check: a list / log overflow in ANY device-API search since the last check */
  uint32_t sticky_violations;  /* ... bound violations summed over those searches (both cleared by the check)    */
} nvdb_hip_scan_stats;

/* ---------------------------------------------------------------------------------------------
 * library / device
 * ------------------------------------------------------------------------------------------- */
int nvdb_hip_abi_version(void);
/* Number of visible HIP devices, or -1 when the runtime cannot initialise (no GPU). */
int nvdb_hip_device_count(void);

/* One context per GPU.  Replaces the reference's implicit device 0 + file-static caches
 * (src/cuda_refine.cu:26-90, :951).  Owns a HIP stream, the resident corpus and a grow-only
 * workspace (reference: ensure_workspace, src/cuda_refine.cu:144-176). */
nvdb_status nvdb_hip_create(int device_ordinal, nvdb_hip_ctx** out_ctx);
void nvdb_hip_destroy(nvdb_hip_ctx* ctx);
const char* nvdb_hip_last_error(const nvdb_hip_ctx* ctx);   /* ctx may be NULL: last create() error */

/* ---------------------------------------------------------------------------------------------
 * corpus residency -- replaces ensure_base_on_gpu (src/cuda_refine.cu:179-204) and the
 * FlatIndex(const VectorDataset*) constructor's borrowed pointer (include/nvdb/flat_index.h:11-16)
 * ------------------------------------------------------------------------------------------- */

/* Copy a row-major corpus into HBM (staged through pinned chunks; `rows` may be an mmap).
 * rows: n*dim elements of dtype; scales: n floats, required iff dtype == I8 (the vecbin layout
 * stores them after the payload, src/vector_dataset.cpp:86-87).  global_row_base is added to
 * every returned id (row-sharding across GPUs: shard g holds rows [base, base+n)). */
nvdb_status nvdb_hip_upload_corpus(nvdb_hip_ctx* ctx, const void* rows, const float* scales,
                                   uint64_t n, uint32_t dim, uint32_t dtype, uint64_t global_row_base);

/* Use a corpus that is already in HBM (e.g. a torch tensor); not copied, not freed. */
nvdb_status nvdb_hip_adopt_corpus(nvdb_hip_ctx* ctx, void* dev_rows, float* dev_scales,
                                  uint64_t n, uint32_t dim, uint32_t dtype, uint64_t global_row_base);

/* Generate the synthetic corpus rows [global_row_base, global_row_base+n) directly in HBM
 * (counter-based rows keyed (seed,row,col), L2-normalised, then f16 = RNE /
 * int8 = the reference quantiser's rule).  Bit-identical to nvdb_synth_rows() on the CPU. */
nvdb_status nvdb_hip_generate_corpus(nvdb_hip_ctx* ctx, uint64_t seed, uint64_t n, uint32_t dim,
                                     uint32_t dtype, uint64_t global_row_base);

nvdb_status nvdb_hip_corpus_info(const nvdb_hip_ctx* ctx, uint64_t* n, uint32_t* dim, uint32_t* dtype,
                                 uint64_t* global_row_base, float* max_row_norm);

/* Copy rows [row0,row0+nrows) (local indices) back to the host; scales_out may be NULL. */
nvdb_status nvdb_hip_download_rows(nvdb_hip_ctx* ctx, uint64_t row0, uint64_t nrows, void* rows_out,
                                   float* scales_out);

/* ---------------------------------------------------------------------------------------------
 * flat scan: batched query x corpus dot products + fused top-k
 * ------------------------------------------------------------------------------------------- */

/* Exact top-k by dot product for nq fp32 queries [nq][dim] (host memory).
 * Stands in for FlatIndex::search_topk_dot / FlatIndexOMP::search_topk_dot called nq times
 * (src/flat_index.cpp:16-48, src/flat_index_omp.cpp:16-85) and for the bench-side batched loop
 * batched_scan_omp_or_st (apps/nvdb_bench.cpp:47-159).
 *   out_ids[nq][k], out_scores[nq][k]: best first; ids are global (base + local row).
 *   k is clamped to the resident row count like the reference (flat_index.cpp:24); *out_k_eff
 *   (optional) receives min(k, n); slots >= k_eff hold id UINT64_MAX / score -inf.
 *   Scores are bit-identical to the reference's AVX2 kernels (simd_dot.cpp:26-49, 102-124,
 *   160-199); ties are ordered (score desc, id asc).
 *   k == 0 -> NVDB_OK, nothing written (flat_index.cpp:18).  Any k > 0 is accepted. */
nvdb_status nvdb_hip_search_batch(nvdb_hip_ctx* ctx, const float* queries, uint32_t nq, uint32_t k,
                                  uint64_t* out_ids, float* out_scores, uint32_t* out_k_eff,
                                  nvdb_hip_timing* timing);

/* Same, with queries and outputs already in HBM and all work enqueued on `hip_stream`
 * (a hipStream_t; NULL = the context's own NON-BLOCKING stream -- note that the legacy default stream also has the
 * handle NULL: a caller whose other work is on the default stream must pass an explicit stream or synchronise the
 * device, the context's stream is not ordered with it).  Returns after enqueueing; no host sync, so
 * overflow / bound self-checks are reported by nvdb_hip_search_check() after the caller has
 * synchronised the stream; the check covers EVERY search enqueued since the previous check (sticky flags), its
 * per-query detail and statistics describe the last one.  This is the form the multi-GPU path uses before its all-gather. */
nvdb_status nvdb_hip_search_batch_dev(nvdb_hip_ctx* ctx, const float* dev_queries, uint32_t nq, uint32_t k,
                                      uint64_t* dev_out_ids, float* dev_out_scores, void* hip_stream);
nvdb_status nvdb_hip_search_check(nvdb_hip_ctx* ctx, nvdb_hip_scan_stats* stats);
/* Statistics of the last nvdb_hip_search_batch() / nvdb_hip_range_search() (summed over its sub-batches). */
nvdb_status nvdb_hip_get_stats(nvdb_hip_ctx* ctx, nvdb_hip_scan_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * range search: every row whose score reaches a per-query radius.  The reference has no range entry point; the shape is the one
 * users know from FAISS: Index::range_search fills a RangeSearchResult whose lims[nq + 1] delimit each query's slice of the
 * labels / distances arrays (faiss/impl/AuxIndexStructures.h).  Here the slices are exact: the scores are the reference-order dot
 * products nvdb_hip_search_batch returns, bit for bit, whichever route (MFMA filter + exact rescore, or exact scores) found them.
 * ------------------------------------------------------------------------------------------- */

/* queries [nq][dim] f32, radius [nq], out_lims [nq + 1]: host memory; synchronous.
 * Row i belongs to query q iff score(q, i) >= radius[q] as a C float comparison: a NaN score never belongs, a NaN radius gives an
 * empty slice, radius = -inf every row whose score is not NaN, +0.0 and -0.0 compare equal.  Inside a slice: score descending, id
 * ascending.  out_lims[q] .. out_lims[q + 1] is query q's slice, out_lims[0] = 0, out_lims[nq] the total; the lims are complete and
 * exact whenever the call returns NVDB_OK or NVDB_ERR_UNSUPPORTED.
 * The packed results (uint64 global ids = global_row_base + local row, float scores) stay in grow-only device buffers of the context
 * until the next range search or corpus load; nvdb_hip_range_results copies them out.
 * Budget: option "range_max_mb" (default 4096).  Packed results (12 bytes per entry) beyond it -> NVDB_ERR_UNSUPPORTED, the message names
 * the total and the option, the lims are written (tighten the radii or raise the option), nothing is held.
 * nq == 0 -> NVDB_OK, out_lims[0] = 0.  Null pointer -> NVDB_ERR_INVALID.  No corpus -> NVDB_ERR_NO_CORPUS.  Any nq (sub-batches of
 * 1024 queries inside).  Option "path": 0 automatic, 1 exact route, 2 filter route, as for the flat search; the result does not depend on it.
 * A violated filter bound (never observed) -> the results are recomputed on the exact route and the call returns NVDB_ERR_INTERNAL.
 * nvdb_hip_get_stats afterwards: path 5 / 6, chunks (filter launches + score-matrix passes), rows_scanned, candidates (list entries
 * that reached the rescore), overflow_queries (queries redone on the exact route), bound_violations.
 * timing (optional): h2d / kernel / total; the results' copy is nvdb_hip_range_results'. */
nvdb_status nvdb_hip_range_search(nvdb_hip_ctx* ctx, const float* queries, uint32_t nq,
                                  const float* radius /* [nq] */, uint64_t* out_lims /* [nq+1] */,
                                  nvdb_hip_timing* timing /* may be NULL */);
/* out_ids / out_scores: out_lims[nq] entries of the last range search (host memory).  NVDB_ERR_INVALID: a null pointer, no range
 * search yet, the last one exceeded its budget, or the corpus has changed since. */
nvdb_status nvdb_hip_range_results(nvdb_hip_ctx* ctx, uint64_t* out_ids, float* out_scores);

/* The int8 filter shadow of an fp16 / fp32 corpus (option "q8_shadow"), read-only: out4[0] = 1 if one is resident, out4[1] = its bytes
 * of HBM, out4[2] = 1 if it has overflowed on this corpus and searches now start on the fp16 filter (cleared by the next corpus load),
 * out4[3] = what the filter launches of the last search streamed: 0 nothing (exact / any-k route), 1 the fp16 rows, 2 the int8
 * shadow, 3 an int8 corpus.  After a host-API call that retried, out4[3] describes the last attempt. */
nvdb_status nvdb_hip_shadow_info(const nvdb_hip_ctx* ctx, uint64_t* out4);

/* The scales of a resident int8 filter shadow, read-only (all 0 without one).  A load writes the shadow under ONE common scale -- the
 * largest per-row reference scale of the corpus, so nothing clips -- where that widens the largest quantisation residual of any row by
 * at most a quarter (option "shadow_common_scale", set before the load: 0 = always the reference's per-row scales); the flat search then
 * tests the filter's accumulators without a multiply.  out4[0] = 1 if every scale of the shadow is the common one (an inserted row
 * above it clears the fact, results stay exact either way), out4[1] = the common scale the load found, out4[2] / out4[3] = the
 * largest residual the load measured under the per-row rule / under the common scale (0: not measured). */
nvdb_status nvdb_hip_shadow_scale_info(const nvdb_hip_ctx* ctx, double* out4);

/* Merge per-shard top-k lists (e.g. after an RCCL all-gather): in[s][nq][k] -> out[nq][k] with
 * the same (score desc, id asc) order.  Device buffers, enqueued on hip_stream.  Any k the flat path accepts (the reference
 * bounds k by N only, src/flat_index.cpp:24): up to nshards*k = 4096 the lists of one query are ranked in LDS; longer ones are
 * merged by binary searches and must arrive sorted best-first with their padding (id ~0, -inf) last, as every search emits them. */
nvdb_status nvdb_hip_merge_topk_dev(nvdb_hip_ctx* ctx, const uint64_t* dev_ids, const float* dev_scores,
                                    uint32_t nshards, uint32_t nq, uint32_t k, uint64_t* dev_out_ids,
                                    float* dev_out_scores, void* hip_stream);
/* Same with explicit byte strides between consecutive shards' blocks: lets each rank all-gather ONE packed buffer
 * [ids (nq*k*8 bytes) | scores (nq*k*4 bytes)] and merge it in place (stride = nq*k*12 for both). */
nvdb_status nvdb_hip_merge_topk_strided_dev(nvdb_hip_ctx* ctx, const uint64_t* dev_ids, const float* dev_scores,
                                            size_t stride_ids_bytes, size_t stride_scores_bytes, uint32_t nshards,
                                            uint32_t nq, uint32_t k, uint64_t* dev_out_ids, float* dev_out_scores,
                                            void* hip_stream);
/* Host version of the same merge (no GPU needed). */
nvdb_status nvdb_merge_topk_host(const uint64_t* ids, const float* scores, uint32_t nshards, uint32_t nq,
                                 uint32_t k, uint64_t* out_ids, float* out_scores);

/* ---------------------------------------------------------------------------------------------
 * device group: ONE process driving several GPUs of a node (the reference has no multi-GPU path; the north star's
 * "corpus row-sharded across the GPUs, RCCL all-gather of per-shard partial top-k over xGMI").  Shard g holds the
 * contiguous rows [g*n/G, (g+1)*n/G) on devices[g] with global ids.  A batch is searched on every shard
 * (nvdb_hip_search_batch_dev, one host thread per device for the enqueue), each device's [ids | scores] block
 * (nq*k*12 bytes) is all-gathered with ONE ncclAllGather per device inside ncclGroupStart/End on the devices' streams,
 * and the k-way merge runs on devices[0] (same (score desc, id asc) order: the result equals the unsharded search bit
 * for bit).  RCCL is bound with dlopen at group creation; when it cannot serve the list (a device named twice, RCCL
 * absent, NVDB_GROUP_NO_RCCL=1) the exchange is G peer copies into devices[0] and the same merge kernel.
 * A shard whose self-check trips (list overflow, non-finite query) sends the sub-batch through the per-shard host API
 * (which retries / falls back by itself) and a host-side merge.
 * NVDB_GROUP_RCCL_LIB=<path> (read at group creation) binds the six RCCL entry points from another library instead: the tests
 * drive the RCCL branch with several ranks on one device through a loopback stand-in (tests/loopback_rccl).
 * One process per GPU (bench.py, torch.distributed) uses nvdb_hip_search_batch_dev + the caller's all-gather +
 * nvdb_hip_merge_topk_strided_dev instead -- same kernels, same packed layout.
 * ------------------------------------------------------------------------------------------- */
typedef struct nvdb_hip_group nvdb_hip_group;
typedef struct nvdb_hip_group_stats {
  uint32_t shards;                /* G */
  uint32_t exchange;              /* 1 = RCCL all-gather, 0 = peer copies into devices[0] */
  uint32_t host_merge_fallbacks;  /* sub-batches of the last call that went through the host merge */
  uint64_t bytes_per_rank;        /* packed block one rank contributes per sub-batch: nq*k*12 */
} nvdb_hip_group_stats;

nvdb_status nvdb_hip_group_create(const int* devices, uint32_t n_devices, nvdb_hip_group** out_group);
void nvdb_hip_group_destroy(nvdb_hip_group* group);
const char* nvdb_hip_group_last_error(const nvdb_hip_group* group);          /* NULL: last create() error */
uint32_t nvdb_hip_group_size(const nvdb_hip_group* group);
/* the shard's own context (options, statistics, corpus_info); owned by the group */
nvdb_hip_ctx* nvdb_hip_group_ctx(nvdb_hip_group* group, uint32_t shard);
/* 1 = RCCL, 0 = peer copies; *why (optional) names the reason */
int nvdb_hip_group_exchange(const nvdb_hip_group* group, const char** why);
/* row-shard a host corpus / the synthetic corpus over the group's devices (same arguments as the per-device calls) */
nvdb_status nvdb_hip_group_upload_corpus(nvdb_hip_group* group, const void* rows, const float* scales, uint64_t n,
                                         uint32_t dim, uint32_t dtype);
nvdb_status nvdb_hip_group_generate_corpus(nvdb_hip_group* group, uint64_t seed, uint64_t n, uint32_t dim, uint32_t dtype);
nvdb_status nvdb_hip_group_set_option(nvdb_hip_group* group, const char* key, int64_t value);   /* every shard */
/* Same contract as nvdb_hip_search_batch (host queries in, [nq][k] global ids + scores out, any nq, k clamped). */
nvdb_status nvdb_hip_group_search_batch(nvdb_hip_group* group, const float* queries, uint32_t nq, uint32_t k,
                                        uint64_t* out_ids, float* out_scores, uint32_t* out_k_eff,
                                        nvdb_hip_group_stats* stats);

/* ---------------------------------------------------------------------------------------------
 * partitioned probe search: exact top-k over a per-query CHOICE of contiguous row partitions -- the inverted-list probe of
 * the reference's IVF evaluation (apps/nvdb_ivf_eval.cpp, done there through FAISS) over a list-ordered corpus, and the
 * tenant / namespace filter of a multi-tenant corpus whose tenants' rows are contiguous (row masks, below, lift that).  Queries that probe the same partition share one read of it.
 * ------------------------------------------------------------------------------------------- */

/* partition p = local rows [offsets[p], offsets[p+1]); offsets[0] == 0, non-decreasing, offsets[nparts] == n (nparts >= 1).
 * Empty partitions are legal.  The table is copied.  Any upload / adopt / generate of a corpus drops it (and the centroids);
 * a new table drops the centroids of the old one. */
nvdb_status nvdb_hip_set_partitions(nvdb_hip_ctx* ctx, const uint64_t* offsets, uint32_t nparts);

/* Optional coarse quantiser: one f32 centroid per partition, [nparts][dim] (host memory, copied); requires partitions. */
nvdb_status nvdb_hip_set_centroids(nvdb_hip_ctx* ctx, const float* centroids);

/* probe[nq][nprobe] (host): partition numbers; 0xFFFFFFFF = empty slot; a partition named twice by one query counts once;
 * any other entry >= nparts -> NVDB_ERR_INVALID before anything is launched.
 * Result per query: exact top-k by dot product over the union of its probed partitions, the same score bits and the same
 * (score desc, global id asc) order as nvdb_hip_search_batch.  out_ids[nq][k], out_scores[nq][k] as there.
 * out_counts[q] (optional) = min(k, rows in the union); slots beyond it hold id UINT64_MAX / -inf.
 * k == 0 or nq == 0 -> NVDB_OK, nothing written.  k > 64 -> NVDB_ERR_UNSUPPORTED: the lists are wavefront-resident (entry j
 * in lane j).  nprobe == 0 -> every count 0, outputs all padding.  No partition table -> NVDB_ERR_INVALID.
 * Non-finite query or corpus values: no fault, no hang, order unspecified.
 * timing (optional): h2d / kernel / d2h / total as on the flat path.  nvdb_hip_get_stats afterwards: path = 4, chunks = scan
 * launches, rows_scanned = rows read (summed over the work items), candidates = candidate slots. */
nvdb_status nvdb_hip_search_partitions(nvdb_hip_ctx* ctx, const float* queries, uint32_t nq, uint32_t k,
                                       const uint32_t* probe, uint32_t nprobe,
                                       uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                       nvdb_hip_timing* timing);

/* IVF-Flat convenience: probe = the nprobe centroids with the largest dot product (reference fp32 order, ties by partition
 * number; ranked by the flat search over the centroids), then as above.  nprobe > nparts clamps to nparts.  out_probe
 * (optional, [nq][nprobe]) returns the chosen partitions, best first (slots beyond the clamp: 0xFFFFFFFF).
 * Without centroids -> NVDB_ERR_INVALID. */
nvdb_status nvdb_hip_search_ivf(nvdb_hip_ctx* ctx, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                                uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                uint32_t* out_probe, nvdb_hip_timing* timing);

/* ---------------------------------------------------------------------------------------------
 * row masks: top-k restricted to live rows on the probe-search path -- deleted rows (tombstones) that must stop being returned
 * without a new upload, and tenant / metadata predicates whose rows are NOT contiguous.  FAISS users know this as
 * SearchParameters::sel with an IDSelectorBitmap.  A context holds nmasks bit planes over its resident corpus; plane m is
 * W = ceil(n / 32) uint32 words, LOCAL row r (global_row_base plays no part) is live in mask m iff bit r & 31 of word
 * m * W + (r >> 5) is 1.  Bits at positions >= n of a plane's last word are ignored on input and read back as 0.
 * Masked entry points: the top-k searches below (k <= 64), the range searches of the next block (nvdb_hip_range_search_partitions /
 * _ivf with masked != 0, nvdb_hip_range_search_masked, nvdb_hip_ivf_range_search) and the probe searches for any k behind them
 * (nvdb_hip_search_partitions_anyk / _ivf_anyk, nvdb_hip_ivf_search_anyk with masked != 0).
 * The masked flat top-k (nvdb_hip_search_batch_masked) rides the MFMA filter kernels where the corpus is large enough to pay for it.
 * NOT masked (out of scope so far): nvdb_hip_search_batch itself and its exact / any-k routes, nvdb_hip_range_search itself, the
 * device group, the _dev stream entry points, the masked FLAT top-k with k > 64 (nvdb_hip_search_batch_masked; on the probe path any
 * k is served, see "probe search for any k" below), the nvdb:: C++ host layer.  Those entry points, and the unmasked probe
 * searches above, ignore resident masks entirely: results, statistics and launches are what they are without masks.
 * ------------------------------------------------------------------------------------------- */

/* bits: [nmasks][W] words, host memory; NULL = every row live in every mask.  Copies the planes into HBM and replaces any
 * earlier set; nmasks == 0 drops them.  Any upload / adopt / generate of a corpus drops them; nvdb_hip_set_partitions and
 * nvdb_hip_set_centroids do not (the rows have not moved).  NVDB_ERR_NO_CORPUS: nothing resident.  NVDB_ERR_UNSUPPORTED:
 * n > 0xFFFFFF00 (the partition table's own limit).  NVDB_ERR_INVALID: nmasks == 0xFFFFFFFF (the number that means "no mask"). */
nvdb_status nvdb_hip_set_row_masks(nvdb_hip_ctx* ctx, const uint32_t* bits /* [nmasks][W], may be NULL */, uint32_t nmasks);

/* The tombstone path: sets (live != 0) or clears the bits of the listed LOCAL rows (host memory) in plane `mask`, on the device
 * (one atomic per listed row); duplicates are legal.  rows[i] >= n or mask >= nmasks -> NVDB_ERR_INVALID before anything is
 * launched, nothing changed.  nrows == 0 -> NVDB_OK.  Synchronous: the next search sees the update. */
nvdb_status nvdb_hip_update_row_mask(nvdb_hip_ctx* ctx, uint32_t mask, const uint64_t* rows, uint64_t nrows, int live);

/* Reads the planes back: *nmasks, *words_per_mask (W; 0 without masks) and, where bits_out is not NULL, the nmasks * W words.
 * Every pointer is optional. */
nvdb_status nvdb_hip_get_row_masks(nvdb_hip_ctx* ctx, uint32_t* nmasks, uint64_t* words_per_mask, uint32_t* bits_out /* may be NULL */);

/* The masked searches: the arguments of the unmasked twin plus mask_of[nq] (host): the plane query q searches under;
 * 0xFFFFFFFF = no mask, every row live; mask_of == NULL = plane 0 for every query.  Any other entry >= nmasks, or a call with no
 * masks resident -> NVDB_ERR_INVALID before anything is launched, nothing written.
 * Result per query: the exact top-k by dot product over the rows of the probed union that are LIVE in the query's mask, with the
 * score bits and the (score desc, global id asc) order of nvdb_hip_search_partitions.  out_counts[q] (optional) = min(k, live rows
 * in the union) -- counted on the device; slots beyond it hold id UINT64_MAX / -inf.  A query whose live set is empty gets count 0
 * and all padding: not an error.  k > 64, k == 0, nq == 0, nprobe == 0, the probe-table rules, timing and nvdb_hip_get_stats
 * (path 4) are the unmasked calls' (rows_scanned counts the rows of the work items, live or not).
 * Cost: the scan reads at most three mask words per 64-row tile and query beside the rows, and skips the arithmetic of a tile in
 * which none of a wavefront's queries has a live row (the rows are still fetched). */
nvdb_status nvdb_hip_search_partitions_masked(nvdb_hip_ctx* ctx, const float* queries, uint32_t nq, uint32_t k,
                                              const uint32_t* probe, uint32_t nprobe, const uint32_t* mask_of /* [nq], may be NULL */,
                                              uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                              nvdb_hip_timing* timing);
/* The coarse step is nvdb_hip_search_ivf's: centroids are not masked, a partition without a live row can still be probed. */
nvdb_status nvdb_hip_search_ivf_masked(nvdb_hip_ctx* ctx, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                                       const uint32_t* mask_of /* [nq], may be NULL */,
                                       uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                       uint32_t* out_probe, nvdb_hip_timing* timing);
/* The masked flat search: exact top-k over ALL rows that are live in the query's plane.  Needs no partition table and leaves a
 * table that is set untouched.  Two routes, one result (ids, score bits, counts, order and padding do not depend on the route):
 *  - the partition scan (nvdb_hip_get_stats: path 4): the whole corpus as ONE implicit partition that every query probes.  What this
 *    costs, plainly: the rows are read once per group of up to 32 queries (16 where the LDS holds no more beside a row tile, e.g.
 *    fp16 d = 768: a batch of 1024 then reads the corpus 64 times); it is the fp32-order VALU scan, not the matrix cores.
 *  - the MFMA filter route (path 2), per sub-batch of up to 1024 queries: per distinct plane the shortest prefix of the corpus that
 *    holds enough live rows, the scan above over that prefix alone, whose k-th best score -- an exact score of a live row -- becomes
 *    the query's bar; then ONE stream of the corpus through the filter kernels at thresholds fixed one error bound under the bars
 *    (nvdb_hip_range_search's pass), the exact rescore, the drop of dead rows, and the k best of what is left.  Queries whose list
 *    overflowed, with a non-finite element, or behind an overflowed wave log are redone on the scan, they alone; a violated filter
 *    bound -> the sub-batch is redone on the scan and the call returns NVDB_ERR_INTERNAL.  A plane with fewer than 4 k live rows
 *    is answered by the scan inside the same call.  Statistics: chunks = launches, rows_scanned = rows of the scan's work items +
 *    rows streamed per query tile, candidates = list entries, overflow_queries = queries redone; nvdb_hip_shadow_info out4[3]
 *    names what the filter streamed.
 *  Option "path": 0 = the filter route where the corpus has a filter (as nvdb_hip_range_search decides: dtype / dim, option
 *  "min_filter_batch", n >= 4 * option "chunk0") AND n >= 262144 rows, else the scan; 1 = the scan; 2 = the filter route, or
 *  NVDB_ERR_UNSUPPORTED where there is no filter for the dtype / dim.  Option "cand_cap" bounds the lists as it does for the range search.
 * k > 64 -> NVDB_ERR_UNSUPPORTED (unlike nvdb_hip_search_batch, k is not clamped: out_counts says how many entries there are). */
nvdb_status nvdb_hip_search_batch_masked(nvdb_hip_ctx* ctx, const float* queries, uint32_t nq, uint32_t k,
                                         const uint32_t* mask_of /* [nq], may be NULL */,
                                         uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                         nvdb_hip_timing* timing);

/* ---------------------------------------------------------------------------------------------
 * compaction: the other half of the tombstones.  A row that nvdb_hip_update_row_mask has marked dead still takes its HBM and is
 * still fetched, and only the masked entry points leave it out.  Compaction squeezes the dead rows of ONE plane out of the
 * resident corpus, on the device, in place; afterwards every unmasked entry point -- nvdb_hip_search_batch and its _dev form,
 * nvdb_hip_range_search, the probe searches -- serves exactly the live set at the cost of a corpus of that many rows.
 * ------------------------------------------------------------------------------------------- */

/* Removes from the resident corpus every row that is dead in plane `mask`, on the device, in place.  Stable: live rows keep
 * their order.  New local row j is old local row out_old_rows[j]; global ids are global_row_base + the NEW local row.
 * What moves, all by the same order-preserving map: the rows, the scales of an int8 corpus, the int8 shadow and its scales (the
 * padded-dim shadow of an int8 corpus as well as the filter shadow of option "q8_shadow"), the fp16 shadow.  Behind the new end
 * every one of them reads as zeros again for the padding rows and the vector-load slack an upload leaves; the scale buffers are
 * zero up to their padded length.  The buffers keep their capacity: HBM is NOT given back.
 * What follows the move: n becomes the live count; global_row_base, dtype, dim, options, statistics and what the context has
 * learnt about the corpus (the list capacity it needed, a demoted shadow) are kept.  The norm bounds of the filters (the largest
 * row norm, the shadow's, its residual, the sign of the int8 scales) are kept too: maxima over a superset of the remaining rows, so
 * every filter bound still holds -- nvdb_hip_corpus_info's max_row_norm is an UPPER BOUND after a compaction.  All resident planes
 * go through the map and are repacked to W' = ceil(n' / 32) words with tail bits 0: plane `mask` becomes all live, every other
 * plane keeps, for each surviving row, the bit it had; the live counts the library keeps per plane become exact.  A resident
 * partition table becomes offsets'[p] = live rows below the old offsets[p] (empty partitions are legal); the centroids stay, no row
 * has changed its partition.  A held range result is invalidated (nvdb_hip_range_results -> NVDB_ERR_INVALID until the next search).
 * The walk: ascending slabs of option "compact_slab_rows" rows (a multiple of 64 in [64, 2^24], default 65536).  A slab whose
 * destination ends at or before its start is moved by one launch; any other is gathered into a bounce buffer of one slab and
 * copied from there, so no launch writes bytes that it reads.  Rows before the first dead row are neither read nor written.  Peak
 * extra HBM: one slab of the widest array, 4 bytes per 64 rows, the new planes (and 4 bytes per live row where out_old_rows is given).
 *   NVDB_ERR_INVALID      ctx == NULL, no planes resident, mask >= nmasks, or no row live in the plane (an empty corpus is not
 *                         representable): nothing changed, nothing written
 *   NVDB_ERR_NO_CORPUS    nothing resident: nothing changed
 *   NVDB_ERR_UNSUPPORTED  an adopted corpus (the caller's memory, unpadded): nothing changed
 *   NVDB_OK               also where no row is dead: *out_n = n, the identity map, nothing launched beyond the count
 *   NVDB_ERR_HIP          a HIP error.  One before the first row has moved (an allocation of the workspace, the rank step): nothing
 *                         changed.  One after it leaves no half-moved corpus: the context drops its corpus, table and planes as a
 *                         load does before it loads; the next call sees NVDB_ERR_NO_CORPUS.
 * Synchronous.  A context is single-owner, as everywhere. */
nvdb_status nvdb_hip_compact_rows(nvdb_hip_ctx* ctx, uint32_t mask, uint64_t* out_n /* may be NULL */,
                                  uint32_t* out_old_rows /* may be NULL; room for the OLD n entries, the first *out_n are written */);

/* The same for an index (nvdb_hip_ivf_build, below): `mask` names a plane set with nvdb_hip_ivf_set_row_masks.  The lists shrink in
 * place and stay contiguous: offsets' = the cumulative sum of the lists' live counts, perm'[j] = perm[old position of j], and
 * nvdb_hip_ivf_info reports the new n, offsets and perm.  Results keep coming in ORIGINAL ids -- the caller's ids do not change --
 * and, the move being stable, equal scores stay ordered by (partition, original id).  nvdb_hip_ivf_set_row_masks and
 * nvdb_hip_ivf_update_row_mask afterwards still speak of ORIGINAL rows (planes of ceil(n / 32) words over the n rows the index
 * was built from); the bit or the update of a row that a compaction has removed is ignored.  Statuses as above (ivf == NULL ->
 * NVDB_ERR_INVALID).  A failure before the first row has moved -- any status but NVDB_ERR_HIP, and NVDB_ERR_HIP from the workspace's
 * allocations or the rank step -- leaves the index exactly as it was; only where the index's context has dropped its corpus (a HIP
 * error during the move: nvdb_hip_corpus_info on nvdb_hip_ivf_ctx then returns NVDB_ERR_NO_CORPUS) does the index hold no rows.
 * No row dead -> NVDB_OK, nothing changed. */
struct nvdb_hip_ivf;
nvdb_status nvdb_hip_ivf_compact(struct nvdb_hip_ivf* ivf, uint32_t mask, uint64_t* out_n /* may be NULL */);

/* ---------------------------------------------------------------------------------------------
 * insertion: the compaction's mirror image.  New rows join the resident corpus on the device, at the END of a partition; the rows
 * behind them shift up.  After an insertion the context is what a fresh context would be that uploaded the resulting rows with the
 * same options (and set the resulting table and planes).
 * Out of scope: the device group; _dev stream forms; updating centroids after an add; giving HBM back; inserting anywhere but at the
 * end of a partition.
 * ------------------------------------------------------------------------------------------- */

/* Makes room for at least `rows` rows in every library-owned array of the resident corpus (rows, scales, shadows and their scales),
 * so that insertions up to that row count move in place.  Never shrinks (rows <= the capacity: NVDB_OK, nothing done); the results
 * of every search are unchanged.  The arrays are reallocated once and copied: peak HBM is old plus new arrays.
 *   NVDB_ERR_INVALID ctx == NULL;  NVDB_ERR_NO_CORPUS nothing resident;  NVDB_ERR_UNSUPPORTED an adopted corpus, rows >= 2^32 - 16;
 *   NVDB_ERR_HIP an allocation or the copy failed: nothing changed. */
nvdb_status nvdb_hip_reserve_rows(nvdb_hip_ctx* ctx, uint64_t rows);

/* Inserts `m` host rows (the resident corpus' dtype and dim; `scales` iff it is int8) into the resident corpus.
 * part_of == NULL: the rows go behind the last resident row; with a partition table they join the last partition.
 * part_of != NULL (needs a partition table): row i goes to the end of partition part_of[i], behind the rows already there; rows that
 * name the same partition keep the order of i (the move is stable); empty partitions are legal targets.
 * Old local row r of partition p becomes r + (new rows in partitions < p); global ids stay global_row_base + the NEW local row, as
 * after a compaction.  out_new_rows[i] = the new local row of inserted row i; *out_n = the new row count.
 * What moves, all by that one order-preserving map: the rows, the scales of an int8 corpus, the int8 shadow and its scales (the
 * padded-dim shadow of an int8 corpus as well as the filter shadow of option "q8_shadow"), the fp16 shadow.  The shadow entries of the
 * new rows are computed from the new rows by the kernels a load runs.  Behind the new end every array reads as zeros again for the
 * padding rows and the vector-load slack an upload leaves (the call zeroes that region itself).  The norm bounds of the filters become
 * the maximum of their old values and the new rows' (the sign flag of the int8 scales is ORed): on a corpus that was never compacted
 * they equal a fresh load's bit for bit.  An insertion never CREATES a shadow: the automatic "q8_shadow" rule is not evaluated again
 * when n crosses its threshold.  Where a new row holds a value a load would not have built the resident shadow for (a non-finite
 * element under the q8 shadow, |x| >= 60000 under the fp16 shadow) the rows are placed, the shadows freed and the load's own pass runs
 * over all rows: slow, rare, correct.  Every resident plane goes through the map and is repacked to W' = ceil(n' / 32) words, tail
 * bits 0: old rows keep their bit, new rows are live in every plane.  A resident partition table becomes offsets'[p] = offsets[p] +
 * new rows in partitions < p; the centroids stay.  A held range result is invalidated.  Options, statistics, what the context has
 * learnt about the corpus (the list capacity it needed, a demoted shadow) and global_row_base are kept.
 * Capacity: the context records how many rows its arrays have room for -- exactly n after a load, more after nvdb_hip_reserve_rows or
 * a grown insertion; nvdb_hip_compact_rows keeps it, so an insertion after it reuses that room.  Where n + m fits, the move is in
 * place: DESCENDING slabs of option "compact_slab_rows" rows from the last row down to the end of the first partition that receives
 * rows (rows below are neither read nor written); a slab [s0, s1) whose smallest shift carries it to or beyond s1 moves in one launch,
 * any other goes through the one-slab bounce buffer, so no launch writes bytes that it reads.  Otherwise every array is reallocated
 * once, to max(n + m, capacity * (100 + option "insert_growth_pct") / 100) rows (default 50; 0: exactly n + m), and old rows are
 * written straight to their new positions: no bounce, but peak HBM on that path is OLD PLUS NEW arrays.
 *   NVDB_ERR_INVALID      ctx == NULL; m > 0 and rows == NULL, or scales == NULL on an int8 corpus; part_of without a partition
 *                         table; an entry of part_of >= nparts: nothing changed, nothing written
 *   NVDB_ERR_NO_CORPUS    nothing resident
 *   NVDB_ERR_UNSUPPORTED  an adopted corpus; n + m >= 0xFFFFFFF0; n + m > 0xFFFFFF00 with a table or planes resident: nothing changed
 *   NVDB_OK               also for m == 0: *out_n = n, nothing launched
 *   NVDB_ERR_HIP          a HIP error.  One before the first row has moved (allocations, staging): nothing changed.  One after it
 *                         leaves no half-moved corpus: the context drops its corpus, table and planes, as nvdb_hip_compact_rows does.
 * Synchronous.  A context is single-owner, as everywhere. */
nvdb_status nvdb_hip_insert_rows(nvdb_hip_ctx* ctx, const void* rows, const float* scales /* iff int8 */, uint64_t m,
                                 const uint32_t* part_of /* [m], may be NULL */,
                                 uint64_t* out_new_rows /* [m], may be NULL */, uint64_t* out_n /* may be NULL */);

/* The same for an index: the new rows get the original ids src_n + i (without the source's row base), src_n = the rows the index
 * speaks of so far (those it was built from plus those added); src_n grows by m, *out_first_id = the old src_n.  Every row is assigned
 * by nvdb_hip_assign_rows' rule -- the row as an f32 query against the index's centroids, fp32 reference order, ties to the lowest
 * centroid -- and joins the end of its list; out_assign returns the lists.  nvdb_hip_ivf_info reports the new n, offsets and perm.
 * New rows have the largest original ids, so lists stay ordered by original row: on an index that was never compacted the result
 * equals nvdb_hip_ivf_build of the concatenated source with the same centroids (rows, scales, offsets, perm, every search).  The
 * centroids are NOT updated.  Planes set with nvdb_hip_ivf_set_row_masks keep speaking of ORIGINAL rows, now src_n + m of them
 * (ceil((src_n + m) / 32) words); new rows are live.  Statuses as above (ivf == NULL -> NVDB_ERR_INVALID; src_n + m > 0xFFFFFF00 ->
 * NVDB_ERR_UNSUPPORTED).  As for nvdb_hip_ivf_compact, a failure leaves the index exactly as it was unless its context has dropped
 * its corpus (a HIP error during the move); then the index holds no rows. */
nvdb_status nvdb_hip_ivf_add_rows(struct nvdb_hip_ivf* ivf, const void* rows, const float* scales /* iff int8 */, uint64_t m,
                                  uint64_t* out_first_id /* may be NULL */, uint32_t* out_assign /* [m], may be NULL */);

/* ---------------------------------------------------------------------------------------------
 * range search on the probe path: nvdb_hip_range_search's question -- every row whose score reaches a per-query radius -- asked of
 * a per-query choice of partitions, of an IVF index, and of the rows that are live in a query's mask.  FAISS users know the
 * combination as IndexIVF::range_search with SearchParameters::sel.
 * Row i belongs to query q iff it is in the union of q's probed partitions, it is live in q's plane (masked calls), and
 * score(q, i) >= radius[q] as a C float comparison.  The score is the reference-order dot product -- the bits
 * nvdb_hip_search_partitions returns.  A NaN score never belongs, a NaN radius gives an empty slice, radius = -inf takes every
 * score that is not NaN, +0.0 and -0.0 compare equal.  Inside a slice: score descending, global id ascending.
 * out_lims [nq + 1], the packed device arrays, option "range_max_mb" and NVDB_ERR_UNSUPPORTED with complete lims above it are
 * nvdb_hip_range_search's; the result is fetched with nvdb_hip_range_results.  A range search of any kind replaces the held result.
 * masked == 0: mask_of is ignored, resident masks play no part.  masked != 0: mask_of[nq] as for the masked searches above --
 * 0xFFFFFFFF = no mask, NULL = plane 0 for every query; an entry >= nmasks or no planes resident -> NVDB_ERR_INVALID before
 * anything is launched, nothing written.
 * ------------------------------------------------------------------------------------------- */

/* probe[nq][nprobe]: nvdb_hip_search_partitions' rules (0xFFFFFFFF = empty slot, duplicates count once, an entry >= nparts ->
 * NVDB_ERR_INVALID before anything is launched).  nprobe == 0 -> all-zero lims.  nq == 0 -> NVDB_OK, out_lims[0] = 0.  Any nq:
 * the batch is cut into query sub-batches inside whose candidate blocks (8 bytes per row of a query's probed union) stay within half
 * of option "largek_budget_mb" -- the other half is the sort's key slabs; one query's block or slab is taken whatever the option
 * says --; the caller does not see the cut.  No partition table -> NVDB_ERR_INVALID; no corpus -> NVDB_ERR_NO_CORPUS.
 * nvdb_hip_get_stats afterwards: path = 7, chunks = scan launches, rows_scanned = rows of the work items, candidates = entries
 * written (= results).  timing (optional): kernel / total (the work list's copies alternate with the launches and ride inside). */
nvdb_status nvdb_hip_range_search_partitions(nvdb_hip_ctx* ctx, const float* queries, uint32_t nq,
                                             const float* radius /* [nq] */, const uint32_t* probe /* [nq][nprobe] */, uint32_t nprobe,
                                             const uint32_t* mask_of /* [nq], may be NULL */, int masked,
                                             uint64_t* out_lims /* [nq+1] */, nvdb_hip_timing* timing /* may be NULL */);
/* The coarse step, the clamp of nprobe and out_probe (optional, [nq][nprobe]) are nvdb_hip_search_ivf's; centroids are not masked.
 * Without centroids -> NVDB_ERR_INVALID. */
nvdb_status nvdb_hip_range_search_ivf(nvdb_hip_ctx* ctx, const float* queries, uint32_t nq, const float* radius /* [nq] */,
                                      uint32_t nprobe, const uint32_t* mask_of /* [nq], may be NULL */, int masked,
                                      uint64_t* out_lims /* [nq+1] */, uint32_t* out_probe /* may be NULL */,
                                      nvdb_hip_timing* timing /* may be NULL */);
/* The masked flat range search: nvdb_hip_range_search over the rows live in each query's plane (always masked: mask_of as above).
 * Where nvdb_hip_range_search takes the MFMA filter route so does this call -- the thresholds are fixed before the first row, so a
 * dead row above one only occupies a list entry until the keep step drops it (a list that overflows because of them sends its
 * query to the scan below like any overflow) -- and nvdb_hip_get_stats reports path 5.  Flagged queries, option path = 1 and
 * dims / dtypes without a filter run on the partition range scan with the corpus as one implicit partition (path 7 when nothing
 * was filtered); no partition table is needed, one that is set stays.  The result does not depend on the route.  A violated filter
 * bound -> recomputed on that scan, NVDB_ERR_INTERNAL. */
nvdb_status nvdb_hip_range_search_masked(nvdb_hip_ctx* ctx, const float* queries, uint32_t nq, const float* radius /* [nq] */,
                                         const uint32_t* mask_of /* [nq], may be NULL */, uint64_t* out_lims /* [nq+1] */,
                                         nvdb_hip_timing* timing /* may be NULL */);

/* ---------------------------------------------------------------------------------------------
 * probe search for any k: nvdb_hip_search_partitions' question for k beyond the 64 entries of its wavefront-resident lists --
 * recall@100 on an IVF-Flat index, or the R candidates per query that nvdb_hip_refine_l2_topk takes.  The existing calls keep
 * their k <= 64 contract; the capability has names of its own, with the argument shape of nvdb_hip_range_search_partitions.
 * Result per query: the exact top-k by dot product over the rows of the probed union -- for masked != 0 only the rows that are
 * live in the query's plane --, with the score bits and the (score desc, global id asc) order of nvdb_hip_search_partitions.
 * Any k >= 1 is accepted and k is NOT clamped (as on the probe search, unlike nvdb_hip_search_batch): out_ids[nq][k],
 * out_scores[nq][k]; out_counts[q] (optional) = min(k, live rows in the union), counted on the device; slots beyond the count
 * hold id UINT64_MAX / -inf.  k <= 64: the call IS its twin (nvdb_hip_search_partitions / _masked, nvdb_hip_search_ivf / _masked)
 * -- result, timing and statistics (path 4) bit for bit.
 * masked == 0: mask_of is ignored, resident masks play no part.  masked != 0: mask_of[nq] as for the masked searches above --
 * 0xFFFFFFFF = no mask, NULL = plane 0 for every query; an entry >= nmasks or no planes resident -> NVDB_ERR_INVALID before
 * anything is launched, nothing written.
 * k == 0 or nq == 0 -> NVDB_OK, nothing written.  nprobe == 0 -> every count 0, outputs all padding.  No partition table ->
 * NVDB_ERR_INVALID; no corpus -> NVDB_ERR_NO_CORPUS.  Non-finite query or corpus values: no fault, no hang, order unspecified
 * (for k > 64 a row whose score is NaN is no candidate, as in the range search: it is neither returned nor counted).
 * Any nq: for k > 64 the batch is cut into query sub-batches whose candidate blocks (8 bytes per row of a query's probed union)
 * stay within half of option "largek_budget_mb", the key slabs of lists longer than 8192 entries within the other half, and the
 * device copy of the results within as many entries as the blocks may hold; one query is taken whatever the option says; the
 * caller does not see the cut.  A single query whose union reaches 2^32 rows, or more than 2^31 results for one query ->
 * NVDB_ERR_UNSUPPORTED.
 * nvdb_hip_get_stats afterwards (k > 64): path = 8, chunks = scan launches, rows_scanned = rows of the work items (live or not),
 * candidates = non-padding entries of the candidate blocks (the live rows of the unions).  timing (optional): kernel / total as for
 * nvdb_hip_range_search_partitions (the work list's copies and the results' alternate with the launches and ride inside).
 * Cost, plainly: the scan of nvdb_hip_range_search_partitions at radius -inf -- every live row of the union is scored and written
 * once, nothing is pruned inside the scan --, then per query one workgroup that reads its block once per radix pass, and k results
 * copied back instead of the union.
 * Out of scope, unchanged: the masked flat search with k > 64 (nvdb_hip_search_batch_masked), the device group, _dev stream forms
 * of these calls, any pruning inside the scan.
 * ------------------------------------------------------------------------------------------- */

/* probe[nq][nprobe]: nvdb_hip_search_partitions' rules (0xFFFFFFFF = empty slot, duplicates count once, an entry >= nparts ->
 * NVDB_ERR_INVALID before anything is launched, nothing written). */
nvdb_status nvdb_hip_search_partitions_anyk(nvdb_hip_ctx* ctx, const float* queries, uint32_t nq, uint32_t k,
                                            const uint32_t* probe /* [nq][nprobe] */, uint32_t nprobe,
                                            const uint32_t* mask_of /* [nq], may be NULL */, int masked,
                                            uint64_t* out_ids /* [nq][k] */, float* out_scores /* [nq][k] */,
                                            uint32_t* out_counts /* [nq], may be NULL */, nvdb_hip_timing* timing /* may be NULL */);
/* The coarse step, the clamp of nprobe and out_probe (optional, [nq][nprobe]) are nvdb_hip_search_ivf's; centroids are not masked.
 * Without centroids -> NVDB_ERR_INVALID. */
nvdb_status nvdb_hip_search_ivf_anyk(nvdb_hip_ctx* ctx, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                                     const uint32_t* mask_of /* [nq], may be NULL */, int masked,
                                     uint64_t* out_ids /* [nq][k] */, float* out_scores /* [nq][k] */,
                                     uint32_t* out_counts /* [nq], may be NULL */, uint32_t* out_probe /* may be NULL */,
                                     nvdb_hip_timing* timing /* may be NULL */);

/* ---------------------------------------------------------------------------------------------
 * IVF-Flat build: from a resident corpus to an index the probe search above can serve -- centroids trained on the GPU
 * (the reference trains them with FAISS, apps/nvdb_ivf_build.cpp:59-64), every row assigned to its best centroid, the rows
 * copied into list order, results answered in the ORIGINAL ids.
 * "A row as an f32 query" below means: an f32 row as it is, an f16 row widened exactly, an int8 row float(x) * scale
 * rounded once.
 * ------------------------------------------------------------------------------------------- */

/* out_assign[i] (host, nrows entries) = the centroid with the largest dot product with resident row row0 + i taken as an f32
 * query, in the reference's fp32 order (the flat search over the centroids: the bits of nvdb_hip_search_batch on an f32 corpus);
 * ties go to the lowest centroid number.  centroids: [nparts][dim] f32, host memory.
 * NVDB_ERR_INVALID: null context / centroids, null out_assign with nrows > 0, nparts == 0 or 0xFFFFFFFF, row0 + nrows > n;
 * NVDB_ERR_NO_CORPUS: nothing resident.  nrows == 0 -> NVDB_OK, nothing written.
 * Non-finite rows or centroids: no fault, no hang, every output < nparts, the value otherwise unspecified. */
nvdb_status nvdb_hip_assign_rows(nvdb_hip_ctx* ctx, const float* centroids, uint32_t nparts,
                                 uint64_t row0, uint64_t nrows, uint32_t* out_assign);

/* Spherical k-means (the companion of search_ivf's dot-product probe): a centroid is the mean of its members scaled to unit
 * length.  out_centroids: [nparts][dim] f32, host memory.  Same arguments + same corpus -> the same bytes (no atomics).
 *   training set: every resident row when max_train_rows == 0 or >= n, else the m = max_train_rows rows floor(i * n / m), i < m.
 *                 nparts > training rows -> NVDB_ERR_INVALID.
 *   start:        init ([nparts][dim] f32, host) as given; NULL: nparts DISTINCT training rows, each as an f32 query scaled to
 *                 unit length in fp64 (one rounding to f32).  Draw rule for centroid j, attempt t = 0, 1, ...: with mix32 and
 *                 synth_row_key the synthetic generator's mixers,
 *                   key = synth_row_key(seed, (uint64) t << 32 | j),
 *                   training row = (((uint64) mix32(key ^ 0x9E3779B9) << 32) | mix32(key + 0x85EBCA6B)) mod m;
 *                 a row some centroid < j already took is drawn again; after 64 attempts the next free training row
 *                 (wrapping at m) is taken.  iters == 0 returns the start.
 *   iteration:    assign the training rows (nvdb_hip_assign_rows' rule); per centroid, sum the members per column in fp64 in
 *                 ascending row order (lists longer than 512 rows: per 512-row chunk, the chunks added in order); the norm in
 *                 fp64; centroid = sum / norm rounded once to f32.  A centroid without members, or with a zero or non-finite
 *                 sum, keeps its value. */
nvdb_status nvdb_hip_train_centroids(nvdb_hip_ctx* ctx, uint32_t nparts, uint32_t iters, uint64_t seed,
                                     uint64_t max_train_rows, const float* init, float* out_centroids);

/* The inverted lists of an assignment (host, no GPU needed): a stable counting sort.  out_offsets[p] (nparts + 1 entries) =
 * first position of list p, out_perm[j] (n entries) = the original row at position j; positions are ordered by partition, then
 * by original row.  NVDB_ERR_INVALID with nothing written: a null pointer, n > 0xFFFFFF00, an entry >= nparts.
 * n == 0 -> every offset 0. */
nvdb_status nvdb_ivf_layout_host(const uint32_t* assign, uint64_t n, uint32_t nparts,
                                 uint64_t* out_offsets /* nparts+1 */, uint32_t* out_perm /* n */);

/* The index: the rows of `src` copied into list order (nvdb_hip_assign_rows -> nvdb_ivf_layout_host -> a permuting copy,
 * int8 scales included) into a context of its own on the same device, with the partition table and the centroids set.
 * src is not touched and may be destroyed afterwards to give its HBM back; DURING the build the device holds the source
 * AND the copy (plus shadows of both where the dtype / dim has them).  Options that act when a corpus becomes resident
 * ("f32_shadow", "q8_shadow" = 1; the automatic shadow serves the flat scan only) are taken over from src.  The index's context has global_row_base 0; src's base is kept and
 * added when ids are mapped back.  NVDB_ERR_NO_CORPUS: src holds no corpus.
 * NVDB_IVF_DEBUG (environment): build / train report their assignment / update / gather hipEvent times on stderr. */
typedef struct nvdb_hip_ivf nvdb_hip_ivf;
nvdb_status nvdb_hip_ivf_build(nvdb_hip_ctx* src, const float* centroids, uint32_t nparts, nvdb_hip_ivf** out);
void nvdb_hip_ivf_destroy(nvdb_hip_ivf* ivf);
const char* nvdb_hip_ivf_last_error(const nvdb_hip_ivf* ivf);     /* NULL: last build error */
/* the index's own context (options, statistics, download_rows: the rows in list order); owned by the index */
nvdb_hip_ctx* nvdb_hip_ivf_ctx(nvdb_hip_ivf* ivf);
/* offsets_out (nparts + 1) / perm_out (n) may be NULL; perm[position] = row of src (without its global_row_base) */
nvdb_status nvdb_hip_ivf_info(const nvdb_hip_ivf* ivf, uint64_t* n, uint32_t* nparts,
                              uint64_t* offsets_out, uint32_t* perm_out);
/* nvdb_hip_search_ivf on the index's context, then every id that is not padding becomes src's global_row_base + perm[id].
 * Scores and their bits are the probe search's.  ORDER: score descending; equal scores by (partition number, original id) --
 * the order of the positions in the lists; the result is not re-sorted by original id.  out_probe, out_counts, timing and the
 * k > 64, nprobe == 0, k == 0 rules are nvdb_hip_search_ivf's. */
nvdb_status nvdb_hip_ivf_search(nvdb_hip_ivf* ivf, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                                uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                uint32_t* out_probe, nvdb_hip_timing* timing);

/* Row masks of an index, in ORIGINAL rows (rows of src, without its global_row_base).  bits: [nmasks][ceil(n / 32)] as for
 * nvdb_hip_set_row_masks; position j of the index is live iff bit perm[j] is set (NULL: every row live).  Errors as there. */
nvdb_status nvdb_hip_ivf_set_row_masks(nvdb_hip_ivf* ivf, const uint32_t* bits, uint32_t nmasks);
/* nvdb_hip_update_row_mask with original rows: mapped through the inverse permutation, which is built once, on first use. */
nvdb_status nvdb_hip_ivf_update_row_mask(nvdb_hip_ivf* ivf, uint32_t mask, const uint64_t* rows, uint64_t nrows, int live);
/* nvdb_hip_search_ivf_masked on the index's context, then the id mapping and the ORDER of nvdb_hip_ivf_search: equal scores by
 * (partition number, original id). */
nvdb_status nvdb_hip_ivf_search_masked(nvdb_hip_ivf* ivf, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                                       const uint32_t* mask_of /* [nq], may be NULL */,
                                       uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                       uint32_t* out_probe, nvdb_hip_timing* timing);

/* nvdb_hip_search_ivf_anyk on the index's context (any k; mask_of names planes set with nvdb_hip_ivf_set_row_masks, original rows),
 * then the id mapping and the ORDER of nvdb_hip_ivf_search: every id that is not padding becomes src's global_row_base + perm[id];
 * equal scores by (partition number, original id) -- the select orders equal scores by position in the lists, not by the mapped id. */
nvdb_status nvdb_hip_ivf_search_anyk(nvdb_hip_ivf* ivf, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                                     const uint32_t* mask_of /* [nq], may be NULL */, int masked,
                                     uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                     uint32_t* out_probe, nvdb_hip_timing* timing);

/* nvdb_hip_range_search_ivf on the index's context; mask_of names planes set with nvdb_hip_ivf_set_row_masks (original rows).
 * The lims are final; the slices are held by the index's context in list positions. */
nvdb_status nvdb_hip_ivf_range_search(nvdb_hip_ivf* ivf, const float* queries, uint32_t nq, const float* radius /* [nq] */,
                                      uint32_t nprobe, const uint32_t* mask_of /* [nq], may be NULL */, int masked,
                                      uint64_t* out_lims /* [nq+1] */, uint32_t* out_probe /* may be NULL */,
                                      nvdb_hip_timing* timing /* may be NULL */);
/* nvdb_hip_range_results on the index's context, then every id becomes src's global_row_base + perm[id], as nvdb_hip_ivf_search
 * maps them.  ORDER inside a slice: score descending; equal scores by (partition number, original id) -- the order of the
 * positions in the lists. */
nvdb_status nvdb_hip_ivf_range_results(nvdb_hip_ivf* ivf, uint64_t* out_ids, float* out_scores);

/* Tunables (defaults are what bench.py measures; the table with meanings is in INTEGRATION.md section 4b):
 * "path" (0 auto, 1 exact, 2 mfma-filter), "chunk0_rows", "chunk_growth", "cand_cap", "min_filter_batch", "mfma_boot", "waves8",
 * "sibling_sync", "sync_every", "sync_lead", "tile_permute", "f32_shadow", "q8_shadow" (-1 automatic, 0 never, 1 always),
 * "q8_auto_min_rows", "q8_auto_max_mb" (all set before the upload), "shadow_exact_thr" (1: a search that streams the int8 shadow
 * takes its thresholds from exact scores of its best 2k candidates, one error bound under them; 0: two bounds under the k-th filter score), "exact_mfma" (exact scores on the fp32
 * matrix cores), "exact_lds", "i8_dense8" (int8 filter, d = 768, batches > 128: 1 = 8 waves of 32 queries per workgroup, 0 = 4 of 64; same results), "i8_defer", "i8_lo_bits", "boot_tiles", "xcd_balance", "rescore8", "refine_v2", "refine_pinned" (reference CUDA_PINNED:
 * pinned host staging in nvdb_hip_refine_l2_topk), "largek_budget_mb" (HBM for the any-k path's score matrix), "range_max_mb" (packed results a range search may hold), "compact_slab_rows" (rows per slab of nvdb_hip_compact_rows' walk and of nvdb_hip_insert_rows' -- the same option: a multiple of 64 in [64, 2^24], default 65536), "insert_growth_pct" (an insertion that outgrows the arrays' capacity reallocates them to max(n + m, capacity * (100 + this) / 100) rows: [0, 400], default 50, 0 = exactly n + m), "time_kernels" (1: start /
 * stop events attached to every launch of the dominant kernel, read by nvdb_hip_collect_kernel_times), "time_launches" (the same for one host-API
 * call with a timing struct -> stats.filter_kernel_ms).  "mfma16", "i8_wide", "i8_pipe", "i8_waves8", "i8_mfma16", "i8_small8" select kernel
 * variants that exist in libnvdb_hip_dev.so only: the product accepts their default values (1, 1, 1, 0, 1) and returns
 * NVDB_ERR_UNSUPPORTED for the others.  Unknown key -> NVDB_ERR_INVALID. */
nvdb_status nvdb_hip_set_option(nvdb_hip_ctx* ctx, const char* key, int64_t value);

/* With "time_kernels" = 1: sum of the hipEvent durations of the dominant (filter) kernel's launches
 * since the last call, with their algorithmic flops (2 * queries * rows * dim) and corpus bytes
 * (rows * dim * bytes/elem).  Synchronises on the recorded events.  bench.py's roofline uses it. */
nvdb_status nvdb_hip_collect_kernel_times(nvdb_hip_ctx* ctx, uint32_t* launches, double* total_ms,
                                          double* total_flops, double* total_bytes);

/* ---------------------------------------------------------------------------------------------
 * exact-L2 refine (rerank of R candidates per query) -- replaces nvdb::cuda_l2_topk_batch
 * (include/nvdb/cuda_refine.h:25-38, src/cuda_refine.cu:839-1173) on the resident corpus
 * ------------------------------------------------------------------------------------------- */

/* queries [Q][dim] f32, cand_ids [Q][R] u32 local row ids (0xFFFFFFFF or >= n are skipped,
 * cuda_refine.cu:437).  out_ids [Q][K] ascending by squared L2 distance, padded with 0xFFFFFFFF;
 * out_dist [Q][K] padded with 1e30f, or NULL for ids only (CUDA_RETURN_DIST=0, :876).
 * Distances use the reference kernel's fp32 order (cuda_refine.cu:326-382 for f16 rows,
 * :383-392 for f32 rows -- the latter is implemented properly; the reference never launches it,
 * :1055-1085).  Corpus dtype must be F16 or F32 (apps/nvdb_ivf_eval.cpp:519-525).
 * K == 0 || Q == 0 || R == 0 -> NVDB_OK with zeroed timing (:853-857); K > 64 -> INVALID (:858-862). */
nvdb_status nvdb_hip_refine_l2_topk(nvdb_hip_ctx* ctx, const float* queries, const uint32_t* cand_ids,
                                    uint32_t Q, uint32_t R, uint32_t K, uint32_t* out_ids, float* out_dist,
                                    nvdb_hip_timing* timing);
nvdb_status nvdb_hip_refine_l2_topk_dev(nvdb_hip_ctx* ctx, const float* dev_queries, const uint32_t* dev_cand_ids,
                                        uint32_t Q, uint32_t R, uint32_t K, uint32_t* dev_out_ids,
                                        float* dev_out_dist, void* hip_stream);

/* ---------------------------------------------------------------------------------------------
 * host-side helpers that define the corpus bits (no GPU needed)
 * ------------------------------------------------------------------------------------------- */

/* Synthetic rows [row0,row0+nrows) as fp32 (the generator nvdb_hip_generate_corpus runs on device). */
void nvdb_synth_rows_f32(uint64_t seed, uint64_t row0, uint64_t nrows, uint32_t dim, float* out);
/* fp32 -> IEEE half, round-to-nearest-even (tools/nvdb_convert_f16.cpp:99-107, the F16C path). */
void nvdb_f32_to_f16(const float* src, uint16_t* dst, uint64_t n);
/* per-row int8 quantisation (apps/nvdb_quantize_i8.cpp:12-16, 71-80). */
void nvdb_quantize_i8_rows(const float* rows, uint64_t nrows, uint32_t dim, int8_t* out, float* scales);

#ifdef __cplusplus
}
#endif
#endif /* NVDB_HIP_H */
