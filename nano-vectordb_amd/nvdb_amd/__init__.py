"""nvdb_amd -- thin ctypes binding of libnvdb_hip.so (include/nvdb_hip.h).

This is plumbing for the tests and bench.py; the product is the C-ABI library and the C++ host
layer.  There is no CPU implementation behind this module: if the HIP library is missing, or no
GPU is present when a computation is requested, the call raises.

Names follow the reference's host API: `FlatIndexHIP.search_topk_dot` mirrors
nvdb::FlatIndex::search_topk_dot (reference include/nvdb/flat_index.h:11-13), `l2_topk_batch`
mirrors nvdb::cuda_l2_topk_batch (include/nvdb/cuda_refine.h:25-38).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libnvdb_hip.so")
DEV_LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libnvdb_hip_dev.so")   # developer build: + nvdb_hip_debug_* (include/nvdb_hip_dev.h)

DT_F32, DT_F16, DT_I8 = 1, 2, 3
REFINE_KMAX = 64
_NP_OF = {DT_F32: np.float32, DT_F16: np.uint16, DT_I8: np.int8}

EXPORTS = [
    "nvdb_hip_abi_version", "nvdb_hip_device_count", "nvdb_hip_create", "nvdb_hip_destroy", "nvdb_hip_last_error",
    "nvdb_hip_upload_corpus", "nvdb_hip_adopt_corpus", "nvdb_hip_generate_corpus", "nvdb_hip_corpus_info",
    "nvdb_hip_download_rows", "nvdb_hip_search_batch", "nvdb_hip_search_batch_dev", "nvdb_hip_search_check",
    "nvdb_hip_get_stats", "nvdb_hip_range_search", "nvdb_hip_range_results", "nvdb_hip_shadow_info", "nvdb_hip_shadow_scale_info", "nvdb_hip_collect_kernel_times", "nvdb_hip_merge_topk_dev", "nvdb_hip_merge_topk_strided_dev", "nvdb_merge_topk_host", "nvdb_hip_set_option",
    "nvdb_hip_refine_l2_topk", "nvdb_hip_refine_l2_topk_dev", "nvdb_synth_rows_f32", "nvdb_f32_to_f16",
    "nvdb_quantize_i8_rows",
    "nvdb_hip_group_create", "nvdb_hip_group_destroy", "nvdb_hip_group_last_error", "nvdb_hip_group_size", "nvdb_hip_group_ctx",
    "nvdb_hip_group_exchange", "nvdb_hip_group_upload_corpus", "nvdb_hip_group_generate_corpus", "nvdb_hip_group_set_option",
    "nvdb_hip_group_search_batch",
    "nvdb_hip_set_partitions", "nvdb_hip_set_centroids", "nvdb_hip_search_partitions", "nvdb_hip_search_ivf",
    "nvdb_hip_assign_rows", "nvdb_hip_train_centroids", "nvdb_ivf_layout_host",
    "nvdb_hip_ivf_build", "nvdb_hip_ivf_destroy", "nvdb_hip_ivf_last_error", "nvdb_hip_ivf_ctx", "nvdb_hip_ivf_info", "nvdb_hip_ivf_search",
    "nvdb_hip_set_row_masks", "nvdb_hip_update_row_mask", "nvdb_hip_get_row_masks", "nvdb_hip_search_partitions_masked",
    "nvdb_hip_search_ivf_masked", "nvdb_hip_search_batch_masked",
    "nvdb_hip_ivf_set_row_masks", "nvdb_hip_ivf_update_row_mask", "nvdb_hip_ivf_search_masked",
    "nvdb_hip_range_search_partitions", "nvdb_hip_range_search_ivf", "nvdb_hip_range_search_masked",
    "nvdb_hip_ivf_range_search", "nvdb_hip_ivf_range_results",
    "nvdb_hip_search_partitions_anyk", "nvdb_hip_search_ivf_anyk", "nvdb_hip_ivf_search_anyk",
    "nvdb_hip_compact_rows", "nvdb_hip_ivf_compact",
    "nvdb_hip_reserve_rows", "nvdb_hip_insert_rows", "nvdb_hip_ivf_add_rows",
]
# only in libnvdb_hip_dev.so; the product library must NOT export them (tests/test_cabi_cpu.py)
DEV_EXPORTS = ["nvdb_hip_debug_clock", "nvdb_hip_debug_clock_i8", "nvdb_permuted_tile", "nvdb_hip_debug_tile_ranges",
               "nvdb_hip_debug_plan"]


class NvdbError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"nvdb_hip status {status}: {msg}")
        self.status = status


class Timing(C.Structure):
    _fields_ = [("h2d_ms", C.c_float), ("kernel_ms", C.c_float), ("d2h_ms", C.c_float), ("total_ms", C.c_float),
                ("threads", C.c_uint32), ("nwarps", C.c_uint32), ("K", C.c_uint32), ("R", C.c_uint32),
                ("shmem_bytes", C.c_size_t), ("dbg_q", C.c_uint32),
                ("dbg_dist_cycles_avg", C.c_double), ("dbg_write_cycles_avg", C.c_double),
                ("dbg_merge_cycles_avg", C.c_double), ("dbg_dist_pct", C.c_double), ("dbg_write_pct", C.c_double),
                ("dbg_merge_pct", C.c_double)]


class ScanStats(C.Structure):
    _fields_ = [("path", C.c_uint32), ("chunks", C.c_uint32), ("rows_scanned", C.c_uint64), ("candidates", C.c_uint64),
                ("overflow_queries", C.c_uint32), ("bound_violations", C.c_uint32), ("filter_kernel_ms", C.c_float),
                ("other_kernel_ms", C.c_float), ("i8_stage1_tiles", C.c_uint32), ("i8_stage2_blocks", C.c_uint32),
                ("sticky_overflow", C.c_uint32), ("sticky_violations", C.c_uint32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class PlanShape(C.Structure):
    _fields_ = [("n", C.c_uint64), ("dim", C.c_uint32), ("fdim", C.c_uint32), ("dtype", C.c_uint32), ("owned", C.c_uint32),
                ("has_shadow16", C.c_uint32), ("has_shadow8", C.c_uint32), ("q8shadow", C.c_uint32), ("i8_scales_signed", C.c_uint32),
                ("num_cu", C.c_uint32), ("cap_hint", C.c_uint32), ("shadow_demoted", C.c_uint32), ("load_rule", C.c_uint32),
                ("free_hbm", C.c_uint64)]


class PlanOption(C.Structure):
    _fields_ = [("key", C.c_char_p), ("value", C.c_int64)]


PLAN_MAX_CHUNKS = 64


class Plan(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("route", "prep", "prep_inits", "k_wide", "k_eff", "cap", "QPB", "QT", "nq_pad", "prog_words", "head",
                                          "padded", "perm_on", "boot", "tile_rows", "n_al", "growth", "boot_tiles", "boot_rows", "r0",
                                          "tail_exact", "helper_tile_rows", "n_chunks")] + \
               [("chunk_lo", C.c_uint32 * PLAN_MAX_CHUNKS), ("chunk_hi", C.c_uint32 * PLAN_MAX_CHUNKS), ("stat_chunks", C.c_uint32),
                ("stat_rows_scanned", C.c_uint64), ("filter_shadow", C.c_uint32)]


class GroupStats(C.Structure):
    _fields_ = [("shards", C.c_uint32), ("exchange", C.c_uint32), ("host_merge_fallbacks", C.c_uint32), ("bytes_per_rank", C.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


_lib = None
_dev_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64.so.7; libnvdb_hip.so is linked
    against /opt/rocm's, which has the same soname.  Whichever is loaded first serves both, and torch cannot
    initialise ("No HIP GPUs are available") on top of /opt/rocm's.  bench.py and the tests share device
    buffers and streams with torch, so when torch is installed its runtime is loaded first -- without importing
    torch.  Stand-alone C++ users of libnvdb_hip.so (the tools in bin/) are unaffected."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def _share_rccl_with_torch():
    """Same for RCCL, which the device group binds with dlopen("librccl.so.1") on first use: PyTorch's bundled copy is built
    against PyTorch's HIP runtime, so it is the one to have in the process.  PyTorch is IMPORTED for that (only DeviceGroup
    does this): a bare dlopen of its librccl.so ahead of a later `import torch` changed the order in which the two tear their
    statics down and aborted the interpreter at exit ("double free or corruption") once both had been used."""
    import importlib.util
    if importlib.util.find_spec("torch") is None:
        return
    import torch  # noqa: F401  (loads libamdhip64 / librccl in its own order)


def _bind(L, dev):
    vp, u32, u64, i64, f32p = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int64, C.POINTER(C.c_float)
    L.nvdb_hip_abi_version.restype = C.c_int
    L.nvdb_hip_device_count.restype = C.c_int
    L.nvdb_hip_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.nvdb_hip_destroy.argtypes = [vp]
    L.nvdb_hip_destroy.restype = None
    L.nvdb_hip_last_error.argtypes = [vp]
    L.nvdb_hip_last_error.restype = C.c_char_p
    L.nvdb_hip_upload_corpus.argtypes = [vp, vp, vp, u64, u32, u32, u64]
    L.nvdb_hip_adopt_corpus.argtypes = [vp, vp, vp, u64, u32, u32, u64]
    L.nvdb_hip_generate_corpus.argtypes = [vp, u64, u64, u32, u32, u64]
    L.nvdb_hip_corpus_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u32), C.POINTER(u32), C.POINTER(u64), f32p]
    L.nvdb_hip_download_rows.argtypes = [vp, u64, u64, vp, vp]
    L.nvdb_hip_search_batch.argtypes = [vp, vp, u32, u32, vp, vp, C.POINTER(u32), C.POINTER(Timing)]
    L.nvdb_hip_search_batch_dev.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.nvdb_hip_search_check.argtypes = [vp, C.POINTER(ScanStats)]
    L.nvdb_hip_get_stats.argtypes = [vp, C.POINTER(ScanStats)]
    L.nvdb_hip_range_search.argtypes = [vp, vp, u32, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_range_results.argtypes = [vp, vp, vp]
    L.nvdb_hip_shadow_info.argtypes = [vp, C.POINTER(u64)]
    L.nvdb_hip_shadow_scale_info.argtypes = [vp, C.POINTER(C.c_double)]
    L.nvdb_hip_collect_kernel_times.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                C.POINTER(C.c_double)]
    L.nvdb_hip_merge_topk_dev.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp, vp]
    L.nvdb_hip_merge_topk_strided_dev.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, u32, u32, u32, vp, vp, vp]
    L.nvdb_merge_topk_host.argtypes = [vp, vp, u32, u32, u32, vp, vp]
    L.nvdb_hip_set_option.argtypes = [vp, C.c_char_p, i64]
    L.nvdb_hip_refine_l2_topk.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_refine_l2_topk_dev.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp, vp]
    L.nvdb_synth_rows_f32.argtypes = [u64, u64, u64, u32, vp]
    L.nvdb_synth_rows_f32.restype = None
    L.nvdb_f32_to_f16.argtypes = [vp, vp, u64]
    L.nvdb_f32_to_f16.restype = None
    L.nvdb_quantize_i8_rows.argtypes = [vp, u64, u32, vp, vp]
    L.nvdb_quantize_i8_rows.restype = None
    L.nvdb_hip_group_create.argtypes = [C.POINTER(C.c_int), u32, C.POINTER(vp)]
    L.nvdb_hip_group_destroy.argtypes = [vp]
    L.nvdb_hip_group_destroy.restype = None
    L.nvdb_hip_group_last_error.argtypes = [vp]
    L.nvdb_hip_group_last_error.restype = C.c_char_p
    L.nvdb_hip_group_size.argtypes = [vp]
    L.nvdb_hip_group_size.restype = u32
    L.nvdb_hip_group_ctx.argtypes = [vp, u32]
    L.nvdb_hip_group_ctx.restype = vp
    L.nvdb_hip_group_exchange.argtypes = [vp, C.POINTER(C.c_char_p)]
    L.nvdb_hip_group_exchange.restype = C.c_int
    L.nvdb_hip_group_upload_corpus.argtypes = [vp, vp, vp, u64, u32, u32]
    L.nvdb_hip_group_generate_corpus.argtypes = [vp, u64, u64, u32, u32]
    L.nvdb_hip_group_set_option.argtypes = [vp, C.c_char_p, i64]
    L.nvdb_hip_group_search_batch.argtypes = [vp, vp, u32, u32, vp, vp, C.POINTER(u32), C.POINTER(GroupStats)]
    L.nvdb_hip_set_partitions.argtypes = [vp, vp, u32]
    L.nvdb_hip_set_centroids.argtypes = [vp, vp]
    L.nvdb_hip_search_partitions.argtypes = [vp, vp, u32, u32, vp, u32, vp, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_search_ivf.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_assign_rows.argtypes = [vp, vp, u32, u64, u64, vp]
    L.nvdb_hip_train_centroids.argtypes = [vp, u32, u32, u64, u64, vp, vp]
    L.nvdb_ivf_layout_host.argtypes = [vp, u64, u32, vp, vp]
    L.nvdb_hip_ivf_build.argtypes = [vp, vp, u32, C.POINTER(vp)]
    L.nvdb_hip_ivf_destroy.argtypes = [vp]
    L.nvdb_hip_ivf_destroy.restype = None
    L.nvdb_hip_ivf_last_error.argtypes = [vp]
    L.nvdb_hip_ivf_last_error.restype = C.c_char_p
    L.nvdb_hip_ivf_ctx.argtypes = [vp]
    L.nvdb_hip_ivf_ctx.restype = vp
    L.nvdb_hip_ivf_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u32), vp, vp]
    L.nvdb_hip_ivf_search.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_set_row_masks.argtypes = [vp, vp, u32]
    L.nvdb_hip_update_row_mask.argtypes = [vp, u32, vp, u64, C.c_int]
    L.nvdb_hip_get_row_masks.argtypes = [vp, C.POINTER(u32), C.POINTER(u64), vp]
    L.nvdb_hip_search_partitions_masked.argtypes = [vp, vp, u32, u32, vp, u32, vp, vp, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_search_ivf_masked.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_search_batch_masked.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_ivf_set_row_masks.argtypes = [vp, vp, u32]
    L.nvdb_hip_ivf_update_row_mask.argtypes = [vp, u32, vp, u64, C.c_int]
    L.nvdb_hip_ivf_search_masked.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_range_search_partitions.argtypes = [vp, vp, u32, vp, vp, u32, vp, C.c_int, vp, C.POINTER(Timing)]
    L.nvdb_hip_range_search_ivf.argtypes = [vp, vp, u32, vp, u32, vp, C.c_int, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_range_search_masked.argtypes = [vp, vp, u32, vp, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_ivf_range_search.argtypes = [vp, vp, u32, vp, u32, vp, C.c_int, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_ivf_range_results.argtypes = [vp, vp, vp]
    L.nvdb_hip_search_partitions_anyk.argtypes = [vp, vp, u32, u32, vp, u32, vp, C.c_int, vp, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_search_ivf_anyk.argtypes = [vp, vp, u32, u32, u32, vp, C.c_int, vp, vp, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_ivf_search_anyk.argtypes = [vp, vp, u32, u32, u32, vp, C.c_int, vp, vp, vp, vp, C.POINTER(Timing)]
    L.nvdb_hip_compact_rows.argtypes = [vp, u32, C.POINTER(u64), vp]
    L.nvdb_hip_ivf_compact.argtypes = [vp, u32, C.POINTER(u64)]
    L.nvdb_hip_reserve_rows.argtypes = [vp, u64]
    L.nvdb_hip_insert_rows.argtypes = [vp, vp, vp, u64, vp, vp, C.POINTER(u64)]
    L.nvdb_hip_ivf_add_rows.argtypes = [vp, vp, vp, u64, C.POINTER(u64), vp]
    for name in EXPORTS:
        getattr(L, name)
    if dev:
        L.nvdb_hip_debug_clock.argtypes = [vp, C.c_int, u32, C.c_float, f32p]
        L.nvdb_hip_debug_clock_i8.argtypes = [vp, C.c_int, u32, C.c_float, f32p]
        L.nvdb_permuted_tile.argtypes = [u32, u32]
        L.nvdb_hip_debug_tile_ranges.argtypes = [vp, u32, u32, f32p, C.POINTER(u32), C.POINTER(u32), f32p]
        L.nvdb_permuted_tile.restype = u32
        L.nvdb_hip_debug_plan.argtypes = [C.POINTER(PlanShape), C.POINTER(PlanOption), u32, u32, u32, C.c_int, u32, C.POINTER(Plan), C.c_char_p, C.c_size_t]
    return L


def load_library():
    """Load libnvdb_hip.so (the product library); raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C nano-vectordb_amd` "
                          "(python -c 'import __graft_entry__ as g; g.build()')")
    _share_hip_runtime_with_torch()
    _lib = _bind(C.CDLL(LIB_PATH), dev=False)
    return _lib


def load_dev_library():
    """Load libnvdb_hip_dev.so: the same ABI plus the developer entry points (tools_dev/ only)."""
    global _dev_lib
    if _dev_lib is not None:
        return _dev_lib
    if not os.path.exists(DEV_LIB_PATH):
        raise ImportError(f"{DEV_LIB_PATH} is missing: build it with `make -C nano-vectordb_amd`")
    _share_hip_runtime_with_torch()
    _dev_lib = _bind(C.CDLL(DEV_LIB_PATH), dev=True)
    return _dev_lib


# ------------------------------------------------------------------------------- host-side helpers (no GPU)
def synth_rows_f32(seed, row0, nrows, dim):
    out = np.empty((nrows, dim), dtype=np.float32)
    load_library().nvdb_synth_rows_f32(seed, row0, nrows, dim, out.ctypes.data)
    return out


def f32_to_f16(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty(x.shape, dtype=np.uint16)
    load_library().nvdb_f32_to_f16(x.ctypes.data, out.ctypes.data, x.size)
    return out


def quantize_i8(rows):
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    out = np.empty(rows.shape, dtype=np.int8)
    scales = np.empty(rows.shape[0], dtype=np.float32)
    load_library().nvdb_quantize_i8_rows(rows.ctypes.data, rows.shape[0], rows.shape[1], out.ctypes.data,
                                         scales.ctypes.data)
    return out, scales


def synth_corpus(seed, row0, nrows, dim, dtype):
    """CPU twin of HipContext.generate_corpus (same bits)."""
    f = synth_rows_f32(seed, row0, nrows, dim)
    if dtype == DT_F32:
        return f, None
    if dtype == DT_F16:
        return f32_to_f16(f), None
    return quantize_i8(f)


def debug_plan(shape, nq, k, options=None, force_path=0, cap_override=0):
    """What a flat search of nq queries for the k best would do on a corpus of `shape` (the PlanShape fields as a dict; fdim
    defaults to dim): nvdb_hip_debug_plan of the developer library, as a dict with the chunk lists cut to n_chunks."""
    sh = PlanShape(**{"fdim": shape["dim"], **shape})
    items = list((options or {}).items())
    opts = (PlanOption * max(len(items), 1))(*[PlanOption(key.encode(), int(v)) for key, v in items])
    out, err = Plan(), C.create_string_buffer(256)
    st = load_dev_library().nvdb_hip_debug_plan(C.byref(sh), opts, len(items), nq, k, force_path, cap_override, C.byref(out), err, len(err))
    if st:
        raise NvdbError(st, err.value.decode())
    p = {f: getattr(out, f) for f, _ in Plan._fields_}
    p["chunk_lo"], p["chunk_hi"] = list(out.chunk_lo[:out.n_chunks]), list(out.chunk_hi[:out.n_chunks])
    return p


def merge_topk_host(ids, scores):
    """ids/scores: [nshards, nq, k] -> ([nq,k],[nq,k]) in (score desc, id asc) order."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    s, nq, k = ids.shape
    oi = np.empty((nq, k), dtype=np.uint64)
    os_ = np.empty((nq, k), dtype=np.float32)
    st = load_library().nvdb_merge_topk_host(ids.ctypes.data, scores.ctypes.data, s, nq, k, oi.ctypes.data,
                                             os_.ctypes.data)
    if st:
        raise NvdbError(st, "merge_topk_host")
    return oi, os_


def ivf_layout_host(assign, nparts):
    """assign: [n] partition numbers -> (offsets [nparts + 1] u64, perm [n] u32): the lists ordered by partition, then by row."""
    assign = np.ascontiguousarray(assign, dtype=np.uint32).ravel()
    offsets = np.zeros(nparts + 1, dtype=np.uint64)
    perm = np.zeros(max(assign.size, 1), dtype=np.uint32)
    st = load_library().nvdb_ivf_layout_host(assign.ctypes.data if assign.size else perm.ctypes.data, assign.size, nparts,
                                             offsets.ctypes.data, perm.ctypes.data)
    if st:
        raise NvdbError(st, "ivf_layout_host: an entry >= nparts, or more than 0xFFFFFF00 rows")
    return offsets, perm[:assign.size]


def pack_row_masks(masks, n):
    """Row masks as the library takes them: [nmasks, ceil(n / 32)] uint32, row r = bit r & 31 of word r >> 5.  `masks`: bool
    [nmasks, n] (or [n]: one mask), or uint32 already packed."""
    masks = np.asarray(masks)
    words = (n + 31) // 32
    if masks.dtype == np.uint32:
        return np.ascontiguousarray(masks).reshape(-1, words)
    if masks.dtype != np.bool_:
        raise TypeError("row masks are bool [nmasks, n] or packed uint32 [nmasks, ceil(n / 32)]")
    masks = masks.reshape(-1, n)
    packed = np.zeros((masks.shape[0], words * 4), dtype=np.uint8)
    packed[:, :(n + 7) // 8] = np.packbits(masks, axis=1, bitorder="little")
    return np.ascontiguousarray(packed).view("<u4")


def unpack_row_masks(packed, n):
    """The inverse: packed uint32 [nmasks, ceil(n / 32)] -> bool [nmasks, n]."""
    packed = np.ascontiguousarray(packed, dtype="<u4")
    return np.unpackbits(packed.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def _mask_of_arg(mask_of, nq):
    """mask_of for a masked search: None (every query plane 0) or one plane number per query (0xFFFFFFFF: no mask)."""
    if mask_of is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(mask_of, dtype=np.uint32), (nq,)))


def _range_call(owner, last_error, results, call, queries, radius, mask_of, masked):
    """The shape every range search shares: call(queries, nq, radius, mask_of pointer, masked flag, lims) -> status, then the packed
    results through results(ids, scores).  masked None: masked iff mask_of is given (masked=True with mask_of None: plane 0)."""
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    if queries.ndim == 1:
        queries = queries[None, :]
    nq = queries.shape[0]
    radius = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))
    mo = _mask_of_arg(mask_of, nq)
    masked = (mo is not None) if masked is None else bool(masked)
    lims = np.zeros(nq + 1, dtype=np.uint64)
    st = call(queries, nq, radius, mo.ctypes.data if mo is not None else None, 1 if masked else 0, lims)
    if st:
        err = NvdbError(st, last_error())
        err.lims = lims
        raise err
    total = int(lims[nq])
    ids = np.empty(max(total, 1), dtype=np.uint64)
    scores = np.empty(max(total, 1), dtype=np.float32)
    owner._chk(results(ids.ctypes.data, scores.ctypes.data))
    return lims, ids[:total], scores[:total]


# ------------------------------------------------------------------------------- device context
class HipContext:
    """One GPU: resident corpus + workspace (nvdb_hip_ctx)."""

    def __init__(self, device=0, dev=False):
        self.lib = load_dev_library() if dev else load_library()   # dev=True: a context of the developer build (tools_dev/)
        h = C.c_void_p()
        st = self.lib.nvdb_hip_create(device, C.byref(h))
        if st:
            raise NvdbError(st, self.lib.nvdb_hip_last_error(None).decode())
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.nvdb_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st):
        if st:
            raise NvdbError(st, self.lib.nvdb_hip_last_error(self.h).decode())

    # -- corpus
    def upload_corpus(self, rows, dtype, scales=None, row_base=0):
        if dtype == DT_F16 and getattr(rows, "dtype", None) == np.float16:
            rows = rows.view(np.uint16)                     # IEEE half bits, not a value conversion to integers
        rows = np.ascontiguousarray(rows, dtype=_NP_OF[dtype])
        sc = np.ascontiguousarray(scales, dtype=np.float32) if scales is not None else None
        self._chk(self.lib.nvdb_hip_upload_corpus(self.h, rows.ctypes.data, sc.ctypes.data if sc is not None else None,
                                                  rows.shape[0], rows.shape[1], dtype, row_base))

    def adopt_corpus(self, dev_ptr, n, dim, dtype, dev_scales_ptr=None, row_base=0):
        self._chk(self.lib.nvdb_hip_adopt_corpus(self.h, dev_ptr, dev_scales_ptr, n, dim, dtype, row_base))

    def generate_corpus(self, seed, n, dim, dtype, row_base=0):
        self._chk(self.lib.nvdb_hip_generate_corpus(self.h, seed, n, dim, dtype, row_base))

    def corpus_info(self):
        n, dim, dt, base, mx = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_float()
        self._chk(self.lib.nvdb_hip_corpus_info(self.h, C.byref(n), C.byref(dim), C.byref(dt), C.byref(base), C.byref(mx)))
        return dict(n=n.value, dim=dim.value, dtype=dt.value, row_base=base.value, max_row_norm=mx.value)

    def download_rows(self, row0, nrows):
        info = self.corpus_info()
        out = np.empty((nrows, info["dim"]), dtype=_NP_OF[info["dtype"]])
        sc = np.empty(nrows, dtype=np.float32) if info["dtype"] == DT_I8 else None
        self._chk(self.lib.nvdb_hip_download_rows(self.h, row0, nrows, out.ctypes.data,
                                                  sc.ctypes.data if sc is not None else None))
        return out, sc

    def set_option(self, key, value):
        self._chk(self.lib.nvdb_hip_set_option(self.h, key.encode(), int(value)))

    # -- flat scan
    def search_batch(self, queries, k, want_timing=False):
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        if queries.ndim == 1:
            queries = queries[None, :]
        nq = queries.shape[0]
        ids = np.full((nq, max(k, 1)), np.iinfo(np.uint64).max, dtype=np.uint64)
        scores = np.full((nq, max(k, 1)), -np.inf, dtype=np.float32)
        keff = C.c_uint32(0)
        t = Timing()
        self._chk(self.lib.nvdb_hip_search_batch(self.h, queries.ctypes.data, nq, k, ids.ctypes.data, scores.ctypes.data,
                                                 C.byref(keff), C.byref(t) if want_timing else None))
        ke = keff.value if k > 0 else 0
        if want_timing:
            return ids[:, :ke], scores[:, :ke], t
        return ids[:, :ke], scores[:, :ke]

    def search_batch_dev(self, dev_q, nq, k, dev_out_ids, dev_out_scores, stream=None):
        self._chk(self.lib.nvdb_hip_search_batch_dev(self.h, dev_q, nq, k, dev_out_ids, dev_out_scores, stream))

    def search_check(self):
        s = ScanStats()
        self._chk(self.lib.nvdb_hip_search_check(self.h, C.byref(s)))
        return s.as_dict()

    def stats(self):
        s = ScanStats()
        self._chk(self.lib.nvdb_hip_get_stats(self.h, C.byref(s)))
        return s.as_dict()

    # -- range search
    def range_search(self, queries, radius, want_timing=False):
        """Every row whose score reaches the query's radius (a scalar, or one per query) -> (lims [nq + 1] u64, ids u64, scores f32):
        query q's rows are ids[lims[q]:lims[q + 1]], score descending, id ascending.  Over the result budget (option range_max_mb)
        the NvdbError carries the complete lims as `.lims`."""
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        if queries.ndim == 1:
            queries = queries[None, :]
        nq = queries.shape[0]
        radius = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))
        lims = np.zeros(nq + 1, dtype=np.uint64)
        t = Timing()
        st = self.lib.nvdb_hip_range_search(self.h, queries.ctypes.data, nq, radius.ctypes.data, lims.ctypes.data,
                                            C.byref(t) if want_timing else None)
        if st:
            err = NvdbError(st, self.lib.nvdb_hip_last_error(self.h).decode())
            err.lims = lims
            raise err
        total = int(lims[nq])
        ids = np.empty(max(total, 1), dtype=np.uint64)
        scores = np.empty(max(total, 1), dtype=np.float32)
        self._chk(self.lib.nvdb_hip_range_results(self.h, ids.ctypes.data, scores.ctypes.data))
        return (lims, ids[:total], scores[:total], t) if want_timing else (lims, ids[:total], scores[:total])

    def shadow_info(self):
        """The int8 filter shadow of an fp16 / fp32 corpus: resident, its bytes, demoted (searches start on the fp16 filter),
        last_filter (what the last search's filter launches streamed: None, "f16", "shadow" or "i8")."""
        out = (C.c_uint64 * 4)()
        self._chk(self.lib.nvdb_hip_shadow_info(self.h, out))
        return dict(resident=bool(out[0]), bytes=int(out[1]), demoted=bool(out[2]), last_filter=(None, "f16", "shadow", "i8")[out[3]])

    def shadow_scale_info(self):
        """The scales of the int8 filter shadow: common (every row under one scale: the flat search runs the bits-domain first
        stage), scale (the common scale the load found), resid_row / resid_common (the largest residual the load measured under the
        per-row rule / under the common scale; 0: not measured)."""
        out = (C.c_double * 4)()
        self._chk(self.lib.nvdb_hip_shadow_scale_info(self.h, out))
        return dict(common=bool(out[0]), scale=float(out[1]), resid_row=float(out[2]), resid_common=float(out[3]))

    def collect_kernel_times(self):
        n, ms, fl, by = C.c_uint32(), C.c_double(), C.c_double(), C.c_double()
        self._chk(self.lib.nvdb_hip_collect_kernel_times(self.h, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
        return dict(launches=n.value, ms=ms.value, flops=fl.value, bytes=by.value)

    def merge_topk_dev(self, dev_ids, dev_scores, nshards, nq, k, dev_out_ids, dev_out_scores, stream=None):
        self._chk(self.lib.nvdb_hip_merge_topk_dev(self.h, dev_ids, dev_scores, nshards, nq, k, dev_out_ids,
                                                   dev_out_scores, stream))

    def merge_topk_strided_dev(self, dev_ids, dev_scores, stride_ids, stride_scores, nshards, nq, k, dev_out_ids, dev_out_scores,
                               stream=None):
        self._chk(self.lib.nvdb_hip_merge_topk_strided_dev(self.h, dev_ids, dev_scores, stride_ids, stride_scores, nshards, nq, k,
                                                           dev_out_ids, dev_out_scores, stream))

    # -- partitioned probe search
    def set_partitions(self, offsets):
        """offsets: nparts + 1 local row numbers, offsets[0] == 0, non-decreasing, offsets[-1] == n."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._chk(self.lib.nvdb_hip_set_partitions(self.h, offsets.ctypes.data, max(offsets.size, 1) - 1))

    def set_centroids(self, centroids):
        centroids = np.ascontiguousarray(centroids, dtype=np.float32)
        self._chk(self.lib.nvdb_hip_set_centroids(self.h, centroids.ctypes.data))

    def _probe_outputs(self, queries, k):
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        if queries.ndim == 1:
            queries = queries[None, :]
        nq = queries.shape[0]
        ids = np.full((nq, k), np.iinfo(np.uint64).max, dtype=np.uint64)
        scores = np.full((nq, k), -np.inf, dtype=np.float32)
        return queries, nq, ids, scores, np.zeros(nq, dtype=np.uint32)

    def search_partitions(self, queries, k, probe, want_timing=False):
        """probe: [nq, nprobe] partition numbers (0xFFFFFFFF = empty slot) -> (ids [nq, k], scores [nq, k], counts [nq])."""
        queries, nq, ids, scores, counts = self._probe_outputs(queries, k)
        probe = np.ascontiguousarray(probe, dtype=np.uint32).reshape(nq, -1)
        t = Timing()
        self._chk(self.lib.nvdb_hip_search_partitions(self.h, queries.ctypes.data, nq, k, probe.ctypes.data, probe.shape[1],
                                                      ids.ctypes.data, scores.ctypes.data, counts.ctypes.data,
                                                      C.byref(t) if want_timing else None))
        return (ids, scores, counts, t) if want_timing else (ids, scores, counts)

    def search_ivf(self, queries, k, nprobe, want_probe=False):
        """IVF-Flat: the nprobe partitions with the best centroids, then search_partitions; (ids, scores, counts[, probe])."""
        queries, nq, ids, scores, counts = self._probe_outputs(queries, k)
        probe = np.full((nq, nprobe), 0xFFFFFFFF, dtype=np.uint32)
        self._chk(self.lib.nvdb_hip_search_ivf(self.h, queries.ctypes.data, nq, k, nprobe, ids.ctypes.data, scores.ctypes.data,
                                               counts.ctypes.data, probe.ctypes.data if want_probe else None, None))
        return (ids, scores, counts, probe) if want_probe else (ids, scores, counts)

    # -- row masks (live rows only, for the *_masked searches and the range searches on the probe path; search_batch and range_search are NOT masked)
    def set_row_masks(self, masks):
        """masks: bool [nmasks, n] / packed uint32 [nmasks, ceil(n / 32)] (pack_row_masks); an int: that many all-live masks;
        None or 0: drop them."""
        if masks is None or (isinstance(masks, (int, np.integer)) and not isinstance(masks, (bool, np.bool_))):
            self._chk(self.lib.nvdb_hip_set_row_masks(self.h, None, int(masks or 0)))
            return
        packed = pack_row_masks(masks, self.corpus_info()["n"])
        self._chk(self.lib.nvdb_hip_set_row_masks(self.h, packed.ctypes.data, packed.shape[0]))

    def update_row_mask(self, mask, rows, live):
        """Set (live) or clear the listed local rows' bits of one mask on the device: the tombstone path."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64).ravel()
        self._chk(self.lib.nvdb_hip_update_row_mask(self.h, mask, rows.ctypes.data if rows.size else None, rows.size, 1 if live else 0))

    def get_row_masks(self):
        """The resident planes as packed uint32 [nmasks, ceil(n / 32)] (unpack_row_masks gives bools)."""
        nm, w = C.c_uint32(), C.c_uint64()
        self._chk(self.lib.nvdb_hip_get_row_masks(self.h, C.byref(nm), C.byref(w), None))
        out = np.zeros((nm.value, w.value), dtype=np.uint32)
        if out.size:
            self._chk(self.lib.nvdb_hip_get_row_masks(self.h, None, None, out.ctypes.data))
        return out

    def compact_rows(self, mask=0):
        """Remove the rows that are dead in plane `mask` from the resident corpus, on the device, in place (stable) ->
        (n_new, old_rows [n_new] u32: new local row j was old local row old_rows[j])."""
        n_old = self.corpus_info()["n"]
        old = np.zeros(max(n_old, 1), dtype=np.uint32)
        n_new = C.c_uint64(0)
        self._chk(self.lib.nvdb_hip_compact_rows(self.h, mask, C.byref(n_new), old.ctypes.data))
        return n_new.value, old[:n_new.value].copy()

    def reserve_rows(self, rows):
        """Make room for at least `rows` rows in the resident corpus' arrays: insertions up to that count move in place."""
        self._chk(self.lib.nvdb_hip_reserve_rows(self.h, int(rows)))

    def insert_rows(self, rows, scales=None, part_of=None):
        """Insert host rows ([m, dim] in the corpus' dtype; scales iff int8) at the end of the corpus (part_of None) or at the ends
        of the partitions part_of [m] names -> (n_new, new_rows [m] u64: the new local row of inserted row i)."""
        info = self.corpus_info()
        if info["dtype"] == DT_F16 and getattr(rows, "dtype", None) == np.float16:
            rows = rows.view(np.uint16)
        rows = np.ascontiguousarray(rows, dtype=_NP_OF[info["dtype"]]).reshape(-1, info["dim"])
        m = rows.shape[0]
        sc = np.ascontiguousarray(scales, dtype=np.float32) if scales is not None else None
        po = np.ascontiguousarray(part_of, dtype=np.uint32).ravel() if part_of is not None else None
        if po is not None and po.size != m:
            raise ValueError("part_of must have one entry per row")
        new_rows = np.zeros(max(m, 1), dtype=np.uint64)
        n_new = C.c_uint64(0)
        self._chk(self.lib.nvdb_hip_insert_rows(self.h, rows.ctypes.data if m else None, sc.ctypes.data if sc is not None else None, m,
                                                po.ctypes.data if po is not None else None, new_rows.ctypes.data, C.byref(n_new)))
        return n_new.value, new_rows[:m].copy()

    def search_partitions_masked(self, queries, k, probe, mask_of=None, want_timing=False):
        """search_partitions over the rows live in each query's mask: mask_of[q] = plane number (0xFFFFFFFF: none; None: plane 0
        for every query) -> (ids, scores, counts); counts[q] = min(k, live rows in the probed union)."""
        queries, nq, ids, scores, counts = self._probe_outputs(queries, k)
        probe = np.ascontiguousarray(probe, dtype=np.uint32).reshape(nq, -1)
        mo = _mask_of_arg(mask_of, nq)
        t = Timing()
        self._chk(self.lib.nvdb_hip_search_partitions_masked(self.h, queries.ctypes.data, nq, k, probe.ctypes.data, probe.shape[1],
                                                             mo.ctypes.data if mo is not None else None, ids.ctypes.data,
                                                             scores.ctypes.data, counts.ctypes.data, C.byref(t) if want_timing else None))
        return (ids, scores, counts, t) if want_timing else (ids, scores, counts)

    def search_ivf_masked(self, queries, k, nprobe, mask_of=None, want_probe=False):
        """search_ivf (unmasked coarse step) with the partition scan restricted to live rows."""
        queries, nq, ids, scores, counts = self._probe_outputs(queries, k)
        probe = np.full((nq, nprobe), 0xFFFFFFFF, dtype=np.uint32)
        mo = _mask_of_arg(mask_of, nq)
        self._chk(self.lib.nvdb_hip_search_ivf_masked(self.h, queries.ctypes.data, nq, k, nprobe, mo.ctypes.data if mo is not None else None,
                                                      ids.ctypes.data, scores.ctypes.data, counts.ctypes.data,
                                                      probe.ctypes.data if want_probe else None, None))
        return (ids, scores, counts, probe) if want_probe else (ids, scores, counts)

    def search_masked(self, queries, k, mask_of=None, want_timing=False):
        """The masked flat search (nvdb_hip_search_batch_masked): exact top-k over ALL live rows, k <= 64.  Large corpora with an
        MFMA filter (option path = 0: at least 262144 rows; path = 2: always) take the filter route -- a bar per query from a
        prefix that holds enough live rows, then one stream of the corpus (stats path 2); the others the partition scan, which
        reads the rows once per group of up to 32 queries (stats path 4).  The result does not depend on the route."""
        queries, nq, ids, scores, counts = self._probe_outputs(queries, k)
        mo = _mask_of_arg(mask_of, nq)
        t = Timing()
        self._chk(self.lib.nvdb_hip_search_batch_masked(self.h, queries.ctypes.data, nq, k, mo.ctypes.data if mo is not None else None,
                                                        ids.ctypes.data, scores.ctypes.data, counts.ctypes.data,
                                                        C.byref(t) if want_timing else None))
        return (ids, scores, counts, t) if want_timing else (ids, scores, counts)

    # -- probe search for any k (k <= 64: the twins above, bit for bit; beyond: scan, radix select, sort -- stats path 8)
    def search_partitions_anyk(self, queries, k, probe, mask_of=None, masked=None, want_timing=False):
        """search_partitions / search_partitions_masked for any k >= 1 (k is not clamped: counts[q] = min(k, live rows in the probed
        union), padding behind it).  masked None: masked iff mask_of is given (masked=True with mask_of None: plane 0)."""
        queries, nq, ids, scores, counts = self._probe_outputs(queries, k)
        probe = np.ascontiguousarray(probe, dtype=np.uint32).reshape(nq, -1)
        mo = _mask_of_arg(mask_of, nq)
        masked = (mo is not None) if masked is None else bool(masked)
        t = Timing()
        self._chk(self.lib.nvdb_hip_search_partitions_anyk(self.h, queries.ctypes.data, nq, k, probe.ctypes.data, probe.shape[1],
                                                           mo.ctypes.data if mo is not None else None, 1 if masked else 0, ids.ctypes.data,
                                                           scores.ctypes.data, counts.ctypes.data, C.byref(t) if want_timing else None))
        return (ids, scores, counts, t) if want_timing else (ids, scores, counts)

    def search_ivf_anyk(self, queries, k, nprobe, mask_of=None, masked=None, want_probe=False):
        """search_ivf / search_ivf_masked for any k >= 1; (ids, scores, counts[, probe])."""
        queries, nq, ids, scores, counts = self._probe_outputs(queries, k)
        probe = np.full((nq, nprobe), 0xFFFFFFFF, dtype=np.uint32)
        mo = _mask_of_arg(mask_of, nq)
        masked = (mo is not None) if masked is None else bool(masked)
        self._chk(self.lib.nvdb_hip_search_ivf_anyk(self.h, queries.ctypes.data, nq, k, nprobe, mo.ctypes.data if mo is not None else None,
                                                    1 if masked else 0, ids.ctypes.data, scores.ctypes.data, counts.ctypes.data,
                                                    probe.ctypes.data if want_probe else None, None))
        return (ids, scores, counts, probe) if want_probe else (ids, scores, counts)

    # -- range search on the probe path (lims, ids, scores as range_search; over range_max_mb the NvdbError carries `.lims`)
    def _range(self, call, queries, radius, mask_of, masked):
        return _range_call(self, lambda: self.lib.nvdb_hip_last_error(self.h).decode(),
                           lambda i, s: self.lib.nvdb_hip_range_results(self.h, i, s), call, queries, radius, mask_of, masked)

    def range_search_partitions(self, queries, radius, probe, mask_of=None, masked=None):
        """range_search over each query's probed partitions (probe as search_partitions), optionally restricted to the rows live in
        its mask (mask_of as search_partitions_masked; masked=True with mask_of None: plane 0 for every query)."""
        def call(q, nq, r, mo, masked_, lims):
            pr = np.ascontiguousarray(probe, dtype=np.uint32).reshape(nq, -1)
            return self.lib.nvdb_hip_range_search_partitions(self.h, q.ctypes.data, nq, r.ctypes.data, pr.ctypes.data, pr.shape[1], mo, masked_,
                                                             lims.ctypes.data, None)
        return self._range(call, queries, radius, mask_of, masked)

    def range_search_ivf(self, queries, radius, nprobe, mask_of=None, masked=None, want_probe=False):
        """range_search over the nprobe partitions with the best centroids (search_ivf's coarse step); (lims, ids, scores[, probe])."""
        box = {}

        def call(q, nq, r, mo, masked_, lims):
            box["probe"] = np.full((nq, nprobe), 0xFFFFFFFF, dtype=np.uint32)
            return self.lib.nvdb_hip_range_search_ivf(self.h, q.ctypes.data, nq, r.ctypes.data, nprobe, mo, masked_, lims.ctypes.data,
                                                      box["probe"].ctypes.data if want_probe else None, None)
        out = self._range(call, queries, radius, mask_of, masked)
        return out + (box["probe"],) if want_probe else out

    def range_search_masked(self, queries, radius, mask_of=None):
        """The masked flat range search: range_search over the rows live in each query's mask (mask_of None: plane 0)."""
        def call(q, nq, r, mo, masked_, lims):
            return self.lib.nvdb_hip_range_search_masked(self.h, q.ctypes.data, nq, r.ctypes.data, mo, lims.ctypes.data, None)
        return self._range(call, queries, radius, mask_of, True)

    # -- IVF-Flat build
    def assign_rows(self, centroids, row0=0, nrows=None):
        """Best centroid ([nparts, dim] f32) of the resident rows [row0, row0 + nrows) -> [nrows] u32."""
        centroids = np.ascontiguousarray(centroids, dtype=np.float32)
        if nrows is None:
            nrows = self.corpus_info()["n"] - row0
        out = np.zeros(max(nrows, 0), dtype=np.uint32)
        self._chk(self.lib.nvdb_hip_assign_rows(self.h, centroids.ctypes.data, centroids.shape[0], row0, nrows,
                                                out.ctypes.data if out.size else None))
        return out

    def train_centroids(self, nparts, iters, seed, max_train_rows=0, init=None):
        """Spherical k-means over the resident corpus -> [nparts, dim] f32 unit centroids."""
        dim = self.corpus_info()["dim"]
        if init is not None:
            init = np.ascontiguousarray(init, dtype=np.float32).reshape(nparts, dim)
        out = np.zeros((nparts, dim), dtype=np.float32)
        self._chk(self.lib.nvdb_hip_train_centroids(self.h, nparts, iters, seed, max_train_rows,
                                                    init.ctypes.data if init is not None else None, out.ctypes.data))
        return out

    # -- refine
    def refine_l2_topk(self, queries, cand_ids, K, want_dist=True, want_timing=False):
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        cand_ids = np.ascontiguousarray(cand_ids, dtype=np.uint32)
        Q, R = cand_ids.shape if cand_ids.ndim == 2 else (0, 0)
        ids = np.full((Q, K), 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full((Q, K), 1e30, dtype=np.float32) if want_dist else None
        t = Timing()
        self._chk(self.lib.nvdb_hip_refine_l2_topk(self.h, queries.ctypes.data, cand_ids.ctypes.data, Q, R, K,
                                                   ids.ctypes.data, dist.ctypes.data if dist is not None else None,
                                                   C.byref(t) if want_timing else None))
        return (ids, dist, t) if want_timing else (ids, dist)

    def refine_l2_topk_dev(self, dev_q, dev_cand, Q, R, K, dev_out_ids, dev_out_dist, stream=None):
        self._chk(self.lib.nvdb_hip_refine_l2_topk_dev(self.h, dev_q, dev_cand, Q, R, K, dev_out_ids, dev_out_dist, stream))


class _BorrowedContext(HipContext):
    """A context somebody else owns (an IvfIndex's): every method of HipContext, close() only forgets the handle."""

    def __init__(self, lib, handle, device):
        self.lib, self.h, self.device = lib, handle, device

    def close(self):
        self.h = None


class IvfIndex:
    """IVF-Flat index over the corpus resident in `src_ctx` (nvdb_hip_ivf): the rows copied into list order under `centroids`
    ([nparts, dim] f32, e.g. from HipContext.train_centroids), searched by probe, answered in src_ctx's ids.  src_ctx is not
    touched and may be closed afterwards."""

    def __init__(self, src_ctx, centroids):
        self.lib = src_ctx.lib
        centroids = np.ascontiguousarray(centroids, dtype=np.float32)
        if centroids.ndim != 2:
            raise ValueError("centroids must be [nparts, dim]")
        h = C.c_void_p()
        st = self.lib.nvdb_hip_ivf_build(src_ctx.h, centroids.ctypes.data, centroids.shape[0], C.byref(h))
        if st:
            raise NvdbError(st, self.lib.nvdb_hip_ivf_last_error(None).decode())
        self.h = h
        self.ctx = _BorrowedContext(self.lib, C.c_void_p(self.lib.nvdb_hip_ivf_ctx(h)), src_ctx.device)
        self.src_n = self.info()["n"]                    # rows of the source corpus: what the planes stay indexed by after compact()

    def close(self):
        if getattr(self, "h", None):
            self.ctx.close()
            self.lib.nvdb_hip_ivf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st):
        if st:
            raise NvdbError(st, self.lib.nvdb_hip_ivf_last_error(self.h).decode())

    def info(self):
        """dict(n, nparts, offsets [nparts + 1] u64, perm [n] u32: perm[position] = row of the source corpus)."""
        n, nparts = C.c_uint64(), C.c_uint32()
        self._chk(self.lib.nvdb_hip_ivf_info(self.h, C.byref(n), C.byref(nparts), None, None))
        offsets = np.zeros(nparts.value + 1, dtype=np.uint64)
        perm = np.zeros(max(n.value, 1), dtype=np.uint32)
        self._chk(self.lib.nvdb_hip_ivf_info(self.h, None, None, offsets.ctypes.data, perm.ctypes.data))
        return dict(n=n.value, nparts=nparts.value, offsets=offsets, perm=perm[:n.value])

    def search(self, queries, k, nprobe, want_probe=False):
        """(ids [nq, k] in the source corpus' ids, scores [nq, k], counts [nq][, probe [nq, nprobe]]); equal scores are ordered
        by (partition, original id)."""
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        if queries.ndim == 1:
            queries = queries[None, :]
        nq = queries.shape[0]
        ids = np.full((nq, k), np.iinfo(np.uint64).max, dtype=np.uint64)
        scores = np.full((nq, k), -np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        probe = np.full((nq, nprobe), 0xFFFFFFFF, dtype=np.uint32)
        self._chk(self.lib.nvdb_hip_ivf_search(self.h, queries.ctypes.data, nq, k, nprobe, ids.ctypes.data, scores.ctypes.data,
                                               counts.ctypes.data, probe.ctypes.data if want_probe else None, None))
        return (ids, scores, counts, probe) if want_probe else (ids, scores, counts)

    # -- row masks in the source corpus' rows (without its row base)
    def set_row_masks(self, masks):
        """As HipContext.set_row_masks, indexed by ORIGINAL row."""
        if masks is None or (isinstance(masks, (int, np.integer)) and not isinstance(masks, (bool, np.bool_))):
            self._chk(self.lib.nvdb_hip_ivf_set_row_masks(self.h, None, int(masks or 0)))
            return
        packed = pack_row_masks(masks, self.src_n)
        self._chk(self.lib.nvdb_hip_ivf_set_row_masks(self.h, packed.ctypes.data, packed.shape[0]))

    def update_row_mask(self, mask, rows, live):
        rows = np.ascontiguousarray(rows, dtype=np.uint64).ravel()
        self._chk(self.lib.nvdb_hip_ivf_update_row_mask(self.h, mask, rows.ctypes.data if rows.size else None, rows.size, 1 if live else 0))

    def compact(self, mask=0):
        """Remove the rows that are dead in plane `mask` from the index, on the device, in place -> n_new.  The lists shrink and
        stay contiguous; ids stay the source corpus' ids; info() reports the new n, offsets and perm."""
        n_new = C.c_uint64(0)
        self._chk(self.lib.nvdb_hip_ivf_compact(self.h, mask, C.byref(n_new)))
        return n_new.value

    def add_rows(self, rows, scales=None):
        """Add host rows ([m, dim] in the index's dtype; scales iff int8): each joins the end of the list of its best centroid and
        gets the original id src_n + i -> (first_id, assign [m] u32).  info() reports the new n, offsets and perm."""
        info = self.ctx.corpus_info()
        if info["dtype"] == DT_F16 and getattr(rows, "dtype", None) == np.float16:
            rows = rows.view(np.uint16)
        rows = np.ascontiguousarray(rows, dtype=_NP_OF[info["dtype"]]).reshape(-1, info["dim"])
        m = rows.shape[0]
        sc = np.ascontiguousarray(scales, dtype=np.float32) if scales is not None else None
        assign = np.zeros(max(m, 1), dtype=np.uint32)
        first = C.c_uint64(0)
        self._chk(self.lib.nvdb_hip_ivf_add_rows(self.h, rows.ctypes.data if m else None, sc.ctypes.data if sc is not None else None, m,
                                                 C.byref(first), assign.ctypes.data))
        self.src_n += m
        return first.value, assign[:m].copy()

    def search_masked(self, queries, k, nprobe, mask_of=None, want_probe=False):
        """search() over the rows live in each query's mask (mask_of as HipContext.search_partitions_masked)."""
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        if queries.ndim == 1:
            queries = queries[None, :]
        nq = queries.shape[0]
        ids = np.full((nq, k), np.iinfo(np.uint64).max, dtype=np.uint64)
        scores = np.full((nq, k), -np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        probe = np.full((nq, nprobe), 0xFFFFFFFF, dtype=np.uint32)
        mo = _mask_of_arg(mask_of, nq)
        self._chk(self.lib.nvdb_hip_ivf_search_masked(self.h, queries.ctypes.data, nq, k, nprobe, mo.ctypes.data if mo is not None else None,
                                                      ids.ctypes.data, scores.ctypes.data, counts.ctypes.data,
                                                      probe.ctypes.data if want_probe else None, None))
        return (ids, scores, counts, probe) if want_probe else (ids, scores, counts)

    def search_anyk(self, queries, k, nprobe, mask_of=None, masked=None, want_probe=False):
        """search() / search_masked() for any k >= 1 (k is not clamped): (ids in the source corpus' ids, scores, counts[, probe]);
        equal scores by (partition, original id).  masked None: masked iff mask_of is given."""
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        if queries.ndim == 1:
            queries = queries[None, :]
        nq = queries.shape[0]
        ids = np.full((nq, k), np.iinfo(np.uint64).max, dtype=np.uint64)
        scores = np.full((nq, k), -np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        probe = np.full((nq, nprobe), 0xFFFFFFFF, dtype=np.uint32)
        mo = _mask_of_arg(mask_of, nq)
        masked = (mo is not None) if masked is None else bool(masked)
        self._chk(self.lib.nvdb_hip_ivf_search_anyk(self.h, queries.ctypes.data, nq, k, nprobe, mo.ctypes.data if mo is not None else None,
                                                    1 if masked else 0, ids.ctypes.data, scores.ctypes.data, counts.ctypes.data,
                                                    probe.ctypes.data if want_probe else None, None))
        return (ids, scores, counts, probe) if want_probe else (ids, scores, counts)

    def range_search(self, queries, radius, nprobe, mask_of=None, masked=None, want_probe=False):
        """Every row of the nprobe best lists whose score reaches the query's radius, optionally restricted to the rows live in its
        mask (original-row planes) -> (lims, ids in the source corpus' ids, scores[, probe]); equal scores by (partition, original id)."""
        box = {}

        def call(q, nq, r, mo, masked_, lims):
            box["probe"] = np.full((nq, nprobe), 0xFFFFFFFF, dtype=np.uint32)
            return self.lib.nvdb_hip_ivf_range_search(self.h, q.ctypes.data, nq, r.ctypes.data, nprobe, mo, masked_, lims.ctypes.data,
                                                      box["probe"].ctypes.data if want_probe else None, None)
        out = _range_call(self, lambda: self.lib.nvdb_hip_ivf_last_error(self.h).decode(),
                          lambda i, s: self.lib.nvdb_hip_ivf_range_results(self.h, i, s), call, queries, radius, mask_of, masked)
        return out + (box["probe"],) if want_probe else out


class DeviceGroup:
    """One process, several GPUs (nvdb_hip_group): corpus row-sharded over `devices`, per-shard top-k exchanged by an RCCL
    all-gather (or peer copies when a device is listed twice), merged on devices[0]."""

    def __init__(self, devices):
        self.lib = load_library()
        if self.lib.nvdb_hip_device_count() > 0:             # (no GPU: creation fails below without ever needing RCCL)
            _share_rccl_with_torch()
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        st = self.lib.nvdb_hip_group_create(arr, len(devices), C.byref(h))
        if st:
            raise NvdbError(st, self.lib.nvdb_hip_group_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.nvdb_hip_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st):
        if st:
            raise NvdbError(st, self.lib.nvdb_hip_group_last_error(self.h).decode())

    def size(self):
        return self.lib.nvdb_hip_group_size(self.h)

    def exchange(self):
        why = C.c_char_p()
        mode = self.lib.nvdb_hip_group_exchange(self.h, C.byref(why))
        return ("rccl" if mode == 1 else "peer-copy"), (why.value or b"").decode()

    def shard_stats(self, shard):
        s = ScanStats()
        st = self.lib.nvdb_hip_get_stats(self.lib.nvdb_hip_group_ctx(self.h, shard), C.byref(s))
        if st:
            raise NvdbError(st, "get_stats")
        return s.as_dict()

    def upload_corpus(self, rows, dtype, scales=None):
        if dtype == DT_F16 and getattr(rows, "dtype", None) == np.float16:
            rows = rows.view(np.uint16)
        rows = np.ascontiguousarray(rows, dtype=_NP_OF[dtype])
        sc = np.ascontiguousarray(scales, dtype=np.float32) if scales is not None else None
        self._chk(self.lib.nvdb_hip_group_upload_corpus(self.h, rows.ctypes.data, sc.ctypes.data if sc is not None else None,
                                                        rows.shape[0], rows.shape[1], dtype))

    def generate_corpus(self, seed, n, dim, dtype):
        self._chk(self.lib.nvdb_hip_group_generate_corpus(self.h, seed, n, dim, dtype))

    def set_option(self, key, value):
        self._chk(self.lib.nvdb_hip_group_set_option(self.h, key.encode(), int(value)))

    def search_batch(self, queries, k, want_stats=False):
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        if queries.ndim == 1:
            queries = queries[None, :]
        nq = queries.shape[0]
        ids = np.full((nq, max(k, 1)), np.iinfo(np.uint64).max, dtype=np.uint64)
        scores = np.full((nq, max(k, 1)), -np.inf, dtype=np.float32)
        keff = C.c_uint32(0)
        gs = GroupStats()
        self._chk(self.lib.nvdb_hip_group_search_batch(self.h, queries.ctypes.data, nq, k, ids.ctypes.data, scores.ctypes.data,
                                                       C.byref(keff), C.byref(gs)))
        ke = keff.value if k > 0 else 0
        if want_stats:
            return ids[:, :ke], scores[:, :ke], gs.as_dict()
        return ids[:, :ke], scores[:, :ke]


class FlatIndexHIP:
    """GPU flat index with the reference's FlatIndex surface (include/nvdb/flat_index.h:11-13):
    constructed over a dataset, `search_topk_dot(q, k)` -> list of (id, score), best first; plus the
    batched entry the reference lacks."""

    def __init__(self, rows, dtype, scales=None, device=0, row_base=0):
        if rows is None or len(rows) == 0:
            raise RuntimeError("Empty base")          # src/flat_index.cpp:17
        self.ctx = HipContext(device)
        self.ctx.upload_corpus(rows, dtype, scales, row_base)

    def search_topk_dot(self, q, k):
        if q is None:
            raise RuntimeError("Null query")          # src/flat_index_pool.cpp:196
        if k == 0:
            return []                                 # src/flat_index.cpp:18
        ids, sc = self.ctx.search_batch(np.asarray(q, dtype=np.float32)[None, :], k)
        return [(int(i), float(s)) for i, s in zip(ids[0], sc[0])]

    def search_topk_dot_batch(self, queries, k):
        return self.ctx.search_batch(queries, k)


def l2_topk_batch(ctx, queries_f32, cand_ids, K, return_dist=True):
    """nvdb::cuda_l2_topk_batch on the context's resident corpus; returns (ids, dist, Timing)."""
    return ctx.refine_l2_topk(queries_f32, cand_ids, K, want_dist=return_dist, want_timing=True)
