"""CPU-side checks of the row masks' C ABI: the nine entry points are declared in include/nvdb_hip.h, exported by libnvdb_hip.so
and bound; the ABI version did not move; without a context or an index every call fails cleanly and writes nothing; the host-side
bit work (csrc/row_mask.h) runs as a stand-alone program under AddressSanitizer / UBSan; the binding's bit packing is the layout
the header states."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nvdb_hip_set_row_masks", "nvdb_hip_update_row_mask", "nvdb_hip_get_row_masks", "nvdb_hip_search_partitions_masked",
         "nvdb_hip_search_ivf_masked", "nvdb_hip_search_batch_masked", "nvdb_hip_ivf_set_row_masks", "nvdb_hip_ivf_update_row_mask",
         "nvdb_hip_ivf_search_masked"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(nvdb_amd.LIB_PATH):
        g.build()
    return nvdb_amd.load_library()


def test_entry_points_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "nvdb_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nvdb_[a-z0-9_]+)\s*\(", hdr))
    syms = subprocess.run(["nm", "-D", "--defined-only", nvdb_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(nvdb_[a-z0-9_]+)\b", syms))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in nvdb_hip.h"
        assert name in exported, f"{name} is not exported by libnvdb_hip.so"
        assert name in nvdb_amd.EXPORTS and hasattr(lib, name)
    assert "#define NVDB_HIP_ABI_VERSION 3" in text
    assert lib.nvdb_hip_abi_version() == 3
    for meth in ("set_row_masks", "update_row_mask", "get_row_masks", "search_partitions_masked", "search_ivf_masked", "search_masked"):
        assert callable(getattr(nvdb_amd.HipContext, meth))
    for meth in ("set_row_masks", "update_row_mask", "search_masked"):
        assert callable(getattr(nvdb_amd.IvfIndex, meth))


def test_calls_without_a_context_fail_cleanly(lib):
    bits = np.full(4, 7, dtype=np.uint32)
    rows = np.array([0, 1], dtype=np.uint64)
    q = np.zeros((2, 8), dtype=np.float32)
    probe = np.zeros((2, 1), dtype=np.uint32)
    mask_of = np.zeros(2, dtype=np.uint32)
    ids = np.full((2, 4), 7, dtype=np.uint64)
    sc = np.full((2, 4), 7.0, dtype=np.float32)
    cnt = np.full(2, 7, dtype=np.uint32)
    pr = np.full((2, 1), 7, dtype=np.uint32)
    nm, w = C.c_uint32(7), C.c_uint64(7)
    assert lib.nvdb_hip_set_row_masks(None, bits.ctypes.data, 1) == 1                       # NVDB_ERR_INVALID
    assert lib.nvdb_hip_update_row_mask(None, 0, rows.ctypes.data, 2, 0) == 1
    assert lib.nvdb_hip_get_row_masks(None, C.byref(nm), C.byref(w), bits.ctypes.data) == 1
    assert lib.nvdb_hip_search_partitions_masked(None, q.ctypes.data, 2, 4, probe.ctypes.data, 1, mask_of.ctypes.data, ids.ctypes.data,
                                                 sc.ctypes.data, cnt.ctypes.data, None) == 1
    assert lib.nvdb_hip_search_ivf_masked(None, q.ctypes.data, 2, 4, 1, mask_of.ctypes.data, ids.ctypes.data, sc.ctypes.data,
                                          cnt.ctypes.data, pr.ctypes.data, None) == 1
    assert lib.nvdb_hip_search_batch_masked(None, q.ctypes.data, 2, 4, mask_of.ctypes.data, ids.ctypes.data, sc.ctypes.data,
                                            cnt.ctypes.data, None) == 1
    assert lib.nvdb_hip_ivf_set_row_masks(None, bits.ctypes.data, 1) == 1
    assert lib.nvdb_hip_ivf_update_row_mask(None, 0, rows.ctypes.data, 2, 1) == 1
    assert lib.nvdb_hip_ivf_search_masked(None, q.ctypes.data, 2, 4, 1, mask_of.ctypes.data, ids.ctypes.data, sc.ctypes.data,
                                          cnt.ctypes.data, pr.ctypes.data, None) == 1
    assert (ids == 7).all() and (sc == 7.0).all() and (cnt == 7).all() and (pr == 7).all() and (bits == 7).all()   # nothing written
    assert nm.value == 7 and w.value == 7


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 30000])
def test_binding_packs_the_layout_of_the_header(n):
    """Row r is bit r & 31 of word r >> 5; bool planes and packed uint32 planes are both taken."""
    rs = np.random.RandomState(n)
    masks = rs.rand(3, n) < 0.5
    packed = nvdb_amd.pack_row_masks(masks, n)
    assert packed.dtype == np.uint32 and packed.shape == (3, (n + 31) // 32)
    want = np.zeros_like(packed)
    for m in range(3):
        for r in np.flatnonzero(masks[m]):
            want[m, r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    assert np.array_equal(packed, want)
    assert np.array_equal(nvdb_amd.unpack_row_masks(packed, n), masks)
    assert nvdb_amd.pack_row_masks(packed, n) is not None and np.array_equal(nvdb_amd.pack_row_masks(packed, n), packed)
    assert nvdb_amd.pack_row_masks(masks[0], n).shape == (1, (n + 31) // 32)


def test_row_mask_bits_under_address_and_ub_sanitizers(tmp_path):
    """tests/row_mask_check.cpp: the bit work the entry points run (csrc/row_mask.h), compiled into a stand-alone program with
    -fsanitize=address,undefined and run with exactly sized heap buffers: tail bits at n = 1, 31, 32, 33, 64, 65, the permute /
    inverse round trip against a naive loop, rejection of out-of-range rows and mask numbers."""
    exe = str(tmp_path / "row_mask_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "nano-vectordb_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "row_mask_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.count("checked") == 6 + 7 + 1

