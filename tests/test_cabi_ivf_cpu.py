"""CPU-side checks of the IVF-Flat build's C ABI: the new entry points are declared in include/nvdb_hip.h, exported by
libnvdb_hip.so and bound; the ABI version did not move; nvdb_ivf_layout_host (host only) against numpy's stable argsort and,
as a stand-alone program, under AddressSanitizer / UBSan; without a context (or without a GPU) the device calls fail cleanly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nvdb_hip_assign_rows", "nvdb_hip_train_centroids", "nvdb_ivf_layout_host", "nvdb_hip_ivf_build", "nvdb_hip_ivf_destroy",
         "nvdb_hip_ivf_last_error", "nvdb_hip_ivf_ctx", "nvdb_hip_ivf_info", "nvdb_hip_ivf_search"]


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
    for meth in ("assign_rows", "train_centroids"):
        assert callable(getattr(nvdb_amd.HipContext, meth))
    assert callable(nvdb_amd.ivf_layout_host)
    for meth in ("search", "info", "close"):
        assert callable(getattr(nvdb_amd.IvfIndex, meth))


def _layout_cases():
    rs = np.random.RandomState(7)
    return {
        "random": (rs.randint(0, 37, size=10000).astype(np.uint32), 37),
        "one partition": (np.full(500, 3, dtype=np.uint32), 7),
        "empty at both ends": (rs.randint(2, 7, size=10000).astype(np.uint32), 10),
        "no rows": (np.zeros(0, dtype=np.uint32), 5),
    }


@pytest.mark.parametrize("case", list(_layout_cases()))
def test_layout_is_the_stable_argsort(lib, case):
    assign, nparts = _layout_cases()[case]
    offsets, perm = nvdb_amd.ivf_layout_host(assign, nparts)
    assert offsets.dtype == np.uint64 and perm.dtype == np.uint32
    assert np.array_equal(perm, np.argsort(assign, kind="stable").astype(np.uint32))
    want = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=nparts))]).astype(np.uint64)
    assert np.array_equal(offsets, want) and offsets[0] == 0 and offsets[-1] == assign.size


def test_layout_refuses_bad_input_and_writes_nothing(lib):
    assign = np.array([0, 1, 2, 3, 1], dtype=np.uint32)                 # the 3 == nparts
    offsets = np.full(4, 99, dtype=np.uint64)
    perm = np.full(5, 99, dtype=np.uint32)
    assert lib.nvdb_ivf_layout_host(assign.ctypes.data, 5, 3, offsets.ctypes.data, perm.ctypes.data) == 1
    assert (offsets == 99).all() and (perm == 99).all()
    with pytest.raises(nvdb_amd.NvdbError) as e:
        nvdb_amd.ivf_layout_host(assign, 3)
    assert e.value.status == 1
    assign[3] = 2
    assert lib.nvdb_ivf_layout_host(None, 5, 3, offsets.ctypes.data, perm.ctypes.data) == 1
    assert lib.nvdb_ivf_layout_host(assign.ctypes.data, 5, 3, None, perm.ctypes.data) == 1
    assert lib.nvdb_ivf_layout_host(assign.ctypes.data, 5, 3, offsets.ctypes.data, None) == 1
    assert lib.nvdb_ivf_layout_host(assign.ctypes.data, 0xFFFFFF01, 3, offsets.ctypes.data, perm.ctypes.data) == 1
    assert (offsets == 99).all() and (perm == 99).all()
    assert lib.nvdb_ivf_layout_host(assign.ctypes.data, 5, 3, offsets.ctypes.data, perm.ctypes.data) == 0
    assert perm.tolist() == [0, 1, 4, 2, 3] and offsets.tolist() == [0, 1, 3, 5]


def test_calls_without_a_context_fail_cleanly(lib):
    cen = np.zeros((2, 8), dtype=np.float32)
    assign = np.full(4, 7, dtype=np.uint32)
    out_cen = np.full((2, 8), 7.0, dtype=np.float32)
    ids = np.full((2, 4), 7, dtype=np.uint64)
    sc = np.full((2, 4), 7.0, dtype=np.float32)
    cnt = np.full(2, 7, dtype=np.uint32)
    h = C.c_void_p(123)
    assert lib.nvdb_hip_assign_rows(None, cen.ctypes.data, 2, 0, 4, assign.ctypes.data) == 1          # NVDB_ERR_INVALID
    assert lib.nvdb_hip_train_centroids(None, 2, 1, 0, 0, None, out_cen.ctypes.data) == 1
    assert lib.nvdb_hip_ivf_build(None, cen.ctypes.data, 2, C.byref(h)) == 1 and not h.value
    assert b"null" in lib.nvdb_hip_ivf_last_error(None)
    assert lib.nvdb_hip_ivf_build(None, cen.ctypes.data, 2, None) == 1
    assert lib.nvdb_hip_ivf_search(None, cen.ctypes.data, 2, 4, 1, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None, None) == 1
    assert lib.nvdb_hip_ivf_info(None, None, None, None, None) == 1
    assert not lib.nvdb_hip_ivf_ctx(None)
    lib.nvdb_hip_ivf_destroy(None)
    assert (assign == 7).all() and (out_cen == 7.0).all() and (ids == 7).all() and (sc == 7.0).all() and (cnt == 7).all()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_index_without_gpu(lib):
    """There is no CPU implementation behind the build either: without a device there is no context to build an index from."""
    with pytest.raises(nvdb_amd.NvdbError) as e:
        nvdb_amd.IvfIndex(nvdb_amd.HipContext(0), np.zeros((2, 8), dtype=np.float32))
    assert e.value.status == 2 and "HIP" in str(e.value)


def test_layout_under_address_and_ub_sanitizers(tmp_path):
    """tests/ivf_layout_check.cpp: the layout code the entry point runs (csrc/ivf_layout.h), compiled into a stand-alone program
    with -fsanitize=address,undefined and run on the cases above with exactly sized heap buffers."""
    exe = str(tmp_path / "ivf_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "nano-vectordb_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "ivf_layout_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.count("checked") == 4
