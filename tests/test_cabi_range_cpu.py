"""CPU-side checks of the range-search boundary (no GPU needed): the two entry points are declared in include/nvdb_hip.h,
exported by libnvdb_hip.so and bound in nvdb_amd; the ABI version did not move (the change is additive); and the calls fail
loudly -- NVDB_ERR_INVALID for null pointers, NVDB_ERR_HIP where a context cannot exist for lack of a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nvdb_hip_range_search", "nvdb_hip_range_results")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(nvdb_amd.LIB_PATH):
        g.build()
    return nvdb_amd.load_library()


def test_range_entry_points_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nvdb_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nvdb_[a-z0-9_]+)\s*\(", hdr))
    syms = subprocess.run(["nm", "-D", "--defined-only", nvdb_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(nvdb_[a-z0-9_]+)\b", syms))
    for name in NAMES:
        assert name in declared, f"{name} not declared in nvdb_hip.h"
        assert name in exported, f"{name} not exported by libnvdb_hip.so"
        assert name in nvdb_amd.EXPORTS and hasattr(lib, name), f"{name} not bound in nvdb_amd"
    assert hasattr(nvdb_amd.HipContext, "range_search")
    assert lib.nvdb_hip_abi_version() == 3
    assert "#define NVDB_HIP_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "nvdb_hip.h")).read()
    # the header says which interface users know the shape from, and the statistics field names the two new routes
    raw = open(os.path.join(ROOT, "include", "nvdb_hip.h")).read()
    assert "FAISS" in raw and "range_search" in raw and "5 = range search" in raw and "range_max_mb" in raw


def test_null_arguments_are_invalid(lib):
    lims = np.zeros(4, dtype=np.uint64)
    q = np.zeros((3, 8), dtype=np.float32)
    r = np.zeros(3, dtype=np.float32)
    ids, sc = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.float32)
    assert lib.nvdb_hip_range_search(None, q.ctypes.data, 3, r.ctypes.data, lims.ctypes.data, None) == 1     # NVDB_ERR_INVALID
    assert lib.nvdb_hip_range_search(None, None, 0, None, None, None) == 1
    assert lib.nvdb_hip_range_results(None, ids.ctypes.data, sc.ctypes.data) == 1
    assert lib.nvdb_hip_range_results(None, None, None) == 1


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_range_search_fails_loudly_without_gpu(lib):
    """There is no CPU implementation behind the call: without a device no context exists to run it on (NVDB_ERR_HIP)."""
    assert lib.nvdb_hip_device_count() <= 0
    h = C.c_void_p()
    assert lib.nvdb_hip_create(0, C.byref(h)) == 2 and not h.value                                               # NVDB_ERR_HIP
    with pytest.raises(nvdb_amd.NvdbError) as e:
        nvdb_amd.HipContext(0).range_search(np.zeros((1, 8), np.float32), 0.0)
    assert e.value.status == 2 and "HIP" in str(e.value)
