"""CPU-side checks of the partitioned probe search's C ABI: the four entry points are declared in include/nvdb_hip.h and exported
by libnvdb_hip.so, the ABI version did not move, and without a context (or without a GPU) the calls fail cleanly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nvdb_hip_set_partitions", "nvdb_hip_set_centroids", "nvdb_hip_search_partitions", "nvdb_hip_search_ivf"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(nvdb_amd.LIB_PATH):
        g.build()
    return nvdb_amd.load_library()


def test_entry_points_declared_and_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nvdb_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nvdb_[a-z0-9_]+)\s*\(", hdr))
    syms = subprocess.run(["nm", "-D", "--defined-only", nvdb_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(nvdb_[a-z0-9_]+)\b", syms))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in nvdb_hip.h"
        assert name in exported, f"{name} is not exported by libnvdb_hip.so"
        assert name in nvdb_amd.EXPORTS and hasattr(lib, name)
    assert "#define NVDB_HIP_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "nvdb_hip.h")).read()
    assert lib.nvdb_hip_abi_version() == 3
    for meth in ("set_partitions", "set_centroids", "search_partitions", "search_ivf"):
        assert callable(getattr(nvdb_amd.HipContext, meth))


def test_calls_without_a_context_fail_cleanly(lib):
    offsets = np.array([0, 5, 10], dtype=np.uint64)
    q = np.zeros((2, 8), dtype=np.float32)
    probe = np.zeros((2, 1), dtype=np.uint32)
    ids = np.full((2, 4), 7, dtype=np.uint64)
    sc = np.full((2, 4), 7.0, dtype=np.float32)
    cnt = np.full(2, 7, dtype=np.uint32)
    assert lib.nvdb_hip_set_partitions(None, offsets.ctypes.data, 2) == 1                  # NVDB_ERR_INVALID
    assert lib.nvdb_hip_set_centroids(None, q.ctypes.data) == 1
    assert lib.nvdb_hip_search_partitions(None, q.ctypes.data, 2, 4, probe.ctypes.data, 1, ids.ctypes.data, sc.ctypes.data,
                                          cnt.ctypes.data, None) == 1
    assert lib.nvdb_hip_search_ivf(None, q.ctypes.data, 2, 4, 1, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None, None) == 1
    assert (ids == 7).all() and (sc == 7.0).all() and (cnt == 7).all()                       # nothing written


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_context_to_partition_without_gpu(lib):
    """There is no CPU implementation behind the probe search either: without a device no context exists to set a table on."""
    with pytest.raises(nvdb_amd.NvdbError) as e:
        nvdb_amd.HipContext(0).set_partitions([0, 1])
    assert e.value.status == 2 and "HIP" in str(e.value)
    h = C.c_void_p()
    assert lib.nvdb_hip_create(0, C.byref(h)) == 2 and not h.value
