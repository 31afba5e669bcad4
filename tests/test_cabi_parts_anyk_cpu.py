"""CPU-side checks of the probe search for any k (no GPU needed): the three entry points are declared in include/nvdb_hip.h,
exported by libnvdb_hip.so and bound in nvdb_amd; the ABI version did not move (the change is additive); without a context or an
index every call fails cleanly and writes nothing; without a device there is nothing to run them on; and the host-side arithmetic
(csrc/parts_anyk_plan.h: a query's slab and its route, the sub-batch cut, a sub-batch's plan) runs as a stand-alone program under
AddressSanitizer / UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nvdb_hip_search_partitions_anyk", "nvdb_hip_search_ivf_anyk", "nvdb_hip_ivf_search_anyk"]


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
        assert name in nvdb_amd.EXPORTS and hasattr(lib, name), f"{name} is not bound in nvdb_amd"
    assert "#define NVDB_HIP_ABI_VERSION 3" in text
    assert lib.nvdb_hip_abi_version() == 3
    for meth in ("search_partitions_anyk", "search_ivf_anyk"):
        assert callable(getattr(nvdb_amd.HipContext, meth))
    assert callable(getattr(nvdb_amd.IvfIndex, "search_anyk"))
    assert "8 = probe search, any k" in text


@pytest.mark.parametrize("k", [10, 100])
def test_calls_without_a_context_fail_cleanly(lib, k):
    q = np.zeros((2, 8), dtype=np.float32)
    probe = np.zeros((2, 1), dtype=np.uint32)
    mask_of = np.zeros(2, dtype=np.uint32)
    ids = np.full((2, k), 7, dtype=np.uint64)
    sc = np.full((2, k), 7.0, dtype=np.float32)
    cnt = np.full(2, 7, dtype=np.uint32)
    pr = np.full((2, 1), 7, dtype=np.uint32)
    for masked in (0, 1):
        assert lib.nvdb_hip_search_partitions_anyk(None, q.ctypes.data, 2, k, probe.ctypes.data, 1, mask_of.ctypes.data, masked, ids.ctypes.data,
                                                   sc.ctypes.data, cnt.ctypes.data, None) == 1                 # NVDB_ERR_INVALID
        assert lib.nvdb_hip_search_ivf_anyk(None, q.ctypes.data, 2, k, 1, mask_of.ctypes.data, masked, ids.ctypes.data, sc.ctypes.data,
                                            cnt.ctypes.data, pr.ctypes.data, None) == 1
        assert lib.nvdb_hip_ivf_search_anyk(None, q.ctypes.data, 2, k, 1, mask_of.ctypes.data, masked, ids.ctypes.data, sc.ctypes.data,
                                            cnt.ctypes.data, pr.ctypes.data, None) == 1
    # ... also with nothing to do, and with null pointers all round
    assert lib.nvdb_hip_search_partitions_anyk(None, None, 0, k, None, 0, None, 0, None, None, None, None) == 1
    assert lib.nvdb_hip_search_ivf_anyk(None, None, 0, k, 0, None, 0, None, None, None, None, None) == 1
    assert lib.nvdb_hip_ivf_search_anyk(None, None, 0, k, 0, None, 0, None, None, None, None, None) == 1
    assert (ids == 7).all() and (sc == 7.0).all() and (cnt == 7).all() and (pr == 7).all()                    # nothing written


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_probe_search_for_any_k_fails_loudly_without_gpu(lib):
    """There is no CPU implementation behind these calls either: without a device no context exists to run them on (NVDB_ERR_HIP)."""
    assert lib.nvdb_hip_device_count() <= 0
    h = C.c_void_p()
    assert lib.nvdb_hip_create(0, C.byref(h)) == 2 and not h.value                                         # NVDB_ERR_HIP
    for call in (lambda c: c.search_partitions_anyk(np.zeros((1, 8), np.float32), 100, [[0]]),
                 lambda c: c.search_ivf_anyk(np.zeros((1, 8), np.float32), 100, 1)):
        with pytest.raises(nvdb_amd.NvdbError) as e:
            call(nvdb_amd.HipContext(0))
        assert e.value.status == 2 and "HIP" in str(e.value)


def test_parts_anyk_plan_under_address_and_ub_sanitizers(tmp_path):
    """tests/parts_anyk_plan_check.cpp: the arithmetic the entry points run (csrc/parts_anyk_plan.h), compiled into a stand-alone
    program with -fsanitize=address,undefined and run with exactly sized heap buffers: slabs around 8192 / 8193 keys (the LDS /
    global sort boundary), plans with and without long lists, a budget that cuts 70 queries on a 20000-row union into sub-batches of
    three, one that forces one query per sub-batch, the 2^32-entry cut and the 2^31-result limit."""
    exe = str(tmp_path / "parts_anyk_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "nano-vectordb_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "parts_anyk_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.count("checked") == 49 + 6 + 1 + 6 + 1
    for what in ("slab k=8193 len=8193 ", "5 long lists, 81920 keys", "cut three queries per sub-batch: 24 sub-batches", "cut one query per sub-batch: 70 ",
                 "2^32 entries", "plan 2^31 results"):
        assert what in r.stdout, what
