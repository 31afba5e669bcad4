"""CPU-side checks of the compaction's C ABI: nvdb_hip_compact_rows and nvdb_hip_ivf_compact are declared in include/nvdb_hip.h,
exported by libnvdb_hip.so and bound; the ABI version did not move; without a context or an index both calls fail cleanly and
write nothing; the host arithmetic (csrc/compact_plan.h: ranks, the slab walk, the table and permutation rewrites) runs as a
stand-alone program under AddressSanitizer / UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nvdb_hip_compact_rows", "nvdb_hip_ivf_compact"]


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
    assert callable(nvdb_amd.HipContext.compact_rows) and callable(nvdb_amd.IvfIndex.compact)


def test_calls_without_a_context_fail_cleanly(lib):
    out_n = C.c_uint64(7)
    old = np.full(4, 7, dtype=np.uint32)
    assert lib.nvdb_hip_compact_rows(None, 0, C.byref(out_n), old.ctypes.data) == 1         # NVDB_ERR_INVALID
    assert lib.nvdb_hip_compact_rows(None, 0, None, None) == 1
    assert lib.nvdb_hip_ivf_compact(None, 0, C.byref(out_n)) == 1
    assert lib.nvdb_hip_ivf_compact(None, 0, None) == 1
    assert out_n.value == 7 and (old == 7).all()                                            # nothing written


def test_compact_plan_under_address_and_ub_sanitizers(tmp_path):
    """tests/compact_plan_check.cpp through the Makefile's compact_plan_check target (g++ -fsanitize=address,undefined): the slab cut
    against a simulation that moves rows one at a time, "a direct slab's destination ends at or before its start", ranks at the
    partition offsets and the permutation rewrite against naive loops, on eight planes x n = 1, 63, 64, 65, 4097 x slab = 64, 4096,
    all with exactly sized heap buffers."""
    exe = str(tmp_path / "compact_plan_check")
    subprocess.run(["make", "-C", os.path.join(ROOT, "nano-vectordb_amd"), "compact_plan_check", "COMPACT_PLAN_CHECK=" + exe], check=True,
                   stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.count("checked") == 5 * 2 * 8
