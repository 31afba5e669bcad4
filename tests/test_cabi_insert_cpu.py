"""CPU-side checks of the insertion's C ABI: nvdb_hip_reserve_rows, nvdb_hip_insert_rows and nvdb_hip_ivf_add_rows are declared in
include/nvdb_hip.h, exported by libnvdb_hip.so and bound; the ABI version did not move; without a context or an index the calls
fail cleanly and write nothing; the host arithmetic (csrc/insert_plan.h: counts, shifts, the new table, the new rows' positions,
the descending slab walk, the permutation rewrite, the capacity rule) runs as a stand-alone program under AddressSanitizer / UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nvdb_hip_reserve_rows", "nvdb_hip_insert_rows", "nvdb_hip_ivf_add_rows"]


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
    assert callable(nvdb_amd.HipContext.reserve_rows) and callable(nvdb_amd.HipContext.insert_rows) and callable(nvdb_amd.IvfIndex.add_rows)
    # what the header promises to say plainly
    block = text[text.index("insertion: the compaction's mirror image"):text.index("nvdb_hip_ivf_add_rows(struct")]
    assert "OLD PLUS NEW" in block and '"insert_growth_pct"' in block and '"compact_slab_rows"' in block
    for word in ("device group", "_dev stream forms", "updating centroids", "giving HBM back", "anywhere but at the"):
        assert word in block, word


def test_calls_without_a_context_fail_cleanly(lib):
    out_n = C.c_uint64(7)
    first = C.c_uint64(7)
    new_rows = np.full(4, 7, dtype=np.uint64)
    assign = np.full(4, 7, dtype=np.uint32)
    rows = np.zeros((4, 8), dtype=np.float32)
    part_of = np.zeros(4, dtype=np.uint32)
    assert lib.nvdb_hip_reserve_rows(None, 100) == 1                                         # NVDB_ERR_INVALID
    assert lib.nvdb_hip_insert_rows(None, rows.ctypes.data, None, 4, part_of.ctypes.data, new_rows.ctypes.data, C.byref(out_n)) == 1
    assert lib.nvdb_hip_insert_rows(None, None, None, 0, None, None, None) == 1
    assert lib.nvdb_hip_ivf_add_rows(None, rows.ctypes.data, None, 4, C.byref(first), assign.ctypes.data) == 1
    assert lib.nvdb_hip_ivf_add_rows(None, None, None, 0, None, None) == 1
    assert out_n.value == 7 and first.value == 7 and (new_rows == 7).all() and (assign == 7).all()   # nothing written


def test_insert_plan_under_address_and_ub_sanitizers(tmp_path):
    """tests/insert_plan_check.cpp through the Makefile's insert_plan_check target (g++ -fsanitize=address,undefined): counts,
    shifts, the new table and the new rows' positions against "old rows then new rows, std::stable_sort by partition"; the
    descending slab walk simulated in an array of exactly n + m rows with a bounce buffer of exactly one slab ("a direct slab writes
    at or beyond its own end"); the permutation and inverse rewrite; the capacity rule -- on nine insertion patterns (m = 1 at the
    end / into the empty partition 0 / into partition 1, one row per partition, all rows into partition 0, 65 into a middle one,
    random, all into the last, a shift beyond a slab) x n = 1, 31, 32, 33, 63, 64, 65, 4097 x slab = 64, 4096 x a table with empty
    partitions / no table."""
    exe = str(tmp_path / "insert_plan_check")
    subprocess.run(["make", "-C", os.path.join(ROOT, "nano-vectordb_amd"), "insert_plan_check", "INSERT_PLAN_CHECK=" + exe], check=True,
                   stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.count("checked") == 8 * 2 * 9 * 2
