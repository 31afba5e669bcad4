"""Codegen guard of the compaction kernels (no GPU needed: hipcc cross-compiles gfx950), in the manner of
tests/test_codegen_range_parts_resources.py but from a dump of the one translation unit that holds them: every build of the mover
(16 / 8 / 4 / 2 / 1-byte lanes), the two rank kernels, the plane squeeze and the map kernel compile with no scratch and no spilled
register -- read from the compiler's resource remarks AND from the code object's metadata in the ISA dump -- and take the VGPRs
and LDS that tests/golden/compact_kernel_resources.json records."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nano-vectordb_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "compact_kernel_resources.json")
MOVER_LANES = {"IDv4_jE": "uint4", "IDv2_jE": "uint2", "IjE": "uint32", "ItE": "uint16", "IhE": "uint8"}
SINGLE = ("compact_tile_rank_kernel", "compact_rank_add_kernel", "compact_planes_kernel", "compact_map_kernel")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("compact_asm")
    asm = str(out / "nvdb_compact.s")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "-Wall",
                        "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-x", "hip", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", asm, os.path.join(PKG, "csrc", "nvdb_compact.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            usage[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and cur and re.fullmatch(r"-?\d+", m.group(2)):
            usage[cur][m.group(1).strip()] = int(m.group(2))
    return usage, open(asm).read()


def kernels(usage):
    """short name -> mangled name"""
    out = {}
    for k in usage:
        if "compact_move_kernel" in k:
            lanes = [name for tag, name in MOVER_LANES.items() if "compact_move_kernel" + tag in k]
            assert len(lanes) == 1, k
            out["compact_move_kernel<%s>" % lanes[0]] = k
        for name in SINGLE:
            if name in k:
                out[name] = k
    return out


def test_compact_kernels_use_no_scratch_and_match_the_recorded_resources(dump):
    usage, asm = dump
    ks = kernels(usage)
    assert sorted(ks) == sorted(["compact_move_kernel<%s>" % v for v in MOVER_LANES.values()] + list(SINGLE)), sorted(ks)
    for name, k in ks.items():
        u = usage[k]
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        # the code object's own metadata
        m = re.search(r"\.amdhsa_kernel %s\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size (\d+)" % re.escape(k), asm)
        assert m and int(m.group(1)) == 0, name
        meta = re.search(r"\.name:\s+%s\n(?:.*\n)*?\s*\.wavefront_size:" % re.escape(k), asm)
        assert meta, name
        block = meta.group(0)
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0 and int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1)) == 0
    golden = json.load(open(GOLDEN))
    got = {name: {"vgprs": usage[k]["VGPRs"], "lds_bytes": usage[k]["LDS Size"]} for name, k in ks.items()}
    assert got == golden["kernels"], got
