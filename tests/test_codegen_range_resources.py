"""Codegen guards of the range search (no GPU needed: hipcc cross-compiles gfx950), read from `make asm` like
tests/test_codegen_resources.py: the new kernels use no scratch, and the hand-scheduled filter kernels -- which the range search
launches as they are, with another threshold array -- kept the resource usage they had before it was added
(tests/golden/filter_kernel_resources.json)."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nano-vectordb_amd")
RANGE_KERNELS = ("range_thr_kernel", "range_keep_kernel", "range_pack_kernel", "range_gather_kernel", "range_count_kernel",
                 "range_collect_kernel", "range_emit_kernel")


@pytest.fixture(scope="module")
def usage():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    report = os.path.join(PKG, "build", "resource_usage.txt")
    srcs = [os.path.join(PKG, "Makefile")] + [os.path.join(PKG, "csrc", f) for f in os.listdir(os.path.join(PKG, "csrc"))]
    # (the dump takes minutes: one made from these very sources, e.g. by tests/test_codegen_resources.py, is read as it is)
    if not os.path.exists(report) or os.path.getmtime(report) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["make", "-C", PKG, "asm"], stdout=subprocess.DEVNULL)
    out, cur = {}, None
    for line in open(report):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and cur and re.fullmatch(r"-?\d+", m.group(2)):
            out[cur][m.group(1).strip()] = int(m.group(2))
    return out


def test_range_kernels_use_no_scratch(usage):
    for name in RANGE_KERNELS:
        hits = [k for k in usage if name in k]
        assert len(hits) == 1, (name, hits)
        u = usage[hits[0]]
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    # and the code objects say the same: .private_segment_fixed_size of every range kernel in the ISA dump
    asm = open(os.path.join(PKG, "build", "nvdb_hip.s")).read()
    for name in RANGE_KERNELS:
        sizes = re.findall(r"\.amdhsa_kernel \S*%s\S*\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size (\d+)" % name, asm)
        assert sizes and all(int(v) == 0 for v in sizes), (name, sizes)


def test_filter_kernels_kept_their_resources(usage):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "filter_kernel_resources.json")))["kernels"]
    assert len(want) > 100
    have = {k: v for k, v in usage.items() if "filter_" in k}
    assert set(have) == set(want), set(have) ^ set(want)
    diff = {k: (want[k], have[k]) for k in want if want[k] != have[k]}
    assert not diff, diff
