"""The product library holds shadow_i8c_kernel -- the 16x16x64 logged int8 kernel whose first-stage test compares raw accumulator
bits, for a filter shadow under one common scale -- at d = 768 on 4 and on 8 waves, both rendezvous variants: the same residency
as its per-row twin filter_i8s_kernel (8 waves: two per SIMD), no scratch, no spills, the same MFMAs per tile, and fewer v_fma_f32
behind the first barrier (the per-row test spends one per accumulator value).  Read off `make -C nano-vectordb_amd asm_product`.
No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nano-vectordb_amd")


@pytest.fixture(scope="module")
def product():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", PKG, "asm_product"], stdout=subprocess.DEVNULL)
    usage, cur = {}, None
    for line in open(os.path.join(PKG, "build", "resource_usage_product.txt")):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            usage[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and cur:
            usage[cur][m.group(1).strip()] = m.group(2)
    names = subprocess.run(["c++filt"] + list(usage), capture_output=True, text=True, check=True).stdout.splitlines()
    asm = open(os.path.join(PKG, "build", "asm_product", "nvdb_launch_i8.s")).read()
    out = {}
    for mangled, pretty in zip(usage, names):
        a = asm.index(f"\n{mangled}:")
        body = asm[a:asm.index(".Lfunc_end", a)]
        out[re.sub(r"\(.*", "", pretty).replace("void nvdbhip::", "")] = dict(usage[mangled], body=body)
    return out


def _loop(k):
    return k["body"][k["body"].index("s_barrier"):]


def _folds(k):
    """v_max3_f32 of the loop and the tail whose two folded operands are different registers: one per pair of accumulator values
    (a fold that names one register twice tests half of the values)"""
    return sum(1 for a, b in re.findall(r"v_max3_f32 v\d+, v\d+, (v\d+), (v\d+)", _loop(k)) if a != b)


@pytest.mark.parametrize("sync", ["true", "false"])
def test_eight_wave_build(product, sync):
    k, twin = product[f"shadow_i8c_kernel<768, {sync}, 6, 8>"], product[f"filter_i8s_kernel<768, {sync}, false, 6, 8>"]
    assert int(k["VGPRs"]) <= 128 and 96 <= int(k["AGPRs"]) <= 128 and int(k["Occupancy"]) == 2, {x: k[x] for x in k if x != "body"}
    assert int(k["ScratchSize"]) == 0 and int(k["SGPRs Spill"]) == 0 and int(k["VGPRs Spill"]) == 0
    assert k["body"].count("v_mfma_i32_16x16x64_i8") == twin["body"].count("v_mfma_i32_16x16x64_i8") == 96
    assert _folds(k) >= 3 * 8                                             # 16 values per block: both halves of the loop and the tail
    assert _loop(k).count("v_fma_f32") < _loop(twin).count("v_fma_f32"), (_loop(k).count("v_fma_f32"), _loop(twin).count("v_fma_f32"))
    assert _loop(k).count("global_load_lds_dwordx4") < _loop(twin).count("global_load_lds_dwordx4")      # no scales piece


@pytest.mark.parametrize("sync", ["true", "false"])
def test_four_wave_build(product, sync):
    k, twin = product[f"shadow_i8c_kernel<768, {sync}, 6, 4>"], product[f"filter_i8s_kernel<768, {sync}, false, 6, 4>"]
    assert int(k["AGPRs"]) >= 192 and int(k["Occupancy"]) == 1 and int(k["VGPRs"]) + int(k["AGPRs"]) <= 512
    assert int(k["ScratchSize"]) == 0 and int(k["SGPRs Spill"]) == 0 and int(k["VGPRs Spill"]) == 0
    assert k["body"].count("v_mfma_i32_16x16x64_i8") == 192 and "v_mfma_i32_32x32x32_i8" not in k["body"]
    assert _folds(k) >= 3 * 16                                            # 32 values per block
    assert _loop(k).count("v_fma_f32") < _loop(twin).count("v_fma_f32"), (_loop(k).count("v_fma_f32"), _loop(twin).count("v_fma_f32"))
    assert _loop(k).count("global_load_lds_dwordx4") < _loop(twin).count("global_load_lds_dwordx4")
