"""The product library holds the 8-wave builds of the 16x16x64 logged int8 kernel at d = 768 that the flat search runs on its dense
chunks (option i8_dense8) -- both rendezvous variants -- and they fit two waves per SIMD: at most 128 VGPRs and 128 AGPRs, occupancy 2,
no scratch, no spills.  Read off `make -C nano-vectordb_amd asm_product`, the resource report (-Rpass-analysis=kernel-resource-usage)
of the launchers' translation unit compiled as the product compiles it (without NVDB_HIP_DEV).  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nano-vectordb_amd")


@pytest.fixture(scope="module")
def product_usage():
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
    return {re.sub(r"\(.*", "", pretty).replace("void nvdbhip::", ""): usage[mangled] for mangled, pretty in zip(usage, names)}


@pytest.mark.parametrize("sync", ["true", "false"])
def test_product_holds_the_eight_wave_build(product_usage, sync):
    name = f"filter_i8s_kernel<768, {sync}, false, 6, 8>"
    assert name in product_usage, sorted(k for k in product_usage if "filter_i8s" in k)
    u = product_usage[name]
    assert int(u["VGPRs"]) <= 128 and int(u["AGPRs"]) <= 128 and int(u["Occupancy"]) == 2, u
    assert int(u["ScratchSize"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["VGPRs Spill"]) == 0, u


def test_product_still_holds_the_four_wave_build(product_usage):
    for sync in ("true", "false"):
        assert f"filter_i8s_kernel<768, {sync}, false, 6, 4>" in product_usage
    # the developer-only stamped build stays out of the product
    assert not [k for k in product_usage if k.startswith("filter_i8s_kernel<768, true, true")]
