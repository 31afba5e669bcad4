"""The PQ candidate scan's nine entry points: declared in include/nvdb_hip.h, exported by the product library, bound by
nvdb_amd with their argument types; the ABI version stays 3."""
import os
import re

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nvdb_hip_pq_build", "nvdb_hip_pq_info", "nvdb_hip_pq_download_codes", "nvdb_hip_pq_search_partitions", "nvdb_hip_pq_search_ivf",
         "nvdb_hip_pq_refine_ivf", "nvdb_hip_ivf_pq_build", "nvdb_hip_ivf_pq_search", "nvdb_hip_ivf_pq_refine"]


def test_pq_names_declared_exported_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nvdb_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nvdb_[a-z0-9_]+)\s*\(", hdr))
    lib = nvdb_amd.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in nvdb_amd.EXPORTS, name
        assert getattr(lib, name).argtypes, name
    assert "#define NVDB_HIP_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "nvdb_hip.h")).read()
    assert lib.nvdb_hip_abi_version() == 3
