"""The 16-codeword trainer's entry points without a GPU: declared in include/nvdb_hip.h, exported and bound with their argument
types; a null context or index is NVDB_ERR_INVALID from each with nothing written.  (Everything else needs a device:
test_gpu_pq4_train.py.)"""
import os
import re

import numpy as np
import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["nvdb_hip_pq4_train", "nvdb_hip_ivf_pq4_train"])
def test_declared_bound_and_null_handle_invalid(name):
    text = open(os.path.join(ROOT, "include", "nvdb_hip.h")).read()
    declared = set(re.findall(r"\b(nvdb_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = nvdb_amd.load_library()
    assert name in declared and name in nvdb_amd.EXPORTS and len(getattr(lib, name).argtypes) == 10 and lib.nvdb_hip_abi_version() == 3
    out, err = np.full((8, 16, 8), 7.0, dtype=np.float32), np.full(2, 7.0)
    assert getattr(lib, name)(None, None, 8, 2, 1, 0, None, out.ctypes.data, err.ctypes.data, 0) == 1
    assert (out == 7.0).all() and (err == 7.0).all()
