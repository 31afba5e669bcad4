"""nvdb_hip_pq_train / nvdb_hip_ivf_pq_train without a GPU: declared, exported, bound; a null context or index is NVDB_ERR_INVALID
with nothing written, whatever else is null.  (The null-output and no-corpus statuses need a context: test_gpu_pq_train.py.)"""
import os
import re

import numpy as np
import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nvdb_hip_pq_train", "nvdb_hip_ivf_pq_train"]


def test_declared_exported_bound():
    text = open(os.path.join(ROOT, "include", "nvdb_hip.h")).read()
    declared = set(re.findall(r"\b(nvdb_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = nvdb_amd.load_library()
    for name in NAMES:
        assert name in declared and name in nvdb_amd.EXPORTS and len(getattr(lib, name).argtypes) == 8, name
    assert "PQ_TRAIN_CHUNK" in text and lib.nvdb_hip_abi_version() == 3


@pytest.mark.parametrize("name", NAMES)
def test_null_handle_writes_nothing(name):
    fn = getattr(nvdb_amd.load_library(), name)
    out = np.full((4, 256, 2), 7.0, dtype=np.float32)
    err = np.full(2, 7.0)
    assert fn(None, 4, 2, 1, 0, None, out.ctypes.data, err.ctypes.data) == 1
    assert fn(None, 4, 2, 1, 0, None, None, None) == 1
    assert (out == 7.0).all() and (err == 7.0).all()

