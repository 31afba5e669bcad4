"""The L2-metric PQ entry points without a GPU: declared in include/nvdb_hip.h, exported and bound with their argument types; a
null context or index, an unknown metric and null outputs are NVDB_ERR_INVALID with nothing written; no context without a device.
(What a context answers is test_gpu_pq_l2.py's.)"""
import os
import re

import numpy as np
import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32p = nvdb_amd.C.POINTER(nvdb_amd.C.c_uint32)
#        name -> (argument count, argument sets behind a null handle; a: a buffer that must stay untouched)
CALLS = {"nvdb_hip_pq_set_metric": (2, lambda a: [(1,), (0,), (2,)]), "nvdb_hip_ivf_pq_set_metric": (2, lambda a: [(1,), (7,)]),
         "nvdb_hip_pq_metric": (2, lambda a: [(a.ctypes.data_as(u32p),), (None,)]),
         "nvdb_hip_pq_norms": (4, lambda a: [(0, 8, a.ctypes.data), (0, 8, None)])}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_bound_and_null_handle_invalid(name):
    text = open(os.path.join(ROOT, "include", "nvdb_hip.h")).read()
    declared = set(re.findall(r"\b(nvdb_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = nvdb_amd.load_library()
    nargs, make = CALLS[name]
    assert name in declared and name in nvdb_amd.EXPORTS and len(getattr(lib, name).argtypes) == nargs and lib.nvdb_hip_abi_version() == 3
    assert "The L2 METRIC" in text and "L2 asymmetric-distance tables" not in text
    buf = np.full(8, 7.0, dtype=np.float32)
    for args in make(buf):
        assert getattr(lib, name)(None, *args) == 1
    assert (buf == 7.0).all()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_context_without_a_gpu():
    with pytest.raises(nvdb_amd.NvdbError) as e:
        nvdb_amd.HipContext(0)
    assert e.value.status == 2
    assert all(hasattr(cls, m) for cls in (nvdb_amd.HipContext, nvdb_amd.IvfIndex) for m in ("pq_set_metric", "pq_metric", "pq_norms"))
