"""The 4-bit PQ entry points without a GPU: declared in include/nvdb_hip.h, exported and bound with their argument types; a null
context or index is NVDB_ERR_INVALID from each with nothing written.  (The shape rules, the binding's width rule and the lifecycle need a context, which needs a device: test_gpu_pq4.py::test_lifecycle.)"""
import os
import re

import numpy as np
import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#        name -> (argument count, the arguments behind the handle; a: a buffer that must stay untouched)
CALLS = {"nvdb_hip_pq4_build": (5, lambda a: (a, a, 8, 0)), "nvdb_hip_ivf_pq4_build": (5, lambda a: (None, a, 8, 1)),
         "nvdb_hip_pq_bits": (2, lambda a: (a.ctypes.data_as(nvdb_amd.C.POINTER(nvdb_amd.C.c_uint32)),))}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_bound_and_null_handle_invalid(name):
    text = open(os.path.join(ROOT, "include", "nvdb_hip.h")).read()
    declared = set(re.findall(r"\b(nvdb_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = nvdb_amd.load_library()
    nargs, make = CALLS[name]
    assert name in declared and name in nvdb_amd.EXPORTS and len(getattr(lib, name).argtypes) == nargs and lib.nvdb_hip_abi_version() == 3
    assert "a 16-codeword trainer on the device" in text and "code widths other" in text
    buf = np.full((8, 8), 7.0, dtype=np.float32)
    assert getattr(lib, name)(None, *[x.ctypes.data if x is buf else x for x in make(buf)]) == 1
    assert (buf == 7.0).all()

