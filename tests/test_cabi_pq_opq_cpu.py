"""The OPQ entry points without a GPU: declared in include/nvdb_hip.h, exported and bound with their argument types; a null context
or index is NVDB_ERR_INVALID from each, as with the existing PQ calls, with nothing written.  (The null rotation, the shape rules, the
range errors and a shadow without a rotation need a context, which needs a device: test_gpu_pq_opq.py::test_state_arguments_and_index.)"""
import os
import re

import numpy as np
import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#        name -> (argument count, the arguments behind the handle; a: a buffer that must stay untouched)
CALLS = {"nvdb_hip_pq_build_opq": (5, lambda a: (a, a, 4, 0)), "nvdb_hip_ivf_pq_build_opq": (5, lambda a: (a, a, 4, 1)),
         "nvdb_hip_pq_train_opq": (10, lambda a: (a, 4, 2, 1, 0, None, a, a, 0)), "nvdb_hip_ivf_pq_train_opq": (10, lambda a: (a, 4, 2, 1, 0, None, a, a, 1)),
         "nvdb_hip_pq_rotation": (3, lambda a: (a.ctypes.data_as(nvdb_amd.C.POINTER(nvdb_amd.C.c_uint32)), a)), "nvdb_hip_pq_rotated_rows": (4, lambda a: (0, 1, a)),
         "nvdb_hip_pq_rotate": (4, lambda a: (a, 1, a))}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_bound_and_null_handle_invalid(name):
    text = open(os.path.join(ROOT, "include", "nvdb_hip.h")).read()
    declared = set(re.findall(r"\b(nvdb_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = nvdb_amd.load_library()
    nargs, make = CALLS[name]
    assert name in declared and name in nvdb_amd.EXPORTS and len(getattr(lib, name).argtypes) == nargs and lib.nvdb_hip_abi_version() == 3
    assert "learning the rotation" in text and "OPQ rotations" not in text
    buf = np.full((8, 8), 7.0, dtype=np.float32)
    for args in (make(buf), tuple(None if x is buf else x for x in make(buf))):      # ... whatever else is null
        assert getattr(lib, name)(None, *[x.ctypes.data if x is buf else x for x in args]) == 1
    assert (buf == 7.0).all()
