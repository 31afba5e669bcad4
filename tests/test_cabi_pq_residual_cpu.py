"""The residual PQ shadow's entry points without a GPU: exported and bound with their argument types; a null context or index is
NVDB_ERR_INVALID from each, with nothing written.  (Everything else needs a context: test_gpu_pq_residual.py.)"""
import numpy as np
import pytest

import nvdb_amd

#        name -> the arguments behind the handle
CALLS = {"nvdb_hip_pq_build_residual": lambda a: (a, 4), "nvdb_hip_ivf_pq_build_residual": lambda a: (a, 4),
         "nvdb_hip_pq_train_residual": lambda a: (4, 2, 1, 0, None, a, None), "nvdb_hip_ivf_pq_train_residual": lambda a: (4, 2, 1, 0, None, a, None),
         "nvdb_hip_pq_kind": lambda a: (a.ctypes.data_as(nvdb_amd.C.POINTER(nvdb_amd.C.c_uint32)),), "nvdb_hip_pq_reconstruct": lambda a: (0, 1, a)}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_bound_and_null_handle_invalid(name):
    lib = nvdb_amd.load_library()
    assert name in nvdb_amd.EXPORTS and getattr(lib, name).argtypes and lib.nvdb_hip_abi_version() == 3
    buf = np.full((4, 256, 2), 7.0, dtype=np.float32)
    args = CALLS[name](buf)
    assert getattr(lib, name)(None, *[x.ctypes.data if x is buf else x for x in args]) == 1
    assert (buf == 7.0).all()
