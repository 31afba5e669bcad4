"""The developer library's in-kernel clock entry points (nvdb_hip_debug_clock, nvdb_hip_debug_clock_i8; include/nvdb_hip_dev.h,
run with -m gpu on an MI355X): every stamped build they still launch returns NVDB_OK with sane numbers, a retired or unknown
variant number is NVDB_ERR_INVALID, and the context searches afterwards exactly as before -- the stamped builds write their
clock pairs behind the rendezvous counters and must leave it usable.

The corpus is the smallest d = 768 one on which a 256-query search takes the MFMA filter route by itself (nvdb_amd.debug_plan):
the clock calls run on the workspace that search leaves.  The brackets on the clock are sanity brackets around the part's clock
range, not a measurement."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import nvdb_amd

pytestmark = pytest.mark.gpu

SEED = 20240613
D, NQ, K = 768, 256, 10
NVDB_OK, NVDB_ERR_INVALID = 0, 1
CALL_LIMIT_S = 60                                # per call into the library: a hang ends the run instead of holding the GPU

# entry point, floats it writes, surviving variants, retired / unknown numbers, (mean, max) tile-loop duration slots
ENTRIES = {
    "f16": (nvdb_amd.DT_F16, "nvdb_hip_debug_clock", 22, (0, 20), (1, 15), (4, 5)),
    "i8": (nvdb_amd.DT_I8, "nvdb_hip_debug_clock_i8", 8, (0, 10, 20, 30, 35), (1, 11, 15, 31), (6, 7)),
}


def limited(fn, *args):
    """fn(*args) under its own time limit (a watchdog thread: it also fires while the call sits inside the library)."""
    faulthandler.dump_traceback_later(CALL_LIMIT_S, exit=True)
    try:
        return fn(*args)
    finally:
        faulthandler.cancel_dump_traceback_later()


def smallest_filter_n(dtype, num_cu):
    """The smallest corpus on which NQ queries for the K best take the filter route (2) with default options."""
    def route(n):
        return nvdb_amd.debug_plan(dict(n=n, dim=D, dtype=dtype, owned=1, num_cu=num_cu), NQ, K)["route"]
    lo, hi = 1, 1 << 24
    assert route(hi) == 2
    while lo < hi:                               # the first n of the route: below it the plan is the exact path
        mid = (lo + hi) // 2
        if route(mid) == 2:
            hi = mid
        else:
            lo = mid + 1
    assert route(lo) == 2 and (lo == 1 or route(lo - 1) != 2)
    return lo


@pytest.mark.parametrize("kind", list(ENTRIES))
def test_clock_entry_points(kind):
    import torch
    dtype, entry, nout, live, retired, (i_mean, i_max) = ENTRIES[kind]
    n = smallest_filter_n(dtype, torch.cuda.get_device_properties(0).multi_processor_count)
    c = nvdb_amd.HipContext(0, dev=True)
    try:
        limited(c.generate_corpus, SEED, n, D, dtype)
        q = nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ, D)
        ids0, sc0 = limited(c.search_batch, q, K)
        st = c.stats()
        assert st["path"] == 2 and st["bound_violations"] == 0, st
        fn = getattr(c.lib, entry)
        for v in live:
            out = (C.c_float * nout)()
            rc = limited(fn, c.h, v, NQ, 0.05, out)
            print(kind, "n", n, "variant", v, "rc", rc, "out", [round(x, 4) for x in out])
            assert rc == NVDB_OK, (v, c.lib.nvdb_hip_last_error(c.h))
            assert out[0] > 0, (v, list(out))
            assert 0.3 < out[1] < 3.5, (v, list(out))
            assert out[i_mean] <= out[i_max], (v, list(out))
        for v in retired:
            out = (C.c_float * nout)()
            assert limited(fn, c.h, v, NQ, 0.05, out) == NVDB_ERR_INVALID, v
            assert b"unknown variant" in c.lib.nvdb_hip_last_error(c.h)
        ids1, sc1 = limited(c.search_batch, q, K)
        st = c.stats()
        assert st["path"] == 2 and st["bound_violations"] == 0, st
        assert np.array_equal(ids0, ids1) and np.array_equal(sc0.view(np.uint32), sc1.view(np.uint32))
    finally:
        c.close()
