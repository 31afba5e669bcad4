"""Option shadow_exact_thr without a GPU: the option table takes it (default 1: include/nvdb_hip.h, INTEGRATION.md section 4b, the
context's field) and the plan of a search that streams the int8 shadow -- route, bootstrap, chunk boundaries -- does not depend on
it: the option changes what the thresholding selects compute, never which launches are enqueued.  (That no filter kernel moved is
tests/test_codegen_range_resources.py::test_filter_kernels_kept_their_resources, untouched.)"""
import os
import re

import pytest

import nvdb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16 = nvdb_amd.DT_F16
SHADOW = dict(n=10_000_000, dim=768, fdim=768, dtype=F16, owned=1, num_cu=256, has_shadow8=1, q8shadow=1)


def _plan(shape, nq, k, options):
    return nvdb_amd.debug_plan(shape, nq, k, options)


@pytest.mark.parametrize("nq,k", [(1024, 10), (1024, 64), (64, 10), (1, 1), (300, 100)])
def test_the_plan_does_not_depend_on_the_option(nq, k):
    base = _plan(SHADOW, nq, k, {})
    assert base["filter_shadow"] == 1 and base["route"] == 2
    for v in (0, 1, 7):                                       # any non-zero value is "on"
        assert _plan(SHADOW, nq, k, {"shadow_exact_thr": v}) == base, v
    small = dict(SHADOW, n=200_009)
    assert _plan(small, nq, k, {"shadow_exact_thr": 0}) == _plan(small, nq, k, {}) == _plan(small, nq, k, {"shadow_exact_thr": 1})


def test_the_flagship_plan_is_the_one_on_record():
    """growth 6 over a 1024-tile bootstrap: four chunks (what tests/test_q8_auto_plan_cpu.py pins, here with the option spelled out)"""
    p = _plan(SHADOW, 1024, 10, {"shadow_exact_thr": 1})
    assert p["growth"] == 6 and p["boot_tiles"] == 1024 and p["boot"] == 0 and p["r0"] == 0
    assert p["chunk_lo"] == [0, 196_608, 1_179_648, 7_077_888] and p["chunk_hi"][-1] == p["n_al"]


def test_option_is_accepted_and_unknown_neighbours_are_not():
    for v in (1, 0, 1):                                       # round trip: on, off, on again
        _plan(SHADOW, 8, 10, {"shadow_exact_thr": v})
    with pytest.raises(nvdb_amd.NvdbError) as e:
        _plan(SHADOW, 8, 10, {"shadow_exact_threshold": 1})
    assert "unknown option" in str(e.value)
    # (a context of the product library needs a device; that the key is outside the developer-only block is read from the source)
    src = open(os.path.join(ROOT, "nano-vectordb_amd", "csrc", "nvdb_corpus.cpp")).read()
    assert 'k == "shadow_exact_thr"' in src and "#ifdef NVDB_HIP_DEV" not in src[src.index('k == "zero_copy"'):src.index('k == "shadow_exact_thr"')]


def test_default_is_on_and_documented():
    ctx_h = open(os.path.join(ROOT, "nano-vectordb_amd", "csrc", "nvdb_ctx.h")).read()
    assert re.search(r"int64_t opt_shadow_exact_thr = 1;", ctx_h)
    assert '"shadow_exact_thr"' in open(os.path.join(ROOT, "include", "nvdb_hip.h")).read()
    row = [ln for ln in open(os.path.join(ROOT, "INTEGRATION.md")) if ln.startswith("| `shadow_exact_thr`")]
    assert len(row) == 1 and row[0].split("|")[2].strip() == "1", row


def test_abi_is_unchanged():
    lib = nvdb_amd.load_library()
    assert lib.nvdb_hip_abi_version() == 3
    fields = [f for f, _ in nvdb_amd.ScanStats._fields_]
    assert "candidates" in fields and "i8_stage1_tiles" in fields and not any("exact_thr" in f for f in fields)
