"""The plan arithmetic of the masked flat top-k's MFMA filter route (csrc/masked_plan.h) on the CPU: tests/masked_plan_check.cpp,
built by the Makefile's masked_plan_check target with -fsanitize=address,undefined, runs as a stand-alone program -- L against cap
and k at the edges (k = 1, 64; cap = 2; 0, k - 1, k, n rows), the prefix's rounding (multiples of 64, P == n) on exactly sized heap
planes with 0 / L - 1 / L / n live rows, 64-bit arithmetic at n = 0xFFFFFF00, the segments, and the automatic route, which keeps
tests/test_gpu_row_masks.py::test_flat's shape (n = 30000, nq up to 70) on the scan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_masked_plan_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "masked_plan_check")
    subprocess.run(["make", "-C", os.path.join(ROOT, "nano-vectordb_amd"), "masked_plan_check", f"MASKED_PLAN_CHECK={exe}"], check=True,
                   capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.count("checked") == 5
    assert "checked route" in r.stdout


def test_the_library_runs_the_checked_header():
    """The entry point and the prefix-rank kernel include masked_plan.h itself: the checker compiles the code they run, no copy."""
    csrc = os.path.join(ROOT, "nano-vectordb_amd", "csrc")
    assert '#include "masked_plan.h"' in open(os.path.join(csrc, "kernels_masked_topk.h")).read()
    src = open(os.path.join(csrc, "nvdb_masked_flat.cpp")).read()
    assert '#include "kernels_masked_topk.h"' in src and "mp_auto_filter(" in src and "mp_segments(" in src
    assert "nvdb_masked_flat.cpp" in open(os.path.join(ROOT, "nano-vectordb_amd", "Makefile")).read()
