"""Refine phase timing on the GPU (option refine_dbg_q; reference CUDA_DBG_TIMING / CUDA_DBG_Q and the eval app's dbg TSV).

The STAMP build of every refine kernel template must return the product kernel's ids and distance bits, and the timing struct's seven
dbg_* fields must carry the reference's reduction (averages over dbg_q = min(option, Q) queries, shares as fractions);
with the option off they stay zero.  The CLI writes the reference's one-row TSV under CUDA_DBG_TIMING=1 and nothing without it."""
import os
import subprocess

import numpy as np
import pytest

import nvdb_amd
import pyoracle as po
from golden_inputs import make_case_inputs

pytestmark = pytest.mark.gpu

SEED = 20240613
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nano-vectordb_amd", "bin")
DBG_FIELDS = ("dbg_q", "dbg_dist_cycles_avg", "dbg_write_cycles_avg", "dbg_merge_cycles_avg", "dbg_dist_pct", "dbg_write_pct", "dbg_merge_pct")
TSV_COLUMNS = ["k", "Q", "R", "nprobe", "refine_k", "kernel_mode", "cuda_threads", "cuda_nwarps", "cuda_shmem_bytes", "cuda_shmem_optin",
               "cuda_pinned", "cuda_return_dist", "git_rev", "dbg_q", "dbg_dist_cycles_avg", "dbg_write_cycles_avg", "dbg_merge_cycles_avg",
               "dbg_dist_pct", "dbg_write_pct", "dbg_merge_pct"]


@pytest.fixture(scope="module")
def ctx():
    c = nvdb_amd.HipContext(0)
    yield c
    c.close()


def _case(oracle, tag, d, R, Q=40, n=30000):
    rs = np.random.RandomState(d + R)
    base32 = nvdb_amd.synth_rows_f32(SEED + 30, 0, n, d)
    base, dt = (oracle.f32_to_f16(base32), po.DT_F16) if tag == "f16" else (base32, po.DT_F32)
    queries = nvdb_amd.synth_rows_f32(SEED + 31, 0, Q, d)
    cand = rs.randint(0, n, size=(Q, R)).astype(np.uint32)
    cand[rs.rand(Q, R) < 0.01] = 0xFFFFFFFF
    cand[0, 1] = n + 5                                      # out of range -> skipped
    cand[1, :] = 0xFFFFFFFF                                 # a sampled query with no valid candidate at all
    cand[2, 5:] = 0xFFFFFFFF
    return base, dt, queries, cand


def _assert_split(t, dbg_q):
    assert t.dbg_q == dbg_q
    avgs = (t.dbg_dist_cycles_avg, t.dbg_write_cycles_avg, t.dbg_merge_cycles_avg)
    pcts = (t.dbg_dist_pct, t.dbg_write_pct, t.dbg_merge_pct)
    assert all(a > 0 for a in avgs), avgs
    assert all(0.0 <= p <= 1.0 for p in pcts), pcts
    assert abs(sum(pcts) - 1.0) < 1e-12, pcts
    tot = sum(avgs)
    assert all(abs(p - a / tot) < 1e-12 for a, p in zip(avgs, pcts))


# (tag, d, R, K, refine_v2): together they launch all ten STAMP builds
SHAPES = [("f16", 768, 1024, 10, 2), ("f16", 768, 1024, 10, 1), ("f16", 768, 1024, 10, 0), ("f16", 512, 300, 10, 2),
          ("f16", 384, 500, 10, 2), ("f16", 256, 200, 10, 2), ("f16", 100, 77, 5, 2), ("f16", 1536, 1024, 10, 2),
          ("f16", 1024, 333, 64, 2), ("f32", 768, 300, 64, 2), ("f32", 768, 300, 64, 0), ("f32", 37, 40, 3, 2)]


@pytest.mark.parametrize("tag,d,R,K,v2", SHAPES)
def test_stamped_twin_matches_the_product_kernel_and_reports_the_split(ctx, oracle, tag, d, R, K, v2):
    base, dt, queries, cand = _case(oracle, tag, d, R)
    ctx.upload_corpus(base, dt)
    ctx.set_option("refine_v2", v2)
    try:
        ctx.set_option("refine_dbg_q", 0)
        ids0, dist0, t0 = ctx.refine_l2_topk(queries, cand, K, want_timing=True)
        assert all(getattr(t0, f) == 0 for f in DBG_FIELDS), [getattr(t0, f) for f in DBG_FIELDS]
        ctx.set_option("refine_dbg_q", 8)
        ids, dist, t = ctx.refine_l2_topk(queries, cand, K, want_timing=True)
    finally:
        ctx.set_option("refine_dbg_q", 0)
        ctx.set_option("refine_v2", 2)
    oid, odist = oracle.refine(base, dt, queries, cand, K, mode=0)
    assert np.array_equal(ids, ids0) and np.array_equal(dist.view(np.uint32), dist0.view(np.uint32))
    assert np.array_equal(ids, oid) and np.array_equal(dist.view(np.uint32), odist.view(np.uint32))
    assert (ids[1] == 0xFFFFFFFF).all()
    _assert_split(t, min(8, queries.shape[0]))
    assert t.K == K and t.R == R and t.kernel_ms > 0 and abs(t.total_ms - (t.h2d_ms + t.kernel_ms + t.d2h_ms)) < 1e-3


def test_option_edge_cases(ctx, oracle):
    base, dt, queries, cand = _case(oracle, "f16", 768, 256, Q=5)
    ctx.upload_corpus(base, dt)
    ref_ids, ref_dist = ctx.refine_l2_topk(queries, cand, 10)
    with pytest.raises(nvdb_amd.NvdbError):
        ctx.set_option("refine_dbg_q", -1)
    try:
        ctx.set_option("refine_dbg_q", 100)                              # more than Q: every query is sampled
        ids, dist, t = ctx.refine_l2_topk(queries, cand, 10, want_timing=True)
        _assert_split(t, 5)
        assert np.array_equal(ids, ref_ids) and np.array_equal(dist.view(np.uint32), ref_dist.view(np.uint32))
        ids, dist = ctx.refine_l2_topk(queries, cand, 10)                # no timing struct: the product kernel, same results
        assert np.array_equal(ids, ref_ids) and np.array_equal(dist.view(np.uint32), ref_dist.view(np.uint32))
        _, _, t = ctx.refine_l2_topk(queries, cand, 0, want_timing=True)  # K == 0: nothing to do, zeroed timing
        assert all(getattr(t, f) == 0 for f in DBG_FIELDS) and t.kernel_ms == 0
    finally:
        ctx.set_option("refine_dbg_q", 0)


# ----------------------------------------------------------------------------- CLI: nvdb_cuda_refine_eval
@pytest.fixture(scope="module")
def vecbins(tmp_path_factory):
    d = tmp_path_factory.mktemp("dbg_vecbin")
    base32, queries = make_case_inputs("main768")
    p = dict(b32=str(d / "b32.vecbin"), q=str(d / "q.raw12"), b16=str(d / "b16.vecbin"))
    po.write_vecbin(p["b32"], base32, po.DT_F32)
    po.write_raw12(p["q"], queries)
    subprocess.run([os.path.join(BIN, "nvdb_convert_f16"), p["b32"], p["b16"]], check=True, capture_output=True)
    return p


def _eval(vecbins, dtkey, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("CUDA_DBG_", "CUDA_PINNED", "CUDA_RETURN_DIST", "CUDA_SHMEM_OPTIN", "GIT_SHA"))}
    e.update(REFINE_K="256", **env)
    return subprocess.run([os.path.join(BIN, "nvdb_cuda_refine_eval"), vecbins[dtkey], vecbins["q"], "10"], check=True,
                          capture_output=True, text=True, env=e).stdout


@pytest.mark.parametrize("dtkey,threads", [("b16", 192), ("b32", 256)])
def test_cli_writes_the_reference_dbg_tsv(vecbins, tmp_path, dtkey, threads):
    outdir = tmp_path / "dbg"
    out = _eval(vecbins, dtkey, dict(CUDA_DBG_TIMING="1", CUDA_DBG_Q="4", CUDA_DBG_DIR=str(outdir)))
    files = sorted(os.listdir(outdir))
    name = f"dbg_K10_Q8_R256_th{threads}_mode=wave64_optin=0_pinned=0_ret=1_git=NA.tsv"
    assert files == [name], files
    lines = (outdir / name).read_text().splitlines()
    assert len(lines) == 2 and lines[0].split("\t") == TSV_COLUMNS
    row = dict(zip(TSV_COLUMNS, lines[1].split("\t")))
    assert row["k"] == "10" and row["Q"] == "8" and row["R"] == "256" and row["nprobe"] == "0" and row["refine_k"] == "256"
    assert row["kernel_mode"] == "wave64" and row["cuda_threads"] == str(threads) and row["git_rev"] == "NA" and row["dbg_q"] == "4"
    assert all(len(row[c].split(".")[1]) == 3 and float(row[c]) > 0 for c in TSV_COLUMNS[14:17])
    assert all(len(row[c].split(".")[1]) == 6 for c in TSV_COLUMNS[17:])
    assert abs(sum(float(row[c]) for c in TSV_COLUMNS[17:]) - 1.0) < 3e-6
    out_lines = out.strip().splitlines()
    dbg = [l for l in out_lines if l.startswith("DBG_TSV=")]
    assert len(dbg) == 1 and dbg[0].split()[0] == f"DBG_TSV={outdir / name}" and " dbg_q=4 dist%=" in dbg[0]
    assert any(l.startswith("dbg_q=4 dbg_merge_pct=") and " dbg_write_pct=" in l and " dbg_dist_pct=" in l for l in out_lines)
    assert out_lines.index(dbg[0]) < len(out_lines) - 1
    assert out_lines[-1].startswith("RESULT ") and " recall_vs_cpu=1.000000" in out_lines[-1]


def test_cli_dbg_q_defaults_to_32_clamped_to_q(vecbins, tmp_path):
    outdir = tmp_path / "dbg"
    out = _eval(vecbins, "b16", dict(CUDA_DBG_TIMING="1", CUDA_DBG_DIR=str(outdir)))
    (f,) = os.listdir(outdir)
    row = dict(zip(TSV_COLUMNS, (outdir / f).read_text().splitlines()[1].split("\t")))
    assert row["dbg_q"] == "8" and " dbg_q=8 " in out


def test_cli_without_the_switch_writes_nothing(vecbins, tmp_path):
    outdir = tmp_path / "dbg"
    out = _eval(vecbins, "b16", dict(CUDA_DBG_DIR=str(outdir)))
    assert not outdir.exists() and "DBG_TSV" not in out and "dbg_q=" not in out
    assert out.strip().splitlines()[-1].startswith("RESULT ")
