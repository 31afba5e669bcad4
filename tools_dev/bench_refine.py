#!/usr/bin/env python3
"""BASELINE config 5: exact-L2 refine, N=2.9M fp16 d=768, Q=10000, R=1024, K=10 (synthetic candidates).

REFINE_DBG_Q=n: for every refine build it runs, also time the STAMP build of the same template (option refine_dbg_q = n, the reference's
CUDA_DBG_TIMING / CUDA_DBG_Q) interleaved with the product kernel, and print the phase split (average shader-clock cycles and
shares of dist / write / merge over the first n queries) beside kernel_ms with the stamps off and on."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nano-vectordb_amd")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np, nvdb_amd, pyoracle as po
N, D, Q, R, K = int(os.environ.get("REFINE_N", 2_900_000)), int(os.environ.get("REFINE_D", 768)), int(os.environ.get("REFINE_Q", 10_000)), int(os.environ.get("REFINE_K", 1024)), 10
ctx = nvdb_amd.HipContext(0)
DT = nvdb_amd.DT_F32 if os.environ.get("REFINE_DT") == "f32" else nvdb_amd.DT_F16
BPE = 4 if DT == nvdb_amd.DT_F32 else 2
ctx.generate_corpus(20240613, N, D, DT)
queries = nvdb_amd.synth_rows_f32(20240614, 0, Q, D)
rs = np.random.RandomState(1)
cand = rs.randint(0, N, size=(Q, R)).astype(np.uint32)
cand[rs.rand(Q, R) < 0.01] = 0xFFFFFFFF
DBG_Q = int(os.environ.get("REFINE_DBG_Q", 0))
per_kernel, split = {}, {}
for v2 in [int(x) for x in os.environ.get("REFINE_V2", "2,1").split(",")]:
    ctx.set_option("refine_v2", v2)
    best = best_on = None
    for it in range(4):
        ids, dist, t = ctx.refine_l2_topk(queries, cand, K, want_timing=True)
        if best is None or t.kernel_ms < best.kernel_ms: best = t
        if DBG_Q:                                      # STAMP build, interleaved with the product kernel
            ctx.set_option("refine_dbg_q", DBG_Q)
            _, _, t = ctx.refine_l2_topk(queries, cand, K, want_timing=True)
            ctx.set_option("refine_dbg_q", 0)
            if best_on is None or t.kernel_ms < best_on.kernel_ms: best_on = t
    per_kernel[f"refine_v2={v2}"] = best.kernel_ms
    if DBG_Q:
        s = {"dbg_q": best_on.dbg_q, "kernel_ms_stamps_off": best.kernel_ms, "kernel_ms_stamps_on": best_on.kernel_ms,
             **{f"{p}_cycles_avg": getattr(best_on, f"dbg_{p}_cycles_avg") for p in ("dist", "write", "merge")},
             **{f"{p}_frac": getattr(best_on, f"dbg_{p}_pct") for p in ("dist", "write", "merge")}}
        split[f"refine_v2={v2}"] = s
        print(f"refine_v2={v2} threads={best_on.threads} dbg_q={s['dbg_q']} cycles dist/write/merge = {s['dist_cycles_avg']:.0f} / "
              f"{s['write_cycles_avg']:.0f} / {s['merge_cycles_avg']:.0f}  shares = {100 * s['dist_frac']:.2f} % / {100 * s['write_frac']:.2f} % / "
              f"{100 * s['merge_frac']:.2f} %  kernel_ms stamps off {s['kernel_ms_stamps_off']:.3f} on {s['kernel_ms_stamps_on']:.3f}", flush=True)
ctx.set_option("refine_v2", int(os.environ.get("REFINE_V2", "2,1").split(",")[0]))
ids, dist, best = ctx.refine_l2_topk(queries, cand, K, want_timing=True)
# parity on a slice against the oracle's restated kernel order (bit-exact) and CPU double order
sub = slice(0, 64)
rows = {}
orc = po.Oracle()
uniq = np.unique(cand[sub][cand[sub] != 0xFFFFFFFF])
remap = {int(u): i for i, u in enumerate(uniq)}
base_sub = np.concatenate([ctx.download_rows(int(u), 1)[0] for u in uniq])
c2 = np.array([[remap.get(int(v), 0xFFFFFFFF) if v != 0xFFFFFFFF else 0xFFFFFFFF for v in row] for row in cand[sub]], dtype=np.uint32)
oid, od = orc.refine(base_sub, po.DT_F32 if BPE == 4 else po.DT_F16, queries[sub], c2, K, mode=0)
ok = np.array_equal(uniq[oid], ids[sub]) and np.array_equal(od.view(np.uint32), dist[sub].view(np.uint32))
gb = Q * R * 0.99 * D * BPE / 1e9
print(json.dumps({"config": f"refine N={N} d={D} Q={Q} R={R} K={K} {'f32' if BPE == 4 else 'f16'}", "kernel_ms": best.kernel_ms, "h2d_ms": best.h2d_ms, "d2h_ms": best.d2h_ms,
                  "us_per_query_kernel": best.kernel_ms * 1e3 / Q, "gather_GBps": gb / (best.kernel_ms * 1e-3), "hbm_frac": gb / (best.kernel_ms * 1e-3) / 8000.0,
                  "parity_vs_oracle_slice": bool(ok), "kernel_ms_by_variant": per_kernel, **({"phase_split_by_variant": split} if DBG_Q else {})}))
