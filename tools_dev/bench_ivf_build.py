#!/usr/bin/env python3
"""IVF-Flat build from a resident corpus: train the centroids, build the index, one probe search.
usage: bench_ivf_build.py [rows] [dim] [dtype] [nlist] [iters] [max_train_rows]
Default: N = 1M, d = 768, fp16 (generated on device), nlist = 1024, 4 k-means iterations over 131072 training rows.
NVDB_IVF_DEBUG is set, so the library reports the hipEvent split on stderr ("[nvdb ivf] train: ..." / "[nvdb ivf] build: ...":
assignment, member sums + normalisation, gather with its rate); this script adds one JSON line with the wall clock of the two
calls, the list-size spread and a search through the index.  Developer tool; GPU box."""
import json, os, sys, time
os.environ.setdefault("NVDB_IVF_DEBUG", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nano-vectordb_amd"))
import numpy as np, nvdb_amd
DT = {"f16": nvdb_amd.DT_F16, "f32": nvdb_amd.DT_F32, "i8": nvdb_amd.DT_I8}
arg = lambda i, d: type(d)(sys.argv[i]) if len(sys.argv) > i else d
n, dim, tag, nlist, iters, mtr = arg(1, 1_000_000), arg(2, 768), arg(3, "f16"), arg(4, 1024), arg(5, 4), arg(6, 131072)

ctx = nvdb_amd.HipContext(0)
ctx.generate_corpus(20240613, n, dim, DT[tag])
t0 = time.perf_counter()
cen = ctx.train_centroids(nlist, iters, seed=1, max_train_rows=mtr)
t1 = time.perf_counter()
ivf = nvdb_amd.IvfIndex(ctx, cen)
t2 = time.perf_counter()
sizes = np.diff(ivf.info()["offsets"].astype(np.int64))
q = nvdb_amd.synth_rows_f32(20240614, 0, 256, dim)
ids, sc, counts = ivf.search(q, 10, 8)
t3 = time.perf_counter()
ids, sc, counts = ivf.search(q, 10, 8)
t4 = time.perf_counter()
print(json.dumps(dict(what="ivf_build", rows=n, dim=dim, dtype=tag, nlist=nlist, iters=iters, train_rows=min(mtr, n) if mtr else n,
                      train_wall_ms=round((t1 - t0) * 1e3, 1), build_wall_ms=round((t2 - t1) * 1e3, 1),
                      list_rows_min=int(sizes.min()), list_rows_median=int(np.median(sizes)), list_rows_max=int(sizes.max()),
                      search_256q_nprobe8_wall_ms=round((t4 - t3) * 1e3, 2), results_full=bool((counts == 10).all()))), flush=True)
ivf.close()
ctx.close()
