"""Range search against the flat search on the same context in the same process.

    python tools_dev/bench_range.py [rows] [dim] [dtype] [batch] [calls] [warmup]      (defaults: 10000000 768 f16 1024 20 3)

Each query's radius is its own 10th-best and 1000th-best score, taken from search_batch, so a range search returns about 10 /
1000 rows per query.  Reports the median wall ms per call of range_search beside search_batch (k = 10 and k = 1000), stats.path,
candidates and fallbacks (queries redone on the exact route), and one JSON line with all of it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nano-vectordb_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import nvdb_amd  # noqa: E402


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    a = sys.argv[1:]
    rows = int(a[0]) if len(a) > 0 else 10_000_000
    dim = int(a[1]) if len(a) > 1 else 768
    dtype = {"f16": nvdb_amd.DT_F16, "i8": nvdb_amd.DT_I8, "f32": nvdb_amd.DT_F32}[a[2] if len(a) > 2 else "f16"]
    batch = int(a[3]) if len(a) > 3 else 1024
    calls = int(a[4]) if len(a) > 4 else 20
    warmup = int(a[5]) if len(a) > 5 else 3
    seed = 20240613
    ctx = nvdb_amd.HipContext(0)
    ctx.generate_corpus(seed, rows, dim, dtype)
    q = np.ascontiguousarray(nvdb_amd.synth_rows_f32(seed + 1, 0, batch, dim))
    out = dict(rows=rows, dim=dim, dtype=a[2] if len(a) > 2 else "f16", batch=batch, calls=calls, warmup=warmup, shadow=ctx.shadow_info())
    ids1000, sc1000 = ctx.search_batch(q, 1000)
    for k in (10, 1000):
        med, lo, hi = median_ms(lambda: ctx.search_batch(q, k), calls, warmup)
        st = ctx.stats()
        out[f"search_batch_k{k}"] = dict(median_ms=med, min_ms=lo, max_ms=hi, path=st["path"], candidates=st["candidates"], chunks=st["chunks"])
        print(f"search_batch k={k:5d}: median {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})  path {st['path']} candidates {st['candidates']} launches {st['chunks']}")
    for k in (10, 1000):
        radius = np.ascontiguousarray(sc1000[:, k - 1])
        lims, ids, sc = ctx.range_search(q, radius)
        n = np.diff(lims.astype(np.int64))
        same = all(np.array_equal(ids[int(lims[i]):int(lims[i]) + k], ids1000[i, :k]) for i in range(batch) if n[i] == k)
        med, lo, hi = median_ms(lambda: ctx.range_search(q, radius), calls, warmup)
        st = ctx.stats()
        # the same without bringing the results to the host: the entry point alone
        lm = np.zeros(batch + 1, dtype=np.uint64)
        med0, lo0, hi0 = median_ms(lambda: ctx.lib.nvdb_hip_range_search(ctx.h, q.ctypes.data, batch, radius.ctypes.data, lm.ctypes.data, None), calls, warmup)
        out[f"range_search_r{k}"] = dict(median_ms=med, min_ms=lo, max_ms=hi, search_only_median_ms=med0, path=st["path"], candidates=st["candidates"],
                                         fallbacks=st["overflow_queries"], launches=st["chunks"], results=int(lims[-1]), results_min=int(n.min()),
                                         results_max=int(n.max()), matches_topk=bool(same))
        print(f"range_search r=k{k:<5d}: median {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f}; without the results' copy {med0:.3f})  path {st['path']} "
              f"candidates {st['candidates']} fallbacks {st['overflow_queries']} launches {st['chunks']} results {int(lims[-1])} "
              f"({int(n.min())}..{int(n.max())} per query) top-k prefix equal: {same}")
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
