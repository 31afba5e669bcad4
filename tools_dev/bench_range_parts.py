"""Range search on the probe path beside the calls it is built from, on the same context in the same process.

    python tools_dev/bench_range_parts.py [rows] [dim] [dtype] [nparts] [batch] [nprobe] [calls] [warmup]
                                          (defaults: 10000000 768 f16 4096 1024 8 20 3)

Equal partitions, random probes.  Each query's radius is its own 10th best score of the probed union (from search_partitions) and
its 1000th best (from a range call with radius -inf).  Reports the median wall ms per call of search_partitions k = 10,
range_search_partitions at both radii (with and without the results' copy), range_search (flat, unmasked) at the same radii (which
far more rows of the whole corpus reach: it may exceed range_max_mb, and says so), then range_search_masked under an all-live and a
random 50 % plane beside range_search at each query's 10th best score of the whole corpus; and one JSON line with all of it."""
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
    dname = a[2] if len(a) > 2 else "f16"
    dtype = {"f16": nvdb_amd.DT_F16, "i8": nvdb_amd.DT_I8, "f32": nvdb_amd.DT_F32}[dname]
    nparts = int(a[3]) if len(a) > 3 else 4096
    batch = int(a[4]) if len(a) > 4 else 1024
    nprobe = int(a[5]) if len(a) > 5 else 8
    calls = int(a[6]) if len(a) > 6 else 20
    warmup = int(a[7]) if len(a) > 7 else 3
    seed = 20240613
    ctx = nvdb_amd.HipContext(0)
    ctx.generate_corpus(seed, rows, dim, dtype)
    ctx.set_partitions((np.arange(nparts + 1, dtype=np.uint64) * rows) // nparts)
    q = np.ascontiguousarray(nvdb_amd.synth_rows_f32(seed + 1, 0, batch, dim))
    rs = np.random.RandomState(11)
    probe = rs.randint(0, nparts, size=(batch, nprobe)).astype(np.uint32)
    out = dict(rows=rows, dim=dim, dtype=dname, nparts=nparts, batch=batch, nprobe=nprobe, calls=calls, warmup=warmup)
    lims = np.zeros(batch + 1, dtype=np.uint64)

    def report(name, fn, **extra):
        med, lo, hi = median_ms(fn, calls, warmup)
        st = ctx.stats()
        out[name] = dict(median_ms=med, min_ms=lo, max_ms=hi, path=st["path"], rows_scanned=st["rows_scanned"], launches=st["chunks"],
                         candidates=st["candidates"], overflow_queries=st["overflow_queries"], **extra)
        print(f"{name:52s}: median {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})  path {st['path']} rows read {st['rows_scanned']} launches {st['chunks']} "
              f"candidates {st['candidates']} fallbacks {st['overflow_queries']}" + "".join(f"  {k} {v}" for k, v in extra.items()))
        return med

    _, sc10, _ = ctx.search_partitions(q, 10, probe)
    r10 = np.ascontiguousarray(sc10[:, 9])
    p10 = r10
    al, _, asc = ctx.range_search_partitions(q, -np.inf, probe)
    r1000 = np.array([asc[int(al[i]):int(al[i + 1])][min(999, int(al[i + 1] - al[i]) - 1)] for i in range(batch)], dtype=np.float32)
    del asc
    report("search_partitions k=10", lambda: ctx.search_partitions(q, 10, probe))
    for name, r in (("10th best", r10), ("1000th best", r1000)):
        got = ctx.range_search_partitions(q, r, probe)
        n = int(got[0][-1])
        report(f"range_search_partitions, radius = {name}", lambda: ctx.range_search_partitions(q, r, probe), results=n)
        report(f"range_search_partitions, radius = {name}, lims only",
               lambda: ctx.lib.nvdb_hip_range_search_partitions(ctx.h, q.ctypes.data, batch, r.ctypes.data, probe.ctypes.data, nprobe, None, 0, lims.ctypes.data, None),
               results=n)
        # the flat search at the SAME radii: a bar that 10 rows of a 1/500 sample reach, thousands of rows of the corpus reach
        try:
            n = int(ctx.range_search(q, r)[0][-1])
            report(f"range_search (flat), radius = {name}", lambda: ctx.range_search(q, r), results=n)
        except nvdb_amd.NvdbError as e:
            out[f"range_search (flat), radius = {name}"] = dict(error=str(e), results=int(e.lims[-1]))
            print(f"range_search (flat), radius = {name}: {e}")

    planes = np.zeros((2, rows), dtype=bool)
    planes[0] = True
    planes[1] = rs.rand(rows) < 0.5
    ctx.set_row_masks(planes)
    # masks on the flat search, at each query's 10th best score of the WHOLE corpus (tools_dev/bench_range.py's radius)
    _, fsc = ctx.search_batch(q, 10)
    r10 = np.ascontiguousarray(fsc[:, 9])
    flat = ctx.range_search(q, r10)
    report("range_search (flat), radius = 10th best of the corpus", lambda: ctx.range_search(q, r10), results=int(flat[0][-1]))
    for m, name in enumerate(("all live", "random 50 %")):
        mo = np.full(batch, m, dtype=np.uint32)
        got = ctx.range_search_masked(q, r10, mo)
        same = bool(all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, flat))) if m == 0 else None
        report(f"range_search_masked {name}, radius = 10th best", lambda: ctx.range_search_masked(q, r10, mo), results=int(got[0][-1]), equals_unmasked=same)
        got = ctx.range_search_partitions(q, p10, probe, mo)
        report(f"range_search_partitions masked {name}, radius = 10th best", lambda: ctx.range_search_partitions(q, p10, probe, mo), results=int(got[0][-1]))
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
