"""Probe search for any k beside what a user had to do without it, on the same context in the same process.

    python tools_dev/bench_anyk_parts.py [rows] [dim] [dtype] [nparts] [batch] [nprobe] [calls] [warmup]
                                         (defaults: 10000000 768 f16 4096 1024 8 20 3)

Equal partitions, random probes, host API.  Reports the median wall ms per call of
  search_partitions k = 64                      the floor: the wavefront-resident lists, the longest list they hold
  search_partitions_anyk k = 100, k = 1024      the new call
  range_search_partitions at radius -inf        the route to the same rows before it: the whole probed union sorted and copied back
                                                (with the results' copy, which the caller then truncates, and lims only)
checks that the first k of every range slice ARE the new call's rows, and prints one JSON line with all of it."""
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
    neg_inf = np.full(batch, -np.inf, dtype=np.float32)

    def report(name, fn, **extra):
        med, lo, hi = median_ms(fn, calls, warmup)
        st = ctx.stats()
        out[name] = dict(median_ms=med, min_ms=lo, max_ms=hi, path=st["path"], rows_scanned=st["rows_scanned"], launches=st["chunks"],
                         candidates=st["candidates"], **extra)
        print(f"{name:56s}: median {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})  path {st['path']} rows read {st['rows_scanned']} launches {st['chunks']} "
              f"candidates {st['candidates']}" + "".join(f"  {k} {v}" for k, v in extra.items()))
        return med

    report("search_partitions k=64", lambda: ctx.search_partitions(q, 64, probe))
    rl, rid, rsc = ctx.range_search_partitions(q, -np.inf, probe)
    for k in (100, 1024):
        ids, sc, counts = ctx.search_partitions_anyk(q, k, probe)
        same = True
        for i in range(batch):
            lo, n = int(rl[i]), int(counts[i])
            same = same and n == min(k, int(rl[i + 1]) - lo) and np.array_equal(ids[i, :n], rid[lo:lo + n]) and \
                np.array_equal(sc[i, :n].view(np.uint32), rsc[lo:lo + n].view(np.uint32))
        report(f"search_partitions_anyk k={k}", lambda: ctx.search_partitions_anyk(q, k, probe), equals_range_prefix=bool(same))
    total = int(rl[-1])
    del rid, rsc
    report("range_search_partitions radius=-inf + range_results", lambda: ctx.range_search_partitions(q, -np.inf, probe), results=total)
    report("range_search_partitions radius=-inf, lims only",
           lambda: ctx.lib.nvdb_hip_range_search_partitions(ctx.h, q.ctypes.data, batch, neg_inf.ctypes.data, probe.ctypes.data, nprobe, None, 0,
                                                            lims.ctypes.data, None), results=total)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
