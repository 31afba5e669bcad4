"""Masked searches against their unmasked twins on the same context in the same process.

    python tools_dev/bench_masked.py [rows] [dim] [dtype] [nparts] [batch] [nprobe] [k] [calls] [warmup] [flat_only]
                                     (defaults: 10000000 768 f16 4096 1024 8 10 20 3 0)

Equal partitions, random probes.  Reports the median wall ms per call of search_partitions (unmasked) beside
search_partitions_masked under an all-live mask, a random 50 % and 1 % mask and a contiguous 10 % mask (skipped with flat_only = 1);
then search_masked (the masked flat search) at batch 1 / 8 / 32 / 128 / 1024 under the all-live, the 50 % and the 1 % mask beside
search_batch at the same batches, with the route it took (stats path: 2 = MFMA filter route, 4 = partition scan); and one JSON line
with all of it."""
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
    k = int(a[6]) if len(a) > 6 else 10
    calls = int(a[7]) if len(a) > 7 else 20
    warmup = int(a[8]) if len(a) > 8 else 3
    flat_only = int(a[9]) if len(a) > 9 else 0
    seed = 20240613
    ctx = nvdb_amd.HipContext(0)
    ctx.generate_corpus(seed, rows, dim, dtype)
    ctx.set_partitions((np.arange(nparts + 1, dtype=np.uint64) * rows) // nparts)
    q = np.ascontiguousarray(nvdb_amd.synth_rows_f32(seed + 1, 0, batch, dim))
    rs = np.random.RandomState(11)
    probe = rs.randint(0, nparts, size=(batch, nprobe)).astype(np.uint32)
    names = ["all live", "random 50 %", "random 1 %", "contiguous 10 %"]
    planes = np.zeros((4, rows), dtype=bool)
    planes[0] = True
    planes[1] = rs.rand(rows) < 0.5
    planes[2] = rs.rand(rows) < 0.01
    planes[3, rows // 3:rows // 3 + rows // 10] = True
    ctx.set_row_masks(planes)
    out = dict(rows=rows, dim=dim, dtype=dname, nparts=nparts, batch=batch, nprobe=nprobe, k=k, calls=calls, warmup=warmup)

    if not flat_only:
        uid, usc, ucnt = ctx.search_partitions(q, k, probe)
        med, lo, hi = median_ms(lambda: ctx.search_partitions(q, k, probe), calls, warmup)
        st = ctx.stats()
        base = med
        out["search_partitions"] = dict(median_ms=med, min_ms=lo, max_ms=hi, rows_scanned=st["rows_scanned"], launches=st["chunks"])
        print(f"search_partitions                       : median {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})  rows read {st['rows_scanned']} launches {st['chunks']}")
        for m, name in enumerate(names):
            mo = np.full(batch, m, dtype=np.uint32)
            ids, sc, cnt = ctx.search_partitions_masked(q, k, probe, mo)
            same = bool(np.array_equal(ids, uid) and np.array_equal(sc.view(np.uint32), usc.view(np.uint32)) and np.array_equal(cnt, ucnt)) if m == 0 else None
            med, lo, hi = median_ms(lambda: ctx.search_partitions_masked(q, k, probe, mo), calls, warmup)
            out[f"search_partitions_masked/{name}"] = dict(median_ms=med, min_ms=lo, max_ms=hi, vs_unmasked=med / base, mean_count=float(cnt.mean()), equals_unmasked=same)
            print(f"search_partitions_masked {name:15s}: median {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})  x{med / base:.3f} of unmasked  mean count {cnt.mean():.2f}"
                  + (f"  equals the unmasked result: {same}" if m == 0 else ""))
    for b in (1, 8, 32, 128, 1024):
        if b > batch:
            continue
        qb = np.ascontiguousarray(q[:b])
        medf, lof, hif = median_ms(lambda: ctx.search_batch(qb, k), calls, warmup)
        pathf = ctx.stats()["path"]
        row = dict(search_batch_median_ms=medf, search_batch_min_ms=lof, search_batch_max_ms=hif, search_batch_path=pathf)
        line = f"batch {b:4d}: search_batch median {medf:8.3f} ms (path {pathf})  search_masked"
        for m, name in enumerate(names[:3]):
            mo = np.full(b, m, dtype=np.uint32)
            medm, lom, him = median_ms(lambda: ctx.search_masked(qb, k, mo), calls, warmup)
            st = ctx.stats()
            row[name] = dict(median_ms=medm, min_ms=lom, max_ms=him, path=st["path"], rows_scanned=st["rows_scanned"], launches=st["chunks"],
                             overflow_queries=st["overflow_queries"], vs_search_batch=medm / medf)
            line += f" | {name}: {medm:8.3f} ms (min {lom:.3f}, max {him:.3f}; path {st['path']}, rows read {st['rows_scanned']}, flagged {st['overflow_queries']})"
        out[f"flat/batch{b}"] = row
        print(line, flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
