#!/usr/bin/env python3
"""Partitioned probe search against the full flat scan on the same context.
usage: bench_partitions.py [rows] [dim] [dtype] [nparts] [batch] [k] [nprobe,nprobe,...]
Default: N = 10M, d = 768, fp16 (generated on device), 4096 equal partitions, batch 1024, k = 10, nprobe 1, 8, 32 with uniformly
random probes.  Per nprobe one JSON line: ms per call (median of 20 after 3 warm-ups; hipEvent = h2d + kernel + d2h of the
call's timing struct, kernel alone, and wall clock), bytes actually read (sum of the work items' segment bytes), that figure
over the kernel time as a fraction of 8 TB/s, and the ratio to search_batch of the same queries.  Developer tool; GPU box."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nano-vectordb_amd"))
import numpy as np, nvdb_amd
DT = {"f16": nvdb_amd.DT_F16, "f32": nvdb_amd.DT_F32, "i8": nvdb_amd.DT_I8}
BPE = {"f16": 2, "f32": 4, "i8": 1}
arg = lambda i, d: type(d)(sys.argv[i]) if len(sys.argv) > i else d
n, dim, tag, nparts, B, k = arg(1, 10_000_000), arg(2, 768), arg(3, "f16"), arg(4, 4096), arg(5, 1024), arg(6, 10)
nprobes = [int(x) for x in arg(7, "1,8,32").split(",")]
REPS, WARM = 20, 3

ctx = nvdb_amd.HipContext(0)
ctx.generate_corpus(20240613, n, dim, DT[tag])
ctx.set_partitions((np.arange(nparts + 1, dtype=np.uint64) * n) // nparts)
q = nvdb_amd.synth_rows_f32(20240614, 0, B, dim)


def median_ms(fn, reps, warm):
    ev, ker, wall = [], [], []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        t = fn()
        w = (time.perf_counter() - t0) * 1e3
        if i >= warm:
            ev.append(t.total_ms); ker.append(t.kernel_ms); wall.append(w)
    return float(np.median(ev)), float(np.median(ker)), float(np.median(wall))


flat_ev, flat_ker, flat_wall = median_ms(lambda: ctx.search_batch(q, k, want_timing=True)[2], 5, 2)
print(json.dumps(dict(what="search_batch", rows=n, dim=dim, dtype=tag, batch=B, k=k, path=ctx.stats()["path"], event_ms=round(flat_ev, 3),
                      kernel_ms=round(flat_ker, 3), wall_ms=round(flat_wall, 3))), flush=True)
rs = np.random.RandomState(7)
for nprobe in nprobes:
    probe = rs.randint(0, nparts, size=(B, nprobe)).astype(np.uint32)
    ev, ker, wall = median_ms(lambda: ctx.search_partitions(q, k, probe, want_timing=True)[3], REPS, WARM)
    st = ctx.stats()
    nbytes = st["rows_scanned"] * dim * BPE[tag]
    print(json.dumps(dict(what="search_partitions", nprobe=nprobe, nparts=nparts, batch=B, k=k, event_ms=round(ev, 3), kernel_ms=round(ker, 3),
                          wall_ms=round(wall, 3), scan_launches=st["chunks"], bytes_read=int(nbytes), read_TBps=round(nbytes / ker / 1e9, 3),
                          frac_of_8TBps=round(nbytes / ker / 1e9 / 8.0, 3), event_ratio_to_search_batch=round(ev / flat_ev, 3),
                          wall_ratio_to_search_batch=round(wall / flat_wall, 3))), flush=True)
ctx.close()
