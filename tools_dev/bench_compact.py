"""In-place compaction: what it costs, what the only other route costs, and what it buys, in one process.

    python tools_dev/bench_compact.py [rows] [dim] [samples] [slabs] [baseline] [payoff]
                                      (defaults: 10000000 768 5 16384,65536,262144 1 1)

1. Compaction time: fp16 with the q8 filter shadow resident, and int8, each under a random 1 % / 10 % / 50 % dead plane and a
   contiguous 10 % dead block; median wall ms of `samples` nvdb_hip_compact_rows calls after one warm-up, each on a freshly
   generated corpus (out_old_rows = NULL: the map's copy to the host is not part of the move).  Beside it the traffic model: every
   moved byte is read and written once on a direct slab, twice on a bounced one; achieved TB/s = that traffic / the time.
2. The slab sweep: fp16, random 10 % dead, option compact_slab_rows at each of `slabs`.
3. baseline = 1: the route a caller has without the entry point, once each: download_rows + host select + upload_corpus (fp16, random
   10 %), and nvdb_hip_ivf_build from the source beside nvdb_hip_ivf_compact of the same index (1024 lists, random 10 %).
4. payoff = 1, 50 % live: search_batch (batch 1024, k = 10) after compaction beside search_masked before and beside search_batch on
   a fresh corpus of as many rows; search_partitions after beside search_partitions_masked before (4096 partitions, nprobe 8).
One JSON line with all of it at the end."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nano-vectordb_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import nvdb_amd  # noqa: E402

SEED = 20240613


def planes_of(rows):
    rs = np.random.RandomState(11)
    out = {}
    for pct in (1, 10, 50):
        out["random %d %% dead" % pct] = rs.rand(rows) >= pct / 100.0
    p = np.ones(rows, bool)
    p[rows // 3:rows // 3 + rows // 10] = False
    out["contiguous 10 % dead"] = p
    return out


def traffic(live, slab, bytes_per_row):
    """(bytes read + written by the walk, share of the moved rows that went through the bounce buffer): compact_plan.h's cut."""
    n = len(live)
    dead = np.flatnonzero(~live)
    if not len(dead):
        return 0, 0.0
    first = int(dead[0])
    rank = np.concatenate([[0], np.cumsum(live)])
    bounds = [first] + list(range(first // 64 * 64 + slab, n, slab)) + [n]
    direct = bounced = 0
    for s0, s1 in zip(bounds[:-1], bounds[1:]):
        moved = int(rank[s1] - rank[s0])
        if rank[s1] <= s0:
            direct += moved
        else:
            bounced += moved
    return (2 * direct + 4 * bounced) * bytes_per_row, bounced / max(direct + bounced, 1)


def make_ctx(rows, dim, dtype, slab=None):
    ctx = nvdb_amd.HipContext(0)
    if dtype == nvdb_amd.DT_F16:
        ctx.set_option("q8_shadow", 1)
    if slab:
        ctx.set_option("compact_slab_rows", slab)
    ctx.generate_corpus(SEED, rows, dim, dtype)
    return ctx


def time_compaction(rows, dim, dtype, packed, samples, slab=None):
    t = []
    for i in range(samples + 1):
        ctx = make_ctx(rows, dim, dtype, slab)
        ctx.lib.nvdb_hip_set_row_masks(ctx.h, packed.ctypes.data, 1)
        n_new = C.c_uint64(0)
        t0 = time.perf_counter()
        st = ctx.lib.nvdb_hip_compact_rows(ctx.h, 0, C.byref(n_new), None)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0, ctx.lib.nvdb_hip_last_error(ctx.h)
        ctx.close()
        if i:
            t.append(dt)
    return float(np.median(t)), float(np.min(t)), float(np.max(t)), n_new.value


def median_ms(fn, calls=10, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    a = sys.argv[1:]
    rows = int(a[0]) if len(a) > 0 else 10_000_000
    dim = int(a[1]) if len(a) > 1 else 768
    samples = int(a[2]) if len(a) > 2 else 5
    slabs = [int(x) for x in (a[3] if len(a) > 3 else "16384,65536,262144").split(",")]
    baseline = int(a[4]) if len(a) > 4 else 1
    payoff = int(a[5]) if len(a) > 5 else 1
    planes = planes_of(rows)
    packed = {name: nvdb_amd.pack_row_masks(p, rows) for name, p in planes.items()}
    out = dict(rows=rows, dim=dim, samples=samples)
    default_slab = 65536

    # bytes per row over every array that moves: fp16 rows + the q8 shadow and its scales; int8 rows + scales
    per_row = {"f16": dim * 2 + dim + 4, "i8": dim + 4}
    for dname, dtype in (("f16", nvdb_amd.DT_F16), ("i8", nvdb_amd.DT_I8)):
        for name, live in planes.items():
            med, lo, hi, n_new = time_compaction(rows, dim, dtype, packed[name], samples)
            byt, share = traffic(live, default_slab, per_row[dname])
            out["compact/%s/%s" % (dname, name)] = dict(median_ms=med, min_ms=lo, max_ms=hi, n_new=n_new, model_bytes=byt, bounced_share=share,
                                                          achieved_tbps=byt / med / 1e9, roof_ms=byt / 6.3e9)
            print(f"compact {dname} {name:22s}: median {med:8.2f} ms (min {lo:.2f}, max {hi:.2f})  n' {n_new}  traffic {byt / 1e9:6.2f} GB "
                  f"({share * 100:4.1f} % of the moved rows bounced)  {byt / med / 1e9:5.2f} TB/s  copy roof {byt / 6.3e9:6.2f} ms", flush=True)
    name = "random 10 % dead"
    for slab in slabs:
        med, lo, hi, _ = time_compaction(rows, dim, nvdb_amd.DT_F16, packed[name], samples, slab)
        byt, share = traffic(planes[name], slab, per_row["f16"])
        out["slab_sweep/%d" % slab] = dict(median_ms=med, min_ms=lo, max_ms=hi, bounced_share=share, model_bytes=byt)
        print(f"slab sweep f16 {name}: compact_slab_rows {slab:8d}: median {med:8.2f} ms (min {lo:.2f}, max {hi:.2f})  {share * 100:4.1f} % bounced", flush=True)

    if baseline:
        live = planes[name]
        ctx = make_ctx(rows, dim, nvdb_amd.DT_F16)
        t0 = time.perf_counter()
        base, _ = ctx.download_rows(0, rows)
        t1 = time.perf_counter()
        kept = np.ascontiguousarray(base[live])
        t2 = time.perf_counter()
        ctx.upload_corpus(kept, nvdb_amd.DT_F16)
        t3 = time.perf_counter()
        out["baseline/download_select_upload"] = dict(download_ms=(t1 - t0) * 1e3, host_select_ms=(t2 - t1) * 1e3, upload_ms=(t3 - t2) * 1e3, total_ms=(t3 - t0) * 1e3)
        print(f"baseline f16 {name}: download_rows {1e3 * (t1 - t0):.0f} ms + host select {1e3 * (t2 - t1):.0f} ms + upload_corpus {1e3 * (t3 - t2):.0f} ms = {1e3 * (t3 - t0):.0f} ms", flush=True)
        del base, kept
        ctx.close()
        src = make_ctx(rows, dim, nvdb_amd.DT_F16)
        cen = np.random.RandomState(5).standard_normal((1024, dim)).astype(np.float32)
        cen /= np.linalg.norm(cen, axis=1, keepdims=True)
        t0 = time.perf_counter()
        ivf = nvdb_amd.IvfIndex(src, cen)
        build_ms = (time.perf_counter() - t0) * 1e3
        ivf.set_row_masks(live[None])
        t0 = time.perf_counter()
        ivf.compact(0)
        compact_ms = (time.perf_counter() - t0) * 1e3
        out["baseline/ivf"] = dict(ivf_build_ms=build_ms, ivf_compact_ms=compact_ms)
        print(f"index, 1024 lists, {name}: nvdb_hip_ivf_build from the source {build_ms:.0f} ms; nvdb_hip_ivf_compact {compact_ms:.1f} ms (with the host's perm rewrite)", flush=True)
        ivf.close()
        src.close()

    if payoff:
        live = planes["random 50 % dead"]
        nparts, batch, nprobe, k = 4096, 1024, 8, 10
        q = np.ascontiguousarray(nvdb_amd.synth_rows_f32(SEED + 1, 0, batch, dim))
        probe = np.random.RandomState(11).randint(0, nparts, size=(batch, nprobe)).astype(np.uint32)
        ctx = make_ctx(rows, dim, nvdb_amd.DT_F16)
        ctx.set_partitions((np.arange(nparts + 1, dtype=np.uint64) * rows) // nparts)
        ctx.set_row_masks(live[None])
        masked_flat = median_ms(lambda: ctx.search_masked(q, k))
        masked_parts = median_ms(lambda: ctx.search_partitions_masked(q, k, probe))
        unmasked_full = median_ms(lambda: ctx.search_batch(q, k))
        n_new, _ = ctx.compact_rows(0)
        after_flat = median_ms(lambda: ctx.search_batch(q, k))
        after_parts = median_ms(lambda: ctx.search_partitions(q, k, probe))
        ctx.close()
        fresh = make_ctx(n_new, dim, nvdb_amd.DT_F16)
        fresh_flat = median_ms(lambda: fresh.search_batch(q, k))
        fresh.close()
        out["payoff"] = dict(n_new=n_new, search_masked_before_ms=masked_flat, search_batch_all_rows_ms=unmasked_full, search_batch_after_ms=after_flat,
                             search_batch_fresh_same_rows_ms=fresh_flat, search_partitions_masked_before_ms=masked_parts, search_partitions_after_ms=after_parts)
        print(f"payoff, 50 % live (n' = {n_new}), batch {batch}, k = {k}: search_masked before {masked_flat:.2f} ms (search_batch over all rows {unmasked_full:.2f} ms) -> "
              f"search_batch after {after_flat:.2f} ms; a fresh corpus of n' rows {fresh_flat:.2f} ms", flush=True)
        print(f"        {nparts} partitions, nprobe {nprobe}: search_partitions_masked before {masked_parts:.2f} ms -> search_partitions after {after_parts:.2f} ms", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
