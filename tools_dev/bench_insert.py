"""In-place insertion: what it costs and what the only other route costs, in one process.

    python tools_dev/bench_insert.py [rows] [dim] [samples] [baseline] [nparts]      (defaults: 10000000 768 5 1 4096)

1. Insertion time: fp16 with the q8 filter shadow resident, and int8; 1 row, 1 % and 10 % of the rows, appended behind the last row
   (no table) or put into a table of `nparts` equal partitions -- the single row into PARTITION 0 (the worst case: every other row
   shifts by one, the whole corpus moves and every slab bounces), the 1 % and 10 % spread uniformly at random; in place
   (nvdb_hip_reserve_rows first) and on the growth path (option insert_growth_pct = 0).  Median wall ms of `samples` nvdb_hip_insert_rows calls after one warm-up, each on a freshly generated
   corpus.  Beside it the traffic model -- every old row that moves is read and written once on a direct slab or on the growth
   path, twice on a bounced slab, every new row once from its staging -- as achieved TB/s and as the time the 6.3 TB/s copy roof of
   the compaction profile would take.  The new rows' host-to-device staging is part of the call and of the time, not of the model.
2. baseline = 1: the only route there was before, once each: download_rows + host concatenate + upload_corpus (fp16, 1 % appended),
   and nvdb_hip_ivf_build of the whole beside nvdb_hip_ivf_add_rows of 1 % (1024 lists).
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
SLAB = 65536


def new_rows(m, dim, dtype):
    """m host rows: a block of synthetic rows, repeated."""
    block, sc = nvdb_amd.synth_corpus(SEED + 7, 0, min(m, 4096), dim, dtype)
    reps = (m + len(block) - 1) // len(block)
    return np.ascontiguousarray(np.tile(block, (reps, 1))[:m]), (np.ascontiguousarray(np.tile(sc, reps)[:m]) if sc is not None else None)


def traffic(n, offsets, part_of, m, bytes_per_row, grow):
    """(bytes read + written by the move, share of the moved rows that went through the bounce buffer): insert_plan.h's cut."""
    nparts = len(offsets) - 1
    cnt = np.bincount(part_of, minlength=nparts) if part_of is not None else np.concatenate([np.zeros(nparts - 1, np.int64), [m]])
    shift = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    first = int(np.argmax(cnt > 0))
    lo = int(offsets[first + 1])
    if grow:
        return (2 * n + 2 * m) * bytes_per_row, 0.0
    direct = bounced = 0
    s1 = n
    while s1 > lo:
        s0 = max(lo, s1 - SLAB)
        p = int(np.searchsorted(offsets, s0, side="right")) - 1
        if s0 + int(shift[min(p, nparts - 1)]) >= s1:
            direct += s1 - s0
        else:
            bounced += s1 - s0
        s1 = s0
    return (2 * direct + 4 * bounced + 2 * m) * bytes_per_row, bounced / max(direct + bounced, 1)


def make_ctx(rows, dim, dtype, offsets=None, growth=None):
    ctx = nvdb_amd.HipContext(0)
    if dtype == nvdb_amd.DT_F16:
        ctx.set_option("q8_shadow", 1)
    if growth is not None:
        ctx.set_option("insert_growth_pct", growth)
    ctx.generate_corpus(SEED, rows, dim, dtype)
    if offsets is not None:
        ctx.set_partitions(offsets)
    return ctx


def time_insert(rows, dim, dtype, add, add_sc, part_of, offsets, reserve, samples):
    t = []
    m = len(add)
    for i in range(samples + 1):
        ctx = make_ctx(rows, dim, dtype, offsets, None if reserve else 0)
        if reserve:
            ctx.reserve_rows(rows + m)
        n_new = C.c_uint64(0)
        t0 = time.perf_counter()
        st = ctx.lib.nvdb_hip_insert_rows(ctx.h, add.ctypes.data, add_sc.ctypes.data if add_sc is not None else None, m,
                                          part_of.ctypes.data if part_of is not None else None, None, C.byref(n_new))
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0 and n_new.value == rows + m, ctx.lib.nvdb_hip_last_error(ctx.h)
        ctx.close()
        if i:
            t.append(dt)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    a = sys.argv[1:]
    rows = int(a[0]) if len(a) > 0 else 10_000_000
    dim = int(a[1]) if len(a) > 1 else 768
    samples = int(a[2]) if len(a) > 2 else 5
    baseline = int(a[3]) if len(a) > 3 else 1
    nparts = int(a[4]) if len(a) > 4 else 4096
    out = dict(rows=rows, dim=dim, samples=samples, nparts=nparts)
    offsets = (np.arange(nparts + 1, dtype=np.uint64) * rows) // nparts
    rs = np.random.RandomState(11)
    # bytes per row over every array that moves: fp16 rows + the q8 shadow and its scales; int8 rows + scales
    per_row = {"f16": dim * 2 + dim + 4, "i8": dim + 4}
    for dname, dtype in (("f16", nvdb_amd.DT_F16), ("i8", nvdb_amd.DT_I8)):
        for label, m in (("1 row", 1), ("1 %", rows // 100), ("10 %", rows // 10)):
            add, add_sc = new_rows(m, dim, dtype)
            spread = rs.randint(0, nparts, size=m).astype(np.uint32) if m > 1 else np.zeros(1, dtype=np.uint32)
            tabled = ("spread over %d partitions" if m > 1 else "into partition 0 of %d") % nparts
            for place, part_of, off in (("appended", None, None), (tabled, spread, offsets)):
                for route, reserve in (("in place", True), ("growth", False)):
                    med, lo, hi = time_insert(rows, dim, dtype, add, add_sc, part_of, off, reserve, samples)
                    model_off = off if off is not None else np.array([0, rows], dtype=np.uint64)
                    byt, share = traffic(rows, model_off.astype(np.int64), part_of, m, per_row[dname], not reserve)
                    out["insert/%s/%s/%s/%s" % (dname, label, place, route)] = dict(median_ms=med, min_ms=lo, max_ms=hi, m=m, model_bytes=byt, bounced_share=share,
                                                                                    achieved_tbps=byt / med / 1e9, roof_ms=byt / 6.3e9)
                    print(f"insert {dname} {label:5s} {place:28s} {route:8s}: median {med:8.2f} ms (min {lo:.2f}, max {hi:.2f})  traffic {byt / 1e9:6.2f} GB "
                          f"({share * 100:5.1f} % of the moved rows bounced)  {byt / med / 1e9:5.2f} TB/s  copy roof {byt / 6.3e9:6.2f} ms", flush=True)

    if baseline:
        m = rows // 100
        add, _ = new_rows(m, dim, nvdb_amd.DT_F16)
        ctx = make_ctx(rows, dim, nvdb_amd.DT_F16)
        t0 = time.perf_counter()
        base, _ = ctx.download_rows(0, rows)
        t1 = time.perf_counter()
        both = np.concatenate([base, add])
        t2 = time.perf_counter()
        ctx.upload_corpus(both, nvdb_amd.DT_F16)
        t3 = time.perf_counter()
        out["baseline/download_concatenate_upload"] = dict(download_ms=(t1 - t0) * 1e3, host_concatenate_ms=(t2 - t1) * 1e3, upload_ms=(t3 - t2) * 1e3, total_ms=(t3 - t0) * 1e3)
        print(f"baseline f16 1 % appended: download_rows {1e3 * (t1 - t0):.0f} ms + host concatenate {1e3 * (t2 - t1):.0f} ms + upload_corpus {1e3 * (t3 - t2):.0f} ms = "
              f"{1e3 * (t3 - t0):.0f} ms", flush=True)
        del base, both
        ctx.close()
        cen = np.random.RandomState(5).standard_normal((1024, dim)).astype(np.float32)
        cen /= np.linalg.norm(cen, axis=1, keepdims=True)
        src = make_ctx(rows, dim, nvdb_amd.DT_F16)
        t0 = time.perf_counter()
        ivf = nvdb_amd.IvfIndex(src, cen)
        build_ms = (time.perf_counter() - t0) * 1e3
        src.close()
        t0 = time.perf_counter()
        ivf.add_rows(add)
        add_ms = (time.perf_counter() - t0) * 1e3
        out["baseline/ivf"] = dict(ivf_build_ms=build_ms, ivf_add_rows_ms=add_ms, m=m)
        print(f"index, 1024 lists: nvdb_hip_ivf_build of the whole {build_ms:.0f} ms; nvdb_hip_ivf_add_rows of 1 % ({m} rows, growth path, with the assignment and the "
              f"host's perm rewrite) {add_ms:.1f} ms", flush=True)
        ivf.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
