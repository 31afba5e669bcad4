"""PQ candidate generation beside the only route to the same candidates without it, on the same index in the same process.

    python tools_dev/bench_pq.py [rows] [dim] [dtype] [nlist] [M] [batch] [calls] [warmup]
                                 (defaults: 10000000 768 f16 4096 48 1024 10 2)

An IVF index over the synthetic corpus (centroids: two k-means rounds over 262144 rows), codebooks from four Lloyd rounds per
sub-quantiser over 20000 sampled rows ON THE DEVICE (pq_train over a context that holds the sample); the numpy trainer stays
beside it on the same sample, start and rounds: median of 5 after a warm-up of both, and the fp64 quantisation error of both
codebook sets on the sample (neither is a tuned quantiser).  For
nprobe in (8, 32) and R in (100, 1024), median wall ms per call, alternating the two routes call by call, of
  ivf_pq_search R                 PQ scan + select                     | ivf_search_anyk k = R     exact scores of the full rows + select
  ivf_pq_refine K = 10            the fused pipeline                   | ivf_search_anyk k = R, then refine_l2_topk on the index's rows
and recall@10 of both refined results against the exact flat top-10 by squared L2 distance over the rows as f32 (the search's
own score is the dot product, so the flat reference is the refine over every row, taken from a flat scan's 1024 best dot
products -- stated with the figure).  Prints the build's wall time and one JSON line with all of it.

    python tools_dev/bench_pq.py [the same arguments] --residual [--clustered]

The non-residual shadow beside the RESIDUAL one.  A context holds one shadow, so the process builds the index twice from the same
rows and centroids -- the same lists, row for row -- and gives each copy one kind: codebooks from pq_train / pq_train(residual=True)
over the same 20000 list-ordered rows and rounds, then, alternating the two copies call by call, median wall ms of ivf_pq_search
and ivf_pq_refine at the shapes above, recall@10 of both, the wall time of both builds (median of 3 after a warm-up: codebook
upload, allocation and the encode kernel) and the fp64 quantisation error of both over 20 blocks of 1000 rows: the mean over rows
and sub-quantisers of |x - pq_reconstruct(x)|^2.  --clustered replaces the synthetic corpus, which has no cluster structure, by
seeded centre + noise rows generated on the host (nlist / 4 centres, noise 0.35 of a centre's element scale, every row scaled
to unit length as the index's spherical k-means expects), labelled as such.

    python tools_dev/bench_pq.py [the same arguments] --opq [--clustered | --decay]

A shadow without a rotation beside one under an OPQ ROTATION, two copies of the same index as above.  The rotation is learnt here,
in numpy, over 20000 rows sampled through the library: four alternations of pq_train(rotation=A) and pq_build(rotation=A) on the
device, yhat from the codes, A <- U V^T of the SVD of sum yhat x^T (learn_rotation).  Reports the wall time of both builds, their
difference against 2 n dim^2 flop at the 157 TFLOP/s of the fp32 matrix cores, the fp64 quantisation error of both, and, alternating
the two copies call by call, ivf_pq_search / ivf_pq_refine times and recall@10.  --decay: unit rows of one Gaussian whose
per-dimension deviation falls as 1 / sqrt(1 + t / 8), t the dimension.

    python tools_dev/bench_pq.py [the same arguments] --bits 4 [--clustered]

The 8-bit shadow at M beside 4-BIT shadows at 2 M (equal bytes per row) and at M (half the bytes), two copies of the same index as
above: copy a keeps the 8-bit shadow, copy b takes the two 4-bit ones in turn.  All codebooks are trained on the device over the same
262144 list-ordered rows (pq_train with bits=8 or bits=4, four rounds).  Reports seconds per Lloyd iteration of each training, the
wall time of the builds, the fp64 quantisation error, and, alternating the two copies call by call, ivf_pq_search / ivf_pq_refine
times and recall@10.

    python tools_dev/bench_pq.py [the same arguments] --l2 [--clustered] [--scaled]

The SAME shadow under both metrics (pq_set_metric), one index, alternating "dot" and "l2" call by call in one process: 8-bit at M,
4-bit at 2 M and at M.  Reports ivf_pq_search / ivf_pq_refine times and recall@10 of the fused refine under both, against the exact
L2 top-10 (--scaled: computed here in numpy over the rows as f32 -- on rows of unequal length a dot-product shortlist would miss --,
else the refine over the flat scan's 1024 best dot products as above), and the
wall time of pq_set_metric("l2") beside pq_build for the plain, residual and rotated (a random orthonormal matrix) kinds at M.
--scaled multiplies row r by 0.5 + (r % 7) / 4 (the rows are then generated on the host).

    python tools_dev/bench_pq.py <rows> <dim> <f16|f32> 0 <M> --train

The trainers alone over every one of <rows> synthetic rows: seconds per Lloyd iteration of pq_train(bits=4) and pq_train(bits=8) at
the same M, alternating the widths run by run (lloyd_seconds), and one round of the numpy trainer over 20000 of the rows with 16
codewords."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nano-vectordb_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import nvdb_amd  # noqa: E402

U64MAX = np.iinfo(np.uint64).max


def train_codebooks(sample, M, rounds, seed, init=None, ksub=256):
    """[M, ksub, dsub] f32: per sub-quantiser ksub sampled sub-vectors (or init[m]), then `rounds` Lloyd rounds (nearest by squared L2, mean)."""
    rs = np.random.RandomState(seed)
    n, dim = sample.shape
    dsub = dim // M
    cb = np.empty((M, ksub, dsub), dtype=np.float32)
    for m in range(M):
        x = sample[:, m * dsub:(m + 1) * dsub]
        c = x[rs.choice(n, ksub, replace=False)].copy() if init is None else init[m].copy()
        for _ in range(rounds):
            d = (x * x).sum(1)[:, None] - 2.0 * x @ c.T + (c * c).sum(1)[None]
            a = d.argmin(1)
            for j in range(ksub):
                if (a == j).any():
                    c[j] = x[a == j].mean(0)
        cb[m] = c
    return cb


def quant_error(sample, cb):
    """fp64 mean over rows and sub-quantisers of the least squared distance to a codeword."""
    M, _, dsub = cb.shape
    total = 0.0
    for m in range(M):
        x, c = sample[:, m * dsub:(m + 1) * dsub].astype(np.float64), cb[m].astype(np.float64)
        total += sum(((x[i:i + 4096, None, :] - c[None]) ** 2).sum(-1).min(1).sum() for i in range(0, len(x), 4096))
    return total / (len(sample) * M)


def median_s(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def lloyd_seconds(owner, M, bits, rounds, max_train_rows=0, reps=7):
    """Seconds per Lloyd iteration of owner.pq_train: wall time of a call with `rounds` iterations minus that of one with none (the
    gather, the start and the copies are in both), over rounds; reps pairs after one warm-up pair -> (median, all)."""
    def call(iters):
        t0 = time.perf_counter(); owner.pq_train(M, iters, 7, max_train_rows=max_train_rows, bits=bits); return time.perf_counter() - t0
    call(rounds), call(0)
    ts = [(call(rounds) - call(0)) / rounds for _ in range(reps)]
    return float(np.median(ts)), ts


def main_train(rows, dim, dname, dtype, M):
    rounds = 4
    ctx = nvdb_amd.HipContext(0)
    ctx.generate_corpus(20240613, rows, dim, dtype)
    out = dict(mode="train", rows=rows, dim=dim, dtype=dname, M=M, rounds=rounds)
    for rep in range(2):                                                # the widths alternate; the second pass is the record
        for bits in (4, 8):
            s, every = lloyd_seconds(ctx, M, bits, rounds)
            out[f"pq{bits}"] = dict(s_per_iteration=s, all_s=every, out_err=ctx.pq_train(M, rounds, 7, bits=bits, want_err=True)[1].tolist())
    pick = np.arange(20000, dtype=np.int64) * rows // 20000
    raw = np.concatenate([ctx.download_rows(int(r), 1)[0] for r in pick])
    sample = (raw.view(np.float16) if dtype == nvdb_amd.DT_F16 else raw).astype(np.float32)
    host_s, host_all = median_s(lambda: train_codebooks(sample, M, 1, 7, ksub=16), reps=3)
    out["numpy_20000_rows_16_codewords"] = dict(s_per_iteration=host_s, all_s=host_all)
    for bits in (4, 8):
        d = out[f"pq{bits}"]
        print(f"pq_train(bits={bits}) M={M}, {rows} rows: {d['s_per_iteration'] * 1e3:.3f} ms per Lloyd iteration (median of 7; min {min(d['all_s']) * 1e3:.3f}, max {max(d['all_s']) * 1e3:.3f})")
    print(f"numpy, 16 codewords, 20000 rows: {host_s:.3f} s per round (median of 3; min {min(host_all):.3f}, max {max(host_all):.3f})")
    print(json.dumps(out))
    ctx.close()


def alternate_ms(fa, fb, calls, warmup):
    for _ in range(warmup):
        fa(); fb()
    ta, tb = [], []
    for _ in range(calls):
        t0 = time.perf_counter(); fa(); t1 = time.perf_counter(); fb(); t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3); tb.append((t2 - t1) * 1e3)
    return [float(np.median(t)) for t in (ta, tb)] + [float(np.min(ta)), float(np.max(ta)), float(np.min(tb)), float(np.max(tb))]


def recall(got, want):
    return float(np.mean([len(set(g[g != U64MAX].tolist()) & set(w.tolist())) / len(w) for g, w in zip(got, want)]))


def main_residual(rows, dim, dname, dtype, nlist, M, batch, calls, warmup, clustered):
    seed, K, rounds = 20240613, 10, 4
    out = dict(mode="residual", corpus="clustered" if clustered else "synthetic", rows=rows, dim=dim, dtype=dname, nlist=nlist, M=M, batch=batch,
               calls=calls, warmup=warmup, K=K)
    src = nvdb_amd.HipContext(0)
    rs = np.random.RandomState(11)
    if clustered:
        centres = rs.standard_normal((max(nlist // 4, 1), dim)).astype(np.float32)
        x = np.empty((rows, dim), dtype=np.float16 if dtype == nvdb_amd.DT_F16 else np.float32)
        for i in range(0, rows, 65536):
            n = min(65536, rows - i)
            v = centres[rs.randint(len(centres), size=n)] + 0.35 * rs.standard_normal((n, dim)).astype(np.float32)
            x[i:i + n] = v / np.linalg.norm(v, axis=1, keepdims=True)      # unit rows: the index's centroids are spherical k-means'
        src.upload_corpus(x.view(np.uint16) if dtype == nvdb_amd.DT_F16 else x, dtype)
        q = np.ascontiguousarray(x[rs.choice(rows, batch, replace=False)].astype(np.float32) + 0.1 * rs.standard_normal((batch, dim)).astype(np.float32))
        del x
    else:
        src.generate_corpus(seed, rows, dim, dtype)
        q = np.ascontiguousarray(nvdb_amd.synth_rows_f32(seed + 1, 0, batch, dim))
    fid, _ = src.search_batch(q, 1024)
    want, _ = src.refine_l2_topk(q, fid.astype(np.uint32), K)
    want = want.astype(np.uint64)
    cents = src.train_centroids(nlist, 2, seed, max_train_rows=262144)
    ixs = {False: nvdb_amd.IvfIndex(src, cents), True: nvdb_amd.IvfIndex(src, cents)}
    src.close()
    blocks = np.sort(rs.choice(rows - 1000, 20, replace=False))
    for residual, ix in ixs.items():
        cb = ix.pq_train(M, rounds, 7, max_train_rows=20000, residual=residual)
        build_s, build_all = median_s(lambda: ix.pq_build(cb, residual=residual), reps=3)
        err = 0.0
        for b in blocks:
            raw = ix.ctx.download_rows(int(b), 1000)[0]
            xs = (raw.view(np.float16) if dtype == nvdb_amd.DT_F16 else raw).astype(np.float64)
            err += ((xs - ix.pq_reconstruct(int(b), 1000).astype(np.float64)) ** 2).sum()
        out["residual" if residual else "plain"] = dict(pq_build_s=build_s, pq_build_all_s=build_all, quant_err=err / (len(blocks) * 1000 * M))
        print(f"{'residual' if residual else 'plain':8s}: pq_build {build_s:.3f} s (median of 3), fp64 quantisation error {err / (len(blocks) * 1000 * M):.6e}")
    a, b = ixs[False], ixs[True]
    for nprobe in (8, 32):
        for R in (100, 1024):
            key = f"nprobe={nprobe} R={R}"
            pa, pb, *spread = alternate_ms(lambda: a.pq_search(q, R, nprobe), lambda: b.pq_search(q, R, nprobe), calls, warmup)
            fa, fb, *fspread = alternate_ms(lambda: a.pq_refine(q, K, R, nprobe), lambda: b.pq_refine(q, K, R, nprobe), calls, warmup)
            ra, rb = recall(a.pq_refine(q, K, R, nprobe)[0], want), recall(b.pq_refine(q, K, R, nprobe)[0], want)
            out[key] = dict(plain_search_ms=pa, residual_search_ms=pb, search_spread=spread, plain_refine_ms=fa, residual_refine_ms=fb, refine_spread=fspread,
                            recall10_plain=ra, recall10_residual=rb)
            print(f"{key:20s}: ivf_pq_search plain {pa:8.3f} ms | residual {pb:8.3f} ms || ivf_pq_refine plain {fa:8.3f} ms | residual {fb:8.3f} ms || "
                  f"recall@10 plain {ra:.4f}, residual {rb:.4f}")
    print(json.dumps(out))
    for ix in ixs.values():
        ix.close()


def learn_rotation(sctx, sample, M, rounds, alternations, residual=False):
    """OPQ's alternation in numpy over a sample context: codebooks and codes under A on the device (pq_train / pq_build with
    rotation=A), yhat from the codes, A <- U V^T of the SVD of sum yhat x^T (orthonormal by construction).  Starts from I."""
    dim = sample.shape[1]
    A = np.eye(dim, dtype=np.float32)
    x64 = sample.astype(np.float64)
    for _ in range(alternations):
        cb = sctx.pq_train(M, rounds, 7, rotation=A, residual=residual)
        sctx.pq_build(cb, rotation=A, residual=residual)
        yhat = cb[np.arange(M), sctx.pq_download_codes()].reshape(len(sample), dim).astype(np.float64)
        u, _, vt = np.linalg.svd(yhat.T @ x64)
        A = np.ascontiguousarray((u @ vt).astype(np.float32))
    return A


def main_opq(rows, dim, dname, dtype, nlist, M, batch, calls, warmup, corpus):
    seed, K, rounds = 20240613, 10, 4
    out = dict(mode="opq", corpus=corpus, rows=rows, dim=dim, dtype=dname, nlist=nlist, M=M, batch=batch, calls=calls, warmup=warmup, K=K)
    src = nvdb_amd.HipContext(0)
    rs = np.random.RandomState(11)
    if corpus == "synthetic":
        src.generate_corpus(seed, rows, dim, dtype)
        q = np.ascontiguousarray(nvdb_amd.synth_rows_f32(seed + 1, 0, batch, dim))
    else:
        # clustered: main_residual's centre + noise rows; decay: one Gaussian whose per-dimension deviation falls as 1 / sqrt(1 + t / 8),
        # t the dimension -- the first sub-vectors carry most of the variance, which is what a rotation can balance
        centres = rs.standard_normal((max(nlist // 4, 1), dim)).astype(np.float32)
        sigma = (1.0 / np.sqrt(1.0 + np.arange(dim) / 8.0)).astype(np.float32)
        x = np.empty((rows, dim), dtype=np.float16 if dtype == nvdb_amd.DT_F16 else np.float32)
        for i in range(0, rows, 65536):
            n = min(65536, rows - i)
            g = rs.standard_normal((n, dim)).astype(np.float32)
            v = centres[rs.randint(len(centres), size=n)] + 0.35 * g if corpus == "clustered" else g * sigma
            x[i:i + n] = v / np.linalg.norm(v, axis=1, keepdims=True)
        src.upload_corpus(x.view(np.uint16) if dtype == nvdb_amd.DT_F16 else x, dtype)
        q = np.ascontiguousarray(x[rs.choice(rows, batch, replace=False)].astype(np.float32) + 0.1 * rs.standard_normal((batch, dim)).astype(np.float32))
        del x
    fid, _ = src.search_batch(q, 1024)
    want, _ = src.refine_l2_topk(q, fid.astype(np.uint32), K)
    want = want.astype(np.uint64)
    cents = src.train_centroids(nlist, 2, seed, max_train_rows=262144)
    ixs = {False: nvdb_amd.IvfIndex(src, cents), True: nvdb_amd.IvfIndex(src, cents)}
    src.close()
    ix = ixs[True]
    # the rotation: learnt over 20000 list-ordered rows sampled through the library
    pick = np.arange(20000, dtype=np.int64) * rows // 20000
    raw = np.concatenate([ix.ctx.download_rows(int(r), 1)[0] for r in pick])
    sample = (raw.view(np.float16) if dtype == nvdb_amd.DT_F16 else raw).astype(np.float32)
    sctx = nvdb_amd.HipContext(0)
    sctx.upload_corpus(raw, dtype)
    t0 = time.perf_counter()
    A = learn_rotation(sctx, sample, M, rounds, 4)
    out["learn_rotation_s"] = time.perf_counter() - t0
    sctx.close()
    out["orthonormality"] = float(np.abs(A.astype(np.float64) @ A.astype(np.float64).T - np.eye(dim)).max())
    blocks = np.sort(rs.choice(rows - 1000, 20, replace=False))
    for rotated, ix in ixs.items():
        rot = A if rotated else None
        cb = ix.pq_train(M, rounds, 7, max_train_rows=20000, rotation=rot)
        build_s, build_all = median_s(lambda: ix.pq_build(cb, rotation=rot), reps=3)
        err = 0.0
        for b in blocks:
            raw = ix.ctx.download_rows(int(b), 1000)[0]
            xs = (raw.view(np.float16) if dtype == nvdb_amd.DT_F16 else raw).astype(np.float64)
            err += ((xs - ix.pq_reconstruct(int(b), 1000).astype(np.float64)) ** 2).sum()
        name = "opq" if rotated else "plain"
        out[name] = dict(pq_build_s=build_s, pq_build_all_s=build_all, quant_err=err / (len(blocks) * 1000 * M))
        print(f"{name:5s}: pq_build {build_s:.3f} s (median of 3), fp64 quantisation error {err / (len(blocks) * 1000 * M):.6e}")
    ideal = 2.0 * rows * dim * dim / 157e12
    extra = out["opq"]["pq_build_s"] - out["plain"]["pq_build_s"]
    out["rotate"] = dict(mfma_bound_s=ideal, build_difference_s=extra, bound_over_difference=ideal / extra if extra > 0 else None)
    print(f"rotation inside the build: opq - plain = {extra:.3f} s (the product, the slab, and an encode that reads f32 rows) against "
          f"2 n dim^2 / 157 TFLOP/s = {ideal:.3f} s: {ideal / extra if extra > 0 else float('nan'):.3f} of the matrix cores' peak")
    a, b = ixs[False], ixs[True]
    for nprobe in (8, 32):
        for R in (100, 1024):
            key = f"nprobe={nprobe} R={R}"
            pa, pb, *spread = alternate_ms(lambda: a.pq_search(q, R, nprobe), lambda: b.pq_search(q, R, nprobe), calls, warmup)
            fa, fb, *fspread = alternate_ms(lambda: a.pq_refine(q, K, R, nprobe), lambda: b.pq_refine(q, K, R, nprobe), calls, warmup)
            ra, rb = recall(a.pq_refine(q, K, R, nprobe)[0], want), recall(b.pq_refine(q, K, R, nprobe)[0], want)
            out[key] = dict(plain_search_ms=pa, opq_search_ms=pb, search_spread=spread, plain_refine_ms=fa, opq_refine_ms=fb, refine_spread=fspread,
                            recall10_plain=ra, recall10_opq=rb)
            print(f"{key:20s}: ivf_pq_search plain {pa:8.3f} ms | opq {pb:8.3f} ms || ivf_pq_refine plain {fa:8.3f} ms | opq {fb:8.3f} ms || "
                  f"recall@10 plain {ra:.4f}, opq {rb:.4f}")
    print(json.dumps(out))
    for ix in ixs.values():
        ix.close()


def main_bits(rows, dim, dname, dtype, nlist, M, batch, calls, warmup, clustered):
    seed, K, rounds = 20240613, 10, 4
    out = dict(mode="bits4", corpus="clustered" if clustered else "synthetic", rows=rows, dim=dim, dtype=dname, nlist=nlist, M=M, batch=batch,
               calls=calls, warmup=warmup, K=K)
    src = nvdb_amd.HipContext(0)
    rs = np.random.RandomState(11)
    if clustered:                                                       # main_residual's centre + noise rows
        centres = rs.standard_normal((max(nlist // 4, 1), dim)).astype(np.float32)
        x = np.empty((rows, dim), dtype=np.float16 if dtype == nvdb_amd.DT_F16 else np.float32)
        for i in range(0, rows, 65536):
            n = min(65536, rows - i)
            v = centres[rs.randint(len(centres), size=n)] + 0.35 * rs.standard_normal((n, dim)).astype(np.float32)
            x[i:i + n] = v / np.linalg.norm(v, axis=1, keepdims=True)
        src.upload_corpus(x.view(np.uint16) if dtype == nvdb_amd.DT_F16 else x, dtype)
        q = np.ascontiguousarray(x[rs.choice(rows, batch, replace=False)].astype(np.float32) + 0.1 * rs.standard_normal((batch, dim)).astype(np.float32))
        del x
    else:
        src.generate_corpus(seed, rows, dim, dtype)
        q = np.ascontiguousarray(nvdb_amd.synth_rows_f32(seed + 1, 0, batch, dim))
    fid, _ = src.search_batch(q, 1024)
    want, _ = src.refine_l2_topk(q, fid.astype(np.uint32), K)
    want = want.astype(np.uint64)
    cents = src.train_centroids(nlist, 2, seed, max_train_rows=262144)
    a, b = nvdb_amd.IvfIndex(src, cents), nvdb_amd.IvfIndex(src, cents)
    src.close()
    blocks = np.sort(rs.choice(rows - 1000, 20, replace=False))

    def shadow(ix, m, ksub):
        bits = 4 if ksub == 16 else 8
        cb = ix.pq_train(m, rounds, 7, max_train_rows=262144, bits=bits)
        it_s, it_all = lloyd_seconds(ix, m, bits, rounds, max_train_rows=262144, reps=3)
        print(f"{bits}-bit M={m}: pq_train over {min(rows, 262144)} rows {it_s * 1e3:.3f} ms per Lloyd iteration (median of 3: {' '.join(f'{t * 1e3:.3f}' for t in it_all)})")
        build_s, build_all = median_s(lambda: ix.pq_build(cb), reps=3)
        err = 0.0
        for blk in blocks:
            r = ix.ctx.download_rows(int(blk), 1000)[0]
            xs = (r.view(np.float16) if dtype == nvdb_amd.DT_F16 else r).astype(np.float64)
            err += ((xs - ix.pq_reconstruct(int(blk), 1000).astype(np.float64)) ** 2).sum()
        d = dict(M=m, bits=ix.pq_bits(), bytes_per_row=ix.ctx.pq_info()["code_bytes"] // rows, pq_train_s_per_iteration=it_s, pq_train_all_s=it_all,
                 pq_build_s=build_s, pq_build_all_s=build_all,
                 quant_err_per_row=err / (len(blocks) * 1000))
        print(f"{d['bits']}-bit M={m}: {d['bytes_per_row']} bytes per row, pq_build {build_s:.3f} s (median of 3), fp64 |x - xhat|^2 per row {d['quant_err_per_row']:.6e}")
        return d

    out["pq8"] = shadow(a, M, 256)
    for m4 in (2 * M, M):
        tag = f"pq4_M{m4}"
        out[tag] = shadow(b, m4, 16)
        for nprobe in (8, 32):
            for R in (100, 1024):
                key = f"{tag} nprobe={nprobe} R={R}"
                pa, pb, *spread = alternate_ms(lambda: a.pq_search(q, R, nprobe), lambda: b.pq_search(q, R, nprobe), calls, warmup)
                fa, fb, *fspread = alternate_ms(lambda: a.pq_refine(q, K, R, nprobe), lambda: b.pq_refine(q, K, R, nprobe), calls, warmup)
                ra, rb = recall(a.pq_refine(q, K, R, nprobe)[0], want), recall(b.pq_refine(q, K, R, nprobe)[0], want)
                out[key] = dict(pq8_search_ms=pa, pq4_search_ms=pb, search_spread=spread, pq8_refine_ms=fa, pq4_refine_ms=fb, refine_spread=fspread,
                                recall10_pq8=ra, recall10_pq4=rb)
                print(f"{key:32s}: ivf_pq_search 8-bit {pa:8.3f} ms | 4-bit {pb:8.3f} ms || ivf_pq_refine 8-bit {fa:8.3f} ms | 4-bit {fb:8.3f} ms || "
                      f"recall@10 8-bit {ra:.4f}, 4-bit {rb:.4f}")
    print(json.dumps(out))
    a.close()
    b.close()


def main_l2(rows, dim, dname, dtype, nlist, M, batch, calls, warmup, clustered, scaled):
    seed, K, rounds = 20240613, 10, 4
    out = dict(mode="l2", corpus=("clustered" if clustered else "synthetic") + (" scaled" if scaled else ""), rows=rows, dim=dim, dtype=dname, nlist=nlist,
               M=M, batch=batch, calls=calls, warmup=warmup, K=K)
    src = nvdb_amd.HipContext(0)
    rs = np.random.RandomState(11)
    if clustered or scaled:                                             # rows made on the host
        centres = rs.standard_normal((max(nlist // 4, 1), dim)).astype(np.float32)
        x = np.empty((rows, dim), dtype=np.float16 if dtype == nvdb_amd.DT_F16 else np.float32)
        for i in range(0, rows, 65536):
            n = min(65536, rows - i)
            if clustered:                                               # main_residual's centre + noise rows, unit length
                v = centres[rs.randint(len(centres), size=n)] + 0.35 * rs.standard_normal((n, dim)).astype(np.float32)
                v /= np.linalg.norm(v, axis=1, keepdims=True)
            else:
                v = nvdb_amd.synth_rows_f32(seed, i, n, dim)
            x[i:i + n] = v * (0.5 + (np.arange(i, i + n) % 7) / 4).astype(np.float32)[:, None] if scaled else v
        src.upload_corpus(x.view(np.uint16) if dtype == nvdb_amd.DT_F16 else x, dtype)
    else:
        src.generate_corpus(seed, rows, dim, dtype)
    q = np.ascontiguousarray(x[rs.choice(rows, batch, replace=False)].astype(np.float32) + 0.1 * rs.standard_normal((batch, dim)).astype(np.float32)) if clustered \
        else np.ascontiguousarray(nvdb_amd.synth_rows_f32(seed + 1, 0, batch, dim))
    if scaled:
        # exact L2 top-K in numpy, |x|^2 - 2 q.x block by block (|q|^2 orders nothing): rows of unequal length, so no dot-product shortlist
        best_d, best_i = np.full((batch, K), np.inf, dtype=np.float32), np.zeros((batch, K), dtype=np.int64)
        for i in range(0, rows, 65536):
            xb = x[i:i + 65536].astype(np.float32)
            d = np.concatenate([best_d, (xb * xb).sum(1)[None] - 2.0 * q @ xb.T], axis=1)
            ids = np.concatenate([best_i, np.broadcast_to(np.arange(i, i + len(xb)), (batch, len(xb)))], axis=1)
            keep = np.argpartition(d, K - 1, axis=1)[:, :K]
            best_d, best_i = np.take_along_axis(d, keep, 1), np.take_along_axis(ids, keep, 1)
        want = best_i.astype(np.uint64)
    else:                                                               # rows of one length: the refine over the flat scan's 1024 best dot products, as above
        fid, _ = src.search_batch(q, 1024)
        want = src.refine_l2_topk(q, fid.astype(np.uint32), K)[0].astype(np.uint64)
    x = None
    cents = src.train_centroids(nlist, 2, seed, max_train_rows=262144)
    ix = nvdb_amd.IvfIndex(src, cents)
    src.close()
    A = np.ascontiguousarray(np.linalg.qr(rs.standard_normal((dim, dim)))[0].astype(np.float32))
    for kind, residual, rot in (("plain", False, None), ("residual", True, None), ("rotated", False, A)):
        cb = ix.pq_train(M, rounds, 7, max_train_rows=20000, residual=residual, rotation=rot)
        build_s, build_all = median_s(lambda: ix.pq_build(cb, residual=residual, rotation=rot), reps=3)

        def to_l2():
            ix.pq_set_metric("dot"); t0 = time.perf_counter(); ix.pq_set_metric("l2"); return time.perf_counter() - t0
        to_l2()
        ts = [to_l2() for _ in range(3)]
        out[f"set_metric {kind}"] = dict(pq_build_s=build_s, pq_build_all_s=build_all, set_metric_l2_s=float(np.median(ts)), set_metric_l2_all_s=ts)
        print(f"{kind:8s} 8-bit M={M}: pq_build {build_s:.3f} s | pq_set_metric('l2') {np.median(ts):.4f} s (medians of 3: {' '.join(f'{t:.4f}' for t in ts)})")

    def under(metric, f):
        def call():
            ix.pq_set_metric(metric)                                    # (timed apart from f: see set_metric above; the toggle is not what a user repeats)
            t0 = time.perf_counter(); r = f(); return time.perf_counter() - t0, r
        return call

    for bits, m in ((8, M), (4, 2 * M), (4, M)):
        ix.pq_build(ix.pq_train(m, rounds, 7, max_train_rows=262144, bits=bits))
        for nprobe in (8, 32):
            for R in (100, 1024):
                key, row = f"pq{bits}_M{m} nprobe={nprobe} R={R}", {}
                for name, f in (("search", lambda: ix.pq_search(q, R, nprobe)), ("refine", lambda: ix.pq_refine(q, K, R, nprobe))):
                    dot, l2 = under("dot", f), under("l2", f)
                    for _ in range(warmup):
                        dot(); l2()
                    td, tl = zip(*[(dot()[0] * 1e3, l2()[0] * 1e3) for _ in range(calls)])
                    row.update({f"dot_{name}_ms": float(np.median(td)), f"l2_{name}_ms": float(np.median(tl)), f"{name}_spread": [min(td), max(td), min(tl), max(tl)]})
                row.update(recall10_dot=recall(under("dot", lambda: ix.pq_refine(q, K, R, nprobe))()[1][0], want),
                           recall10_l2=recall(under("l2", lambda: ix.pq_refine(q, K, R, nprobe))()[1][0], want))
                out[key] = row
                print(f"{key:32s}: ivf_pq_search dot {row['dot_search_ms']:8.3f} ms | l2 {row['l2_search_ms']:8.3f} ms || ivf_pq_refine dot {row['dot_refine_ms']:8.3f} ms | "
                      f"l2 {row['l2_refine_ms']:8.3f} ms || recall@10 dot {row['recall10_dot']:.4f}, l2 {row['recall10_l2']:.4f}")
    print(json.dumps(out))
    ix.close()


def main():
    argv = [x for i, x in enumerate(sys.argv[1:]) if not (i and sys.argv[i] == "--bits")]       # (--bits takes a value)
    if "--bits" in sys.argv and sys.argv[sys.argv.index("--bits") + 1:][:1] != ["4"]:
        raise SystemExit("--bits 4 is the only width beside the default")
    flags = [x for x in argv if x.startswith("--")]
    a = [x for x in argv if not x.startswith("--")]
    rows = int(a[0]) if len(a) > 0 else 10_000_000
    dim = int(a[1]) if len(a) > 1 else 768
    dname = a[2] if len(a) > 2 else "f16"
    dtype = {"f16": nvdb_amd.DT_F16, "f32": nvdb_amd.DT_F32}[dname]
    nlist = int(a[3]) if len(a) > 3 else 4096
    M = int(a[4]) if len(a) > 4 else 48
    batch = int(a[5]) if len(a) > 5 else 1024
    calls = int(a[6]) if len(a) > 6 else 10
    warmup = int(a[7]) if len(a) > 7 else 2
    if "--train" in flags:
        return main_train(rows, dim, dname, dtype, M)
    if "--l2" in flags:
        return main_l2(rows, dim, dname, dtype, nlist, M, batch, calls, warmup, "--clustered" in flags, "--scaled" in flags)
    if "--bits" in flags:
        return main_bits(rows, dim, dname, dtype, nlist, M, batch, calls, warmup, "--clustered" in flags)
    if "--opq" in flags:
        corpus = "clustered" if "--clustered" in flags else "decay" if "--decay" in flags else "synthetic"
        return main_opq(rows, dim, dname, dtype, nlist, M, batch, calls, warmup, corpus)
    if "--residual" in flags:
        return main_residual(rows, dim, dname, dtype, nlist, M, batch, calls, warmup, "--clustered" in flags)
    seed, K = 20240613, 10
    out = dict(rows=rows, dim=dim, dtype=dname, nlist=nlist, M=M, batch=batch, calls=calls, warmup=warmup, K=K)

    src = nvdb_amd.HipContext(0)
    src.generate_corpus(seed, rows, dim, dtype)
    q = np.ascontiguousarray(nvdb_amd.synth_rows_f32(seed + 1, 0, batch, dim))
    # the exact flat top-10 by squared L2: the refine over the flat scan's 1024 best dot products
    fid, _ = src.search_batch(q, 1024)
    want, _ = src.refine_l2_topk(q, fid.astype(np.uint32), K)
    want = want.astype(np.uint64)
    t0 = time.perf_counter()
    cents = src.train_centroids(nlist, 2, seed, max_train_rows=262144)
    t1 = time.perf_counter()
    ix = nvdb_amd.IvfIndex(src, cents)
    t2 = time.perf_counter()
    rs = np.random.RandomState(3)
    pick = np.sort(rs.choice(rows, 20000, replace=False))
    raw = np.concatenate([src.download_rows(int(r), 1)[0] for r in pick])
    sample = raw.view(np.float16).astype(np.float32) if dtype == nvdb_amd.DT_F16 else raw
    src.close()
    sctx = nvdb_amd.HipContext(0)                                       # the sample as a corpus of its own: both trainers see the same rows
    sctx.upload_corpus(raw, dtype)
    rounds = 4
    start = sctx.pq_train(M, 0, 7)
    t3 = time.perf_counter()
    cb = sctx.pq_train(M, rounds, 7)                                    # (first call: the code object loads here)
    t4 = time.perf_counter()
    ix.pq_build(cb)
    t5 = time.perf_counter()
    dev_s, dev_all = median_s(lambda: sctx.pq_train(M, rounds, 7))
    host_s, host_all = median_s(lambda: train_codebooks(sample, M, rounds, 7, start))
    cb_host = train_codebooks(sample, M, rounds, 7, start)
    sctx.close()
    out["build"] = dict(train_centroids_s=t1 - t0, ivf_build_s=t2 - t1, codebooks_device_first_call_s=t4 - t3, pq_build_s=t5 - t4)
    out["codebooks"] = dict(sample_rows=len(sample), rounds=rounds, device_s=dev_s, device_all_s=dev_all, host_s=host_s, host_all_s=host_all,
                            err_start=quant_error(sample, start), err_device=quant_error(sample, cb), err_host=quant_error(sample, cb_host))
    print(f"train_centroids {t1 - t0:.2f} s, ivf_build {t2 - t1:.2f} s, device codebooks (first call) {t4 - t3:.3f} s, pq_build (upload + encode {rows} rows) {t5 - t4:.3f} s")
    print("codebooks, {sample_rows} rows, {rounds} rounds, same start: device {device_s:.4f} s | numpy {host_s:.3f} s (medians of 5 after a warm-up); "
          "fp64 quantisation error: start {err_start:.6e}, device {err_device:.6e}, numpy {err_host:.6e}".format(**out["codebooks"]))
    perm = ix.info()["perm"].astype(np.uint64)

    def exact_then_refine(R, nprobe):
        ids, _, _ = ix.ctx.search_ivf_anyk(q, R, nprobe)                 # positions in the index's rows, as the refine wants them
        return ix.ctx.refine_l2_topk(q, np.where(ids == U64MAX, 0xFFFFFFFF, ids).astype(np.uint32), K)

    for nprobe in (8, 32):
        for R in (100, 1024):
            key = f"nprobe={nprobe} R={R}"
            pq, ex, *spread = alternate_ms(lambda: ix.pq_search(q, R, nprobe), lambda: ix.search_anyk(q, R, nprobe), calls, warmup)
            st = ix.ctx.stats()
            fpq, fex, *fspread = alternate_ms(lambda: ix.pq_refine(q, K, R, nprobe), lambda: exact_then_refine(R, nprobe), calls, warmup)
            got_pq, _ = ix.pq_refine(q, K, R, nprobe)
            rid, _ = exact_then_refine(R, nprobe)
            got_ex = np.where(rid == 0xFFFFFFFF, U64MAX, perm[np.minimum(rid, rows - 1)])
            out[key] = dict(pq_search_ms=pq, anyk_ms=ex, search_spread=spread, pq_refine_ms=fpq, anyk_refine_ms=fex, refine_spread=fspread,
                            recall10_pq=recall(got_pq, want), recall10_exact_route=recall(got_ex, want), rows_scanned_last=st["rows_scanned"])
            print(f"{key:20s}: ivf_pq_search {pq:8.3f} ms | ivf_search_anyk {ex:8.3f} ms || ivf_pq_refine {fpq:8.3f} ms | anyk + refine {fex:8.3f} ms || "
                  f"recall@10 pq {out[key]['recall10_pq']:.4f}, exact route {out[key]['recall10_exact_route']:.4f}")
    print(json.dumps(out))
    ix.close()


if __name__ == "__main__":
    main()
