"""PQ shadows under an OPQ rotation (nvdb_hip_pq_build_opq / _train_opq / _rotation / _rotated_rows / _rotate, the searches and
pq_reconstruct over such a shadow) against numpy fp64 of the header's definitions.  Fixture: test_gpu_pq_residual.py's 5000 rows and
six awkward partitions, every case plain and residual, plus dim 1024 at 600 rows (64 K slices).  A: np.linalg.qr's Q as float32.
Bounds.  y[i] is a chain of dim fmas, one rounding each: |y - y64| <= 1.01 dim eps sum_t |A[i][t] e[t]|; the reconstruction adds one
addition: 1.01 (dim + 1) eps (sum_i |A[i][t] yhat[i]| + |c[t]|).  The encode and the scores are checked on the GPU's OWN y and q'
bits, so their bounds are test_gpu_pq_residual.py's: the winner within 2 (dsub + 3) eps of the least fp64 distance, and tol = 1.01
eps ((ceil(dim / 64) + 7) sum |q c| + (dsub + M + 1) sum_m A[m][code]) -- a plain shadow, without base term and last addition: dsub + M."""
import numpy as np
import pytest

import nvdb_amd
from test_gpu_pq_residual import BIG, EPS, F16, F32, I8, ROW_BASE, SEED, U64MAX, make_codebooks, rows_f32

pytestmark = pytest.mark.gpu

TABLES = {5000: [0, 0, 37, 101, 2300, 4990, 5000], 600: [0, 0, 37, 101, 300, 590, 600]}
SHAPES = [(F16, 32, 4), (F16, 96, 48), (F16, 100, 4),    # column tail 4, dsub 25
          (F16, 272, 68),                                # three column panels, the last of 16 columns; 17 K slices
          (F32, 64, 16), (I8, 64, 16)]
CASES = [s + (5000, r) for s in SHAPES for r in (False, True)] + [(F16, 1024, 32, 600, True)]
_cache = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def case(dtype, dim, M, n, residual):
    """One corpus with its rotated shadow, built once: E the float32 rows the rotation reads, Y the GPU's own rotated rows."""
    key = (dtype, dim, M, n, residual)
    if key not in _cache:
        base, scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, n, dim, dtype)
        off = np.array(TABLES[n], dtype=np.uint64)
        list_of = np.repeat(np.arange(len(off) - 1), np.diff(off).astype(np.int64))
        X = rows_f32(base, scales, dtype)
        cents = np.ones((len(off) - 1, dim), dtype=np.float32)
        for p in range(len(off) - 1):
            if off[p + 1] > off[p]:
                cents[p] = X[int(off[p]):int(off[p + 1])].mean(0, dtype=np.float32)
        A = np.linalg.qr(np.random.RandomState(dim).standard_normal((dim, dim)))[0].astype(np.float32)
        E = X - cents[list_of] if residual else X
        ctx = nvdb_amd.HipContext(0)
        ctx.upload_corpus(base, dtype, scales, ROW_BASE)
        ctx.set_partitions(off)
        ctx.set_centroids(cents)
        cb = make_codebooks((E.astype(np.float64) @ A.astype(np.float64).T).astype(np.float32), M)
        ctx.pq_build(cb, residual=residual, rotation=A)
        _cache[key] = dict(ctx=ctx, off=off, list_of=list_of, cents=cents, A=A, E=E, cb=cb, Y=ctx.pq_rotated_rows(), codes=ctx.pq_download_codes(),
                           queries=nvdb_amd.synth_rows_f32(SEED + 1, 0, 19, dim))
    return _cache[key]


def chain_ratio(got, mat, x, extra=0.0, steps=None):
    """max of |got - fp64(x . mat^T + extra)| over its bound 1.01 steps eps (|x| . |mat|^T + |extra|)"""
    m64, x64 = mat.astype(np.float64), x.astype(np.float64)
    bound = 1.01 * (steps or mat.shape[1]) * EPS * (np.abs(x64) @ np.abs(m64).T + np.abs(extra))
    return (np.abs(got.astype(np.float64) - (x64 @ m64.T + extra)) / np.maximum(bound, 1e-300)).max()


def windows(fn, full, n):
    """single rows and a 66-row window across a list boundary are bit-equal to slices of the full call, and so is a second full call"""
    for r in (0, 36, 37, 100, 101, n - 11, n - 1):
        assert np.array_equal(bits(fn(r, 1)), bits(full[r:r + 1])), r
    assert np.array_equal(bits(fn(36, 66)), bits(full[36:102])) and np.array_equal(bits(fn()), bits(full))


@pytest.mark.parametrize("dtype,dim,M,n,residual", CASES)
def test_rotation(dtype, dim, M, n, residual):
    c = case(dtype, dim, M, n, residual)
    ctx, q = c["ctx"], c["queries"]
    ratio = chain_ratio(c["Y"], c["A"], c["E"])
    qr = ctx.pq_rotate(q)
    qratio = chain_ratio(qr, c["A"], q)
    print(f"worst |y - y64| / bound: rows {ratio:.3f}, queries {qratio:.3f}")
    assert ratio <= 1 and qratio <= 1
    windows(ctx.pq_rotated_rows, c["Y"], n)
    assert np.array_equal(bits(ctx.pq_rotate(q[:1])), bits(qr[:1])) and np.array_equal(bits(ctx.pq_rotate(q)), bits(qr))
    assert np.array_equal(bits(ctx.pq_rotation()), bits(c["A"])) and ctx.pq_kind() == dict(residual=residual)


@pytest.mark.parametrize("dtype,dim,M,n,residual", CASES)
def test_encode_and_reconstruct(dtype, dim, M, n, residual):
    c = case(dtype, dim, M, n, residual)
    dsub, codes, ctx = dim // M, c["codes"], c["ctx"]
    sub = c["Y"].astype(np.float64).reshape(n, M, dsub)                                                # the GPU's own y: what the encode saw
    for m in range(M):
        d64 = ((sub[:, m, None, :] - c["cb"][m].astype(np.float64)[None]) ** 2).sum(-1)
        got = d64[np.arange(n), codes[:, m]]
        assert (got <= d64.min(1) * (1 + 2 * (dsub + 3) * EPS)).all(), m
    yhat = c["cb"][np.arange(M), codes].reshape(n, dim)
    full = ctx.pq_reconstruct()
    ratio = chain_ratio(full, c["A"].T, yhat, c["cents"][c["list_of"]].astype(np.float64) if residual else 0.0, dim + 1)
    print(f"worst |xhat - xhat64| / bound: {ratio:.3f}")
    assert ratio <= 1
    windows(ctx.pq_reconstruct, full, n)


@pytest.mark.parametrize("dtype,dim,M,n,residual", [CASES[0], CASES[5], CASES[7], CASES[9], CASES[11]])
def test_train(dtype, dim, M, n, residual):
    c = case(dtype, dim, M, n, residual)
    ctx, A, dsub, b = c["ctx"], c["A"], dim // M, 2 * (dim // M + 3) * EPS
    kw = dict(init=c["cb"], rotation=A, residual=residual)
    cb1, cb2 = ctx.pq_train(M, 1, SEED, **kw), ctx.pq_train(M, 2, SEED, **kw)
    assert np.array_equal(bits(cb2), bits(ctx.pq_train(M, 2, SEED, **kw))) and not np.array_equal(cb1, cb2)
    assert not np.array_equal(cb2, ctx.pq_train(M, 2, SEED, init=c["cb"], residual=residual))          # (and not the unrotated trainer's)
    ctx.pq_build(cb1, residual=residual, rotation=A)                     # the second iteration's assignment is this build's codes
    codes = ctx.pq_download_codes()
    ctx.pq_build(c["cb"], residual=residual, rotation=A)                 # (the cached shadow back)
    sub = c["Y"].astype(np.float64).reshape(n, M, dsub)
    for m in range(M):
        d64 = ((sub[:, m, None, :] - cb1[m].astype(np.float64)[None]) ** 2).sum(-1)
        two = np.partition(d64, 1, axis=1)
        clear = two[:, 1] * (1 - b) > two[:, 0] * (1 + b)                # the fp64 margin exceeds the encode bound: the code is decided
        assert clear.any() and np.array_equal(codes[clear, m], d64.argmin(1)[clear]), m
        count = np.bincount(codes[:, m], minlength=256)
        live = count > 0
        s, sabs = (np.stack([np.bincount(codes[:, m], weights=w[:, m, t], minlength=256) for t in range(dsub)], 1) for w in (sub, np.abs(sub)))
        ref = (s[live] / count[live, None]).astype(np.float32)
        assert (np.abs(cb2[m][live].astype(np.float64) - ref) <= np.spacing(np.abs(ref)).astype(np.float64) + 2.0 ** -52 * sabs[live]).all(), m
        assert np.array_equal(bits(cb2[m][~live]), bits(cb1[m][~live])), m


@pytest.mark.parametrize("R", [10, 5000])
@pytest.mark.parametrize("dtype,dim,M,n,residual", CASES)
def test_scores(dtype, dim, M, n, residual, R):
    c = case(dtype, dim, M, n, residual)
    ctx, off, list_of, codes, queries, dsub = c["ctx"], c["off"], c["list_of"], c["codes"], c["queries"], dim // M
    probe = np.stack([np.full(19, BIG), np.arange(19) % 6, (np.arange(19) * 5 + 1) % 6], axis=1).astype(np.uint32)
    qrot = ctx.pq_rotate(queries)                                        # the GPU's own q' bits: what the tables are made of
    ids, scores, counts = ctx.pq_search_partitions(queries, R, probe)
    marange, worst = np.arange(M), 0.0
    for q in range(19):
        prod = qrot[q].astype(np.float64).reshape(M, 1, dsub) * c["cb"].astype(np.float64)
        L64, A64 = prod.sum(-1), np.abs(prod).sum(-1)
        qc = queries[q].astype(np.float64)[None] * c["cents"].astype(np.float64) * residual            # the UNROTATED base term, or none
        rows = np.concatenate([np.arange(off[p], off[p + 1], dtype=np.int64) for p in sorted(set(probe[q].tolist()))])
        s64 = qc.sum(1)[list_of[rows]] + L64[marange, codes[rows]].sum(1)
        tol = 1.01 * EPS * ((-(-dim // 64) + 7) * np.abs(qc).sum(1)[list_of[rows]] + (dsub + M + residual) * A64[marange, codes[rows]].sum(1)).max()
        cnt = min(R, len(rows))
        assert counts[q] == cnt and (ids[q, cnt:] == U64MAX).all() and np.isneginf(scores[q, cnt:]).all()
        local = (ids[q, :cnt] - np.uint64(ROW_BASE)).astype(np.int64)
        assert np.isin(local, rows).all() and len(set(local)) == cnt
        pos = np.searchsorted(rows, local)
        worst = max(worst, np.abs(scores[q, :cnt].astype(np.float64) - s64[pos]).max() / tol)
        rest = np.delete(s64, pos)
        assert not rest.size or s64[pos].min() >= rest.max() - 2 * tol
        assert (np.lexsort((local, -scores[q, :cnt])) == np.arange(cnt)).all()
    print(f"worst |score - s64| / tol: {worst:.3f}")
    assert worst <= 1


def test_non_finite_reach_only_their_outputs():
    """A non-orthonormal A with NaN and inf in row 5, a corpus row (50) with both: y is non-finite in row 50 and column 5 ONLY, q' in column 5, xhat in columns 3 and 40"""
    n, dim, M = 5000, 64, 16
    base = nvdb_amd.synth_corpus(SEED, ROW_BASE, n, dim, F32)[0].copy()
    A = np.random.RandomState(9).standard_normal((dim, dim)).astype(np.float32)
    Aok, Xok = A.copy(), base.copy()
    A[5, 3], A[5, 40], base[50, 7], base[50, 9] = np.nan, np.inf, np.nan, np.inf
    ctx = nvdb_amd.HipContext(0)
    ctx.upload_corpus(base, F32, None, ROW_BASE)
    ctx.pq_build(make_codebooks(Xok @ Aok.T, M), rotation=A)
    Y, q = ctx.pq_rotated_rows(), nvdb_amd.synth_rows_f32(SEED + 1, 0, 19, dim)
    bad = np.zeros((n, dim), dtype=bool)
    bad[50], bad[:, 5] = True, True
    assert np.array_equal(~np.isfinite(Y), bad)
    assert chain_ratio(np.where(bad, 0, Y), np.where(np.arange(dim)[:, None] == 5, 0, Aok), np.where(np.arange(n)[:, None] == 50, 0, Xok)) <= 1
    assert np.array_equal(~np.isfinite(ctx.pq_rotate(q)), np.broadcast_to(np.arange(dim) == 5, (19, dim)))
    assert np.isfinite(np.delete(ctx.pq_reconstruct(), [3, 40], axis=1)).all()
    ctx.set_partitions(np.array(TABLES[n], dtype=np.uint64))
    assert ctx.pq_search_partitions(q, 10, np.array([[2, 3, 5]] * 19, dtype=np.uint32))[2].tolist() == [0] * 19   # every table of m = 1 holds NaN
    ctx.close()


def test_state_arguments_and_index():
    c = case(F16, 96, 48, 5000, True)
    ctx, A, cb, q, dim, M = c["ctx"], c["A"], c["cb"], c["queries"], 96, 48

    def invalid(fn, word):
        with pytest.raises(nvdb_amd.NvdbError) as e:
            fn()
        assert e.value.status == 1 and word in str(e.value), str(e.value)

    lib, out = ctx.lib, np.zeros((2, dim), dtype=np.float32)
    assert lib.nvdb_hip_pq_build_opq(ctx.h, None, cb.ctypes.data, M, 1) == 1 and b"null rotation" in lib.nvdb_hip_last_error(ctx.h)
    assert lib.nvdb_hip_pq_train_opq(ctx.h, None, M, 1, 1, 0, None, cb.ctypes.data, None, 1) == 1 and lib.nvdb_hip_pq_rotate(ctx.h, None, 2, out.ctypes.data) == 1
    invalid(lambda: ctx.pq_build(np.zeros((6, 256, 16), np.float32), rotation=A), "M must be")
    invalid(lambda: ctx.pq_train(6, 1, SEED, rotation=A), "M must be")
    invalid(lambda: ctx.pq_rotated_rows(4990, 11), "row0 + nrows > n")
    assert ctx.pq_rotated_rows(5000, 0).shape == (0, dim) and ctx.pq_rotate(q[:0]).shape == (0, dim)
    assert np.array_equal(bits(ctx.pq_rotation()), bits(A)) and np.array_equal(ctx.pq_download_codes(), c["codes"])   # failed builds: the shadow stands
    ix = nvdb_amd.IvfIndex(ctx, c["cents"])                              # the index form: the context-level call mapped through the permutation
    cbi = ix.pq_train(M, 1, SEED, rotation=A, residual=True)
    ix.pq_build(cbi, residual=True, rotation=A)
    assert np.array_equal(bits(ix.pq_rotation()), bits(A)) and np.array_equal(bits(ix.pq_rotate(q)), bits(ctx.pq_rotate(q)))
    assert np.array_equal(bits(ix.pq_rotated_rows(7, 3)), bits(ix.ctx.pq_rotated_rows(7, 3)))
    perm = ix.info()["perm"].astype(np.uint64)
    pid, iid = ix.ctx.pq_search_ivf(q, 100, 3)[0], ix.pq_search(q, 100, 3)[0]
    assert np.array_equal(iid, np.where(pid == U64MAX, U64MAX, np.uint64(ROW_BASE) + perm[np.minimum(pid, 4999)]))
    rid, rdist = ix.ctx.pq_refine_ivf(q, 10, 100, 3)
    fi, fd = ix.pq_refine(q, 10, 100, 3)
    assert (rid != U64MAX).any() and np.array_equal(fi, np.where(rid == U64MAX, U64MAX, np.uint64(ROW_BASE) + perm[np.minimum(rid, 4999)]))
    assert np.array_equal(bits(fd), bits(rdist))
    ix.close()
    plain = nvdb_amd.HipContext(0)                                       # a later build without a rotation holds none
    plain.upload_corpus(c["E"], F32, None, 0)
    invalid(lambda: plain.pq_rotate(q), "nvdb_hip_pq_build")
    plain.pq_build(cb, rotation=A)
    assert plain.pq_rotation() is not None
    plain.pq_build(cb)
    assert plain.pq_rotation() is None
    invalid(lambda: plain.pq_rotated_rows(0, 1), "no rotation")
    invalid(lambda: plain.pq_rotate(q), "no rotation")
    plain.close()
