"""PQ codebook training on the device (nvdb_hip_pq_train, the index form) against plain numpy fp64 of the header's definitions.
Fixture: 5000 rows -- one full 4096-row chunk plus a partial one whose last 256-row tile is partial.  make_codebooks is
test_gpu_pq.py's recipe: sampled row sub-vectors plus noise, codewords 3 and 7 of sub-quantiser 0 bit-identical (7 never wins)."""
import numpy as np
import pytest

import nvdb_amd

pytestmark = pytest.mark.gpu

N, ROW_BASE, SEED = 5000, 1_000_003, 20261126
F32, F16, I8 = nvdb_amd.DT_F32, nvdb_amd.DT_F16, nvdb_amd.DT_I8
EPS = 2.0 ** -24
# dsub 8; 5 (padded to 8, rows no multiple of 16 bytes); 2; 1; 32 (the widest build); the other dtypes
CASES = [(F16, 32, 4), (F16, 60, 12), (F16, 96, 48), (F16, 128, 128), (F16, 128, 4), (F32, 64, 16), (I8, 64, 16)]
_cache = {}


def rows_f32(base, scales, dtype):
    if dtype == I8:
        return base.astype(np.float32) * scales[:, None].astype(np.float32)
    return base.view(np.float16).astype(np.float32) if dtype == F16 else base


def make_codebooks(X, M, seed=5):
    rs = np.random.RandomState(seed)
    dsub = X.shape[1] // M
    sub = X.reshape(len(X), M, dsub)
    cb = np.stack([sub[rs.choice(len(X), 256, replace=False), m] for m in range(M)])
    cb = (cb + 0.01 * rs.standard_normal(cb.shape)).astype(np.float32)
    cb[0, 7] = cb[0, 3]
    return cb


def case(dtype, dim, M):
    key = (dtype, dim, M)
    if key not in _cache:
        base, scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
        ctx = nvdb_amd.HipContext(0)
        ctx.upload_corpus(base, dtype, scales, ROW_BASE)
        X = rows_f32(base, scales, dtype)
        _cache[key] = dict(ctx=ctx, X=X, init=make_codebooks(X, M), base=base, scales=scales)
    return _cache[key]


def min_d64(X, cb):
    """[rows, M] fp64: the least squared distance of every sub-vector to its sub-quantiser's codewords."""
    M, _, dsub = cb.shape
    sub = X.astype(np.float64).reshape(len(X), M, dsub)
    out = np.empty((len(X), M))
    for m in range(M):
        d = np.zeros((len(X), 256))
        for t in range(dsub):
            d += (sub[:, m, t, None] - cb[m, None, :, t].astype(np.float64)) ** 2
        out[:, m] = d.min(1)
    return out


def as_bytes(a):                                                         # [rows, dsub] f32 -> one item per row, compared byte for byte
    return np.ascontiguousarray(a).view(np.dtype((np.void, a.shape[1] * 4))).ravel()


@pytest.mark.parametrize("max_train_rows", [0, 1000])
@pytest.mark.parametrize("dtype,dim,M", CASES)
def test_start(dtype, dim, M, max_train_rows):
    c = case(dtype, dim, M)
    dsub = dim // M
    T = c["X"] if not max_train_rows else c["X"][np.arange(max_train_rows) * N // max_train_rows]
    cb = c["ctx"].pq_train(M, 0, SEED, max_train_rows)
    assert np.array_equal(cb.view(np.uint32), c["ctx"].pq_train(M, 0, SEED, max_train_rows).view(np.uint32))
    picked = []
    for m in range(M):
        rows, first, have = np.unique(as_bytes(T[:, m * dsub:(m + 1) * dsub]), return_index=True, return_counts=True)
        cws, want = np.unique(as_bytes(cb[m]), return_counts=True)
        at = np.searchsorted(rows, cws)
        assert (at < len(rows)).all() and (rows[np.minimum(at, len(rows) - 1)] == cws).all(), m      # every codeword is a training row's sub-vector
        assert (want <= have[at]).all(), m                                                           # ... of 256 distinct rows
        picked.append(set(first[at].tolist()) if len(rows) == len(T) else None)                     # (the rows, where bytes identify them)
    assert dsub < 4 or all(p is not None and len(p) == 256 for p in picked)
    assert all(a is None or b is None or a != b for a, b in zip(picked, picked[1:]))


@pytest.mark.parametrize("dtype,dim,M", CASES)
def test_one_step(dtype, dim, M):
    c = case(dtype, dim, M)
    ctx, X, init, dsub = c["ctx"], c["X"], c["init"], dim // M
    ctx.pq_build(init)
    codes = ctx.pq_download_codes()
    got, err = ctx.pq_train(M, 1, SEED, init=init, want_err=True)
    sub = X.astype(np.float64).reshape(N, M, dsub)
    for m in range(M):
        count = np.bincount(codes[:, m], minlength=256)
        live = count > 0
        s = np.stack([np.bincount(codes[:, m], weights=sub[:, m, t], minlength=256) for t in range(dsub)], 1)
        sabs = np.stack([np.bincount(codes[:, m], weights=np.abs(sub[:, m, t]), minlength=256) for t in range(dsub)], 1)
        ref = (s[live] / count[live, None]).astype(np.float32)
        tol = np.spacing(np.abs(ref)).astype(np.float64) + 2.0 ** -52 * sabs[live]                  # one f32 ulp + count * 2^-52 * mean|x|
        assert (np.abs(got[m][live].astype(np.float64) - ref) <= tol).all(), m
        assert np.array_equal(got[m][~live].view(np.uint32), init[m][~live].view(np.uint32)), m      # no members: the bits stay
        assert m != 0 or (count[7] == 0 and count[3] > 0)
    want = min_d64(X, init).mean()
    print(f"out_err[0] / fp64 - 1 = {err[0] / want - 1:.3e} (bound {2 * (dsub + 3) * EPS:.3e})")
    assert abs(err[0] - want) <= 2 * (dsub + 3) * EPS * want


@pytest.mark.parametrize("dtype,dim,M", CASES)
def test_descent(dtype, dim, M):
    c = case(dtype, dim, M)
    dsub = dim // M
    bound = (dsub + 3) * EPS
    runs = [c["ctx"].pq_train(M, k, SEED, want_err=True) for k in range(5)]
    E = [min_d64(c["X"], cb).mean() for cb, _ in runs]
    print("E_0..E_4 =", " ".join(f"{e:.6e}" for e in E))
    for k in range(4):
        assert E[k + 1] <= E[k] * (1 + 4 * bound), k
        assert abs(runs[4][1][k] - E[k]) <= 2 * bound * E[k], k
    assert E[4] < E[0]


@pytest.mark.parametrize("dtype,dim,M", CASES)
def test_non_finite(dtype, dim, M):
    c = case(dtype, dim, M)
    base, scales = c["base"].copy(), None if c["scales"] is None else c["scales"].copy()
    (scales if dtype == I8 else base)[17] = 0x7E00 if dtype == F16 else np.nan                     # one NaN training row
    init = c["init"].copy()
    init[1, 9] = np.inf
    ctx = nvdb_amd.HipContext(0)
    ctx.upload_corpus(base, dtype, scales, ROW_BASE)
    got, err = ctx.pq_train(M, 2, SEED, init=init, want_err=True)
    ctx.close()
    assert np.array_equal(got[1, 9].view(np.uint32), init[1, 9].view(np.uint32))
    for m in range(M):
        assert np.array_equal(got[m, 0].view(np.uint32), init[m, 0].view(np.uint32)) or np.isfinite(got[m, 0]).all(), m
    rest = np.ones(got.shape[:2], bool)
    rest[1, 9] = False
    assert np.isfinite(got[rest]).all() and np.isfinite(err).all()


def test_index_form():
    dtype, dim, M = F16, 64, 16
    base, _ = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
    src = nvdb_amd.HipContext(0)
    src.upload_corpus(base, dtype, None, ROW_BASE)
    ix = nvdb_amd.IvfIndex(src, nvdb_amd.synth_rows_f32(SEED + 2, 0, 6, dim))
    flat = nvdb_amd.HipContext(0)
    flat.upload_corpus(np.ascontiguousarray(base[ix.info()["perm"]]), dtype, None, 0)
    cb, err = ix.pq_train(M, 2, SEED, 1000, want_err=True)
    want, want_err = flat.pq_train(M, 2, SEED, 1000, want_err=True)
    assert np.array_equal(cb.view(np.uint32), want.view(np.uint32)) and np.array_equal(err, want_err)
    ix.pq_build(cb)
    assert ix.ctx.pq_info()["M"] == M
    ix.close()


def test_arguments():
    ctx = nvdb_amd.HipContext(0)
    out = np.full((4, 256, 64), 7.0, dtype=np.float32)

    def train(M, out_p, rows=0):
        return ctx.lib.nvdb_hip_pq_train(ctx.h, M, 1, SEED, rows, None, out_p, None)

    assert train(4, out.ctypes.data) == 4                                # no corpus
    base, _ = nvdb_amd.synth_corpus(SEED, 0, 300, 256, F16)
    ctx.upload_corpus(base, F16, None, 0)
    assert train(4, None) == 1                                           # null output
    assert train(8, out.ctypes.data, 255) == 1                           # fewer than 256 training rows
    assert train(4, out.ctypes.data) == 3                                # dsub 64
    for bad_m in (0, 6, 132, 24):                                        # (256 % 24 != 0)
        assert train(bad_m, out.ctypes.data) == 1
    assert (out == 7.0).all()
    assert ctx.pq_train(8, 1, SEED).shape == (8, 256, 32) and ctx.pq_info()["M"] == 0
    ctx.close()
