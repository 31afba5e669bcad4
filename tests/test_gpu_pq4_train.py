"""The 16-codeword PQ trainer (nvdb_hip_pq4_train, the index form) against plain numpy fp64 of the header's definitions: the codes
are nvdb_hip_pq4_build's under the same codebooks, the update np.bincount (which adds in array order) per 4096-row chunk.  Fixture:
test_gpu_pq_train.py's 5000 rows and test_gpu_pq4.py's codebooks (codewords 3 and 7 of sub-quantiser 0 bit-identical)."""
import numpy as np
import pytest

import nvdb_amd
from test_gpu_pq_train import N, ROW_BASE, SEED, F32, F16, I8, EPS, rows_f32, as_bytes
from test_gpu_pq4 import make_codebooks, unpack

pytestmark = pytest.mark.gpu

# dsub 8 (SQ 8, one group); two groups; dsub 5 padded to 8; dsub 2; dsub 16 (SQ 4); dsub 32 (SQ 2); dsub 4
CASES = [(F16, 64, 8), (F16, 128, 16), (F16, 40, 8), (F16, 16, 8), (F16, 256, 16), (F32, 256, 8), (I8, 64, 16)]
_cache = {}
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def case(dtype, dim, M):
    if (dtype, dim, M) not in _cache:
        base, scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
        ctx = nvdb_amd.HipContext(0)
        ctx.upload_corpus(base, dtype, scales, ROW_BASE)
        X = rows_f32(base, scales, dtype)
        _cache[(dtype, dim, M)] = dict(ctx=ctx, X=X, init=make_codebooks(X, M), base=base, scales=scales)
    return _cache[(dtype, dim, M)]


def lloyd_step(E, codes, init):
    """The header's update over the rows E the encode saw, and whether each codeword moves (members and a finite sum)."""
    M, _, dsub = init.shape
    sub, want, moves = E.astype(np.float64).reshape(len(E), M, dsub), init.copy(), np.zeros((M, 16), bool)
    for m in range(M):
        chunks = [slice(lo, lo + 4096) for lo in range(0, len(E), 4096)]
        s = sum(np.stack([np.bincount(codes[c, m], weights=sub[c, m, t], minlength=16) for t in range(dsub)], 1) for c in chunks)
        count = np.bincount(codes[:, m], minlength=16)
        moves[m] = (count > 0) & np.isfinite(s).all(1)
        want[m][moves[m]] = (s[moves[m]] / count[moves[m], None]).astype(np.float32)
    return want, moves


def mean_min_d64(E, cb):
    sub = E.astype(np.float64).reshape(len(E), cb.shape[0], 1, cb.shape[2])
    return np.mean([((sub[:, m] - cb[m].astype(np.float64)[None]) ** 2).sum(-1).min(1).mean() for m in range(cb.shape[0])])


@pytest.mark.parametrize("dtype,dim,M", CASES)
def test_one_step(dtype, dim, M):
    c = case(dtype, dim, M)
    ctx, init, dsub = c["ctx"], c["init"], dim // M
    ctx.pq_build(init)                                                   # the reference assignment: the build's own codes
    codes = unpack(ctx.pq_download_codes())
    got, err = ctx.pq_train(M, 1, SEED, init=init, bits=4, want_err=True)
    want, moves = lloyd_step(c["X"], codes, init)
    assert got.shape == (M, 16, dsub) and np.array_equal(bits(got), bits(want))
    assert moves[0, 3] and not moves[0, 7] and moves.sum() > 8 * M       # the duplicated codeword has no members
    E0 = mean_min_d64(c["X"], init)
    print(f"out_err[0] / fp64 - 1 = {err[0] / E0 - 1:.3e} (bound {2 * (dsub + 3) * EPS:.3e})")
    assert abs(err[0] - E0) <= 2 * (dsub + 3) * EPS * E0


@pytest.mark.parametrize("dtype,dim,M", CASES)
def test_start_determinism_and_descent(dtype, dim, M):
    c = case(dtype, dim, M)
    ctx, dsub = c["ctx"], dim // M
    for max_train_rows in (0, 1000):
        T = c["X"] if not max_train_rows else c["X"][np.arange(max_train_rows) * N // max_train_rows]
        cb = ctx.pq_train(M, 0, SEED, max_train_rows, bits=4)
        for m in range(M):                                               # every codeword a training row's sub-vector, of 16 distinct rows
            rows, have = np.unique(as_bytes(T[:, m * dsub:(m + 1) * dsub]), return_counts=True)
            cws, want = np.unique(as_bytes(cb[m]), return_counts=True)
            at = np.minimum(np.searchsorted(rows, cws), len(rows) - 1)
            assert want.sum() == 16 and (rows[at] == cws).all() and (want <= have[at]).all(), m
    a, b = ctx.pq_train(M, 3, SEED, bits=4, want_err=True), ctx.pq_train(M, 3, SEED, bits=4, want_err=True)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    err = ctx.pq_train(M, 4, SEED, bits=4, want_err=True)[1]
    print("out_err =", " ".join(f"{e:.6e}" for e in err))
    assert (err[1:] <= err[:-1] * (1 + (dsub + 3) * EPS)).all() and err[3] < err[0]


@pytest.mark.parametrize("residual,rotated", [(True, False), (False, True), (True, True)])
def test_kinds_on_an_index(residual, rotated):
    dtype, dim, M = F16, 64, 8
    c = case(dtype, dim, M)
    cents = nvdb_amd.synth_rows_f32(SEED + 2, 0, 6, dim)
    ix = nvdb_amd.IvfIndex(c["ctx"], cents)
    A = np.linalg.qr(np.random.RandomState(dim).standard_normal((dim, dim)))[0].astype(np.float32) if rotated else None
    ix.pq_build(c["init"], residual=residual, rotation=A)
    codes, info = unpack(ix.ctx.pq_download_codes()), ix.info()
    list_of = np.searchsorted(info["offsets"], np.arange(N), side="right") - 1
    E = ix.pq_rotated_rows() if rotated else c["X"][info["perm"]] - cents[list_of]
    got = ix.pq_train(M, 1, SEED, init=c["init"], bits=4, residual=residual, rotation=A)
    ix.close()
    assert np.array_equal(bits(got), bits(lloyd_step(E, codes, c["init"])[0]))


@pytest.mark.parametrize("dtype,dim,M", [(F16, 64, 8), (F32, 256, 8)])
def test_non_finite_rows(dtype, dim, M):
    c = case(dtype, dim, M)
    base = c["base"].copy()
    base[17] = 0x7E00 if dtype == F16 else np.nan                        # a row without a winner anywhere
    base[4500, 5] = 0x7C00 if dtype == F16 else np.inf                   # ... and one in sub-quantiser 0 only
    ctx = nvdb_amd.HipContext(0)
    ctx.upload_corpus(base, dtype, None, ROW_BASE)
    ctx.pq_build(c["init"])
    codes = unpack(ctx.pq_download_codes())
    got = ctx.pq_train(M, 1, SEED, init=c["init"], bits=4)
    ctx.close()
    want, moves = lloyd_step(rows_f32(base, None, dtype), codes, c["init"])
    assert (codes[17] == 0).all() and codes[4500, 0] == 0 and not moves[:, 0].any() and moves[:, 1:].sum() > 8 * M
    assert np.array_equal(bits(got), bits(want))


def test_arguments():
    ctx, out = case(F16, 64, 8)["ctx"], np.full((8, 16, 64), 7.0, dtype=np.float32)
    wide = nvdb_amd.HipContext(0)                                        # dim / M = 64: valid arguments, no such build
    wide.generate_corpus(SEED, 100, 512, F16)
    train = lambda cx, M, rows=0, residual=0: cx.lib.nvdb_hip_pq4_train(cx.h, None, M, 1, SEED, rows, None, out.ctypes.data, None, residual)
    assert train(ctx, 12) == 1 and train(wide, 8) == 3 and train(ctx, 8, rows=10) == 1 and train(ctx, 8, residual=1) == 1
    wide.close()
    assert (out == 7.0).all()
    with pytest.raises(ValueError):
        ctx.pq_train(8, 1, SEED, bits=5)
