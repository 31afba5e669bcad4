"""4-bit PQ shadows (nvdb_hip_pq4_build / nvdb_hip_pq_bits and every PQ call over such a shadow) against plain numpy fp64 of the
header's definitions.  Fixture: test_gpu_pq.py's -- 5000 rows, partitions [0, 0, 37, 101, 2300, 4990, 5000] (an empty list, one
shorter than a tile, starts off the 64-row grid, 2690 rows in two segments, a 10-row tail); codebooks: 16 sampled row sub-vectors
plus small noise, codewords 3 and 7 of sub-quantiser 0 bit-identical.  Kinds: plain, residual, residual under a random orthonormal
rotation (the rotated rows and queries are the GPU's own bits, as in test_gpu_pq_opq.py).  Tolerances: test_gpu_pq.py's and, for
residual kinds, test_gpu_pq_residual.py's 1.01 eps ((ceil(dim / 64) + 7) sum |q c| + (dsub + M + 1) sum A)."""
import numpy as np
import pytest

import nvdb_amd
from test_gpu_pq import N, ROW_BASE, SEED, OFFSETS, U64MAX, F32, F16, I8, EPS, rows_f32, probe_table, union_rows
from test_gpu_pq_residual import NPARTS, LIST_OF

pytestmark = pytest.mark.gpu

NQ = 2 * 32 + 3                                                          # two full groups and a partial one at the largest G (32)
CASES = [(F16, 32, 8),     # (dtype, dim, M): G = 32, a 4-byte row
         (F16, 48, 24),    # 32, 12 bytes: dwords only; dsub 2
         (F16, 64, 32),    # 32, one 16-byte piece
         (F16, 96, 48),    # 16 (the group size the issue's table leaves out), dwords
         (F16, 96, 96),    # 8, three pieces; dsub 1
         (F16, 256, 256),  # 8, M at its maximum
         (F16, 256, 8),    # 32, dsub 32: the widest encode
         (F32, 64, 32), (I8, 64, 32)]
ALL_KINDS = [(F16, 64, 32), (F16, 96, 48)]
CASE_KINDS = [c + (k,) for c in CASES for k in (("plain", "resid", "rot") if c in ALL_KINDS else ("plain",))]
_cache = {}
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def make_codebooks(X, M, seed=5):
    rs = np.random.RandomState(seed)
    sub = X.reshape(len(X), M, X.shape[1] // M)
    cb = np.stack([sub[rs.choice(len(X), 16, replace=False), m] for m in range(M)])
    cb = (cb + 0.01 * rs.standard_normal(cb.shape)).astype(np.float32)
    cb[0, 7] = cb[0, 3]
    return cb


def new_ctx(c, cents):
    ctx = nvdb_amd.HipContext(0)
    ctx.upload_corpus(c["base"], c["dtype"], c["scales"], ROW_BASE)
    ctx.set_partitions(OFFSETS)
    ctx.set_centroids(cents)
    return ctx


def unpack(packed):
    return np.stack([packed & 15, packed >> 4], axis=2).reshape(len(packed), -1)


def case(dtype, dim, M, kind):
    """One corpus with its shadow, built once; E: what the encode sees (the row, its residual, or the GPU's rotated residual)."""
    key = (dtype, dim, M, kind)
    if key not in _cache:
        base, scales = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
        c = dict(base=base, scales=scales, dtype=dtype, X=rows_f32(base, scales, dtype), A=None)
        cents = np.ones((NPARTS, dim), dtype=np.float32)
        for p in range(NPARTS):
            if OFFSETS[p + 1] > OFFSETS[p]:
                cents[p] = c["X"][int(OFFSETS[p]):int(OFFSETS[p + 1])].mean(0, dtype=np.float32)
        c.update(cents=cents, ctx=new_ctx(c, cents), queries=nvdb_amd.synth_rows_f32(SEED + 1, 0, NQ, dim))
        E = c["X"] if kind == "plain" else c["X"] - cents[LIST_OF]
        if kind == "rot":
            c["A"] = np.linalg.qr(np.random.RandomState(dim).standard_normal((dim, dim)))[0].astype(np.float32)
            E = (E.astype(np.float64) @ c["A"].astype(np.float64).T).astype(np.float32)      # (for the codebooks' sampling only)
        c["cb"] = make_codebooks(E, M)
        c["ctx"].pq_build(c["cb"], residual=kind != "plain", rotation=c["A"])
        c["E"] = c["ctx"].pq_rotated_rows() if kind == "rot" else E
        c.update(packed=c["ctx"].pq_download_codes(), codes=unpack(c["ctx"].pq_download_codes()))
        _cache[key] = c
    return _cache[key]


@pytest.mark.parametrize("dtype,dim,M,kind", CASE_KINDS)
def test_encode_and_reconstruct(dtype, dim, M, kind):
    c = case(dtype, dim, M, kind)
    dsub, codes, ctx = dim // M, c["codes"], c["ctx"]
    assert ctx.pq_info() == dict(M=M, dsub=dsub, code_bytes=N * M // 2) and ctx.pq_bits() == 4
    assert ctx.pq_kind() == dict(residual=kind != "plain") and (ctx.pq_rotation() is None) == (kind != "rot") and c["packed"].shape == (N, M // 2)
    sub = c["E"].astype(np.float64).reshape(N, M, dsub)
    for m in range(M):
        d64 = ((sub[:, m, None, :] - c["cb"][m].astype(np.float64)[None]) ** 2).sum(-1)              # [N, 16]
        got = d64[np.arange(N), codes[:, m]]
        print(f"m={m} worst d(code) / min d = 1 + {(got / np.maximum(d64.min(1), 1e-300)).max() - 1:.3e}  (bound {2 * (dsub + 3) * EPS:.3e})")
        assert (got <= d64.min(1) * (1 + 2 * (dsub + 3) * EPS)).all(), m
    assert (codes[:, 0] == 3).any() and not (codes[:, 0] == 7).any()                                # the duplicated pair: the lower index
    cw = c["cb"][np.arange(M), codes].reshape(N, dim)                                                # the codewords side by side
    if kind != "rot":                                                                                # (the transpose product: test_gpu_pq_opq.py)
        want = cw if kind == "plain" else c["cents"][LIST_OF] + cw
        assert np.array_equal(bits(ctx.pq_reconstruct()), bits(want)) and np.array_equal(bits(ctx.pq_reconstruct(36, 66)), bits(want[36:102]))


@pytest.mark.parametrize("R", [1, 100, 3000])
@pytest.mark.parametrize("nq", [1, NQ])
@pytest.mark.parametrize("dtype,dim,M,kind", CASE_KINDS)
def test_scores_and_membership(dtype, dim, M, kind, nq, R):
    c = case(dtype, dim, M, kind)
    dsub, codes, ctx = dim // M, c["codes"], c["ctx"]
    queries, probe, resid = c["queries"][:nq], probe_table(nq), kind != "plain"
    ids, scores, counts = ctx.pq_search_partitions(queries, R, probe)
    assert ctx.stats()["path"] == 9
    qtab = ctx.pq_rotate(queries) if kind == "rot" else queries                                      # what the tables are made of
    marange = np.arange(M)
    for q in range(nq):
        prod = qtab[q].astype(np.float64).reshape(M, 1, dsub) * c["cb"].astype(np.float64)            # [M, 16, dsub]
        L64, A64 = prod.sum(-1), np.abs(prod).sum(-1)
        qc = queries[q].astype(np.float64)[None] * c["cents"].astype(np.float64) * resid             # [NPARTS, dim]; plain: zeros
        rows = union_rows(probe[q])
        s64 = qc.sum(1)[LIST_OF[rows]] + L64[marange, codes[rows]].sum(1)
        tol = 1.01 * EPS * (resid * (-(-dim // 64) + 7) * np.abs(qc).sum(1)[LIST_OF[rows]] + (dsub + M + resid) * A64[marange, codes[rows]].sum(1)).max()
        cnt = min(R, len(rows))
        assert counts[q] == cnt and (ids[q, cnt:] == U64MAX).all() and np.isneginf(scores[q, cnt:]).all()
        local = (ids[q, :cnt] - np.uint64(ROW_BASE)).astype(np.int64)
        assert np.isin(local, rows).all() and len(set(local)) == cnt
        pos = np.searchsorted(rows, local)
        err = np.abs(scores[q, :cnt].astype(np.float64) - s64[pos]).max()
        print(f"q={q} max |score - s64| = {err:.3e} (tol {tol:.3e})")
        assert err <= tol
        rest = np.delete(s64, pos)
        assert not rest.size or s64[pos].min() >= rest.max() - 2 * tol
        assert (np.lexsort((local, -scores[q, :cnt])) == np.arange(cnt)).all()                         # score descending, id ascending


@pytest.mark.parametrize("dtype,dim,M", ALL_KINDS)
def test_zero_centroids_and_identity_rotation_repeat_the_plain_shadow(dtype, dim, M):
    c = case(dtype, dim, M, "plain")
    ctx, probe, got = new_ctx(c, np.zeros((NPARTS, dim), dtype=np.float32)), probe_table(NQ), []
    for residual, rotation in ((False, None), (True, None), (False, np.eye(dim, dtype=np.float32))):
        ctx.pq_build(c["cb"], residual=residual, rotation=rotation)
        assert ctx.pq_bits() == 4 and ctx.pq_kind()["residual"] == residual
        got.append((ctx.pq_download_codes(),) + tuple(x for R in (100, N) for x in ctx.pq_search_partitions(c["queries"], R, probe)))
    assert np.array_equal(got[0][0], c["packed"]) and np.array_equal(got[2][0], got[0][0])            # identity rotation: the same codes
    for a, b in zip(got[0], got[1]):                                                                  # zero centroids: ids and score bits
        assert np.array_equal(a, b)
    ctx.close()


def test_fused_refine_equals_its_halves():
    dtype, dim, M = F16, 64, 32
    c = case(dtype, dim, M, "resid")
    ctx, queries, K, R, nprobe = c["ctx"], c["queries"], 10, 100, 3

    def halves(cx, row_base):
        ids, _, _ = cx.pq_search_ivf(queries, R, nprobe)
        cand = np.where(ids == U64MAX, np.uint64(0xFFFFFFFF), ids - np.uint64(row_base)).astype(np.uint32)
        return cx.refine_l2_topk(queries, cand, K)

    rid, rdist = halves(ctx, ROW_BASE)
    fi, fd = ctx.pq_refine_ivf(queries, K, R, nprobe)
    assert (rid != 0xFFFFFFFF).any()
    assert np.array_equal(fi, np.where(rid == 0xFFFFFFFF, U64MAX, rid.astype(np.uint64) + np.uint64(ROW_BASE)))
    assert np.array_equal(bits(fd), bits(rdist))
    ix = nvdb_amd.IvfIndex(ctx, c["cents"])                                # the index form: its own lists, the source corpus' ids
    ix.pq_build(c["cb"], residual=True)
    assert ix.pq_bits() == 4 and ix.ctx.pq_info()["code_bytes"] == N * M // 2
    perm = ix.info()["perm"].astype(np.uint64)
    rid, rdist = halves(ix.ctx, 0)
    fi, fd = ix.pq_refine(queries, K, R, nprobe)
    assert np.array_equal(fi, np.where(rid == 0xFFFFFFFF, U64MAX, np.uint64(ROW_BASE) + perm[np.minimum(rid, N - 1)]))
    assert np.array_equal(bits(fd), bits(rdist))
    ix.close()


def test_lifecycle():
    dtype, dim = F16, 64
    base, _ = nvdb_amd.synth_corpus(SEED, ROW_BASE, N, dim, dtype)
    X = rows_f32(base, None, dtype)
    cb4, cb8 = make_codebooks(X, 8), np.ascontiguousarray(X[:256].reshape(256, 4, 16).transpose(1, 0, 2))
    q, probe = nvdb_amd.synth_rows_f32(SEED + 1, 0, 2, dim), probe_table(1).repeat(2, 0)
    ctx = nvdb_amd.HipContext(0)
    ctx.upload_corpus(base, dtype, None, ROW_BASE)
    ctx.set_partitions(OFFSETS)
    assert ctx.pq_bits() == 0
    ctx.pq_build(cb4)
    codes = ctx.pq_download_codes()
    for bad_m in (4, 12, 264):                                          # rejected with the standing shadow unchanged
        with pytest.raises(nvdb_amd.NvdbError) as e:
            ctx.pq_build(np.zeros((bad_m, 16, max(1, dim // bad_m)), np.float32))
        assert e.value.status == 1
        assert ctx.pq_bits() == 4 and np.array_equal(ctx.pq_download_codes(), codes)
    with pytest.raises(ValueError):
        ctx.pq_build(np.zeros((8, 32, 8), np.float32))
    wide = nvdb_amd.HipContext(0)                                       # dim / M = 64: valid arguments, no such build
    wide.generate_corpus(SEED, 100, 512, F16)
    with pytest.raises(nvdb_amd.NvdbError) as e:
        wide.pq_build(np.zeros((8, 16, 64), np.float32))
    assert e.value.status == 3 and "dim / M" in str(e.value) and wide.pq_bits() == 0
    wide.close()
    ctx.pq_build(cb8)                                                   # an 8-bit build replaces a 4-bit one and back
    assert ctx.pq_bits() == 8 and ctx.pq_info() == dict(M=4, dsub=16, code_bytes=N * 4) and ctx.pq_download_codes().shape == (N, 4)
    assert ctx.pq_search_partitions(q, 10, probe)[2].tolist() == [10, 10]
    ctx.pq_build(cb4)
    assert ctx.pq_bits() == 4 and np.array_equal(ctx.pq_download_codes(), codes)
    assert ctx.pq_search_partitions(q, 10, probe)[2].tolist() == [10, 10]
    ctx.insert_rows(base[:1], part_of=[5])
    assert ctx.pq_bits() == 0 and ctx.pq_info() == dict(M=0, dsub=0, code_bytes=0)
    ctx.close()
