"""The adversarial filter-bound cases (tests/filter_bound_cases.py), checked without a GPU and without the library: the planted
neighbourhood is ranked strictly, the victim is the exact k-th best and holds the largest norm, and the share of the granted band
that the numpy model of the filter reaches is the derived one.  The GPU module (tests/test_gpu_filter_bound.py) imports these
shares for its shrunk-bound runs; none of them comes from a GPU run."""
import numpy as np
import pytest

import filter_bound_cases as fb

IDS = [f"{f}-{d}" for f, d in fb.CASES]


@pytest.fixture(scope="module", params=fb.CASES, ids=IDS)
def case(request):
    fam, dim = request.param
    yield fb.build(fam, dim)
    fb.drop(fam, dim)                                          # (123 MB at d = 1536: one case resident at a time)


def test_planted_neighbourhood_is_strictly_ranked_and_the_victim_is_kth(case):
    order, ex = case.order, case.exact
    best = order[:fb.K + 9]
    assert set(best) <= set(range(fb.N_PLANTED)), "a filler row reached the planted neighbourhood"
    assert np.all(np.diff(ex[best]) < 0), "equal scores among the best k + 9"
    assert order[fb.K - 1] == fb.VICTIM and set(order[:fb.K - 1]) == set(fb.TOPS)
    assert np.array_equal(case.expected, order[:fb.K])
    assert np.all(ex[fb.DECOYS] < ex[fb.VICTIM])
    # every decoy is closer to the victim than the victim's own filter error (I8LO: than the band)
    room = case.err_victim if case.family != "I8LO" else 2.0 * case.E
    assert np.all(ex[fb.VICTIM] - ex[fb.DECOYS] < room)
    # fillers: far below -- at least ten bounds under the victim
    assert np.max(ex[fb.N_PLANTED:]) < ex[fb.VICTIM] - 10.0 * case.E


def test_victim_holds_the_largest_norm_alone(case):
    assert np.all(case.norms <= case.norms[fb.VICTIM])
    assert np.sum(case.norms == case.norms[fb.VICTIM]) == 1
    if case.family == "SH8":
        assert np.argmax(case.resid) == fb.VICTIM and np.sum(case.resid == case.resid[fb.VICTIM]) == 1
        assert np.max(case.resid[fb.N_PLANTED:]) < 0.9 * case.resid[fb.VICTIM]


def test_model_filter_is_on_the_planned_side(case):
    mf, ex = case.model_filter, case.exact
    if case.family == "I8LO":                                  # the query is its own quantisation: the filter is exact
        assert np.allclose(mf, ex[:fb.N_PLANTED], rtol=1e-12, atol=0)
        b = case.budget
        assert b["victim_hi_part"] == 0.0
        assert b["lo_plane"] == pytest.approx(b["lo_plane_allowance"] / 1.0001 ** 2, rel=1e-6), "not Cauchy-Schwarz equality"
        return
    assert mf[fb.VICTIM] < ex[fb.VICTIM]
    assert np.all(mf[fb.DECOYS] > ex[fb.DECOYS])
    assert np.all(mf[fb.DECOYS] > mf[fb.VICTIM]), "the victim is not behind every decoy in filter order"
    assert np.all(mf[fb.TOPS] > np.max(mf[fb.DECOYS])), "tau would not be a decoy's filter value"
    # nothing planted breaks the bound itself
    assert np.all(np.abs(mf - ex[:fb.N_PLANTED]) < case.E)


def test_reached_share_of_the_band(case):
    want = fb.DERIVED[case.family]
    for share in (case.share_topk, case.share_range):
        assert want * (1.0 - fb.SLACK) <= share < 1.0, (case.family, case.dim, share, want)
    if case.family == "I8LO":
        assert case.share_topk <= want + 1e-3 and case.share_range > case.share_topk
    else:
        assert max(case.share_topk, case.share_range) <= want
    pct = fb.bound_pct(case.family, case.dim)
    assert 1 <= pct < 100 * case.share_topk
    # the shrunk bound must lose the victim in the model: the band under the best decoy no longer reaches it
    if case.family == "I8LO":
        bar = case.model_filter[fb.VICTIM] - 2.0 * case.E * pct / 100.0
        assert case.budget["victim_hi_part"] < bar - case.qdelta * pct / 100.0
    else:
        assert case.model_filter[fb.VICTIM] < case.model_filter[case.best_decoy] - 2.0 * case.E * pct / 100.0
        assert case.err_victim > case.E * pct / 100.0


def test_oracle_orders_the_planted_rows_as_fp64_does(case, oracle):
    """The reference's fp32 chains must not flip the planted order, or the GPU module's expectation would differ from the builder's."""
    import pyoracle as po
    dt = {"f16": po.DT_F16, "f32": po.DT_F32, "i8": po.DT_I8}[case.dtype]
    rows = case.rows[:fb.N_PLANTED]
    rows = rows.view(np.uint16) if case.dtype == "f16" else rows
    sc = oracle.scores(rows, dt, case.query, case.scales[:fb.N_PLANTED] if case.scales is not None else None)
    order32 = np.lexsort((np.arange(fb.N_PLANTED), -sc.astype(np.float64)))
    order64 = np.lexsort((np.arange(fb.N_PLANTED), -case.exact[:fb.N_PLANTED]))
    assert np.array_equal(order32, order64)
    assert len(np.unique(sc)) == fb.N_PLANTED, "the reference's fp32 scores tie"


def test_every_gpu_shape_plans_a_bootstrap_and_two_chunks():
    """n = 65 541 on the filter route: a bootstrap (d <= 768) or an exact first chunk (d > 768) and at least two filter chunks."""
    nvdb_amd = pytest.importorskip("nvdb_amd")
    kinds = {"f16": dict(dtype=nvdb_amd.DT_F16), "f32": dict(dtype=nvdb_amd.DT_F32, has_shadow16=1), "i8": dict(dtype=nvdb_amd.DT_I8),
             "sh8": dict(dtype=nvdb_amd.DT_F16, has_shadow8=1, q8shadow=1)}
    shapes = [("f16", 768, 768, (1, 64, 300)), ("f16", 384, 384, (300,)), ("f16", 600, 640, (300,)), ("f16", 1536, 1536, (300,)),
              ("i8", 768, 768, (64, 300)), ("i8", 384, 384, (300,)), ("i8", 1536, 1536, (300,)), ("sh8", 768, 768, (300,)), ("f32", 768, 768, (64,))]
    for kind, d, fdim, nqs in shapes:
        extra = dict(kinds[kind])
        if kind == "f16" and fdim != d:
            extra["has_shadow16"] = 1
        for nq in nqs:
            p = nvdb_amd.debug_plan(dict(n=fb.N, dim=d, fdim=fdim, owned=1, num_cu=256, **extra), nq, fb.K, {"path": 2})
            assert p["route"] == 2 and p["n_chunks"] >= 2, (kind, d, nq, p)
            assert p["boot"] == (0 if fdim <= 768 else 1), (kind, d, nq, p)      # BOOT_MFMA / BOOT_EXACT_CHUNK (nvdb_plan.h)
            assert p["boot_rows"] < p["chunk_hi"][0]
            assert fb.N % p["tile_rows"] != 0
