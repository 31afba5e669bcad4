"""Which filter a flat search streams on an fp16 corpus (csrc/nvdb_plan.h, field `filter_shadow` of nvdb_hip_debug_plan): the
int8 shadow exactly where the load-time rule (csrc/nvdb_ctx.h q8_shadow_wanted) builds one, the fp16 filter when the shadow
has been demoted or switched off.  Pure integer arithmetic: no GPU.  shape field load_rule = 1 applies the rule a corpus load
applies, from the options and free_hbm bytes of free HBM."""
import pytest

import nvdb_amd

F16, F32, I8 = nvdb_amd.DT_F16, nvdb_amd.DT_F32, nvdb_amd.DT_I8
GB = 1 << 30
KEYS = ("route", "QPB", "QT", "cap", "tile_rows", "growth", "boot_tiles", "boot", "perm_on", "padded", "n_al", "chunk_lo", "chunk_hi")


def plan(n, d=768, nq=1024, k=10, dtype=F16, options=None, free_hbm=256 * GB, owned=1, **shape):
    return nvdb_amd.debug_plan(dict(n=n, dim=d, fdim=d, dtype=dtype, owned=owned, num_cu=256, load_rule=1, free_hbm=free_hbm, **shape),
                               nq, k, options or {})


def same_plan(a, b):
    return all(a[key] == b[key] for key in KEYS)


def test_default_thresholds_take_the_flagship_and_a_shard_but_not_100M_rows():
    assert plan(10_000_000)["filter_shadow"] == 1                # 7.72 GB
    assert plan(12_500_000)["filter_shadow"] == 1                # 9.65 GB: one of eight shards of the 100M-row corpus
    assert plan(100_000_000)["filter_shadow"] == 0               # 77.2 GB > 16384 MB
    assert plan(1 << 20)["filter_shadow"] == 1 and plan((1 << 20) - 1)["filter_shadow"] == 0      # q8_auto_min_rows
    # what the shadow plan is: the int8 two-stage build's tiles and growth, exactly the explicit option's plan
    auto = plan(10_000_000)
    explicit = nvdb_amd.debug_plan(dict(n=10_000_000, dim=768, fdim=768, dtype=F16, owned=1, num_cu=256, has_shadow8=1, q8shadow=1), 1024, 10,
                                   {"q8_shadow": 1})
    assert explicit["filter_shadow"] == 1 and same_plan(auto, explicit)
    assert (auto["route"], auto["tile_rows"], auto["growth"], auto["boot_tiles"]) == (2, 64, 6, 1024)


@pytest.mark.parametrize("nq", [1, 8, 64, 200, 1024])
def test_each_rule_of_the_automatic_shadow(nq):
    n, low = 40_037, {"q8_auto_min_rows": 1024}
    on = plan(n, nq=nq, options=low)
    assert on["route"] == 2 and on["filter_shadow"] == 1 and on["tile_rows"] == 64
    off = nvdb_amd.debug_plan(dict(n=n, dim=768, fdim=768, dtype=F16, owned=1, num_cu=256), nq, 10, {})    # the plan without a shadow
    assert off["filter_shadow"] == 0
    for what, p in {
        "rows below q8_auto_min_rows": plan(n, nq=nq, options={"q8_auto_min_rows": n + 1}),
        "default q8_auto_min_rows": plan(n, nq=nq),
        "over q8_auto_max_mb": plan(n, nq=nq, options={**low, "q8_auto_max_mb": 29}),          # 40 037 x 772 B = 29.48 MB
        "over a quarter of the free HBM": plan(n, nq=nq, options=low, free_hbm=4 * n * 772 - 1),
        "q8_shadow = 0": plan(n, nq=nq, options={**low, "q8_shadow": 0}),
    }.items():
        assert p["filter_shadow"] == 0 and same_plan(p, off), what
    assert plan(n, nq=nq, options={**low, "q8_auto_max_mb": 30})["filter_shadow"] == 1
    assert plan(n, nq=nq, options=low, free_hbm=4 * n * 772)["filter_shadow"] == 1
    # dtype and dim: fp32 keeps its fp16 shadow routing, int8 its own kernels, d = 2048 has no int8 build
    assert plan(n, nq=nq, dtype=F32, options=low, has_shadow16=1)["filter_shadow"] == 0
    assert plan(n, nq=nq, dtype=I8, options=low)["filter_shadow"] == 0
    assert plan(n, d=2048, nq=nq, options=low)["filter_shadow"] == 0
    # the explicit option builds it wherever the int8 kernels take the dim, fp32 corpora included, whatever the size
    assert plan(2048, nq=nq, options={"q8_shadow": 1})["filter_shadow"] == 1
    assert plan(n, nq=nq, dtype=F32, options={"q8_shadow": 1})["filter_shadow"] == 1
    assert plan(n, d=2048, nq=nq, options={"q8_shadow": 1})["filter_shadow"] == 0


@pytest.mark.parametrize("owned", [1, 0])
def test_a_demoted_shadow_plans_the_fp16_filter(owned):
    """... with the fp16 filter's own geometry: an adopted corpus is not padded for it (the shadow is), so its ragged tail goes to
    the exact kernel."""
    n, low = 40_037, {"q8_auto_min_rows": 1024}
    for nq in (8, 200, 1024):
        off = nvdb_amd.debug_plan(dict(n=n, dim=768, fdim=768, dtype=F16, owned=owned, num_cu=256), nq, 10, {})
        dem = plan(n, nq=nq, options=low, owned=owned, shadow_demoted=1)
        assert dem["filter_shadow"] == 0 and same_plan(dem, off) and dem["tail_exact"] == off["tail_exact"] == (0 if owned else 1)
        on = plan(n, nq=nq, options=low, owned=owned)
        assert on["filter_shadow"] == 1 and on["padded"] == 1 and on["tail_exact"] == 0
    # switched off after the load: the resident shadow is left alone
    sw = nvdb_amd.debug_plan(dict(n=n, dim=768, fdim=768, dtype=F16, owned=owned, num_cu=256, has_shadow8=1, q8shadow=1), 200, 10, {"q8_shadow": 0})
    assert sw["filter_shadow"] == 0
    # an fp32 corpus under the explicit option has no fp16 filter beside its shadow: nothing to demote to
    p = nvdb_amd.debug_plan(dict(n=n, dim=768, fdim=768, dtype=F32, owned=owned, num_cu=256, has_shadow8=1, q8shadow=1, shadow_demoted=1), 200, 10, {})
    assert p["filter_shadow"] == 1


def test_exact_and_any_k_routes_stream_no_filter():
    low = {"q8_auto_min_rows": 1024}
    assert plan(40_037, nq=8, options={**low, "path": 1})["filter_shadow"] == 0
    assert plan(40_037, nq=8, k=2000, options=low)["filter_shadow"] == 0
