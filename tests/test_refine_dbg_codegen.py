"""Codegen guard of the refine kernels' STAMP builds (option refine_dbg_q, reference CUDA_DBG_TIMING): no GPU needed.

Every refine kernel template has a STAMP = true build (TWINS below) that runs the same body with four s_memtime stamps in wave 0
(kernel entry, after the candidate loop, after the list write + barrier, after the merge and the output stores).  The STAMP builds
must exist for all ten product instantiations, hold exactly those four stamps, write them with vector stores only, keep the v3 kernel's hand-placed
instructions and register budget, and use no scratch; the product kernels hold no stamp at all.  Reads the same
`make -C nano-vectordb_amd asm` output as tests/test_codegen_resources.py, through its fixture."""
import re

from test_codegen_resources import _body, _find, codegen  # noqa: F401  (codegen: the shared module fixture)

PRODUCT = ["refine_l2_kernel<1, false, false>", "refine_l2_kernel<1, true, false>", "refine_l2_kernel<2, false, false>", "refine_l2_kernel<2, true, false>",
           "refine_l2_lds_kernel<1, false>", "refine_l2_lds_kernel<2, false>",
           "refine_l2_rows_kernel<768, false>", "refine_l2_rows_kernel<512, false>", "refine_l2_rows_kernel<384, false>", "refine_l2_rows_kernel<256, false>"]
TWINS = ["refine_l2_kernel<1, false, true>", "refine_l2_kernel<1, true, true>", "refine_l2_kernel<2, false, true>", "refine_l2_kernel<2, true, true>",
         "refine_l2_lds_kernel<1, true>", "refine_l2_lds_kernel<2, true>",
         "refine_l2_rows_kernel<768, true>", "refine_l2_rows_kernel<512, true>", "refine_l2_rows_kernel<384, true>", "refine_l2_rows_kernel<256, true>"]


def _mnemonics(body):
    return [ln.split()[0] for ln in body.splitlines() if ln.startswith("\t") and ln.strip() and not ln.strip().startswith((".", ";"))]


def test_every_refine_kernel_has_a_stamped_twin(codegen):
    by_name, _ = codegen
    assert sorted(k for k in by_name if k.startswith("refine_l2_") and k.endswith(", true>")) == sorted(TWINS)
    for name in PRODUCT:
        _find(by_name, name)                      # exactly one match: the STAMP builds' names do not contain the product names


def test_twins_hold_exactly_four_stamps_and_store_them_with_vector_stores(codegen):
    by_name, asm = codegen
    for name in TWINS:
        ops = _mnemonics(_body(asm, by_name[name]["mangled"]))
        assert ops.count("s_memtime") == 4, (name, ops.count("s_memtime"))
        stores = {op for op in ops if "store" in op}
        assert stores and all(op.startswith("global_store_") for op in stores), (name, stores)


def test_product_refine_kernels_hold_no_stamp(codegen):
    by_name, asm = codegen
    for name in PRODUCT:
        assert "s_memtime" not in _mnemonics(_body(asm, _find(by_name, name)["mangled"])), name


def test_v3_twin_keeps_the_hand_placed_instructions_and_register_budget(codegen):
    by_name, asm = codegen
    k = by_name["refine_l2_rows_kernel<768, true>"]
    assert k["vgpr"] + k["agpr"] <= 256 and k["occ"] >= 2, k
    body = _body(asm, k["mangled"])
    assert body.count("v_fma_mix_f32") == 192 and body.count("v_cvt_f32_f16") == 0 and body.count("global_load_lds_dwordx4") == 24
    # the stamps stay outside the hand-counted issue / consume step: no stamp between two direct-to-LDS loads
    ops = _mnemonics(body)
    first, last = ops.index("global_load_lds_dwordx4"), len(ops) - 1 - ops[::-1].index("global_load_lds_dwordx4")
    assert "s_memtime" not in ops[first:last]


def test_twins_use_no_scratch(codegen):
    by_name, _ = codegen
    for name in TWINS:
        v = by_name[name]
        assert v["scratch"] == 0 and v["vspill"] == 0 and v["sspill"] == 0, (name, v)
