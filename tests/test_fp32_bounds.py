"""CPU proof that the two tiers of fp32_bounds.py (max z, rms z) reject subtly wrong fp32 kernels which the
per-element formulas of the GPU tests accept, and that plain torch fp32 and the intact x3 emulation pass them.

One one-stage case (K 80 on an 11 x 11 map: a partial K chunk, a partial pixel tile), one inverted-residual chain
(24 -> 144 -> 24 with residual) and the smallest C3 case, all members of the GPU tests' case lists, seeds fixed.
The "kernels" are the emulations of fp32_bounds.py: ``run32("torch")`` and ``run32("x3", damage)``.
"""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

import fp32_bounds as fb


def _old_single(got, case):
    """test_fp32_gpu.py::_fp32_check on a one-stage case: |got - ref| <= 2e-6 (sum |x||w| + |b| (+ |res|))."""
    st = case.stages[0]
    ref = case.refs()[0]
    x, w, b = case.x.double(), st["w"].float().double(), st["b"].float().double()
    scale = F.conv2d(x.abs(), w.abs(), b.abs(), stride=st.get("stride", 1), padding=st.get("padding", 0))
    if st.get("res") is not None:
        scale = scale + st["res"].double().abs()
    worst = ((got.double() - ref).abs() / (2e-6 * scale + 1e-30)).max().item()
    return worst <= 1.0


def _old_fused(got, case):
    """The fused-kernel tests' formula: max |got - ref| < 2e-5 (1 + max |ref|)."""
    ref = case.refs()[0]
    return (got.double() - ref).abs().max().item() < 2e-5 * (1.0 + ref.abs().max().item())


ONE = fb.x3g_case(2, 11, 80, 80, 1, 1, "silu", False)
ONE_CLAMP = fb.conv_clamp_case("x3hg", *fb.CLAMP_X3HG)
ONE_PLAIN = fb.x3hg_case(*fb.CLAMP_X3HG)
IR1 = fb.strips_case(24, 144, 24, 1, 20, True)
IR_CLAMP = fb.ir_case(24, 144, 24, 1, 19, True, gain=fb.CLAMP_GAIN, B=2)
IR_PLAIN = fb.ir_case(24, 144, 24, 1, 28, True)
C3 = fb.c3_case(1, 8, 16)
CASES = {"one": (ONE, _old_single), "ir": (IR1, _old_fused), "ir_clamp": (IR_CLAMP, _old_fused), "c3": (C3, _old_fused)}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("mode", ["torch", "x3"])
def test_correct_arithmetic_passes_both_tiers(name, mode):
    case, old = CASES[name]
    got = case.run32(mode)
    mx, rms = fb.zstats(got, *case.refs()[:2])
    print(f"{case.key} {mode}: max z {mx:.2f} (limit {fb.ZMAX[case.family]}), rms z {rms:.3f} ({fb.ZRMS[case.family]})")
    assert fb.passes(got, case) and old(got, case)


# damage -> per case name: the stage it hits and the damage's arguments; the old formula accepts each of these
_LAST_CHUNK = {"one": 64, "ir": 128, "ir_clamp": 128, "c3": 16}   # K 80, 144, 144, 32: the chunk past the last full 32 / 64
_LAST_STAGE = {"one": 0, "ir": 2, "ir_clamp": 2, "c3": 3}
SUBTLE = {
    "mm": lambda n: {"drop": ("mm",)},
    "lh": lambda n: {"drop": ("lh",)},
    "hl": lambda n: {"drop": ("hl",)},
    "mm_last_column": lambda n: {"drop": ("mm",), "cols": -1, "stages": (_LAST_STAGE[n],)},
    "mm_last_k_chunk": lambda n: {"drop": ("mm",), "chans": _LAST_CHUNK[n], "stages": (_LAST_STAGE[n],)},
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("damage", list(SUBTLE))
def test_lost_partial_products_fail_a_tier_but_pass_the_old_formula(name, damage):
    case, old = CASES[name]
    got = case.run32("x3", SUBTLE[damage](name))
    mx, rms = fb.zstats(got, *case.refs()[:2])
    print(f"{case.key} {damage}: max z {mx:.1f} (limit {fb.ZMAX[case.family]}), rms z {rms:.2f} ({fb.ZRMS[case.family]})")
    assert old(got, case), "the per-element formula was expected to accept this damage"
    assert not fb.passes(got, case)
    assert mx > fb.ZMAX[case.family]  # every one of these is caught by the localized tier


@pytest.mark.parametrize("name", ["ir", "ir_clamp", "c3"])
def test_scaled_bias_tile_fails_a_tier_but_passes_the_old_formula(name):
    """A bias scaled by 1 + 2^-12 in one 16-channel tile of the last stage: an error of 2.4e-4 |b|, |b| ~ 0.1, inside
    the fused tests' 1e-4.  (At K 80 the single-op formula, 2e-6 sum |x||w| ~ 1e-5, already rejects it.)"""
    case, old = CASES[name]
    got = case.run32("x3", {"bias_tile": 0, "stages": (_LAST_STAGE[name],)})
    assert old(got, case)
    assert not fb.passes(got, case)


@pytest.mark.parametrize("case", [ONE_CLAMP, IR_CLAMP], ids=["one", "ir"])
def test_relu_for_relu6_fails_on_clamp_reaching_inputs(case):
    fb.assert_clamped(case)
    assert fb.passes(case.run32("x3"), case)
    assert not fb.passes(case.run32("x3", {"relu": True}), case)


@pytest.mark.parametrize("case", [ONE_PLAIN, IR_PLAIN, IR1], ids=["one", "ir", "ir_strips"])
def test_relu_for_relu6_is_bit_identical_on_unit_gain_inputs(case):
    """The gap the clamp-reaching cases close: no pre-activation of the x 1 inputs exceeds 6, so a kernel with ReLU
    in place of ReLU6 returns the very same bits and no check of any tightness can see it."""
    assert all(hi == 0.0 for hi, _ in case.clamp_shares())
    with pytest.raises(AssertionError):
        fb.assert_clamped(case)
    assert torch.equal(case.run32("x3", {"relu": True}), case.run32("x3"))


@pytest.mark.parametrize("name", list(CASES))
def test_nan_fails(name):
    case, _ = CASES[name]
    assert not fb.passes(case.run32("x3", {"nan": True}), case)


def test_split_k_and_hidden_slice_terms_only_widen_sigma():
    """The extra-add terms are additions to the variance: a case checked with them is never held tighter."""
    ref, var0, _ = ONE.refs()
    assert torch.all(ONE.refs(adds=3)[1] >= var0) and torch.equal(ONE.refs(adds=3)[0], ref)
    assert fb.sk_adds(171, 80, 1) == 1 and fb.sk_adds(173, 80, 1) == 2 and fb.sk_adds(179, 512, 1) == 7
    assert fb.sk_adds(111, 512, 1) == 0 and fb.sk_adds(172, 16, 1) == 0
    a, b = fb.ir_chain_case(3, 5, 2), fb.ir_chain_case(1, 5, 2)
    assert a.stages[2]["parts"] == 3 and b.stages[2]["parts"] == 1


@pytest.mark.parametrize("case", [ONE, ONE_CLAMP, IR1, IR_CLAMP, C3], ids=lambda c: c.key)
def test_reference_rows_reproduce(case):
    """The REFERENCE rows of this file's cases, recomputed, within 10 % (torch's CPU conv choice moves the fp32
    figures a little; see bf16_bounds.ir_emulate on contiguous inputs.  So does a single-threaded run, which takes
    another conv path: the rows are recomputed on four threads, as the suite's default is)."""
    n = torch.get_num_threads()
    torch.set_num_threads(4)
    try:
        row = fb.reference_row(case)
    finally:
        torch.set_num_threads(n)
    want = fb.REFERENCE[case.key]
    print(case.key, [f"{v:.3g}" for v in row], want)
    for got, w in zip(row, want):
        assert abs(got - w) <= 0.10 * w, (case.key, row, want)


def test_families_separate_and_constants_are_their_geometric_means():
    """Per family: the mildest damaged figure is >= 4 x the largest torch fp32 figure over the REFERENCE rows, and
    ZMAX / ZRMS are the geometric means of the two (as recorded, to the rounding of the constants)."""
    fam = {c.key: c.family for c in fb.all_cases()}
    fam.update({k: "silu" for k in fb.REFERENCE if k.startswith("front-")})
    assert set(fam) == set(fb.REFERENCE)
    for f, (zm, zr, sm, sr) in fb.constants(fb.REFERENCE, fam).items():
        assert sm >= 4.0 and sr >= 4.0, (f, sm, sr)
        assert abs(fb.ZMAX[f] - zm) <= 0.02 * zm and abs(fb.ZRMS[f] - zr) <= 0.02 * zr, (f, zm, zr)
