"""The bf16 bounds of bf16_bounds.py accept a correct kernel and reject a subtly wrong one, shown on the CPU.

The "kernel" here is its emulation: fp32 torch, one round-to-nearest-even bf16 store (single-rounding kernels)
or bf16 rounding at the fused kernels' store points.  The emulation must pass; the emulation with a small bug
must fail.  For the conv bugs the check these bounds replace (a share of 0.1 % of the elements exempt,
2e-2 + 2e-2 |ref|) is shown to accept every one of them.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_bounds as bb

# the first six parametrisations of test_kernels_gpu.py::test_conv_matches_torch, same seeds
CONV_CASES = [
    (2, 40, 32, 64, 3, 1, "silu"),
    (2, 40, 64, 128, 3, 2, "silu"),
    (1, 80, 16, 32, 3, 2, "silu"),
    (3, 20, 256, 128, 1, 1, "silu"),
    (2, 28, 32, 144, 1, 1, "relu6"),
    (1, 20, 80, 80, 3, 1, "silu"),
]


def _old_check_passes(got, ref, rtol=2e-2, atol=2e-2):
    """The check being replaced (test_kernels_gpu.py::_check before this module), as a predicate."""
    err = (got.float() - ref.float()).abs()
    tol = atol + rtol * ref.float().abs()
    bad = (err > tol).float().mean().item()
    return bad < 1e-3


def _conv_case(B, H, Cin, Cout, k, s, act):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + Cin)
    x = bb.bf(torch.randn(B, Cin, H, H, generator=g))
    w = bb.bf(torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k))
    b = torch.randn(Cout, generator=g) * 0.1
    return x, w, b


def _act32(y, act):
    return F.silu(y) if act == "silu" else F.relu6(y) if act == "relu6" else y


def _emulate_conv(x, w, b, k, s, act):
    """fp32 value before the store."""
    return _act32(F.conv2d(x, w, b, stride=s, padding=k // 2), act)


def _truncate_bf16(y32):
    return (y32.contiguous().view(torch.int32) & -65536).view(torch.float32)


@pytest.fixture(scope="module", params=CONV_CASES, ids=lambda c: "-".join(str(v) for v in c))
def conv_case(request):
    B, H, Cin, Cout, k, s, act = request.param
    x, w, b = _conv_case(*request.param)
    ref, scale = bb.conv_refs(x.double(), w.double(), b.double(), stride=s, padding=k // 2, act=act)
    y32 = _emulate_conv(x, w, b, k, s, act)
    return {"p": request.param, "x": x, "w": w, "b": b, "ref": ref, "scale": scale, "y32": y32}


def _conv_mutants(c):
    """name -> the output of the emulated kernel with one bug."""
    B, H, Cin, Cout, k, s, act = c["p"]
    x, w, b, y32 = c["x"], c["w"], c["b"], c["y32"]
    out = {}
    good = bb.bf(y32)
    if k == 3:  # a halo / edge-tile bug: the last input column read as zero, for the last output column of
        # one image and 4 channels
        xz = x.clone()
        xz[..., -1] = 0
        edge = _emulate_conv(xz, w, b, k, s, act)
        m = good.clone()
        m[B - 1, 4:8, :, -1] = bb.bf(edge)[B - 1, 4:8, :, -1]
        out["edge_column"] = m
    out["bias_x0.9"] = bb.bf(_emulate_conv(x, w, b * 0.9, k, s, act))
    m = good.clone()
    m.view(-1)[torch.arange(50) * (m.numel() // 50) + 3] = float("nan")
    out["nan_x50"] = m
    out["truncating_store"] = _truncate_bf16(y32)
    return out


def test_once_accepts_the_emulated_conv(conv_case):
    c = conv_case
    worst = bb.assert_bf16_once(bb.bf(c["y32"]), c["ref"], c["scale"], what=str(c["p"]))
    assert worst > 0.5  # the bound is the rounding's own size, not a multiple of it
    # with an fp32 store the rounding term drops and the fp32 bound alone holds
    bb.assert_bf16_once(c["y32"], c["ref"], c["scale"], f32out=True, what=str(c["p"]))


def test_once_rejects_every_conv_mutant(conv_case):
    c = conv_case
    mutants = _conv_mutants(c)
    assert len(mutants) == (4 if c["p"][4] == 3 else 3)
    for name, m in mutants.items():
        with pytest.raises(AssertionError, match="single-rounding bound"):
            bb.assert_bf16_once(m, c["ref"], c["scale"], what=name)


def test_old_check_accepts_the_conv_mutants():
    """What made the replacement necessary: on the first 3x3 SiLU case the old formula passes all four bugs."""
    p = CONV_CASES[0]
    B, H, Cin, Cout, k, s, act = p
    x, w, b = _conv_case(*p)
    ref, scale = bb.conv_refs(x.double(), w.double(), b.double(), stride=s, padding=1, act=act)
    c = {"p": p, "x": x, "w": w, "b": b, "ref": ref, "scale": scale, "y32": _emulate_conv(x, w, b, k, s, act)}
    mutants = _conv_mutants(c)
    assert sorted(mutants) == ["bias_x0.9", "edge_column", "nan_x50", "truncating_store"]
    ref32 = F.silu(F.conv2d(x, w, b, padding=1))  # the old test's fp32 torch reference
    changed = (mutants["edge_column"] != bb.bf(c["y32"])).sum().item()
    assert changed >= 100, changed  # the edge bug really changes the column
    for name, m in mutants.items():
        assert _old_check_passes(m, ref32), name
        with pytest.raises(AssertionError):
            bb.assert_bf16_once(m, ref, scale, what=name)


def test_once_f32out_rejects_a_bf16_rounded_value():
    """f32out drops the rounding term: a value that was rounded to bf16 on the way is outside it."""
    p = CONV_CASES[3]
    x, w, b = _conv_case(*p)
    ref, scale = bb.conv_refs(x.double(), w.double(), b.double(), act="silu")
    with pytest.raises(AssertionError):
        bb.assert_bf16_once(bb.bf(_emulate_conv(x, w, b, 1, 1, "silu")), ref, scale, f32out=True)


def test_ulp_bf16():
    v = torch.tensor([1.0, 1.99, 2.0, -3.0, 0.75, 100.0], dtype=torch.float64)
    assert bb.ulp_bf16(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8, 0.5]
    one = torch.tensor([1.0])
    assert (one.to(torch.bfloat16).view(torch.int16) + 1).view(torch.bfloat16).float().item() == 1 + 2.0 ** -7


# ---------------------------------------------------------------------------------------------- fused check
# test_kernels_gpu.py::test_ir_block_matches_torch's 28x28 residual block and 14x14 block, same seeds
IR_CASES = [(2, 28, 32, 192, 32, 1, True), (3, 14, 64, 384, 96, 1, False)]


def _ir_case(B, H, inp, hid, oup, s, res):
    g = torch.Generator().manual_seed(H * 100 + inp + oup)
    x = bb.bf(torch.rand(B, inp, H, H, generator=g) * 2)
    expand = (torch.randn(hid, inp, 1, 1, generator=g) / np.sqrt(inp), torch.randn(hid, generator=g) * 0.1)
    dw = (torch.randn(hid, 1, 3, 3, generator=g) / 3, torch.randn(hid, generator=g) * 0.1)
    project = (torch.randn(oup, hid, 1, 1, generator=g) / np.sqrt(hid), torch.randn(oup, generator=g) * 0.1)
    return x, expand, dw, project


@pytest.fixture(scope="module", params=IR_CASES, ids=lambda c: "-".join(str(v) for v in c))
def ir_case(request):
    B, H, inp, hid, oup, s, res = request.param
    x, expand, dw, project = _ir_case(*request.param)
    refs = bb.ir_refs(x, expand, dw, project, s, res)
    y32, hd = bb.ir_emulate(x, expand, dw, project, s, res, parts=True)
    flips, rms = bb.fused_stats(bb.bf(y32), refs[2], refs[3])
    return {"p": request.param, "project": project, "refs": refs, "y32": y32, "hd": hd, "flips": flips, "rms": rms}


def test_fused_accepts_the_emulated_ir_block(ir_case):
    c = ir_case
    r = bb.assert_bf16_fused(bb.bf(c["y32"]), *c["refs"], bb.flip_cap(c["flips"]), c["rms"], what=str(c["p"]))
    # tier 1 is derived with slack (worst-case propagation); the emulation sits well inside it, and its rms error
    # is that of one rounding (1 / sqrt(3) of a half-ulp at most) plus the rare flipped intermediates
    assert 0.05 < r["worst"] < 0.6, r
    assert c["flips"] < 5e-4 and 0.3 < c["rms"] < 0.6, (c["flips"], c["rms"])


def test_fused_rejects_every_ir_mutant(ir_case):
    c = ir_case
    B = c["p"][0]
    wp, bp = bb.bf(c["project"][0]), c["project"][1].float()
    cap, rms_ref = bb.flip_cap(c["flips"]), c["rms"]
    # one hidden channel's contribution missing from the last output column of one image: a channel whose
    # depthwise output is live (non-zero) on that column
    col = c["hd"][B - 1, :, :, -1]  # [hid, Ho]
    live = int(torch.argmax((col > 0).float().sum(1) + col.mean(1) * 1e-3))
    assert (col[live] > 0).float().mean() > 0.5, "pick a live channel"
    m = c["y32"].clone()
    m[B - 1, :, :, -1] -= wp[:, live, 0, 0][:, None] * col[live][None, :]
    with pytest.raises(AssertionError, match="tier"):
        bb.assert_bf16_fused(bb.bf(m), *c["refs"], cap, rms_ref, what="hidden channel dropped on the edge column")
    # the project bias missing on 4 channels
    m = c["y32"].clone()
    m[:, 8:12] -= bp[8:12][None, :, None, None]
    with pytest.raises(AssertionError, match="tier"):
        bb.assert_bf16_fused(bb.bf(m), *c["refs"], cap, rms_ref, what="project bias dropped")
    # one NaN
    m = bb.bf(c["y32"])
    m[0, 1, 2, 3] = float("nan")
    with pytest.raises(AssertionError, match="tier 1"):
        bb.assert_bf16_fused(m, *c["refs"], cap, rms_ref, what="one NaN")


def test_fused_tier3_sees_a_small_uniform_error(ir_case):
    """A project bias scaled by 0.9 stays inside tier 1's slack on (nearly) every element; the rms tier sees it."""
    c = ir_case
    bp = c["project"][1].float()
    m = bb.bf(c["y32"] - 0.1 * bp[None, :, None, None])
    exact, bound, mimic, tight = c["refs"]
    over1 = ((m.double() - exact).abs() > bound).double().mean().item()
    assert over1 < 1e-3, over1  # tier 1 alone, with a share exempt as the old check had, would pass it
    _, rms = bb.fused_stats(m, mimic, tight)
    assert rms > bb.RMS_FACTOR * c["rms"], (rms, c["rms"])
    with pytest.raises(AssertionError, match="tier"):
        bb.assert_bf16_fused(m, *c["refs"], bb.flip_cap(c["flips"]), c["rms"], what="project bias x 0.9")


C3_CASES = [(32, 16, 1, True), (64, 32, 2, True), (128, 32, 1, False)]


@pytest.mark.parametrize("C1,ch,n,shortcut", C3_CASES)
def test_fused_accepts_the_emulated_c3_block(C1, ch, n, shortcut):
    x, cv12, bn, cv3 = bb.c3_case(C1, ch, C1 + n)
    refs = bb.c3_refs(x, cv12, bn, cv3, n, shortcut)
    emu = bb.c3_emulate(x, cv12, bn, cv3, n, shortcut)
    flips, rms = bb.fused_stats(emu, refs[2], refs[3])
    r = bb.assert_bf16_fused(emu, *refs, bb.flip_cap(flips), rms, what=f"c3 {C1}/{ch}/{n}")
    assert r["worst"] < 0.7, r  # worst-case propagation through four to six stages: far inside
    assert flips < 2e-3 and 0.3 < rms < 0.7, (flips, rms)
    # a 3x3 that reads zero past the right map edge of U where the true neighbour tile has data would be an
    # interior-border bug; its mirror image here: the last column computed without the 3x3's contribution
    bad = emu.float().clone()
    noconv = bb.c3_emulate(x, cv12, (bn[0], (bn[1][0] * 0, bn[1][1])), cv3, n, shortcut).float()
    bad[1, :, :, 15] = noconv[1, :, :, 15]  # the column left of the tile border at x = 16
    with pytest.raises(AssertionError, match="tier"):
        bb.assert_bf16_fused(bad, *refs, bb.flip_cap(flips), rms, what="3x3 dropped on a tile-border column")


@pytest.mark.parametrize("H", [16, 32])
def test_fused_accepts_the_emulated_two_stage_stem(H):
    """stem2_refs / stem2_emulate (the detector front end of stem_fused.hip: a bf16 SiLU stem map in LDS, then the
    3x3 stride-2 conv): the emulation passes the three tiers; a stem map that is not zeroed outside the S/2 map
    (the second conv then reads stem values of padding instead of its own zero padding) fails them."""
    g = torch.Generator().manual_seed(H)
    x = bb.bf(torch.rand(2, 16, H, H, generator=g))
    x[:, 12:] = 0
    stem = (torch.randn(16, 16, 3, 3, generator=g) * 3 / 108 ** 0.5, torch.randn(16, generator=g) * 0.1)
    second = (torch.randn(32, 16, 3, 3, generator=g) / 12, torch.randn(32, generator=g) * 0.1)
    refs = bb.stem2_refs(x, stem, second)
    y32, T = bb.stem2_emulate(x, stem, second, parts=True)
    flips, rms = bb.fused_stats(bb.bf(y32), refs[2], refs[3])
    r = bb.assert_bf16_fused(bb.bf(y32), *refs, bb.flip_cap(flips), rms, what=f"stem2 {H}")
    assert r["worst"] < 0.7 and flips < 5e-4 and 0.3 < rms < 0.6, (r, flips, rms)
    # the stem output of the padding ring is SiLU(bias), not zero
    ring = F.pad(T, (1, 1, 1, 1)) + F.pad(torch.zeros_like(T), (1, 1, 1, 1), value=1.0) * \
        bb.bf(F.silu(stem[1].float()))[None, :, None, None]
    bad = F.silu(F.conv2d(ring, bb.bf(second[0]), second[1].float(), stride=2))
    with pytest.raises(AssertionError, match="tier"):
        bb.assert_bf16_fused(bb.bf(bad), *refs, bb.flip_cap(flips), rms, what="stem map not zeroed outside the map")
