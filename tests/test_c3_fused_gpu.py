"""The bf16 C3 block kernel (csrc/kernels/c3_fused.hip) on its own against fp64 references (MI355X only).

B 2, H 16, W 32 is 2 x 2 tiles of 8 x 16: every interior tile border and every map edge is there, and with two
bottleneck repeats the two-pixel halo is exercised.  The binding feeds one bottleneck weight set to both repeats;
the references do the same.  The kernel's bf16 store points (its LDS ``pack4`` stores of T, U and the updated
T[:c_]) are modelled by bf16_bounds.c3_refs / c3_emulate; the three tiers are those of bf16_bounds.py.
"""
from __future__ import annotations

import pytest
import torch

import bf16_bounds as bb
from inference_arena_amd.ops import functional as AF

pytestmark = pytest.mark.gpu

GEOMETRIES = [(32, 16, 1, True), (64, 32, 2, True), (128, 32, 1, False)]


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).float()


_cases: dict = {}


def _case(C1, ch, n, shortcut):
    """Inputs, the four reference tensors and the emulation's tier 2 / 3 figures, computed once per geometry."""
    key = (C1, ch, n, shortcut)
    if key not in _cases:
        x, cv12, bn, cv3 = bb.c3_case(C1, ch, C1 + n)
        refs = bb.c3_refs(x, cv12, bn, cv3, n, shortcut)
        emu = bb.c3_emulate(x, cv12, bn, cv3, n, shortcut)
        flips, rms = bb.fused_stats(emu, refs[2], refs[3])
        _cases[key] = (x, cv12, bn, cv3, refs, flips, rms, emu)
    return _cases[key]


@pytest.mark.parametrize("C1,ch,n,shortcut", GEOMETRIES)
def test_c3_fused_matches_fp64(device, C1, ch, n, shortcut):
    x, cv12, bn, cv3, refs, flips, rms, emu = _case(C1, ch, n, shortcut)
    y = AF.c3_fused_nhwc(_nhwc(x).to(torch.bfloat16).to(device), cv12, bn, cv3, n=n, shortcut=shortcut)
    assert y.shape == (2, 16, 32, 2 * ch) and y.dtype == torch.bfloat16
    r = bb.assert_bf16_fused(_nchw(y.cpu()), *refs, bb.flip_cap(flips), rms, what=f"c3_fused {C1}/{ch}/{n}")
    print(f"c3_fused-{C1}-{ch}-{n}: emulation flips {flips:.3g} rms {rms:.4f}; kernel flips {r['flips']:.3g} "
          f"rms {r['rms']:.4f} worst {r['worst']:.3f}")


def test_c3_fused_live_batch(device):
    """Images past the device-side live count are not written."""
    C1, ch, n, shortcut = GEOMETRIES[1]
    x, cv12, bn, cv3, refs, flips, rms, emu = _case(C1, ch, n, shortcut)
    out = torch.full((2, 16, 32, 2 * ch), -7.0, dtype=torch.bfloat16, device=device)
    bdev = torch.tensor([1], dtype=torch.int32, device=device)
    AF.c3_fused_nhwc(_nhwc(x).to(torch.bfloat16).to(device), cv12, bn, cv3, n=n, shortcut=shortcut, out=out, bdev=bdev)
    o = out.cpu()
    assert torch.all(o[1] == -7.0), "the image past the live count must not be written"
    flips, rms = bb.fused_stats(emu[:1], refs[2][:1], refs[3][:1])  # the emulation's figures on the live image
    bb.assert_bf16_fused(_nchw(o[:1]), *(t[:1] for t in refs), bb.flip_cap(flips), rms, what="c3_fused live 1 of 2")


@pytest.mark.parametrize("C1,ch,n,shortcut", [GEOMETRIES[0], GEOMETRIES[2]])
def test_c3_fused_channel_slices(device, C1, ch, n, shortcut):
    """Reads a channel slice of a wider buffer and writes into a channel slice of a wider one (the concat buffers
    of the detector); the channels around both slices are neither read nor written."""
    x, cv12, bn, cv3, refs, flips, rms, emu = _case(C1, ch, n, shortcut)
    g = torch.Generator().manual_seed(5)
    buf = torch.randn(2, 16, 32, C1 + 48, generator=g).to(torch.bfloat16)
    buf[..., 16:16 + C1] = _nhwc(x).to(torch.bfloat16)
    out = torch.full((2, 16, 32, 2 * ch + 40), -7.0, dtype=torch.bfloat16, device=device)
    AF.c3_fused_nhwc(buf.to(device), cv12, bn, cv3, n=n, shortcut=shortcut, x_coff=16, c1=C1, out=out, out_coff=8)
    o = out.cpu()
    assert torch.all(o[..., :8] == -7.0) and torch.all(o[..., 8 + 2 * ch:] == -7.0)
    plain = AF.c3_fused_nhwc(_nhwc(x).to(torch.bfloat16).to(device), cv12, bn, cv3, n=n, shortcut=shortcut)
    assert torch.equal(o[..., 8:8 + 2 * ch], plain.cpu())  # the same arithmetic, other addresses
    bb.assert_bf16_fused(_nchw(o[..., 8:8 + 2 * ch]), *refs, bb.flip_cap(flips), rms, what="c3_fused slices")


def test_c3_fused_refuses_other_geometries(device):
    x, cv12, bn, cv3, *_ = _case(*GEOMETRIES[0])
    with pytest.raises(RuntimeError, match="unsupported geometry"):
        # H 12 is not whole 8-row tiles
        AF.c3_fused_nhwc(_nhwc(x)[:, :12].contiguous().to(torch.bfloat16).to(device), cv12, bn, cv3)
    with pytest.raises(RuntimeError, match="unsupported geometry"):
        AF.c3_fused_nhwc(_nhwc(x).to(torch.bfloat16).to(device), cv12, bn, cv3, n=2)
