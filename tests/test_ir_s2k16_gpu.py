"""MobileNetV2 block 2 (stride 2, 16 -> 96 -> 24 channels) on K-packed x3 matrix-core products
(csrc/kernels/ir_s2k16_x3.hip) against the fp64 chain, with the native switch ``set_ir_s2k16`` on (the new kernel)
and off (``ir_f32_kernel``, exact-fp32 MFMAs) on the same operands.

Everything goes through ``AF.ir_block_nhwc`` with fp32 input, under the bound of
``test_fp32_gpu.py::test_ir_block_f32_matches_fp64``: max abs error < 2e-5 * (1 + max|ref|).
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp32_bounds as fb
from inference_arena_amd.ops import functional as AF

pytestmark = pytest.mark.gpu

INP, HID, OUP, STRIDE = 16, 96, 24, 2
SENTINEL = 12345.0


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _ir_ref64(x, expand, dw, project, stride, res):
    h = x.double()
    if expand is not None:
        h = F.conv2d(h, expand[0].double(), expand[1].double()).clamp(0, 6)
    C = dw[0].shape[0]
    h = F.conv2d(h, dw[0].double(), dw[1].double(), stride=stride, padding=1, groups=C).clamp(0, 6)
    y = F.conv2d(h, project[0].double(), project[1].double())
    return y + x.double() if res else y


def _bound(ref):
    return 2e-5 * (1.0 + ref.abs().max().item())


_cases: dict = {}


def _case(H, W, B):
    """Input, weights and the fp64 reference of one shape: computed once, shared, never modified."""
    key = (H, W, B)
    if key not in _cases:
        g = torch.Generator().manual_seed(1000 * H + 10 * W + B)
        x = torch.randn(B, INP, H, W, generator=g)
        expand = (torch.randn(HID, INP, 1, 1, generator=g) / INP ** 0.5, torch.randn(HID, generator=g) * 0.1)
        dw = (torch.randn(HID, 1, 3, 3, generator=g) / 3, torch.randn(HID, generator=g) * 0.1)
        project = (torch.randn(OUP, HID, 1, 1, generator=g) / HID ** 0.5, torch.randn(OUP, generator=g) * 0.1)
        zc = fb.s2k16_case(H, W, B)  # the same draws: its fp64 variance model for the two tiers of fp32_bounds.py
        assert torch.equal(zc.x, x)
        _cases[key] = (x, expand, dw, project, _ir_ref64(x, expand, dw, project, STRIDE, False), zc)
    return _cases[key]


@pytest.fixture
def s2k16(request):
    """Sets the native switch for the test and restores the library's default after it."""
    from inference_arena_amd.ops import native

    def set_(on):
        native().set_ir_s2k16(bool(on))

    try:  # the library's own default: the environment variable read as an integer, on when unset
        default = int(os.environ.get("ARENA_IR_S2K16", "1")) != 0
    except ValueError:
        default = False
    request.addfinalizer(lambda: native().set_ir_s2k16(default))
    return set_


def _run(device, case, **kw):
    x, expand, dw, project = case[:4]
    y = AF.ir_block_nhwc(_nhwc(x).to(device), expand, dw, project, stride=STRIDE, res=False, **kw)
    return y


def _nchw64(y):
    return y.permute(0, 3, 1, 2).double().cpu()


@pytest.mark.parametrize("H,W,B", [
    (8, 8, 1),      # one output tile; every halo side is the zero border
    (37, 37, 3),    # odd size, partial tiles on both axes
    (16, 24, 2),    # non-square, exact tiles
    (112, 112, 1),  # the block's real size
])
@pytest.mark.parametrize("on", [1, 0])
def test_block2_matches_fp64(device, s2k16, H, W, B, on):
    s2k16(on)
    case = _case(H, W, B)
    ref = case[4]
    got = _nchw64(_run(device, case))
    assert got.shape == ref.shape
    err = (got - ref).abs().max().item()
    print(f"s2k16={on} {H}x{W}x{B}: max abs err {err:.3g}, bound {_bound(ref):.3g}")
    assert err < _bound(ref), err
    fb.check(case[5], got, f"s2k16={on}")


@pytest.mark.parametrize("on", [1, 0])
def test_block2_live_batch(device, s2k16, on):
    """5 crops with a device-side live count of 3: crops 0-2 match the fp64 chain, crops 3-4 are not written."""
    s2k16(on)
    case = _case(20, 20, 5)
    ref = case[4]
    bdev = torch.tensor([3], dtype=torch.int32, device=device)
    out = torch.full((5, 10, 10, OUP), SENTINEL, dtype=torch.float32, device=device)
    y = _run(device, case, bdev=bdev, out=out)
    got = _nchw64(y)
    err = (got[:3] - ref[:3]).abs().max().item()
    assert err < _bound(ref[:3]), err
    fb.check(case[5], got, f"s2k16={on} live", live=3)
    assert torch.equal(y[3:].cpu(), torch.full((2, 10, 10, OUP), SENTINEL))


@pytest.mark.parametrize("on", [1, 0])
def test_block2_channel_guard(device, s2k16, on):
    """Output pixel stride 32 for 24 channels: channels 24-31 of every pixel stay as they were."""
    s2k16(on)
    case = _case(37, 37, 3)
    ref = case[4]
    out = torch.full((3, 19, 19, 32), SENTINEL, dtype=torch.float32, device=device)
    y = _run(device, case, out=out).cpu()
    assert torch.equal(y[..., OUP:], torch.full((3, 19, 19, 32 - OUP), SENTINEL))
    err = (_nchw64(y[..., :OUP]) - ref).abs().max().item()
    assert err < _bound(ref), err
    fb.check(case[5], _nchw64(y[..., :OUP]), f"s2k16={on} guard")


def test_block2_new_against_old(device, s2k16):
    """Both kernels evaluate the same function to fp32 accuracy: each may use the whole fp64 bound, so they
    differ by less than twice that bound."""
    case = _case(37, 37, 3)
    ref = case[4]
    s2k16(1)
    new = _nchw64(_run(device, case))
    s2k16(0)
    old = _nchw64(_run(device, case))
    d = (new - old).abs().max().item()
    print(f"new against old: max abs diff {d:.3g}, bound {2 * _bound(ref):.3g}")
    assert d < 2 * _bound(ref), d


def test_classifier_program_switch_on_off(device, s2k16):
    """Crop-fed classifier program, 5 crops into a capacity of 8: the same top-1 class for every crop with the
    switch on and off, top-1 logits within the rel < 1e-3 of test_headline_gpu.py."""
    from inference_arena_amd.engine.pipeline import GpuClassifier
    from inference_arena_amd.models.zoo import make_mobilenet

    rng = np.random.default_rng(5)
    crops = [rng.integers(0, 256, (224, 224, 3), dtype=np.uint8) for _ in range(5)]
    mnet = make_mobilenet(1)
    out = []
    for on in (1, 0):  # the program's kernels are captured into graphs at construction: one runner per setting
        s2k16(on)
        cls = GpuClassifier(mnet, device=0, buckets=[8], dtype="fp32")
        out.append(cls.infer(crops))
        del cls
    new, old = out
    assert len(new) == len(old) == 5
    for (ni, nl, _), (oi, ol, _) in zip(new, old):
        assert int(ni[0]) == int(oi[0]), (ni[0], oi[0], nl[0], ol[0])
        rel = abs(float(nl[0]) - float(ol[0])) / (abs(float(ol[0])) + 1e-6)
        print(f"top-1 {int(ni[0])}: logit {float(nl[0]):.6f} vs {float(ol[0]):.6f}, rel {rel:.3g}")
        assert rel < 1e-3, rel
