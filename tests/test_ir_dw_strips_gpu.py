"""Depthwise phase of the tiled inverted-residual kernels (csrc/kernels/ir_tile_x3.hip): vertical strips of four
outputs per thread at stride 1, packed FMAs and the pairwise bf16 split at both strides.

The blocks run through ``AF.ir_block_nhwc`` with ``ARENA_IR_X3T=1`` at the smallest maps where the strips can go
wrong, against the fp64 reference and under the bound of ``test_fp32_gpu.py::test_ir_block_f32_matches_fp64``
(max abs error < 2e-5 * (1 + max|ref|)).  The stem kernel (``ir_stem_x3_kernel``) runs inside classifier programs.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp32_bounds as fb
from inference_arena_amd.ops import functional as AF

pytestmark = pytest.mark.gpu


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _ir_ref64(x, expand, dw, project, stride, res):
    h = F.conv2d(x.double(), expand[0].double(), expand[1].double()).clamp(0, 6)
    h = F.conv2d(h, dw[0].double(), dw[1].double(), stride=stride, padding=1, groups=dw[0].shape[0]).clamp(0, 6)
    y = F.conv2d(h, project[0].double(), project[1].double())
    return y + x.double() if res else y


def _block(inp, hid, oup, stride, H, B=3):
    g = torch.Generator().manual_seed(inp * 7 + hid + stride + H)
    x = torch.randn(B, inp, H, H, generator=g)
    expand = (torch.randn(hid, inp, 1, 1, generator=g) / inp ** 0.5, torch.randn(hid, generator=g) * 0.1)
    dw = (torch.randn(hid, 1, 3, 3, generator=g) / 3, torch.randn(hid, generator=g) * 0.1)
    project = (torch.randn(oup, hid, 1, 1, generator=g) / hid ** 0.5, torch.randn(oup, generator=g) * 0.1)
    return x, expand, dw, project


def _assert_tiled(inp, hid, oup, stride, H):
    """The block is one the tiled x3 kernel takes (else the test would check another kernel)."""
    from inference_arena_amd.engine.planner import ir_x3_plan, pack_ir_weights

    x, expand, dw, project = _block(inp, hid, oup, stride, H, B=1)
    pk = pack_ir_weights(expand, dw, project, inp, k_align=16)
    x3w, inp_pad = ir_x3_plan(H, H, stride, inp, pk["hid_pad"], pk["oup_pad"], 1)
    assert x3w == 1 and inp_pad == 32, (x3w, inp_pad)


@pytest.mark.parametrize("inp,hid,oup,stride,H,res", [
    # 8 x 16 tiles on a 12 x 12 map: one full and one partial tile row, a partial tile column; the strips of the
    # second tile row cross the map's last row
    (32, 64, 32, 1, 12, False),
    (32, 64, 32, 1, 12, True),
    # padded hidden chunk (144 -> 160), padded input (24 -> 32), W = 16 + 4
    (24, 144, 24, 1, 20, True),
    # stride 2 (4 x 8 tiles, one output per thread): packed FMAs and the pair split, odd tile count
    (32, 96, 24, 2, 10, False),
])
def test_ir_tile_strips_match_fp64(device, inp, hid, oup, stride, H, res, monkeypatch):
    monkeypatch.setenv("ARENA_IR_X3T", "1")
    _assert_tiled(inp, hid, oup, stride, H)
    x, expand, dw, project = _block(inp, hid, oup, stride, H)
    y = AF.ir_block_nhwc(_nhwc(x).to(device), expand, dw, project, stride=stride, res=res)
    ref = _ir_ref64(x, expand, dw, project, stride, res)
    got = y.permute(0, 3, 1, 2).double().cpu()
    err = (got - ref).abs().max().item()
    print(f"max abs err {err:.3g}, bound {2e-5 * (1.0 + ref.abs().max().item()):.3g}")
    assert err < 2e-5 * (1.0 + ref.abs().max().item()), err
    case = fb.strips_case(inp, hid, oup, stride, H, res)
    assert torch.equal(case.x, x)
    fb.check(case, got, "ir_tile_x3")


def test_ir_tile_strips_live_batch(device, monkeypatch):
    """Batch of 3 with a device-side live batch of 2: the first two crops match the fp64 reference, the third
    crop's output is not written (the output tensor is pre-filled with a sentinel)."""
    monkeypatch.setenv("ARENA_IR_X3T", "1")
    inp, hid, oup, stride, H = 32, 64, 32, 1, 12
    _assert_tiled(inp, hid, oup, stride, H)
    x, expand, dw, project = _block(inp, hid, oup, stride, H)
    sentinel = 12345.0
    real_empty = torch.empty

    def filled_empty(*a, **k):  # uninitialised memory may hold anything: make it the sentinel
        t = real_empty(*a, **k)
        return t.fill_(sentinel) if t.is_floating_point() else t

    bdev = torch.tensor([2], dtype=torch.int32, device=device)
    xn = _nhwc(x).to(device)
    monkeypatch.setattr(torch, "empty", filled_empty)
    y = AF.ir_block_nhwc(xn, expand, dw, project, stride=stride, res=True, bdev=bdev)
    monkeypatch.undo()
    ref = _ir_ref64(x, expand, dw, project, stride, True)
    got = y.permute(0, 3, 1, 2).double().cpu()
    err = (got[:2] - ref[:2]).abs().max().item()
    assert err < 2e-5 * (1.0 + ref.abs().max().item()), err
    case = fb.strips_case(inp, hid, oup, stride, H, True)
    assert torch.equal(case.x, x)
    fb.check(case, got, "ir_tile_x3 live", live=2)
    assert torch.equal(y[2].cpu(), torch.full_like(y[2].cpu(), sentinel))


@pytest.fixture(scope="module")
def mnet():
    from inference_arena_amd.models.zoo import make_mobilenet

    return make_mobilenet(1)


def test_classifier_program_matches_torch(mnet, device):
    """The classifier tensor program (bucket 4) on three 224 x 224 crops, under the tolerance of
    test_fp32_gpu.py::test_fp32_tensor_models_match_torch: its 56 x 56 and 28 x 28 blocks run the tiled kernels."""
    from inference_arena_amd.engine.pipeline import GpuTensorModel

    g = torch.Generator().manual_seed(11)
    c = torch.randn(3, 3, 224, 224, generator=g)
    cm = GpuTensorModel.mobilenet(mnet, device=0, buckets=[4], dtype="fp32")
    got = cm.infer(c.numpy())
    with torch.no_grad():
        ref = mnet.eval()(c).float().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-3 * np.abs(ref).max())


def test_stem_kernel_matches_torch(mnet, device):
    """Crop-fed classifier program (its first op is ir_stem_x3_kernel: crop gather + stem + block 1) on three
    224 x 224 uint8 crops (no resize: the gather is exact), same tolerance: the top-5 logits equal the torch
    logits of those classes, and the best class is a best class of the reference."""
    from inference_arena_amd.config import get_controlled_variable
    from inference_arena_amd.engine.pipeline import GpuClassifier
    from inference_arena_amd.engine.planner import BUF_NONE, OP_IRBLOCK

    rng = np.random.default_rng(3)
    crops = [rng.integers(0, 256, (224, 224, 3), dtype=np.uint8) for _ in range(3)]
    cls = GpuClassifier(mnet, device=0, buckets=[4], dtype="fp32")
    # the fused front end is the inverted-residual op without a source tensor (ProgramBuilder.ir_block_stem)
    assert any(int(op[0]) == OP_IRBLOCK and int(op[1]) == BUF_NONE for op in cls.program.ops), "no fused stem op"
    out = cls.infer(crops)
    mb = get_controlled_variable("preprocessing", "mobilenet")
    mean = torch.tensor(mb["mean"], dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(mb["std"], dtype=torch.float64).view(1, 3, 1, 1)
    x = torch.from_numpy(np.stack(crops)).permute(0, 3, 1, 2).double() / 255.0
    with torch.no_grad():
        ref = mnet.eval()(((x - mean) / std).float()).float().numpy()
    atol = 1e-3 * np.abs(ref).max()
    for (idx, logit, _), r in zip(out, ref):
        np.testing.assert_allclose(logit, r[idx.astype(np.int64)], rtol=1e-3, atol=atol)
        assert r[int(idx[0])] >= r.max() - 2 * atol

