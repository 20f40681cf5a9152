"""The fused fp32 C3 bottleneck (csrc/kernels/c3_bneck_x3.hip) against fp64 torch at the fp32 arm's bounds
(fp32_bounds.py), and the fp32 detector with ``ARENA_C3_BNECK=1`` against the same program without it."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import fp32_bounds as fb
from inference_arena_amd.ops import functional as AF

pytestmark = pytest.mark.gpu
B, LIVE, X_COFF, Y_COFF = 3, 2, 8, 4  # source / destination: channel slices at these offsets of wider buffers


@functools.lru_cache(maxsize=None)
def _case(c, H, W, shortcut):
    """Inputs, weights and the fp64 reference with its variance (computed once per shape, never modified)."""
    g = torch.Generator().manual_seed(1000 * c + 10 * H + W + int(shortcut))
    xbuf = torch.randn(B, H, W, c + 16, generator=g, dtype=torch.float64).float()
    w1 = (torch.randn(c, c, 1, 1, generator=g, dtype=torch.float64) / c ** 0.5).float()
    b1 = (torch.randn(c, generator=g, dtype=torch.float64) * 0.1).float()
    w2 = (torch.randn(c, c, 3, 3, generator=g, dtype=torch.float64) / (9 * c) ** 0.5).float()
    b2 = (torch.randn(c, generator=g, dtype=torch.float64) * 0.1).float()
    ybuf = torch.randn(B, H, W, c + 12, generator=g)
    x = xbuf[..., X_COFF:X_COFF + c].permute(0, 3, 1, 2)
    case = fb.Case(f"c3bneck-{c}-{H}-{W}-{int(shortcut)}", "silu", x,
                   [dict(w=w1, b=b1, act="silu", begin=True),
                    dict(w=w2, b=b2, padding=1, act="silu", res=True if shortcut else None)])
    return case, xbuf, ybuf, (w1, b1), (w2, b2)


CASES = [(c, 20, 20, s, sc) for c in (32, 64, 128) for s in sorted({1, c // 32}) for sc in (True, False)]
CASES += [(64, H, W, s, True) for H, W in ((5, 7), (9, 17)) for s in (1, 2)]  # below a tile; one tile + 1 pixel
CASES += [(128, 20, 20, 0, True)]  # the launcher's own slice rule (18 workgroups: four slices)


@pytest.mark.parametrize("c,H,W,slices,shortcut", CASES)
def test_c3_bottleneck_matches_fp64(device, c, H, W, slices, shortcut):
    """Channel slices of wider buffers, a live count below the capacity, edge tiles masked in both directions, one
    slice and the split-K form: the written slice is the fp64 bottleneck, nothing else changes."""
    case, xbuf, ybuf, pw, conv3 = _case(c, H, W, shortcut)
    out = ybuf.clone().to(device)
    bdev = torch.tensor([LIVE], dtype=torch.int32, device=device)
    AF.c3_bottleneck_nhwc(xbuf.to(device), pw, conv3, shortcut=shortcut, x_coff=X_COFF, out=out, out_coff=Y_COFF,
                          bdev=bdev, slices=slices)
    got = out.cpu()
    assert torch.equal(got[LIVE:], ybuf[LIVE:])  # images at or past the live count
    assert torch.equal(got[..., :Y_COFF], ybuf[..., :Y_COFF])
    assert torch.equal(got[..., Y_COFF + c:], ybuf[..., Y_COFF + c:])
    nchw = got[:LIVE, ..., Y_COFF:Y_COFF + c].permute(0, 3, 1, 2).double()
    n = slices if slices else c // 32  # several slices: slices - 1 more fp32 adds in the reduce (fp32_bounds adds)
    ref = case.refs(n - 1)[0][:LIVE]
    err = (nchw - ref).abs().max().item()
    print(f"C3BNECK {case.key} slices {slices} max_err {err:.3e} max_ref {ref.abs().max().item():.3f}")
    assert err < 2e-5 * (1.0 + ref.abs().max().item()), err
    fb.check(case, nchw, f"slices {slices}", adds=n - 1, live=LIVE, listed=False)


def test_c3_bottleneck_refuses_overlap_and_other_widths(device):
    x = torch.zeros(1, 8, 16, 96, device=device)
    w = lambda c, k: (torch.zeros(c, c, k, k), torch.zeros(c))  # noqa: E731
    with pytest.raises(ValueError):  # out's channels [16, 48) meet the channels read, [0, 32)
        AF.c3_bottleneck_nhwc(x, w(32, 1), w(32, 3), shortcut=True, out=x, out_coff=16)
    with pytest.raises(ValueError):
        AF.c3_bottleneck_nhwc(x, w(48, 1), w(48, 3), shortcut=True)
    with pytest.raises(ValueError):
        AF.c3_bottleneck_nhwc(x.to(torch.bfloat16), w(32, 1), w(32, 3), shortcut=True)


def _iou(a, b):
    lt, rb = np.maximum(a[:, None, :2], b[None, :, :2]), np.minimum(a[:, None, 2:4], b[None, :, 2:4])
    inter = np.clip(rb - lt, 0, None).prod(-1)
    area = lambda t: (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])  # noqa: E731
    return inter / (area(a)[:, None] + area(b)[None, :] - inter + 1e-9)


def test_fp32_detector_with_fused_bottlenecks_matches_unfused(device, monkeypatch):
    """Buckets 1 and 4: equal detection counts and matched boxes with IoU > 0.99 (the criteria test_fp32_gpu.py
    holds the pipeline to against the reference); no bit-equality, the summation order differs."""
    from inference_arena_amd.data.synthetic import synthetic_images
    from inference_arena_amd.engine.pipeline import GpuDetector
    from inference_arena_amd.engine.planner import OP_C3BNECK
    from inference_arena_amd.models.zoo import make_yolo

    yolo = make_yolo(0, cls_shift=-20.0)
    imgs = synthetic_images(3, 61) + synthetic_images(1, 62, hw=(333, 500))
    monkeypatch.setenv("ARENA_TUNING", "off")  # no table entry for the fused program: kernel defaults, no timing
    monkeypatch.setenv("ARENA_C3_BNECK", "0")
    plain = GpuDetector(yolo, device=0, buckets=[1, 4], dtype="fp32")
    monkeypatch.setenv("ARENA_C3_BNECK", "1")
    fused = GpuDetector(yolo, device=0, buckets=[1, 4], dtype="fp32")
    assert int((fused.program.ops[:, 0] == OP_C3BNECK).sum()) == 10
    assert int((plain.program.ops[:, 0] == OP_C3BNECK).sum()) == 0
    n_det = 0
    for batch in (imgs[:1], imgs):
        for i, (a, b) in enumerate(zip(plain.infer(batch), fused.infer(batch))):
            assert len(a) == len(b), f"image {i} of {len(batch)}: {len(b)} detections vs {len(a)} unfused"
            if len(a):
                iou = _iou(a.boxes, b.boxes)
                assert iou.max(1).min() > 0.99, (i, iou.max(1).min())
                n_det += len(a)
    assert n_det >= 8, n_det
