"""The fused fp32 downsampling pair (x3ds, csrc/kernels/down_x3.hip: 3x3 stride 2 + SiLU + 1x1 + SiLU) against fp64
torch at the fp32 arm's bounds (fp32_bounds.py), and the fp32 detector with ``ARENA_DOWN_PW=1`` against the same
program without it.

Measured on MI355X: max z 5.0 .. 13.7 of 21.4, rms z 1.04 .. 2.50 of 3.26, per-element error at most 2.3e-6, the
same bits from every tile variant (profiles/down_pw/README.md)."""
from __future__ import annotations

import functools

import pytest
import torch

import fp32_bounds as fb
from inference_arena_amd.ops import functional as AF
from test_c3_bneck_gpu import _iou

pytestmark = pytest.mark.gpu
B, LIVE, X_COFF, Y_COFF = 3, 2, 8, 4  # source / destination: channel slices at these offsets of wider buffers
PAIRS = ((32, 64), (64, 128), (128, 256))
MAPS = ((9, 13), (18, 34), (40, 40))  # outputs 5x7 (below a tile, odd: pad taps live), 9x17 (tile + 1), 20x20
IMPLS = (0, 145, 146, 147)            # the launcher's rule and every tile variant


@functools.lru_cache(maxsize=None)
def _case(cin, c, H, W):
    """Inputs, weights and the fp64 reference with its variance (computed once per shape, never modified)."""
    g = torch.Generator().manual_seed(1000 * cin + 10 * H + W)
    xbuf = torch.randn(B, H, W, cin + 16, generator=g, dtype=torch.float64).float()
    w1 = (torch.randn(c, cin, 3, 3, generator=g, dtype=torch.float64) / (9 * cin) ** 0.5).float()
    b1 = (torch.randn(c, generator=g, dtype=torch.float64) * 0.1).float()
    w2 = (torch.randn(c, c, 1, 1, generator=g, dtype=torch.float64) / c ** 0.5).float()
    b2 = (torch.randn(c, generator=g, dtype=torch.float64) * 0.1).float()
    ybuf = torch.randn(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, c + 12, generator=g)
    x = xbuf[..., X_COFF:X_COFF + cin].permute(0, 3, 1, 2)
    case = fb.Case(f"x3ds-{cin}-{c}-{H}-{W}", "silu", x,
                   [dict(w=w1, b=b1, stride=2, padding=1, act="silu", begin=True), dict(w=w2, b=b2, act="silu")])
    return case, xbuf, ybuf, (w1, b1), (w2, b2)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("cin,c", PAIRS)
def test_down_x3_matches_fp64(device, cin, c, H, W, impl):
    """Channel slices of wider buffers, a live count below the capacity, edge tiles masked in both directions: the
    written slice is the fp64 pair, nothing else changes."""
    case, xbuf, ybuf, (w1, b1), pw = _case(cin, c, H, W)
    out = ybuf.clone().to(device)
    bdev = torch.tensor([LIVE], dtype=torch.int32, device=device)
    AF.conv2d_nhwc(xbuf.to(device), w1, b1, stride=2, act="silu", x_coff=X_COFF, cin=cin, pw=pw, pw_act="silu",
                   pw_out=out, pw_out_coff=Y_COFF, bdev=bdev, impl=impl)
    got = out.cpu()
    assert torch.equal(got[LIVE:], ybuf[LIVE:])  # images at or past the live count
    assert torch.equal(got[..., :Y_COFF], ybuf[..., :Y_COFF])
    assert torch.equal(got[..., Y_COFF + c:], ybuf[..., Y_COFF + c:])
    nchw = got[:LIVE, ..., Y_COFF:Y_COFF + c].permute(0, 3, 1, 2).double()
    ref, var = case.refs()[0][:LIVE], case.refs()[1][:LIVE]
    err = (nchw - ref).abs().max().item()
    mx, rms = fb.zstats(nchw, ref, var)
    print(f"X3DS {case.key} impl {impl} max_z {mx:.2f} rms_z {rms:.2f} max_err {err:.3e} "
          f"max_ref {ref.abs().max().item():.3f}")
    assert err < 2e-5 * (1.0 + ref.abs().max().item()), err
    fb.check(case, nchw, f"impl {impl}", live=LIVE, listed=False)


def test_down_x3_refusals(device):
    x = torch.zeros(1, 8, 16, 128, device=device)
    w = lambda co, ci, k: (torch.zeros(co, ci, k, k), torch.zeros(co))  # noqa: E731
    run = lambda x, w1, w2, **kw: AF.conv2d_nhwc(x, *w1, stride=2, act="silu", pw=w2, pw_act="silu",  # noqa: E731
                                                 cin=w1[0].shape[1], **kw)
    with pytest.raises(ValueError):
        run(x, w(64, 48, 3), w(64, 64, 1))
    with pytest.raises(ValueError):  # C2 != C
        run(x, w(64, 32, 3), w(32, 64, 1))
    with pytest.raises(ValueError):
        run(x.to(torch.bfloat16), w(64, 32, 3), w(64, 64, 1))
    with pytest.raises(ValueError):  # the output is the first half of the input's memory
        run(x, w(64, 32, 3), w(64, 64, 1), pw_out=x.view(-1)[:4 * 8 * 128].view(1, 4, 8, 128), pw_out_coff=64)
    with pytest.raises(ValueError):
        run(x, w(64, 32, 3), w(64, 64, 1), window=(0, 32))


def test_fp32_detector_with_fused_downsampling_matches_unfused(device, monkeypatch):
    """Buckets 1 and 4: equal detection counts and matched boxes with IoU > 0.99; no bit-equality, the summation
    order differs."""
    from inference_arena_amd.data.synthetic import synthetic_images
    from inference_arena_amd.engine.pipeline import GpuDetector
    from inference_arena_amd.models.zoo import make_yolo

    yolo = make_yolo(0, cls_shift=-20.0)
    imgs = synthetic_images(3, 61) + synthetic_images(1, 62, hw=(333, 500))
    monkeypatch.setenv("ARENA_TUNING", "off")  # no table entry for the fused program: kernel defaults, no timing
    monkeypatch.setenv("ARENA_DOWN_PW", "0")
    plain = GpuDetector(yolo, device=0, buckets=[1, 4], dtype="fp32")
    monkeypatch.setenv("ARENA_DOWN_PW", "1")
    fused = GpuDetector(yolo, device=0, buckets=[1, 4], dtype="fp32")
    assert len(fused.program.ops) == len(plain.program.ops) - 3
    n_det = 0
    for batch in (imgs[:1], imgs):
        for i, (a, b) in enumerate(zip(plain.infer(batch), fused.infer(batch))):
            assert len(a) == len(b), f"image {i} of {len(batch)}: {len(b)} detections vs {len(a)} unfused"
            if len(a):
                iou = _iou(a.boxes, b.boxes)
                assert iou.max(1).min() > 0.99, (i, iou.max(1).min())
                n_det += len(a)
    assert n_det >= 8, n_det
