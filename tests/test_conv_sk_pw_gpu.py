"""Split-K x3g on a fused-1x1 record (impl 171 + v with ``pw``; csrc/kernels/sk_pw_x3.hip: the Detect-head 1x1 is
applied to the reduced tile in the second pass) against fp64 torch at the fp32 arm's bounds (fp32_bounds.py), bit for
bit against the unfused split-K conv through an identity 1x1, under the tile gate, and in the fp32 detector."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp32_bounds as fb
from inference_arena_amd.ops import functional as AF
from test_c3_bneck_gpu import _iou
from test_fp32_gpu import _act64, _fp32_check, _nhwc

pytestmark = pytest.mark.gpu
IMPLS = tuple(range(171, 180))  # XG_SK_VARIANTS: 64 x 64, 128 x 32, 64 x 128 tiles by 2 / 4 / 8 splits


@functools.lru_cache(maxsize=None)
def _case(B, H, Cin, C):
    """The shared case with the coarse bound's reference and scale (computed once per shape, never modified)."""
    case = fb.pw_case(B, H, Cin, C)
    s3, s1 = case.stages
    x, w, b, w2, b2 = (t.double() for t in (case.x, s3["w"], s3["b"], s1["w"], s1["b"]))
    a = _act64(F.conv2d(x, w, b, padding=1), "silu")
    ref = F.conv2d(a, w2, b2)
    scale = F.conv2d(1.2 * F.conv2d(x.abs(), w.abs(), b.abs(), padding=1) + a.abs(), w2.abs(), b2.abs())
    return case, ref, scale


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("B,H,Cin,C", fb.PW)
def test_conv_sk_pw_matches_fp64(device, B, H, Cin, C, impl):
    """H 19: 722 pixels, a partial 64-pixel tile and a partial last image; C 80: five output fragments and a K padded
    to 96; Cin 144: 45 K chunks over 8 uneven splits."""
    case, ref, scale = _case(B, H, Cin, C)
    s3, s1 = case.stages
    y = AF.conv2d_nhwc(_nhwc(case.x).to(device), s3["w"], s3["b"], act="silu", impl=impl, pw=(s1["w"], s1["b"]))
    assert y.shape == (B, H, H, C)
    _fp32_check(y.permute(0, 3, 1, 2), ref, scale)
    fb.check(case, y.permute(0, 3, 1, 2), impl, adds=fb.sk_adds(impl, Cin, 3))


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("B,H,Cin,C", [fb.PW[0], fb.PW[1], (5, 58, 32, 64)])
def test_conv_sk_pw_identity_equals_unfused_split_k(device, B, H, Cin, C, impl):
    """W2 = I, b2 = 0, no second activation: of the six products l, m and h of the value remain, l + m is exact in
    fp32 and adding h restores the value.  So the output equals the unfused split-K conv's bit for bit, which pins the
    split order, the K-column permutation of the weight blob and the epilogue's channel mapping.  16 820 pixels: 263 tiles of
    64 pixels, at least one per CU, so the launcher takes the 64-pixel second-pass tile, with a partial last one."""
    case = fb.pw_case(B, H, Cin, C)
    w, b = case.stages[0]["w"], case.stages[0]["b"]
    x = _nhwc(case.x).to(device)
    packed = AF.pack_weights(w, b, device, "fp32")
    plain = AF.conv2d_nhwc(x, w, b, act="silu", packed=packed, impl=impl)
    fused = AF.conv2d_nhwc(x, w, b, act="silu", packed=packed, impl=impl,
                           pw=(torch.eye(C).reshape(C, C, 1, 1), torch.zeros(C)))
    torch.cuda.synchronize()
    assert torch.equal(fused, plain)


def test_conv_sk_pw_gate(device):
    """One passing logit: that pixel is written with the ungated bits; a pixel of the other image, more than 128
    linear pixels (the largest first-pass tile) away, keeps the sentinel."""
    B, H, Cin, C = fb.PW[0]
    case = _case(B, H, Cin, C)[0]
    s3, s1 = case.stages
    x = _nhwc(case.x).to(device)
    run = functools.partial(AF.conv2d_nhwc, x, s3["w"], s3["b"], act="silu", impl=172, pw=(s1["w"], s1["b"]))
    full = run()
    buf = torch.full((B, H, H, C + 80), -7.0, device=device)  # box channels, then the level's class logits
    buf[0, 3, 5, C + 17] = 0.5
    out = run(pw_out=buf, gate=(buf, C, 80, 0.0))
    torch.cuda.synchronize()
    assert torch.equal(out[0, 3, 5, :C], full[0, 3, 5])
    assert bool((out[1, H // 2:, :, :C] == -7.0).all())
    assert int((out[..., C:] == -7.0).sum()) == B * H * H * 80 - 1  # the logits themselves are only read


def test_fp32_detector_with_split_k_head_matches_tabled(device, tmp_path, monkeypatch):
    """Bucket 1: the four fused-1x1 head ops at 80 x 80 and 40 x 40 moved to impl 172.  Equal detection counts and
    matched boxes with IoU > 0.99 (test_down_x3_gpu.py's on / off criteria); the summation order differs."""
    from inference_arena_amd.data.synthetic import synthetic_images
    from inference_arena_amd.engine import tuning
    from inference_arena_amd.engine.pipeline import GpuDetector
    from inference_arena_amd.engine.planner import OP_CONV
    from inference_arena_amd.models.zoo import make_yolo

    yolo = make_yolo(0, cls_shift=-20.0)
    imgs = synthetic_images(3, 61) + synthetic_images(1, 62, hw=(333, 500))
    own = GpuDetector(yolo, device=0, buckets=[1], dtype="fp32")
    ops = np.asarray(own.program.ops)
    choices = list(own.ex.conv_choices(1))
    head = [i for i, r in enumerate(ops) if r[0] == OP_CONV and r[34] > 0 and r[19] == 1 and r[13] in (80, 40)]
    assert len(head) == 4, head
    for i in head:
        choices[i] = 172
    table = tmp_path / "tuning.json"
    assert tuning.store(own.program.ops, 1, choices, table)
    monkeypatch.setenv("ARENA_TUNING_FILE", str(table))
    monkeypatch.setenv("ARENA_TUNING", "table")
    split = GpuDetector(yolo, device=0, buckets=[1], dtype="fp32")
    assert split.tuning_source == "table" and [split.ex.conv_choices(1)[i] for i in head] == [172] * 4
    n_det = 0
    for img in imgs:
        (a,), (b,) = own.infer([img]), split.infer([img])
        assert len(a) == len(b), f"{len(b)} detections vs {len(a)}"
        if len(a):
            assert _iou(a.boxes, b.boxes).max(1).min() > 0.99
            n_det += len(a)
    assert n_det >= 8, n_det
