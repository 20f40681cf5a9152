"""Detect-head tile gate on the GPU: the gated x3hg fused-1x1 kernel (ConvParams.gate) tile by tile, the gate as
a superset of what decode_kernel accepts, and whole pipelines with the gate on against the gate off."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from inference_arena_amd.ops import functional as AF
from inference_arena_amd.ops import native

pytestmark = pytest.mark.gpu

SENTINEL = 12288.0
BOX, CLS = 64, 80
# (impl, tile rows, tile columns): kF32X3HGPw + 0 = conv_x3hg_kernel<16, 4, 1, 1, 2, 2> (bucket 32's ops 48 / 51),
# kF32X3HGPwSmall + 0 = <8, 2, 1, 1, 2, 2> (bucket 1's)
VARIANTS = [(145, 8, 16), (181, 8, 8)]


def _conv_case(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, 64, generator=g)
    w = torch.randn(64, 64, 3, 3, generator=g) * 0.05
    b = torch.randn(64, generator=g) * 0.1
    w2 = torch.randn(BOX, 64, 1, 1, generator=g) * 0.1
    b2 = torch.randn(BOX, generator=g) * 0.1
    return x, w, b, w2, b2


def _run(case, D, impl, live, gate_min=None, packed=None):
    """The box conv into channels [0, 64) of D ([B, H, W, 144], class logits in [64, 144)), gated by them or dense."""
    x, w, b, w2, b2 = case
    bdev = torch.tensor([live], dtype=torch.int32, device=D.device)
    gate = None if gate_min is None else (D, BOX, CLS, gate_min)
    AF.conv2d_nhwc(x.to(D.device), w, b, act="silu", impl=impl, pw=(w2, b2), pw_out=D, gate=gate, bdev=bdev,
                   packed=packed)
    torch.cuda.synchronize()
    return D.cpu().numpy()


def _tiles(H, W, th, tw):
    return [(ty, tx) for ty in range((H + th - 1) // th) for tx in range((W + tw - 1) // tw)]


def _tile(a, ty, tx, th, tw):
    return a[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]


@pytest.mark.parametrize("impl,th,tw", VARIANTS)
def test_gated_tiles(impl, th, tw):
    """3x3 64 -> 64 with the 1x1 -> 64 epilogue on a 20 x 24 map, capacity 3 with 2 live images, the output
    pre-filled with a sentinel: kept tiles are bit-equal to the dense call, every other tile keeps the sentinel.  The
    8 x 16 tile is partial on both axes; 24 columns are three whole 8 x 8 tiles, so that variant is partial on the
    row axis only."""
    dev = torch.device("cuda:0")
    B, live, H, W = 3, 2, 20, 24
    gm = native().head_gate_min(0.5)
    gm32 = np.float32(gm)
    below = np.nextafter(gm32, np.float32(-np.inf))
    case = _conv_case(B, H, W, 1)
    ny, nx = (H + th - 1) // th, (W + tw - 1) // tw
    logits = np.full((B, H, W, CLS), -9.0, dtype=np.float32)
    # image 0
    logits[0, th - 1, tw - 1, CLS - 1] = gm32            # tile (0, 0): exactly gate_min at its last in-map corner
    logits[0, 2, tw + 3, 5] = below                      # tile (0, 1): one float32 below it
    logits[0, th + 1, 1, 17] = np.nan                    # tile (1, 0): NaN
    logits[0, th + 2, tw + 2, 40] = np.inf               # tile (1, 1): +inf
    logits[0, H - 1, W - 1, 0] = 3.0                     # the last tile, partial: hot only at the map's last pixel
    # image 1: hot at (row 1, column 0).  An unmasked read past the map's right edge in tile (0, last) of this image
    # would alias this pixel, and one past the bottom edge of image 0's tile (last, 0) would too
    logits[1, 1, 0, 0] = 0.25
    # image 2 is dead (live count 2): hot everywhere
    logits[2] = 5.0
    want = {(0, 0, 0): True, (0, 0, 1): False, (0, 1, 0): False, (0, 1, 1): True, (0, ny - 1, nx - 1): True,
            (0, ny - 1, 0): False, (1, 0, 0): True, (1, 0, nx - 1): False, (1, ny - 1, nx - 1): False}

    D = torch.full((B, H, W, BOX + CLS), SENTINEL, dtype=torch.float32)
    D[..., BOX:] = torch.from_numpy(logits)
    dense = _run(case, D.clone().to(dev), impl, live)
    gated = _run(case, D.clone().to(dev), impl, live, gate_min=gm)

    assert np.all(dense[:live, ..., :BOX] != SENTINEL) and np.all(np.isfinite(dense[:live, ..., :BOX]))
    for a in (dense, gated):
        assert np.array_equal(a[..., BOX:], logits, equal_nan=True)  # the class logits are only read
        assert np.all(a[live:, ..., :BOX] == SENTINEL)               # nothing of image 3 is written
    n_kept = 0
    for img in range(live):
        for ty, tx in _tiles(H, W, th, tw):
            keep = bool(np.any(_tile(logits[img], ty, tx, th, tw) >= gm32))  # NaN compares false
            if (img, ty, tx) in want:
                assert keep == want[(img, ty, tx)], (img, ty, tx)
            got, ref = _tile(gated[img], ty, tx, th, tw)[..., :BOX], _tile(dense[img], ty, tx, th, tw)[..., :BOX]
            if keep:
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (img, ty, tx)
            else:
                assert np.all(got == SENTINEL), (img, ty, tx)
            n_kept += keep
    assert n_kept == 4


@pytest.mark.parametrize("thr", [0.25, 0.5, 0.999])
def test_gate_keeps_every_anchor_decode_accepts(thr):
    """Class logits around the threshold, the float32 neighbours of logit(thr) among them, through decode_kernel
    and through the gated conv: every anchor decode accepts lies in a tile the gate keeps."""
    dev = torch.device("cuda:0")
    B, hw = 4, 20
    t32 = np.float32(thr)
    gm = native().head_gate_min(float(t32))
    logit = np.float32(np.log(np.float64(t32) / (1.0 - np.float64(t32))))
    rng = np.random.default_rng(7)
    logits = (-9.0 + rng.standard_normal((B, hw, hw, CLS)) * 0.5).astype(np.float32)
    ulps = 0
    for img in range(B):
        for by in range(3):  # 8 x 8 blocks: the tiles of one variant, halves of the other's
            for bx in range(3):
                kind = (img + by * 3 + bx) % 3
                y, x = by * 8 + int(rng.integers(0, 3)), bx * 8 + int(rng.integers(0, 2))  # (y + 1, x + 2) in the map
                c = int(rng.integers(0, CLS))
                if kind == 1:  # a near miss for the gate
                    logits[img, y, x, c] = np.float32(gm) - np.float32(rng.uniform(1e-4, 2.0 / 64))
                elif kind == 2:  # around logit(thr): random, and an exact neighbour k ulps away
                    logits[img, y, x, c] = logit + np.float32(rng.uniform(-1.0 / 64, 1.0 / 64))
                    v = logit
                    k = ulps % 7 - 3
                    for _ in range(abs(k)):
                        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
                    logits[img, y + 1, x + 2, (c + 1) % CLS] = v
                    ulps += 1
    head0 = torch.zeros(B, hw, hw, BOX + CLS)
    head0[..., BOX:] = torch.from_numpy(logits)
    small = torch.full((B, 4, 4, BOX + CLS), -20.0)
    heads = [head0.to(dev), small.to(dev), small.clone().to(dev)]
    cap = hw * hw + 32
    cand = torch.zeros((B * cap, 8), dtype=torch.int32, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    ctrl = AF.ctrl_tensor(B, dev)
    native().detect_decode({"head": [h.data_ptr() for h in heads], "hw": [hw, 4, 4], "xs": [BOX + CLS] * 3,
                            "strides": [8.0, 16.0, 32.0], "B": B, "conf_thr": float(t32), "cand": cand.data_ptr(),
                            "cand_count": cnt.data_ptr(), "cand_cap": cap, "ctrl": ctrl.data_ptr(), "f32": 1,
                            "stream": torch.cuda.current_stream().cuda_stream})
    torch.cuda.synchronize()
    cnt = cnt.cpu().numpy()
    rec = cand.cpu().numpy().reshape(B, cap, 8)
    accepted = [(img, int(a) // hw, int(a) % hw) for img in range(B) for a in rec[img, :cnt[img], 6]]
    assert all(a < hw * hw for img in range(B) for a in rec[img, :cnt[img], 6])
    assert 4 <= len(accepted) <= B * 9 * 2, len(accepted)

    case = _conv_case(B, hw, hw, 2)
    for impl, th, tw in VARIANTS:
        D = torch.full((B, hw, hw, BOX + CLS), SENTINEL, dtype=torch.float32)
        D[..., BOX:] = torch.from_numpy(logits)
        gated = _run(case, D.to(dev), impl, B, gate_min=gm)
        written = gated[..., 0] != SENTINEL
        for img, y, x in accepted:
            assert written[img, y, x], (impl, img, y, x, logits[img, y, x].max())
        tiles = [_tile(written[img], ty, tx, th, tw) for img in range(B) for ty, tx in _tiles(hw, hw, th, tw)]
        assert all(t.all() or not t.any() for t in tiles)
        assert any(not t.any() for t in tiles)  # and some tiles were skipped


def _images():
    from inference_arena_amd.data.synthetic import synthetic_images

    return synthetic_images(5, 11) + synthetic_images(1, 12, hw=(360, 520))  # the last one is not square


def _pipeline_results(gate: bool, **kw):
    from inference_arena_amd.engine.pipeline import GpuPipeline
    from inference_arena_amd.models.zoo import default_models

    C = native()
    before = C.get_head_gate()
    C.set_head_gate(gate)  # read when the buckets are captured
    try:
        pipe = GpuPipeline(*default_models(0), device=0, dtype="fp32", **kw)
    finally:
        C.set_head_gate(before)
    imgs = _images()
    res = pipe.infer(imgs)  # max batch 4: one full batch and one of two images
    if 1 in pipe.buckets:
        res += pipe.infer(imgs[:1])
    gated = {B: list(pipe.ex.gated_ops(B)) for B in pipe.buckets}
    order = {B: list(pipe.ex.exec_order(B)) for B in pipe.buckets}
    n_ops = len(pipe.program.ops)
    pairs = [tuple(p) for p in C.head_gate_pairs(pipe.program.ops)]
    del pipe
    return res, gated, order, n_ops, pairs


def _assert_same(on, off):
    assert len(on) == len(off)
    for a, b in zip(on, off):
        for key in ("boxes", "scores", "classes", "topk_idx", "topk_logit"):
            assert np.array_equal(getattr(a, key), getattr(b, key)), key
        assert a.det_count == b.det_count


def _check_order(gated, order, n_ops, pairs, on):
    for B, o in order.items():
        assert sorted(o) == list(range(n_ops))
        want = list(range(n_ops))
        for box in gated[B]:
            want[box], want[box + 1] = box + 1, box
        assert o == want
        assert set(gated[B]) <= {p[0] for p in pairs}
        if not on:
            assert gated[B] == []


def test_pipeline_gate_on_equals_off():
    on, g_on, o_on, n_ops, pairs = _pipeline_results(True, buckets=[1, 4])
    off, g_off, o_off, _, _ = _pipeline_results(False, buckets=[1, 4])
    _check_order(g_on, o_on, n_ops, pairs, True)
    _check_order(g_off, o_off, n_ops, pairs, False)
    assert g_on[1] == [p[0] for p in pairs]  # bucket 1 runs both box convs on x3hg fused-1x1 tiles
    assert sum(r.det_count for r in on) > 0
    _assert_same(on, off)


def test_pipeline_gate_many_tiles_marked(monkeypatch):
    monkeypatch.setenv("ARENA_TUNING", "off")  # no table entry for this program: the kernel defaults, no timing
    on, g_on, o_on, n_ops, pairs = _pipeline_results(True, buckets=[1, 4], conf_thr=0.001)
    off, g_off, _, _, _ = _pipeline_results(False, buckets=[1, 4], conf_thr=0.001)
    _check_order(g_on, o_on, n_ops, pairs, True)
    assert g_on[1] == [p[0] for p in pairs] and g_on[4] == g_on[1] and g_off[4] == []
    assert sum(r.det_count for r in on) > sum(1 for _ in on)
    _assert_same(on, off)


def test_pipeline_gate_staggered_capture():
    """Bucket 16 is captured as two graphs split at the default stagger point; the pairs lie inside one part."""
    on, g_on, o_on, n_ops, pairs = _pipeline_results(True, buckets=[16])
    off, _, _, _, _ = _pipeline_results(False, buckets=[16])
    _check_order(g_on, o_on, n_ops, pairs, True)
    assert g_on[16] == [p[0] for p in pairs]
    _assert_same(on, off)
