"""The fused bf16 front ends (csrc/kernels/stem_fused.hip) on their own, through ops.functional.stem_fused_nhwc.

Exact tests: with selector weights (one 1.0 per row, zero bias, no activation) every output channel is one bf16
value of the LDS s2d tile times 1.0, summed with zeros in fp32 and stored as bf16: bit for bit the s2d value at that
tap.  It must equal the bf16 output of the unfused op (letterbox_s2d, crop_gather_s2d) on the same pool, shifted by
the tap and zero outside the map; every tap is read, so the halo ring and the conv's padding are too.  The unfused
ops are pinned to the host preprocessor in test_fp32_gpu.py, test_kernels_gpu.py and test_detect_tail_gpu.py; the
letterbox and the unnormalised crops are compared with it here as well (a bf16 value k / 255 names its k).

Numeric tests: random weights at the models' scale and the real activations against fp64 references through
bf16_bounds.py: one rounding for the single-stage kernels, the three tiers for the kernels that keep bf16
intermediates in LDS.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_bounds as bb
import stem_cases as sc
from inference_arena_amd.ops import functional as AF
from inference_arena_amd.ops import native
from inference_arena_amd.processing.transforms import letterbox, resize_bilinear

pytestmark = pytest.mark.gpu

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
INV_STD = [1 / v for v in STD]
NORMS = {"imagenet": (MEAN, INV_STD), "unit": ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])}
_ENV: dict = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _sentinel(shape, device):
    return torch.full(shape, sc.SENTINEL, dtype=torch.int16, device=device).view(torch.bfloat16)


def _grey(s2d):
    """uint8 image [B, S, S, 3] that a [B, S/2, S/2, 16] bf16 tensor of k / 255 values holds."""
    B, h, w, _ = s2d.shape
    v = s2d[..., :12].double().reshape(B, h, w, 2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * w, 3)
    return torch.round(v * 255).to(torch.int64).numpy()


def lb_env(device, S, group):
    """Pool, records and control block of one letterbox group, and the unfused op's bf16 output (CPU, read-only) —
    built once per (S, group) and shared."""
    key = ("lb", S, group)
    if key not in _ENV:
        images = list(sc.letterbox_groups(S)[group])
        meta, pool = AF.image_pool(images, S, device)
        ctrl = AF.ctrl_tensor(sc.LIVE, device)
        out = _sentinel((sc.CAP, S // 2, S // 2, 16), device)
        native().letterbox_s2d({"pool": pool.data_ptr(), "meta": meta.data_ptr(), "ctrl": ctrl.data_ptr(),
                                "out": out.data_ptr(), "B": sc.CAP, "T": S, "f32": 0, "stream": _stream()})
        torch.cuda.synchronize()
        out = out.cpu()
        assert (_bits(out[sc.LIVE:]) == sc.SENTINEL).all()
        s2d = out[:sc.LIVE]
        # the expected value is itself the host preprocessor's: the same grey level at every pixel, tie image included
        grey = _grey(s2d)
        for i, im in enumerate(images):
            assert np.array_equal(grey[i], letterbox(im, S)[0]), (S, group, i, im.shape)
        _ENV[key] = {"pool": pool, "meta": meta, "ctrl": ctrl, "s2d": s2d, "images": images}
    return _ENV[key]


def crop_env(device, S, norm):
    """The same for the crops of stem_cases.crops(S): ctrl.crop_base = CROP_BASE, LIVE live crops of CAP."""
    key = ("crop", S, norm)
    if key not in _ENV:
        images = list(sc.crop_images(S))
        meta, pool = AF.image_pool(images, S, device)
        crops = torch.from_numpy(sc.pack_crops(S)).to(device)
        ctrl = AF.ctrl_tensor(len(images), device, n_crops=sc.LIVE, crop_base=sc.CROP_BASE)
        mean, inv_std = NORMS[norm]
        out = _sentinel((sc.CAP, S // 2, S // 2, 16), device)
        native().crop_gather_s2d({"pool": pool.data_ptr(), "meta": meta.data_ptr(), "crops": crops.data_ptr(),
                                  "ctrl": ctrl.data_ptr(), "out": out.data_ptr(), "cap": sc.CAP, "S": S, "mean": mean,
                                  "inv_std": inv_std, "f32": 0, "stream": _stream()})
        torch.cuda.synchronize()
        out = out.cpu()
        assert (_bits(out[sc.LIVE:]) == sc.SENTINEL).all()
        s2d = out[:sc.LIVE]
        if norm == "unit":  # k / 255 values: compare with the host resize of the crop (empty: 1 x 1 black)
            grey = _grey(s2d)
            for i, (im, x1, y1, x2, y2) in enumerate(sc.crops(S)[sc.CROP_BASE:sc.CROP_BASE + sc.LIVE]):
                c = images[im][y1:y2, x1:x2]
                want = resize_bilinear(c, S, S) if c.size else np.zeros((S, S, 3), np.uint8)
                assert np.array_equal(grey[i], want), (S, i, c.shape)
        _ENV[key] = {"pool": pool, "meta": meta, "ctrl": ctrl, "crops": crops, "s2d": s2d, "images": images,
                     "mean": mean, "inv_std": inv_std}
    return _ENV[key]


def _launch(env, S, stem, act, cdst, side, extra=4, **kw):
    """One launch into a sentinel-filled [CAP, side, side, cdst + extra] output -> the live items' channels
    (CPU); dead items and the channels past the output must keep the sentinel."""
    dev = env["pool"].device
    out = _sentinel((sc.CAP, side, side, cdst + extra), dev)
    if "crops" in env:
        kw.update(crops=env["crops"], mean=env["mean"], inv_std=env["inv_std"])
    AF.stem_fused_nhwc(env["pool"], env["meta"], env["ctrl"], stem, S=S, act=act, out=out, **kw)
    got = out.cpu()
    assert (_bits(got[sc.LIVE:]) == sc.SENTINEL).all(), "a dead item was written"
    assert (_bits(got[:sc.LIVE, ..., cdst:]) == sc.SENTINEL).all(), "channels past the output were written"
    return got[:sc.LIVE, ..., :cdst]


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    bad = g != w
    if bad.any():
        idx = bad.nonzero()
        per_item = bad.flatten(1).sum(1).tolist()
        first = idx[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} values differ (per item {per_item}); first at "
                             f"{first}: got {got[tuple(first)].item()!r} want {want[tuple(first)].item()!r}")


def _assert_paths(kernel, S, kinds):
    have = set().union(*kinds)
    assert {"staged", "global"} <= have, f"{kernel} S={S}: tiles are only {sorted(have)}"


def _lb_kinds(kernel, S, groups):
    return [set(sc.tile_kinds(kernel, S, image=im.shape[:2])) for g in groups for im in sc.letterbox_groups(S)[g]]


def _crop_kinds(kernel, S):
    return [set(sc.tile_kinds(kernel, S, crop=(x2 - x1, y2 - y1)))
            for _, x1, y1, x2, y2 in sc.crops(S)[sc.CROP_BASE:sc.CROP_BASE + sc.LIVE]]


ZERO16, ZERO32 = torch.zeros(16), torch.zeros(32)


# ------------------------------------------------------------------ exact: the s2d tile through selector weights
@pytest.mark.parametrize("S", [96, 80])
def test_detector_stem_tile_is_the_letterbox(device, S):
    """stem_fused_kernel<0, 3, 1, 8, 32>: output channel o of tap (kh, kw) is letterbox_s2d[Y + kh - 1, X + kw - 1, o]
    bit for bit, zero outside the map (channels 12..15: zero).  S = 96: a full and a partial tile column, 6 tile
    rows; S = 80: a partial column only.  Both groups of images, the tie image in the second (S = 96)."""
    _assert_paths("det", S, _lb_kinds("det", S, (0, 1)))
    for group in (0, 1):
        env = lb_env(device, S, group)
        for tap in range(9):
            w = sc.selector(16, 3, [(tap, o) for o in range(16)])
            got = _launch(env, S, (w, ZERO16), None, 16, S // 2)
            _same(got, sc.shifted(env["s2d"], tap // 3 - 1, tap % 3 - 1), f"S {S} group {group} tap {tap}")


# (stem tap, second-conv tap) pairs: every second tap with the centre stem tap, every stem tap with the centre
# second tap, and a diagonal
PAIRS = sorted({(t, 4) for t in range(9)} | {(4, t) for t in range(9)} | {(t, (2 * t + 1) % 9) for t in range(9)})


@pytest.mark.parametrize("S,pairs", [(64, [(a, b) for a in range(9) for b in range(9)]), (192, PAIRS)],
                         ids=["64", "192"])
def test_two_stage_detector_tiles_are_the_letterbox(device, S, pairs):
    """stem2_kernel<8, 16> with a selector stem (tap t1) and a selector second conv (tap t2), no activations:
    output channel o is letterbox_s2d[2y + kh2 - 1 + kh1 - 1, 2x + kw2 - 1 + kw1 - 1, o % 16] where the stem-output
    position (2y + kh2 - 1, 2x + kw2 - 1) lies inside the S/2 map, else zero: the stem-output tile's indexing and
    its zeroing outside the map.  S = 64: 1 x 2 tiles, all 81 pairs; S = 192: 3 x 6 tiles, the tie image."""
    groups = (0, 1) if S == 192 else (0,)
    _assert_paths("det2", S, _lb_kinds("det2", S, groups))
    for group in groups:
        env = lb_env(device, S, group)
        for t1, t2 in pairs:
            w1 = sc.selector(16, 3, [(t1, o) for o in range(16)])
            w2 = sc.selector(32, 3, [(t2, o % 16) for o in range(32)])
            got = _launch(env, S, (w1, ZERO16), None, 32, S // 4, second=(w2, ZERO32, None))
            stem_out = sc.shifted(env["s2d"], t1 // 3 - 1, t1 % 3 - 1)
            want = sc.shifted(stem_out, t2 // 3 - 1, t2 % 3 - 1, stride=2, out=S // 4)
            _same(got, torch.cat([want, want], -1), f"S {S} group {group} taps {t1}, {t2}")


@pytest.mark.parametrize("S", [96, 80])
def test_classifier_stem_tile_is_the_crop_gather(device, S):
    """stem_fused_kernel<1, 2, 2, 16, 16>: rows 0..15 copy tap t, rows 16..31 tap (t + 2) % 4 of crop_gather_s2d
    (ImageNet normalisation: the empty crop is (0 - mean) * inv_std), pad top / left 1.  S = 96: 3 x 3 tiles, the
    tie image; S = 80: partial tiles.  ctrl.crop_base = 2, 10 live crops of capacity 11."""
    _assert_paths("cls", S, _crop_kinds("cls", S))
    env = crop_env(device, S, "imagenet")
    for tap in range(4):
        taps = [tap] * 16 + [(tap + 2) % 4] * 16
        w = sc.selector(32, 2, [(taps[o], o % 16) for o in range(32)])
        got = _launch(env, S, (w, ZERO32), None, 32, S // 2)
        want = torch.cat([sc.shifted(env["s2d"], t // 2 - 1, t % 2 - 1) for t in (tap, (tap + 2) % 4)], -1)
        _same(got, want, f"S {S} tap {tap}")


# (stem tap, depthwise tap, project half): every depthwise tap, every stem tap, both halves of the 32 channels
IR_PICKS = sorted({(td % 4, td, td % 2) for td in range(9)} | {(ts, 4, h) for ts in range(4) for h in (0, 1)})


@pytest.mark.parametrize("S", [32, 96])
def test_classifier_block1_tiles_are_the_crop_gather(device, S):
    """stem_ir_kernel<16> with mean 0 and inv_std 1 (every value in [0, 1]: ReLU6 is the identity), a selector stem
    (rows 0..15 tap ts, rows 16..31 tap (ts + 1) % 4), depthwise weight 1.0 on tap td with zero bias, and a
    selector project of one half of the 32 channels: the output is crop_gather_s2d shifted by both taps, zero where
    the stem-output position lies outside the map.  S = 32: one tile whose four sides are map edges; S = 96: 3 x 3."""
    _assert_paths("ir", S, _crop_kinds("ir", S))
    env = crop_env(device, S, "unit")
    for ts, td, half in IR_PICKS:
        taps = [ts] * 16 + [(ts + 1) % 4] * 16
        w = sc.selector(32, 2, [(taps[o], o % 16) for o in range(32)])
        wd = torch.zeros(32, 1, 3, 3)
        wd[:, 0, td // 3, td % 3] = 1.0
        wp = torch.zeros(16, 32, 1, 1)
        wp[torch.arange(16), torch.arange(16) + 16 * half] = 1.0
        got = _launch(env, S, (w, ZERO32), "relu6", 16, S // 2, ir=((wd, ZERO32), (wp, ZERO16)))
        t = taps[16 * half]
        stem_out = sc.shifted(env["s2d"], t // 2 - 1, t % 2 - 1)
        _same(got, sc.shifted(stem_out, td // 3 - 1, td % 3 - 1), f"S {S} stem tap {t} dw tap {td} half {half}")


# ------------------------------------------------------------------ numeric: real weights against fp64
def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _weights(seed, cout, ks, gain):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, 16, ks, ks, generator=g) * gain / (12 * ks * ks) ** 0.5
    w[:, 12:] = 0  # the s2d input has 12 live channels
    return w, torch.randn(cout, generator=g) * 0.1


def _shares(pre64):
    return (pre64 > 6).double().mean().item(), (pre64 < 0).double().mean().item()


@pytest.mark.parametrize("S", [96, 80])
def test_detector_stem_bound(device, S):
    """Detector stem with SiLU on both image groups: one rounding (bf16_bounds.assert_bf16_once) against the fp64
    conv over the bf16 s2d values."""
    stem = _weights(S, 16, 3, 3.0)
    for group in (0, 1):
        env = lb_env(device, S, group)
        got = _launch(env, S, stem, "silu", 16, S // 2)
        ref, scale = bb.conv_refs(_nchw(env["s2d"]).double(), bb.bf64(stem[0]), stem[1].double(), padding=1,
                                  act="silu")
        worst = bb.assert_bf16_once(_nchw(got), ref, scale, what=f"detector stem S {S} group {group}")
        print(f"stem_fused-det-{S}-{group}: worst / bound {worst:.3f}")


@pytest.mark.parametrize("S", [96, 80])
def test_classifier_stem_bound(device, S):
    """Classifier stem with ReLU6 (pad top / left 1) over the normalised crops: one rounding; the weights' gain puts
    >= 0.5 % of the pre-activations above 6 and >= 10 % below 0, as the fp32 clamp tests ask."""
    stem = _weights(S + 1, 32, 2, 4.0)
    env = crop_env(device, S, "imagenet")
    got = _launch(env, S, stem, "relu6", 32, S // 2)
    x = F.pad(_nchw(env["s2d"]).double(), (1, 0, 1, 0))
    w64, b64 = bb.bf64(stem[0]), stem[1].double()
    hi, lo = _shares(F.conv2d(x, w64, b64))
    assert hi >= 0.005 and lo >= 0.10, (hi, lo)
    ref, scale = bb.conv_refs(x, w64, b64, act="relu6")
    worst = bb.assert_bf16_once(_nchw(got), ref, scale, what=f"classifier stem S {S}")
    print(f"stem_fused-cls-{S}: worst / bound {worst:.3f}; above 6: {hi:.4f}, below 0: {lo:.4f}")


def _fused(name, got, refs, emu):
    flips, rms = bb.fused_stats(emu, refs[2], refs[3])
    r = bb.assert_bf16_fused(got, *refs, bb.flip_cap(flips), rms, what=name)
    print(f'    "{name}": ({flips:.3g}, {rms:.4f}, {r["flips"]:.3g}, {r["rms"]:.4f}, {r["worst"]:.3f}),')


@pytest.mark.parametrize("S", [64, 192])
def test_two_stage_detector_bounds(device, S):
    """stem2_kernel keeps the SiLU stem output as bf16 in LDS: the three tiers of assert_bf16_fused against
    stem2_refs / stem2_emulate."""
    stem = _weights(S, 16, 3, 3.0)
    g = torch.Generator().manual_seed(S + 7)
    second = (torch.randn(32, 16, 3, 3, generator=g) / 12.0, torch.randn(32, generator=g) * 0.1)
    env = lb_env(device, S, 0)
    got = _launch(env, S, stem, "silu", 32, S // 4, second=(second[0], second[1], "silu"))
    x = _nchw(env["s2d"]).float()
    _fused(f"stem2-{S}", _nchw(got), bb.stem2_refs(x, stem, second), bb.stem2_emulate(x, stem, second))


@pytest.mark.parametrize("S", [32, 96])
def test_classifier_block1_bounds(device, S):
    """stem_ir_kernel keeps the ReLU6 stem output and the depthwise output as bf16 in LDS.  The 2 x 2 stem over the
    s2d map (pad top / left 1) is a 1 x 1 conv over its four taps stacked on the channel axis, so the kernel is
    ir_refs / ir_emulate's expand -> depthwise -> project chain with the stem as the expand conv: all three stores
    are modelled (expand=None would take the stem output as exact).  Both ReLU6 stages reach the clamp."""
    stem = _weights(S + 2, 32, 2, 4.0)
    g = torch.Generator().manual_seed(S + 9)
    dw = (torch.randn(32, 1, 3, 3, generator=g) * 0.6, torch.randn(32, generator=g) * 0.1)
    project = (torch.randn(16, 32, 1, 1, generator=g) / 32 ** 0.5, torch.randn(16, generator=g) * 0.1)
    env = crop_env(device, S, "imagenet")
    got = _launch(env, S, stem, "relu6", 16, S // 2, ir=(dw, project))
    xp = F.pad(_nchw(env["s2d"]).float(), (1, 0, 1, 0))
    S2 = S // 2
    x4 = torch.cat([xp[:, :, kh:kh + S2, kw:kw + S2] for kh in (0, 1) for kw in (0, 1)], 1)  # [B, 64, S2, S2]
    expand = (stem[0].permute(0, 2, 3, 1).reshape(32, 64, 1, 1).contiguous(), stem[1])
    he = F.conv2d(x4.double(), bb.bf64(expand[0]), expand[1].double())
    hd = F.conv2d(he.clamp(0, 6), bb.bf64(dw[0]), dw[1].double(), padding=1, groups=32)
    for hi, lo in (_shares(he), _shares(hd)):
        assert hi >= 0.005 and lo >= 0.10, (hi, lo)
    _fused(f"stem_ir-{S}", _nchw(got), bb.ir_refs(x4, expand, dw, project, 1, False),
           bb.ir_emulate(x4, expand, dw, project, 1, False))
