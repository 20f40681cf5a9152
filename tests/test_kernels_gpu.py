"""HIP bf16 kernels vs fp64 references of the same op on the bf16-rounded operands (MI355X only).

Kernels that round once (one bf16 store after an fp32 epilogue) are held to the half-ulp bound of
bf16_bounds.assert_bf16_once on every element; the fused kernels with bf16 intermediates to the three tiers of
bf16_bounds.assert_bf16_fused, next to the looser share-based check they had before (``_check``): tier 1's
propagated bound can exceed it on single elements.  test_bf16_bounds.py shows on the CPU what these bounds reject.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_bounds as bb
import tie_image as ti
from inference_arena_amd.ops import functional as AF
from inference_arena_amd.ops import native

pytestmark = pytest.mark.gpu


def _bf(t):
    return t.to(torch.bfloat16).float()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).float()


def _check(got, ref, rtol=2e-2, atol=2e-2):
    err = (got.float() - ref.float()).abs()
    tol = atol + rtol * ref.float().abs()
    bad = (err > tol).float().mean().item()
    assert bad < 1e-3, f"{bad*100:.3f}% elements out of tolerance; max err {err.max().item():.4g}"


def _once(got_nchw, x_nhwc, w, b, stride, pad, act, res=None, groups=1, f32out=False, what=""):
    """Single-rounding bound of act(conv(x, w) + b) (+ res): ``x_nhwc`` / ``res`` the bf16 tensors the kernel read
    (on the host), ``w`` the fp32 weights it rounds to bf16, ``b`` its fp32 bias."""
    ref, scale = bb.conv_refs(_nchw(x_nhwc).double(), bb.bf64(w), b.float().double(), stride=stride, padding=pad,
                              act=act, res64=None if res is None else _nchw(res).double(), groups=groups)
    return bb.assert_bf16_once(got_nchw, ref, scale, f32out=f32out, what=what)


def _fused_ir(got_nchw, x_nhwc, expand, dw, project, stride, res, what, refs=None):
    """Three-tier bound of one inverted residual (bf16_bounds.ir_refs; flip share and rms ratio capped against the
    CPU emulation on the same inputs) and the share-based check these tests had before.  -> refs, for a second
    kernel on the same inputs."""
    x = _nchw(x_nhwc)
    if refs is None:
        r4 = bb.ir_refs(x, expand, dw, project, stride, res)
        flips, rms = bb.fused_stats(bb.ir_emulate(x, expand, dw, project, stride, res), r4[2], r4[3])
        refs = (r4, flips, rms)
    r4, flips, rms = refs
    r = bb.assert_bf16_fused(got_nchw, *r4, bb.flip_cap(flips), rms, what=what)
    print(f"{what}: emulation flips {flips:.3g} rms {rms:.4f}; kernel flips {r['flips']:.3g} rms {r['rms']:.4f} "
          f"worst {r['worst']:.3f}")
    _check(got_nchw, _ref_ir(x_nhwc, expand, dw, project, stride, res), rtol=3e-2, atol=3e-2)
    return refs


def test_native_loaded():
    C = native()
    assert C.SIZEOF_IMAGE_META == 48 and C.SIZEOF_CANDIDATE == 32 and C.SIZEOF_TOPK == 64


@pytest.fixture(params=[2, 1, 3], ids=["lds", "direct", "igemm"])
def conv_impl(request):
    C = native()
    old = C.get_conv_impl()
    C.set_conv_impl(request.param)
    yield request.param
    C.set_conv_impl(old)


@pytest.mark.parametrize(
    "B,H,Cin,Cout,k,s,act",
    [
        (2, 40, 32, 64, 3, 1, "silu"),
        (2, 40, 64, 128, 3, 2, "silu"),
        (1, 80, 16, 32, 3, 2, "silu"),  # Cin=16: k-groups straddle taps
        (3, 20, 256, 128, 1, 1, "silu"),
        (2, 28, 32, 144, 1, 1, "relu6"),  # 9 channel tiles (WC=3)
        (1, 20, 80, 80, 3, 1, "silu"),  # Cin=80, Cout=80 (WC=5)
        (2, 14, 96, 24, 1, 1, None),
        (1, 7, 320, 1280, 1, 1, "relu6"),
        (3, 20, 128, 64, 3, 2, "silu"),  # stride-2 tile with a partial column tile
        (2, 27, 64, 48, 3, 1, None),  # odd spatial size, 3 channel tiles
        (1, 20, 256, 144, 3, 1, "silu"),  # 8 input-channel slices
    ],
)
def test_conv_matches_torch(device, conv_impl, B, H, Cin, Cout, k, s, act):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + Cin)
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g) * 0.1
    xn = _nhwc(x).to(torch.bfloat16).to(device)
    y = AF.conv2d_nhwc(xn, w, b, stride=s, act=act)
    _once(_nchw(y.cpu()), xn.cpu(), w, b, s, k // 2, act, what="conv")


# The smallest shapes at which tiling can still go wrong: (B, H, W, Cin, Cout, k, s, act, res, up)
SMALL_CONVS = [
    (2, 5, 5, 8, 4, 3, 1, "silu", False, False),     # the smallest legal channel counts
    (3, 1, 1, 16, 8, 3, 1, "silu", False, False),    # 3x3 over a 1x1 map: every tap but the centre is padding
    (2, 6, 19, 16, 20, 3, 1, "silu", False, False),  # non-square map, a partial column tile, Cout 20
    (2, 7, 7, 32, 16, 3, 2, "silu", False, False),   # stride 2 on an odd map (7 -> 4)
    (2, 3, 3, 40, 20, 1, 1, "relu6", False, False),  # 1x1 with partial K slab and channel tile
    (2, 5, 5, 16, 16, 3, 1, "silu", True, True),     # residual and the 2x upsampled copy
    (2, 5, 5, 16, 16, 1, 1, None, True, True),
]


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,s,act,res,up", SMALL_CONVS)
def test_conv_small_shapes(device, conv_impl, B, H, W, Cin, Cout, k, s, act, res, up):
    """Every conv family takes these shapes itself or hands them to one that does: a refusal would raise here."""
    g = torch.Generator().manual_seed(H * 100 + W + Cin + Cout)
    x = torch.randn(B, H, W, Cin, generator=g).to(torch.bfloat16)
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g) * 0.1
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    r = torch.randn(B, Ho, Wo, Cout, generator=g).to(torch.bfloat16) if res else None
    out = torch.full((B, Ho, Wo, Cout + 16), -7.0, dtype=torch.bfloat16, device=device)
    out2 = torch.full((B, 2 * Ho, 2 * Wo, Cout + 16), -7.0, dtype=torch.bfloat16, device=device) if up else None
    AF.conv2d_nhwc(x.to(device), w, b, stride=s, act=act, res=r.to(device) if res else None, out=out, out_coff=8,
                   out2=out2, out2_coff=8)
    torch.cuda.synchronize()
    o = out.cpu()
    _once(_nchw(o[..., 8:8 + Cout]), x, w, b, s, k // 2, act, res=r, what="small conv")
    assert torch.all(o[..., :8] == -7.0) and torch.all(o[..., 8 + Cout:] == -7.0)
    if up:
        o2 = out2.cpu()
        assert torch.equal(o2[..., 8:8 + Cout], o[..., 8:8 + Cout].repeat_interleave(2, 1).repeat_interleave(2, 2))
        assert torch.all(o2[..., :8] == -7.0) and torch.all(o2[..., 8 + Cout:] == -7.0)


def test_conv_slices_residual_upsample(device, conv_impl):
    g = torch.Generator().manual_seed(7)
    B, H, Cbuf, Cin, Cout = 2, 20, 96, 32, 48
    buf = torch.randn(B, H, H, Cbuf, generator=g).to(torch.bfloat16).to(device)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g) * 0.1
    out = torch.zeros(B, H, H, 128, dtype=torch.bfloat16, device=device)
    res_buf = torch.randn(B, H, H, 64, generator=g).to(torch.bfloat16).to(device)
    up = torch.zeros(B, 2 * H, 2 * H, 64, dtype=torch.bfloat16, device=device)
    AF.conv2d_nhwc(buf, w, b, act="silu", x_coff=16, cin=Cin, out=out, out_coff=64, res=res_buf, res_coff=8,
                   out2=up, out2_coff=8)
    torch.cuda.synchronize()
    xs = buf.cpu()[..., 16:16 + Cin]
    _once(_nchw(out.cpu()[..., 64:64 + Cout]), xs, w, b, 1, 1, "silu", res=res_buf.cpu()[..., 8:8 + Cout],
          what="conv slices")
    assert out.cpu()[..., :64].abs().sum() == 0 and out.cpu()[..., 64 + Cout:].abs().sum() == 0
    upref = F.interpolate(_nchw(out.cpu()[..., 64:64 + Cout]), scale_factor=2, mode="nearest")
    assert torch.equal(_nchw(up.cpu()[..., 8:8 + Cout]), upref)


def test_conv_fp32_out_and_live_batch(device, conv_impl):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 1, 1, 1280, generator=g).to(torch.bfloat16).to(device)
    w = torch.randn(1000, 1280, 1, 1, generator=g) / np.sqrt(1280)
    b = torch.randn(1000, generator=g)
    out = torch.full((6, 1, 1, 1000), -7.0, dtype=torch.float32, device=device)
    bdev = torch.tensor([4], dtype=torch.int32, device=device)
    AF.conv2d_nhwc(x, w, b, act=None, f32out=True, out=out, bdev=bdev)
    torch.cuda.synchronize()
    _once(_nchw(out.cpu())[:4], x.cpu()[:4], w, b, 1, 0, None, f32out=True, what="fp32-out conv")
    assert torch.all(out.cpu()[4:] == -7.0), "rows past the live batch must not be written"


def test_stem_s2d_equivalence(device, conv_impl):
    from inference_arena_amd.engine.plans import s2d_stem_3x3, s2d_stem_6x6

    g = torch.Generator().manual_seed(11)
    img = torch.rand(2, 3, 64, 64, generator=g)
    s2d = img.reshape(2, 3, 32, 2, 32, 2).permute(0, 2, 4, 3, 5, 1).reshape(2, 32, 32, 12)
    s2d = torch.cat([s2d, torch.zeros(2, 32, 32, 4)], -1).to(torch.bfloat16)
    xin = s2d.to(device)
    w6 = torch.randn(16, 3, 6, 6, generator=g) * 0.2
    b = torch.zeros(16)
    y = AF.conv2d_nhwc(xin, s2d_stem_6x6(w6), b, act=None)
    img_nhwc = _nhwc(img).to(torch.bfloat16)  # the values the s2d tensor holds
    _once(_nchw(y.cpu()), img_nhwc, w6, b, 2, 2, None, what="s2d 6x6 stem")
    w3 = torch.randn(32, 3, 3, 3, generator=g) * 0.2
    y3 = AF.conv2d_nhwc(xin, s2d_stem_3x3(w3), torch.zeros(32), pad=(1, 1), act=None, out_hw=(32, 32))
    _once(_nchw(y3.cpu()), img_nhwc, w3, torch.zeros(32), 2, 1, None, what="s2d 3x3 stem")


@pytest.mark.parametrize("C,H,s", [(96, 56, 2), (144, 28, 1), (960, 7, 1), (32, 112, 1)])
def test_dwconv_matches_torch(device, C, H, s):
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(2, C, H, H, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.3
    b = torch.randn(C, generator=g) * 0.1
    xn = _nhwc(x).to(torch.bfloat16).to(device)
    y = AF.dwconv3x3_nhwc(xn, w, b, stride=s, act="relu6")
    _once(_nchw(y.cpu()), xn.cpu(), w, b, s, 1, "relu6", groups=C, what="dwconv")


def test_sppf_matches_torch(device):
    g = torch.Generator().manual_seed(5)
    C = 128
    buf = torch.zeros(2, 20, 20, 4 * C, dtype=torch.bfloat16)
    buf[..., :C] = torch.randn(2, 20, 20, C, generator=g).to(torch.bfloat16)
    d = buf.to(device)
    AF.sppf_nhwc(d, C)
    torch.cuda.synchronize()
    x = _nchw(buf[..., :C])
    y1 = F.max_pool2d(x, 5, 1, 2)
    y2 = F.max_pool2d(y1, 5, 1, 2)
    y3 = F.max_pool2d(y2, 5, 1, 2)
    got = _nchw(d.cpu())
    for i, ref in enumerate((y1, y2, y3)):
        assert torch.equal(got[:, (i + 1) * C:(i + 2) * C], ref)


def test_letterbox_matches_host(device):
    from inference_arena_amd.data.synthetic import synthetic_images
    from inference_arena_amd.processing import letterbox

    imgs = synthetic_images(3, 5) + [np.random.default_rng(0).integers(0, 255, (300, 1000, 3), dtype=np.uint8)]
    imgs.append(np.array(ti.tie_image(1344, 84, 640, 40, 0, 1)))  # resized samples on uint8 rounding ties
    out = AF.letterbox_s2d(imgs, 640, device)
    got = AF.s2d_to_nchw(out.cpu())
    for i, im in enumerate(imgs):
        ref = torch.from_numpy(letterbox(im, 640)[0].astype(np.float32).transpose(2, 0, 1) / 255.0)
        err = (got[i] - ref).abs()
        # bf16 storage (~3 significant digits) + at most one uint8 rounding step
        assert (err <= 1.0 / 255 + 4e-3).float().mean() > 0.999, err.max()
        assert err.max() < 3.0 / 255 + 4e-3
    # against the fp32 form of the same kernel (pinned to the host bit for bit in test_fp32_gpu.py): the two share
    # the sampling and differ in the normalisation alone (v * (1 / 255) here, v / 255 there: within 2^-22 of each
    # other) and in the store, so the bf16 value is within half a bf16 ulp of the fp32 one
    f32 = AF.letterbox_s2d(imgs, 640, device, dtype=torch.float32).double().cpu()
    worst = ((out.double().cpu() - f32).abs() / ((2.0 ** -8 + 2.0 ** -22) * f32.abs() + 1e-30)).max().item()
    assert worst <= 1.0, worst
    assert torch.equal(out[..., 12:].cpu().float(), torch.zeros(len(imgs), 320, 320, 4))


def test_topk_and_avgpool(device):
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(37, 1000, generator=g) * 3
    idx, lg, pr = AF.topk_softmax(logits.to(device))
    ref_v, ref_i = torch.topk(logits, 5, dim=1)
    assert torch.equal(idx.long(), ref_i)
    assert torch.allclose(lg, ref_v)
    assert torch.allclose(pr, torch.softmax(logits, 1).gather(1, ref_i), rtol=1e-4, atol=1e-6)
    # ties resolve to the lowest index (register path, N <= 1024) and the streaming path (N > 1024)
    for N in (1000, 77, 1500):
        t = torch.randint(0, 6, (9, N), generator=g).float()
        idx, lg, _ = AF.topk_softmax(t.to(device))
        order = np.lexsort((np.arange(N)[None, :].repeat(9, 0), -t.numpy()), axis=1)[:, :5]
        assert np.array_equal(idx.cpu().numpy(), order), N
        assert torch.equal(lg.cpu(), t.gather(1, torch.from_numpy(order)))
    x = torch.randn(5, 7, 7, 1280, generator=g).to(torch.bfloat16)
    y = AF.avgpool_nhwc(x.to(device))
    torch.cuda.synchronize()
    x64 = x.double()  # fp32 sum of bf16 values, * 1 / HW, one bf16 store
    bb.assert_bf16_once(y.cpu(), x64.mean((1, 2)), x64.abs().mean((1, 2)), what="avgpool")


def _ref_ir(x_nhwc, expand, dw, project, stride, res):
    """fp32 torch reference of one inverted residual on bf16-rounded operands."""
    x = _nchw(x_nhwc).float()
    h = x
    if expand is not None:
        h = F.relu6(F.conv2d(h, _bf(expand[0]), expand[1].float()))
        h = _bf(h)  # the kernel stores the expanded tile as bf16
    hid = dw[0].shape[0]
    h = F.relu6(F.conv2d(h, _bf(dw[0]), dw[1].float(), stride=stride, padding=1, groups=hid))
    h = _bf(h)
    y = F.conv2d(h, _bf(project[0]), project[1].float())
    return y + x if res else y


@pytest.mark.parametrize(
    "B,H,inp,hid,oup,s,res",
    [
        (2, 112, 32, 32, 16, 1, False),   # block 1: no expand
        (2, 112, 16, 96, 24, 2, False),   # block 2: 112 -> 56
        (2, 56, 24, 144, 24, 1, True),    # hidden 144 padded to 160
        (1, 56, 24, 144, 32, 2, False),
        (2, 28, 32, 192, 32, 1, True),
        (1, 28, 32, 192, 64, 2, False),
        (3, 14, 64, 384, 96, 1, False),
        (1, 14, 96, 576, 160, 2, False),
        (2, 7, 160, 960, 160, 1, True),
        (2, 7, 160, 960, 320, 1, False),
        (1, 20, 24, 144, 24, 1, True),    # partial 8x8 tiles are not used at 20 -> 7x7 tiles, partial edge
    ],
)
def test_ir_block_matches_torch(device, B, H, inp, hid, oup, s, res):
    g = torch.Generator().manual_seed(H * 100 + inp + oup)
    x = (torch.rand(B, inp, H, H, generator=g) * 2).to(torch.bfloat16)
    expand = None if hid == inp and H == 112 and inp == 32 else (
        torch.randn(hid, inp, 1, 1, generator=g) / np.sqrt(inp), torch.randn(hid, generator=g) * 0.1)
    dw = (torch.randn(hid, 1, 3, 3, generator=g) / 3, torch.randn(hid, generator=g) * 0.1)
    project = (torch.randn(oup, hid, 1, 1, generator=g) / np.sqrt(hid), torch.randn(oup, generator=g) * 0.1)
    xn = _nhwc(x).to(device)
    y = AF.ir_block_nhwc(xn, expand, dw, project, stride=s, res=res)
    _fused_ir(_nchw(y.cpu()), xn.cpu(), expand, dw, project, s, res, f"ir_block-{B}-{H}-{inp}-{hid}-{oup}-{s}")


@pytest.mark.parametrize("B,HW,live", [(3, 7, None), (5, 7, 3), (2, 8, None)])
def test_head_pool_matches_torch(device, B, HW, live):
    """Fused head 1x1 conv (320 -> 1280) + ReLU6 + global average pool vs fp32 torch; crops past the
    device-side live count are not written."""
    g = torch.Generator().manual_seed(B * 10 + HW)
    x = (torch.rand(B, 320, HW, HW, generator=g) * 2).to(torch.bfloat16)
    w = torch.randn(1280, 320, 1, 1, generator=g) / np.sqrt(320)
    b = torch.randn(1280, generator=g) * 0.5
    xn = _nhwc(x).to(device)
    bdev = None if live is None else torch.tensor([live], dtype=torch.int32, device=device)
    y = torch.full((B, 1280), -7.0, dtype=torch.bfloat16, device=device)
    y = AF.head_pool_nhwc(xn, w, b, "relu6", bdev=bdev, out=y)
    # per-pixel conv + ReLU6 in fp32, summed over the pixels in fp32, * 1 / HW, one bf16 store (head_pool.hip)
    ref, scale = bb.conv_refs(x.double(), bb.bf64(w), b.double(), act="relu6")
    n = B if live is None else live
    bb.assert_bf16_once(y[:n].cpu(), ref.mean(dim=(2, 3))[:n], scale.mean(dim=(2, 3))[:n], what="head_pool")
    assert torch.all(y[n:].cpu() == -7.0), "crops past the live count must not be written"


@pytest.mark.parametrize("B,live,f32", [(37, None, True), (20, 9, True), (16, None, False)])
def test_fc_splitk_matches_torch(device, B, live, f32):
    """Classifier FC (1x1 conv on a 1x1 map, 1280 -> 1000) on the split-K kernel vs fp32 torch."""
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 1280, 1, 1, generator=g).to(torch.bfloat16)
    w = torch.randn(1000, 1280, 1, 1, generator=g) / np.sqrt(1280)
    b = torch.randn(1000, generator=g)
    bdev = None if live is None else torch.tensor([live], dtype=torch.int32, device=device)
    y = AF.conv2d_nhwc(_nhwc(x).to(device), w, b, f32out=f32, bdev=bdev)
    n = B if live is None else live
    _once(_nchw(y.cpu())[:n], _nhwc(x)[:n], w, b, 1, 0, None, f32out=f32, what="fc_splitk")


@pytest.mark.parametrize("f32", [True, False], ids=["f32out", "bf16out"])
@pytest.mark.parametrize("B,live", [(17, None), (32, 16), (32, 17)])
def test_fc_splitk_crop_tiles(device, B, live, f32):
    """The 16-crop tiles of fc_splitk.hip: B 17 is two tiles, the second with one live row; a device-side live
    count of 16 ends at a tile border, 17 one row past it.  Cout 1000: the last 32-class tile holds 8.  Rows past
    the live count keep their contents."""
    g = torch.Generator().manual_seed(B * 3 + (live or 0))
    x = torch.randn(B, 1, 1, 1280, generator=g).to(torch.bfloat16)
    w = torch.randn(1000, 1280, 1, 1, generator=g) / np.sqrt(1280)
    b = torch.randn(1000, generator=g)
    out = torch.full((B, 1, 1, 1000), -7.0, dtype=torch.float32 if f32 else torch.bfloat16, device=device)
    bdev = None if live is None else torch.tensor([live], dtype=torch.int32, device=device)
    AF.conv2d_nhwc(x.to(device), w, b, f32out=f32, out=out, bdev=bdev)
    torch.cuda.synchronize()
    n = B if live is None else live
    _once(_nchw(out.cpu())[:n], x[:n], w, b, 1, 0, None, f32out=f32, what="fc_splitk tiles")
    assert torch.all(out.cpu()[n:] == -7.0), "rows past the live count must not be written"


def test_ir_block_live_batch(device):
    """Crops past the device-side live count are not written."""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(4, 28, 28, 32, generator=g).to(torch.bfloat16).to(device)
    expand = (torch.randn(192, 32, 1, 1, generator=g) / 6, torch.zeros(192))
    dw = (torch.randn(192, 1, 3, 3, generator=g) / 3, torch.zeros(192))
    project = (torch.randn(64, 192, 1, 1, generator=g) / 14, torch.zeros(64))
    bdev = torch.tensor([2], dtype=torch.int32, device=device)
    y = AF.ir_block_nhwc(x, expand, dw, project, stride=2, bdev=bdev)
    full = AF.ir_block_nhwc(x, expand, dw, project, stride=2)
    assert torch.equal(y[:2].cpu(), full[:2].cpu())


@pytest.mark.parametrize(
    "B,H,Cin,Cout",
    [(2, 40, 64, 64), (2, 40, 128, 64), (1, 20, 80, 80), (2, 14, 64, 384), (2, 14, 96, 576), (2, 7, 160, 960),
     (2, 20, 256, 256), (3, 20, 128, 128), (2, 33, 16, 16), (2, 30, 32, 32), (1, 14, 384, 96)],
)
def test_pointwise_fast_path(device, B, H, Cin, Cout):
    """1x1 fast path (conv_pw.hip) vs torch, with residual; and identical to the generic kernel."""
    C = native()
    g = torch.Generator().manual_seed(Cin * 7 + Cout)
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / np.sqrt(Cin)
    b = torch.randn(Cout, generator=g) * 0.1
    xn = _nhwc(x).to(torch.bfloat16).to(device)
    res = torch.randn(B, H, H, Cout, generator=g).to(torch.bfloat16).to(device)
    y = AF.conv2d_nhwc(xn, w, b, act="silu", res=res)
    _once(_nchw(y.cpu()), xn.cpu(), w, b, 1, 0, "silu", res=res.cpu(), what="pointwise")
    C.set_conv_pw(False)
    try:
        y2 = AF.conv2d_nhwc(xn, w, b, act="silu", res=res)
    finally:
        C.set_conv_pw(True)
    _once(_nchw(y2.cpu()), xn.cpu(), w, b, 1, 0, "silu", res=res.cpu(), what="pointwise, generic kernel")
    _one_ulp_apart(y, y2)
    assert (y.float() - y2.float()).abs().max().item() <= 0.0625  # one ulp is more than this from |v| = 16 up


def _one_ulp_apart(y, y2):
    """Two kernels doing the same arithmetic in another order: each inside the bound, and no element further from
    its twin than one bf16 ulp of the larger of the two."""
    a, c = y.double().cpu(), y2.double().cpu()
    ulp = bb.ulp_bf16(torch.maximum(a.abs(), c.abs()))
    worst = ((a - c).abs() / ulp).max().item()
    assert worst <= 1.0, f"the two kernels differ by {worst:.2f} bf16 ulps"


@pytest.mark.parametrize("B,H,Cin,Cout,up", [(2, 257, 16, 16, False), (1, 257, 64, 64, True)])
def test_pointwise_fast_path_large_maps(device, B, H, Cin, Cout, up):
    """conv_pw.hip itself: it takes a layer only from 512 workgroups of 256 (Cout 16) / 128 (Cout 64) pixels up,
    which the maps of test_pointwise_fast_path never reach.  257 x 257: the last workgroup is partial."""
    C = native()
    g = torch.Generator().manual_seed(H + Cin)
    x = torch.randn(B, H, H, Cin, generator=g).to(torch.bfloat16)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / np.sqrt(Cin)
    b = torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(B, H, H, Cout, generator=g).to(torch.bfloat16)
    xd, rd = x.to(device), res.to(device)
    out2 = torch.zeros(B, 2 * H, 2 * H, Cout, dtype=torch.bfloat16, device=device) if up else None
    old = C.get_conv_impl()
    C.set_conv_impl(2)
    try:
        y = AF.conv2d_nhwc(xd, w, b, act="silu", res=rd, out2=out2)
        C.set_conv_pw(False)
        y2 = AF.conv2d_nhwc(xd, w, b, act="silu", res=rd)
    finally:
        C.set_conv_pw(True)
        C.set_conv_impl(old)
    _once(_nchw(y.cpu()), x, w, b, 1, 0, "silu", res=res, what="conv_pw")
    _one_ulp_apart(y, y2)
    if up:
        assert torch.equal(out2, y.repeat_interleave(2, 1).repeat_interleave(2, 2))


def test_pointwise_slices_and_upsample(device):
    g = torch.Generator().manual_seed(17)
    B, H, Cbuf, Cin, Cout = 2, 20, 384, 256, 128
    buf = torch.randn(B, H, H, Cbuf, generator=g).to(torch.bfloat16).to(device)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / np.sqrt(Cin)
    b = torch.randn(Cout, generator=g) * 0.1
    out = torch.zeros(B, H, H, 256, dtype=torch.bfloat16, device=device)
    up = torch.zeros(B, 2 * H, 2 * H, 192, dtype=torch.bfloat16, device=device)
    AF.conv2d_nhwc(buf, w, b, act="silu", x_coff=64, cin=Cin, out=out, out_coff=128, out2=up, out2_coff=64)
    torch.cuda.synchronize()
    _once(_nchw(out.cpu()[..., 128:]), buf.cpu()[..., 64:64 + Cin], w, b, 1, 0, "silu", what="pointwise slices")
    assert out.cpu()[..., :128].abs().sum() == 0
    upref = F.interpolate(_nchw(out.cpu()[..., 128:]), scale_factor=2, mode="nearest")
    assert torch.equal(_nchw(up.cpu()[..., 64:]), upref)
    assert up.cpu()[..., :64].abs().sum() == 0


@pytest.mark.parametrize("H,Cin,Cout,s", [(40, 64, 64, 1), (80, 64, 144, 1), (20, 256, 144, 1), (40, 128, 256, 2),
                                          (27, 96, 80, 2), (13, 32, 48, 1)])
def test_conv3x3_v3_matches_v2(device, H, Cin, Cout, s):
    """v3 halo-tile kernel == v2 tile kernel (same math, different staging) and close to torch."""
    C = native()
    g = torch.Generator().manual_seed(H + Cin + Cout)
    x = torch.randn(2, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g) * 0.1
    xn = _nhwc(x).to(torch.bfloat16).to(device)
    y3 = AF.conv2d_nhwc(xn, w, b, stride=s, act="silu")
    C.set_conv_v3(False)
    try:
        y2 = AF.conv2d_nhwc(xn, w, b, stride=s, act="silu")
    finally:
        C.set_conv_v3(True)
    assert (y3.float() - y2.float()).abs().max().item() <= 0.0625
    _once(_nchw(y3.cpu()), xn.cpu(), w, b, s, 1, "silu", what="conv3x3_v3")


def test_executor_autotune_choices(device, tmp_path, monkeypatch):
    """Autotuned conv kernel choices are persisted per (program, bucket) and a table-driven capture runs
    exactly the same kernels: identical choices and bitwise-identical results (engine/tuning.py)."""
    from inference_arena_amd.data.synthetic import synthetic_images
    from inference_arena_amd.engine.pipeline import GpuPipeline
    from inference_arena_amd.models.zoo import make_mobilenet, make_yolo

    yolo, mnet = make_yolo(0, cls_shift=-20.0), make_mobilenet(1)
    imgs = synthetic_images(4, 77)
    monkeypatch.setenv("ARENA_TUNING_FILE", str(tmp_path / "tuning.json"))
    monkeypatch.setenv("ARENA_TUNING", "retune")
    pipe = GpuPipeline(yolo, mnet, device=0, buckets=[4], dtype="bf16")
    assert pipe.tuning_source == "tuned"
    choices = pipe.ex.conv_choices(4)
    # ~50 conv ops remain once the C3 / inverted-residual / stem / head fusions have absorbed the rest
    assert set(c for c in choices if c) <= {1, 2, 3} and sum(1 for c in choices if c) >= 45
    tuned = pipe.infer(imgs)
    monkeypatch.setenv("ARENA_TUNING", "table")
    again = GpuPipeline(yolo, mnet, device=0, buckets=[4], dtype="bf16")
    assert again.tuning_source == "table" and again.ex.conv_choices(4) == choices
    table = again.infer(imgs)
    for a, b in zip(tuned, table):
        assert len(a) == len(b)
        ka, kb = np.lexsort(a.boxes.T), np.lexsort(b.boxes.T)
        np.testing.assert_array_equal(a.boxes[ka], b.boxes[kb])
        np.testing.assert_array_equal(a.topk_logit[ka], b.topk_logit[kb])
    monkeypatch.setenv("ARENA_TUNING", "off")
    plain = GpuPipeline(yolo, mnet, device=0, buckets=[4], dtype="bf16").infer(imgs)
    for a, b in zip(tuned, plain):
        assert abs(len(a) - len(b)) <= 1


@pytest.mark.parametrize("H,s,Cin,Cout", [(64, 1, 16, 32), (64, 2, 16, 32), (37, 1, 16, 32), (40, 1, 80, 80),
                                          (21, 2, 80, 80), (20, 1, 48, 64)])
def test_conv3x3_v3_cin16(device, H, s, Cin, Cout):
    """Cin % 32 == 16 (s2d stems, first C3, the 80-class detect branch) through the v3 halo-tile kernel:
    the last 32-channel slab is half empty."""
    C = native()
    g = torch.Generator().manual_seed(H * 3 + s + Cin)
    x = torch.randn(2, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g) * 0.1
    xn = _nhwc(x).to(torch.bfloat16).to(device)
    old = C.get_conv_impl()
    C.set_conv_impl(2)
    try:
        C.set_conv_pw(False)
        y = AF.conv2d_nhwc(xn, w, b, stride=s, act="silu")
    finally:
        C.set_conv_pw(True)
        C.set_conv_impl(old)
    _once(_nchw(y.cpu()), xn.cpu(), w, b, s, 1, "silu", what="conv3x3_v3 Cin 16")


@pytest.mark.parametrize("H,inp,hid,oup,res,s", [(112, 32, 32, 16, False, 1), (56, 24, 144, 24, True, 1),
                                                 (28, 32, 192, 32, True, 1), (14, 64, 384, 64, True, 1),
                                                 (20, 24, 144, 24, True, 1), (112, 16, 96, 24, False, 2),
                                                 (56, 24, 144, 32, False, 2)])
def test_ir_wave_matches_block_kernel(device, H, inp, hid, oup, res, s):
    """Wave-per-tile IR kernel (stride 1: 8x8 / 7x7 tiles, stride 2: 4x4) == block-cooperative kernel."""
    C = native()
    g = torch.Generator().manual_seed(H + hid)
    x = (torch.rand(2, inp, H, H, generator=g) * 2).to(torch.bfloat16)
    expand = None if hid == inp else (torch.randn(hid, inp, 1, 1, generator=g) / np.sqrt(inp),
                                      torch.randn(hid, generator=g) * 0.1)
    dw = (torch.randn(hid, 1, 3, 3, generator=g) / 3, torch.randn(hid, generator=g) * 0.1)
    project = (torch.randn(oup, hid, 1, 1, generator=g) / np.sqrt(hid), torch.randn(oup, generator=g) * 0.1)
    xn = _nhwc(x).to(device)
    yw = AF.ir_block_nhwc(xn, expand, dw, project, stride=s, res=res)
    C.set_ir_wave(False)
    try:
        yb = AF.ir_block_nhwc(xn, expand, dw, project, stride=s, res=res)
    finally:
        C.set_ir_wave(True)
    assert (yw.float() - yb.float()).abs().max().item() <= 0.07
    refs = _fused_ir(_nchw(yw.cpu()), xn.cpu(), expand, dw, project, s, res, f"ir_wave-{H}-{inp}-{hid}-{oup}-{s}")
    _fused_ir(_nchw(yb.cpu()), xn.cpu(), expand, dw, project, s, res, f"ir_block(wave off)-{H}-{inp}-{hid}-{oup}-{s}",
              refs=refs)


@pytest.mark.gpu
@pytest.mark.parametrize("B,inp,hid,oup,res", [(3, 64, 384, 64, True), (2, 64, 384, 96, False),
                                                 (3, 96, 576, 96, True)])
def test_ir_block_whole_crop_14(device, B, inp, hid, oup, res):
    """Stride-1 14x14 blocks as one whole-crop tile per workgroup (ARENA_IR_T14) == torch fp32 reference."""
    C = native()
    g = torch.Generator().manual_seed(hid + oup)
    x = (torch.rand(B, inp, 14, 14, generator=g) * 2).to(torch.bfloat16)
    expand = (torch.randn(hid, inp, 1, 1, generator=g) / np.sqrt(inp), torch.randn(hid, generator=g) * 0.1)
    dw = (torch.randn(hid, 1, 3, 3, generator=g) / 3, torch.randn(hid, generator=g) * 0.1)
    project = (torch.randn(oup, hid, 1, 1, generator=g) / np.sqrt(hid), torch.randn(oup, generator=g) * 0.1)
    xn = _nhwc(x).to(device)
    C.set_ir_t14(True)
    try:
        y = AF.ir_block_nhwc(xn, expand, dw, project, stride=1, res=res)
    finally:
        C.set_ir_t14(False)
    _fused_ir(_nchw(y.cpu()), xn.cpu(), expand, dw, project, 1, res, f"ir_t14-{B}-{inp}-{hid}-{oup}")


@pytest.mark.gpu
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("H,inp,hid,oup,s,res", [(14, 96, 576, 160, 2, False), (7, 160, 960, 160, 1, True),
                                                 (7, 160, 960, 160, 1, False), (7, 160, 960, 320, 1, False)])
def test_ir_crop_matches_tile_kernel_and_torch(device, H, inp, hid, oup, s, res, split):
    """Whole-crop IR kernel (waves split the hidden channels, ir_crop.hip; ``split`` workgroups per crop
    split its output rows) == torch fp32 reference and the 7x7-tile kernel; crops past the device-side
    live count are not written."""
    C = native()
    C.set_ir_crop_split(split)
    g = torch.Generator().manual_seed(H * 7 + hid)
    x = (torch.rand(5, inp, H, H, generator=g) * 2).to(torch.bfloat16)
    expand = (torch.randn(hid, inp, 1, 1, generator=g) / np.sqrt(inp), torch.randn(hid, generator=g) * 0.1)
    dw = (torch.randn(hid, 1, 3, 3, generator=g) / 3, torch.randn(hid, generator=g) * 0.1)
    project = (torch.randn(oup, hid, 1, 1, generator=g) / np.sqrt(hid), torch.randn(oup, generator=g) * 0.1)
    xn = _nhwc(x).to(device)
    y = AF.ir_block_nhwc(xn, expand, dw, project, stride=s, res=res)
    tag = f"{H}-{inp}-{hid}-{oup}-{s}-{int(res)}"
    refs = _fused_ir(_nchw(y.cpu()), xn.cpu(), expand, dw, project, s, res, f"ir_crop-split{split}-{tag}")
    C.set_ir_crop(False)
    try:
        yt = AF.ir_block_nhwc(xn, expand, dw, project, stride=s, res=res)
    finally:
        C.set_ir_crop(True)
    assert (y.float() - yt.float()).abs().max().item() <= 0.07
    _fused_ir(_nchw(yt.cpu()), xn.cpu(), expand, dw, project, s, res, f"ir_tile(crop off)-{tag}", refs=refs)
    bdev = torch.tensor([3], dtype=torch.int32, device=device)
    yl = AF.ir_block_nhwc(xn, expand, dw, project, stride=s, res=res, bdev=bdev)
    C.set_ir_crop_split(2)
    assert torch.equal(yl[:3].cpu(), y[:3].cpu())
