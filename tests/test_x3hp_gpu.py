"""x3hp (csrc/kernels/halo_x3p.hip): the 16x16x32 halo tiles of impl 101 / 102 / 103 / 108 / 109 fed from the
plan's pre-split weight planes instead of splitting the fp32 weights in every workgroup.

The family changes where the operands come from, not the arithmetic: same K order (32-channel chunk, ky, kx),
same six products per step, fp32 accumulation.  The host split (planner.split_bf16x3) rounds as the device split
does, so every variant must equal the old kernels bit for bit whatever its tile shape, and meet the fp32 bound
of tests/test_fp32_gpu.py against an fp64 reference.
"""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

import fp32_bounds as fb
from inference_arena_amd.ops import functional as AF

pytestmark = pytest.mark.gpu

X3HP_IMPLS = [191 + v for v in range(9)]
X3_HALO_IMPLS = [101, 102, 103, 108, 109]  # conv_x3_halo_kernel: auto / 48 / 32-channel tiles, 8 or 16 rows


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _act64(y, act):
    if act == "silu":
        return y * torch.sigmoid(y)
    if act == "relu6":
        return y.clamp(0.0, 6.0)
    return y


def _fp32_check(got, ref64, scale64, rel=2e-6):
    """|got - ref| <= rel * sum|x||w| (+ a denormal floor): the bound of test_fp32_gpu.py."""
    err = (got.double().cpu() - ref64).abs()
    bound = rel * scale64 + 1e-30
    worst = (err / bound).max().item()
    assert worst <= 1.0, f"max error {err.max().item():.3g} is {worst:.2f}x the fp32 bound"


@pytest.mark.parametrize(
    "B,H,Cin,Cout,act,res,up",
    [
        (2, 20, 64, 144, "silu", False, False),  # partial pixel tiles both ways (16 + 4, 8 + 8 + 4), 9 fragments
        (2, 19, 80, 80, "silu", False, False),   # tail chunk of 16 real channels (Cin32 = 96), NF 5, odd side
        (3, 17, 32, 32, "silu", True, False),    # one chunk, residual epilogue
        (2, 12, 128, 64, None, False, True),     # four chunks, 2x-upsampled second store
        (2, 9, 20, 48, "relu6", False, False),   # Cin 20 (Cin % 4 == 0 only), map smaller than one tile
    ],
)
def test_conv_x3hp_matches_fp64_and_old_halo_bits(device, B, H, Cin, Cout, act, res, up):
    g = torch.Generator().manual_seed(B * 977 + H + Cin + Cout)
    x = torch.randn(B, Cin, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g, dtype=torch.float64) * 0.1
    x32, w32, b32 = x.float(), w.float(), b.float()
    ref = _act64(F.conv2d(x32.double(), w32.double(), b32.double(), padding=1), act)
    scale = F.conv2d(x32.double().abs(), w32.double().abs(), b32.double().abs(), padding=1)
    r = torch.randn(B, Cout, H, H, generator=g).float() if res else None
    if res:
        ref = ref + r.double()
        scale = scale + r.double().abs()
    xd = _nhwc(x32).to(device)
    rd = _nhwc(r).to(device) if res else None
    packed = AF.pack_weights(w32, b32, device, "fp32")

    def run(impl):
        out2 = torch.full((B, 2 * H, 2 * H, Cout), float("nan"), device=device) if up else None
        y = AF.conv2d_nhwc(xd, w32, b32, act=act, res=rd, packed=packed, impl=impl, out2=out2)
        torch.cuda.synchronize()
        return y, out2

    # the old kernels take tap-major rows only (Kpad == 9 * Cin, so 9 * Cin % 16 == 0); 101 takes all of those
    old = {}
    for impl in X3_HALO_IMPLS:
        try:
            old[impl] = run(impl)
        except RuntimeError:
            assert (9 * Cin) % 16 != 0 or impl != 101, "impl 101 must take this shape"
    assert (101 in old) == ((9 * Cin) % 16 == 0)

    case = fb.x3hg_case(B, H, Cin, Cout, act, res)  # the inputs of test_fp32_gpu.py::test_conv_x3hg_matches_fp64
    assert torch.equal(case.x, x32)
    bad = []
    for impl in X3HP_IMPLS:
        y, out2 = run(impl)
        try:
            _fp32_check(y.permute(0, 3, 1, 2), ref, scale)
            fb.check(case, y.permute(0, 3, 1, 2), impl)
        except AssertionError as e:
            bad.append((impl, str(e)))
            continue
        if up:
            want = y.permute(0, 3, 1, 2).repeat_interleave(2, 2).repeat_interleave(2, 3)
            assert torch.equal(out2.permute(0, 3, 1, 2), want), impl
        for o, (yo, out2o) in old.items():
            if not torch.equal(y, yo):
                bad.append((impl, f"differs from impl {o} in {(y != yo).sum().item()} elements"))
            if up and not torch.equal(out2, out2o):
                bad.append((impl, f"upsampled copy differs from impl {o}"))
    assert not bad, bad


def test_conv_x3hp_channel_slices_and_live_batch(device):
    """Channel-slice input and output views and the device-side live batch count: blocks past it, and channels
    outside the output slice, leave memory untouched."""
    g = torch.Generator().manual_seed(13)
    buf = torch.randn(4, 11, 11, 96, generator=g)
    w = torch.randn(64, 32, 3, 3, generator=g) * 0.05
    b = torch.randn(64, generator=g) * 0.1
    packed = AF.pack_weights(w, b, device, "fp32")
    ref = F.conv2d(buf[..., 32:64].permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1)
    live = torch.tensor([3], dtype=torch.int32, device=device)
    case = fb.slice_case(13, 11, 1)
    assert torch.equal(case.buf, buf)
    want = None
    for impl in [101] + X3HP_IMPLS:
        out = torch.full((4, 11, 11, 128), 7.0, device=device)
        AF.conv2d_nhwc(buf.to(device), w, b, stride=1, act=None, x_coff=32, cin=32, out=out, out_coff=64,
                       packed=packed, impl=impl, bdev=live)
        torch.cuda.synchronize()
        got = out[:3, :, :, 64:].permute(0, 3, 1, 2).double().cpu()
        assert (got - ref[:3]).abs().max().item() < 1e-5, impl
        assert torch.all(out[:, :, :, :64] == 7.0) and torch.all(out[3] == 7.0), impl
        fb.check(case, got, impl, live=3, rms=False)
        if want is None:
            want = out
        assert torch.equal(out, want), impl


def test_conv_x3hp_relu6_reaches_the_clamp(device):
    """The Cin 20 case with its input x 3 (about 1.5 % of the pre-activations above 6): a ReLU in place of ReLU6
    would differ.  Every x3hp variant under the fp32 bound and both tiers of fp32_bounds.py."""
    case = fb.conv_clamp_case("x3hg", *fb.CLAMP_X3HG)
    fb.assert_clamped(case)
    st = case.stages[0]
    x64, w64, b64 = case.x.double(), st["w"].double(), st["b"].double()
    ref = _act64(F.conv2d(x64, w64, b64, padding=1), "relu6")
    scale = F.conv2d(x64.abs(), w64.abs(), b64.abs(), padding=1)
    xd = _nhwc(case.x).to(device)
    packed = AF.pack_weights(st["w"], st["b"], device, "fp32")
    bad = []
    for impl in X3HP_IMPLS:
        y = AF.conv2d_nhwc(xd, st["w"], st["b"], act="relu6", packed=packed, impl=impl)
        torch.cuda.synchronize()
        try:
            _fp32_check(y.permute(0, 3, 1, 2), ref, scale)
            fb.check(case, y.permute(0, 3, 1, 2), impl)
        except AssertionError as e:
            bad.append((impl, str(e)))
    assert not bad, bad
