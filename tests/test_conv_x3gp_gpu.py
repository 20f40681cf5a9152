"""x3gp (csrc/kernels/gemm_x3p.hip): the x3g implicit GEMM reading and / or writing activations as x3 planes
(``conv2d_nhwc(x_planes=..., out_planes=...)``, ``to_x3_planes`` / ``from_x3_planes``).

Cases, the smallest at which each path can fail: 1x1 on 9 x 7 (M = 126 live pixels, no multiple of 32); 3x3 s1 over
64 channels with residual and SiLU (even chunk count per tap, 7 pixel tiles); 3x3 s2 over 96 channels (odd chunk count:
the odd tail of the K loop; 96 < BN of the 128-wide tile, two tiles of the 64-wide one); 1x1 256 -> 32 (8 chunks, one
N tile mostly padding).  Every case runs a batch of 3 with a live count of 2, on tile 0 (4 waves, 128 px x 64 ch,
TM 2) and tile 7 (8 waves, 128 px x 128 ch, TN 2), for (planes in, planes out) = (0, 1), (1, 0), (1, 1).

The fp32 output must have the bits of x3g (impl 111 + v) on the same fp32 input: same instruction, k-to-lane map, chain
and K order.  The planes output must be ``to_x3_planes`` of it, bit for bit, also when stored alone.  The fp32 output
is held to the single-conv fp64 checks (2e-6 sum |x||w| per element, both tiers of fp32_bounds "one").  A sentinel in
the dead image's planes and in a guard tail after the planes buffer must survive."""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

import fp32_bounds as fb
from inference_arena_amd.ops import functional as AF

pytestmark = pytest.mark.gpu

B, LIVE, X3G, GUARD, SENTINEL = 3, 2, 111, 4096, 0x5A5A
CASES = {  # k, stride, (H, W), Cin, Cout, act, residual
    "1x1-9x7": (1, 1, (9, 7), 32, 64, None, False),
    "3x3-res-silu": (3, 1, (17, 17), 64, 64, "silu", True),
    "3x3-s2-96": (3, 2, (18, 18), 96, 96, None, False),
    "1x1-256-32": (1, 1, (5, 5), 256, 32, None, False),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(fp32_bounds Case, per-element scale sum |x||w| + |b| + |res|), computed once."""
    k, s, (H, W), cin, cout, act, res = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64).float()
    w = (torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** 0.5).float()
    b = (torch.randn(cout, generator=g, dtype=torch.float64) * 0.1).float()
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    r = torch.randn(B, cout, Ho, Wo, generator=g).float() if res else None
    scale = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=s, padding=k // 2)
    if res:
        scale = scale + r.double().abs()
    return fb.Case(f"x3gp-{name}", "one", x, [dict(w=w, b=b, stride=s, padding=k // 2, act=act, res=r)]), scale


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


@pytest.mark.parametrize("v", [0, 7])
@pytest.mark.parametrize("name", list(CASES))
def test_conv_x3gp_matches_x3g_bits_and_fp64(device, name, v):
    case, scale = _case(name)
    st = case.stages[0]
    k, s, _, cin, cout, act, _ = CASES[name]
    x = case.x.permute(0, 2, 3, 1).contiguous().to(device)
    res = st["res"].permute(0, 2, 3, 1).contiguous().to(device) if st["res"] is not None else None
    live = torch.tensor([LIVE], dtype=torch.int32, device=device)
    kw = dict(stride=s, act=act, res=res, bdev=live, impl=X3G + v, packed=AF.pack_weights(st["w"], st["b"], device, "fp32"))
    want = AF.conv2d_nhwc(x, st["w"], st["b"], **kw)[:LIVE]  # x3g itself
    want_planes = _bits(AF.to_x3_planes(want.cpu()))
    Ho, Wo = want.shape[1:3]
    n = B * Ho * Wo * cout * 3
    xp = AF.to_x3_planes(case.x.permute(0, 2, 3, 1).contiguous()).to(device)
    assert torch.equal(AF.from_x3_planes(xp.cpu()), case.x.permute(0, 2, 3, 1))  # h + m + l is the value

    for pin, pout in ((0, 1), (1, 0), (1, 1)):
        flat = torch.full((n + GUARD,), SENTINEL, dtype=torch.int16, device=device)
        planes = flat[:n].view(B, Ho, Wo, cout // 32, 96)
        got = AF.conv2d_nhwc(xp if pin else x, st["w"], st["b"], x_planes=bool(pin),
                             out_planes=planes if pout else None, **kw)
        what = f"v{v} pin{pin} pout{pout}"
        assert torch.equal(got[:LIVE], want), what
        nchw = got[:LIVE].permute(0, 3, 1, 2).cpu()
        err = (nchw.double() - case.refs()[0][:LIVE]).abs()
        worst = (err / (2e-6 * scale[:LIVE] + 1e-30)).max().item()
        print(f"x3gp {case.key} {what}: max error {err.max().item():.3g}, {worst:.3f} x the per-element bound")
        assert worst <= 1.0, what
        fb.check(case, nchw, what, live=LIVE, listed=False)
        if not pout:
            continue
        assert torch.equal(_bits(planes[:LIVE]), want_planes), what
        assert torch.all(planes[LIVE:] == SENTINEL) and torch.all(flat[n:] == SENTINEL), what
        flat.fill_(SENTINEL)  # the planes alone
        only = AF.conv2d_nhwc(xp if pin else x, st["w"], st["b"], x_planes=bool(pin), out_planes=planes,
                              planes_only=True, **kw)
        assert only is planes and torch.equal(AF.from_x3_planes(planes[:LIVE].cpu()), want.cpu()), what
        assert torch.all(planes[LIVE:] == SENTINEL) and torch.all(flat[n:] == SENTINEL), what


@pytest.mark.parametrize("opt", ["y2", "pw", "window", "impl", "cin48", "cout80"])
def test_conv_x3gp_refuses(device, opt):
    cin, cout = (48 if opt == "cin48" else 64), (80 if opt == "cout80" else 64)
    w, b = torch.zeros(cout, cin, 3, 3), torch.zeros(cout)
    x = torch.zeros(1, 4, 4, cin, device=device)
    planes = torch.zeros(1, 4, 4, 2, 96, dtype=torch.int16, device=device)
    kw = dict(impl=40 if opt == "impl" else X3G, out_planes=planes)
    kw.update({"y2": dict(out2=torch.zeros(1, 8, 8, 64, device=device)),
               "pw": dict(pw=(torch.zeros(16, 64, 1, 1), torch.zeros(16))), "window": dict(window=(0, 32))}.get(opt, {}))
    if opt == "cin48":
        x, kw = planes[:, :, :, :1].contiguous(), dict(impl=X3G, x_planes=True)
    with pytest.raises((RuntimeError, ValueError), match="x3gp|plane|window"):
        AF.conv2d_nhwc(x, w, b, **kw)
