"""x3hc (csrc/kernels/halo_x3c.hip, impl 211 + v): the exact 80-channel 3x3 halo tiles of the Detect head's class
branch, plain and with the fused 1x1, against torch fp64 at the fp32 bounds of fp32_bounds.py.

Every case reads its input from a channel slice of a wider buffer, writes its output into a channel slice of a wider
tensor, and runs a batch of 3 with a live count of 2: all bytes outside the written slice must keep their contents.
19 x 19 is no multiple of a tile side (4 / 8 / 16 rows x 16 columns: partial tiles right and below), 3 x 3 is smaller
than one tile; Cin 64 is two whole 32-deep K chunks, 80 ends in the 16-deep half step, 128 takes four halo chunks."""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

import fp32_bounds as fb
from inference_arena_amd.ops import functional as AF
from inference_arena_amd.ops import native

pytestmark = pytest.mark.gpu

B, LIVE, XOFF, YOFF, FILL = 3, 2, 16, 16, 7.0


@functools.lru_cache(maxsize=None)
def _case(cin, H, c2):
    """(Case, fp64 reference, per-element scale); c2: channels of the fused 1x1, None = the plain conv."""
    g = torch.Generator().manual_seed(cin * 100 + H + (c2 or 0))
    x = torch.randn(B, cin, H, H, generator=g, dtype=torch.float64).float()
    w = (torch.randn(80, cin, 3, 3, generator=g, dtype=torch.float64) / (cin * 9) ** 0.5).float()
    b = (torch.randn(80, generator=g, dtype=torch.float64) * 0.1).float()
    stages = [dict(w=w, b=b, padding=1, act="silu")]
    pre = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ref = pre * torch.sigmoid(pre)
    s1 = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1)
    if c2 is None:  # "one": the family of the single convs
        return fb.Case(f"x3hc-{cin}-{H}", "one", x, stages), ref, s1
    w2 = (torch.randn(c2, 80, 1, 1, generator=g, dtype=torch.float64) / 80 ** 0.5).float()
    b2 = (torch.randn(c2, generator=g, dtype=torch.float64) * 0.1).float()
    stages.append(dict(w=w2, b=b2))
    scale = F.conv2d(1.2 * s1 + ref.abs(), w2.double().abs(), b2.double().abs())  # the fused-chain form
    return fb.Case(f"x3hc-{cin}-{H}-pw{c2}", "silu", x, stages), F.conv2d(ref, w2.double(), b2.double()), scale


@pytest.mark.parametrize("c2", [None, 80, 64])
@pytest.mark.parametrize("H", [19, 3])
@pytest.mark.parametrize("cin", [64, 80, 128])
def test_conv_x3hc_matches_fp64(device, cin, H, c2):
    case, ref, scale = _case(cin, H, c2)
    st = case.stages
    xbuf = torch.full((B, H, H, cin + 32), 3.0)
    xbuf[..., XOFF:XOFF + cin] = case.x.permute(0, 2, 3, 1)
    xbuf = xbuf.to(device)
    n = c2 or 80
    live = torch.tensor([LIVE], dtype=torch.int32, device=device)
    for v in range(native().X3HC_VARIANTS):  # every variant the table row declares
        out = torch.full((B, H, H, n + 32), FILL, device=device)
        kw = dict(act="silu", x_coff=XOFF, cin=cin, impl=native().X3HC_IMPL + v, bdev=live)
        if c2 is None:
            AF.conv2d_nhwc(xbuf, st[0]["w"], st[0]["b"], out=out, out_coff=YOFF, **kw)
        else:
            AF.conv2d_nhwc(xbuf, st[0]["w"], st[0]["b"], pw=(st[1]["w"], st[1]["b"]), pw_out=out, pw_out_coff=YOFF, **kw)
        torch.cuda.synchronize()
        out = out.cpu()
        assert torch.all(out[..., :YOFF] == FILL) and torch.all(out[..., YOFF + n:] == FILL) and torch.all(out[LIVE:] == FILL)
        got = out[:LIVE, :, :, YOFF:YOFF + n].permute(0, 3, 1, 2)
        err = (got.double() - ref[:LIVE]).abs()
        worst = (err / (2e-6 * scale[:LIVE] + 1e-30)).max().item()
        print(f"x3hc {case.key} v{v}: max error {err.max().item():.3g}, {worst:.3f} x the per-element bound")
        assert worst <= 1.0, v
        fb.check(case, got, f"x3hc v{v}", live=LIVE, listed=False)


def test_conv_x3hc_refuses_window_gate_and_marks(device):
    x = torch.zeros(1, 4, 4, 64, device=device)
    w, b = torch.zeros(80, 64, 3, 3), torch.zeros(80)
    for opt in (dict(window=(0, 80)), dict(marks=(torch.zeros(1, 1, 1, dtype=torch.int32, device=device), 8, 8, 1)),
                dict(pw=(torch.zeros(80, 80, 1, 1), torch.zeros(80)), gate=(torch.zeros(1, 4, 4, 80, device=device), 0, 80, 0.0))):
        with pytest.raises(ValueError, match="not x3hc options"):
            AF.conv2d_nhwc(x, w, b, impl=native().X3HC_IMPL, **opt)
