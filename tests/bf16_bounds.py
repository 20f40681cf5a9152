"""Error bounds of the bf16 kernels against fp64 references, shared by test_bf16_bounds.py (CPU: proves the
checks reject subtly wrong kernels), test_kernels_gpu.py, test_c3_fused_gpu.py and test_stem_fused_gpu.py.  A plain
helper module, imported like detect_cases.py.

Two kinds of kernel, two checks.

**One rounding** (conv at every impl, conv_pw, conv3x3_v3, fc_splitk, dwconv3x3, avgpool, head_pool): fp32
accumulation of exact bf16 x bf16 products, an fp32 epilogue (bias, activation, residual, pool), one
round-to-nearest-even store.  ``assert_bf16_once``: for every element

    |got - ref64| <= 2^-8 |ref64| + 2e-6 scale64 (+ 1e-30)

2^-8 is the half-ulp of an 8-bit significand relative to the value; 2e-6 * scale64 (scale64: the same op on
absolute values, plus |bias| and |residual|) is the project's fp32 bound for the value before the store
(test_fp32_gpu.py::_fp32_check), which also covers SiLU's v_exp / v_rcp.  No share of elements is exempt and a
NaN fails (the maximum of a ratio is taken).  With an fp32 store the first term drops.

**bf16 intermediates** (ir_block, ir_block_wave, ir_crop, the 14x14 whole-crop tile, c3_fused, the two-stage front
ends of stem_fused.hip): the kernel stores intermediate tensors as bf16 in LDS.  ``assert_bf16_fused`` has three
tiers over the same tensors:

1. every element: |got - exact64| <= bound64, ``exact64`` the block in fp64 without intermediate rounding,
   ``bound64`` the half-ulp error of every store propagated stage by stage through the absolute weights
   (``ir_refs`` / ``c3_refs``); derived, not measured.  NaN fails.
2. ``mimic64`` rounds where the kernel rounds but sums in fp64; an element further from it than
   ``tight64 = 2^-8 |mimic64| + 2e-6 scale_last_stage`` had an intermediate rounded the other way (its fp32 sum
   sat next to a bf16 tie).  The share of such elements may be at most ``cap`` = max(4 x the share of the CPU
   emulation of the kernel on the same inputs, 1e-4): the matrix cores' accumulation order can give an fp32 error a
   few times the CPU's and the flip rate scales with it; the floor keeps a zero count on the CPU from demanding
   zero on the GPU.  These elements are still inside tier 1.
3. rms(got - mimic64) / rms(2^-8 mimic64) at most 1.5 x the same ratio of the CPU emulation (``rms_ref``): the tier
   that sees a small uniform error (a scaled bias, one wrong weight column), which tier 1's slack would hide.

The emulation (``ir_emulate`` / ``c3_emulate`` / ``stem2_emulate``) is fp32 torch with bf16 rounding at the kernel's
store points; tests compute its share and ratio on the CPU with the inputs they give the kernel.  ``MEASURED``
records them per fused case next to the kernels' values of one MI355X run.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

HALF_ULP = 2.0 ** -8   # bf16: 8-bit significand, round to nearest even
FP32_REL = 2e-6        # the fp32 arm's bound on a value before its store, relative to sum |x||w| + |b|
LIP_SILU = 1.1         # max |d silu / dv| = 1.0998...; ReLU6 is 1-Lipschitz
FLIP_FLOOR = 1e-4      # tier 2: cap = max(4 x emulation share, FLIP_FLOOR)
FLIP_FACTOR = 4.0
RMS_FACTOR = 1.5       # tier 3


def bf(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even) and widen back: the value a bf16 store keeps, as fp32."""
    return t.float().to(torch.bfloat16).float()


def bf64(t: torch.Tensor) -> torch.Tensor:
    return bf(t).double()


def act64(y: torch.Tensor, act) -> torch.Tensor:
    if act == "silu":
        return y * torch.sigmoid(y)
    if act == "relu6":
        return y.clamp(0.0, 6.0)
    return y


# --------------------------------------------------------------------------------------------- one rounding
def once_bound(ref64: torch.Tensor, scale64: torch.Tensor, f32out: bool = False) -> torch.Tensor:
    b = FP32_REL * scale64 + 1e-30
    return b if f32out else b + HALF_ULP * ref64.abs()


def assert_bf16_once(got: torch.Tensor, ref64: torch.Tensor, scale64: torch.Tensor, f32out: bool = False,
                     what: str = "") -> float:
    """Every element of ``got`` within 2^-8 |ref64| + 2e-6 scale64 of ``ref64`` (fp32 store: the second term alone).
    -> the worst error / bound ratio."""
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape == scale64.shape, (got.shape, ref64.shape, scale64.shape)
    err = (got - ref64).abs()
    ratio = err / once_bound(ref64, scale64, f32out)
    # a NaN anywhere must fail: max() propagates it and `nan <= 1` is false
    worst = ratio.max().item()
    assert worst <= 1.0, (f"{what}: max error {err.max().item():.4g} is {worst:.3f}x the bf16 single-rounding bound "
                          f"({int((ratio > 1).sum())} + {int(torch.isnan(ratio).sum())} NaN of {ratio.numel()} over)")
    return worst


def conv_refs(x64: torch.Tensor, w64: torch.Tensor, b64: torch.Tensor, *, stride: int = 1, padding=0, act=None,
              res64: torch.Tensor | None = None, groups: int = 1):
    """(ref64, scale64) of act(conv(x, w) + b) (+ res) on NCHW fp64 tensors holding the operands the kernel sees
    (bf16-rounded activations / weights, fp32 bias)."""
    ref = act64(F.conv2d(x64, w64, b64, stride=stride, padding=padding, groups=groups), act)
    scale = F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=stride, padding=padding, groups=groups)
    if res64 is not None:
        ref = ref + res64
        scale = scale + res64.abs()
    return ref, scale


def ulp_bf16(v: torch.Tensor) -> torch.Tensor:
    """One bf16 ulp at |v| (fp64): 2^(floor(log2 |v|) - 7); the smallest normal's ulp below that."""
    e = torch.floor(torch.log2(v.abs().double().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


# --------------------------------------------------------------------------------------------- fused kernels
def fused_stats(got: torch.Tensor, mimic64: torch.Tensor, tight64: torch.Tensor) -> tuple[float, float]:
    """(share of elements further than tight64 from mimic64, rms(got - mimic64) / rms(2^-8 mimic64))."""
    d = (got.detach().double().cpu() - mimic64).abs()
    flips = (~(d <= tight64)).double().mean().item()  # a NaN counts as over
    rms = (d.pow(2).mean().sqrt() / (HALF_ULP * mimic64).pow(2).mean().sqrt()).item()
    return flips, rms


def flip_cap(emu_share: float) -> float:
    return max(FLIP_FACTOR * emu_share, FLIP_FLOOR)


def assert_bf16_fused(got: torch.Tensor, exact64: torch.Tensor, bound64: torch.Tensor, mimic64: torch.Tensor,
                      tight64: torch.Tensor, cap: float, rms_ref: float, what: str = "") -> dict:
    """The three tiers of the module docstring.  ``cap``: the largest share of elements allowed over ``tight64``
    (``flip_cap`` of the emulation's share); ``rms_ref``: the emulation's RMS ratio.  -> the measured figures."""
    g = got.detach().double().cpu()
    assert g.shape == exact64.shape == bound64.shape == mimic64.shape == tight64.shape
    err = (g - exact64).abs()
    ratio = err / (bound64 + 1e-30)
    worst = ratio.max().item()  # NaN propagates and fails
    assert worst <= 1.0, (f"{what}: tier 1: max error {err.max().item():.4g} is {worst:.3f}x the propagated "
                          f"half-ulp bound ({int((~(ratio <= 1)).sum())} of {ratio.numel()} elements over)")
    flips, rms = fused_stats(g, mimic64, tight64)
    assert flips <= cap, f"{what}: tier 2: {flips:.3g} of the elements over the tight bound, cap {cap:.3g}"
    assert rms <= RMS_FACTOR * rms_ref, (f"{what}: tier 3: rms error {rms:.4f} half-ulps, emulation {rms_ref:.4f} "
                                         f"(limit {RMS_FACTOR * rms_ref:.4f})")
    return {"worst": worst, "flips": flips, "rms": rms, "cap": cap, "rms_ref": rms_ref}


def _stage_bound(val64: torch.Tensor, pre_err: torch.Tensor) -> torch.Tensor:
    """Error bound of a bf16-stored value whose exact value is val64 and whose fp32 value before the store is
    within pre_err of it: half an ulp of the stored value, which is itself within pre_err of val64."""
    return HALF_ULP * val64.abs() + (1.0 + HALF_ULP) * pre_err


def ir_refs(x: torch.Tensor, expand, dw, project, stride: int, res: bool):
    """MobileNetV2 inverted residual on bf16-rounded operands, NCHW.  ``x``: the bf16 input widened to fp32/fp64.
    The kernels store the expanded tile and the depthwise output as bf16 (ReLU6 applied before each store) and
    round the output (+ residual, added in fp32) once.  -> exact64, bound64, mimic64, tight64."""
    x = x.double()
    hid = dw[0].shape[0]
    wd, bd = bf64(dw[0]), dw[1].float().double()
    wp, bp = bf64(project[0]), project[1].float().double()
    # exact chain and its propagated bound
    if expand is not None:
        we, be = bf64(expand[0]), expand[1].float().double()
        he = F.conv2d(x, we, be).clamp(0, 6)
        Be = _stage_bound(he, FP32_REL * F.conv2d(x.abs(), we.abs(), be.abs()))
        me = bf64(he)
    else:
        he, Be, me = x, torch.zeros_like(x), x
    hd = F.conv2d(he, wd, bd, stride=stride, padding=1, groups=hid).clamp(0, 6)
    sd = F.conv2d(he.abs() + Be, wd.abs(), bd.abs(), stride=stride, padding=1, groups=hid)
    Bd = _stage_bound(hd, F.conv2d(Be, wd.abs(), None, stride=stride, padding=1, groups=hid) + FP32_REL * sd)
    y = F.conv2d(hd, wp, bp)
    sp = F.conv2d(hd.abs() + Bd, wp.abs(), bp.abs())
    if res:
        y = y + x
        sp = sp + x.abs()
    Bo = _stage_bound(y, F.conv2d(Bd, wp.abs(), None) + FP32_REL * sp)
    # the kernel's rounding points, fp64 sums
    md = bf64(F.conv2d(me, wd, bd, stride=stride, padding=1, groups=hid).clamp(0, 6))
    mim = F.conv2d(md, wp, bp)
    sl = F.conv2d(md.abs(), wp.abs(), bp.abs())
    if res:
        mim = mim + x
        sl = sl + x.abs()
    tight = HALF_ULP * mim.abs() + FP32_REL * sl + 1e-30
    return y, Bo, mim, tight


def ir_emulate(x: torch.Tensor, expand, dw, project, stride: int, res: bool, parts: bool = False):
    """The CPU emulation of the IR kernels: fp32 torch convs, bf16 rounding at the kernels' store points.
    -> NCHW bf16; ``parts``: (the fp32 output before its store, the stored depthwise output) instead, for tests
    that damage the emulation.  ``x`` is made NCHW-contiguous first: torch picks its conv kernel, and with it the
    summation order, by the memory layout, and which handful of elements sit next to a tie depends on that order
    (on the 3 x 14 x 14, 64 -> 384 -> 96 block: 6 of 56,448 elements for a contiguous input, the same 6 as the
    MI355X kernels, none for a channels-last view of the same values)."""
    x = x.float().contiguous()
    h = x
    if expand is not None:
        h = bf(F.relu6(F.conv2d(h, bf(expand[0]), expand[1].float())))
    hid = dw[0].shape[0]
    h = bf(F.relu6(F.conv2d(h, bf(dw[0]), dw[1].float(), stride=stride, padding=1, groups=hid)))
    y = F.conv2d(h, bf(project[0]), project[1].float())
    y = y + x if res else y
    return (y, h) if parts else y.to(torch.bfloat16)


def _silu64(t):
    return t * torch.sigmoid(t)


def c3_refs(x: torch.Tensor, cv12, bottleneck, cv3, n: int, shortcut: bool):
    """YOLOv5 C3 block as c3_fused.hip runs it, NCHW, on bf16-rounded weights: T = SiLU(cv12 x) [2c_]; n times
    (the same bottleneck weights): U = SiLU(w1 T[:c_] + b1), zero outside the map (the 3x3 pads U),
    T[:c_] = (T[:c_] if shortcut) + SiLU(conv3x3(U) + b2); y = SiLU(cv3 T).  T, U and the updated T[:c_] are bf16
    LDS stores (pack4; the shortcut is added in fp32 before the store), y the bf16 output.
    -> exact64, bound64, mimic64, tight64."""
    x = x.double()
    w12, b12 = bf64(cv12[0]), cv12[1].float().double()
    (w1, b1), (w2, b2) = bottleneck
    w1, b1, w2, b2 = bf64(w1), b1.float().double(), bf64(w2), b2.float().double()
    w3, b3 = bf64(cv3[0]), cv3[1].float().double()
    ch = w1.shape[0]

    def pre(v_abs, w, b, pad=0):
        return F.conv2d(v_abs, w.abs(), b.abs(), padding=pad)

    T = _silu64(F.conv2d(x, w12, b12))
    BT = _stage_bound(T, LIP_SILU * FP32_REL * pre(x.abs(), w12, b12))
    M = bf64(T)
    Tc, BTc, T2, BT2 = T[:, :ch], BT[:, :ch], T[:, ch:], BT[:, ch:]
    Mc, M2 = M[:, :ch], M[:, ch:]
    for _ in range(n):
        U = _silu64(F.conv2d(Tc, w1, b1))
        BU = _stage_bound(U, LIP_SILU * (F.conv2d(BTc, w1.abs()) + FP32_REL * pre(Tc.abs() + BTc, w1, b1)))
        V = _silu64(F.conv2d(U, w2, b2, padding=1))
        eV = LIP_SILU * (F.conv2d(BU, w2.abs(), padding=1) + FP32_REL * pre(U.abs() + BU, w2, b2, 1))
        if shortcut:
            eV = eV + BTc + FP32_REL * (Tc.abs() + BTc)  # the fp32 add of the stored T
            V = V + Tc
        Tc, BTc = V, _stage_bound(V, eV)
        MU = bf64(_silu64(F.conv2d(Mc, w1, b1)))
        MV = _silu64(F.conv2d(MU, w2, b2, padding=1))
        Mc = bf64(MV + Mc if shortcut else MV)
    cat, Bcat, Mcat = torch.cat([Tc, T2], 1), torch.cat([BTc, BT2], 1), torch.cat([Mc, M2], 1)
    y = _silu64(F.conv2d(cat, w3, b3))
    By = _stage_bound(y, LIP_SILU * (F.conv2d(Bcat, w3.abs()) + FP32_REL * pre(cat.abs() + Bcat, w3, b3)))
    mim = _silu64(F.conv2d(Mcat, w3, b3))
    tight = HALF_ULP * mim.abs() + FP32_REL * pre(Mcat.abs(), w3, b3) + 1e-30
    return y, By, mim, tight


def c3_emulate(x: torch.Tensor, cv12, bottleneck, cv3, n: int, shortcut: bool) -> torch.Tensor:
    """The CPU emulation of c3_fused.hip: fp32 torch, bf16 rounding at its LDS stores, on the NCHW-contiguous
    input (see ir_emulate).  -> NCHW bf16."""
    x = x.float().contiguous()
    (w1, b1), (w2, b2) = bottleneck
    ch = w1.shape[0]
    T = bf(F.silu(F.conv2d(x, bf(cv12[0]), cv12[1].float())))
    Tc, T2 = T[:, :ch], T[:, ch:]
    for _ in range(n):
        U = bf(F.silu(F.conv2d(Tc, bf(w1), b1.float())))
        V = F.silu(F.conv2d(U, bf(w2), b2.float(), padding=1))
        Tc = bf(V + Tc if shortcut else V)
    return F.silu(F.conv2d(torch.cat([Tc, T2], 1), bf(cv3[0]), cv3[1].float())).to(torch.bfloat16)


def stem2_refs(x: torch.Tensor, stem, second, act="silu", act2="silu"):
    """Detector front end as stem2_kernel (stem_fused.hip) runs it on the bf16 s2d input ``x`` (NCHW [B, 16, H, W]):
    T = act(conv3x3(x, w1) + b1) stored as bf16 in LDS, zero outside the map (the second conv pads T);
    y = act2(conv3x3 stride 2 (T, w2) + b2), the bf16 output.  -> exact64, bound64, mimic64, tight64."""
    x = x.double()
    w1, b1 = bf64(stem[0]), stem[1].float().double()
    w2, b2 = bf64(second[0]), second[1].float().double()
    lip1 = LIP_SILU if act == "silu" else 1.0
    lip2 = LIP_SILU if act2 == "silu" else 1.0
    T = act64(F.conv2d(x, w1, b1, padding=1), act)
    BT = _stage_bound(T, lip1 * FP32_REL * F.conv2d(x.abs(), w1.abs(), b1.abs(), padding=1))
    y = act64(F.conv2d(T, w2, b2, stride=2, padding=1), act2)
    By = _stage_bound(y, lip2 * (F.conv2d(BT, w2.abs(), stride=2, padding=1)
                                 + FP32_REL * F.conv2d(T.abs() + BT, w2.abs(), b2.abs(), stride=2, padding=1)))
    M = bf64(T)
    mim = act64(F.conv2d(M, w2, b2, stride=2, padding=1), act2)
    tight = HALF_ULP * mim.abs() + FP32_REL * F.conv2d(M.abs(), w2.abs(), b2.abs(), stride=2, padding=1) + 1e-30
    return y, By, mim, tight


def stem2_emulate(x: torch.Tensor, stem, second, act="silu", act2="silu", parts: bool = False):
    """The CPU emulation of stem2_kernel: fp32 torch convs, bf16 rounding of the stem output (see ir_emulate for
    the contiguous input).  -> NCHW bf16; ``parts``: (the fp32 output before its store, the stored stem output)."""
    f = {"silu": F.silu, "relu6": F.relu6, None: lambda t: t}
    x = x.float().contiguous()
    T = bf(f[act](F.conv2d(x, bf(stem[0]), stem[1].float(), padding=1)))
    y = f[act2](F.conv2d(T, bf(second[0]), second[1].float(), stride=2, padding=1))
    return (y, T) if parts else y.to(torch.bfloat16)


def c3_case(C1, ch, seed):
    """Weights and input of one C3 block (test_bf16_bounds.py, test_c3_fused_gpu.py): B 2, H 16, W 32 is 2 x 2
    tiles of 8 x 16."""
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(2, C1, 16, 32, generator=g))
    cv12 = (torch.randn(2 * ch, C1, 1, 1, generator=g) / C1 ** 0.5, torch.randn(2 * ch, generator=g) * 0.1)
    bn = ((torch.randn(ch, ch, 1, 1, generator=g) / ch ** 0.5, torch.randn(ch, generator=g) * 0.1),
          (torch.randn(ch, ch, 3, 3, generator=g) / (9 * ch) ** 0.5, torch.randn(ch, generator=g) * 0.1))
    cv3 = (torch.randn(2 * ch, 2 * ch, 1, 1, generator=g) / (2 * ch) ** 0.5, torch.randn(2 * ch, generator=g) * 0.1)
    return x, cv12, bn, cv3


# Measured figures per fused case: (emulation flip share, emulation RMS ratio, kernel flip share, kernel RMS ratio,
# kernel worst error / tier-1 bound).  The emulation columns are what the tests recompute on the CPU; the kernel
# columns are one MI355X run of test_kernels_gpu.py / test_c3_fused_gpu.py (the names are the ones those tests
# print; "(wave off)" / "(crop off)": the same inputs through the kernel the named switch falls back to).
# A record of where the caps sit; no assertion reads it.  The flip counts are small numbers of clustered
# elements (one intermediate next to a tie moves a few outputs of its pixel): 1e-4 is 5 to 50 elements here.
MEASURED: dict[str, tuple[float, float, float, float, float]] = {
    "c3_fused-32-16-1": (0, 0.4211, 0, 0.4211, 0.087),
    "c3_fused-64-32-2": (9.16e-05, 0.4284, 3.05e-05, 0.4284, 0.001),
    "c3_fused-128-32-1": (0.000366, 0.4228, 4.58e-05, 0.4227, 0.023),
    "ir_block-2-112-32-32-16-1": (1.74e-05, 0.4243, 9.96e-06, 0.4242, 0.652),
    "ir_block-2-112-16-96-24-2": (8.64e-05, 0.4273, 6.64e-05, 0.4273, 0.235),
    "ir_block-2-56-24-144-24-1": (5.31e-05, 0.4290, 1.99e-05, 0.4290, 0.284),
    "ir_block-1-56-24-144-32-2": (3.99e-05, 0.4248, 3.99e-05, 0.4248, 0.187),
    "ir_block-2-28-32-192-32-1": (3.99e-05, 0.4311, 3.99e-05, 0.4311, 0.243),
    "ir_block-1-28-32-192-64-2": (0, 0.4235, 0, 0.4235, 0.126),
    "ir_block-3-14-64-384-96-1": (0.000106, 0.4246, 0.000106, 0.4246, 0.107),
    "ir_block-1-14-96-576-160-2": (0, 0.4368, 0, 0.4368, 0.082),
    "ir_block-2-7-160-960-160-1": (0, 0.4295, 0, 0.4295, 0.111),
    "ir_block-2-7-160-960-320-1": (0.0022, 0.4255, 0.000128, 0.4250, 0.090),
    "ir_block-1-20-24-144-24-1": (0, 0.4348, 0, 0.4348, 0.222),
    "ir_wave-112-32-32-16-1": (1.25e-05, 0.4323, 1.25e-05, 0.4323, 0.690),
    "ir_block(wave off)-112-32-32-16-1": (1.25e-05, 0.4323, 1.25e-05, 0.4323, 0.690),
    "ir_wave-56-24-144-24-1": (0, 0.4307, 0, 0.4307, 0.295),
    "ir_block(wave off)-56-24-144-24-1": (0, 0.4307, 0, 0.4307, 0.295),
    "ir_wave-28-32-192-32-1": (3.99e-05, 0.4298, 3.99e-05, 0.4298, 0.256),
    "ir_block(wave off)-28-32-192-32-1": (3.99e-05, 0.4298, 3.99e-05, 0.4298, 0.256),
    "ir_wave-14-64-384-64-1": (0, 0.4313, 0, 0.4313, 0.176),
    "ir_block(wave off)-14-64-384-64-1": (0, 0.4313, 0, 0.4313, 0.176),
    "ir_wave-20-24-144-24-1": (5.21e-05, 0.4280, 0, 0.4280, 0.220),
    "ir_block(wave off)-20-24-144-24-1": (5.21e-05, 0.4280, 0, 0.4280, 0.220),
    "ir_wave-112-16-96-24-2": (3.99e-05, 0.4314, 2.66e-05, 0.4314, 0.208),
    "ir_block(wave off)-112-16-96-24-2": (3.99e-05, 0.4314, 2.66e-05, 0.4314, 0.208),
    "ir_wave-56-24-144-32-2": (1.99e-05, 0.4206, 0, 0.4206, 0.141),
    "ir_block(wave off)-56-24-144-32-2": (1.99e-05, 0.4206, 0, 0.4206, 0.141),
    "ir_t14-3-64-384-64": (0, 0.4316, 0, 0.4316, 0.168),
    "ir_t14-2-64-384-96": (0, 0.4312, 0, 0.4312, 0.115),
    "ir_t14-3-96-576-96": (0, 0.4309, 0, 0.4309, 0.134),
    "ir_crop-split1-14-96-576-160-2-0": (0.000357, 0.4275, 0, 0.4275, 0.091),
    "ir_tile(crop off)-14-96-576-160-2-0": (0.000357, 0.4275, 0, 0.4275, 0.091),
    "ir_crop-split2-14-96-576-160-2-0": (0.000357, 0.4275, 0, 0.4275, 0.091),
    "ir_crop-split1-7-160-960-160-1-1": (0.000332, 0.4317, 5.1e-05, 0.4317, 0.124),
    "ir_tile(crop off)-7-160-960-160-1-1": (0.000332, 0.4317, 5.1e-05, 0.4317, 0.124),
    "ir_crop-split2-7-160-960-160-1-1": (0.000332, 0.4317, 5.1e-05, 0.4317, 0.124),
    "ir_crop-split1-7-160-960-160-1-0": (0.000638, 0.4249, 0.00023, 0.4249, 0.060),
    "ir_tile(crop off)-7-160-960-160-1-0": (0.000638, 0.4249, 0.00023, 0.4249, 0.060),
    "ir_crop-split2-7-160-960-160-1-0": (0.000638, 0.4249, 0.00023, 0.4249, 0.060),
    "ir_crop-split1-7-160-960-320-1-0": (0.00051, 0.4244, 0.000166, 0.4244, 0.079),
    "ir_tile(crop off)-7-160-960-320-1-0": (0.00051, 0.4244, 0.000166, 0.4244, 0.079),
    "ir_crop-split2-7-160-960-320-1-0": (0.00051, 0.4244, 0.000166, 0.4244, 0.079),
    # the fused front ends (stem_fused.hip; test_stem_fused_gpu.py: stem2 = letterbox -> stem -> 3x3 s2 conv at S,
    # stem_ir = crop gather -> stem -> block 1 at S; 10 live items)
    "stem2-64": (0, 0.4394, 0, 0.4394, 0.334),
    "stem2-192": (2.03e-05, 0.4187, 2.17e-05, 0.4187, 0.360),
    "stem_ir-32": (4.88e-05, 0.4207, 9.77e-05, 0.4208, 0.255),
    "stem_ir-96": (8.41e-05, 0.4197, 0, 0.4197, 0.293),
}
