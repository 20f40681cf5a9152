"""Statistical error bounds of the fp32 kernels against fp64 references, shared by test_fp32_bounds.py (CPU: proves
the two tiers reject subtly wrong kernels that the per-element formulas accept) and the fp32 GPU tests
(test_fp32_gpu.py, test_x3hp_gpu.py, test_ir_s2k16_gpu.py, test_ir_dw_strips_gpu.py, test_native_tensor_gpu.py,
and test_shipped_convs_gpu.py, whose cases shipped_convs.py generates from the tuning table: ``check(listed=False)``).
A plain helper module, imported like bf16_bounds.py.

**Why.**  The x3 kernels form a * b from six bf16 products (am bm, al bh, ah bl, am bh, ah bm, ah bh).  Losing one
of the three small ones leaves ~2^-17 per product, 100 x the fp32 error, but with random signs it grows as sqrt(K)
while the per-element formulas (2e-6 sum |x||w|, 2e-5 (1 + max |ref|)) grow as K: they accept it.  The statistic
below scales as the error does.

**The normalised error.**  z = |got - ref64| / sigma, u = 2^-24, sigma a random-walk model of fp32 rounding.  One
stage out = act(conv(x, w) + b) (+ res), every conv below being the same op on squared operands:

    var_pre = u^2 (conv(x^2, w^2) + b^2 + pre^2)  +  conv(var_in, w^2)          (var_in: the input's own variance)
    none:          var_act = var_pre
    ReLU6:         var_act = var_pre inside the clamp (-8 sd < pre < 6 + 8 sd, sd = sqrt(var_pre)), 0 outside
    SiLU:          var_act = silu'(pre)^2 var_pre + u^2 act^2 ((1 - s)^2 (pre^2 + 4) + 6),   s = sigmoid(pre)
    var = var_act (+ var_res) + u^2 out^2

ReLU6 is 1-Lipschitz, but passing var_pre through unchanged overstates sigma wherever the clamp holds (the
output is exactly 0 or 6 there, about half the elements): downstream stages and the pooled mean then hide a lost
product behind variance that does not exist, and the chain cases with more clamping separated by only 3 x.  The
clamp's derivative (0 outside (0, 6)) is the same rule as SiLU's; the 8 sd margin keeps elements whose fp32
pre-activation may fall on the other side of an end.  A residual read from memory is exact and adds no term of its
own (the add's rounding is the u^2 out^2); a residual computed in the chain brings its variance, var_res.

The SiLU term follows common.h ``silu()``: v * rcp(1 + __expf(-v)), __expf(t) = v_exp_f32(t * log2 e).  With
e = exp(-v), d = 1 + e, act = v / d, a relative error r_e of e reaches act as (e / d) r_e = (1 - s) r_e:
  * the product v * log2 e rounds by u relative, an absolute |v| u log2 e in the exponent, so r_e = |v| u;
  * v_exp_f32: 1 ulp = 2 u relative (the accuracy the CDNA3 / CDNA4 ISA reference states for the transcendental
    instructions; nobody has measured it on this hardware), r_e = 2 u;
  * the add 1 + e: u relative in d (the 1 of the 6);
  * v_rcp_f32: 1 ulp = 2 u (the 4 of the 6);
  * the final multiply: u (the last 1 of the 6).
Chains (inverted residual: expand, depthwise, project (+ x); the fused 3x3 -> 1x1 of halo_x3g.hip; the fused
detector front end; C3 in the stage order of bf16_bounds.c3_refs, the zero-padded U included) carry ``var`` from
stage to stage through the squared weights.  head_pool: the variance of the mean over the pixels plus the
sum's and the scaling's own rounding, u^2 (sum a^2 / HW^2 + mean^2).  With HW > 1 the mean of non-negative values
makes u^2 mean^2 the largest term, so a pooled output shows a lost product less than an unpooled one does: the
pooled cases are a family of their own.

Further rounding sources read from the kernels, each u^2 value^2 per extra fp32 add:
  * split-K x3g (impl 171-179, gemm_x3.hip x3g_sk_reduce_kernel): S partial tiles from a workspace summed in split
    order before the bias, S = min(2 / 4 / 8, K chunks of 32 per tap): (S - 1) adds of a running sum that ends at
    pre - b, modelled by its end value: (S - 1) u^2 pre^2;
  * hidden slices (ir_crop_f32.hip x_parts / y_parts): the producer stores P partial sums, each an fp32 project
    sum over its slice of the hidden channels: one more u^2 conv(hd^2, wp^2) for the P stores in place of one; the
    consumer adds them while loading, (P - 1) adds of a sum that ends at y: (P - 1) u^2 y^2.  It enters the next
    block as var_in, through the expand conv and through the residual.

**Two tiers**, on top of the per-element assertions of the GPU tests: ``max z <= ZMAX[family]`` (a localized loss:
one edge column, one partial K chunk; NaN fails since max propagates it) and ``rms z <= ZRMS[family]`` (a small
uniform error).  The constants come from the CPU, never from the kernels: per family (one stage, pooled, IR chain,
SiLU chains: C3, the fused 3x3 -> 1x1, the detector front end) the geometric mean of the largest figure of plain
torch fp32 (``run32(case, "torch")``) and the smallest figure of the mildest damaged x3 emulation
(``run32(case, "x3", {"drop": (t,)})``, t one of mm / lh / hl, each tried) over the family's cases in
``REFERENCE``; ``python tests/fp32_bounds.py --front`` (package importable) recomputes the table and the constants
and says so if a family separates by less than 4 x; test_fp32_bounds.py asserts the separation and the constants
against the table.  ``MEASURED`` holds the kernels' largest figures per case of one MI355X run; no assertion reads
it.  There the matrix cores' sequential fp32 accumulation shows at large K (K 960: max z 40, rms z 4.6 on a single
conv, against torch's 25 and 3.3 on the CPU), still below the limits and a third of the mildest damage.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from bf16_bounds import act64, bf

U = 2.0 ** -24
U2 = U * U
TERMS = ("mm", "lh", "hl", "mh", "hm", "hh")  # a part x b part, summed small to large
SMALL = ("mm", "lh", "hl")


# ------------------------------------------------------------------------------------------------- fp64 + sigma
def _sq(t):
    return t * t


def stage64(x, w, b, *, stride=1, padding=0, groups=1, act=None, res=None, var_in=None, var_res=None, adds=0,
            parts=1):
    """One stage in fp64 -> (out, var, pre); the module docstring's formulas."""
    kw = dict(stride=stride, padding=padding, groups=groups)
    pre = F.conv2d(x, w, b, **kw)
    c2 = F.conv2d(_sq(x), _sq(w), None, **kw)
    var = U2 * (c2 + _sq(b).view(1, -1, 1, 1) + (1 + adds) * _sq(pre))
    if var_in is not None:
        var = var + F.conv2d(var_in, _sq(w), None, **kw)
    out = act64(pre, act)
    if act == "relu6":  # the clamp's derivative: 1 inside (0, 6), 0 outside; kept within 8 sigma of either end
        m = 8.0 * var.sqrt()
        var = var * ((pre > -m) & (pre < 6.0 + m))
    elif act == "silu":
        s = torch.sigmoid(pre)
        var = var * _sq(s * (1 + pre * (1 - s))) + U2 * _sq(out) * (_sq(1 - s) * (_sq(pre) + 4) + 6)
    if res is not None:
        out = out + res
        if var_res is not None:
            var = var + var_res
    var = var + U2 * _sq(out)
    if parts > 1:
        var = var + U2 * (c2 + (parts - 1) * _sq(out))
    return out, var, pre


def split3(t: torch.Tensor) -> dict:
    """fp32 -> its three bf16 planes (held as fp32), as planner.split_bf16x3 and the kernels split."""
    t = t.float()
    h = bf(t)
    m = bf(t - h)
    return {"h": h, "m": m, "l": bf(t - h - m)}


def x3_conv(x, w, *, stride=1, padding=0, groups=1, drop=(), cols=None, chans=None):
    """The CPU emulation of an x3 product: six fp32 convs of bf16 planes, summed small to large.  ``drop`` names the
    partial products left out; with ``cols`` only output columns >= cols lose them, with ``chans`` only input
    channels >= chans (a last partial K chunk)."""
    kw = dict(stride=stride, padding=padding, groups=groups)
    xs, ws = split3(x), split3(w)
    acc = None
    for t in TERMS:
        a, b = xs[t[0]], ws[t[1]]
        if t in drop:
            if chans is not None:
                p = F.conv2d(a[:, :chans].contiguous(), b[:, :chans].contiguous(), None, **kw)
            elif cols is not None:
                p = F.conv2d(a, b, None, **kw)
                p[..., cols:] = 0
            else:
                continue
        else:
            p = F.conv2d(a, b, None, **kw)
        acc = p if acc is None else acc + p
    return acc


def _stage32(x, st, mode, dmg, idx, res):
    kw = dict(stride=st.get("stride", 1), padding=st.get("padding", 0), groups=st.get("groups", 1))
    w, b = st["w"].float(), st["b"].float()
    hit = dmg is not None and idx in dmg.get("stages", (idx,))
    if hit and "bias_tile" in dmg:
        b = b.clone()
        b[dmg["bias_tile"]:dmg["bias_tile"] + 16] *= 1.0 + 2.0 ** -12
    if mode == "x3" and st.get("x3", True):
        d = {k: dmg[k] for k in ("drop", "cols", "chans") if hit and k in dmg}
        y = x3_conv(x, w, **kw, **d) + b.view(1, -1, 1, 1)
    else:
        y = F.conv2d(x, w, b, **kw)
    act = st.get("act")
    if act == "relu6":
        y = F.relu(y) if (dmg is not None and dmg.get("relu")) else F.relu6(y)
    elif act == "silu":
        y = F.silu(y)
    return y + res if res is not None else y


class Case:
    """Inputs of one test case, its fp64 reference and variance (computed once, never modified).  ``stages``: dicts
    of w, b, stride, padding, groups, act, x3 (False: plain fp32 in the kernel, the depthwise convs), begin (this
    stage's input is the block's residual source), res (True: add the block's input; a tensor: add it), parts (the
    stage's output is stored as that many partial sums).  ``pool``: mean over the pixels at the end."""

    def __init__(self, key, family, x, stages, pool=False):
        self.key, self.family, self.x, self.stages, self.pool = key, family, x.float().contiguous(), stages, pool
        self._c = {}

    def _run64(self, adds):
        h, var, mark, vmark, pres = self.x.double(), None, None, None, []
        for st in self.stages:
            if st.get("begin"):
                mark, vmark = h, var
            r = st.get("res")
            res, vres = (mark, vmark) if r is True else ((r.double(), None) if r is not None else (None, None))
            h, var, pre = stage64(h, st["w"].float().double(), st["b"].float().double(), stride=st.get("stride", 1),
                                  padding=st.get("padding", 0), groups=st.get("groups", 1), act=st.get("act"), res=res,
                                  var_in=var, var_res=vres, adds=adds if st is self.stages[-1] else 0,
                                  parts=st.get("parts", 1))
            if st.get("act") == "relu6":
                pres.append(pre)
        if self.pool:
            n = h.shape[2] * h.shape[3]
            m = h.mean((2, 3))
            var = var.sum((2, 3)) / n ** 2 + U2 * (_sq(h).sum((2, 3)) / n ** 2 + _sq(m))
            h = m
        return h, var, pres

    def refs(self, adds=0):
        """-> (ref64, var, ReLU6 pre-activations); ``adds``: extra fp32 adds on the last stage's sum (split-K)."""
        if adds not in self._c:
            self._c[adds] = self._run64(adds)
        return self._c[adds]

    def run32(self, mode="torch", dmg=None):
        h, mark = self.x, None
        for i, st in enumerate(self.stages):
            if st.get("begin"):
                mark = h
            r = st.get("res")
            h = _stage32(h, st, mode, dmg, i, mark if r is True else (r.float() if r is not None else None))
        if self.pool:
            h = h.mean((2, 3))
        if dmg is not None and dmg.get("nan"):
            h = h.clone()
            h.view(-1)[h.numel() // 2] = float("nan")
        return h

    def clamp_shares(self):
        """Per ReLU6 stage: (share of pre-activations above 6, share below 0) of the fp64 reference."""
        return [((p > 6).double().mean().item(), (p < 0).double().mean().item()) for p in self.refs()[2]]


class C3Case(Case):
    """c3_x3.hip: T = SiLU(cv12 x); U = SiLU(w1 T[:c] + b1); T[:c] += SiLU(conv3x3(U) + b2); y = SiLU(cv3 T)."""

    def __init__(self, key, x, cv12, bn, cv3):
        super().__init__(key, "silu", x, [])
        self.w = [cv12, bn[0], bn[1], cv3]

    def _run64(self, adds):
        d = lambda t: t.float().double()  # noqa: E731
        (w12, b12), (w1, b1), (w2, b2), (w3, b3) = [(d(w), d(b)) for w, b in self.w]
        ch = w1.shape[0]
        T, vT, _ = stage64(self.x.double(), w12, b12, act="silu")
        Uo, vU, _ = stage64(T[:, :ch], w1, b1, act="silu", var_in=vT[:, :ch])
        T1, v1, _ = stage64(Uo, w2, b2, padding=1, act="silu", var_in=vU, res=T[:, :ch], var_res=vT[:, :ch])
        y, vy, _ = stage64(torch.cat([T1, T[:, ch:]], 1), w3, b3, act="silu", var_in=torch.cat([v1, vT[:, ch:]], 1))
        return y, vy, []

    def run32(self, mode="torch", dmg=None):
        st = [dict(w=w, b=b, act="silu") for w, b in self.w]
        st[2]["padding"] = 1
        ch = self.w[1][0].shape[0]
        T = _stage32(self.x, st[0], mode, dmg, 0, None)
        Uo = _stage32(T[:, :ch].contiguous(), st[1], mode, dmg, 1, None)
        T1 = _stage32(Uo, st[2], mode, dmg, 2, T[:, :ch])
        y = _stage32(torch.cat([T1, T[:, ch:]], 1), st[3], mode, dmg, 3, None)
        if dmg is not None and dmg.get("nan"):
            y.view(-1)[y.numel() // 2] = float("nan")
        return y


def zstats(got, ref64, var) -> tuple[float, float]:
    """(max z, rms z); a NaN in ``got`` makes both NaN."""
    z = (got.detach().double().cpu() - ref64).abs() / (var + 1e-60).sqrt()
    return z.max().item(), z.pow(2).mean().sqrt().item()


def passes(got, case, adds=0) -> bool:
    mx, rms = zstats(got, *case.refs(adds)[:2])
    return mx <= ZMAX[case.family] and rms <= ZRMS[case.family]


def check(case: Case, got, what="", adds=0, live=None, rms=True, listed=True, hw=None):
    """The two tiers on a kernel's NCHW (pooled: [B, N]) output; ``live``: the leading batch entries to compare.
    Prints the figures before it asserts.  ``listed=False``: a generated case (shipped_convs.py), held to its
    family's limits without a ``REFERENCE`` row; test_shipped_convs.py asserts on every such case what the rows
    record for the listed ones.  ``hw=(Ho, Wo)``: the kernel computes only the leading Ho x Wo of the reference map
    (a conv planned with ``out_hw``)."""
    assert not listed or case.key in REFERENCE, \
        f"{case.key}: no REFERENCE row (python tests/fp32_bounds.py prints the table)"
    ref, var, _ = case.refs(adds)
    got = got.detach().double().cpu()
    if hw is not None:
        ref, var = ref[..., :hw[0], :hw[1]], var[..., :hw[0], :hw[1]]
    if live is not None:
        got, ref, var = got[:live], ref[:live], var[:live]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    mx, r = zstats(got, ref, var)
    print(f"FP32Z {case.key} {what} max_z {mx:.3f} rms_z {r:.4f}")
    assert mx <= ZMAX[case.family], f"{case.key} {what}: max z {mx:.2f} over {ZMAX[case.family]} ({case.family})"
    if rms:
        assert r <= ZRMS[case.family], f"{case.key} {what}: rms z {r:.3f} over {ZRMS[case.family]} ({case.family})"
    return mx, r


def assert_clamped(case: Case):
    """On the fp64 reference alone: every ReLU6 stage has >= 0.5 % of its pre-activations above 6 and >= 10 % below 0."""
    sh = case.clamp_shares()
    assert sh and all(hi >= 0.005 and lo >= 0.10 for hi, lo in sh), (case.key, sh)


# ------------------------------------------------------------------------------------------------------- cases
def _key(kind, *p):
    return kind + "-" + "-".join("x" if v is None else str(int(v) if isinstance(v, bool) else v) for v in p)


def _conv_case(kind, seed, B, H, Cin, Cout, k, s, act, res, family="one", pad=None):
    """test_fp32_gpu.py / test_x3hp_gpu.py single convs: fp64 draws rounded to fp32, the residual drawn last."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, H, generator=g, dtype=torch.float64).float()
    w = (torch.randn(Cout, Cin, k, k, generator=g, dtype=torch.float64) / (Cin * k * k) ** 0.5).float()
    b = (torch.randn(Cout, generator=g, dtype=torch.float64) * 0.1).float()
    pad = k // 2 if pad is None else pad
    Ho = (H + 2 * pad - k) // s + 1
    r = torch.randn(B, Cout, Ho, Ho, generator=g).float() if res else None
    return Case(_key(kind, B, H, Cin, Cout, k, s, act, res), family, x,
                [dict(w=w, b=b, stride=s, padding=pad, act=act, res=r)])


def conv_case(B, H, Cin, Cout, k, s, act, res):        # test_conv_f32_matches_fp64, test_conv_x3_split_matches_fp64
    return _conv_case("conv", B * 100 + H + Cin + Cout, B, H, Cin, Cout, k, s, act, res)


def x3g_case(B, H, Cin, Cout, k, s, act, res):         # test_conv_x3g_matches_fp64
    return _conv_case("x3g", B * 1000 + H + Cin + Cout + k, B, H, Cin, Cout, k, s, act, res)


def x3hg_case(B, H, Cin, Cout, act, res):              # test_conv_x3hg_matches_fp64, test_conv_x3hp_matches_...
    return _conv_case("x3hg", B * 977 + H + Cin + Cout, B, H, Cin, Cout, 3, 1, act, res)


def sk_adds(impl, Cin, k):
    """Extra fp32 adds of a split-K x3g variant (gemm_x3.hip XG_SK_VARIANTS): splits - 1, 0 for any other impl."""
    if not 171 <= impl < 180:
        return 0
    s = min((2, 4, 8)[(impl - 171) % 3], k * k * ((Cin + 31) // 32))
    return s - 1 if s >= 2 else 0


def slice_case(seed, H, stride):                       # the channel-slice / live-batch tests (seeds 11 and 13)
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(4, H, H, 96, generator=g)
    w = torch.randn(64, 32, 3, 3, generator=g) * 0.05
    b = torch.randn(64, generator=g) * 0.1
    c = Case(_key("slice", seed, H, stride), "one", buf[..., 32:64].permute(0, 3, 1, 2),
             [dict(w=w, b=b, stride=stride, padding=1)])
    c.buf = buf
    return c


def pw_case(B, H, Cin, C):                             # test_conv_x3hg_fused_pointwise_matches_fp64
    g = torch.Generator().manual_seed(B * 31 + H + Cin + C)
    x = torch.randn(B, Cin, H, H, generator=g, dtype=torch.float64).float()
    w = (torch.randn(C, Cin, 3, 3, generator=g, dtype=torch.float64) / (Cin * 9) ** 0.5).float()
    b = (torch.randn(C, generator=g, dtype=torch.float64) * 0.1).float()
    w2 = (torch.randn(C, C, 1, 1, generator=g, dtype=torch.float64) / C ** 0.5).float()
    b2 = (torch.randn(C, generator=g, dtype=torch.float64) * 0.1).float()
    return Case(_key("pw", B, H, Cin, C), "silu", x, [dict(w=w, b=b, padding=1, act="silu"), dict(w=w2, b=b2)])


def fc_case(B, live):                                  # test_fc_f32_crop_tiles
    g = torch.Generator().manual_seed(B * 5 + (live or 0))
    x = torch.randn(B, 1280, 1, 1, generator=g)
    w = torch.randn(1000, 1280, 1, 1, generator=g) / 1280 ** 0.5
    b = torch.randn(1000, generator=g)
    return Case(_key("fc", B, live), "one", x, [dict(w=w, b=b)])


def dw_case(stride, H, gain=1.0):                      # test_dwconv_f32 (gain 2.5: the clamp-reaching cases)
    g = torch.Generator().manual_seed(stride * 10 + H)
    x = torch.randn(3, 96, H, H, generator=g)
    w = torch.randn(96, 1, 3, 3, generator=g) * 0.3 * gain
    b = torch.randn(96, generator=g) * 0.1
    return Case(_key("dw", stride, H, gain), "one", x,
                [dict(w=w, b=b, stride=stride, padding=1, groups=96, act="relu6", x3=False)])


def head_pool_case(B, HW, gain=1.0):                   # test_head_pool_f32_matches_fp64
    g = torch.Generator().manual_seed(B * 7 + HW)
    H = int(round(HW ** 0.5)) if int(round(HW ** 0.5)) ** 2 == HW else 1
    x = torch.randn(B, 320, H, HW // H, generator=g)
    w = torch.randn(1280, 320, 1, 1, generator=g) / 320 ** 0.5 * gain
    b = torch.randn(1280, generator=g) * 0.1
    return Case(_key("head_pool", B, HW, gain), "pool" if HW > 1 else "one", x, [dict(w=w, b=b, act="relu6")], pool=True)


def _ir_weights(g, inp, hid, oup, gain=1.0):
    expand = None if hid == inp else (torch.randn(hid, inp, 1, 1, generator=g) / inp ** 0.5 * gain,
                                      torch.randn(hid, generator=g) * 0.1)
    dw = (torch.randn(hid, 1, 3, 3, generator=g) / 3 * gain, torch.randn(hid, generator=g) * 0.1)
    project = (torch.randn(oup, hid, 1, 1, generator=g) / hid ** 0.5, torch.randn(oup, generator=g) * 0.1)
    return expand, dw, project


def ir_stages(expand, dw, project, stride, res, parts=1):
    st = []
    if expand is not None:
        st.append(dict(w=expand[0], b=expand[1], act="relu6"))
    st.append(dict(w=dw[0], b=dw[1], stride=stride, padding=1, groups=dw[0].shape[0], act="relu6", x3=False))
    st.append(dict(w=project[0], b=project[1], res=True if res else None, parts=parts))
    st[0]["begin"] = True
    return st


def _ir(key, x, blocks):
    """blocks: (expand, dw, project, stride, res, y_parts) in chain order."""
    c = Case(key, "ir", x, [s for b in blocks for s in ir_stages(*b)])
    c.blocks = blocks
    return c


def ir_case(inp, hid, oup, stride, H, res, gain=1.0, B=3):  # test_ir_block_f32_matches_fp64 (+ clamp cases)
    g = torch.Generator().manual_seed(inp * 7 + hid + stride)
    x = torch.randn(B, inp, H, H, generator=g)
    return _ir(_key("ir", inp, hid, oup, stride, H, res, gain), x, [(*_ir_weights(g, inp, hid, oup, gain), stride, res, 1)])


def ir_chain_case(parts, crops, bands, gain=1.0):      # test_ir_block_f32_hidden_slices_chain
    eff = min(parts, 3) if crops > 32 else parts
    g = torch.Generator().manual_seed(parts * 11 + bands)
    ws = [_ir_weights(g, inp, hid, oup, gain) for inp, hid, oup in ((64, 384, 96), (96, 576, 96))]
    x = torch.randn(crops, 64, 14, 14, generator=g)
    return _ir(_key("ir_chain", parts, crops, bands, gain), x, [(*ws[0], 1, False, eff), (*ws[1], 1, True, 1)])


def ir_tail_case(parts):                               # test_ir_block_f32_hidden_slices_tail
    g = torch.Generator().manual_seed(parts + 70)
    b14, b15, b17 = (_ir_weights(g, *s) for s in ((96, 576, 160), (160, 960, 160), (160, 960, 320)))
    x = torch.randn(6, 96, 14, 14, generator=g)
    return _ir(_key("ir_tail", parts), x, [(*b14, 2, False, parts), (*b15, 1, True, parts), (*b17, 1, False, 1)])


def s2k16_case(H, W, B):                               # test_ir_s2k16_gpu.py
    g = torch.Generator().manual_seed(1000 * H + 10 * W + B)
    x = torch.randn(B, 16, H, W, generator=g)
    return _ir(_key("s2k16", H, W, B), x, [(*_ir_weights(g, 16, 96, 24), 2, False, 1)])


def strips_case(inp, hid, oup, stride, H, res, B=3):   # test_ir_dw_strips_gpu.py
    g = torch.Generator().manual_seed(inp * 7 + hid + stride + H)
    x = torch.randn(B, inp, H, H, generator=g)
    return _ir(_key("strips", inp, hid, oup, stride, H, res), x, [(*_ir_weights(g, inp, hid, oup), stride, res, 1)])


def c3_case(B, H, W):                                  # test_c3_x3_matches_fp64
    g = torch.Generator().manual_seed(B * 100 + H + W)
    x = torch.randn(B, 32, H, W, generator=g)
    cv12 = (torch.randn(32, 32, 1, 1, generator=g) / 32 ** 0.5, torch.randn(32, generator=g) * 0.1)
    bn = ((torch.randn(16, 16, 1, 1, generator=g) / 4, torch.randn(16, generator=g) * 0.1),
          (torch.randn(16, 16, 3, 3, generator=g) / 12, torch.randn(16, generator=g) * 0.1))
    cv3 = (torch.randn(32, 32, 1, 1, generator=g) / 32 ** 0.5, torch.randn(32, generator=g) * 0.1)
    return C3Case(_key("c3", B, H, W), x, cv12, bn, cv3)


def front_case(name, x, w0, b0, w1, b1):               # test_native_tensor_gpu.py: s2d stem 6x6 s2 -> 3x3 s2
    return Case(_key("front", name), "silu", x, [dict(w=w0, b=b0, stride=2, padding=2, act="silu"),
                                                 dict(w=w1, b=b1, stride=2, padding=1, act="silu")])


def front_weights():
    """Folded fp32 weights of the detector's first two convs, the stem in its 6x6 space-to-depth-free form."""
    from inference_arena_amd.engine.plans import s2d_stem_6x6  # noqa: F401  (the packed form; the reference is 6x6)
    from inference_arena_amd.models.common import fold
    from inference_arena_amd.models.zoo import default_models

    y = default_models(0)[0]
    (w0, b0), (w1, b1) = fold(y.b0), fold(y.b1)
    return w0.float(), b0.float(), w1.float(), b1.float()


# The GPU tests' case lists (the existing ones repeat the parametrize lists of their tests; ``check`` refuses a case
# that has no REFERENCE row, so a list that drifts shows).
CONV_F32 = [(2, 20, 16, 16, 3, 1, "silu", False), (2, 40, 16, 32, 3, 2, "silu", False), (3, 20, 32, 32, 3, 1, "silu", True),
            (2, 10, 64, 128, 1, 1, "silu", False), (4, 7, 160, 960, 1, 1, "relu6", False), (4, 7, 960, 160, 1, 1, None, True),
            (2, 10, 256, 144, 3, 1, "silu", False), (2, 20, 64, 80, 3, 1, "silu", False), (5, 1, 1280, 1000, 1, 1, None, False)]
X3_SPLIT = [(2, 20, 32, 32, 3, 1, "silu", True), (2, 24, 80, 80, 3, 1, "silu", False), (2, 20, 64, 144, 3, 1, "silu", False),
            (2, 40, 16, 32, 3, 2, "silu", False), (2, 12, 16, 32, 2, 1, "relu6", False), (2, 20, 16, 16, 3, 1, "silu", True),
            (4, 7, 160, 960, 1, 1, "relu6", False), (4, 7, 960, 160, 1, 1, None, True)]
CLAMP_CONV = (2, 7, 160, 960, 1, 1, "relu6", False)    # inputs x 3 (conv_clamp_case)
X3G = [(2, 40, 32, 64, 3, 2, "silu", False), (3, 20, 64, 128, 3, 2, "silu", False), (2, 10, 128, 256, 3, 2, "silu", False),
       (3, 13, 128, 128, 1, 1, "silu", False), (2, 9, 256, 128, 1, 1, "silu", False), (2, 11, 80, 80, 1, 1, "silu", False),
       (5, 7, 160, 960, 1, 1, "relu6", False), (5, 7, 960, 160, 1, 1, None, True), (5, 7, 960, 320, 1, 1, None, False),
       (2, 5, 512, 256, 1, 1, "silu", False)]
X3HG = [(2, 20, 64, 144, "silu", False), (2, 19, 80, 80, "silu", False), (3, 17, 32, 32, "silu", True),
        (2, 12, 128, 64, None, False), (2, 9, 20, 48, "relu6", False)]
CLAMP_X3HG = (2, 9, 20, 48, "relu6", False)
PW = [(2, 20, 64, 64), (2, 19, 80, 80), (3, 11, 144, 64)]
FC = [(17, None), (32, 16), (32, 17)]
DW = [(1, 14), (2, 28), (1, 7), (2, 112)]
CLAMP_DW = [(1, 14), (2, 9)]
HEAD_POOL = [(5, 49), (3, 64), (2, 1)]
CLAMP_HEAD_POOL = [(2, 49), (2, 1)]
IR = [(32, 32, 16, 1, 40, False), (16, 96, 24, 2, 37, False), (32, 96, 24, 2, 37, False), (24, 144, 24, 1, 28, True),
      (24, 144, 24, 1, 56, True), (32, 192, 32, 1, 30, False), (24, 144, 32, 2, 28, False), (32, 192, 32, 1, 28, True),
      (32, 192, 64, 2, 28, False), (64, 384, 64, 1, 14, True), (64, 384, 96, 1, 14, False), (96, 576, 96, 1, 14, True),
      (96, 576, 160, 2, 14, False), (160, 960, 160, 1, 7, True), (160, 960, 320, 1, 7, False)]
CLAMP_IR = [(32, 32, 16, 1, 20, False), (16, 96, 24, 2, 17, False), (24, 144, 24, 1, 19, True), (32, 192, 64, 2, 28, False),
            (64, 384, 96, 1, 14, False), (96, 576, 160, 2, 14, False), (160, 960, 160, 1, 7, True)]
CLAMP_GAIN = 2.5
DW_CLAMP_GAIN = 3.0  # x 2.5 leaves the 9 x 9 stride-2 map (a large share of border sums) at 0.36 % above 6
IR_CHAIN = [(p, c, b) for b in (2, 4) for p, c in ((2, 5), (3, 5), (6, 5), (6, 40))]
IR_TAIL = [1, 3, 5]
S2K16 = [(8, 8, 1), (37, 37, 3), (16, 24, 2), (112, 112, 1), (20, 20, 5)]
STRIPS = [(32, 64, 32, 1, 12, False), (32, 64, 32, 1, 12, True), (24, 144, 24, 1, 20, True), (32, 96, 24, 2, 10, False)]
C3 = [(2, 24, 48), (1, 8, 16), (3, 16, 32)]


def conv_clamp_case(kind, *p):
    """A ReLU6 conv case with its input x 3: pre-activations ~ N(0, 3), about 2 % above 6 (x 2.5 leaves the 3x3 case,
    whose border sums are shorter, at 0.35 %)."""
    c = {"conv": conv_case, "x3hg": x3hg_case}[kind](*p)
    return Case(c.key + "-clamp", "one", c.x * 3.0, c.stages)


def all_cases():
    """Every Case the GPU tests check except the detector front end (its weights come from the model zoo:
    front_cases())."""
    for p in CONV_F32 + [q for q in X3_SPLIT if q not in CONV_F32]:
        yield conv_case(*p)
    yield conv_clamp_case("conv", *CLAMP_CONV)
    for p in X3G:
        yield x3g_case(*p)
    for p in X3HG:
        yield x3hg_case(*p)
    yield conv_clamp_case("x3hg", *CLAMP_X3HG)
    yield slice_case(11, 12, 2)
    yield slice_case(13, 11, 1)
    for p in PW:
        yield pw_case(*p)
    for p in FC:
        yield fc_case(*p)
    for p in DW:
        yield dw_case(*p)
    for p in CLAMP_DW:
        yield dw_case(*p, gain=DW_CLAMP_GAIN)
    for p in HEAD_POOL:
        yield head_pool_case(*p)
    for p in CLAMP_HEAD_POOL:
        yield head_pool_case(*p, gain=CLAMP_GAIN)
    for p in IR:
        yield ir_case(*p)
    for p in CLAMP_IR:
        yield ir_case(*p, gain=CLAMP_GAIN, B=2)
    for p in IR_CHAIN:
        yield ir_chain_case(*p)
    yield ir_chain_case(3, 5, 2, gain=CLAMP_GAIN)
    for p in IR_TAIL:
        yield ir_tail_case(p)
    for p in S2K16:
        yield s2k16_case(*p)
    for p in STRIPS:
        yield strips_case(*p)
    for p in C3:
        yield c3_case(*p)


def reference_row(case: Case):
    """(torch max z, torch rms z, intact x3 max z, rms z, mildest damaged max z, rms z): the smallest figures over
    mm / lh / hl dropped."""
    ref, var, _ = case.refs()
    t = zstats(case.run32("torch"), ref, var)
    e = zstats(case.run32("x3"), ref, var)
    if not any(st.get("x3", True) for st in case.stages or [{}]):  # no x3 product in the case: nothing to drop
        return (*t, *e, None, None)
    d = [zstats(case.run32("x3", {"drop": (s,)}), ref, var) for s in SMALL]
    return (*t, *e, min(m for m, _ in d), min(r for _, r in d))


def constants(table: dict, family_of: dict):
    """Per family: (ZMAX, ZRMS, separation of max z, of rms z) from a REFERENCE-shaped table."""
    out = {}
    for fam in sorted(set(family_of.values())):
        rows = [table[k] for k in table if family_of[k] == fam]
        tm, tr = max(r[0] for r in rows), max(r[1] for r in rows)
        dm, dr = min(r[4] for r in rows if r[4] is not None), min(r[5] for r in rows if r[5] is not None)
        out[fam] = (math.sqrt(tm * dm), math.sqrt(tr * dr), dm / tm, dr / tr)
    return out


# family -> limit; the geometric means that ``python tests/fp32_bounds.py`` prints, rounded
ZMAX = {"one": 55.0, "pool": 14.6, "ir": 22.6, "silu": 21.4}
ZRMS = {"one": 8.1, "pool": 3.4, "ir": 5.3, "silu": 3.26}

# case -> (torch fp32 max z, rms z, intact x3 emulation max z, rms z, mildest damaged emulation max z, rms z), CPU
REFERENCE: dict[str, tuple] = {
    "conv-2-20-16-16-3-1-silu-0": (10.6, 1.34, 3.21, 0.507, 138, 23.2),
    "conv-2-40-16-32-3-2-silu-0": (12.5, 1.36, 4.3, 0.512, 149, 23),
    "conv-3-20-32-32-3-1-silu-1": (13.7, 1.3, 5.77, 0.574, 129, 16.8),
    "conv-2-10-64-128-1-1-silu-0": (8.95, 0.945, 2.72, 0.386, 146, 22.8),
    "conv-4-7-160-960-1-1-relu6-0": (17.9, 1.57, 5.83, 0.576, 152, 21.3),
    "conv-4-7-960-160-1-1-x-1": (23.8, 2.98, 8.06, 1.2, 145, 26.8),
    "conv-2-10-256-144-3-1-silu-0": (14, 1.89, 6.09, 0.861, 146, 22.5),
    "conv-2-20-64-80-3-1-silu-0": (16.2, 1.82, 6.75, 0.712, 170, 22.9),
    "conv-5-1-1280-1000-1-1-x-0": (19.4, 3.46, 10.9, 1.38, 129, 30.5),
    "conv-2-20-32-32-3-1-silu-1": (11.6, 1.26, 4.66, 0.57, 125, 16.8),
    "conv-2-24-80-80-3-1-silu-0": (15.2, 1.88, 7.63, 0.746, 154, 22.7),
    "conv-2-20-64-144-3-1-silu-0": (18.8, 1.83, 7.2, 0.716, 154, 22.6),
    "conv-2-12-16-32-2-1-relu6-0": (8.49, 0.934, 2.74, 0.367, 154, 22),
    "conv-2-20-16-16-3-1-silu-1": (8.26, 1.09, 3.08, 0.497, 134, 17.1),
    "conv-2-7-160-960-1-1-relu6-0-clamp": (16.1, 1.51, 6.51, 0.56, 160, 21.2),
    "x3g-2-40-32-64-3-2-silu-0": (19.2, 1.71, 7.18, 0.647, 143, 22.5),
    "x3g-3-20-64-128-3-2-silu-0": (25.6, 1.83, 7.35, 0.722, 145, 22.4),
    "x3g-2-10-128-256-3-2-silu-0": (11.9, 1.86, 5.17, 0.754, 142, 22.8),
    "x3g-3-13-128-128-1-1-silu-0": (12.5, 1.19, 4.53, 0.47, 149, 22.7),
    "x3g-2-9-256-128-1-1-silu-0": (25.8, 1.87, 6.25, 0.664, 140, 22.5),
    "x3g-2-11-80-80-1-1-silu-0": (8.42, 1.06, 4.32, 0.417, 135, 22.2),
    "x3g-5-7-160-960-1-1-relu6-0": (16.6, 1.56, 6.74, 0.577, 169, 21.4),
    "x3g-5-7-960-160-1-1-x-1": (18.7, 2.96, 10.4, 1.19, 145, 26.6),
    "x3g-5-7-960-320-1-1-x-0": (25.4, 3.31, 9.79, 1.28, 157, 30.2),
    "x3g-2-5-512-256-1-1-silu-0": (17.1, 2.27, 7.54, 0.839, 132, 22.2),
    "x3hg-2-20-64-144-3-1-silu-0": (20.3, 1.83, 7.65, 0.716, 158, 22.6),
    "x3hg-2-19-80-80-3-1-silu-0": (16.3, 1.85, 6.95, 0.733, 161, 22.8),
    "x3hg-3-17-32-32-3-1-silu-1": (15.7, 1.31, 4.6, 0.568, 132, 16.7),
    "x3hg-2-12-128-64-3-1-x-0": (15, 2.51, 8.47, 1.07, 149, 30.2),
    "x3hg-2-9-20-48-3-1-relu6-0": (13.3, 1.36, 3.27, 0.526, 123, 21.1),
    "x3hg-2-9-20-48-3-1-relu6-0-clamp": (10.8, 1.36, 4.72, 0.513, 137, 21.1),
    "slice-11-12-2": (15.6, 2.27, 5.22, 0.879, 127, 30.3),
    "slice-13-11-1": (16.1, 2.27, 7, 0.87, 162, 29.4),
    "pw-2-20-64-64": (5.51, 1.31, 2.92, 0.596, 71.1, 17),
    "pw-2-19-80-80": (6.99, 1.34, 2.79, 0.613, 71.8, 16.9),
    "pw-3-11-144-64": (5.65, 1.29, 2.9, 0.646, 71.3, 17.3),
    "fc-17-x": (22.9, 3.93, 10.8, 1.12, 125, 23.9),
    "fc-32-16": (25, 3.87, 9.14, 1.14, 150, 24.6),
    "fc-32-17": (21.3, 3.89, 8.19, 1.13, 145, 24.5),
    "dw-1-14-1.0": (4.1, 0.368, 4.1, 0.368, None, None),
    "dw-2-28-1.0": (3.49, 0.38, 3.49, 0.38, None, None),
    "dw-1-7-1.0": (3.48, 0.36, 3.48, 0.36, None, None),
    "dw-2-112-1.0": (3.64, 0.392, 3.64, 0.392, None, None),
    "dw-1-14-3.0": (2.9, 0.363, 2.9, 0.363, None, None),
    "dw-2-9-3.0": (3.28, 0.34, 3.28, 0.34, None, None),
    "head_pool-5-49-1.0": (5.56, 1.34, 3.44, 0.954, 48.1, 9.59),
    "head_pool-3-64-1.0": (4.67, 1.2, 3.18, 0.849, 38.7, 8.71),
    "head_pool-2-1-1.0": (20.5, 1.68, 3.93, 0.573, 116, 18.9),
    "head_pool-2-49-2.5": (5.25, 1.32, 3.17, 0.939, 38.5, 9.94),
    "head_pool-2-1-2.5": (11.2, 1.6, 4.45, 0.58, 117, 19),
    "ir-32-32-16-1-40-0-1.0": (3.29, 0.641, 2.48, 0.49, 73.5, 16.8),
    "ir-16-96-24-2-37-0-1.0": (4.22, 0.824, 2.5, 0.466, 90.2, 19.5),
    "ir-32-96-24-2-37-0-1.0": (4.58, 0.867, 2.33, 0.478, 91.1, 19.6),
    "ir-24-144-24-1-28-1-1.0": (7.26, 0.963, 2.9, 0.513, 94.3, 17),
    "ir-24-144-24-1-56-1-1.0": (6.12, 0.909, 3.52, 0.508, 80.9, 16.6),
    "ir-32-192-32-1-30-0-1.0": (7.41, 1.14, 3.3, 0.538, 80.8, 18.7),
    "ir-24-144-32-2-28-0-1.0": (4.79, 0.848, 2.42, 0.486, 85, 19.4),
    "ir-32-192-32-1-28-1-1.0": (7.94, 1.02, 3.12, 0.529, 84.9, 17.6),
    "ir-32-192-64-2-28-0-1.0": (4.45, 0.927, 2.55, 0.51, 90.4, 20.2),
    "ir-64-384-64-1-14-1-1.0": (5.58, 0.999, 2.8, 0.56, 83.4, 17.3),
    "ir-64-384-96-1-14-0-1.0": (5.18, 1.1, 2.79, 0.57, 90.7, 19.6),
    "ir-96-576-96-1-14-1-1.0": (8.3, 1.15, 3.22, 0.614, 84.8, 17.6),
    "ir-96-576-160-2-14-0-1.0": (8.95, 1.54, 3.64, 0.67, 88.5, 19.8),
    "ir-160-960-160-1-7-1-1.0": (6.76, 1.55, 3.4, 0.721, 84, 17.1),
    "ir-160-960-320-1-7-0-1.0": (9.34, 1.77, 3.53, 0.764, 84.2, 19.8),
    "ir-32-32-16-1-20-0-2.5": (3.26, 0.643, 1.99, 0.473, 73.2, 16.8),
    "ir-16-96-24-2-17-0-2.5": (3.29, 0.829, 1.84, 0.439, 78.9, 19.1),
    "ir-24-144-24-1-19-1-2.5": (4.75, 0.874, 2.73, 0.487, 89.9, 18.7),
    "ir-32-192-64-2-28-0-2.5": (4.39, 0.915, 2.26, 0.489, 88.6, 19.2),
    "ir-64-384-96-1-14-0-2.5": (5.74, 1.13, 2.53, 0.564, 91.4, 19.4),
    "ir-96-576-160-2-14-0-2.5": (7.3, 1.53, 3.58, 0.669, 90.2, 19.5),
    "ir-160-960-160-1-7-1-2.5": (7.81, 1.81, 3.88, 0.773, 87.6, 19.7),
    "ir_chain-2-5-2-1.0": (5.78, 1.05, 2.44, 0.56, 79.5, 16.8),
    "ir_chain-3-5-2-1.0": (4.89, 1.03, 2.58, 0.539, 86, 17.1),
    "ir_chain-6-5-2-1.0": (4.49, 0.935, 2.68, 0.496, 80.6, 15.7),
    "ir_chain-6-40-2-1.0": (5.75, 1, 2.8, 0.534, 90.4, 16.9),
    "ir_chain-2-5-4-1.0": (5.25, 1.05, 2.73, 0.542, 75.8, 17.9),
    "ir_chain-3-5-4-1.0": (4.79, 1.03, 2.3, 0.534, 82, 17.2),
    "ir_chain-6-5-4-1.0": (4.85, 0.953, 2.37, 0.495, 75.1, 15.9),
    "ir_chain-6-40-4-1.0": (5.25, 1.02, 2.89, 0.532, 95.9, 17),
    "ir_chain-3-5-2-2.5": (4.35, 1.02, 2.64, 0.527, 75.4, 17.3),
    "ir_tail-1": (9.14, 1.67, 3.16, 0.731, 91.3, 18.8),
    "ir_tail-3": (7.34, 1.51, 3.18, 0.654, 80.2, 16.8),
    "ir_tail-5": (6.62, 1.42, 2.83, 0.626, 70.5, 15.6),
    "s2k16-8-8-1": (3.49, 0.793, 1.39, 0.429, 54.8, 19.5),
    "s2k16-37-37-3": (4.66, 0.78, 2.37, 0.452, 83.3, 20),
    "s2k16-16-24-2": (4.11, 0.854, 2.82, 0.471, 84.3, 19.8),
    "s2k16-112-112-1": (5.18, 0.822, 2.37, 0.458, 92.2, 20.2),
    "s2k16-20-20-5": (4.85, 0.865, 2.23, 0.459, 82.9, 19.4),
    "strips-32-64-32-1-12-0": (4.36, 0.834, 2.22, 0.469, 76.5, 19.9),
    "strips-32-64-32-1-12-1": (4.07, 0.781, 2.46, 0.484, 82.5, 17.3),
    "strips-24-144-24-1-20-1": (4.35, 0.835, 2.54, 0.499, 81.9, 17.3),
    "strips-32-96-24-2-10-0": (3.42, 0.955, 1.85, 0.478, 68.2, 19.6),
    "c3-2-24-48": (3.42, 0.632, 1.66, 0.353, 70, 13.8),
    "c3-1-8-16": (2.88, 0.631, 1.38, 0.352, 63.4, 14.1),
    "c3-3-16-32": (3.27, 0.652, 1.7, 0.361, 82.1, 14.5),
    "front-uniform": (9.65, 1.54, 4.8, 0.757, 90.3, 19.3),
    "front-mixed": (6.23, 0.863, 4.61, 0.618, 92.8, 13.5),
    "front-pixels": (4.04, 0.871, 4.87, 0.283, 47.3, 6.9),
}

# case -> (largest max z, largest rms z) over the kernels / variants that ran it in one MI355X run
MEASURED: dict[str, tuple] = {
    "conv-2-20-16-16-3-1-silu-0": (11.6, 1.34),
    "conv-2-40-16-32-3-2-silu-0": (13.1, 1.38),
    "conv-3-20-32-32-3-1-silu-1": (12.5, 1.53),
    "conv-2-10-64-128-1-1-silu-0": (8.43, 0.97),
    "conv-4-7-160-960-1-1-relu6-0": (19, 1.56),
    "conv-4-7-960-160-1-1-x-1": (34.8, 4.97),
    "conv-2-10-256-144-3-1-silu-0": (40.4, 5.23),
    "conv-2-20-64-80-3-1-silu-0": (26.6, 2.67),
    "conv-5-1-1280-1000-1-1-x-0": (17.5, 3.8),
    "x3g-2-40-32-64-3-2-silu-0": (16.9, 1.63),
    "x3g-3-20-64-128-3-2-silu-0": (19.8, 2.28),
    "x3g-2-10-128-256-3-2-silu-0": (23.5, 3.13),
    "x3g-3-13-128-128-1-1-silu-0": (11.1, 1.1),
    "x3g-2-9-256-128-1-1-silu-0": (13.3, 1.55),
    "x3g-2-11-80-80-1-1-silu-0": (7.15, 0.873),
    "x3g-5-7-160-960-1-1-relu6-0": (15.8, 1.29),
    "x3g-5-7-960-160-1-1-x-1": (32.5, 4.21),
    "x3g-5-7-960-320-1-1-x-0": (40, 4.55),
    "x3g-2-5-512-256-1-1-silu-0": (25.1, 2.21),
    "slice-11-12-2": (21.2, 2.31),
    "x3hg-2-20-64-144-3-1-silu-0": (25.9, 2.29),
    "x3hg-2-19-80-80-3-1-silu-0": (28.7, 2.54),
    "x3hg-3-17-32-32-3-1-silu-1": (13.2, 1.28),
    "x3hg-2-12-128-64-3-1-x-0": (30.5, 4.68),
    "x3hg-2-9-20-48-3-1-relu6-0": (13.1, 1.44),
    "pw-2-20-64-64": (9.12, 1.97),
    "pw-2-19-80-80": (10.4, 2.22),
    "pw-3-11-144-64": (15.6, 2.84),
    "slice-13-11-1": (17.7, 2.3),
    "conv-2-20-32-32-3-1-silu-1": (12.2, 1.28),
    "conv-2-24-80-80-3-1-silu-0": (32.8, 2.58),
    "conv-2-20-64-144-3-1-silu-0": (25.2, 2.29),
    "conv-2-12-16-32-2-1-relu6-0": (6.89, 0.929),
    "conv-2-20-16-16-3-1-silu-1": (11.6, 1.09),
    "conv-2-7-160-960-1-1-relu6-0-clamp": (19.7, 1.51),
    "x3hg-2-9-20-48-3-1-relu6-0-clamp": (10.9, 1.43),
    "fc-17-x": (20.3, 3.04),
    "fc-32-16": (22.8, 3.14),
    "fc-32-17": (23.4, 3.13),
    "dw-1-14-1.0": (4.1, 0.368),
    "dw-2-28-1.0": (3.49, 0.381),
    "dw-1-7-1.0": (3.48, 0.36),
    "dw-2-112-1.0": (3.64, 0.392),
    "dw-1-14-3.0": (2.9, 0.363),
    "dw-2-9-3.0": (3.28, 0.34),
    "ir-32-32-16-1-40-0-1.0": (3.75, 0.673),
    "ir-16-96-24-2-37-0-1.0": (5.32, 0.822),
    "ir-32-96-24-2-37-0-1.0": (5.14, 0.921),
    "ir-24-144-24-1-28-1-1.0": (7.43, 0.94),
    "ir-24-144-24-1-56-1-1.0": (7.62, 0.918),
    "ir-32-192-32-1-30-0-1.0": (8.8, 1.13),
    "ir-24-144-32-2-28-0-1.0": (5.71, 1),
    "ir-32-192-32-1-28-1-1.0": (7.48, 1.01),
    "ir-32-192-64-2-28-0-1.0": (7.63, 1.14),
    "ir-64-384-64-1-14-1-1.0": (11.5, 1.42),
    "ir-64-384-96-1-14-0-1.0": (10.8, 1.57),
    "ir-96-576-96-1-14-1-1.0": (12.8, 1.74),
    "ir-96-576-160-2-14-0-1.0": (10.1, 1.89),
    "ir-160-960-160-1-7-1-1.0": (18.4, 2.34),
    "ir-160-960-320-1-7-0-1.0": (18.5, 2.58),
    "ir-32-32-16-1-20-0-2.5": (4.34, 0.646),
    "ir-16-96-24-2-17-0-2.5": (4.8, 0.866),
    "ir-24-144-24-1-19-1-2.5": (6.59, 1),
    "ir-32-192-64-2-28-0-2.5": (6.93, 1.11),
    "ir-64-384-96-1-14-0-2.5": (10.8, 1.61),
    "ir-96-576-160-2-14-0-2.5": (12.8, 2),
    "ir-160-960-160-1-7-1-2.5": (19, 2.61),
    "ir_chain-2-5-2-1.0": (8.23, 1.37),
    "ir_chain-3-5-2-1.0": (8.08, 1.21),
    "ir_chain-6-5-2-1.0": (6.56, 0.931),
    "ir_chain-6-40-2-1.0": (8.32, 1.1),
    "ir_chain-2-5-4-1.0": (9.15, 1.24),
    "ir_chain-3-5-4-1.0": (8.06, 1.14),
    "ir_chain-6-5-4-1.0": (7.61, 0.993),
    "ir_chain-6-40-4-1.0": (10.1, 1.16),
    "ir_chain-3-5-2-2.5": (7.11, 1.21),
    "ir_tail-1": (15.4, 2.4),
    "ir_tail-3": (11.3, 1.82),
    "ir_tail-5": (11.3, 1.71),
    "c3-2-24-48": (2.23, 0.395),
    "c3-1-8-16": (1.6, 0.374),
    "c3-3-16-32": (2.22, 0.392),
    "head_pool-5-49-1.0": (5.11, 1.38),
    "head_pool-3-64-1.0": (5.49, 1.15),
    "head_pool-2-1-1.0": (13.3, 1.52),
    "head_pool-2-49-2.5": (4.92, 1.36),
    "head_pool-2-1-2.5": (10.3, 1.48),
    "s2k16-8-8-1": (2.92, 0.849),
    "s2k16-37-37-3": (5.15, 0.851),
    "s2k16-16-24-2": (5.27, 0.869),
    "s2k16-112-112-1": (5.24, 0.836),
    "s2k16-20-20-5": (4.89, 0.848),
    "strips-32-64-32-1-12-0": (3.65, 0.595),
    "strips-32-64-32-1-12-1": (3.37, 0.578),
    "strips-24-144-24-1-20-1": (7.41, 0.933),
    "strips-32-96-24-2-10-0": (3.84, 0.822),
    "front-uniform": (8.64, 1.53),
    "front-mixed": (6.58, 0.855),
    "front-pixels": (3.1, 0.407),
}


if __name__ == "__main__":
    import sys

    table, fam = {}, {}
    cases = list(all_cases())
    if "--front" in sys.argv:  # needs the package importable (model zoo)
        from test_native_tensor_gpu import _inputs

        cases += [front_case(n, _inputs(n), *front_weights()) for n in ("uniform", "mixed", "pixels")]
    for c in cases:
        table[c.key], fam[c.key] = reference_row(c), c.family
        print(f'    "{c.key}": ({", ".join("None" if v is None else f"{v:.3g}" for v in table[c.key])}),', flush=True)
    for f, (zm, zr, sm, sr) in constants(table, fam).items():
        print(f"# {f}: ZMAX {zm:.3g} ZRMS {zr:.3g} separation max {sm:.1f}x rms {sr:.1f}x")
        if sm < 4 or sr < 4:
            print(f"# family {f} separates by less than 4x: fix the sigma model")
