"""The (conv geometry, kernel) pairs that data/tuning/conv_tuning.json ships for the default programs, and a small
test case for each.  A plain helper module, imported like fp32_bounds.py: test_shipped_convs.py (CPU) checks the
enumeration and that the fp32 bounds reject damage on every generated case, test_shipped_convs_gpu.py runs every pair.

**Inputs.**  The planner (the 14 default programs, ``default_programs``) and the table, nothing else: a re-tuned
table changes what is tested without an edit here.  For every table entry whose fingerprint matches a program, every
``OP_CONV`` record (``ProgramBuilder.decode_conv``) gives a ``Geometry`` and the entry gives its ``ConvParams.impl``.

**Reduced maps.**  Channels, kernel, stride, padding, activation, epilogue, channel offsets and pixel strides are the
plan's; only the map shrinks (``reduced_hw``): H' = H for H <= 24, else 16 + H mod 16 (+ 16 when H mod 16 == 0):
40 -> 24, 80 / 112 / 160 -> 32.  H' keeps H's remainder against the 8- and 16-pixel tiles and at least one interior
tile border.  W' = H'; Ho' is H' through the conv formula plus the plan's own difference from it (``out_hw`` convs:
the 2x2 stem over the space-to-depth input computes H, not H + 1, rows).

**Batch.**  3 images, a device-side live count of 2 (``BATCH``, ``LIVE``).

**What the small batch changes.**  impl 0 (the dispatch policy) and the bf16 families pick their tile by the block
count, so at 3 small images they may launch another tile than the bucket does; the numbered fp32 variants do not.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import torch

import bf16_bounds as bb
import fp32_bounds as fb

BATCH, LIVE = 3, 2
DTYPES = ("fp32", "bf16")

# (Geometry.id, impl) of a pair whose kernel refuses the reduced map but takes the plan's own:
# it runs at the plan's H with one image.  -> the text of the refusal at H'.  test_shipped_convs_gpu.py asserts that
# each pair listed here does refuse at H' and that no other pair does; test_shipped_convs.py caps the list at 10 %.
REFUSES_REDUCED: dict[tuple, str] = {
}


def default_programs():
    """(name, dtype, Program) of the 14 default programs (also test_f32_impl_table.py's)."""
    from inference_arena_amd.engine import plans
    from inference_arena_amd.models.zoo import default_models

    y, m = default_models(0)
    for dtype in DTYPES:
        yield "pipeline", dtype, plans.plan_pipeline(y, m, conf_thr=0.5, iou_thr=0.45, dtype=dtype)
        yield "detector", dtype, plans.plan_detector(y, conf_thr=0.5, iou_thr=0.45, dtype=dtype)
        yield "classifier", dtype, plans.plan_classifier(m, dtype=dtype)
        yield "split_detector", dtype, plans.plan_split_detector(y, conf_thr=0.5, iou_thr=0.45, dtype=dtype)
        yield "split_classifier", dtype, plans.plan_split_classifier(m, dtype=dtype)
        yield "yolo_raw", dtype, plans.plan_yolo_raw(y, dtype=dtype)
        yield "mobilenet_raw", dtype, plans.plan_mobilenet_raw(m, dtype=dtype)


@dataclass(frozen=True)
class Slice:
    """A channel slice of an NHWC buffer: ``coff`` the first channel, ``cs`` the buffer's pixel stride (channels)."""
    present: bool
    coff: int = 0
    cs: int = 0


@dataclass(frozen=True)
class Geometry:
    dtype: str
    H: int
    W: int
    Cin: int
    Cout: int
    KH: int
    KW: int
    stride: int
    pad_t: int
    pad_l: int
    Ho: int
    Wo: int
    act: str | None
    f32out: bool
    src: Slice
    dst: Slice           # absent: a fused 1x1 whose 3x3 result is never stored
    res: Slice
    res_in_dst: bool     # the residual is read from the destination buffer (another slice, or the same: in place)
    dst2: Slice          # the 2x upsampled copy
    pw: tuple | None     # (Cout2, Slice, act2) of the fused pointwise block

    @property
    def f32(self) -> bool:
        return self.dtype == "fp32"

    @property
    def id(self) -> str:
        s = f"{self.dtype}-{self.H}x{self.W}-{self.Cin}to{self.Cout}-k{self.KH}s{self.stride}"
        s += f"-{self.act or 'none'}-x{self.src.coff}of{self.src.cs}"
        if self.dst.present:
            s += f"-y{self.dst.coff}of{self.dst.cs}"
        if self.res.present:
            s += f"-r{self.res.coff}of{self.res.cs}" + ("d" if self.res_in_dst else "")
        if self.dst2.present:
            s += f"-up{self.dst2.coff}of{self.dst2.cs}"
        if self.pw is not None:
            s += f"-pw{self.pw[0]}at{self.pw[1].coff}of{self.pw[1].cs}"
        return s + ("-f32out" if self.f32out and not self.f32 else "")


def geometry_of(rec) -> Geometry:
    """An OP_CONV record -> its Geometry (buffer ids dropped: only presence, offset and stride matter to a kernel)."""
    from inference_arena_amd.engine import planner as P

    d = P.ProgramBuilder.decode_conv(rec)
    if d["x_buf"] == P.BUF_POOL:
        raise ValueError("a letterbox-source conv runs only inside the executor; conv2d_nhwc cannot address it")

    def sl(name):
        present = d[name + "_buf"] != P.BUF_NONE
        return Slice(present, d[name + "_coff"], d[name + "_cs"]) if present else Slice(False)

    pw = (d["pw_cout"], sl("pw_y"), P.ACT_NAMES[d["pw_act"]]) if d["pw_cout"] else None
    return Geometry(P.DTYPES[d["f32"]], d["H"], d["W"], d["Cin"], d["Cout"], d["KH"], d["KW"], d["stride"], d["pad_t"],
                    d["pad_l"], d["Ho"], d["Wo"], P.ACT_NAMES[d["act"]], bool(d["f32out"]),
                    Slice(True, d["x_coff"], d["x_cs"]), sl("y"), sl("res"),
                    d["res_buf"] != P.BUF_NONE and d["res_buf"] == d["y_buf"], sl("y2"), pw)


def shipped_impl(geo: Geometry, impl: int) -> int:
    """The impl the executor launches for a table number: a bf16 conv with a fused 1x1 always takes the v3 halo-tile
    kernel (impl 2, executor.cpp OP_CONV)."""
    return 2 if (not geo.f32 and geo.pw is not None) else int(impl)


@functools.lru_cache(maxsize=None)
def enumerate_shipped():
    """-> (pairs, programs, uses): ``pairs`` {Geometry: {impl: sorted [(program, dtype, bucket)]}} of every conv op of
    every table entry of the default programs; ``programs`` {(name, dtype): (conv ops, sorted buckets of its
    entries)}; ``uses`` {(program, dtype, bucket): [(op index, Geometry, impl)]}."""
    from inference_arena_amd.engine import planner as P
    from inference_arena_amd.engine import tuning

    table = tuning.load_table(tuning.DEFAULT_FILE)
    pairs: dict = {}
    programs: dict = {}
    uses: dict = {}
    for name, dtype, prog in default_programs():
        fp = tuning.fingerprint(prog.ops)
        convs = [(i, geometry_of(r)) for i, r in enumerate(prog.ops) if int(r[0]) == P.OP_CONV]
        buckets = []
        for key, entry in table.items():
            f, _, b = key.partition(":")
            if f != fp:
                continue
            assert len(entry) == len(prog.ops), (name, dtype, key)
            buckets.append(int(b))
            for i, geo in convs:
                assert geo.dtype == dtype, (name, dtype, i)
                impl = shipped_impl(geo, entry[i])
                pairs.setdefault(geo, {}).setdefault(impl, set()).add((name, dtype, int(b)))
                uses.setdefault((name, dtype, int(b)), []).append((i, geo, impl))
        programs[(name, dtype)] = (len(convs), sorted(buckets))
    return {g: {i: sorted(s) for i, s in sorted(v.items())} for g, v in pairs.items()}, programs, uses


def geometries(dtype: str | None = None) -> list[Geometry]:
    return sorted((g for g in enumerate_shipped()[0] if dtype in (None, g.dtype)), key=lambda g: g.id)


def pair_count(dtype: str) -> int:
    return sum(len(v) for g, v in enumerate_shipped()[0].items() if g.dtype == dtype)


def refusal_key(geo: Geometry, impl: int) -> tuple:
    return (geo.id, int(impl))


# ------------------------------------------------------------------------------------------------- reduced maps
def reduced_hw(H: int) -> int:
    if H <= 24:
        return H
    return 16 + H % 16 + (16 if H % 16 == 0 else 0)


def _conv_out(H: int, k: int, pad: int, stride: int) -> int:
    return (H + 2 * pad - k) // stride + 1


def out_hw(geo: Geometry, H: int) -> int:
    """Output rows of the conv on an H x H map, derived as the plan derives Ho from its own H."""
    return _conv_out(H, geo.KH, geo.pad_t, geo.stride) + (geo.Ho - _conv_out(geo.H, geo.KH, geo.pad_t, geo.stride))


# -------------------------------------------------------------------------------------------------------- cases
def _seed(geo: Geometry, H: int) -> int:
    return ((H * 131 + geo.Cin) * 131 + geo.Cout) * 131 + geo.KH * 16 + geo.stride * 4 + int(geo.res.present) * 2 + \
        int(geo.pw is not None)


def _checked(geo: Geometry) -> None:
    """The forms the cases below can express; anything else the planner starts to emit must fail, not pass unseen."""
    assert geo.H == geo.W and geo.KH == geo.KW and geo.pad_t == geo.pad_l and geo.Ho == geo.Wo, geo.id
    assert not geo.res.present or out_hw(geo, geo.H) == _conv_out(geo.H, geo.KH, geo.pad_t, geo.stride), geo.id
    if geo.pw is not None:
        co2, _, act2 = geo.pw
        assert (geo.KH, geo.stride, geo.pad_t, geo.act, act2, co2) == (3, 1, 1, "silu", None, geo.Cout), geo.id
        assert not (geo.res.present or geo.dst2.present or geo.dst.present), geo.id


def fp32_case(geo: Geometry, H: int | None = None, B: int = BATCH) -> fb.Case:
    """The fp32_bounds.Case of a geometry at map H (default: the reduced map): family "one" for a plain conv, the
    two-stage "silu" form of pw_case for a fused 1x1.  Data as fp32_bounds._conv_case draws it."""
    _checked(geo)
    H = reduced_hw(geo.H) if H is None else H
    if geo.pw is not None:
        return fb.pw_case(B, H, geo.Cin, geo.Cout)
    return fb._conv_case("shipped", _seed(geo, H), B, H, geo.Cin, geo.Cout, geo.KH, geo.stride, geo.act,
                         geo.res.present, family="one", pad=geo.pad_t)


def case_hw(geo: Geometry, case: fb.Case) -> tuple[int, int]:
    """(Ho, Wo) the kernel computes on the case's map (fp32_bounds.check ``hw``)."""
    h = out_hw(geo, case.x.shape[2])
    return h, h


def bf16_case(geo: Geometry, H: int | None = None, B: int = BATCH) -> dict:
    """bf16 operands of a geometry (drawn as the fp32 case, activations and residual rounded to bf16 as the kernel
    reads them; the weights stay fp32, the kernel's packer rounds them) with the fp64 reference and scale of
    bf16_bounds.conv_refs, cut to the rows the kernel computes.  A fused 1x1: ``pw_refs``."""
    case = fp32_case(geo, H, B)
    st = case.stages[0]
    x = bb.bf(case.x)
    r = bb.bf(st["res"]) if st.get("res") is not None else None
    d = dict(x=x, w=st["w"], b=st["b"], res=r, hw=case_hw(geo, case))
    if geo.pw is not None:
        st2 = case.stages[1]
        d.update(w2=st2["w"], b2=st2["b"], refs=pw_refs(x, (st["w"], st["b"]), (st2["w"], st2["b"])))
        return d
    ref, scale = bb.conv_refs(x.double(), bb.bf64(st["w"]), st["b"].double(), stride=geo.stride, padding=geo.pad_t,
                              act=geo.act, res64=None if r is None else r.double())
    h = d["hw"][0]
    d.update(ref=ref[..., :h, :h], scale=scale[..., :h, :h])
    return d


def pw_refs(x, conv, pw):
    """The bf16 3x3 (+ SiLU) -> 1x1 of conv3x3_v3.hip: T = SiLU(conv3x3(x, w) + b) stored as bf16 in LDS,
    y = w2 T + b2, the bf16 output.  -> exact64, bound64, mimic64, tight64 as bf16_bounds.stem2_refs, and ties64.

    ``ties64`` replaces the share of bf16_bounds' tier 2, which is a count of 5 to 10 elements on these maps (one
    intermediate rounded the other way moves several of its pixel's 64 or 80 outputs).  An intermediate can be
    stored one bf16 step away from bf(T) only if T lies within the fp32 error of its sum (``e``, the bound
    bf16_bounds gives the value before its store) of the midpoint between two bf16 values; ``ties64`` is one ulp of
    each such intermediate through |w2|, zero for an output none of whose inputs is near a tie.  Every element must
    then lie within tight64 + ties64 of mimic64."""
    import torch.nn.functional as F

    x = x.double()
    w1, b1 = bb.bf64(conv[0]), conv[1].float().double()
    w2, b2 = bb.bf64(pw[0]), pw[1].float().double()
    T = bb.act64(F.conv2d(x, w1, b1, padding=1), "silu")
    e = bb.LIP_SILU * bb.FP32_REL * F.conv2d(x.abs(), w1.abs(), b1.abs(), padding=1)
    BT = bb._stage_bound(T, e)
    y = F.conv2d(T, w2, b2)
    By = bb._stage_bound(y, F.conv2d(BT, w2.abs()) + bb.FP32_REL * F.conv2d(T.abs() + BT, w2.abs(), b2.abs()))
    M = bb.bf64(T)
    mim = F.conv2d(M, w2, b2)
    tight = bb.HALF_ULP * mim.abs() + bb.FP32_REL * F.conv2d(M.abs(), w2.abs(), b2.abs()) + 1e-30
    ulp = bb.ulp_bf16(T)
    near = (0.5 * ulp - (T - M).abs()) <= e  # distance from T to the nearer midpoint
    ties = F.conv2d(ulp * near, w2.abs())
    return y, By, mim, tight, ties


def assert_bf16_pw(got, refs, rms_ref: float, what: str = "") -> dict:
    """Three tiers on the bf16 fused 3x3 -> 1x1: bf16_bounds.assert_bf16_fused's tier 1 (every element within the
    propagated half-ulp bound of the exact chain) and tier 3 (rms against 1.5 x the CPU emulation's), and between
    them every element within tight64 + ties64 of the mimic (``pw_refs``).  NaN fails each."""
    exact, bound, mim, tight, ties = refs
    g = got.detach().double().cpu()
    assert g.shape == exact.shape, (g.shape, exact.shape)
    r1 = ((g - exact).abs() / (bound + 1e-30)).max().item()
    assert r1 <= 1.0, f"{what}: tier 1: {r1:.3f}x the propagated half-ulp bound"
    r2 = ((g - mim).abs() / (tight + ties)).max().item()
    assert r2 <= 1.0, (f"{what}: tier 2: {r2:.3f}x the single-rounding bound plus the ulps of the intermediates "
                       f"next to a tie ({int((~((g - mim).abs() <= tight + ties)).sum())} of {g.numel()} over)")
    flips, rms = bb.fused_stats(g, mim, tight)
    assert rms <= bb.RMS_FACTOR * rms_ref, (f"{what}: tier 3: rms error {rms:.4f} half-ulps, emulation {rms_ref:.4f} "
                                            f"(limit {bb.RMS_FACTOR * rms_ref:.4f})")
    return {"tier1": r1, "tier2": r2, "flips": flips, "rms": rms, "rms_ref": rms_ref,
            "near_tie_outputs": (ties > 0).double().mean().item()}


def pw_emulate(x, conv, pw):
    """The CPU emulation of the bf16 fused 3x3 -> 1x1 (see bf16_bounds.stem2_emulate).  -> NCHW bf16."""
    import torch.nn.functional as F

    T = bb.bf(F.silu(F.conv2d(x.float().contiguous(), bb.bf(conv[0]), conv[1].float(), padding=1)))
    return F.conv2d(T, bb.bf(pw[0]), pw[1].float()).to(torch.bfloat16)


def fp32_scale(geo: Geometry, case: fb.Case):
    """(ref64, scale64) of the per-element 2e-6 sum |x||w| bound (test_fp32_gpu._fp32_check), cut to the computed
    rows; a fused 1x1: the composite scale of test_conv_x3hg_fused_pointwise_matches_fp64."""
    import torch.nn.functional as F

    st = case.stages[0]
    x, w, b = case.x.double(), st["w"].double(), st["b"].double()
    kw = dict(stride=geo.stride, padding=geo.pad_t)
    scale = F.conv2d(x.abs(), w.abs(), b.abs(), **kw)
    if geo.pw is not None:
        st2 = case.stages[1]
        a = bb.act64(F.conv2d(x, w, b, **kw), "silu")
        scale = F.conv2d(1.2 * scale + a.abs(), st2["w"].double().abs(), st2["b"].double().abs())
    elif st.get("res") is not None:
        scale = scale + st["res"].double().abs()
    h, _ = case_hw(geo, case)
    return case.refs()[0][..., :h, :h], scale[..., :h, :h]


# ------------------------------------------------------------------------------------ which file a pair exercises
def kernel_file(dtype: str, impl: int) -> str:
    """The kernel file an impl number names (csrc/kernels/f32_impl.h; bf16: conv_mfma.hip's dispatch).  0 and the
    bf16 numbers are dispatch policies: the file depends on the shape."""
    if dtype == "bf16":
        return {0: "policy", 1: "conv_mfma.hip", 2: "conv_pw.hip / conv3x3_v3.hip / conv_mfma.hip",
                3: "conv_igemm.hip"}[impl]
    if impl == 0:
        return "policy"
    if impl == 106:
        return "fc_splitk.hip"
    if 111 <= impl <= 130 or 171 <= impl <= 179:
        return "gemm_x3.hip"
    if 131 <= impl <= 166 or impl in (181, 182):
        return "halo_x3g.hip"
    if 191 <= impl <= 200:
        return "halo_x3p.hip"
    return "conv_f32.hip"
