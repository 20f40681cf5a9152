"""Every (conv geometry, kernel) pair that data/tuning/conv_tuning.json ships for the default programs
(tests/shipped_convs.py), run through AF.conv2d_nhwc in the plan's own layout on a reduced map: channel slices and pixel
strides of source, destination, residual and upsampled copy as planned, 3 images with a device-side live count of 2.

Per pair: the live rows against the fp64 reference (fp32: the per-element 2e-6 sum |x||w| bound and both tiers of
fp32_bounds; bf16: bf16_bounds.assert_bf16_once, the fused 3x3 -> 1x1 the three tiers of
shipped_convs.assert_bf16_pw), and nothing else written: every byte outside the written channel slice and every row
from the live count on keeps what it held; the upsampled copy equals the output repeated 2x2 bit for bit.

The tile gate, cell marks and output-channel window are the executor's run-time options, not the table's
(test_head_gate_gpu.py, test_head_split_gpu.py).

Which pairs exercise which kernel file: shipped_convs.kernel_file; the test prints it per pair.
"""
from __future__ import annotations

import pytest
import torch

import bf16_bounds as bb
import fp32_bounds as fb
import shipped_convs as sc
from inference_arena_amd.ops import functional as AF
from test_fp32_gpu import _fp32_check

pytestmark = pytest.mark.gpu

GEOS = sc.geometries()
SENTINEL = 7.0        # destinations, and the residual / upsampled buffers outside their slices
SRC_SENTINEL = 1000.0  # source channels outside the slice: a kernel that reads them is far off, not NaN x 0


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _is_refusal(e: RuntimeError) -> bool:
    """A launcher's own "this conv does not fit the kernel" (conv_f32.hip, conv_mfma.hip, conv3x3_v3.hip), as
    opposed to a HIP error."""
    return str(e).startswith(("conv2d_f32:", "conv2d:", "conv3x3_v3:"))


class _Data:
    """Operands and references of one geometry at one map size, built once and shared by the geometry's impls."""

    def __init__(self, geo, device, H, B, live):
        self.geo, self.H, self.B, self.live = geo, H, B, live
        if geo.f32:
            self.case = sc.fp32_case(geo, H, B)
            st = self.case.stages[0]
            self.x, self.w, self.b, self.r = self.case.x, st["w"], st["b"], st.get("res")
            self.ref, self.scale = sc.fp32_scale(geo, self.case)
            self.pw = (self.case.stages[1]["w"], self.case.stages[1]["b"]) if geo.pw is not None else None
        else:
            d = sc.bf16_case(geo, H, B)
            self.x, self.w, self.b, self.r = d["x"], d["w"], d["b"], d["res"]
            self.pw = (d["w2"], d["b2"]) if geo.pw is not None else None
            if self.pw is not None:
                self.refs = [t[:live] for t in d["refs"]]
                emu = sc.pw_emulate(self.x, (self.w, self.b), self.pw)[:live]
                self.rms = bb.fused_stats(emu, self.refs[2], self.refs[3])[1]
            else:
                self.ref, self.scale = d["ref"], d["scale"]
        self.Ho = sc.out_hw(geo, H)
        self.packed = AF.pack_weights(self.w, self.b, device, geo.dtype)
        self.bdev = torch.tensor([live], dtype=torch.int32, device=device)


def _slice_buffer(device, B, H, sl, C, dtype, fill, value=None):
    buf = torch.full((B, H, H, sl.cs), fill, dtype=dtype)
    if value is not None:
        buf[..., sl.coff:sl.coff + C] = _nhwc(value).to(dtype)
    return buf.to(device)


def _untouched(buf, before, sl, C, live, what):
    """Outside channels [coff, coff + C) of the first ``live`` items ``buf`` still holds ``before``, bit for bit."""
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:live, ..., sl.coff:sl.coff + C] = False
    assert torch.equal(buf[keep], before[keep]), \
        f"{what}: written outside channels [{sl.coff}, {sl.coff + C}) of the {live} live items"


def _run(device, d: _Data, impl: int, what: str):
    """One pair: launch in the plan's layout, then every assertion of the module docstring."""
    geo, B, H, Ho, live = d.geo, d.B, d.H, d.Ho, d.live
    act_dt = torch.float32 if geo.f32 else torch.bfloat16
    out_dt = torch.float32 if (geo.f32 or geo.f32out) else torch.bfloat16
    xb = _slice_buffer(device, B, H, geo.src, geo.Cin, act_dt, SRC_SENTINEL, d.x)
    out = res = out2 = pw_out = None
    kw = {}
    if geo.dst.present:
        own_res = d.r if (geo.res.present and geo.res_in_dst) else None
        assert own_res is None or geo.res == geo.dst, "a residual from another slice of the destination buffer"
        out = _slice_buffer(device, B, Ho, geo.dst, geo.Cout, out_dt, SENTINEL, own_res)  # in place: y += conv
        kw.update(out=out, out_coff=geo.dst.coff)
    if geo.res.present:
        res = out if geo.res_in_dst else _slice_buffer(device, B, Ho, geo.res, geo.Cout, act_dt, SENTINEL, d.r)
        kw.update(res=res, res_coff=geo.res.coff)
    if geo.dst2.present:
        out2 = torch.full((B, 2 * Ho, 2 * Ho, geo.dst2.cs), SENTINEL, dtype=out_dt, device=device)
        kw.update(out2=out2, out2_coff=geo.dst2.coff)
    if geo.pw is not None:
        co2, psl, _ = geo.pw
        pw_out = torch.full((B, Ho, Ho, psl.cs), SENTINEL, dtype=out_dt, device=device)
        kw.update(pw=d.pw, pw_out=pw_out, pw_out_coff=psl.coff)
    before = {k: t.clone() for k, t in (("x", xb), ("out", out), ("res", res), ("out2", out2), ("pw", pw_out))
              if t is not None}
    AF.conv2d_nhwc(xb, d.w, d.b, stride=geo.stride, pad=(geo.pad_t, geo.pad_l), act=geo.act, x_coff=geo.src.coff,
                   cin=geo.Cin, f32out=geo.f32out, out_hw=(Ho, Ho), bdev=d.bdev, packed=d.packed, impl=impl, **kw)
    torch.cuda.synchronize()

    # nothing else written
    assert torch.equal(xb, before["x"]), f"{what}: the source changed"
    if res is not None and res is not out:
        assert torch.equal(res, before["res"]), f"{what}: the residual buffer changed"
    if geo.pw is not None:
        y, ysl, C = pw_out, geo.pw[1], geo.pw[0]
        _untouched(pw_out, before["pw"], ysl, C, live, what + " 1x1 output")
    else:
        y, ysl, C = out, geo.dst, geo.Cout
        _untouched(out, before["out"], ysl, C, live, what + " output")
    got = y[:live, ..., ysl.coff:ysl.coff + C]
    if out2 is not None:
        _untouched(out2, before["out2"], geo.dst2, C, live, what + " upsampled copy")
        up = out2[:live, ..., geo.dst2.coff:geo.dst2.coff + C]
        assert torch.equal(up, got.repeat_interleave(2, 1).repeat_interleave(2, 2)), \
            f"{what}: the upsampled copy is not the output repeated 2x2"

    # the live rows against fp64
    got = got.permute(0, 3, 1, 2).cpu()
    if geo.f32:
        _fp32_check(got, d.ref[:live], d.scale[:live])
        family = "silu" if geo.pw is not None else "one"
        assert d.case.family == family
        return fb.check(d.case, got, what, adds=fb.sk_adds(impl, geo.Cin, geo.KH), live=live, listed=False,
                        hw=(Ho, Ho))
    if geo.pw is not None:
        fig = sc.assert_bf16_pw(got, d.refs, d.rms, what)
        print(f"BF16PW {what} " + " ".join(f"{k} {v:.4g}" for k, v in fig.items()))
        return fig
    return bb.assert_bf16_once(got, d.ref[:live], d.scale[:live], f32out=geo.f32out, what=what)


@pytest.mark.parametrize("geo", GEOS, ids=[g.id for g in GEOS])
def test_shipped_pairs_match_fp64_in_the_plans_layout(device, geo):
    impls = sc.enumerate_shipped()[0][geo]
    small = _Data(geo, device, sc.reduced_hw(geo.H), sc.BATCH, sc.LIVE)
    full = None
    bad = []
    for impl, users in impls.items():
        what = f"{geo.id} impl {impl}"
        print(f"SHIPPED {what} [{sc.kernel_file(geo.dtype, impl)}] {len(users)} program buckets, first {users[0]}")
        listed = sc.REFUSES_REDUCED.get(sc.refusal_key(geo, impl))
        refused = None
        try:
            _run(device, small, impl, what)
        except RuntimeError as e:
            if not _is_refusal(e):
                raise
            refused = str(e)
        except AssertionError as e:
            bad.append((impl, str(e)))
        if listed is not None and (refused is None or listed not in refused):
            bad.append((impl, f"REFUSES_REDUCED expects {listed!r} at {small.H}x{small.H}, got {refused!r}"))
        if refused is None:
            continue
        if listed is None:
            bad.append((impl, f"refuses the reduced {small.H}x{small.H} map and is not in REFUSES_REDUCED: {refused}"))
        if geo.H == small.H:
            bad.append((impl, f"the table ships a kernel that cannot run this layer: {refused}"))
            continue
        full = full or _Data(geo, device, geo.H, 1, 1)  # the plan's own map, one image
        try:
            _run(device, full, impl, what + f" at {geo.H}x{geo.H}")
        except RuntimeError as e:
            if not _is_refusal(e):
                raise
            bad.append((impl, f"the table ships a kernel that cannot run this layer: {e}"))
        except AssertionError as e:
            bad.append((impl, str(e)))
    assert not bad, bad
