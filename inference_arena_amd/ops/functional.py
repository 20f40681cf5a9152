"""Tensor-level wrappers around the HIP kernels (torch tensors on ROCm).

These call the same launchers the executor uses, on the current torch stream,
so every kernel can be tested against a PyTorch fp32 reference op and used
outside the executor.  Activations are NHWC tensors — bf16 for the tuned bf16
kernels, float32 for the exact-fp32 kernels (selected by the input dtype); a
"view" into a concat buffer is passed as the buffer plus a channel offset.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np
import torch

from ..engine.planner import ACT, pack_conv_weight, pack_conv_weight_x3
from . import native

IMAGE_META = struct.Struct("<qiiiiiif12x")  # must match arena::ImageMeta (48 bytes)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: torch.Tensor | None, elem_off: int = 0) -> int:
    if t is None:
        return 0
    return t.data_ptr() + elem_off * t.element_size()


def pack_weights(w: torch.Tensor, b: torch.Tensor, device, dtype: str = "bf16"):
    """-> (weights, bias, Kpad, Cout_pad, w3): ``w3`` the pre-split bf16 planes of the fp32 x3g kernels
    (planner.pack_conv_weight_x3; None for bf16)."""
    wb, bb, kpad, cpad = pack_conv_weight(w.detach().cpu().float(), b.detach().cpu().float(), dtype)
    wt = torch.frombuffer(bytearray(wb), dtype=torch.float32 if dtype == "fp32" else torch.bfloat16).to(device)
    bt = torch.frombuffer(bytearray(bb), dtype=torch.float32).to(device)
    w3 = None
    if dtype == "fp32":
        w3 = torch.frombuffer(bytearray(pack_conv_weight_x3(w.detach().cpu().float())), dtype=torch.int16).to(device)
    return wt, bt, kpad, cpad, w3


def conv2d_nhwc(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, *, stride: int = 1, pad=None, act=None,
                x_coff: int = 0, cin: int | None = None, out: torch.Tensor | None = None, out_coff: int = 0,
                res: torch.Tensor | None = None, res_coff: int = 0, out2: torch.Tensor | None = None,
                out2_coff: int = 0, f32out: bool = False, out_hw=None, bdev: torch.Tensor | None = None,
                packed=None, impl: int = 0, pw=None, pw_out: torch.Tensor | None = None, pw_out_coff: int = 0,
                gate=None, window=None, marks=None) -> torch.Tensor:
    """NHWC conv with fused bias/act/residual/upsampled copy.

    ``window=(n_lo, n_hi)`` (x3hp kernels, impl 191 + v, only): compute and store only the output channels
    [n_lo, n_hi); the rest of ``out`` keeps its contents.  ``marks=(m, uh, uw, halo)`` (x3hp only): int32 ``m``
    [B, ceil(Ho / 8), ceil(Wo / 8)] cell marks (``head_mark``); an output tile that no continuing ``uh`` x ``uw``
    consumer tile grown by ``halo`` pixels reads is skipped and keeps its contents (ConvParams.marks).

    ``pw=(w2, b2)`` (fp32 3x3 stride-1 only): the Detect-head 1x1 ``w2`` [C2, Cout, 1, 1] is applied to the
    activated result inside the x3hg epilogue (impl 145 + v) and only its [B, Ho, Wo, C2] output is returned (a
    bf16 ``x``: the v3 halo-tile kernel's epilogue, csrc/kernels/conv3x3_v3.hip, bf16 output);
    ``pw_out`` (float32 / bf16 as the output, [B, Ho, Wo, C], optional): write those C2 channels at ``pw_out_coff`` of it instead and
    return it.  ``gate=(logits, coff, n, gate_min)`` (x3hg fused-1x1 kernels only): float32 ``logits`` with the shape
    of the tensor the 1x1 output is written to; a tile none of whose pixels has ``logits[..., coff:coff + n] >=
    gate_min`` is skipped and keeps its previous contents (ConvParams.gate).

    x: [B, H, W, Cx] bf16 or float32 (reads channels [x_coff, x_coff + Cin)); w: [Cout, Cin, KH, KW] fp32.
    A float32 ``x`` runs the exact-fp32 kernel (fp32 weights, v_mfma_f32_16x16x4_f32, fp32 output).
    ``impl`` pins a kernel (0 = the dispatch policy; fp32: 1 direct, 2 LDS, 10 + v LDS tile variant v,
    40 + v triple-bf16-split variant v, 100 halo, 101 split halo, 102 / 103 split halo with 48 / 32-channel
    tiles, 104 / 105 weight-stationary streaming 1x1 (auto / 32-channel tiles), 111 + v the x3g 32x32x16 GEMM
    over pre-split weights, 191 + v the 16-wide split halo tiles over pre-split weights — the whole table: csrc/kernels/f32_impl.h).
    """
    f32 = x.dtype == torch.float32
    B, H, W, Cx = x.shape
    cout, cin_w, kh, kw = w.shape
    cin = cin or cin_w
    if pad is None:
        pad = (kh // 2, kw // 2)
    if isinstance(pad, int):
        pad = (pad, pad)
    if out_hw is None:
        Ho = (H + 2 * pad[0] - kh) // stride + 1
        Wo = (W + 2 * pad[1] - kw) // stride + 1
    else:
        Ho, Wo = out_hw
    if out is None:
        out = torch.empty(B, Ho, Wo, cout, dtype=torch.float32 if (f32out or f32) else torch.bfloat16, device=x.device)
    wt, bt, kpad, cpad, w3 = packed if packed is not None else pack_weights(w, b, x.device, "fp32" if f32 else "bf16")
    pwd = {}
    if pw is not None:
        from ..engine.planner import pack_pw_weight_x3

        w2, b2 = pw
        co2 = w2.shape[0]
        if f32:
            k2 = (cout + 31) // 32 * 32
            w2p = torch.frombuffer(bytearray(pack_pw_weight_x3(w2.detach().cpu().float(), k2)),
                                   dtype=torch.int16).to(x.device)
            b2p = torch.zeros((co2 + 15) // 16 * 16)
            b2p[:co2] = b2.detach().float()
            b2p = b2p.to(x.device)
        else:  # bf16 (conv3x3_v3.hip): W2 [Cout2_pad][Kpad2] bf16 as the planner packs it, bf16 output
            if gate is not None:
                raise ValueError("conv2d_nhwc: the tile gate is an fp32 x3hg option")
            w2p, b2p, k2, _, _ = pack_weights(w2, b2, x.device, "bf16")
        pw_dtype = torch.float32 if f32 else torch.bfloat16
        if pw_out is None:
            out = torch.empty(B, Ho, Wo, co2, dtype=pw_dtype, device=x.device)
            pw_out_coff = 0
        else:
            out = pw_out
            if (out.shape[:3] != (B, Ho, Wo) or out.shape[3] < pw_out_coff + co2 or out.dtype != pw_dtype
                    or out.device != x.device or not out.is_contiguous()):
                raise ValueError(f"conv2d_nhwc: pw_out {tuple(out.shape)} {out.dtype} does not fit the 1x1 output")
        pwd = {"pw_w": _ptr(w2p), "pw_bias": _ptr(b2p), "pw_y": _ptr(out, pw_out_coff), "pw_ys": out.shape[-1],
               "pw_cout": co2, "pw_kpad": k2, "pw_act": 0}
        if gate is not None:
            gt, gcoff, gn, gmin = gate
            if (gt.shape != out.shape or gt.dtype != torch.float32 or gt.device != x.device or not gt.is_contiguous()
                    or gcoff < 0 or gn <= 0 or gcoff + gn > gt.shape[3]):
                raise ValueError("conv2d_nhwc: the gate logits must match the 1x1 output tensor's shape and stride")
            pwd.update({"gate": _ptr(gt, gcoff), "gate_n": int(gn), "gate_min": float(gmin)})
    elif gate is not None or pw_out is not None:
        raise ValueError("conv2d_nhwc: gate / pw_out need pw")
    if window is not None:
        pwd.update({"n_lo": int(window[0]), "n_hi": int(window[1])})
    if marks is not None:
        mt, uh, uw, halo = marks
        if (mt.dtype != torch.int32 or mt.device != x.device or not mt.is_contiguous()
                or tuple(mt.shape) != (B, (Ho + 7) // 8, (Wo + 7) // 8)):
            raise ValueError("conv2d_nhwc: marks must be contiguous int32 [B, ceil(Ho / 8), ceil(Wo / 8)]")
        pwd.update({"marks": _ptr(mt), "mark_uh": int(uh), "mark_uw": int(uw), "mark_halo": int(halo)})
    skd = {}
    if 171 <= int(impl) < 180:  # split-K x3g: a workspace for the partial tiles (splits <= 8)
        ws = torch.empty(8 * B * Ho * Wo * cpad, dtype=torch.float32, device=x.device)
        skd = {"sk_ws": _ptr(ws), "sk_ws_bytes": ws.numel() * 4}
    native().conv2d({
        "x": _ptr(x, x_coff), "B": B, "H": H, "W": W, "xs": Cx, "Cin": cin,
        "w": _ptr(wt), "Kpad": kpad, "bias": _ptr(bt),
        "y": _ptr(out, out_coff), "Ho": Ho, "Wo": Wo, "ys": out.shape[-1], "Cout": cout, "Cout_pad": cpad,
        "KH": kh, "KW": kw, "stride": stride, "pad_t": pad[0], "pad_l": pad[1],
        "res": _ptr(res, res_coff), "rs": res.shape[-1] if res is not None else 0,
        "y2": _ptr(out2, out2_coff), "y2s": out2.shape[-1] if out2 is not None else 0,
        "act": ACT[act], "f32out": int(f32out), "bdev": _ptr(bdev), "stream": _stream(), "f32": int(f32),
        "impl": int(impl), "w3": _ptr(w3), **pwd, **skd,
    })
    if pw is not None:
        torch.cuda.synchronize(x.device)  # keep the packed 1x1 weights alive until the kernel ran
    return out


def head_mark(logits: torch.Tensor, coff: int, n: int, gate_min: float, marks: torch.Tensor | None = None,
              bdev: torch.Tensor | None = None, levels=None) -> torch.Tensor | list:
    """Detect-head cell marks (csrc/kernels/head_mark.hip): int32 [B, ceil(H / 8), ceil(W / 8)], 1 iff one of
    ``logits[b, y, x, coff:coff + n]`` (float32 [B, H, W, C]) of an in-map pixel of the 8 x 8 cell is >= gate_min.
    Cells of images at or past the live count (``bdev``) keep the contents of ``marks``.  ``levels``: further
    (logits, marks) pairs marked by the same launch; the result is then the list of all mark tensors."""
    lv = [(logits, marks)] + list(levels or [])
    out = []
    for lg, mk in lv:
        B, H, W, C = lg.shape
        if lg.dtype != torch.float32 or not lg.is_contiguous() or coff < 0 or coff + n > C:
            raise ValueError("head_mark: logits must be contiguous float32 [B, H, W, >= coff + n]")
        if mk is None:
            mk = torch.zeros(B, (H + 7) // 8, (W + 7) // 8, dtype=torch.int32, device=lg.device)
        if (mk.dtype != torch.int32 or mk.device != lg.device or not mk.is_contiguous()
                or tuple(mk.shape) != (B, (H + 7) // 8, (W + 7) // 8) or B != lv[0][0].shape[0]):
            raise ValueError("head_mark: marks must be contiguous int32 [B, ceil(H / 8), ceil(W / 8)]")
        out.append(mk)
    native().head_mark({"logits": [_ptr(lg, coff) for lg, _ in lv], "marks": [_ptr(mk) for mk in out],
                        "H": [lg.shape[1] for lg, _ in lv], "W": [lg.shape[2] for lg, _ in lv],
                        "ps": [lg.shape[3] for lg, _ in lv], "n": int(n), "gate_min": float(gate_min),
                        "B": lv[0][0].shape[0], "bdev": _ptr(bdev), "stream": _stream()})
    return out if levels else out[0]


def dwconv3x3_nhwc(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, *, stride: int = 1, act="relu6",
                   bdev: torch.Tensor | None = None) -> torch.Tensor:
    B, H, W, C = x.shape
    f32 = x.dtype == torch.float32
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty(B, Ho, Wo, C, dtype=x.dtype, device=x.device)
    wt = w.detach().float().reshape(C, 9).t().contiguous().to(x.dtype).to(x.device)
    bt = b.detach().float().contiguous().to(x.device)
    native().dwconv3x3({"x": _ptr(x), "B": B, "H": H, "W": W, "xs": C, "C": C, "w": _ptr(wt), "bias": _ptr(bt),
                        "y": _ptr(y), "Ho": Ho, "Wo": Wo, "ys": C, "stride": stride, "act": ACT[act],
                        "bdev": _ptr(bdev), "stream": _stream(), "f32": int(f32)})
    return y


def ir_block_nhwc(x: torch.Tensor, expand, dw, project, *, stride: int, res: bool = False,
                  bdev: torch.Tensor | None = None, x_parts: int = 1, y_parts: int = 1,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """Fused MobileNetV2 inverted residual (expand 1x1+ReLU6 -> dw3x3+ReLU6 -> project 1x1 [+x]).
    ``expand``/``dw``/``project`` are (weight, bias) pairs with BN folded; ``expand`` None for t=1.
    ``x_parts`` / ``y_parts`` (fp32 14x14 whole-map kernel): ``x`` holds x_parts partial sums of the input side by
    side on the channel axis; the result holds y_parts partial sums (hidden channels split over workgroups).
    ``out``: a contiguous [B, Ho, Wo, >= oup * y_parts] tensor to write into (its last extent is the output's
    channel stride; channels past the block's are left as they are) instead of a fresh one."""
    from ..engine.planner import ir_x3_plan, pack_ir_weights, split_bf16x3

    B, H, W, Ct = x.shape
    C = Ct // x_parts
    f32 = x.dtype == torch.float32  # fp32 kernels (csrc/kernels/ir_f32.hip, ir_crop_f32.hip, ir_tile_x3.hip)
    pk = pack_ir_weights(expand, dw, project, C, k_align=16 if f32 else 32)
    x3w = 0
    if f32:
        x3w, inp_x3 = ir_x3_plan(H, W, stride, C, pk["hid_pad"], pk["oup_pad"], int(expand is not None))
        if x3w and inp_x3 != pk["inp_pad"]:
            pk = pack_ir_weights(expand, dw, project, C, k_align=32)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = out if out is not None else torch.empty(B, Ho, Wo, pk["oup"] * y_parts, dtype=x.dtype, device=x.device)
    if (y.shape[:3] != (B, Ho, Wo) or y.shape[3] < pk["oup"] * y_parts or y.dtype != x.dtype or y.device != x.device
            or not y.is_contiguous()):
        raise ValueError(f"ir_block_nhwc: out {tuple(y.shape)} {y.dtype} does not fit the block's output")
    mat = torch.float32 if f32 else torch.bfloat16
    dev = {k: (pk[k].to(mat) if k in ("we", "wd", "wp") else pk[k].float()).contiguous().to(x.device)
           for k in ("we", "be", "wd", "bd", "wp", "bp")}
    if x3w:  # the whole-map kernel reads pre-split [h|m|l] bf16 expand / project weights
        dev["we"] = split_bf16x3(pk["we"]).to(x.device)
        dev["wp"] = split_bf16x3(pk["wp"]).to(x.device)
    native().ir_block({"x": _ptr(x), "x_cs": Ct, "H": H, "W": W, "inp": C, "inp_pad": pk["inp_pad"],
                       "hid_pad": pk["hid_pad"], "oup": pk["oup"], "oup_pad": pk["oup_pad"], "stride": stride,
                       "expand": int(expand is not None), "res": int(res),
                       **{k: _ptr(v) for k, v in dev.items()}, "y": _ptr(y), "y_cs": y.shape[3], "Ho": Ho,
                       "Wo": Wo, "B": B, "bdev": _ptr(bdev), "stream": _stream(), "f32": int(f32), "x3w": x3w,
                       "x_parts": x_parts, "y_parts": y_parts})
    torch.cuda.synchronize(x.device)  # keep the packed weights alive until the kernel ran
    return y


def c3_x3_nhwc(x: torch.Tensor, cv12, bottleneck, cv3) -> torch.Tensor:
    """fp32 YOLOv5 C3 block at 160x160 geometry (C1 32, c_ 16, one bottleneck with shortcut) as one kernel
    (csrc/kernels/c3_x3.hip); ``cv12`` = (w [32, 32, 1, 1], b) of cv1|cv2 stacked, ``bottleneck`` =
    ((w1 [16, 16, 1, 1], b1), (w2 [16, 16, 3, 3], b2)), ``cv3`` = (w [32, 32, 1, 1], b); BN folded."""
    from ..engine.planner import split_bf16x3

    B, H, W, C = x.shape
    (w1, b1), (w2, b2) = bottleneck
    w2k = torch.zeros(16, 160)
    w2k[:, :144] = w2.detach().float().permute(0, 2, 3, 1).reshape(16, 144)
    dev = {"w12": split_bf16x3(cv12[0].reshape(32, 32)), "b12": cv12[1].float(),
           "wb1": split_bf16x3(w1.reshape(16, 16)), "bb1": b1.float(), "wb2": split_bf16x3(w2k), "bb2": b2.float(),
           "w3": split_bf16x3(cv3[0].reshape(32, 32)), "b3": cv3[1].float()}
    dev = {k: v.contiguous().to(x.device) for k, v in dev.items()}
    y = torch.empty(B, H, W, 32, dtype=torch.float32, device=x.device)
    native().c3_block({"x": _ptr(x), "xs": C, "B": B, "H": H, "W": W, "bdev": 0, "C1": 32, "CH": 16, "NB": 1,
                       "res": 1, **{k: _ptr(v) for k, v in dev.items()}, "y": _ptr(y), "ys": 32,
                       "stream": _stream(), "f32": 1})
    torch.cuda.synchronize(x.device)
    return y


def c3_fused_nhwc(x: torch.Tensor, cv12, bottleneck, cv3, *, n: int = 1, shortcut: bool = True, x_coff: int = 0,
                  c1: int | None = None, out: torch.Tensor | None = None, out_coff: int = 0,
                  bdev: torch.Tensor | None = None) -> torch.Tensor:
    """bf16 YOLOv5 C3 block as one kernel (csrc/kernels/c3_fused.hip): C1 32 / c_ 16 / n 1 / shortcut, C1 64 / c_ 32 /
    n 2 / shortcut or C1 128 / c_ 32 / n 1 / no shortcut, on a map of whole 8 x 16 tiles.  ``cv12`` = (w [2c_, C1, 1,
    1], b) of cv1|cv2 stacked, ``bottleneck`` = ((w1 [c_, c_, 1, 1], b1), (w2 [c_, c_, 3, 3], b2)) — one weight set,
    applied ``n`` times —, ``cv3`` = (w [2c_, 2c_, 1, 1], b); BN folded.  Reads channels [x_coff, x_coff + C1) of
    ``x``; ``out``: a contiguous bf16 [B, H, W, >= out_coff + 2c_] tensor to write channels [out_coff, out_coff +
    2c_) of (the rest is left as it is) instead of a fresh one."""
    B, H, W, Cx = x.shape
    (w1, b1), (w2, b2) = bottleneck
    ch = w1.shape[0]
    c1 = c1 or cv12[0].shape[1]
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or x_coff < 0 or x_coff + c1 > Cx:
        raise ValueError("c3_fused_nhwc: x must be contiguous bf16 [B, H, W, >= x_coff + C1]")
    if x_coff % 8 or out_coff % 4:  # 16-byte loads, 8-byte stores
        raise ValueError("c3_fused_nhwc: x_coff must be a multiple of 8 and out_coff of 4")
    if cv12[0].shape[:2] != (2 * ch, c1) or cv3[0].shape[:2] != (2 * ch, 2 * ch) or w2.shape != (ch, ch, 3, 3):
        raise ValueError("c3_fused_nhwc: weight shapes do not form a C3 block")
    if out is None:
        out = torch.empty(B, H, W, 2 * ch, dtype=torch.bfloat16, device=x.device)
    if (out.shape[:3] != (B, H, W) or out_coff < 0 or out.shape[3] < out_coff + 2 * ch or out.dtype != torch.bfloat16
            or out.device != x.device or not out.is_contiguous()):
        raise ValueError(f"c3_fused_nhwc: out {tuple(out.shape)} {out.dtype} does not fit the block's output")
    w1p = torch.zeros(ch, 32, 1, 1)  # [c_][32]: the kernel reads T's first 32 channels, columns past c_ are zero
    w1p[:, :ch] = w1.detach().float().reshape(ch, ch, 1, 1)
    dev = {}
    for k, (w, b) in (("12", cv12), ("b1", (w1p, b1)), ("b2", (w2, b2)), ("3", cv3)):
        wt, bt = pack_weights(w, b, x.device, "bf16")[:2]
        dev["w" + k], dev["b" + k] = wt, bt
    native().c3_block({"x": _ptr(x, x_coff), "xs": Cx, "B": B, "H": H, "W": W, "bdev": _ptr(bdev), "C1": c1, "CH": ch,
                       "NB": n, "res": int(shortcut), **{k: _ptr(v) for k, v in dev.items()},
                       "y": _ptr(out, out_coff), "ys": out.shape[3], "stream": _stream(), "f32": 0})
    torch.cuda.synchronize(x.device)  # keep the packed weights alive until the kernel ran
    return out


def sppf_nhwc(buf: torch.Tensor, C: int) -> torch.Tensor:
    """In place: buf[..., C:4C] = cascaded 5x5 max pools of buf[..., :C]."""
    B, H, W, Ct = buf.shape
    native().sppf_pool({"buf": _ptr(buf), "B": B, "H": H, "W": W, "xs": Ct, "C": C, "stream": _stream(),
                        "f32": int(buf.dtype == torch.float32)})
    return buf


def image_meta_bytes(images: list[np.ndarray], T: int) -> tuple[bytes, np.ndarray]:
    """Pack images into one uint8 pool (256-B aligned) + ImageMeta records."""
    from ..processing.transforms import letterbox_geometry

    metas, chunks, off = [], [], 0
    for im in images:
        h, w = im.shape[:2]
        scale, nw, nh, pw, ph = letterbox_geometry(h, w, T)
        metas.append(IMAGE_META.pack(off, h, w, nw, nh, pw, ph, scale))
        data = np.ascontiguousarray(im, np.uint8).tobytes()
        pad = (-len(data)) % 256
        chunks.append(data + b"\0" * pad)
        off += len(data) + pad
    return b"".join(metas), np.frombuffer(b"".join(chunks), dtype=np.uint8)


def ctrl_tensor(n_images: int, device, n_crops: int = 0, crop_base: int = 0) -> torch.Tensor:
    c = torch.zeros(16, dtype=torch.int32)
    c[0], c[1], c[2] = n_images, n_crops, crop_base
    return c.to(device)


def letterbox_s2d(images: list[np.ndarray], T: int, device, dtype=torch.bfloat16) -> torch.Tensor:
    meta, pool = image_meta_bytes(images, T)
    meta_t = torch.frombuffer(bytearray(meta), dtype=torch.uint8).to(device)
    pool_t = torch.from_numpy(pool.copy()).to(device)
    ctrl = ctrl_tensor(len(images), device)
    out = torch.empty(len(images), T // 2, T // 2, 16, dtype=dtype, device=device)
    native().letterbox_s2d({"pool": _ptr(pool_t), "meta": _ptr(meta_t), "ctrl": _ptr(ctrl), "out": _ptr(out),
                            "B": len(images), "T": T, "stream": _stream(), "f32": int(dtype == torch.float32)})
    torch.cuda.current_stream().synchronize()
    return out


POOL_SLACK = 8  # bytes the staged source loads of stem_fused.hip may read behind an image's last byte


def image_pool(images: list[np.ndarray], T: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """(ImageMeta records, uint8 pool) on ``device`` for the fused front ends: ``image_meta_bytes`` plus one more
    256-byte pad block when fewer than POOL_SLACK pad bytes follow the last image (csrc/kernels/stem_fused.hip
    stages source rows with whole aligned dwords and reads up to 7 bytes past a row's end)."""
    meta, pool = image_meta_bytes(images, T)
    if images and (-images[-1].size) % 256 < POOL_SLACK:
        pool = np.concatenate([pool, np.zeros(256, np.uint8)])
    meta_t = torch.frombuffer(bytearray(meta), dtype=torch.uint8).to(device)
    return meta_t, torch.from_numpy(pool.copy()).to(device)


def stem_fused_nhwc(pool: torch.Tensor, meta: torch.Tensor, ctrl: torch.Tensor, stem, *, S: int, act,
                    out: torch.Tensor, crops: torch.Tensor | None = None, mean=None, inv_std=None,
                    second=None, ir=None) -> torch.Tensor:
    """bf16 front end as one kernel (csrc/kernels/stem_fused.hip), the four forms the planner emits:

    * letterbox to ``S`` -> detector stem: ``stem`` = (w [16, 16, 3, 3] over the space-to-depth input, b);
      ``out`` [cap, S/2, S/2, >= 16];
    * the same -> 3x3 stride-2 conv: ``second`` = (w2 [32, 16, 3, 3], b2, act2); ``out`` [cap, S/4, S/4, >= 32],
      S a multiple of 64;
    * crop gather (``crops``: CropRef records, int32 [n, 8]; ``mean`` / ``inv_std``) -> classifier stem: ``stem`` =
      (w [32, 16, 2, 2], b); ``out`` [cap, S/2, S/2, >= 32];
    * the same -> MobileNetV2 block 1: ``ir`` = ((wd [32, 1, 3, 3], bd), (wp [16, 32, 1, 1], bp)); ``out``
      [cap, S/2, S/2, >= 16], S a multiple of 32.

    ``pool`` / ``meta``: ``image_pool``; ``ctrl``: ``ctrl_tensor`` (live images, live crops, crop base).  ``out``
    is a contiguous bf16 tensor whose first extent is the batch capacity and whose last extent is the pixel stride:
    items past the live count and channels past the form's are left as they are.  Weights are packed as the planner
    packs them (pack_conv_weight, pack_ir_weights)."""
    from ..engine.planner import pack_ir_weights

    w, b = stem
    if w.dim() != 4 or w.shape[1] != 16 or w.shape[2] != w.shape[3] or w.shape[0] % 16:
        raise ValueError("stem_fused_nhwc: stem weights must be [Cout, 16, KS, KS] with Cout a multiple of 16")
    if second is not None and ir is not None:
        raise ValueError("stem_fused_nhwc: second (detector) and ir (classifier) exclude each other")
    if (w.shape[2] != 3 or ir is not None) if crops is None else (w.shape[2] != 2 or second is not None):
        raise ValueError("stem_fused_nhwc: the 3x3 stem (and second) letterbox images, the 2x2 stem (and ir) "
                         "gathers crops")
    if S <= 0 or S % 2:
        raise ValueError("stem_fused_nhwc: S must be positive and even")
    cout, ks = w.shape[0], w.shape[2]
    if second is not None:
        side, cdst = S // 4, second[0].shape[0]
        if tuple(second[0].shape[1:]) != (cout, 3, 3):
            raise ValueError("stem_fused_nhwc: second conv must be [C2, Cout, 3, 3]")
    elif ir is not None:
        (wd, _), (wp, _) = ir
        side, cdst = S // 2, wp.shape[0]
        if tuple(wd.shape) != (cout, 1, 3, 3) or tuple(wp.shape[1:]) != (cout, 1, 1):
            raise ValueError("stem_fused_nhwc: fused block must be depthwise [Cout, 1, 3, 3] + project [C, Cout, 1, 1]")
    else:
        side, cdst = S // 2, cout
    if (out.dim() != 4 or out.shape[1] != side or out.shape[2] != side or out.shape[3] < cdst or out.shape[3] % 4
            or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != pool.device):
        raise ValueError(f"stem_fused_nhwc: out {tuple(out.shape)} {out.dtype} does not fit the form's output "
                         f"[cap, {side}, {side}, >= {cdst} and a multiple of 4] bf16")
    if pool.dtype != torch.uint8 or ctrl.dtype != torch.int32 or ctrl.numel() < 3:
        raise ValueError("stem_fused_nhwc: pool must be uint8 and ctrl the int32 control block")
    if crops is not None and (crops.dtype != torch.int32 or crops.dim() != 2 or crops.shape[1] != 8
                              or not crops.is_contiguous()):
        raise ValueError("stem_fused_nhwc: crops must be contiguous int32 [n, 8] CropRef records")
    dev = pool.device
    wt, bt, kpad, _ = pack_weights(w, b, dev, "bf16")[:4]
    d = {"src": 0 if crops is None else 1, "pool": _ptr(pool), "meta": _ptr(meta), "ctrl": _ptr(ctrl),
         "crops": _ptr(crops), "cap": out.shape[0], "S": S, "KS": ks, "w": _ptr(wt), "Kpad": kpad, "bias": _ptr(bt),
         "Cout": cout, "act": ACT[act], "stream": _stream()}
    if mean is not None:
        d["mean"], d["inv_std"] = [float(v) for v in mean], [float(v) for v in inv_std]
    keep = [wt, bt]
    if second is not None:
        w2, b2, act2 = second
        w2t, b2t, kpad2, _ = pack_weights(w2, b2, dev, "bf16")[:4]
        keep += [w2t, b2t]
        d.update({"w2": _ptr(w2t), "Kpad2": kpad2, "bias2": _ptr(b2t), "Cout2": w2.shape[0], "act2": ACT[act2],
                  "y2": _ptr(out), "y2s": out.shape[3]})
    elif ir is not None:
        pk = pack_ir_weights(None, ir[0], ir[1], cout)
        irt = {"ir_wd": pk["wd"].to(torch.bfloat16), "ir_bd": pk["bd"].float(), "ir_wp": pk["wp"].to(torch.bfloat16),
               "ir_bp": pk["bp"].float()}
        irt = {k: v.contiguous().to(dev) for k, v in irt.items()}
        keep += list(irt.values())
        d.update({k: _ptr(v) for k, v in irt.items()})
        d.update({"ir_y": _ptr(out), "ir_ys": out.shape[3]})
    else:
        d.update({"y": _ptr(out), "ys": out.shape[3]})
    native().stem_fused(d)
    torch.cuda.synchronize(dev)  # keep the packed weights alive until the kernel ran
    del keep
    return out


def s2d_to_nchw(x: torch.Tensor) -> torch.Tensor:
    """[B, h, w, 16] space-to-depth (12 live channels) -> [B, 3, 2h, 2w] fp32."""
    B, h, w, _ = x.shape
    y = x[..., :12].float().reshape(B, h, w, 2, 2, 3)  # p, q, c
    return y.permute(0, 5, 1, 3, 2, 4).reshape(B, 3, 2 * h, 2 * w)


def avgpool_nhwc(x: torch.Tensor) -> torch.Tensor:
    B, H, W, C = x.shape
    y = torch.empty(B, C, dtype=x.dtype, device=x.device)
    native().global_avgpool({"x": _ptr(x), "B": B, "HW": H * W, "C": C, "y": _ptr(y), "stream": _stream(),
                             "f32": int(x.dtype == torch.float32)})
    return y


def head_pool_nhwc(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, act: str | None = "relu6",
                   bdev: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """mean over pixels of act(conv1x1(x, w) + b): [B,H,W,C] -> [B, N] (head_pool.hip); bf16 in/out, or fp32
    in/out (fp32-accurate triple-bf16-split kernel) for a float32 ``x``.  ``out``: a contiguous [B, N] tensor of
    ``x``'s dtype to write into (rows past the live count ``bdev`` keep their contents) instead of a fresh one."""
    from ..engine.planner import ACT, pack_conv_weight

    B, H, W, C = x.shape
    N = w.shape[0]
    f32 = x.dtype == torch.float32
    wb, bb, kpad, npad = pack_conv_weight(w, b, "fp32" if f32 else "bf16")
    wd = torch.frombuffer(bytearray(wb), dtype=torch.float32 if f32 else torch.bfloat16).to(x.device)
    bd = torch.frombuffer(bytearray(bb), dtype=torch.float32).to(x.device)
    y = out if out is not None else torch.empty(B, N, dtype=x.dtype, device=x.device)
    if y.shape != (B, N) or y.dtype != x.dtype or y.device != x.device or not y.is_contiguous():
        raise ValueError(f"head_pool_nhwc: out {tuple(y.shape)} {y.dtype} does not fit the pooled output")
    native().head_pool({"x": _ptr(x), "xs": C, "HW": H * W, "K": C, "w": _ptr(wd), "Kpad": kpad, "bias": _ptr(bd),
                        "N": N, "Npad": npad, "y": _ptr(y), "ys": N, "act": ACT[act], "B": B, "bdev": _ptr(bdev),
                        "stream": _stream(), "f32": int(f32)})
    torch.cuda.synchronize(x.device)  # keep the packed weights alive until the kernel ran
    return y


def topk_softmax(logits: torch.Tensor):
    """[B, N] fp32 -> (idx [B,5] int32, logit [B,5], prob [B,5])."""
    B, N = logits.shape
    out = torch.empty(B, 16, dtype=torch.int32, device=logits.device)
    native().topk_softmax({"logits": _ptr(logits), "B": B, "N": N, "ld": logits.stride(0), "out": _ptr(out),
                           "stream": _stream()})
    torch.cuda.current_stream().synchronize()
    o = out.cpu()
    return o[:, 0:5].clone(), o[:, 5:10].view(torch.float32).clone(), o[:, 10:15].view(torch.float32).clone()
