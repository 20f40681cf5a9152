"""Planner side of ``ARENA_C3_BNECK`` on the CPU: off changes nothing, on plans ten fused ops that validate and never
write what they read, and the three-slot buffer with cv3's swapped halves computes the unfused block."""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from inference_arena_amd.engine import plans, tuning
from inference_arena_amd.engine.planner import OP_C3BNECK, OP_CONV, ProgramBuilder, View
from inference_arena_amd.engine.validate import validate_program
from inference_arena_amd.models.common import init_random_
from inference_arena_amd.models.yolov5nu import C3
from inference_arena_amd.models.zoo import make_yolo


def _detector(monkeypatch, switch):
    if switch is None:
        monkeypatch.delenv("ARENA_C3_BNECK", raising=False)
    else:
        monkeypatch.setenv("ARENA_C3_BNECK", switch)
    return plans.plan_detector(make_yolo(0), conf_thr=0.5, iou_thr=0.45, dtype="fp32")


def test_switch_off_is_the_parent_program(monkeypatch):
    unset, off = _detector(monkeypatch, None), _detector(monkeypatch, "0")
    assert np.array_equal(off.ops, unset.ops) and np.array_equal(off.weights, unset.weights)
    assert tuning.fingerprint(off.ops) == tuning.fingerprint(unset.ops)
    assert [(b.name, b.per_item, b.first, b.last) for b in off.buffers] == \
           [(b.name, b.per_item, b.first, b.last) for b in unset.buffers]
    assert tuning.lookup(unset.ops, 1) is not None  # still the program the shipped table was tuned for


def test_switch_on_plans_ten_fused_bottlenecks(monkeypatch):
    off, on = _detector(monkeypatch, None), _detector(monkeypatch, "1")
    kinds = lambda p, k: int((p.ops[:, 0] == k).sum())  # noqa: E731
    # ten (1x1, 3x3) conv pairs become ten ops: ten ops fewer, twenty convs fewer
    assert kinds(on, OP_C3BNECK) == 10 and len(on.ops) == len(off.ops) - 10
    assert kinds(on, OP_CONV) == kinds(off, OP_CONV) - 20
    assert not any(b.name.endswith(".U") for b in on.buffers if b.last >= 0)
    for B in (1, 32):
        validate_program(on, B, 16, max_det=300, cand_cap=8400)
    for r in on.ops[on.ops[:, 0] == OP_C3BNECK]:
        (xb, xc), (yb, yc), c = (int(r[1]), int(r[2])), (int(r[12]), int(r[13])), int(r[6])
        assert xb != yb or xc + c <= yc or yc + c <= xc, r[:16]


def _planes_weight(blob, off, c, taps):
    """pack_conv_weight_x3 planes [taps * c / 32][c][h | m | l][32] at ``off`` -> fp32 [c, c, k, k]."""
    n = taps * (c // 32) * c * 96
    p = torch.from_numpy(blob[off:off + 2 * n].view(np.int16).copy()).view(torch.bfloat16)
    w = p.reshape(taps, c // 32, c, 3, 32).double().sum(3).float()  # [tap][chunk][n][k]
    k = int(taps ** 0.5)
    return w.permute(2, 1, 3, 0).reshape(c, c, k, k)


def _run(prog, x, dst_id):
    """The program's convs and fused bottlenecks in torch fp32 over NCHW buffers."""
    bufs = {b.id: torch.zeros(1, b.C, b.H, b.W) for b in prog.buffers}
    bufs[0] = x
    f32 = lambda off, n: torch.from_numpy(prog.weights[off:off + 4 * n].view(np.float32).copy())  # noqa: E731
    for r in prog.ops:
        if int(r[0]) == OP_CONV:
            d = ProgramBuilder.decode_conv(r)
            w = f32(d["w_off"], d["Cout_pad"] * d["Kpad"]).reshape(d["Cout_pad"], d["Kpad"])[:d["Cout"], :d["Cin"]]
            xin = bufs[d["x_buf"]][:, d["x_coff"]:d["x_coff"] + d["Cin"]]
            y = F.silu(F.conv2d(xin, w.reshape(d["Cout"], d["Cin"], 1, 1), f32(d["b_off"], d["Cout"])))
            bufs[d["y_buf"]][:, d["y_coff"]:d["y_coff"] + d["Cout"]] = y
        else:
            assert int(r[0]) == OP_C3BNECK
            c = int(r[6])
            xin = bufs[int(r[1])][:, int(r[2]):int(r[2]) + c]
            u = F.silu(F.conv2d(xin, _planes_weight(prog.weights, int(r[8]), c, 1), f32(int(r[9]), c)))
            y = F.silu(F.conv2d(u, _planes_weight(prog.weights, int(r[10]), c, 9), f32(int(r[11]), c), padding=1))
            bufs[int(r[12])][:, int(r[13]):int(r[13]) + c] = y + xin if int(r[7]) else y
    return bufs[dst_id]


@pytest.mark.parametrize("n", [1, 2])  # odd: the chain ends in slot 2 and cv3's halves swap; even: slot 0
def test_three_slot_block_computes_the_c3_block(monkeypatch, n):
    m = init_random_(C3(64, 64, n=n, shortcut=True), 7 + n).eval()
    x = torch.randn(1, 64, 9, 11, generator=torch.Generator().manual_seed(n))
    monkeypatch.setenv("ARENA_C3_BNECK", "1")
    pb = ProgramBuilder("fp32")
    src, dst = pb.tensor("x", 9, 11, 64), pb.tensor("y", 9, 11, 64)
    plans._c3(pb, m, View(src, 0, 64), View(dst, 0, 64), 9, 11, "blk")
    prog = pb.build()
    assert int((prog.ops[:, 0] == OP_C3BNECK).sum()) == n
    cv3 = ProgramBuilder.decode_conv(prog.ops[-1])
    assert (cv3["x_coff"], cv3["Cin"]) == ((32, 64) if n % 2 else (0, 64))
    with torch.no_grad():
        ref = m(x)
    got = _run(prog, x.clone(), dst.id)
    assert (got - ref).abs().max().item() < 2e-5 * (1.0 + ref.abs().max().item())
