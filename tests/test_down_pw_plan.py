"""Planner side of ``ARENA_DOWN_PW`` on the CPU: off changes nothing; on, each backbone downsampling conv and the
cv1|cv2 1x1 behind it are one stride-2 conv record with a fused 1x1 that validates, in both C3 layouts."""
from __future__ import annotations

import numpy as np
import pytest

from inference_arena_amd.engine import plans, tuning
from inference_arena_amd.engine.planner import ACT, OP_CONV, ProgramBuilder
from inference_arena_amd.engine.validate import validate_program
from inference_arena_amd.models.zoo import make_yolo


def _detector(monkeypatch, switch, bneck):
    monkeypatch.setenv("ARENA_C3_BNECK", bneck)
    if switch is None:
        monkeypatch.delenv("ARENA_DOWN_PW", raising=False)
    else:
        monkeypatch.setenv("ARENA_DOWN_PW", switch)
    return plans.plan_detector(make_yolo(0), conf_thr=0.5, iou_thr=0.45, dtype="fp32")


@pytest.mark.parametrize("bneck", ["0", "1"])
def test_switch_off_is_the_parent_program(monkeypatch, bneck):
    unset, off = _detector(monkeypatch, None, bneck), _detector(monkeypatch, "0", bneck)
    assert np.array_equal(off.ops, unset.ops) and np.array_equal(off.weights, unset.weights)
    assert tuning.fingerprint(off.ops) == tuning.fingerprint(unset.ops)
    assert [(b.name, b.per_item, b.first, b.last) for b in off.buffers] == \
           [(b.name, b.per_item, b.first, b.last) for b in unset.buffers]
    if bneck == "0":
        assert tuning.lookup(unset.ops, 1) is not None  # still the program the shipped table was tuned for


@pytest.mark.parametrize("bneck", ["0", "1"])
def test_switch_on_fuses_the_three_backbone_pairs(monkeypatch, bneck):
    off, on = _detector(monkeypatch, None, bneck), _detector(monkeypatch, "1", bneck)
    convs = lambda p: [ProgramBuilder.decode_conv(r) for r in p.ops if int(r[0]) == OP_CONV]  # noqa: E731
    assert len(on.ops) == len(off.ops) - 3 and len(convs(on)) == len(convs(off)) - 3
    s2pw = [d for d in convs(on) if d["stride"] == 2 and d["pw_cout"] > 0]
    assert [(d["Cin"], d["Cout"], d["pw_cout"], d["pw_act"], d["act"]) for d in s2pw] == \
           [(ci, c, c, ACT["silu"], ACT["silu"]) for ci, c in ((32, 64), (64, 128), (128, 256))]
    assert not any(d["stride"] == 2 and d["pw_cout"] > 0 for d in convs(off))
    names = lambda p: {b.name for b in p.buffers}  # noqa: E731
    assert names(off) - names(on) == {"b3", "b5", "b7"} and names(on) <= names(off)
    t = {b.id: b.name for b in on.buffers}
    assert [t[d["pw_y_buf"]] for d in s2pw] == ["b4.T", "b6.T", "b8.T"] and all(d["pw_y_coff"] == 0 for d in s2pw)
    for B in (1, 32):
        validate_program(on, B, 16, max_det=300, cand_cap=8400)
