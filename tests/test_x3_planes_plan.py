"""x3 planes, planner side (``ARENA_X3_PLANES``; engine/planner.py OP_CONV fields 42-44, engine/validate.py,
engine/tuning.py): off leaves every program byte-identical; on marks conv -> conv edges with planes buffers that
the static check accepts, that decode_conv names, and that keep the plain program's tuning fingerprint."""
from __future__ import annotations

import numpy as np
import pytest

from inference_arena_amd.engine import tuning
from inference_arena_amd.engine.planner import OP_CONV, ProgramBuilder, layout
from inference_arena_amd.engine.plans import plan_detector, plan_pipeline
from inference_arena_amd.engine.validate import ProgramError, validate_program

PLANS = {"detector": lambda y, m: plan_detector(y, conf_thr=0.5, iou_thr=0.45, dtype="fp32"),
         "pipeline": lambda y, m: plan_pipeline(y, m, conf_thr=0.5, iou_thr=0.45, dtype="fp32")}
CHECK = dict(max_det=300, cand_cap=8400)


def _plan(models, monkeypatch, kind, switch):
    if switch is None:
        monkeypatch.delenv("ARENA_X3_PLANES", raising=False)
    else:
        monkeypatch.setenv("ARENA_X3_PLANES", switch)
    return PLANS[kind](*models)


@pytest.mark.parametrize("kind", list(PLANS))
def test_switch_off_is_the_plain_program(models, monkeypatch, kind):
    a, b = _plan(models, monkeypatch, kind, None), _plan(models, monkeypatch, kind, "0")
    assert a.ops.tobytes() == b.ops.tobytes() and a.weights.tobytes() == b.weights.tobytes()
    assert not a.ops[:, 42:46].any()
    la, lb = layout(a.buffers, 4, 64), layout(b.buffers, 4, 64)
    assert la[1] == lb[1] and la[0].tobytes() == lb[0].tobytes()
    assert [(x.name, x.per_item) for x in a.buffers] == [(x.name, x.per_item) for x in b.buffers]


@pytest.mark.parametrize("kind", list(PLANS))
def test_switch_on_marks_edges(models, monkeypatch, kind):
    plain, p = _plan(models, monkeypatch, kind, "0"), _plan(models, monkeypatch, kind, "1")
    readers = [i for i, r in enumerate(p.ops) if int(r[0]) == OP_CONV and int(r[43])]
    assert readers and p.weights.tobytes() == plain.weights.tobytes()
    cleared = p.ops.copy()
    cleared[:, 42:46] = 0
    assert cleared.tobytes() == plain.ops.tobytes()  # nothing but the four fields differs
    assert tuning.fingerprint(p.ops) == tuning.fingerprint(plain.ops)
    assert tuning.lookup(p.ops, 1) == tuning.lookup(plain.ops, 1) != None  # noqa: E711  the shipped entries
    for Bn in (1, 3):
        validate_program(p, Bn, 16, **CHECK)
    for i in readers:
        d = ProgramBuilder.decode_conv(p.ops[i])
        src = ProgramBuilder.decode_conv(p.ops[d["x3_src_op"] - 1])
        buf = p.buffers[d["x3_buf"]]
        assert src["y3_buf"] == d["x3_buf"] > 0 and int(p.ops[i][45]) == 0 and d["Cin"] % 32 == 0
        assert (src["y_buf"], src["y_coff"], src["Cout"], src["Ho"], src["Wo"]) == \
            (d["x_buf"], d["x_coff"], d["Cin"], d["H"], d["W"])
        assert buf.per_item == 6 * d["H"] * d["W"] * d["Cin"] and buf.first == d["x3_src_op"] - 1 and buf.last >= i


def test_validate_rejects_damaged_planes_fields(models, monkeypatch):
    p = _plan(models, monkeypatch, "detector", "1")
    i = next(i for i, r in enumerate(p.ops) if int(r[0]) == OP_CONV and int(r[43]))
    keep = p.ops.copy()
    other = next(j for j, r in enumerate(p.ops) if int(r[0]) == OP_CONV and j + 1 != int(keep[i][44]))
    for src in (other + 1, i + 1, 0, len(p.ops) + 5):  # another conv, itself, none, past the program
        p.ops = keep.copy()
        p.ops[i][44] = src
        with pytest.raises(ProgramError, match="x3"):
            validate_program(p, 2, 16, **CHECK)
    p.ops = keep
    buf = p.buffers[int(keep[i][43])]
    buf.per_item -= 6 * int(keep[i][6])  # one pixel short
    with pytest.raises(ProgramError, match="x3 planes"):
        validate_program(p, 2, 16, **CHECK)
    buf.per_item += 6 * int(keep[i][6])
    validate_program(p, 2, 16, **CHECK)
