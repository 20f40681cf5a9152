"""The crop-group switch in the planner (ARENA_IRX_GROUP, csrc/kernels/ir_group_x3.hip), on the CPU."""
import numpy as np

from inference_arena_amd.engine import tuning
from inference_arena_amd.engine.planner import ir_group_planned
from inference_arena_amd.engine.plans import plan_pipeline, plan_split_classifier
from inference_arena_amd.engine.validate import ir_group_x3_supported, validate_program
from inference_arena_amd.models.zoo import default_models

HEADLINE = "30fa0d2e"  # the shipped fp32 pipeline fingerprint's first digits (data/tuning/conv_tuning.json keys)
# (H, stride, inp_pad, hid_pad, oup_pad) of MobileNetV2's 14x14 / 7x7 blocks, features[8..17]
TAIL = [(14, 1, 64, 384, 64)] * 3 + [(14, 1, 64, 384, 96)] + [(14, 1, 96, 576, 96)] * 2 + [(14, 2, 96, 576, 160)] \
    + [(7, 1, 160, 960, 160)] * 2 + [(7, 1, 160, 960, 320)]


def _programs():
    y, m = default_models(0)
    return (plan_pipeline(y, m, conf_thr=0.5, iou_thr=0.45, dtype="fp32"), plan_split_classifier(m, dtype="fp32"))


def test_programs_without_the_switch_are_unchanged(monkeypatch):
    monkeypatch.delenv("ARENA_IRX_GROUP", raising=False)
    unset = _programs()
    monkeypatch.setenv("ARENA_IRX_GROUP", "0")
    for a, b in zip(unset, _programs()):
        assert np.array_equal(np.asarray(a.ops), np.asarray(b.ops))
        assert tuning.fingerprint(a.ops) == tuning.fingerprint(b.ops)
    assert tuning.fingerprint(unset[0].ops).startswith(HEADLINE)


def test_switch_plans_the_three_7x7_blocks_as_group_ops(monkeypatch):
    monkeypatch.delenv("ARENA_IRX_GROUP", raising=False)
    off = _programs()[0]
    monkeypatch.setenv("ARENA_IRX_GROUP", "4")
    on = _programs()[0]
    ir = lambda p: [(int(o[4]), int(o[11]), int(o[26])) for o in p.ops if int(o[0]) == 14]  # noqa: E731
    assert ir(on) == ir(off) + [(7, 1, 4), (7, 1, 4), (7, 1, 2)]
    assert len(on.ops) == len(off.ops) - 6  # nine unfused ops became three
    last = [o for o in on.ops if int(o[0]) == 14][-1]
    assert int(last[28]) == 0  # the block that feeds head_pool writes one plain tensor
    validate_program(on, 8, 32, max_det=300, cand_cap=8400)
    for H, s, inp_pad, hid_pad, oup_pad in TAIL:
        assert bool(ir_group_planned(H, s, inp_pad, hid_pad, oup_pad, 1)) == \
            ir_group_x3_supported(H, s, inp_pad, hid_pad, oup_pad, 1) == (H == 7 and s == 1)
