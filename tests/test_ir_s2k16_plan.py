"""The K-packed x3 kernel for MobileNetV2 block 2 (csrc/kernels/ir_s2k16_x3.hip) is chosen at launch time in
native code, from the operands the plan already packs: ``ARENA_IR_S2K16`` changes no program record, so the fp32
headline program keeps the fingerprint it had before the kernel existed and still finds its entries in the shipped
tuning table."""
from __future__ import annotations

import pytest

# tuning.fingerprint of plan_pipeline(*default_models(0), conf_thr=0.5, iou_thr=0.45, dtype="fp32") on the commit
# before ARENA_IR_S2K16 was added
PARENT_FINGERPRINT = "30fa0d2ef1578e67eae55176"


@pytest.mark.parametrize("value", ["0", "1", None])
def test_fp32_pipeline_fingerprint_unchanged(value, monkeypatch):
    from inference_arena_amd.engine import tuning
    from inference_arena_amd.engine.plans import plan_pipeline
    from inference_arena_amd.models.zoo import default_models

    if value is None:
        monkeypatch.delenv("ARENA_IR_S2K16", raising=False)
    else:
        monkeypatch.setenv("ARENA_IR_S2K16", value)
    monkeypatch.delenv("ARENA_TUNING_FILE", raising=False)  # the shipped table
    ops = plan_pipeline(*default_models(0), conf_thr=0.5, iou_thr=0.45, dtype="fp32").ops
    assert tuning.fingerprint(ops) == PARENT_FINGERPRINT
    assert tuning.lookup(ops, 1) is not None
    assert tuning.lookup(ops, 32) is not None
