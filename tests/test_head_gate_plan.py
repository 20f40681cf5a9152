"""Detect-head tile gate (csrc/runtime/head_gate.h): which ops the executor pairs, that the switch changes no
program record, and that the gate's logit threshold keeps every logit the decode's sigmoid test accepts."""
from __future__ import annotations

import numpy as np
import pytest

OP_CONV, OP_DECODE, DTYPE_FIELD = 1, 6, 47
# tuning.fingerprint of plan_pipeline(*default_models(0), conf_thr=0.5, iou_thr=0.45, dtype="fp32"), pinned by
# tests/test_ir_s2k16_plan.py
PARENT_FINGERPRINT = "30fa0d2ef1578e67eae55176"


def _native():
    from inference_arena_amd.ops import native

    return native()


def _expected_pairs(ops: np.ndarray) -> list[tuple[int, int, int]]:
    """The pairs read off the records: per DECODE level, the conv whose fused 1x1 writes the level's 64 box channels
    and the conv right after it that writes the 80 class channels."""
    dec = [r for r in ops if r[0] == OP_DECODE]
    assert len(dec) == 1
    dec = dec[0]
    out = []
    for lvl in range(3):
        buf, coff = int(dec[1 + 4 * lvl]), int(dec[2 + 4 * lvl])
        box = [i for i, r in enumerate(ops) if r[0] == OP_CONV and r[34] == 64 and r[36] == buf and r[37] == coff]
        for i in box:
            nxt = ops[i + 1]
            writes_cls = (nxt[34] == 80 and nxt[36] == buf and nxt[37] == coff + 64) or \
                (nxt[34] == 0 and nxt[15] == 80 and nxt[10] == buf and nxt[11] == coff + 64)
            if nxt[0] == OP_CONV and writes_cls:
                out.append((i, i + 1, lvl))
    return out


def _pipeline_ops(dtype="fp32"):
    from inference_arena_amd.engine.plans import plan_pipeline
    from inference_arena_amd.models.zoo import default_models

    return plan_pipeline(*default_models(0), conf_thr=0.5, iou_thr=0.45, dtype=dtype).ops


def test_pairs_of_the_default_fp32_pipeline():
    ops = _pipeline_ops()
    pairs = [tuple(p) for p in _native().head_gate_pairs(ops)]
    exp = _expected_pairs(ops)
    assert pairs == exp and len(pairs) == 2
    assert [int(ops[b][13]) for b, _, _ in pairs] == [80, 40]  # 80x80 and 40x40; the 20x20 head is not fused
    assert [lvl for _, _, lvl in pairs] == [0, 1]
    for box, cls, _ in pairs:
        assert cls == box + 1 and ops[box][DTYPE_FIELD] == 1 and ops[cls][DTYPE_FIELD] == 1
        # the two read disjoint channel ranges of the same buffer
        assert ops[box][1] == ops[cls][1] and ops[box][2] + ops[box][6] <= ops[cls][2]


def test_pairs_of_the_fp32_detector_program():
    from inference_arena_amd.engine.plans import plan_detector
    from inference_arena_amd.models.zoo import default_models

    ops = plan_detector(default_models(0)[0], conf_thr=0.5, iou_thr=0.45, dtype="fp32").ops
    pairs = [tuple(p) for p in _native().head_gate_pairs(ops)]
    assert pairs == _expected_pairs(ops) and [int(ops[b][13]) for b, _, _ in pairs] == [80, 40]


def test_no_pairs_bf16():
    assert _native().head_gate_pairs(_pipeline_ops("bf16")) == []


def test_no_pairs_raw_detector():
    from inference_arena_amd.engine.plans import plan_yolo_raw
    from inference_arena_amd.models.zoo import default_models

    assert _native().head_gate_pairs(plan_yolo_raw(default_models(0)[0], dtype="fp32").ops) == []


def test_no_pairs_unfused_head(monkeypatch):
    monkeypatch.setenv("ARENA_FUSE_HEAD", "0")
    ops = _pipeline_ops()
    assert not any(r[0] == OP_CONV and r[34] > 0 for r in ops)
    assert _native().head_gate_pairs(ops) == []


@pytest.mark.parametrize("value", ["0", "1", None])
def test_fp32_pipeline_fingerprint_unchanged(value, monkeypatch):
    from inference_arena_amd.engine import tuning

    if value is None:
        monkeypatch.delenv("ARENA_HEAD_GATE", raising=False)
    else:
        monkeypatch.setenv("ARENA_HEAD_GATE", value)
    monkeypatch.delenv("ARENA_TUNING_FILE", raising=False)  # the shipped table
    ops = _pipeline_ops()
    assert tuning.fingerprint(ops) == PARENT_FINGERPRINT
    assert tuning.lookup(ops, 1) is not None
    assert tuning.lookup(ops, 32) is not None


def _sweep(center: np.float32, steps: int = 64) -> np.ndarray:
    """float32 neighbours of ``center``: ``steps`` nextafter steps to either side, and the value itself."""
    up, dn = [center], []
    v = center
    for _ in range(steps):
        v = np.nextafter(v, np.float32(np.inf))
        up.append(v)
    v = center
    for _ in range(steps):
        v = np.nextafter(v, np.float32(-np.inf))
        dn.append(v)
    return np.asarray(dn[::-1] + up, dtype=np.float32)


@pytest.mark.parametrize("thr", [1e-3, 0.25, 0.5, 0.9, 0.999])
def test_gate_threshold_keeps_what_decode_accepts(thr):
    t = np.float32(thr)
    gm = _native().head_gate_min(float(t))
    assert gm is not None
    gm32 = np.float32(gm)
    assert float(gm32) == gm  # a float32 value
    logit = np.log(np.float64(t) / (1.0 - np.float64(t)))
    # one definition: logit(thr) - 1/64 in double precision, rounded to float32 downwards
    assert logit - 1.0 / 64 - 1e-6 < gm <= logit - 1.0 / 64
    v = np.concatenate([_sweep(gm32), _sweep(np.float32(logit)), _sweep(np.float32(logit - 1.0 / 128))])
    sig = np.float32(1.0) / (np.float32(1.0) + np.exp(-v, dtype=np.float32))
    assert sig.dtype == np.float32
    accepted = sig >= t
    assert accepted.any() and (~accepted).any()
    assert np.all(v[accepted] >= gm32)
    # the margin is real: everything below gate_min is at least 1e-5 short of the threshold
    assert np.all(sig[v < gm32].astype(np.float64) <= np.float64(t) - 1e-5)


@pytest.mark.parametrize("thr", [0.0, 5e-4, 0.9995, 1.0, 1.5, -0.1, float("nan")])
def test_gate_off_outside_the_range(thr):
    assert _native().head_gate_min(thr) is None
