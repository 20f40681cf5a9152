"""Tensor source of the fused fp32 detector front end, planner side (engine/planner.py ``stem_fused(tensor=True)``,
engine/plans.py ``plan_yolo(tensor_input=True)``, engine/validate.py): which programs take it, what its record and
weight pack hold, what the static check rejects, and that the shipped tuning table covers the new program while
every other program keeps the fingerprint it had."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from inference_arena_amd.engine import tuning
from inference_arena_amd.engine.planner import (BUF_NONE, IMAGES, OP_CONV, OP_STEMFUSED, OP_TENSORIN, ProgramBuilder,
                                                View, pack_stem_s2_x3)
from inference_arena_amd.engine.plans import plan_mobilenet_raw, plan_pipeline, plan_yolo_raw, s2d_stem_6x6
from inference_arena_amd.engine.validate import ProgramError, validate_program
from inference_arena_amd.models.common import fold

# tuning.fingerprint of the programs on the commit before the tensor source existed
PARENT_BF16_YOLO_RAW = "0a1a9dcce951472ff648d8eb"
PARENT_FP32_YOLO_RAW = "37292847c246d4904c35b508"   # tensor_in + stem conv + s2 conv (ARENA_F32_STEM_S2=0 today)
PARENT_FP32_PIPELINE = "30fa0d2ef1578e67eae55176"
PARENT_MOBILENET_RAW = {"bf16": "a238253b28488e6a47d584ec", "fp32": "093af1ecdabd54f1a22d280e"}
BUCKETS = (1, 2, 4, 8, 16, 32)


@pytest.fixture(autouse=True)
def _shipped_table(monkeypatch):
    for v in ("ARENA_TUNING_FILE", "ARENA_F32_STEM_S2", "ARENA_FUSE_STEM", "ARENA_FUSE_STEM2"):
        monkeypatch.delenv(v, raising=False)


def test_fp32_yolo_raw_starts_with_the_fused_tensor_stem(models, monkeypatch):
    p = plan_yolo_raw(models[0], dtype="fp32")
    r = p.ops[0]
    assert int(r[0]) == OP_STEMFUSED
    # src 2, S 640, 3x3 16 -> 16 stem (Kpad 160) over images, second conv 16 -> 32 with Kpad 160, no crops
    assert (int(r[1]), int(r[5]), int(r[7]), int(r[9]), int(r[18]), int(r[19])) == (2, 640, 160, 16, IMAGES, 3)
    assert (int(r[11]), int(r[20]), int(r[22]), int(r[24]), int(r[26])) == (BUF_NONE, 1, 160, 32, 0)
    kinds = [int(o[0]) for o in p.ops]
    assert kinds.count(OP_STEMFUSED) == 1 and OP_TENSORIN not in kinds
    # the parent's first three ops (tensor_in, stem conv, s2 conv) became one; the rest is the same list
    old = _unfused(models, monkeypatch)
    assert len(p.ops) == len(old.ops) - 2
    assert [int(o[0]) for o in old.ops[3:]] == kinds[1:]
    for B in (1, 3, 32):
        validate_program(p, B, 16, max_det=300, cand_cap=8400, pool_bytes_per_image=3 * 640 * 640 * 4)


def _unfused(models, monkeypatch):
    monkeypatch.setenv("ARENA_F32_STEM_S2", "0")
    p = plan_yolo_raw(models[0], dtype="fp32")
    monkeypatch.delenv("ARENA_F32_STEM_S2")
    return p


def test_switch_keeps_the_parent_program(models, monkeypatch):
    """ARENA_F32_STEM_S2=0: the parent's fp32 tensor program, record for record (its table entries stay)."""
    old = _unfused(models, monkeypatch)
    assert tuning.fingerprint(old.ops) == PARENT_FP32_YOLO_RAW
    assert [int(o[0]) for o in old.ops[:3]] == [OP_TENSORIN, OP_CONV, OP_CONV]
    assert all(tuning.lookup(old.ops, B) is not None for B in BUCKETS)


def test_other_programs_are_unchanged(models):
    y, m = models
    bf = plan_yolo_raw(y, dtype="bf16")
    assert tuning.fingerprint(bf.ops) == PARENT_BF16_YOLO_RAW  # op for op: the fingerprint hashes every record
    assert int(bf.ops[0][0]) == OP_TENSORIN
    for dt, fp in PARENT_MOBILENET_RAW.items():
        assert tuning.fingerprint(plan_mobilenet_raw(m, dtype=dt).ops) == fp
    pipe = plan_pipeline(y, m, conf_thr=0.5, iou_thr=0.45, dtype="fp32")
    assert tuning.fingerprint(pipe.ops) == PARENT_FP32_PIPELINE
    assert int(pipe.ops[[int(o[0]) for o in pipe.ops].index(OP_STEMFUSED)][1]) == 0  # still the letterbox source


def test_shipped_table_has_the_new_program(models):
    ops = plan_yolo_raw(models[0], dtype="fp32").ops
    assert tuning.fingerprint(ops) != PARENT_FP32_YOLO_RAW
    table = tuning.load_table()
    for B in BUCKETS:
        e = tuning.lookup(ops, B)
        assert e is not None and len(e) == len(ops), B
        assert f"{PARENT_FP32_YOLO_RAW}:{B}" in table  # the old keys stay


def test_small_det_sizes_follow_the_letterbox_rule(models):
    """Fused when T % 64 == 0 (as the letterbox form), the unfused three ops otherwise."""
    assert int(plan_yolo_raw(models[0], det_size=64, dtype="fp32").ops[0][0]) == OP_STEMFUSED
    assert int(plan_yolo_raw(models[0], det_size=96, dtype="fp32").ops[0][0]) == OP_TENSORIN


def test_tensor_pack_carries_no_255(models):
    """Stem planes [3 ky][2 slabs][16][h|m|l][32]: h + m + l is the fp32 weight itself for the tensor source and
    the weight / 255 for the letterbox source; the s2 conv's pack is the same for both."""
    w0 = s2d_stem_6x6(fold(models[0].b0)[0])
    w1 = fold(models[0].b1)[0]
    (t0, t1), (l0, l1) = pack_stem_s2_x3(w0, w1, tensor_src=True), pack_stem_s2_x3(w0, w1)
    assert t1 == l1 and len(t0) == len(l0) == 3 * 2 * 16 * 3 * 32 * 2

    def planes(b):
        p = torch.frombuffer(bytearray(b), dtype=torch.bfloat16).reshape(3, 2, 16, 3, 32).double().sum(3)
        return p.permute(2, 0, 1, 3).reshape(16, 3, 64)[:, :, :48]  # [n][ky][kx * 16 + c]

    want = w0.double().permute(0, 2, 3, 1).reshape(16, 3, 48)
    assert (planes(t0) - want).abs().max() <= 2.0 ** -23 * want.abs().max()
    assert (planes(l0) - (w0 / 255.0).double().permute(0, 2, 3, 1).reshape(16, 3, 48)).abs().max() <= \
        2.0 ** -23 * want.abs().max() / 255.0


def _tiny_tensor_program(S: int = 64):
    pb = ProgramBuilder("fp32")
    A1 = pb.tensor("b1", S // 4, S // 4, 32)
    pb.stem_fused(View(A1, 0, 32), torch.randn(16, 16, 3, 3), torch.zeros(16), S=S, act="silu",
                  second=(torch.randn(32, 16, 3, 3), torch.zeros(32), "silu"), tensor=True)
    return pb.build()


def test_validate_checks_the_pool(models):
    p = _tiny_tensor_program(64)
    need = 3 * 64 * 64 * 4
    validate_program(p, 2, 16, max_det=300, cand_cap=8400, pool_bytes_per_image=need)
    validate_program(p, 2, 16, max_det=300, cand_cap=8400)  # pool size unknown: not checked
    with pytest.raises(ProgramError, match="pool bytes"):
        validate_program(p, 2, 16, max_det=300, cand_cap=8400, pool_bytes_per_image=need - 4)
    with pytest.raises(ProgramError, match="pool bytes"):  # the letterbox pipelines' uint8 pool
        validate_program(p, 2, 16, max_det=300, cand_cap=8400, pool_bytes_per_image=640 * 640 * 3 // 100)


def test_validate_rejects_a_bf16_tensor_stem():
    p = _tiny_tensor_program(64)
    p.ops[0, 47] = 0  # the op's dtype field: bf16
    with pytest.raises(ProgramError):
        validate_program(p, 1, 16, max_det=300, cand_cap=8400)
    with pytest.raises(ValueError, match="tensor source"):
        pb = ProgramBuilder("bf16")
        A1 = pb.tensor("b1", 16, 16, 32)
        pb.stem_fused(View(A1, 0, 32), torch.randn(16, 16, 3, 3), torch.zeros(16), S=64, act="silu",
                      second=(torch.randn(32, 16, 3, 3), torch.zeros(32), "silu"), tensor=True)


def test_validate_rejects_a_tensor_stem_without_second_conv_or_odd_size():
    p = _tiny_tensor_program(64)
    q = p.ops.copy()
    p.ops[0, 5] = 96  # S % 64 != 0
    with pytest.raises(ProgramError):
        validate_program(p, 1, 16, max_det=300, cand_cap=8400)
    p.ops[:] = q
    p.ops[0, 20] = 0
    with pytest.raises(ProgramError):
        validate_program(p, 1, 16, max_det=300, cand_cap=8400)
    assert np.array_equal(q[0, :2], [OP_STEMFUSED, 2])
