"""Head split (csrc/runtime/head_gate.h head_gate_first_conv, head_marks.h): which first head convs the executor
may split, that the switch changes no program record, and the host definition of a needed tile against a brute-force
dilation."""
from __future__ import annotations

import numpy as np
import pytest

OP_CONV = 1
PARENT_FINGERPRINT = "30fa0d2ef1578e67eae55176"  # pinned by tests/test_ir_s2k16_plan.py
CELL = 8


def _native():
    from inference_arena_amd.ops import native

    return native()


def _pipeline_ops(dtype="fp32"):
    from inference_arena_amd.engine.plans import plan_pipeline
    from inference_arena_amd.models.zoo import default_models

    return plan_pipeline(*default_models(0), conf_thr=0.5, iou_thr=0.45, dtype=dtype).ops


def _check_first_convs(ops):
    C = _native()
    pairs = [tuple(p) for p in C.head_gate_pairs(ops)]
    first = list(C.head_gate_first_convs(ops))
    assert len(pairs) == 2 and len(first) == 2
    for (box, cls, _), f in zip(pairs, first):
        assert f == box - 1
        r, a, c = ops[f], ops[box], ops[cls]
        assert r[0] == OP_CONV and (r[17], r[18], r[19]) == (3, 3, 1) and r[15] == 144 and r[34] == 0
        assert r[22] < 0 and r[25] < 0
        # output range = the box conv's input channels, then the class conv's
        assert (a[1], a[2], a[6]) == (r[10], r[11], 64) and (c[1], c[2], c[6]) == (r[10], r[11] + 64, 80)
        readers = [i for i, o in enumerate(ops) if i not in (f, box, cls) and o[1] == r[10]]
        assert readers == []
    assert [int(ops[f][13]) for f in first] == [80, 40]


def test_first_convs_of_the_default_fp32_pipeline():
    _check_first_convs(_pipeline_ops())


def test_first_convs_of_the_fp32_detector_program():
    from inference_arena_amd.engine.plans import plan_detector
    from inference_arena_amd.models.zoo import default_models

    _check_first_convs(plan_detector(default_models(0)[0], conf_thr=0.5, iou_thr=0.45, dtype="fp32").ops)


def test_no_first_convs_bf16():
    assert list(_native().head_gate_first_convs(_pipeline_ops("bf16"))) == []


def test_no_first_convs_raw_detector():
    from inference_arena_amd.engine.plans import plan_yolo_raw
    from inference_arena_amd.models.zoo import default_models

    assert list(_native().head_gate_first_convs(plan_yolo_raw(default_models(0)[0], dtype="fp32").ops)) == []


def test_no_first_convs_unfused_head(monkeypatch):
    monkeypatch.setenv("ARENA_FUSE_HEAD", "0")
    assert list(_native().head_gate_first_convs(_pipeline_ops())) == []


def test_first_conv_with_another_reader_is_refused():
    """A third reader of F's output buffer (here: a later conv made to read it) leaves the pair without a split."""
    C = _native()
    ops = _pipeline_ops().copy()
    pairs = [tuple(p) for p in C.head_gate_pairs(ops)]
    f0 = C.head_gate_first_convs(ops)[0]
    other = pairs[1][0] + 2  # a conv after both pairs
    assert ops[other][0] == OP_CONV
    ops[other][1] = ops[f0][10]
    first = list(C.head_gate_first_convs(ops))
    assert len(first) == len(C.head_gate_pairs(ops)) and first[0] == -1


@pytest.mark.parametrize("value", ["0", "1", "2", None])
def test_fp32_pipeline_fingerprint_unchanged(value, monkeypatch):
    from inference_arena_amd.engine import tuning

    if value is None:
        monkeypatch.delenv("ARENA_HEAD_SPLIT", raising=False)
    else:
        monkeypatch.setenv("ARENA_HEAD_SPLIT", value)
    monkeypatch.delenv("ARENA_TUNING_FILE", raising=False)  # the shipped table
    ops = _pipeline_ops()
    assert tuning.fingerprint(ops) == PARENT_FINGERPRINT
    e1, e32 = tuning.lookup(ops, 1), tuning.lookup(ops, 32)
    assert e1 is not None and e32 is not None
    monkeypatch.delenv("ARENA_HEAD_SPLIT", raising=False)
    assert np.array_equal(np.asarray(tuning.lookup(ops, 1)), np.asarray(e1))
    assert np.array_equal(np.asarray(tuning.lookup(ops, 32)), np.asarray(e32))


def test_switch_roundtrip():
    C = _native()
    before = C.get_head_split()
    try:
        for v, want in [(0, 0), (1, 1), (2, 2), (7, 2), (-3, 0)]:
            C.set_head_split(v)
            assert C.get_head_split() == want
    finally:
        C.set_head_split(before)
    assert C.MARK_CELL == CELL and C.HEAD_SPLIT_MIN_BUCKET >= 1


def needed_brute_force(marks, H, W, th, tw, uh, uw, halo):
    """Pixel maps: the consumer tiles that hold a marked cell's in-map pixel, dilated by ``halo`` inside the map; a
    producer tile is needed iff it holds a pixel of that set."""
    hot = np.kron(marks != 0, np.ones((CELL, CELL), dtype=bool))[:H, :W]
    cont = np.zeros((H, W), dtype=bool)
    for y0 in range(0, H, uh):
        for x0 in range(0, W, uw):
            if hot[y0:y0 + uh, x0:x0 + uw].any():
                cont[max(0, y0 - halo):y0 + uh + halo, max(0, x0 - halo):x0 + uw + halo] = True
    nty, ntx = -(-H // th), -(-W // tw)
    return np.array([[cont[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].any() for tx in range(ntx)]
                     for ty in range(nty)])


@pytest.mark.parametrize("uh,uw", [(8, 16), (8, 8)])
@pytest.mark.parametrize("H,W", [(20, 24), (21, 35), (80, 80), (8, 16), (5, 3)])
@pytest.mark.parametrize("halo", [0, 1, 3])
def test_needed_against_brute_force(uh, uw, H, W, halo):
    """Random marks of several densities, a single marked cell in every corner, none and all; producer tiles 8 x 16
    and 16 x 16; maps partial on both axes."""
    C = _native()
    ncy, ncx = -(-H // CELL), -(-W // CELL)
    rng = np.random.default_rng(H * 1000 + W * 10 + halo + uw)
    cases = [np.zeros((ncy, ncx), np.int32), np.ones((ncy, ncx), np.int32)]
    for cy, cx in [(0, 0), (0, ncx - 1), (ncy - 1, 0), (ncy - 1, ncx - 1)]:
        m = np.zeros((ncy, ncx), np.int32)
        m[cy, cx] = 1
        cases.append(m)
    for dens in (0.03, 0.2, 0.5):
        for _ in range(4):
            cases.append((rng.random((ncy, ncx)) < dens).astype(np.int32))
    seen = set()
    for m in cases:
        for th, tw in [(8, 16), (16, 16)]:
            got = np.asarray(C.head_marks_needed(m, H, W, th, tw, uh, uw, halo))
            want = needed_brute_force(m, H, W, th, tw, uh, uw, halo)
            assert got.shape == want.shape and got.dtype == np.bool_
            assert np.array_equal(got, want), (m, th, tw)
            seen.update(want.ravel().tolist())
    assert not cases[0].any() and seen == {False, True}


def test_needed_rejects_a_wrong_cell_grid():
    with pytest.raises(RuntimeError):
        _native().head_marks_needed(np.zeros((3, 3), np.int32), 20, 40, 8, 16, 8, 16, 1)


@pytest.mark.parametrize("B", [1, 16, 32])
def test_layout_keeps_the_first_convs_input_clear_of_the_class_logits(B):
    """The box window of a split first conv reads the conv's input after the class conv has written its logits, so
    the arena layout must not place the two in shared memory (the executor checks the same ranges natively)."""
    from inference_arena_amd.engine import planner
    from inference_arena_amd.engine.plans import plan_pipeline
    from inference_arena_amd.models.zoo import default_models

    prog = plan_pipeline(*default_models(0), conf_thr=0.5, iou_thr=0.45, dtype="fp32")
    ops, C = prog.ops, _native()
    offs, _ = planner.layout(prog.buffers, B, 4 * B)
    for (box, cls, _), f in zip(C.head_gate_pairs(ops), C.head_gate_first_convs(ops)):
        xin, det = int(ops[f][1]), int(ops[cls][36])
        a = (int(offs[xin]), int(offs[xin]) + prog.buffers[xin].per_item * B)
        d = (int(offs[det]), int(offs[det]) + prog.buffers[det].per_item * B)
        assert a[1] <= d[0] or d[1] <= a[0], (a, d)
        assert prog.buffers[xin].last >= cls
