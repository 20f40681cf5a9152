"""x3 planes end to end (``ARENA_X3_PLANES``, csrc/runtime/executor.cpp): the fp32 detector with the switch off and
on, both with the kernel choices of the shipped tuning table, gives bit-identical detections.

Bucket 8: the shipped table selects no x3g -> x3g edge of the detector at buckets 1, 2 and 4 (one to three x3g convs,
none feeding another); 8 is the smallest bucket that has some (seven readers)."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BUCKET = 8


def test_detector_with_planes_is_bit_identical(device, monkeypatch):
    from inference_arena_amd.data.synthetic import synthetic_images
    from inference_arena_amd.engine.pipeline import GpuDetector
    from inference_arena_amd.models.zoo import make_yolo

    for v in ("ARENA_TUNING", "ARENA_TUNING_FILE"):
        monkeypatch.delenv(v, raising=False)
    yolo = make_yolo(0, cls_shift=-20.0)
    imgs = synthetic_images(2, 41)
    runs = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("ARENA_X3_PLANES", switch)
        det = GpuDetector(yolo, device=0, buckets=[BUCKET], dtype="fp32")
        assert det.tuning_source == "table"
        reads, writes = det.ex.planes_ops(BUCKET)
        assert (reads > 0 and writes > 0) if switch == "1" else (reads, writes) == (0, 0)
        runs[switch] = (det.infer(imgs), det.ex.conv_choices(BUCKET))
        del det
    (off, c_off), (on, c_on) = runs["0"], runs["1"]
    assert c_off == c_on and sum(len(r) for r in off) > 0
    for a, b in zip(off, on):
        assert a.det_count == b.det_count
        for f in ("boxes", "scores", "classes"):
            assert np.array_equal(getattr(a, f).view(np.int32), getattr(b, f).view(np.int32)), f
