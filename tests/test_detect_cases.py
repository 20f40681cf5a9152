"""The crafted inputs of the detector-tail GPU tests (detect_cases.py) have the properties that let those tests
demand equality: the margin filter removes little, and the fp32 host NMS keeps what an fp64 one keeps."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import detect_cases as dc
from inference_arena_amd.ops import functional as AF


@pytest.mark.parametrize("name", sorted(dc.NMS_LAUNCHES))
def test_nms_cases_are_rounding_proof(name):
    for (n, _), case in zip(dc.NMS_LAUNCHES[name], dc.nms_launch(name)):
        assert len(case["boxes"]) == n and np.all(np.diff(case["anchors"]) > 0)
        assert case["filtered"] <= 0.02, (n, case["filtered"])
        assert dc.margin_keep(case["boxes"], case["cls"]).all()
        k32, k64 = dc.nms_keep(case), dc.nms_keep_f64(case)
        assert np.array_equal(k32, k64), (n, len(k32), len(k64))
        # coordinates on the 4-px grid survive the cxcywh round trip of the oracle exactly
        c = dc.to_cxcywh(case["boxes"])
        assert np.array_equal(dc.raw_to_xyxy(c), case["boxes"])


def test_nms_variants_keep_and_suppress():
    """The sparse draw keeps most candidates, the dense one suppresses most: both branches of the sweep run."""
    sparse, dense = dc.nms_launch("counts")[-1], dc.nms_launch("dense")[-1]
    assert len(dc.nms_keep(sparse)) > 0.8 * 8400
    assert len(dc.nms_keep(dense)) < 0.5 * 8400


def test_pack_candidates_round_trip():
    case = dc.nms_launch("counts")[4]
    rec = dc.pack_candidates(case, 1100, 3)
    live = rec[:1023]
    assert (rec[1023:] == dc.SENTINEL).all()
    order = np.argsort(live[:, 6])
    assert np.array_equal(live[order, 6], case["anchors"]) and not np.array_equal(live[:, 6], case["anchors"])
    assert np.array_equal(live[order, :4].view(np.float32), case["boxes"])
    assert np.array_equal(live[order, 4].view(np.float32), case["scores"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_decode_inputs_hold_the_stated_cases(dtype):
    x, passing, exact = dc.decode_inputs(dtype)
    assert torch.equal(x, x.to(dtype).double())
    raw = dc.decode_oracle(x)
    best = raw[:, 4:].max(1)
    assert (np.abs(best - dc.CONF_THR) > 0.05).all()
    for b, n_pass in enumerate(dc.N_PASS):
        assert np.array_equal(np.nonzero(best[b] >= dc.CONF_THR)[0], passing[b]) and len(passing[b]) == n_pass
    logits = x[:, 64:].numpy()
    ties = [(b, a) for b in range(3) for a in passing[b] if (logits[b, :, a] == logits[b, :, a].max()).sum() == 2]
    assert len(ties) >= 4
    assert (best.astype(np.float32) == 1.0).any() and (logits.max(1) == -0.25).any()
    # the one-hot side decodes to its bin, the flat side to 7.5
    s, ax = dc.STRIDES[0], exact % dc.HW[0] + 0.5
    x1, x2 = dc.raw_to_xyxy(raw)[0, [0, 2], exact]
    assert abs(x1 - (ax - dc.ONE_HOT_BIN) * s) < 1e-9 and abs(x2 - (ax + 7.5) * s) < 1e-9
    d_score, d_px = dc.decode_tolerances(x)
    assert 0 < d_score < 1e-6 and 0 < d_px < 1e-3


def test_s2d_helper_inverts_s2d_to_nchw():
    x = torch.randn(2, 3, 8, 6)
    y = dc.nchw_to_s2d(x)
    assert y.shape == (2, 4, 3, 16) and (y[..., 12:] == 0).all()
    assert torch.equal(AF.s2d_to_nchw(y), x)
