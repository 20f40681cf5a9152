"""Tensor source of the fused fp32 detector front end (csrc/kernels/stem_x3.hip, StemFusedParams.src 2): the
request's fp32 NCHW [3, S, S] tensor -> s2d stem conv -> 3x3 stride-2 conv in one kernel.

1. The kernel against float64, every instantiated <TH, NW>, every output element under the project's fp64 conv
   bound (tests/test_fp32_gpu.py ``_fp32_check``: 2e-6 * (sum |x||w| + |b|) per conv) propagated through the first
   SiLU into the second conv.
2. The fp32 ``yolo_raw`` program, fused front end against the unfused three ops, at the tolerance
   tests/test_fp32_gpu.py::test_fp32_stem_s2_fused_matches_unfused uses for the same comparison.
3. The native KServe endpoint (csrc/runtime/http_front.h ``tensor_models``) in front of the GPU tensor programs,
   in-process on an ephemeral port: the session's own bytes sequentially, the program tolerance concurrently.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detect_cases as dc
import fp32_bounds as fb
from inference_arena_amd.models.common import fold
from inference_arena_amd.ops import functional as AF
from inference_arena_amd.ops import native

pytestmark = pytest.mark.gpu

S = 128          # 32 x 32 output: two 16-wide tile columns, 8 (TH 4) or 4 (TH 8) tile rows
CAP, LIVE = 3, 2
SENTINEL = 12288.0
FP32_REL = 2e-6  # the project's fp64 conv bound, relative to sum |x||w| + |b|
SILU_LIP = 1.1   # max |d silu / dx| = 1.0998


def _inputs(name: str) -> torch.Tensor:
    g = torch.Generator().manual_seed(len(name) + 17)
    if name == "uniform":
        return torch.rand(CAP, 3, S, S, generator=g)
    if name == "mixed":
        # +-(1 + k 2^-23) 2^e with k odd and e in [-4, 7]: the significand's last bit is set, so h and m (8 bits
        # each) leave a remainder and the split needs its third plane (unless x - h happens to fit m's 8 bits, one
        # element in a few hundred); both signs, magnitudes up to 2^8
        k = torch.randint(0, 1 << 22, (CAP, 3, S, S), generator=g) * 2 + 1
        e = torch.randint(-4, 8, (CAP, 3, S, S), generator=g)
        sign = torch.randint(0, 2, (CAP, 3, S, S), generator=g) * 2 - 1
        x = (sign * (1.0 + k.double() * 2.0 ** -23) * 2.0 ** e.double()).float()
        h = x.bfloat16().float()
        m = (x - h).bfloat16().float()
        assert ((x - h - m) != 0).float().mean() > 0.99 and x.abs().max() < 256.0
        assert (x < 0).any() and (x > 0).any()
        return x
    # single pixels: corners, edges, and both sides of the tile seams (output column 16 <-> input x 64; output rows
    # 4 k <-> input y 16 k), both s2d phases in y and x, every channel; distinct values so a swapped pixel shows
    x = torch.zeros(CAP, 3, S, S)
    pts = [(0, 0), (0, 127), (127, 0), (127, 127), (0, 63), (0, 64), (63, 0), (64, 0), (127, 65), (62, 127),
           (15, 63), (16, 64), (31, 62), (32, 65), (63, 63), (64, 64), (95, 64), (96, 63), (47, 17), (48, 110)]
    for k, (yy, xx) in enumerate(pts):
        x[k % LIVE, k % 3, yy, xx] = (-1.0) ** k * (1.0 + 0.37 * k)
    x[LIVE:] = 5.0  # the dead image: must not be read into any output
    return x


@pytest.fixture(scope="module")
def front(models):
    """Folded weights of the first two YOLO convs and their packed device forms."""
    from inference_arena_amd.engine.planner import pack_stem_s2_x3
    from inference_arena_amd.engine.plans import s2d_stem_6x6

    y = models[0]
    (w0, b0), (w1, b1) = fold(y.b0), fold(y.b1)
    p0, p1 = pack_stem_s2_x3(s2d_stem_6x6(w0), w1, tensor_src=True)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()  # noqa: E731
    return {"w0": w0.double(), "b0": b0.double(), "w1": w1.double(), "b1": b1.double(),
            "p0": dev(p0), "p1": dev(p1), "bias0": b0.float().cuda(), "bias1": b1.float().cuda()}


@pytest.fixture(scope="module")
def refs(front):
    """Per input set: (x, float64 reference [B, 32, S/4, S/4], per-element bound); computed once, read only."""
    silu = lambda t: t * torch.sigmoid(t)  # noqa: E731
    out = {}
    for name in ("uniform", "mixed", "pixels"):
        x = _inputs(name)
        xd = x.double()
        a = silu(F.conv2d(xd, front["w0"], front["b0"], stride=2, padding=2))
        ref = silu(F.conv2d(a, front["w1"], front["b1"], stride=2, padding=1))
        # stem activation error: the conv bound as the project applies it (to the activated value)
        e_a = FP32_REL * F.conv2d(xd.abs(), front["w0"].abs(), front["b0"].abs(), stride=2, padding=2)
        # second conv: the stem's error carried through |w1| and the closing SiLU, plus the conv's own bound
        bound = SILU_LIP * F.conv2d(e_a, front["w1"].abs(), None, stride=2, padding=1) + \
            FP32_REL * F.conv2d(a.abs(), front["w1"].abs(), front["b1"].abs(), stride=2, padding=1) + 1e-30
        zc = fb.front_case(name, x, front["w0"].float(), front["b0"].float(), front["w1"].float(), front["b1"].float())
        out[name] = (x, ref, bound, zc)
    return out


@pytest.mark.parametrize("th,nw", [("4", "4"), ("4", "2"), ("8", "4")])
@pytest.mark.parametrize("name", ["uniform", "mixed", "pixels"])
def test_tensor_front_end_matches_fp64(device, front, refs, monkeypatch, name, th, nw):
    """Every element of both live images within the propagated fp64 bound, no NaN, the dead image untouched."""
    monkeypatch.setenv("ARENA_STEM_X3_TH", th)
    monkeypatch.setenv("ARENA_STEM_X3_NW", nw)
    x, ref, bound, zc = refs[name]
    meta, pool = dc.tensor_pool(x)
    meta_t = torch.frombuffer(bytearray(meta), dtype=torch.uint8).to(device)
    pool_t = torch.from_numpy(pool.copy()).to(device)
    y = torch.full((CAP, S // 4, S // 4, 32), SENTINEL, device=device)
    ctrl = AF.ctrl_tensor(LIVE, device)
    native().stem_s2_f32({"src": 2, "pool": pool_t.data_ptr(), "meta": meta_t.data_ptr(), "ctrl": ctrl.data_ptr(),
                          "cap": CAP, "S": S, "w": front["p0"].data_ptr(), "bias": front["bias0"].data_ptr(),
                          "w2": front["p1"].data_ptr(), "bias2": front["bias1"].data_ptr(), "y": y.data_ptr(),
                          "ys": 32, "stream": torch.cuda.current_stream().cuda_stream})
    torch.cuda.synchronize()
    got = y.cpu()
    assert (got[LIVE:] == SENTINEL).all()
    g = got[:LIVE].permute(0, 3, 1, 2).double()
    assert torch.isfinite(g).all()
    err = (g - ref[:LIVE]).abs()
    worst = (err / bound[:LIVE]).max().item()
    print(f"{name} <{th},{nw}>: max error {err.max().item():.3e}, {worst:.3f} of the bound")
    assert worst <= 1.0, (name, th, nw, err.max().item(), worst)
    fb.check(zc, g, f"<{th},{nw}>", live=LIVE)


def test_fp32_yolo_raw_fused_front_matches_unfused(models, device, monkeypatch):
    """fp32 ``yolo_raw`` at det_size 64, B = 2, kernel defaults: the fused front end against tensor_in + stem conv
    + s2 conv on the same tensors.  The b1 map at the tolerance of test_fp32_stem_s2_fused_matches_unfused, the raw
    boxes at that test's box tolerance, the scores at test_fp32_gpu's 1e-4."""
    from inference_arena_amd.engine.pipeline import GpuTensorModel
    from inference_arena_amd.engine.planner import OP_STEMFUSED, OP_TENSORIN
    from inference_arena_amd.engine.plans import plan_yolo_raw

    monkeypatch.setenv("ARENA_TUNING", "off")
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).numpy()
    monkeypatch.setenv("ARENA_F32_STEM_S2", "0")
    plain = GpuTensorModel(plan_yolo_raw(models[0], det_size=64, dtype="fp32"), device=0, buckets=[2],
                           share_buffers=False)
    monkeypatch.setenv("ARENA_F32_STEM_S2", "1")
    fused = GpuTensorModel(plan_yolo_raw(models[0], det_size=64, dtype="fp32"), device=0, buckets=[2],
                           share_buffers=False)
    assert int(plain.program.ops[0, 0]) == OP_TENSORIN
    assert int(fused.program.ops[0, 0]) == OP_STEMFUSED and int(fused.program.ops[0, 1]) == 2
    assert not any(int(op[0]) == OP_TENSORIN for op in fused.program.ops)
    a, b = plain.infer(x), fused.infer(x)
    for i in range(2):
        np.testing.assert_allclose(fused.read_buffer("b1", 2, i), plain.read_buffer("b1", 2, i), rtol=1e-5, atol=1e-5)
    assert np.isfinite(b).all()
    np.testing.assert_allclose(b[:, :4], a[:, :4], rtol=2e-5, atol=5e-3)
    np.testing.assert_allclose(b[:, 4:], a[:, 4:], rtol=0, atol=1e-4)


# ------------------------------------------------------------------ the native endpoint in front of the GPU programs
def _endpoint(models, buckets, monkeypatch):
    """yolov5n at det_size 64 and mobilenetv2 at cls_size 32 (the smallest its plan accepts), fp32, kernel
    defaults, each behind its own DynamicBatcher, both on one in-process NativeFrontEnd (ephemeral port)."""
    from types import SimpleNamespace

    from inference_arena_amd.engine.pipeline import GpuTensorModel
    from inference_arena_amd.engine.plans import plan_mobilenet_raw, plan_yolo_raw
    from inference_arena_amd.labels import load_labels
    from inference_arena_amd.server.native_front import NativeFrontEnd

    monkeypatch.setenv("ARENA_TUNING", "off")
    C = native()
    tm = {"yolov5n": GpuTensorModel(plan_yolo_raw(models[0], det_size=64, dtype="fp32"), device=0, buckets=buckets),
          "mobilenetv2": GpuTensorModel(plan_mobilenet_raw(models[1], cls_size=32, dtype="fp32"), device=0,
                                        buckets=buckets)}
    names = {"yolov5n": ("images", "output0"), "mobilenetv2": ("input", "output")}
    bat, entries = {}, []
    for n, m in tm.items():
        bat[n] = C.DynamicBatcher([m.ex], {"max_batch": buckets[-1], "max_queue_delay_us": 2000})
        entries.append({"name": n, "input": names[n][0], "in_dims": list(m.input_shape), "output": names[n][1],
                        "out_dims": list(m.output_shape), "max_batch_size": 8, "batcher": bat[n]})
    fe = NativeFrontEnd(bat["yolov5n"], load_labels(None), port=0, host="127.0.0.1", io_threads=2, decode_procs=1,
                        slots=4, decode_threads=1, jpeg_device=False, tensor_models=entries)

    def close():
        fe.close()
        for b in bat.values():
            b.shutdown()

    return SimpleNamespace(tm=tm, fe=fe, close=close, names=names)


def _post(port, model, in_name, x, conn=None):
    import http.client
    import json

    raw = np.ascontiguousarray(x, np.float32).tobytes()
    hb = json.dumps({"inputs": [{"name": in_name, "shape": list(x.shape), "datatype": "FP32",
                                 "parameters": {"binary_data_size": len(raw)}}]}).encode()
    c = conn or http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    c.request("POST", f"/v2/models/{model}/infer", body=hb + raw,
              headers={"Inference-Header-Content-Length": str(len(hb))})
    r = c.getresponse()
    data = r.read()
    assert r.status == 200, data[:300]
    n = int(r.getheader("Inference-Header-Content-Length"))
    out = json.loads(data[:n])["outputs"][0]
    return np.frombuffer(data[n:], np.float32).reshape(out["shape"])


def _tensors(model, k, seed):
    s = 64 if model == "yolov5n" else 32
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(k, 3, s, s, generator=g) if model == "yolov5n" else torch.randn(k, 3, s, s, generator=g)
    return x.numpy()


@pytest.mark.parametrize("model", ["mobilenetv2", "yolov5n"])
def test_endpoint_answers_are_the_sessions_bytes(models, device, monkeypatch, model):
    """Three distinct tensors, one after the other, buckets [1]: the same program, bucket and deterministic kernels
    as ``infer`` of the same session, so the endpoint's bytes are identical."""
    import http.client

    ep = _endpoint(models, [1], monkeypatch)
    try:
        xs = _tensors(model, 3, 21)
        want = [ep.tm[model].infer(xs[i:i + 1]) for i in range(3)]
        c = http.client.HTTPConnection("127.0.0.1", ep.fe.port, timeout=60)
        for i in range(3):
            got = _post(ep.fe.port, model, ep.names[model][0], xs[i:i + 1], c)
            assert got.shape == want[i].shape and got.tobytes() == want[i].tobytes(), i
        assert _post(ep.fe.port, model, ep.names[model][0], xs[1], c).tobytes() == want[1][0].tobytes()
        assert ep.fe.stats()["tensor_models"][model]["ok"] == 4
    finally:
        ep.close()


@pytest.mark.parametrize("model", ["mobilenetv2", "yolov5n"])
def test_endpoint_concurrent_requests_match_sequential(models, device, monkeypatch, model):
    """Buckets [1, 4], eight concurrent requests: each answer against its own sequential answer.  A request may run
    in the other bucket (other kernels' summation order), so the comparison is the program test's: boxes rtol 2e-5 /
    atol 5e-3, scores atol 1e-4; MobileNet logits rtol 1e-4 / atol 1e-4 max|logit| (a tenth of what
    test_fp32_tensor_models_match_torch allows either program against torch)."""
    import threading

    ep = _endpoint(models, [1, 4], monkeypatch)
    try:
        xs = _tensors(model, 8, 33)
        want = [_post(ep.fe.port, model, ep.names[model][0], xs[i:i + 1]) for i in range(8)]
        got = [None] * 8

        def worker(i):
            got[i] = _post(ep.fe.port, model, ep.names[model][0], xs[i:i + 1])

        ts = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(60)
        for i in range(8):
            assert got[i] is not None and got[i].shape == want[i].shape, i
            if model == "yolov5n":
                np.testing.assert_allclose(got[i][:, :4], want[i][:, :4], rtol=2e-5, atol=5e-3)
                np.testing.assert_allclose(got[i][:, 4:], want[i][:, 4:], rtol=0, atol=1e-4)
            else:
                np.testing.assert_allclose(got[i], want[i], rtol=1e-4, atol=1e-4 * np.abs(want[i]).max())
        assert all(not np.array_equal(want[0], want[i]) for i in range(1, 8))  # distinct requests, distinct answers
    finally:
        ep.close()
