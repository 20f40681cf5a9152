"""Tensor models on the native KServe-v2 endpoint (csrc/runtime/kserve.h, http_front.h ``tensor_models``), on CPU:
the host-only EchoInstance behind real sockets.  With ``raw_out_bytes`` the echo answers output float j of an item
with ``in[(7 j) mod n_in] + (j mod 13)``, so every response can be matched to its own request."""
from __future__ import annotations

import http.client
import json
import re
import socket
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from inference_arena_amd.labels import load_labels
from inference_arena_amd.ops import native
from inference_arena_amd.repository import model_config as mc
from inference_arena_amd.server.model_server import native_tensor_entry, render_metrics, start_native_kserve
from inference_arena_amd.server.modelserver_core import ModelHandle, ModelStats
from inference_arena_amd.server.native_front import NativeFrontEnd

N_OUT = 21
CONFIG = """
name: "{name}"
platform: "arena_hip"
max_batch_size: {mb}
input [{{ name: "images"  data_type: TYPE_FP32  dims: [ {dims} ] }}]
output [{{ name: "output0"  data_type: TYPE_FP32  dims: [ {odims} ] }}]
instance_group [{{ count: 1  kind: KIND_CPU }}]
"""


class EchoTensorModel(ModelHandle):
    """A model-server handle (config.pbtxt contract, ModelStats) whose native batcher runs an EchoInstance."""

    def __init__(self, name="tiny", side=8, max_batch=8, latency_us=0, mb_cfg=None, **bcfg):
        mb_cfg = max_batch if mb_cfg is None else mb_cfg
        dims = f"3, {side}, {side}" if mb_cfg > 0 else f"1, 3, {side}, {side}"
        cfg = mc.parse(CONFIG.format(name=name, mb=mb_cfg, dims=dims, odims=N_OUT if mb_cfg > 0 else f"1, {N_OUT}"))
        super().__init__(SimpleNamespace(name=name, config=cfg, versions=[1]))
        self.in_name, self.out_name = "images", "output0"
        C = native()
        b = C.DynamicBatcher([C.EchoInstance(2, max_batch, 4, latency_us, 0, N_OUT * 4)],
                             {"max_batch": max_batch, "max_queue_delay_us": 2000, **bcfg})
        self.batcher = SimpleNamespace(_b=b, stats=b.stats)


def echo(x: np.ndarray) -> np.ndarray:
    f = np.asarray(x, np.float32).ravel()
    j = np.arange(N_OUT)
    return (f[(7 * j) % f.size] + (j % 13).astype(np.float32)).astype(np.float32)


def request(x: np.ndarray, name="images", datatype="FP32", shape=None, size=None, outputs=None, rid="r-1",
            extra_inputs=()) -> tuple[bytes, int]:
    raw = np.ascontiguousarray(x, np.float32).tobytes()
    hdr = {"id": rid, "inputs": [{"name": name, "shape": list(x.shape) if shape is None else shape,
                                  "datatype": datatype,
                                  "parameters": {"binary_data_size": len(raw) if size is None else size}},
                                 *extra_inputs]}
    if outputs is not None:
        hdr["outputs"] = outputs
    hb = json.dumps(hdr).encode()
    return hb + raw, len(hb)


def post(conn, model, body, ihcl, version=False):
    path = f"/v2/models/{model}" + ("/versions/1" if version else "") + "/infer"
    headers = {"Content-Type": "application/octet-stream"}
    if ihcl is not None:
        headers["Inference-Header-Content-Length"] = str(ihcl)
    conn.request("POST", path, body=body, headers=headers)
    r = conn.getresponse()
    data = r.read()
    if r.status != 200:
        return r.status, json.loads(data), None
    n = int(r.getheader("Inference-Header-Content-Length"))
    hdr = json.loads(data[:n])
    out = hdr["outputs"][0]
    assert out["parameters"]["binary_data_size"] == len(data) - n
    return 200, hdr, np.frombuffer(data[n:], np.float32).reshape(out["shape"])


class Front:
    def __init__(self, *models, **kw):
        C = native()
        self.models = list(models)
        self.ens = C.DynamicBatcher([C.EchoInstance(2, 8, 4, 200)], {"max_batch": 8, "max_queue_delay_us": 200})
        self.fe = NativeFrontEnd(self.ens, load_labels(None), port=0, host="127.0.0.1", io_threads=2, decode_procs=1,
                                 slots=16, decode_threads=2, jpeg_device=False, kserve_model="arena_pipeline",
                                 tensor_models=[native_tensor_entry(m) for m in self.models], **kw)

    def conn(self):
        return http.client.HTTPConnection("127.0.0.1", self.fe.port, timeout=30)

    def close(self):
        self.fe.close()
        for m in self.models:
            m.batcher._b.shutdown()
        self.ens.shutdown()


@pytest.fixture(scope="module")
def front():
    f = Front(EchoTensorModel())
    yield f
    f.close()


@pytest.fixture(scope="module")
def spec():
    """One handle and its contract dict for the tests that need no sockets."""
    h = EchoTensorModel()
    yield h, {k: v for k, v in native_tensor_entry(h).items() if k != "batcher"}
    h.batcher._b.shutdown()


# ------------------------------------------------------------------ parser, through the binding
def test_parser_cases(spec):
    C = native()
    model = spec[1]
    x = np.arange(3 * 8 * 8, dtype=np.float32).reshape(1, 3, 8, 8)
    body, n = request(x)
    got = C.kserve_parse_tensor_input(body, n, model)
    assert got == {"id": "r-1", "off": n, "n": 1, "item_bytes": 768, "batch_dim": True}
    body3, n3 = request(np.zeros((3, 3, 8, 8), np.float32), outputs=[{"name": "output0"}])
    assert C.kserve_parse_tensor_input(body3, n3, model)["n"] == 3
    assert C.kserve_parse_tensor_input(*request(x[0]), model)["batch_dim"] is False
    more = {"name": "more", "shape": [1, 3, 8, 8], "datatype": "FP32", "parameters": {"binary_data_size": 768}}
    bad = {
        "wrong datatype": request(x, datatype="FP16"),
        "rank 2": request(x.reshape(24, 8)),
        "channels not 3": request(np.zeros((1, 4, 8, 8), np.float32)),
        "size != product * 4": request(x, size=764),
        "size past the body": request(x, shape=[2, 3, 8, 8], size=1536),
        "header length past the body": (body, len(body) + 1),
        "two inputs": request(x, extra_inputs=[more]),
        "unknown input name": request(x, name="input"),
        "N above max_batch_size": request(np.zeros((9, 3, 8, 8), np.float32)),
        "unknown output name": request(x, outputs=[{"name": "output1"}]),
    }
    for what, (b, h) in bad.items():
        with pytest.raises(ValueError):
            C.kserve_parse_tensor_input(b, h, model)
            pytest.fail(f"{what}: accepted")
    with pytest.raises(ValueError, match="binary tensor data extension"):
        C.kserve_parse_tensor_input(body, -1, model)
    # max_batch_size 0: the dims carry the batch dimension, N must be 1
    m0 = dict(model, max_batch_size=0, in_dims=[1, 3, 8, 8], out_dims=[1, N_OUT])
    assert C.kserve_parse_tensor_input(body, n, m0)["n"] == 1
    with pytest.raises(ValueError, match="max_batch_size"):
        C.kserve_parse_tensor_input(*request(np.zeros((2, 3, 8, 8), np.float32)), m0)


def test_response_builder_and_metadata(spec):
    C = native()
    h, model = spec
    items = [np.full(N_OUT, k, np.float32).tobytes() for k in range(3)]
    body, n = C.kserve_build_tensor_response(model, "abc", True, items)
    hdr = json.loads(body[:n])
    assert hdr == {"model_name": "tiny", "model_version": "1", "id": "abc",
                   "outputs": [{"name": "output0", "datatype": "FP32", "shape": [3, N_OUT],
                                "parameters": {"binary_data_size": 3 * N_OUT * 4}}]}
    assert body[n:] == b"".join(items)
    body, n = C.kserve_build_tensor_response(model, "", False, items[:1])
    assert json.loads(body[:n])["outputs"][0]["shape"] == [N_OUT]
    with pytest.raises(ValueError):
        C.kserve_build_tensor_response(model, "", True, [b"\0" * 80])
    assert json.loads(C.kserve_tensor_model_metadata(model)) == h.metadata()
    h0 = EchoTensorModel(name="ref", mb_cfg=0, max_batch=1)
    m0 = {k: v for k, v in native_tensor_entry(h0).items() if k != "batcher"}
    assert json.loads(C.kserve_tensor_model_metadata(m0)) == h0.metadata()
    assert h0.metadata()["inputs"][0]["shape"] == [1, 3, 8, 8]
    h0.batcher._b.shutdown()


# ------------------------------------------------------------------ sockets
def test_round_trip(front, rng):
    c = front.conn()
    x = rng.standard_normal((1, 3, 8, 8)).astype(np.float32)
    code, hdr, y = post(c, "tiny", *request(x, rid="first"))
    assert code == 200 and hdr["model_name"] == "tiny" and hdr["model_version"] == "1" and hdr["id"] == "first"
    assert hdr["outputs"][0]["name"] == "output0" and hdr["outputs"][0]["datatype"] == "FP32"
    assert y.shape == (1, N_OUT) and np.array_equal(y[0], echo(x[0]))
    code, _, y = post(c, "tiny", *request(x[0]), version=True)   # no batch dimension: the item shape comes back
    assert code == 200 and y.shape == (N_OUT,) and np.array_equal(y, echo(x[0]))
    x3 = rng.standard_normal((3, 3, 8, 8)).astype(np.float32)
    code, _, y = post(c, "tiny", *request(x3))
    assert code == 200 and y.shape == (3, N_OUT)
    for i in range(3):
        assert np.array_equal(y[i], echo(x3[i])), i
    st = front.fe.stats()["tensor_models"]["tiny"]
    assert st["ok"] >= 3 and st["items"] >= 5 and st["failed"] == 0


def test_concurrent_requests_match_and_batch():
    """64 distinct tensors over 8 keep-alive connections against a 2 ms instance with max_batch 8: every answer is
    its own request's, and the batcher merged them (mean batch >= 2: a condition, not a rate)."""
    f = Front(EchoTensorModel(latency_us=2000))
    try:
        rng = np.random.default_rng(7)
        xs = rng.standard_normal((64, 3, 8, 8)).astype(np.float32)
        bad = []

        def worker(k):
            c = f.conn()
            for i in range(k, 64, 8):
                code, hdr, y = post(c, "tiny", *request(xs[i:i + 1], rid=f"q{i}"))
                if code != 200 or hdr["id"] != f"q{i}" or not np.array_equal(y[0], echo(xs[i])):
                    bad.append(i)

        ts = [threading.Thread(target=worker, args=(k,)) for k in range(8)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(60)
        assert not bad, bad
        st = f.models[0].batcher.stats()
        assert st["requests"] == 64 and st["mean_batch"] >= 2.0, st
        assert f.fe.stats()["tensor_models"]["tiny"]["ok"] == 64
    finally:
        f.close()


def test_coexistence_and_errors(front, rng):
    from inference_arena_amd.data.synthetic import encode_jpeg

    c = front.conn()
    # the ensemble still answers on the same port
    up = encode_jpeg((rng.random((48, 64, 3)) * 255).astype(np.uint8))
    eh = json.dumps({"inputs": [{"name": "IMAGE_BYTES", "shape": [1], "datatype": "BYTES",
                                 "parameters": {"binary_data_size": len(up) + 4}}]}).encode()
    c.request("POST", "/v2/models/arena_pipeline/infer", body=eh + len(up).to_bytes(4, "little") + up,
              headers={"Inference-Header-Content-Length": str(len(eh))})
    r = c.getresponse()
    data = r.read()
    assert r.status == 200, data[:200]
    n = int(r.getheader("Inference-Header-Content-Length"))
    assert [o["name"] for o in json.loads(data[:n])["outputs"]][0] == "DETECTIONS"
    # metadata and ready routes of the tensor model
    for path in ("/v2/models/tiny", "/v2/models/tiny/versions/1"):
        c.request("GET", path)
        r = c.getresponse()
        assert r.status == 200 and json.loads(r.read()) == front.models[0].metadata()
    for path, want in (("/v2/models/tiny/ready", 200), ("/v2/models/tiny/versions/1/ready", 200),
                       ("/v2/models/tinyx/ready", 404), ("/v2/models/tiny/versions/2/ready", 404)):
        c.request("GET", path)
        r = c.getresponse()
        r.read()
        assert r.status == want, path
    x = rng.standard_normal((1, 3, 8, 8)).astype(np.float32)
    code, err, _ = post(c, "nope", *request(x))
    assert code == 404 and "error" in err
    js = json.dumps({"inputs": [{"name": "images", "shape": [1, 3, 8, 8], "datatype": "FP32",
                                 "data": x.ravel().tolist()}]}).encode()
    for ihcl in (None, len(js)):
        code, err, _ = post(c, "tiny", js, ihcl)
        assert code == 400 and "binary tensor data extension" in err["error"], err
    code, err, _ = post(c, "tiny", *request(x, datatype="INT8"))
    assert code == 400 and "FP32" in err["error"]
    front.fe.set_healthy(False)
    try:
        code, err, _ = post(c, "tiny", *request(x))
        assert code == 503
    finally:
        front.fe.set_healthy(True)
    code, _, y = post(c, "tiny", *request(x))   # the connection survived every error
    assert code == 200 and np.array_equal(y[0], echo(x[0]))


def test_full_queue_is_503():
    """One request of 8 items against a queue of 2 that holds its batch for 20 ms: the third item finds the queue
    full, the request is answered 503 once the two queued items are back, and the next request is served."""
    f = Front(EchoTensorModel(max_queue_size=2, max_queue_delay_us=20000, idle_queue_delay_us=20000))
    try:
        c = f.conn()
        x = np.random.default_rng(3).standard_normal((8, 3, 8, 8)).astype(np.float32)
        code, err, _ = post(c, "tiny", *request(x))
        assert code == 503 and "queue" in err["error"]
        st = f.fe.stats()
        assert st["tensor_models"]["tiny"]["failed"] == 1 and st["unavailable"] == 1
        code, _, y = post(c, "tiny", *request(x[:2]))
        assert code == 200 and np.array_equal(y[1], echo(x[1]))
    finally:
        f.close()


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_native_requests_count_in_model_metrics(rng):
    """start_native_kserve registers the tensor models of a server next to the ensemble and folds the front end's
    per-model counters into ModelStats: render_metrics and the statistics routes count native requests."""
    C = native()
    eb = C.DynamicBatcher([C.EchoInstance(2, 8, 4, 200)], {"max_batch": 8, "max_queue_delay_us": 200})
    ens = SimpleNamespace(backend=SimpleNamespace(batcher=SimpleNamespace(_b=eb, stats=eb.stats)),
                          stats=ModelStats(), version="1")
    tiny = EchoTensorModel()
    server = SimpleNamespace(device="fake", models={"arena_pipeline": ens, "tiny": tiny})

    def success():
        m = re.search(r'nv_inference_request_success(?:_total)?\{model="tiny",version="1"\} (\S+)',
                      render_metrics(server).decode())
        return float(m.group(1))

    fe = start_native_kserve(server, "127.0.0.1", _free_port())
    try:
        assert fe is not None
        before, count0 = success(), tiny.stats.inference_count
        c = http.client.HTTPConnection("127.0.0.1", fe.port, timeout=30)
        k = 5
        for i in range(k):
            code, _, _ = post(c, "tiny", *request(rng.standard_normal((2, 3, 8, 8)).astype(np.float32)))
            assert code == 200
        code, _, _ = post(c, "tiny", *request(np.zeros((1, 3, 8, 8), np.float32), datatype="FP16"))
        assert code == 400
        assert success() == before + k
        st = tiny.stats
        assert st.inference_count == count0 + 2 * k and st.execution_count == k and st.failure == 1
        assert st.request_us > 0 and st.last_inference_ms > 0
        assert success() == before + k   # reading twice folds nothing twice
    finally:
        fe.close()
        tiny.batcher._b.shutdown()
        eb.shutdown()


def test_body_pool_stays_within_its_budget():
    """Eight 4.9 MB tensor bodies in flight at once against a pool budget of 3 bodies (2 I/O threads + depth 1), then
    small requests: the pool retains no more than its budget and frees what came back beyond it."""
    big = EchoTensorModel(name="big", side=640, latency_us=20000)
    f = Front(EchoTensorModel(), big, body_pool_depth=1)
    try:
        x = np.zeros((1, 3, 640, 640), np.float32)
        x[0, 0, 0, :8] = np.arange(8)
        body, n = request(x)
        bad = []

        def worker():
            code, _, y = post(f.conn(), "big", body, n)
            if code != 200 or not np.array_equal(y[0], echo(x[0])):
                bad.append(code)

        ts = [threading.Thread(target=worker) for _ in range(8)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(60)
        assert not bad, bad
        st = f.fe.stats()
        assert st["bodies_budget_bytes"] >= 3 * len(body) and st["bodies_budget_bytes"] < 4 * 2 * len(body)
        assert 0 < st["bodies_retained_bytes"] <= st["bodies_budget_bytes"], st
        assert st["bodies_over_budget"] >= 1
        c = f.conn()
        for i in range(20):
            code, _, _ = post(c, "tiny", *request(np.full((1, 3, 8, 8), i, np.float32)))
            assert code == 200
        st = f.fe.stats()
        assert st["bodies_retained_bytes"] <= st["bodies_budget_bytes"], st
    finally:
        f.close()


def test_tensor_codec_fuzz_under_sanitizers():
    """csrc/runtime/kserve.cpp built host-only with AddressSanitizer + UBSan and driven by the stand-alone
    csrc/tests/kserve_tensor_fuzz.cpp: the fixed malformed requests are rejected, valid ones located exactly, the
    builder's responses parse back, 4000 random mutations end without a memory error."""
    import os
    import shutil
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (Path(hipcc).exists() or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    srcs = [root / "csrc" / "tests" / "kserve_tensor_fuzz.cpp", root / "csrc" / "runtime" / "kserve.cpp"]
    exe = root / "build" / "kserve_tensor_fuzz_asan"
    exe.parent.mkdir(parents=True, exist_ok=True)
    newest = max(p.stat().st_mtime for p in srcs + list((root / "csrc" / "runtime").glob("*.h")))
    if not exe.exists() or exe.stat().st_mtime < newest:
        cmd = [hipcc, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Xarch_host",
               "-fsanitize=address,undefined", "-I" + str(root / "csrc"), *map(str, srcs), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe), "4000"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    report = r.stdout + r.stderr
    assert "Sanitizer" not in report and "runtime error" not in report and r.returncode == 0, report[-6000:]
    assert "kserve_tensor_fuzz: ok" in r.stdout
