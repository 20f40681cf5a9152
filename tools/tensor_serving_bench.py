#!/usr/bin/env python3
"""Tensor models of the model server, native REST endpoint against the Python gRPC servicer, on one GPU.

One server process (model repository built from seed 0, ``ModelServer(device="gpu")``, gRPC servicer and the native
KServe endpoint over the same batchers) and one client process per measurement (this script with ``--client``; it
opens no GPU).  For ``yolov5n`` ([1,3,640,640]) and ``mobilenetv2`` ([1,3,224,224]) and each connection count, the
two paths run one after the other with the same closed-loop client: a thread per connection builds every request
from the same float32 array (HTTP: JSON header + raw bytes; gRPC: a ModelInferRequest), sends it, decodes the output
tensor.  Recorded per run: req/s, P50 / P99 latency at the client, the batcher's mean batch over the run, and the
client's CPU seconds per wall second (about 1.0 = the Python client, one GIL, is the bottleneck).

    python tools/tensor_serving_bench.py --out profiles/native_tensor/serving.json
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import tempfile
import threading
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

MODELS = {"yolov5n": ("images", "output0", (1, 3, 640, 640)), "mobilenetv2": ("input", "output", (1, 3, 224, 224))}


def client(path: str, port: int, model: str, conns: int, seconds: float) -> dict:
    in_name, out_name, shape = MODELS[model]
    x = np.random.default_rng(1).random(shape, dtype=np.float32)
    lat: list[list[float]] = [[] for _ in range(conns)]
    errors = [0] * conns
    t_end = time.monotonic() + seconds

    def http_worker(k):
        import http.client

        c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        while time.monotonic() < t_end:
            t0 = time.perf_counter()
            raw = x.tobytes()
            hb = json.dumps({"inputs": [{"name": in_name, "shape": list(shape), "datatype": "FP32",
                                         "parameters": {"binary_data_size": len(raw)}}]}).encode()
            c.request("POST", f"/v2/models/{model}/infer", body=hb + raw,
                      headers={"Inference-Header-Content-Length": str(len(hb))})
            r = c.getresponse()
            data = r.read()
            if r.status != 200:
                errors[k] += 1
                continue
            n = int(r.getheader("Inference-Header-Content-Length"))
            np.frombuffer(data[n:], np.float32)
            lat[k].append(time.perf_counter() - t0)

    def grpc_worker(k):
        import grpc

        from inference_arena_amd.proto import kserve as kv
        from inference_arena_amd.server.model_server import GRPC_OPTIONS

        ch = grpc.insecure_channel(f"127.0.0.1:{port}", options=GRPC_OPTIONS)
        stub = kv.GRPCInferenceService.stub(ch)
        while time.monotonic() < t_end:
            t0 = time.perf_counter()
            try:
                kv.decode_outputs(stub.ModelInfer(kv.make_infer_request(model, {in_name: x}, [out_name]), timeout=60))
            except grpc.RpcError:
                errors[k] += 1
                continue
            lat[k].append(time.perf_counter() - t0)

    c0, w0 = time.process_time(), time.monotonic()
    ts = [threading.Thread(target=http_worker if path == "native" else grpc_worker, args=(k,)) for k in range(conns)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    wall = time.monotonic() - w0
    all_lat = np.sort(np.concatenate([np.asarray(v) for v in lat])) if any(lat) else np.zeros(1)
    return {"req_s": round(len(all_lat) / wall, 1), "p50_ms": round(float(np.percentile(all_lat, 50)) * 1e3, 3),
            "p99_ms": round(float(np.percentile(all_lat, 99)) * 1e3, 3), "errors": int(sum(errors)),
            "client_cpu_per_wall": round((time.process_time() - c0) / wall, 2)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--client", nargs=4, metavar=("PATH", "PORT", "MODEL", "CONNS"), default=None)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--conns", default="1,8,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.client:
        path, port, model, conns = a.client
        print(json.dumps(client(path, int(port), model, int(conns), a.seconds)))
        return 0

    import asyncio
    import socket

    from inference_arena_amd.repository import store
    from inference_arena_amd.server.model_server import start_grpc, start_native_kserve
    from inference_arena_amd.server.modelserver_core import ModelServer

    def free_port():
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            return s.getsockname()[1]

    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        store.build_repository(Path(tmp), seed=0)
        server = ModelServer(Path(tmp), device="gpu")
        assert not server.failed, server.failed
        loop = asyncio.new_event_loop()
        gport, ready = free_port(), threading.Event()
        holder = {}

        async def boot():
            holder["g"], _ = await start_grpc(server, "127.0.0.1", gport)
            ready.set()

        th = threading.Thread(target=lambda: (loop.run_until_complete(boot()), loop.run_forever()), daemon=True)
        th.start()
        assert ready.wait(60)
        fe = start_native_kserve(server, "127.0.0.1", free_port())
        assert fe is not None
        try:
            for model in MODELS:
                for conns in (int(c) for c in a.conns.split(",")):
                    for path, port in (("native", fe.port), ("grpc", gport)):
                        b0 = server.models[model].batcher.stats()
                        r = subprocess.run([sys.executable, __file__, "--client", path, str(port), model, str(conns),
                                            "--seconds", str(a.seconds)], capture_output=True, text=True, timeout=300)
                        if r.returncode != 0:
                            raise SystemExit(f"client failed: {r.stderr[-2000:]}")
                        b1 = server.models[model].batcher.stats()
                        nb = b1["batches"] - b0["batches"]
                        row = {"model": model, "conns": conns, "path": path, **json.loads(r.stdout.strip().splitlines()[-1]),
                               "mean_batch": round((b1["requests"] - b0["requests"]) / nb, 2) if nb else 0.0}
                        rows.append(row)
                        print(json.dumps(row), flush=True)
        finally:
            fe.close()
            asyncio.run_coroutine_threadsafe(holder["g"].stop(0), loop).result(10)
            loop.call_soon_threadsafe(loop.stop)
            th.join(10)
            server.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
