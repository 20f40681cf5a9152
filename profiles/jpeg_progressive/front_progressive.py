"""One native-front-end run over the curated workload (GPU): req/s and host CPU per request.

    python profiles/jpeg_progressive/front_progressive.py off|on|baseline [requests]

off / on: the 100 curated images as progressive JPEG (q90, 4:2:0) with FrontConfig.progressive off (every upload to
the 8 PIL decode processes: the behaviour before the switch existed) or on (8 split-decoder threads); baseline: the
same images as baseline JPEG.  bench.py's program (default_models(0), buckets [1, 32], fp32) behind its batcher
settings, 256 closed-loop users of the native load generator, 1500 warm-up requests.  Prints one RESULT line: req/s,
P50, the front end's own CPU counters per request, and the CPU of the whole process tree per request (decode
processes and the load generator's two threads included)."""
import io, json, os, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from PIL import Image
import bench
from inference_arena_amd.data.curator import workload_images
from inference_arena_amd.engine.pipeline import GpuPipeline
from inference_arena_amd.labels import load_labels
from inference_arena_amd.models.zoo import default_models
from inference_arena_amd.ops import native
from inference_arena_amd.server.native_front import NativeFrontEnd

def tree_cpu():
    tick, stats = os.sysconf("SC_CLK_TCK"), {}
    for p in os.listdir("/proc"):
        if not p.isdigit():
            continue
        try:
            f = open(f"/proc/{p}/stat").read().rsplit(")", 1)[1].split()
        except OSError:
            continue
        stats[int(p)] = (int(f[1]), (int(f[11]) + int(f[12])) / tick)
    keep, grew = {os.getpid()}, True
    while grew:  # every descendant (the decode processes hang below multiprocessing's helpers)
        grew = False
        for pid, (ppid, _) in stats.items():
            if ppid in keep and pid not in keep:
                keep.add(pid)
                grew = True
    return sum(stats[p][1] for p in keep if p in stats)

if __name__ == '__main__':
    C = native()
    imgs = workload_images()
    def enc(im, **kw):
        b = io.BytesIO(); Image.fromarray(im).save(b, format="JPEG", quality=90, **kw); return b.getvalue()
    which = sys.argv[1]
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 12000
    uploads = [enc(im, progressive=(which != "baseline")) for im in imgs]
    reqs = [bench.http_request(u) for u in uploads]
    pipe = GpuPipeline(*default_models(0), device=0, buckets=[1, 32], dtype="fp32")
    batcher = C.DynamicBatcher([pipe.ex], {"max_batch": 32, "max_queue_delay_us": 2000, "idle_queue_delay_us": 100, "max_queue_size": 0})
    fe = NativeFrontEnd(batcher, load_labels(None), port=0, host="127.0.0.1", io_threads=4, decode_procs=8, slots=512,
                        decode_threads=8, progressive=(which == "on"))
    try:
        users, warm = 256, 1500
        lg = C.HttpLoadGen({"host": "127.0.0.1", "port": fe.port, "users": users, "threads": 2}, reqs)
        lg.start()
        try:
            assert lg.wait_completed(warm, 200.0), lg.completed()
            s0, c0, t0 = fe.stats(), tree_cpu(), time.time()
            assert lg.wait_completed(warm + N, 400.0), lg.completed()
            s1, c1, t1 = fe.stats(), tree_cpu(), time.time()
        finally:
            lg.stop(60.0)
        r = lg.records(warm, warm + N)
        t = r["t_done"]
        n = s1["requests"] - s0["requests"]
        out = {"workload": which, "requests": int(len(t)), "errors": int((r["status"] != 200).sum()),
               "req_s": round(float((len(t) - 1) / (t[-1] - t[0])), 1),
               "p50_ms": round(float(np.percentile(r["latency"] * 1e3, 50)), 2),
               "front_cpu_us_per_req": {k: round((s1[k] - s0[k]) / n * 1e3, 1) for k in ("cpu_parse_ms", "cpu_decode_ms", "cpu_json_ms")},
               "process_tree_cpu_us_per_req(incl. load generator)": round((c1 - c0) / n * 1e6, 1),
               "native_decoded": s1["native_decoded"], "fallback_decoded": s1["fallback_decoded"],
               "progressive_decoded": s1["progressive_decoded"]}
        print("RESULT " + json.dumps(out), flush=True)
    finally:
        fe.close()
        batcher.shutdown()
