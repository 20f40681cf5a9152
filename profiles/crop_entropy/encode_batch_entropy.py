"""One GpuCropEncoder.encode() call with entropy="host" next to entropy="gpu", the protocol of
profiles/crop_encode/encode_batch.py.

For each of the first N curated images: the GPU detector finds the boxes, the frame goes into a device ring slot, and
both encoders make the crops' JPEGs, alternating; the bytes must equal PIL's.  Prints one JSON line: per-image
medians over REPS repetitions of the encode() wall time (submit to completed future) in both modes and their sums
over the workload, the bytes each mode copied device to host and its launches (chunks; entropy="gpu" queues five
more kernels and a memset per chunk), and the fallbacks.  Run from the repository root on an idle GPU:
python profiles/crop_entropy/encode_batch_entropy.py [N] [REPS]
"""
import asyncio
import json
import statistics
import sys
import time

sys.path.insert(0, ".")

from inference_arena_amd.data.curator import workload_images  # noqa: E402
from inference_arena_amd.models.zoo import default_models  # noqa: E402
from inference_arena_amd.processing import extract_crop  # noqa: E402
from inference_arena_amd.server.crop_codec import GpuCropEncoder, encode_crop  # noqa: E402
from inference_arena_amd.server.device_transport import DeviceImageRing  # noqa: E402
from inference_arena_amd.server.service_backends import GpuDetectorBackend  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
MODES = ("host", "gpu")


async def main():
    images = workload_images(N)
    yolo, _ = default_models(0)  # the seeded networks the curated workload was made for
    be = GpuDetectorBackend(yolo, device=0, max_batch=1)
    ring = DeviceImageRing(1, 640 * 640 * 3, device=0)
    encs = {m: GpuCropEncoder(device=0, entropy=m) for m in MODES}
    rows = []
    try:
        for im in images:
            det, _ = await be.detect(im)
            if len(det) == 0:
                continue
            slot, _ = ring.put(im)
            h, w = im.shape[:2]
            t = {m: [] for m in MODES}
            blobs = {}
            for _ in range(REPS):
                for m in MODES:
                    t0 = time.perf_counter()
                    blobs[m] = await encs[m].encode(ring.slot_ptr(slot), h, w, det, frame_bytes=ring.slot_bytes)
                    t[m].append(time.perf_counter() - t0)
            ref = [encode_crop(extract_crop(im, d), "jpeg") for d in det]
            assert blobs["host"] == ref and blobs["gpu"] == ref
            ring.release(slot)
            rows.append((len(det), sum(len(b) for b in ref), {m: statistics.median(t[m]) * 1e3 for m in MODES}))
        stats = {m: (encs[m].enc.d2h_bytes, encs[m].enc.launches, encs[m].enc.entropy_fallbacks) for m in MODES}
    finally:
        for e in encs.values():
            e.close()
        be.close()
    out = {"images": len(rows), "crops": sum(r[0] for r in rows), "jpeg_bytes": sum(r[1] for r in rows), "reps": REPS,
           "bytes_equal": True}
    jobs = len(rows) * REPS
    for m in MODES:
        ms = [r[2][m] for r in rows]
        out[f"{m}_encode_ms_median_per_image"] = round(statistics.median(ms), 4)
        out[f"{m}_encode_ms_sum"] = round(sum(ms), 3)
        out[f"{m}_d2h_bytes_per_job"] = round(stats[m][0] / jobs, 1)
        out[f"{m}_chunks_per_job"] = round(stats[m][1] / jobs, 3)
        out[f"{m}_entropy_fallbacks"] = stats[m][2]
    print(json.dumps(out))


asyncio.run(main())
