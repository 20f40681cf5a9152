"""One GpuCropEncoder.encode() call next to PIL's encode_crop over the same crops of the curated workload.

For each of the first N curated images: the GPU detector finds the boxes, the frame goes into a device ring slot,
and both encoders make the crops' JPEGs (they must be equal).  Prints one JSON line: per-image medians of the
encode() wall time (submit to completed future: kernel, copy back, Huffman threads) and of the PIL loop, and the
sums over the workload.  Run from the repository root on a GPU: python profiles/crop_encode/encode_batch.py [N]
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
REPS = 7


async def main():
    images = workload_images(N)
    yolo, _ = default_models(0)  # the seeded networks the curated workload was made for
    be = GpuDetectorBackend(yolo, device=0, max_batch=1)
    ring = DeviceImageRing(1, 640 * 640 * 3, device=0)
    enc = GpuCropEncoder(device=0)
    rows = []
    try:
        for im in images:
            det, _ = await be.detect(im)
            if len(det) == 0:
                continue
            slot, _ = ring.put(im)
            h, w = im.shape[:2]
            t_gpu, t_pil = [], []
            for _ in range(REPS):
                t0 = time.perf_counter()
                blobs = await enc.encode(ring.slot_ptr(slot), h, w, det, frame_bytes=ring.slot_bytes)
                t_gpu.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                ref = [encode_crop(extract_crop(im, d), "jpeg") for d in det]
                t_pil.append(time.perf_counter() - t0)
            assert blobs == ref
            ring.release(slot)
            rows.append((len(det), sum(len(b) for b in blobs), statistics.median(t_gpu), statistics.median(t_pil)))
    finally:
        enc.close()
        be.close()
    g = [r[2] * 1e3 for r in rows]
    p = [r[3] * 1e3 for r in rows]
    print(json.dumps({"images": len(rows), "crops": sum(r[0] for r in rows), "jpeg_bytes": sum(r[1] for r in rows),
                      "reps": REPS, "gpu_encode_ms_median_per_image": round(statistics.median(g), 4),
                      "pil_encode_ms_median_per_image": round(statistics.median(p), 4),
                      "gpu_encode_ms_sum": round(sum(g), 3), "pil_encode_ms_sum": round(sum(p), 3),
                      "bytes_equal": True}))


asyncio.run(main())
