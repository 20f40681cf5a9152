"""Classifier batches of the curated workload's crops: launch plan (CPU) and kernel-time driver (GPU) of the ragged
JPEG reconstruction against the rectangular one.

The crops are those of profiles/crop_encode/encode_batch.py: for each of the 100 curated images the detector's
boxes, cut with extract_crop and encoded with encode_crop(..., "jpeg") (q95, 4:2:0), in arrival order.  Here the
boxes come from the fp32 CPU detector (CpuDetectorBackend, the oracle of the GPU program), so that the plan needs
no GPU; `--save` keeps the crops for the GPU run.  Run from the repository root:

  python profiles/crop_decode/crop_batches.py plan [--save crops.npz]
      per batch of 128 crops: workgroups launched by the ragged kernels and by the rectangular pair (host only)
  rocprofv3 --kernel-trace --stats ... -- python profiles/crop_decode/crop_batches.py kernels [--crops crops.npz]
      one batch of 128 crops through jpeg_decode_device: one warm-up and three repeats of the ragged launch, then
      of the rectangular one (compact payload, as the serving path ships it); results compared equal
  python profiles/crop_decode/crop_batches.py trace <kernel_trace.csv>
      per dispatch of the four reconstruction kernels in a rocprofv3 kernel trace: duration; sums per launch
"""
import argparse
import csv
import json
import re
import sys

import numpy as np

sys.path.insert(0, ".")

BATCH = 128
KERNELS = ("jpeg_idct_ragged_kernel", "jpeg_color_ragged_kernel", "jpeg_idct_kernel", "jpeg_color_kernel")


def workload_crops() -> list[bytes]:
    from inference_arena_amd.config import get_model_config
    from inference_arena_amd.data.curator import workload_images
    from inference_arena_amd.models.zoo import default_models
    from inference_arena_amd.processing import extract_crop
    from inference_arena_amd.server.crop_codec import encode_crop
    from inference_arena_amd.server.service_backends import CpuDetectorBackend

    y = get_model_config("yolov5n")
    be = CpuDetectorBackend(default_models(0)[0], threads=8, conf_thr=float(y["confidence_threshold"]),
                            iou_thr=float(y["iou_threshold"]))
    crops = []
    try:
        for im in workload_images(100):
            det, _ = be._run(im)
            crops += [encode_crop(extract_crop(im, d), "jpeg") for d in det]
    finally:
        be.close()
    return crops


def load_crops(path) -> list[bytes]:
    if not path:
        return workload_crops()
    z = np.load(path)
    blob, ends = z["blob"].tobytes(), z["ends"]
    return [blob[a:b] for a, b in zip([0, *ends[:-1]], ends)]


def plan(args):
    from inference_arena_amd.ops import native

    C = native()
    crops = load_crops(args.crops)
    if args.save:
        np.savez(args.save, blob=np.frombuffer(b"".join(crops), np.uint8), ends=np.cumsum([len(c) for c in crops]))
    sizes = [(d["height"], d["width"]) for d in (C.jpeg_coefs(c) for c in crops)]
    px = [h * w for h, w in sizes]
    rows = []
    for k in range(0, len(crops), BATCH):
        p = C.jpeg_ragged_plan(crops[k:k + BATCH])
        rows.append({"crops": len(crops[k:k + BATCH]), "min_pixels": min(px[k:k + BATCH]),
                     "max_pixels": max(px[k:k + BATCH]),
                     **{key: int(p[key]) for key in ("idct_units", "color_units", "rect_idct_units", "rect_color_units")}})
    tot = {key: sum(r[key] for r in rows) for key in ("idct_units", "color_units", "rect_idct_units", "rect_color_units")}
    print(json.dumps({"crops": len(crops), "jpeg_bytes": sum(len(c) for c in crops), "batch": BATCH, "batches": rows,
                      "total": tot, "ragged_workgroups": tot["idct_units"] + tot["color_units"],
                      "rectangular_workgroups": tot["rect_idct_units"] + tot["rect_color_units"]}))


def kernels(args):
    from inference_arena_amd.ops import native

    C = native()
    batch = load_crops(args.crops)[:BATCH]
    out = {}
    for ragged in (True, False):
        for _ in range(1 + args.repeats):  # the first launch of each loads the code object: warm-up
            out[ragged] = C.jpeg_decode_device(batch, 0, compact=True, ragged=ragged)
    equal = all(np.array_equal(a, b) for a, b in zip(out[True], out[False]))
    print(json.dumps({"crops": len(batch), "repeats": args.repeats, "ragged_equals_rectangular": equal,
                      "plan": {k: (int(v) if not isinstance(v, list) else None)
                               for k, v in C.jpeg_ragged_plan(batch).items() if not isinstance(v, list)}}))
    if not equal:
        sys.exit(1)


def trace(args):
    rows = []
    with open(args.csv, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            k = next((k for k in KERNELS if re.search(r"(?<![A-Za-z_])" + k + r"($|[(E. ])", name)), None)
            if k is not None:
                rows.append((int(r["Start_Timestamp"]), k, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    per = {k: [ns for _, kk, ns in rows if kk == k] for k in KERNELS}
    pairs = {"ragged": [a + b for a, b in zip(per[KERNELS[0]], per[KERNELS[1]])],
             "rectangular": [a + b for a, b in zip(per[KERNELS[2]], per[KERNELS[3]])]}
    print(json.dumps({"duration_ns": per, "pair_sum_ns_first_is_warmup": pairs}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)
    p = sub.add_parser("plan")
    p.add_argument("--crops")
    p.add_argument("--save")
    p.set_defaults(fn=plan)
    k = sub.add_parser("kernels")
    k.add_argument("--crops")
    k.add_argument("--repeats", type=int, default=3)
    k.set_defaults(fn=kernels)
    t = sub.add_parser("trace")
    t.add_argument("csv")
    t.set_defaults(fn=trace)
    a = ap.parse_args()
    a.fn(a)


if __name__ == "__main__":
    main()
