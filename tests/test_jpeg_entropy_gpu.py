"""Device entropy coder of the JPEG crop encoder (csrc/kernels/jpeg_huff.hip, ``entropy="gpu"``) on the GPU.

* the bytes of every crop against PIL over the frames and boxes of test_jpeg_encode_gpu.py, no fallback, guards intact;
* the entropy kernels alone on the crafted coefficient sets (entropy_cases.py) against ``jpeg_write``: with a reserve
  that holds them the device itself makes the heavily stuffed streams and the stuffed padded last byte; with the
  default reserve the all-+1023 sets overflow, are counted as fallbacks and still give the oracle's bytes;
* crops that span many workgroups and stuffing segments: the whole 333x500 synthetic frame (4 032 slots) and a
  640x640 frame of noise (9 600 slots, the most a frame slot holds);
* a buffer so small that the crops need several launches gives the single-launch bytes;
* fewer bytes come back from the device than with ``entropy="host"``;
* end to end: detector -> frame slot -> ``GpuCropEncoder(entropy="gpu")`` gives PIL's bytes.
"""
from __future__ import annotations

import asyncio

import numpy as np
import pytest

import entropy_cases as ec
from inference_arena_amd.ops import native
from inference_arena_amd.processing import extract_crop
from inference_arena_amd.server.crop_codec import encode_crop

pytestmark = pytest.mark.gpu

CASES = ec.cases()
IDS = [c[0] for c in CASES]


def _frames():
    from inference_arena_amd.data.synthetic import synthetic_images

    rng = np.random.default_rng(7)
    return [rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), rng.integers(0, 256, (41, 66, 3), dtype=np.uint8),
            rng.integers(0, 256, (64, 48, 3), dtype=np.uint8), synthetic_images(1, 32, hw=(333, 500))[0]]


def _boxes(h: int, w: int) -> list[tuple[float, float, float, float]]:
    boxes = [(0, 0, w, h),                                                       # the whole frame
             (0, 0, 1, 1), (w - 1, 0, w, 1), (0, h - 1, 1, h), (w - 1, h - 1, w, h),  # 1x1 corners
             (w - 10.5, h - 9.25, w + 7.3, h + 30.0), (-5.5, -2.2, 12.7, 9.9),  # past the edges, below 0: clipped
             (5, 5, 5, 9), (10, 10, 4, 4)]                                       # empty
    sizes = [8, 9, 15, 16, 17, 24]
    for i, s in enumerate(sizes):  # odd x1 / y1: unaligned RGB reads; every width with every other height
        x1, y1 = 1 + 2 * i, 3 + 2 * (i % 2)
        boxes.append((x1 + 0.6, y1 + 0.4, x1 + s + 0.9, y1 + sizes[-1 - i] + 0.2))
        boxes.append((x1, y1, x1 + s, y1 + s))
    return [tuple(float(v) for v in b) for b in boxes]


def _pil_crops(frame, boxes):
    return [encode_crop(extract_crop(frame, b), "jpeg") for b in boxes]


@pytest.fixture(scope="module")
def oracle():
    C = native()
    return {cid: C.jpeg_write(w, h, coefs) for cid, w, h, _, coefs in CASES}


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_device_coded_bytes_equal_pil(device, which):
    C = native()
    frame = _frames()[which]
    boxes = _boxes(*frame.shape[:2])
    assert C.jpeg_encode_device(frame, boxes, 0, entropy="gpu") == _pil_crops(frame, boxes)
    out = C.jpeg_encode_device_coefs(frame, boxes, 0, entropy="gpu", keep_coefs=False)  # raises on touched guards
    want = _pil_crops(frame, boxes)
    assert len(out["blobs"]) == len(want)
    for i, (g, p) in enumerate(zip(out["blobs"], want)):
        assert g == p, f"frame {which} box {i} {boxes[i]}: {len(g)} bytes, PIL {len(p)}"
    assert out["entropy_fallbacks"] == 0 and out["launches"] == 1


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_entropy_kernels_equal_jpeg_write_on_crafted_coefficients(device, case, oracle):
    C = native()
    cid, w, h, kind, coefs = case
    out = C.jpeg_entropy_device(w, h, coefs, reserve_per_block=512)  # raises on touched guards
    assert out["status"] == "ok" and out["fallbacks"] == 0
    assert out["blob"] == oracle[cid]
    assert out["bits"] == int(C.jpeg_block_bits(w, h, coefs).astype(np.int64).sum())
    assert out["scan_bytes"] == len(ec.scan_of(oracle[cid]))
    # the default reserve: 128 bytes per slot
    small = C.jpeg_entropy_device(w, h, coefs)
    assert small["blob"] == oracle[cid]
    if kind == "plus":
        assert small["status"] == "overflow" and small["fallbacks"] >= 1
    elif kind in ("zero", "sparse", "runs"):
        assert small["status"] == "ok" and small["fallbacks"] == 0


def test_entropy_kernels_read_natural_order_blocks(device, oracle):
    C = native()
    zz = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
          61, 54, 47, 55, 62, 63]
    for cid, w, h, kind, coefs in CASES:
        if kind not in ("uniform", "runs") or (w, h) not in ((17, 9), (33, 47)):
            continue
        nat = np.zeros_like(coefs)
        nat[:, zz] = coefs
        out = C.jpeg_entropy_device(w, h, nat, reserve_per_block=512, natural=True)
        assert out["status"] == "ok" and out["blob"] == oracle[cid], cid
    with pytest.raises(ValueError, match="1023"):
        C.jpeg_entropy_device(16, 16, np.full((6, 64), 1024, np.int16))


def test_crops_that_span_many_workgroups_and_segments(device):
    from inference_arena_amd.data.synthetic import synthetic_images

    C = native()
    frame = synthetic_images(1, 32, hw=(333, 500))[0]
    noise = np.random.default_rng(23).integers(0, 256, (640, 640, 3), dtype=np.uint8)
    for img, slots in ((frame, 4032), (noise, 9600)):
        h, w = img.shape[:2]
        assert ec.blocks(w, h) == slots
        out = C.jpeg_encode_device_coefs(img, [(0.0, 0.0, float(w), float(h))], 0, entropy="gpu", keep_coefs=False)
        want = encode_crop(img, "jpeg")
        assert len(ec.scan_of(want)) > 3 * 4096  # several stuffing segments
        assert out["blobs"] == [want]
        assert out["entropy_fallbacks"] == 0


def test_chunked_launches_give_the_single_launch_bytes(device):
    C = native()
    frame = _frames()[3]
    h, w = frame.shape[:2]
    rng = np.random.default_rng(11)
    boxes = []
    for _ in range(24):
        x1, y1 = rng.uniform(0, w - 40), rng.uniform(0, h - 40)
        boxes.append((float(x1), float(y1), float(x1 + rng.uniform(20, 120)), float(y1 + rng.uniform(20, 120))))
    single = C.jpeg_encode_device_coefs(frame, boxes, 0, entropy="gpu")
    assert single["launches"] == 1
    # room for the largest crop (128 x 128 pixels at most: 8 x 8 MCUs of 6 blocks of 128 bytes) and little more
    chunked = C.jpeg_encode_device_coefs(frame, boxes, 0, capacity_bytes=2 * 64 * 6 * 128, entropy="gpu")
    assert chunked["launches"] >= 3
    assert chunked["blobs"] == single["blobs"] == _pil_crops(frame, boxes)
    assert chunked["entropy_fallbacks"] == single["entropy_fallbacks"] == 0
    host = C.jpeg_encode_device_coefs(frame, boxes, 0)  # keep_coefs keeps working in gpu mode: the same coefficients
    for a, b, c in zip(chunked["coefs"], single["coefs"], host["coefs"]):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)


def test_fewer_bytes_come_back_from_the_device(device):
    C = native()
    frame = _frames()[3]
    boxes = _boxes(*frame.shape[:2])
    host = C.jpeg_encode_device_coefs(frame, boxes, 0, entropy="host", keep_coefs=False)
    gpu = C.jpeg_encode_device_coefs(frame, boxes, 0, entropy="gpu", keep_coefs=False)
    print(f"d2h_bytes: host {host['d2h_bytes']}, gpu {gpu['d2h_bytes']}")
    assert gpu["blobs"] == host["blobs"]
    assert 0 < gpu["d2h_bytes"] < host["d2h_bytes"]
    assert "coefs" not in gpu and "coefs" not in host


def test_detector_frame_to_crop_bytes_end_to_end(device):
    """detect_bytes(upload, export_to=slot) then GpuCropEncoder(entropy="gpu").encode from that slot: the bytes of PIL
    encodes of extract_crop(PIL-decoded upload, det)."""
    from inference_arena_amd.data.synthetic import encode_jpeg, synthetic_images
    from inference_arena_amd.models.zoo import make_yolo
    from inference_arena_amd.processing.transforms import load_image_from_bytes
    from inference_arena_amd.server.crop_codec import GpuCropEncoder
    from inference_arena_amd.server.device_transport import DeviceImageRing
    from inference_arena_amd.server.service_backends import GpuDetectorBackend

    uploads = [encode_jpeg(im) for im in synthetic_images(1, 51) + synthetic_images(1, 52, hw=(333, 500))]
    be = GpuDetectorBackend(make_yolo(0, cls_shift=-20.0), device=0, max_batch=1)
    ring = DeviceImageRing(2, 640 * 640 * 3, device=0)
    enc = GpuCropEncoder(device=0, entropy="gpu")
    assert enc.enc.entropy == "gpu"

    async def decode(data):
        raise AssertionError("the split decoder covers these uploads")

    async def go():
        outs = []
        for data in uploads:
            image = load_image_from_bytes(data)
            h, w = image.shape[:2]
            slot = ring.acquire()
            try:
                det, _ = await be.detect_bytes(data, decode, export_to=ring.slot_ptr(slot))
                blobs = await enc.encode(ring.slot_ptr(slot), h, w, det, frame_bytes=ring.slot_bytes)
            finally:
                ring.release(slot)
            outs.append((image, det, blobs))
        return outs

    try:
        outs = asyncio.run(go())
        fallbacks = enc.enc.entropy_fallbacks
    finally:
        enc.close()
        be.close()
    total = 0
    for image, det, blobs in outs:
        assert len(blobs) == len(det)
        total += len(det)
        for d, b in zip(det, blobs):
            assert b == encode_crop(extract_crop(image, d), "jpeg")
    assert total >= 1 and fallbacks == 0
