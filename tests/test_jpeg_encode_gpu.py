"""Device half of the JPEG crop encoder (csrc/kernels/jpeg_fdct.hip) on the GPU.

* the bytes of every crop of a device-resident frame against PIL (``encode_crop(extract_crop(frame, box))``):
  whole frames, 1x1 corners, clipped float boxes, odd origins (unaligned RGB reads), sizes around the 8 / 16 block
  and MCU edges, an empty box; the guard bytes around the encoder's device buffer stay intact;
* the kernel's coefficients against the host oracle (the same arithmetic, kernels/jpeg_enc_math.h) and against the
  coefficients the repository's decoder reads out of PIL's file, to localise a failure;
* a buffer so small that the crops need several launches gives the single-launch result;
* end to end: the GPU detector reconstructs an upload into a frame slot (split decoder), the encoder cuts the
  detections' crops from that slot — the bytes PIL makes from the PIL-decoded upload.
"""
from __future__ import annotations

import asyncio

import numpy as np
import pytest

from inference_arena_amd.ops import native
from inference_arena_amd.processing import extract_crop
from inference_arena_amd.server.crop_codec import encode_crop

pytestmark = pytest.mark.gpu

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
      28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
      47, 55, 62, 63]  # zigzag index -> natural index


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


def _scan_blocks(C, data: bytes, w: int, h: int):
    """The coefficients the repository's decoder reads from ``data`` in the encoder's layout (int16[blocks][64],
    zigzag, scan order MCU by MCU) and the mask of real (not dummy) block slots."""
    d = C.jpeg_coefs(data)
    assert d["status"] == "ok", d["error"]
    mcux, mcuy, ybw, ybh = (w + 15) // 16, (h + 15) // 16, (w + 7) // 8, (h + 7) // 8
    out = np.zeros((mcux * mcuy * 6, 64), np.int16)
    real = np.zeros(len(out), bool)
    for my in range(mcuy):
        for mx in range(mcux):
            for s in range(6):
                c = 0 if s < 4 else s - 3
                by, bx = (2 * my + (s >> 1), 2 * mx + (s & 1)) if s < 4 else (my, mx)
                k = d["comps"][c]
                off = k["coef_off"] + (by * k["bw"] + bx) * 64
                i = (my * mcux + mx) * 6 + s
                out[i] = d["coef"][off:off + 64][ZZ]
                real[i] = s >= 4 or (by < ybh and bx < ybw)
    return out, real


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_device_bytes_equal_pil(device, which):
    C = native()
    frame = _frames()[which]
    boxes = _boxes(*frame.shape[:2])
    got = C.jpeg_encode_device(frame, boxes, 0)  # raises if the guard bytes were touched
    want = _pil_crops(frame, boxes)
    assert len(got) == len(want)
    for i, (g, p) in enumerate(zip(got, want)):
        assert g == p, f"frame {which} box {i} {boxes[i]}: {len(g)} bytes, PIL {len(p)}"


@pytest.mark.parametrize("which", [0, 3])
def test_device_coefficients_equal_the_host_oracle_and_pil(device, which):
    C = native()
    frame = _frames()[which]
    boxes = _boxes(*frame.shape[:2])
    out = C.jpeg_encode_device_coefs(frame, boxes, 0)
    assert out["launches"] == 1
    decoded = 0
    for i, (b, cf) in enumerate(zip(boxes, out["coefs"])):
        crop = extract_crop(frame, b)
        h, w = crop.shape[:2]
        if cf.size == 0:  # an empty box: no device work, the 1x1 black crop
            assert np.array_equal(crop, np.zeros((1, 1, 3), np.uint8))
            continue
        np.testing.assert_array_equal(cf, C.jpeg_encode_coefs_host(crop), err_msg=f"box {i} {b}: device vs host oracle")
        if w <= 4:  # the decoder leaves files with fewer than 3 chroma columns to PIL
            continue
        pil, real = _scan_blocks(C, encode_crop(crop, "jpeg"), w, h)
        np.testing.assert_array_equal(cf[real], pil[real], err_msg=f"box {i} {b}: device vs PIL's coefficients")
        decoded += 1
    assert decoded >= 10


def test_chunked_launches_give_the_single_launch_result(device):
    C = native()
    frame = _frames()[3]
    h, w = frame.shape[:2]
    rng = np.random.default_rng(11)
    boxes = []
    for _ in range(24):
        x1, y1 = rng.uniform(0, w - 40), rng.uniform(0, h - 40)
        boxes.append((float(x1), float(y1), float(x1 + rng.uniform(20, 120)), float(y1 + rng.uniform(20, 120))))
    single = C.jpeg_encode_device_coefs(frame, boxes, 0)
    assert single["launches"] == 1
    # room for the largest crop (128 x 128 pixels at most: 8 x 8 MCUs of 6 blocks of 128 bytes) and little more
    chunked = C.jpeg_encode_device_coefs(frame, boxes, 0, capacity_bytes=2 * 64 * 6 * 128)
    assert chunked["launches"] >= 3
    assert chunked["blobs"] == single["blobs"] == _pil_crops(frame, boxes)
    for a, b in zip(chunked["coefs"], single["coefs"]):
        np.testing.assert_array_equal(a, b)


def test_detector_frame_to_crop_bytes_end_to_end(device):
    """detect_bytes(upload, export_to=slot) then GpuCropEncoder.encode from that slot: the bytes of PIL encodes of
    extract_crop(PIL-decoded upload, det), because the split decoder's frame is PIL's."""
    from inference_arena_amd.data.synthetic import encode_jpeg, synthetic_images
    from inference_arena_amd.models.zoo import make_yolo
    from inference_arena_amd.processing.transforms import load_image_from_bytes
    from inference_arena_amd.server.crop_codec import GpuCropEncoder
    from inference_arena_amd.server.device_transport import DeviceImageRing
    from inference_arena_amd.server.service_backends import GpuDetectorBackend

    uploads = [encode_jpeg(im) for im in synthetic_images(1, 51) + synthetic_images(1, 52, hw=(333, 500))]
    be = GpuDetectorBackend(make_yolo(0, cls_shift=-20.0), device=0, max_batch=1)
    ring = DeviceImageRing(2, 640 * 640 * 3, device=0)
    enc = GpuCropEncoder(device=0)

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
    finally:
        enc.close()
        be.close()
    total = 0
    for image, det, blobs in outs:
        assert len(blobs) == len(det)
        total += len(det)
        for d, b in zip(det, blobs):
            assert b == encode_crop(extract_crop(image, d), "jpeg")
    assert total >= 1
