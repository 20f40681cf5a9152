"""Crop transport between the detection and classification services (arm B).

``jpeg``  reference behaviour: PIL JPEG at quality 95 on the detection side,
          PIL decode (gray -> RGB, RGBA -> RGB) on the classification side
          (architectures/microservices/detection/app/grpc_client.py:99-103,
          architectures/microservices/classification/app/servicer.py:65-76).
``png``   lossless, still a standard image format.
``raw``   arena fast path: a 12-byte header (b"ARW1", uint32 h, uint32 w)
          followed by the RGB uint8 pixels — no codec cost on either side,
          and bit-exact crops.

``decode_crop`` sniffs the format, so a classification service accepts all
three from any client.

``GpuCropEncoder`` (``ARENA_CROP_ENCODE=gpu``) makes the ``jpeg`` bytes without
host pixels: the GPU cuts each crop out of the device-resident frame and does
everything up to quantisation (csrc/kernels/jpeg_fdct.hip), C++ threads do the
Huffman pass (csrc/runtime/jpeg_encode.h) — or, with ``entropy="gpu"``
(``ARENA_CROP_ENTROPY=gpu``), the GPU does that too (csrc/kernels/jpeg_huff.hip)
and only the JPEG bytes come back.  The bytes are those of
``encode_crop(extract_crop(frame, box), "jpeg")`` either way.
"""
from __future__ import annotations

import asyncio
import io
import struct

import numpy as np
from PIL import Image

RAW_MAGIC = b"ARW1"
JPEG_QUALITY = 95


def encode_crop(crop: np.ndarray, transport: str = "jpeg") -> bytes:
    crop = np.ascontiguousarray(crop, dtype=np.uint8)
    if crop.ndim != 3 or crop.shape[2] != 3:
        raise ValueError(f"crop must be HxWx3 uint8, got {crop.shape}")
    if transport == "raw":
        return RAW_MAGIC + struct.pack("<II", crop.shape[0], crop.shape[1]) + crop.tobytes()
    buf = io.BytesIO()
    if transport == "jpeg":
        Image.fromarray(crop).save(buf, format="JPEG", quality=JPEG_QUALITY)
    elif transport == "png":
        Image.fromarray(crop).save(buf, format="PNG", compress_level=1)
    else:
        raise ValueError(f"unknown crop transport '{transport}'")
    return buf.getvalue()


def decode_crop(data: bytes) -> np.ndarray:
    if data[:4] == RAW_MAGIC:
        if len(data) < 12:
            raise ValueError("truncated raw crop header")
        h, w = struct.unpack("<II", data[4:12])
        if h <= 0 or w <= 0 or len(data) != 12 + h * w * 3:
            raise ValueError(f"raw crop size mismatch: {h}x{w} with {len(data) - 12} bytes")
        return np.frombuffer(data, dtype=np.uint8, offset=12).reshape(h, w, 3)
    img = Image.open(io.BytesIO(data))
    arr = np.asarray(img)
    if arr.ndim == 2:
        arr = np.stack([arr, arr, arr], axis=-1)
    elif arr.shape[2] == 4:
        arr = arr[:, :, :3]
    return np.ascontiguousarray(arr, dtype=np.uint8)


class GpuCropEncoder:
    """Async face of the native ``CropJpegEncoder``: ``await encode(frame_ptr, h, w, det)`` gives one JPEG per
    detection, cut from the packed RGB frame at device address ``frame_ptr``.  The frame must stay untouched until
    the call has completed; a cancelled caller therefore keeps waiting (the await is shielded) — see
    ``detection_service`` for how the frame's ring slot is held."""

    def __init__(self, device: int = 0, capacity_bytes: int = 0, threads: int = 2, native_encoder=None,
                 entropy: str = "host"):
        if entropy not in ("host", "gpu"):
            raise ValueError(f"unknown crop entropy mode '{entropy}' (host | gpu)")
        if native_encoder is None:
            from ..ops import native

            native_encoder = native().CropJpegEncoder(device, capacity_bytes, threads, entropy)
        self.enc = native_encoder
        self.entropy = entropy

    def submit(self, frame_ptr: int, h: int, w: int, det, frame_bytes: int = 0) -> "asyncio.Future[list[bytes]]":
        """Start the encode; the future completes on the running loop with the blobs or a RuntimeError."""
        loop = asyncio.get_running_loop()
        fut: asyncio.Future = loop.create_future()

        def finish(blobs, error):
            if fut.done():
                return
            if error:
                fut.set_exception(RuntimeError(error))
            else:
                fut.set_result(list(blobs))

        def done(blobs, error):  # on an encoder thread
            loop.call_soon_threadsafe(finish, blobs, error)

        boxes = [(float(d[0]), float(d[1]), float(d[2]), float(d[3])) for d in det]
        self.enc.submit(int(frame_ptr), int(h), int(w), boxes, done, int(frame_bytes))
        return fut

    async def encode(self, frame_ptr: int, h: int, w: int, det, frame_bytes: int = 0) -> list[bytes]:
        return await asyncio.shield(self.submit(frame_ptr, h, w, det, frame_bytes))

    def close(self) -> None:
        self.enc.stop()
