"""Builders shared by the EXIF orientation tests (test_jpeg_orientation.py, test_jpeg_orientation_gpu.py): tagged
JPEGs written two ways, and the expected upright pixels from PIL's unrotated decode."""
from __future__ import annotations

import io
import struct

import numpy as np
from PIL import Image

LAYOUTS = ["gray", "444", "422", "420"]
_SUB = {"444": 0, "422": 1, "420": 2}


def scene(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([x / max(w, 1) * 200, y / max(h, 1) * 180, (x + y) / max(h + w, 1) * 150], -1)
    img += rng.normal(0, 25, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(arr, layout, exif=None, **kw) -> bytes:
    """A baseline JPEG of `arr` (HxWx3) in one of LAYOUTS; exif: an Image.Exif PIL writes after the JFIF APP0."""
    im = Image.fromarray(arr)
    if layout == "gray":
        im = im.convert("L")
    else:
        kw["subsampling"] = _SUB[layout]
    if exif is not None:
        kw["exif"] = exif
    b = io.BytesIO()
    im.save(b, "JPEG", quality=kw.pop("quality", 90), **kw)
    return b.getvalue()


def pil_exif(orientation: int) -> Image.Exif:
    e = Image.Exif()
    e[0x0112] = orientation
    return e


def app1(orientation, order="<", ifd=8, before=0, after=0, typ=3, count=1, n_entries=None, tag=0x0112) -> bytes:
    """A hand-packed EXIF APP1 segment: byte order `order`, IFD0 at offset `ifd`, `before` / `after` other entries
    around the orientation entry, which has type `typ` and count `count`; n_entries overrides the stated count."""
    tiff = (b"II" if order == "<" else b"MM") + struct.pack(order + "HI", 42, ifd) + bytes(ifd - 8)
    val = struct.pack(order + "HH", orientation, 0) if typ == 3 else struct.pack(order + "I", orientation)
    entries = [struct.pack(order + "HHI", 0x010F + i, 3, 1) + struct.pack(order + "HH", 7, 0) for i in range(before)]
    entries.append(struct.pack(order + "HHI", tag, typ, count) + val)
    entries += [struct.pack(order + "HHI", 0x0131 + i, 3, 1) + struct.pack(order + "HH", 7, 0) for i in range(after)]
    n = len(entries) if n_entries is None else n_entries
    tiff += struct.pack(order + "H", n) + b"".join(entries) + struct.pack(order + "I", 0)
    return segment(0xE1, b"Exif\0\0" + tiff)


def segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def splice(jpeg: bytes, seg: bytes) -> bytes:
    """`seg` right after SOI."""
    assert jpeg[:2] == b"\xff\xd8"
    return jpeg[:2] + seg + jpeg[2:]


def tagged(arr, layout, orientation, how) -> bytes:
    """how: 'pil' (big-endian EXIF written by PIL after APP0), 'le' (hand-packed little-endian after SOI),
    'le_far' (IFD offset 26 and the tag third in the IFD)."""
    if how == "pil":
        return encode(arr, layout, exif=pil_exif(orientation))
    plain = encode(arr, layout)
    if how == "le":
        return splice(plain, app1(orientation))
    return splice(plain, app1(orientation, ifd=26, before=2, after=1))


def unrotated(data: bytes) -> np.ndarray:
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def expected(a: np.ndarray, orientation: int) -> np.ndarray:
    o = orientation
    r = (a if o == 1 else a[:, ::-1] if o == 2 else a[::-1, ::-1] if o == 3 else a[::-1] if o == 4
         else a.transpose(1, 0, 2) if o == 5 else np.rot90(a, -1) if o == 6
         else a[::-1, ::-1].transpose(1, 0, 2) if o == 7 else np.rot90(a, 1) if o == 8 else a)
    return np.ascontiguousarray(r)
