"""EXIF orientation of a JPEG upload, by the rule of the native parser (csrc/runtime/jpeg_decode.h).

The reference decodes with ``cv2.imdecode``, which applies the EXIF ``Orientation`` tag of a JPEG; every decode
path of the arena therefore returns the upright image.  The split decoder reads the tag in ``jpeg_parse``; this
module is its pure-Python twin for the paths that decode with PIL (``processing/transforms.py``,
``server/app_common.py::probe_size``), so that the two never disagree on a file.  ``Image.getexif()`` is not used:
Pillow falls back to an orientation stated in XMP, which cv2 ignores.

Rule: the first APP1 segment before SOS whose payload starts with ``Exif\\0\\0`` decides.  Its TIFF header
(``II`` or ``MM``, 42, IFD0 offset) leads to IFD0; the first entry with tag 0x0112 counts when it is one SHORT
with a value of 1..8.  Everything else is 1: no such segment, another type or count, a value of 0 or 9, an IFD
or entry table that leaves the segment.
"""
from __future__ import annotations

_EXIF = b"Exif\0\0"


def _tiff_orientation(t: bytes) -> int:
    n = len(t)
    if n < 8:
        return 1
    if t[:2] == b"II":
        order = "little"
    elif t[:2] == b"MM":
        order = "big"
    else:
        return 1

    def u(o: int, k: int) -> int:
        return int.from_bytes(t[o:o + k], order)

    if u(2, 2) != 42:
        return 1
    ifd = u(4, 4)
    if ifd + 2 > n:
        return 1
    count = u(ifd, 2)
    if ifd + 2 + 12 * count > n:
        return 1
    for i in range(count):
        e = ifd + 2 + 12 * i
        if u(e, 2) != 0x0112:
            continue
        if u(e + 2, 2) != 3 or u(e + 4, 4) != 1:
            return 1
        v = u(e + 8, 2)
        return v if 1 <= v <= 8 else 1
    return 1


def jpeg_orientation(data: bytes | bytearray | memoryview) -> int:
    """EXIF orientation (1..8) of encoded image bytes; 1 for anything that is not a JPEG with a well-formed tag.
    The marker walk is ``jpeg_parse``'s: fill bytes and garbage between markers are skipped, the walk ends at SOS,
    EOI or a segment that runs past the data."""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        return 1
    pos = 2
    while True:
        while pos < n and d[pos] != 0xFF:
            pos += 1
        while pos < n and d[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return 1
        m = d[pos]
        pos += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9 or m == 0xDA or pos + 2 > n:
            return 1
        ln = (d[pos] << 8) | d[pos + 1]
        if ln < 2 or pos + ln > n:
            return 1
        seg = d[pos + 2:pos + ln]
        pos += ln
        if m == 0xE1 and seg[:6] == _EXIF:
            return _tiff_orientation(seg[6:])


def orient(im, orientation: int):
    """A PIL image turned upright for an EXIF orientation (the transposes of ``ImageOps.exif_transpose``)."""
    if not 2 <= orientation <= 8:
        return im
    from PIL import Image

    T = Image.Transpose
    return im.transpose({2: T.FLIP_LEFT_RIGHT, 3: T.ROTATE_180, 4: T.FLIP_TOP_BOTTOM, 5: T.TRANSPOSE,
                         6: T.ROTATE_270, 7: T.TRANSVERSE, 8: T.ROTATE_90}[orientation])
