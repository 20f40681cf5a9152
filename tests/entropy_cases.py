"""Crafted coefficient sets of the entropy-coder tests (test_jpeg_entropy.py on the CPU, test_jpeg_entropy_gpu.py on
the GPU): int16[blocks][64] in zigzag order, every value in +-1023, in the layout ``jpeg_write`` reads.

Each of the sizes gets: all zero; all +1023 (the longest codes: the scan overflows the default reserve and its padded
last byte is 0xFF, hence stuffed); all -1023; a sparse mix of +-1023 and +-1 (many 0xFF bytes, adjacent stuffed
pairs); uniform in +-1023; and "runs": alternating DC of +-1023, coefficient 63 = +-1 and coefficient 35 = 5 in every
third block, so that there are zero runs above 15 (ZRL symbols) and no end-of-block code.
test_jpeg_entropy.py asserts those properties on the oracle's bytes, so a case cannot quietly stop exercising its path.
"""
from __future__ import annotations

import numpy as np

SIZES = [(1, 1), (16, 16), (17, 9), (40, 24), (33, 47)]  # w x h
KINDS = ["zero", "plus", "minus", "sparse", "uniform", "runs"]
SEED = 20


def blocks(w: int, h: int) -> int:
    return ((w + 15) // 16) * ((h + 15) // 16) * 6


def make(kind: str, w: int, h: int) -> np.ndarray:
    n = blocks(w, h)
    rng = np.random.default_rng([SEED, KINDS.index(kind), w, h])
    if kind == "zero":
        return np.zeros((n, 64), np.int16)
    if kind == "plus":
        return np.full((n, 64), 1023, np.int16)
    if kind == "minus":
        return np.full((n, 64), -1023, np.int16)
    if kind == "sparse":
        r = rng.integers(0, 8, (n, 64))
        return np.select([r == 0, r == 1, r == 2, r == 3], [1023, -1023, 1, -1], 0).astype(np.int16)
    if kind == "uniform":
        return rng.integers(-1023, 1024, (n, 64)).astype(np.int16)
    if kind == "runs":
        c = np.zeros((n, 64), np.int16)
        b = np.arange(n)
        c[:, 0] = np.where(b % 2 == 0, 1023, -1023)
        c[:, 63] = np.where(b % 4 < 2, 1, -1)
        c[b % 3 == 0, 35] = 5
        return c
    raise ValueError(kind)


def cases():
    """(id, w, h, kind, coefs) for every size and kind."""
    return [(f"{kind}-{w}x{h}", w, h, kind, make(kind, w, h)) for w, h in SIZES for kind in KINDS]


def random_crops(n: int = 50, seed: int = 3):
    """n random RGB crops of 1..70 x 1..70 pixels: noise, flat, or a 0/255 checkerboard."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w, h = int(rng.integers(1, 71)), int(rng.integers(1, 71))
        if i % 3 == 0:
            c = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        elif i % 3 == 1:
            c = np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)).copy()
        else:
            yy, xx = np.mgrid[0:h, 0:w]
            ck = (((yy + xx) & 1) * 255).astype(np.uint8)
            c = np.stack([ck, 255 - ck if i % 2 else ck, ck], -1)
        out.append(c)
    return out


def scan_of(data: bytes) -> bytes:
    """The entropy-coded segment of a baseline file: between the SOS header and EOI."""
    i = data.index(b"\xff\xda")
    n = int.from_bytes(data[i + 2:i + 4], "big")
    assert data[-2:] == b"\xff\xd9"
    return data[i + 2 + n:-2]
