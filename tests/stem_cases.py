"""Inputs and host models shared by the tests of the fused bf16 front ends (csrc/kernels/stem_fused.hip):
test_stem_cases.py (CPU) and test_stem_fused_gpu.py.  A plain helper module, imported like detect_cases.py.

* letterbox images and crops sized for a small ``S`` that reach every path of ``build_s2d_tile`` (unit scale,
  clamped upscales, source rows staged in LDS at all four byte alignments, regions over the staging budget);
* ``tile_kinds``: which tiles of an item the kernel stages, by the kernel's own rule ``nrows * pitch <= budget``;
* selector weights that copy one (tap, channel) of the s2d tile to an output channel, and the shift of the unfused
  op's output that the fused kernel must then reproduce bit for bit.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import tie_image as ti
from inference_arena_amd.processing.transforms import _lin_taps, letterbox_geometry

CAP, LIVE = 11, 10  # batch capacity / live items: item = (j / ntiles) * 8 + xcd covers both groups of 8 and a dead item
SENTINEL = -0x5A5B  # int16 bit pattern (bf16 -3.9e16) of what a kernel must leave alone

# kernel -> output tile th x tw, s2d halo tile hh x hw starting at s2d position (unit * output tile origin + off),
# staging budget in bytes, and S / out_div as the side of the output map
TILES = {
    "det": dict(th=8, tw=32, hh=10, hw=34, off=-1, unit=1, budget=8192, out_div=2),    # stem_fused_kernel<0, ..., 8, 32>
    "det2": dict(th=8, tw=16, hh=19, hw=35, off=-2, unit=2, budget=12288, out_div=4),  # stem2_kernel<8, 16>
    "cls": dict(th=16, tw=16, hh=17, hw=17, off=-1, unit=1, budget=8192, out_div=2),   # stem_fused_kernel<1, ..., 16, 16>
    "ir": dict(th=16, tw=16, hh=19, hw=19, off=-2, unit=1, budget=8192, out_div=2),    # stem_ir_kernel<16>
}


def _rand(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def tie_for(S: int):
    """The tie image (tie_image.py) whose letterbox to S is a 10/3 downscale without padding; None where S is no
    multiple of 3 (10 S / 3 is then no integer; S = 64 and 32 are powers of two, where every scale is dyadic and
    no tie exists)."""
    if S % 3:
        return None
    src = S * 10 // 3
    _, nw, nh, pw, ph = letterbox_geometry(src, src, S)
    assert (nw, nh, pw, ph) == (S, S, 0, 0), (nw, nh, pw, ph)
    return ti.tie_image(src, src, S, S, 0, 3 if S <= 96 else 1)


@functools.lru_cache(maxsize=None)
def letterbox_groups(S: int) -> tuple[tuple[np.ndarray, ...], ...]:
    """Groups of LIVE images for a letterbox to S.  Widths cover 3 w % 4 in {0, 1, 2, 3}: the staged rows then start
    at all four byte alignments."""
    a = (
        _rand(S, S - 37, 1),           # unit scale, padding on x with an odd remainder
        _rand(S - 22, S, 2),           # unit scale, padding on y
        _rand(1, 1, 3),                # upscales: both taps clamp
        _rand(2, 3, 4),
        _rand(7, 5, 5),
        _rand(S + S // 5, S + 5, 6),   # mild downscale: staged
        _rand(3 * S + 12, 3 * S + 2, 7),   # strong downscale (factor > 3): over the staging budget
        _rand(S + S // 3, S + 3, 8),   # mild downscale, another row alignment
        _rand(9, 4 * S + 16, 9),       # long and thin
        _rand(4 * S + 16, 9, 10),
    )
    tie = tie_for(S)
    b = (
        tie if tie is not None else _rand(2 * S + 40, 2 * S + 41, 11),
        _rand(S // 2 + 2, S // 3 + 1, 12),   # upscales
        _rand(S // 3 + 1, S // 2 + 2, 13),
        _rand(S + 1, S - 1, 14),             # scale just below 1
        _rand(2 * S, 2 * S, 15),             # exactly 2: every weight 0.5
        _rand(2 * S + S // 2 + 10, S // 2 + 13, 16),
        _rand(S // 2 + 13, 2 * S + S // 2 + 10, 17),
        _rand(S, S, 18),                     # unit scale, no padding
        _rand(3, 1, 19),
        _rand(2 * S + 8, 2 * S + 11, 20),    # factor 2.1: over the budget of the detector tiles
    )
    for g in (a, b):
        assert len(g) == LIVE
        for im in g:
            im.setflags(write=False)
    assert {3 * im.shape[1] % 4 for im in a + b} == {0, 1, 2, 3}
    return a, b


@functools.lru_cache(maxsize=None)
def crop_images(S: int) -> tuple[np.ndarray, ...]:
    tie = tie_for(S)
    imgs = (_rand(S + 54, S + 35, 21), tie if tie is not None else _rand(2 * S + 9, 2 * S + 7, 22),
            _rand(2 * S + 26, 2 * S + 19, 23))
    for im in imgs:
        im.setflags(write=False)
    return imgs


CROP_BASE = 2  # records in front of the live ones (ctrl.crop_base)


@functools.lru_cache(maxsize=None)
def crops(S: int) -> tuple[tuple[int, int, int, int, int], ...]:
    """(image, x1, y1, x2, y2) of the LIVE crops, in front of them CROP_BASE records that must not be read as
    crops 0.. and behind them one that no live item reads."""
    im = crop_images(S)
    (h0, w0), (h1, w1), (h2, w2) = (i.shape[:2] for i in im)
    live = (
        (0, 0, 0, w0, h0),                    # the whole image
        (0, 17, 23, 18, 24),                  # 1 x 1
        (0, 30, 10, 30, 40),                  # empty: black
        (2, 5, 7, 5 + S, 7 + S),              # exactly S x S: unit scale
        (2, 3, 2, 3 + S + 1, 2 + S - 1),      # S + 1 by S - 1
        (0, 41, 0, 46, h0),                   # a 5-pixel-wide strip
        (0, w0 - 30, h0 - 27, w0, h0),        # ends on the image's right and bottom edge, odd x1
        (2, 0, 0, w2, h2),                    # factor > 2: over the staging budget
        (1, 0, 0, w1, h1),                    # the tie image (S a multiple of 3)
        (2, w2 - 44, 1, w2, 34),              # an upscale ending on the right edge, odd x1
    )
    assert len(live) == LIVE and (w0 - 30) % 2 == 1 and (w2 - 44) % 2 == 1
    return ((2, 1, 1, 9, 9), (0, 0, 0, 3, 3)) + live + ((0, 2, 2, 20, 20),)


def pack_crops(S: int) -> np.ndarray:
    """int32 [n, 8] CropRef records (img, x1, y1, x2, y2, det, pad, pad)."""
    c = crops(S)
    out = np.zeros((len(c), 8), np.int32)
    out[:, :5] = np.asarray(c, np.int32)
    return out


# ------------------------------------------------------------------ which tiles are staged
def _taps(dst, src):
    i0, i1, _ = _lin_taps(dst, src)
    return i0, i1


def tile_kinds(kernel: str, S: int, *, image=None, crop=None) -> list[str]:
    """Per tile of one item: "staged" (source rows copied to LDS), "global" (region over the budget: taps read
    global memory) or "none" (nothing to sample: padding only, or an empty crop) — the rule of build_s2d_tile.
    ``image``: (h, w) letterboxed to S; ``crop``: (cw, ch) resized to S x S."""
    t = TILES[kernel]
    if image is not None:
        h, w = image
        _, nw, nh, pw, ph = letterbox_geometry(h, w, S)
        lim_y, lim_x, rh, rw, empty = nh, nw, h, w, False
    else:
        cw, ch = crop
        pw = ph = 0
        lim_y = lim_x = S
        rh, rw, empty = ch, cw, cw <= 0 or ch <= 0
    out_side = S // t["out_div"]
    kinds = []
    if not empty:
        (y0, y1), (x0, x1) = _taps(lim_y, rh), _taps(lim_x, rw)
    for ty in range(-(-out_side // t["th"])):
        for tx in range(-(-out_side // t["tw"])):
            sY0, sX0 = t["unit"] * ty * t["th"] + t["off"], t["unit"] * tx * t["tw"] + t["off"]
            sy_lo, sy_hi = max(2 * sY0 - ph, 0), min(2 * (sY0 + t["hh"] - 1) + 1 - ph, lim_y - 1)
            sx_lo, sx_hi = max(2 * sX0 - pw, 0), min(2 * (sX0 + t["hw"] - 1) + 1 - pw, lim_x - 1)
            if empty or sy_lo > sy_hi or sx_lo > sx_hi:
                kinds.append("none")
                continue
            nrows = int(y1[sy_hi] - y0[sy_lo] + 1)
            rbytes = int(x1[sx_hi] - x0[sx_lo] + 1) * 3
            pitch = ((rbytes + 3 + 3) >> 2) * 4
            kinds.append("staged" if nrows * pitch <= t["budget"] else "global")
    return kinds


# ------------------------------------------------------------------ selectors
def selector(cout: int, ks: int, picks) -> torch.Tensor:
    """[cout, 16, ks, ks] weights with one 1.0 per row: ``picks[o]`` = (tap, channel) that output o copies."""
    w = torch.zeros(cout, 16, ks, ks)
    for o, (tap, c) in enumerate(picks):
        w[o, c, tap // ks, tap % ks] = 1.0
    return w


def shifted(x: torch.Tensor, dy: int, dx: int, stride: int = 1, out: int | None = None) -> torch.Tensor:
    """y[b, Y, X] = x[b, stride * Y + dy, stride * X + dx], zero outside x (a conv's zero padding); [B, H, W, C]
    -> [B, out, out, C] (out: H by default)."""
    B, H, W, C = x.shape
    n = out or H
    pad = torch.zeros(B, H + 2 * 4, W + 2 * 4, C, dtype=x.dtype)
    pad[:, 4:4 + H, 4:4 + W] = x
    ys = 4 + dy + stride * torch.arange(n)
    xs = 4 + dx + stride * torch.arange(n)
    assert ys.min() >= 0 and xs.min() >= 0 and ys.max() < H + 8 and xs.max() < W + 8
    return pad[:, ys][:, :, xs]
