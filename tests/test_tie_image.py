"""The tie image (tests/tie_image.py) on the CPU: it is made of rounding ties of the host resize, and arithmetic
with fused multiply-adds visibly differs from the host on it."""
from __future__ import annotations

import numpy as np
import pytest

import tie_image as ti
from inference_arena_amd.processing.transforms import letterbox, letterbox_geometry, resize_bilinear

GEOMETRIES = [(160, 160, 48, 48), (320, 320, 96, 96)]  # scale 10/3 on both axes: the images the GPU tests use


@pytest.mark.parametrize("sh,sw,dh,dw", GEOMETRIES)
def test_tie_image_is_made_of_ties(sh, sw, dh, dw):
    """At least a tenth of the resized samples are ties: the host value (fp32, separately rounded operations)
    differs from floor(x + 0.5) of the exact value of the same expression in float64.  Measured: 30.1 % of the
    6,912 samples at 160 -> 48 and 14.9 % of the 27,648 at 320 -> 96 (the fp32 error of the tap weights grows with
    the coordinate, and with it the distance of the block's exact value from k + 0.5)."""
    img = ti.tie_image(sh, sw, dh, dw)
    assert img.dtype == np.uint8 and img.shape == (sh, sw, 3) and not img.flags.writeable
    assert np.array_equal(img, ti.tie_image.__wrapped__(sh, sw, dh, dw))  # deterministic
    host = resize_bilinear(img, dw, dh)
    share = float(np.mean(host != ti.resize_exact(img, dw, dh)))
    print(f"tie share {sh}x{sw} -> {dh}x{dw}: {share:.4f}")
    assert share >= 0.1, share
    # a random image of the same size has none to speak of
    rnd = np.random.default_rng(0).integers(0, 256, (sh, sw, 3)).astype(np.uint8)
    assert np.mean(resize_bilinear(rnd, dw, dh) != ti.resize_exact(rnd, dw, dh)) < 1e-3


@pytest.mark.parametrize("sh,sw,dh,dw", GEOMETRIES)
def test_tie_image_has_teeth(sh, sw, dh, dw):
    """The emulation with the tap coordinate and the three lerps fused (what a kernel computes without the
    ``fp contract(off)`` of csrc/kernels/letterbox.h) differs from the host on the image, by one grey level.
    Measured share of differing samples: 1.56 % at 160 -> 48 (108 samples), 0.67 % at 320 -> 96 (185 samples); on a
    random image of the same size: none.  Fusing the lerps alone, or the coordinate alone, differs too."""
    img = ti.tie_image(sh, sw, dh, dw)
    host = resize_bilinear(img, dw, dh)
    fused = ti.resize_fused(img, dw, dh)
    diff = np.abs(fused.astype(np.int64) - host)
    share = float(np.mean(diff != 0))
    print(f"fused != host {sh}x{sw} -> {dh}x{dw}: {share:.4f} ({int((diff != 0).sum())} samples)")
    assert diff.max() == 1 and (diff != 0).sum() >= 50, (diff.max(), int((diff != 0).sum()))
    # the lerps alone (host taps)
    y0, y1, fy = ti._lin_taps(dh, sh)
    x0, x1, fx = ti._lin_taps(dw, sw)
    f = img.astype(np.float32)
    lerp = ti.fused_tuple(f[y0][:, x0], f[y0][:, x1], f[y1][:, x0], f[y1][:, x1], fx[None, :, None],
                          fy[:, None, None])
    assert (lerp != host).sum() >= 20
    # the host arithmetic written tuple-wise is the host resize: the generator searched the right function
    tup = ti.host_tuple(f[y0][:, x0], f[y0][:, x1], f[y1][:, x0], f[y1][:, x1], fx[None, :, None], fy[:, None, None])
    assert np.array_equal(tup.astype(np.uint8), host)


def test_tie_image_through_letterbox():
    """letterbox_geometry(320, 320, 96) resizes to 96 x 96 (no padding), so the letterboxed tie image is its resize;
    a geometry the generator cannot serve raises."""
    scale, nw, nh, pw, ph = letterbox_geometry(320, 320, 96)
    assert (nw, nh, pw, ph) == (96, 96, 0, 0)
    img = ti.tie_image(320, 320, 96, 96)
    assert np.array_equal(letterbox(img, 96)[0], resize_bilinear(img, 96, 96))
    with pytest.raises(ValueError, match="downscale"):
        ti.tie_image(100, 100, 96, 96)
