"""EXIF orientation on the GPU: the oriented colour kernel (csrc/kernels/jpeg_idct.hip), the executor's JPEG input
path and the native front end over the GPU engine.

The kernel's tile side is 64 (kTile), so the sizes below reach: a single block, partial MCUs, the narrowest
chroma, more than one tile with a remainder each way (65x65), the aligned store form after transposition (128x64),
aligned loads with byte stores (64x67), W % 4 == 0 with H % 4 != 0 and the reverse, and a batch whose grid is
smaller than its tile count (the tile loop's stride)."""
from __future__ import annotations

import io
import json

import numpy as np
import pytest
from PIL import Image

import exif_cases as X
from inference_arena_amd.ops import native

pytestmark = pytest.mark.gpu

T = 64
COMMON = [(T + 1, T + 1), (2 * T, T), (T, T + 3), (40, 30), (30, 40)]  # (w, h)
OWN = {"gray": [(8, 8)], "444": [(17, 9)], "420": [(6, 6)], "422": [(35, 18)]}
HOWS = ["pil", "le", "le_far"]


def _check(C, cases):
    """cases: (upload, orientation).  One guarded device decode of the whole list against the host reference and
    the rearranged PIL decode."""
    got = C.jpeg_decode_device([u for u, _ in cases], 0, guard=True)
    assert len(got) == len(cases)
    for i, ((data, o), rgb) in enumerate(zip(cases, got)):
        st, err, host = C.jpeg_decode_host(data)
        assert st == "ok", err
        want = X.expected(X.unrotated(data), o)
        assert rgb.shape == want.shape, (i, o, rgb.shape, want.shape)
        np.testing.assert_array_equal(rgb, host, err_msg=f"upload {i} orientation {o}: device vs host reference")
        np.testing.assert_array_equal(rgb, want, err_msg=f"upload {i} orientation {o}: device vs PIL")


@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_oriented_reconstruction_is_bit_exact(device, layout):
    C = native()
    cases = []
    for k, (w, h) in enumerate(OWN[layout] + COMMON):
        arr = X.scene(h, w, seed=k)
        for o in range(1, 9):
            # tagged and untagged images of different sizes interleaved in one call
            cases.append((X.tagged(arr, layout, o, HOWS[(o + k) % 3]), o) if o > 1 else (X.encode(arr, layout), 1))
    assert sum(o == 1 for _, o in cases) == len(OWN[layout] + COMMON)
    _check(C, cases)
    # a grid of one workgroup over three tiles, in both directions
    _check(C, [(X.tagged(X.scene(5, 2 * T + 1, 7), layout if layout != "420" else "444", 6, "le"), 6),
               (X.tagged(X.scene(2 * T + 1, 5, 8), layout if layout != "420" else "444", 8, "pil"), 8)])
    # an untagged batch alone still takes the plain kernels and equals PIL
    _check(C, [(X.encode(X.scene(h, w, 9), layout), 1) for w, h in COMMON[:2]])


@pytest.fixture(scope="module")
def fp32_pipe():
    import torch

    from inference_arena_amd.engine.pipeline import GpuPipeline
    from inference_arena_amd.models.zoo import make_mobilenet, make_yolo

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return GpuPipeline(make_yolo(0, cls_shift=-20.0), make_mobilenet(1), device=0, buckets=[1, 4], dtype="fp32")


def _tagged_frames():
    from inference_arena_amd.data.synthetic import synthetic_images

    imgs = synthetic_images(3, 31) + synthetic_images(1, 32, hw=(333, 500))
    out = []
    for i, (im, o) in enumerate(zip(imgs, [6, 8, 3, 5])):
        data = X.tagged(im, X.LAYOUTS[1 + i % 3], o, HOWS[i % 3])
        out.append((data, X.expected(X.unrotated(data), o)))
    return out


def test_executor_tagged_uploads_match_upright_pixels(fp32_pipe):
    """Executor.run of tagged uploads == Executor.run of the expected upright pixel arrays, also in a batch that
    mixes tagged, untagged and pixel inputs."""
    cases = _tagged_frames()
    plain = X.encode(cases[0][1], "420")
    ex = fp32_pipe.ex
    a = ex.run([u for u, _ in cases])
    b = ex.run([w for _, w in cases])
    mixed = ex.run([cases[1][0], plain, cases[2][1], cases[3][0]])
    ref = ex.run([cases[1][1], X.unrotated(plain), cases[2][1], cases[3][1]])
    for x, y in ((a, b), (mixed, ref)):
        assert list(x["det_count"]) == list(y["det_count"])
        for k in ("det", "topk_idx", "topk_logit"):
            np.testing.assert_array_equal(np.asarray(x[k]), np.asarray(y[k]), err_msg=k)
    assert sum(b["det_count"]) > 0


def test_native_front_tagged_jpeg_matches_png_of_upright_pixels(fp32_pipe):
    import http.client

    from inference_arena_amd.labels import load_labels
    from inference_arena_amd.server.native_front import NativeFrontEnd

    C = native()
    bnd = "b0undary"

    def post(port, data):
        body = (f"--{bnd}\r\nContent-Disposition: form-data; name=\"file\"; filename=\"x\"\r\n"
                f"Content-Type: application/octet-stream\r\n\r\n").encode() + data + f"\r\n--{bnd}--\r\n".encode()
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        c.request("POST", "/predict", body=body, headers={"Content-Type": f"multipart/form-data; boundary={bnd}"})
        r = c.getresponse()
        out = (r.status, json.loads(r.read()))
        c.close()
        return out

    batcher = C.DynamicBatcher([fp32_pipe.ex], {"max_batch": 4, "max_queue_delay_us": 200})
    fe = NativeFrontEnd(batcher, load_labels(None), port=0, host="127.0.0.1", io_threads=2, decode_procs=1, slots=8,
                        decode_threads=2)
    try:
        n_det = 0
        for data, want in _tagged_frames():
            png = io.BytesIO()
            Image.fromarray(want).save(png, "PNG")
            (s1, d1), (s2, d2) = post(fe.port, data), post(fe.port, png.getvalue())
            assert s1 == s2 == 200, (d1, d2)
            strip = [(d["detection"], d["classification"]) for d in d1["detections"]]
            assert strip == [(d["detection"], d["classification"]) for d in d2["detections"]]
            n_det += len(strip)
        st = fe.stats()
        assert st["oriented_decoded"] == 4 and st["native_decoded"] == 4 and st["fallback_decoded"] == 4, st
        assert n_det > 0
    finally:
        fe.close()
        batcher.shutdown()
