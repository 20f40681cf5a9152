"""4:4:0, 4:1:1 and the other integral chroma ratios, RGB-coded files and multi-scan sequential files through the
device half of the split JPEG decoder (csrc/kernels/jpeg_idct.hip) on the GPU.

* the reconstruction kernels (color_quad's h1v2, box and identity branches in the oriented and the ragged colour
  kernel) against the host reference and against PIL, bit for bit, between guard bytes, over every file of
  jpeg_layout_cases.cases() in one batch: dense, compact and ragged;
* the eight EXIF orientations of 4:4:0 and 4:1:1 files in a batch with a plain 4:2:0 upload;
* the executor's JPEG input path and the native front end on such uploads against the same pixels submitted decoded.
"""
from __future__ import annotations

import io
import json

import numpy as np
import pytest
from PIL import Image

import exif_cases as X
import jpeg_layout_cases as L
from inference_arena_amd.ops import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference():
    """(name, bytes, host reference == PIL pixels) of every case, computed once."""
    C = native()
    out = []
    for name, data in L.cases():
        st, err, host = C.jpeg_decode_host(data)
        assert st == "ok", (name, err)
        np.testing.assert_array_equal(host, L.pil(data), err_msg=name)
        host.setflags(write=False)
        out.append((name, data, host))
    return out


@pytest.mark.parametrize("mode", ["dense", "compact", "ragged", "ragged_compact"])
def test_device_reconstruction_is_bit_exact(device, reference, mode):
    C = native()
    got = C.jpeg_decode_device([d for _, d, _ in reference], 0, guard=True, compact="compact" in mode,
                               ragged="ragged" in mode)
    assert len(got) == len(reference)
    for (name, _, want), rgb in zip(reference, got):
        np.testing.assert_array_equal(rgb, want, err_msg=f"{name} ({mode}): device vs host reference and PIL")


def test_todays_layouts_alone_and_mixed_with_a_new_one(device):
    """A batch of 4:4:4 / 4:2:2 / 4:2:0 / grey files takes the plain kernels; one 4:1:1 file among them moves the
    batch to the general colour kernel: the same pixels either way."""
    C = native()
    plain = [X.encode(X.scene(40 + 3 * i, 61 + 5 * i, i), lay) for i, lay in enumerate(X.LAYOUTS)]
    new = dict(L.cases())["411_37x53"]
    want = [X.unrotated(u) for u in plain]
    for batch, exp in ((plain, want), (plain[:2] + [new] + plain[2:], want[:2] + [L.pil(new)] + want[2:])):
        for rgb, w in zip(C.jpeg_decode_device(batch, 0, guard=True), exp):
            np.testing.assert_array_equal(rgb, w)


@pytest.mark.parametrize("sampling", ["440", "411"])
def test_oriented_new_layouts_in_a_mixed_batch(device, sampling):
    C = native()
    batch = [(X.encode(X.scene(45, 70, 1), "420"), 1)]
    for k, (h, w) in enumerate([(37, 53), (70, 130), (131, 66), (9, 7)]):  # within one 64x64 tile and across tiles
        for o in range(1, 9):
            data = L.write(L.scene(h, w, 10 * k + o), L.SAMPLINGS[sampling][0])
            batch.append((X.splice(data, X.app1(o)) if o > 1 else data, o))
    got = C.jpeg_decode_device([u for u, _ in batch], 0, guard=True)
    for i, ((data, o), rgb) in enumerate(zip(batch, got)):
        st, err, host = C.jpeg_decode_host(data)
        assert st == "ok", err
        np.testing.assert_array_equal(rgb, host, err_msg=f"upload {i} orientation {o}: device vs host reference")
        np.testing.assert_array_equal(rgb, X.expected(X.unrotated(data), o), err_msg=f"upload {i} orientation {o}")


@pytest.fixture(scope="module")
def fp32_pipe():
    import torch

    from inference_arena_amd.engine.pipeline import GpuPipeline
    from inference_arena_amd.models.zoo import make_mobilenet, make_yolo

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return GpuPipeline(make_yolo(0, cls_shift=-20.0), make_mobilenet(1), device=0, buckets=[1, 4], dtype="fp32")


@pytest.fixture(scope="module")
def frames():
    """(upload, PIL's pixels): a PIL-written 4:2:0 file and a 4:4:0, a 4:1:1 and an RGB-coded file of the writer."""
    from inference_arena_amd.data.synthetic import synthetic_images

    # the two synthetic frames in which the seeded detector finds objects whatever the chroma resolution
    wide, tall = synthetic_images(2, 32, hw=(333, 500))[1], synthetic_images(2, 33, hw=(640, 427))[1]
    uploads = [X.encode(wide, "420"), L.write(L.ycc(tall), L.S440), L.write(L.ycc(wide), L.S411, restart=7),
               L.write(tall, L.S444, jfif=False, adobe=0)]
    return [(u, L.pil(u)) for u in uploads]


def test_executor_new_layout_uploads_match_decoded_pixels(fp32_pipe, frames):
    C = native()
    assert [C.jpeg_coefs(u)["layout"] for u, _ in frames] == [3, 4, 5, 1]
    ex = fp32_pipe.ex
    a = ex.run([u for u, _ in frames])
    b = ex.run([p for _, p in frames])
    assert list(a["det_count"]) == list(b["det_count"])
    for k in ("det", "topk_idx", "topk_logit"):
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
    assert min(b["det_count"]) > 0  # the comparison saw detections and crops in every layout


def test_native_front_counts_new_layouts_as_native(fp32_pipe, frames):
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

    scans = L.write(L.ycc(frames[1][1]), L.S420, scans=[[0], [1, 2]])
    uploads = frames + [(scans, L.pil(scans))]
    batcher = C.DynamicBatcher([fp32_pipe.ex], {"max_batch": 4, "max_queue_delay_us": 200})
    fe = NativeFrontEnd(batcher, load_labels(None), port=0, host="127.0.0.1", io_threads=2, decode_procs=1, slots=8,
                        decode_threads=2)
    try:
        n_det = 0
        for i, (data, want) in enumerate(uploads):
            (s1, d1) = post(fe.port, data)
            st = fe.stats()
            assert st["native_decoded"] == i + 1 and st["fallback_decoded"] == i, st  # the PNGs so far
            png = io.BytesIO()
            Image.fromarray(want).save(png, "PNG")
            (s2, d2) = post(fe.port, png.getvalue())
            assert s1 == s2 == 200, (d1, d2)
            strip = [(d["detection"], d["classification"]) for d in d1["detections"]]
            assert strip == [(d["detection"], d["classification"]) for d in d2["detections"]]
            n_det += len(strip)
        st = fe.stats()
        # the 4:2:0 single-scan upload is native but not counted among the new layouts
        assert st["native_decoded"] == 5 and st["layout_decoded"] == 4 and st["fallback_decoded"] == 5, st
        assert n_det > 0
    finally:
        fe.close()
        batcher.shutdown()
