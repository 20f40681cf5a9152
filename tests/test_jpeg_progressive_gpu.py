"""Progressive (SOF2) uploads through the device half of the split JPEG decoder (csrc/kernels/jpeg_idct.hip).

The kernels are the baseline path's: a progressive file has the frame geometry they already take, and its
coefficients arrive in the same dense or compact form.  What is new is the producer (the scan-by-scan entropy decode
of csrc/runtime/jpeg_decode.cpp), so these tests prove that its payloads drive the kernels to PIL's pixels:

* the reconstruction kernels on dense and compact payloads against the host reference and PIL, a baseline file in
  the same call;
* the executor's JPEG input path on a batch that mixes progressive, baseline and raw-pixel inputs;
* the native HTTP front end with the switch on (split decoder) against every upload through the PIL processes, and
  with the switch off (today's behaviour: all to the PIL pool).
"""
from __future__ import annotations

import io
import json

import numpy as np
import pytest
from PIL import Image

from inference_arena_amd.ops import native

pytestmark = pytest.mark.gpu


def _enc(arr, **kw) -> bytes:
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "JPEG", **kw)
    return b.getvalue()


def _pil(data: bytes) -> np.ndarray:
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def _frames():
    from inference_arena_amd.data.synthetic import synthetic_images

    imgs = synthetic_images(6, 31) + synthetic_images(2, 32, hw=(333, 500)) + synthetic_images(2, 33, hw=(640, 427))
    rng = np.random.default_rng(5)
    imgs.append((rng.random((37, 53, 3)) * 255).astype(np.uint8))
    imgs.append((rng.random((41, 66, 3)) * 255).astype(np.uint8))  # width 2 mod 4 (the colour kernel's quads)
    return imgs


def _small(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([x / w * 200, y / h * 180, (x + y) / (h + w) * 150], -1) + rng.normal(0, 25, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("subsampling", [0, 1, 2])
def test_device_reconstruction_is_bit_exact(device, subsampling, compact):
    C = native()
    sizes = [(9, 7), (13, 17), (16, 16), (37, 53), (41, 66)]  # the last: the colour kernel's width 2 mod 4
    frames = [_small(h, w, i) for i, (h, w) in enumerate(sizes)]
    uploads = [_enc(f, quality=q, subsampling=subsampling, progressive=True) for f in frames for q in (50, 90, 100)]
    uploads.append(_enc(np.asarray(Image.fromarray(frames[3]).convert("L")), quality=90, progressive=True))
    uploads.append(_enc(frames[4], quality=85, subsampling=subsampling, progressive=True, restart_marker_blocks=3))
    exif = Image.Exif()
    exif[0x0112] = 6
    uploads.append(_enc(frames[3], quality=90, subsampling=subsampling, progressive=True, exif=exif.tobytes()))
    n_prog = len(uploads)
    uploads.append(_enc(frames[3], quality=90, subsampling=subsampling))  # a baseline file in the same call
    assert all((b"\xff\xc2" in u) == (i < n_prog) for i, u in enumerate(uploads))
    got = C.jpeg_decode_device(uploads, 0, guard=True, progressive=True, compact=compact)
    for i, (data, rgb) in enumerate(zip(uploads, got)):
        st, err, host = C.jpeg_decode_host(data, progressive=True)
        assert st == "ok", err
        np.testing.assert_array_equal(rgb, host, err_msg=f"upload {i}: device vs host reference")
        want = _pil(data)
        if i == n_prog - 1:  # orientation 6: PIL's convert() leaves the stored frame
            want = np.rot90(want, -1)
        np.testing.assert_array_equal(rgb, want, err_msg=f"upload {i}: device vs PIL")
    with pytest.raises(ValueError):  # the control: without the switch the progressive uploads are not taken
        C.jpeg_decode_device(uploads[:1], 0)


@pytest.fixture(scope="module")
def fp32_pipe():
    import torch

    from inference_arena_amd.engine.pipeline import GpuPipeline
    from inference_arena_amd.models.zoo import make_mobilenet, make_yolo

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return GpuPipeline(make_yolo(0, cls_shift=-20.0), make_mobilenet(1), device=0, buckets=[1, 8], dtype="fp32")


def test_executor_takes_mixed_progressive_baseline_and_pixel_inputs(fp32_pipe):
    """Executor.run on encoded bytes follows the process default of the switch."""
    C = native()
    imgs = _frames()
    # frames 7, 9 and 11 are the ones this detector finds something in
    prog = [_enc(imgs[7], quality=90, progressive=True), _enc(imgs[9], quality=90, progressive=True)]
    base = _enc(imgs[11], quality=90)
    ex = fp32_pipe.ex
    with pytest.raises(ValueError):  # the control: off by default
        ex.run([prog[0]])
    before = C.set_jpeg_progressive_default(True)
    try:
        assert C.jpeg_progressive_default()
        got = ex.run([prog[0], base, imgs[2], prog[1]])
    finally:
        C.set_jpeg_progressive_default(before)
    assert not C.jpeg_progressive_default()
    ref = ex.run([_pil(prog[0]), _pil(base), imgs[2], _pil(prog[1])])
    assert list(got["det_count"]) == list(ref["det_count"])
    for k in ("det", "topk_idx", "topk_logit"):
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(ref[k]), err_msg=k)
    assert sum(ref["det_count"]) > 0  # the comparison saw detections and crops


def test_native_front_takes_progressive_uploads_when_switched_on(fp32_pipe):
    import http.client

    from inference_arena_amd.labels import load_labels
    from inference_arena_amd.server.native_front import NativeFrontEnd

    C = native()
    frames = _frames()
    # three frames the detector finds something in (7, 9, 11: 7 detections in all) and three it does not
    uploads = [_enc(frames[i], quality=90, progressive=True) for i in (7, 9, 11, 0, 1, 10)]
    bnd = "b0undary"

    def post(port, data):
        body = (f"--{bnd}\r\nContent-Disposition: form-data; name=\"file\"; filename=\"x.jpg\"\r\n"
                f"Content-Type: image/jpeg\r\n\r\n").encode() + data + f"\r\n--{bnd}--\r\n".encode()
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        c.request("POST", "/predict", body=body, headers={"Content-Type": f"multipart/form-data; boundary={bnd}"})
        r = c.getresponse()
        out = (r.status, json.loads(r.read()))
        c.close()
        return out

    answers = {}
    # split decoder with the switch on / with it off / no decode threads at all (every upload to the PIL processes)
    for name, threads, progressive in (("on", 4, True), ("off", 4, False), ("pil", 0, True)):
        batcher = C.DynamicBatcher([fp32_pipe.ex], {"max_batch": 8, "max_queue_delay_us": 200})
        fe = NativeFrontEnd(batcher, load_labels(None), port=0, host="127.0.0.1", io_threads=2, decode_procs=2,
                            slots=16, decode_threads=threads, progressive=progressive)
        try:
            answers[name] = [post(fe.port, u) for u in uploads]
            st = fe.stats()
            on = name == "on"
            assert st["native_decoded"] == (6 if on else 0)
            assert st["progressive_decoded"] == (6 if on else 0)
            assert st["fallback_decoded"] == (0 if on else 6)
        finally:
            fe.close()
            batcher.shutdown()
    n_det = 0
    for a, b, c in zip(answers["on"], answers["pil"], answers["off"]):
        assert a[0] == b[0] == c[0] == 200
        strip = [(d["detection"], d["classification"]) for d in a[1]["detections"]]
        assert strip == [(d["detection"], d["classification"]) for d in b[1]["detections"]]
        assert strip == [(d["detection"], d["classification"]) for d in c[1]["detections"]]
        n_det += len(strip)
    assert n_det >= 3
