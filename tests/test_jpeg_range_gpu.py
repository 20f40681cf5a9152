"""The coefficient range of the split JPEG decoder (kCoefRangeLimit, csrc/kernels/jpeg_math.h) on the GPU.

jpeg_range_cases.py writes files with crafted coefficients on both sides of the limit (test_jpeg_range.py checks the
lists themselves on CPU).  Here

* the int32 reconstruction kernels (csrc/kernels/jpeg_idct.hip) meet coefficients at and just under the limit their
  exactness is proved for, and the colour kernels all six clamps of ycc_to_rgb: device == host reference == PIL on
  every inside file, dense, compact, ragged and ragged compact;
* crafted files in one batch with natural and oriented uploads leave their neighbours' pixels alone, and the oriented
  colour kernel clamps like the plain one;
* outside files never reach a kernel: jpeg_decode_device and the executor refuse them, the native front end answers
  them through the PIL pool, with the answer of a front end that has no split decoder at all;
* the inside files among those uploads are decoded natively (test_jpeg_range.py holds the whole corpus to "ok")."""
from __future__ import annotations

import http.client
import json

import numpy as np
import pytest

import exif_cases as X
import jpeg_layout_cases as L
import jpeg_range_cases as R
from inference_arena_amd.ops import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference():
    """(name, bytes, host reference == PIL pixels) of every inside case, computed once."""
    C = native()
    out = []
    for c in R.inside():
        st, err, host = C.jpeg_decode_host(c.data)
        assert st == "ok", (c.name, err)
        np.testing.assert_array_equal(host, L.pil(c.data), err_msg=c.name)
        host.setflags(write=False)
        out.append((c.name, c.data, host))
    return out


@pytest.mark.parametrize("mode", ["dense", "compact", "ragged", "ragged_compact"])
def test_device_reconstruction_is_bit_exact_inside_the_range(device, reference, mode):
    C = native()
    got = C.jpeg_decode_device([d for _, d, _ in reference], 0, guard=True, compact="compact" in mode,
                               ragged="ragged" in mode)
    assert len(got) == len(reference)
    for (name, _, want), rgb in zip(reference, got):
        np.testing.assert_array_equal(rgb, want, err_msg=f"{name} ({mode}): device vs host reference and PIL")


@pytest.mark.parametrize("ragged", [False, True])
def test_crafted_files_in_a_mixed_batch_with_an_oriented_upload(device, reference, ragged):
    """Crafted files between natural uploads: in the ragged grid (which takes no oriented upload) a crafted block
    must not disturb its neighbours; in the rectangular launch one EXIF-6 upload moves the batch to the oriented
    colour kernel, and that upload is a clamp file, so that kernel meets the six clamps too."""
    C = native()
    by_name = {n: d for n, d, _ in reference}
    o = 1 if ragged else 6
    clamp = by_name["clamps_420"] if ragged else X.splice(by_name["clamps_420"], X.app1(o))
    batch = [(X.encode(X.scene(45, 70, 1), "420"), 1), (by_name["at_limit_pairs"], 1),
             (X.encode(X.scene(40, 61, 2), "444"), 1), (by_name["random_cols04_row_420_1"], 1), (clamp, o),
             (by_name["at_limit_single"], 1), (X.encode(X.scene(37, 53, 3), "422"), 1), (by_name["clamps_422"], 1),
             (by_name["random_dense_444_2"], 1), (L.write(L.scene(33, 17, 4), L.S440), 1)]
    got = C.jpeg_decode_device([u for u, _ in batch], 0, guard=True, ragged=ragged)
    for i, ((data, ori), rgb) in enumerate(zip(batch, got)):
        st, err, host = C.jpeg_decode_host(data)
        assert st == "ok", err
        np.testing.assert_array_equal(rgb, host, err_msg=f"upload {i}: device vs host reference")
        np.testing.assert_array_equal(rgb, X.expected(X.unrotated(data), ori), err_msg=f"upload {i} vs PIL")


@pytest.mark.parametrize("compact", [False, True])
def test_outside_files_never_reach_a_kernel(device, reference, compact):
    """jpeg_decode_device treats them as any upload whose host half says unsupported: it raises before it touches
    the device, whatever else is in the batch."""
    C = native()
    good = reference[0][1]
    for c in R.outside():
        with pytest.raises(ValueError, match="16-bit IDCT"):
            C.jpeg_decode_device([good, c.data], 0, guard=True, compact=compact)


@pytest.fixture(scope="module")
def fp32_pipe():
    import torch

    from inference_arena_amd.engine.pipeline import GpuPipeline
    from inference_arena_amd.models.zoo import make_mobilenet, make_yolo

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return GpuPipeline(make_yolo(0, cls_shift=-20.0), make_mobilenet(1), device=0, buckets=[1, 8], dtype="fp32")


def test_the_executor_refuses_outside_files(fp32_pipe):
    c = R.outside()[0]
    with pytest.raises(ValueError, match="16-bit IDCT"):
        fp32_pipe.ex.run([c.data])


def test_native_front_answers_outside_files_through_the_pil_pool(fp32_pipe):
    """/predict: every outside file is answered, counted in fallback_decoded and not in native_decoded, with the
    answer of a front end without decode threads; the inside files among them are all decoded natively."""
    from inference_arena_amd.data.synthetic import synthetic_images
    from inference_arena_amd.labels import load_labels
    from inference_arena_amd.server.native_front import NativeFrontEnd

    C = native()
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

    outside = [c.data for c in R.outside()]
    by_name = {c.name: c.data for c in R.inside()}
    inside = [by_name[k] for k in ("at_limit_pairs", "clamps_444", "random_sparse_420_0", "extreme_noise_q50_s2",
                                   "extreme_checker1_q100_s0")]
    # two natural frames in which the seeded detector finds objects: the comparison of answers below is not one of
    # empty lists only
    inside += [X.encode(synthetic_images(2, 32, hw=(333, 500))[1], "420"),
               X.encode(synthetic_images(2, 33, hw=(640, 427))[1], "444")]
    answers = {}
    for threads in (2, 0):
        batcher = C.DynamicBatcher([fp32_pipe.ex], {"max_batch": 8, "max_queue_delay_us": 200})
        fe = NativeFrontEnd(batcher, load_labels(None), port=0, host="127.0.0.1", io_threads=2, decode_procs=1,
                            slots=8, decode_threads=threads)
        try:
            answers[threads] = [post(fe.port, u) for u in outside + inside]
            st = fe.stats()
            assert st["native_decoded"] == (len(inside) if threads else 0), st
            assert st["fallback_decoded"] == (len(outside) if threads else len(outside) + len(inside)), st
        finally:
            fe.close()
            batcher.shutdown()
    n_det = 0
    for (s1, d1), (s2, d2) in zip(answers[2], answers[0]):
        assert s1 == s2 == 200, (d1, d2)
        strip = [(d["detection"], d["classification"]) for d in d1["detections"]]
        assert strip == [(d["detection"], d["classification"]) for d in d2["detections"]]
        n_det += len(strip)
    assert n_det > 0
