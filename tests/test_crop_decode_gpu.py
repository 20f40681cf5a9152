"""``ARENA_CROP_DECODE=gpu`` on the GPU: the ragged launch of the JPEG reconstruction kernels
(csrc/kernels/jpeg_idct.hip jpeg_idct_ragged_kernel / jpeg_color_ragged_kernel) and arm B's JPEG crops through
them in the classifier program and the classification service.

The reference decodes each crop with PIL (architectures/microservices/classification/app/servicer.py:65-76), so
the pixels must be PIL's bit for bit, and the classifier's answers those of the PIL-decoded crop.  CPU half
(routing, setting, launch plan): test_crop_decode.py."""
from __future__ import annotations

import asyncio
import io

import numpy as np
import pytest
from PIL import Image

from inference_arena_amd.ops import native
from inference_arena_amd.server.crop_codec import decode_crop, encode_crop

pytestmark = pytest.mark.gpu

# (h, w): a 1-pixel row, one block, MCU edges in both directions, several block groups / quad units per image
SIZES = [(1, 5), (8, 8), (9, 7), (16, 16), (17, 33), (37, 53), (130, 97), (250, 180)]


def _scene(h, w, seed=0):
    """Gradients + blobs + noise: every DCT band populated."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([x / max(w, 1) * 200, y / max(h, 1) * 180, (x + y) / max(h + w, 1) * 150], -1)
    for _ in range(6):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(3, max(4, min(h, w) / 3))
        img += (((y - cy) ** 2 + (x - cx) ** 2) < r * r)[..., None] * rng.uniform(-90, 90, 3)
    img += rng.normal(0, 12, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def _jpeg(arr, **kw) -> bytes:
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "JPEG", **{"quality": 95, **kw})
    return b.getvalue()


def _pil(data: bytes) -> np.ndarray:
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


@pytest.fixture(scope="module")
def crop_batch():
    """The q95 batch (largest image last) with its references, computed once: [(bytes, host decode, PIL decode)]."""
    C = native()
    batch = [_jpeg(_scene(h, w, 10 * s + i), subsampling=s) for s in (0, 1, 2) for i, (h, w) in enumerate(SIZES)]
    batch.append(_jpeg(np.asarray(Image.fromarray(_scene(9, 9, 99)).convert("L"))))
    out = []
    for data in batch:
        st, err, host = C.jpeg_decode_host(data)
        assert st == "ok", err
        out.append((data, host, _pil(data)))
    out.sort(key=lambda t: t[1].size)  # stable: ascending, so the largest image is last
    return out


def _check(items, compact):
    C = native()
    data = [d for d, _, _ in items]
    ragged = C.jpeg_decode_device(data, 0, guard=True, compact=compact, ragged=True)  # raises on a touched guard byte
    rect = C.jpeg_decode_device(data, 0, guard=True, compact=compact, ragged=False)
    assert len(ragged) == len(items)
    for i, ((_, host, pil), a, b) in enumerate(zip(items, ragged, rect)):
        np.testing.assert_array_equal(a, host, err_msg=f"image {i}: ragged vs host reference")
        np.testing.assert_array_equal(a, pil, err_msg=f"image {i}: ragged vs PIL")
        np.testing.assert_array_equal(a, b, err_msg=f"image {i}: ragged vs rectangular launch")


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("order", ["largest_first", "largest_last", "shuffled"])
def test_ragged_reconstruction_is_bit_exact(device, crop_batch, order, compact):
    """All SIZES decode ``ok`` on the host path at 4:4:4, 4:2:2 and 4:2:0 (the fixture asserts it), so none was
    replaced.  25 images per batch: 1 to 69 IDCT units and 1 to 44 colour units per image."""
    items = list(crop_batch)
    if order == "largest_first":
        items.reverse()
    elif order == "shuffled":
        items = [items[i] for i in np.random.default_rng(7).permutation(len(items))]
    _check(items, compact)


@pytest.mark.parametrize("compact", [False, True])
def test_ragged_batch_of_one_and_of_33_single_mcu_crops(device, crop_batch, compact):
    C = native()
    _check([crop_batch[-1]], compact)  # one image: the rectangular grid
    _check([crop_batch[0]], compact)  # ... and one unit in all
    tiny = [_jpeg(_scene(8, 8, i), subsampling=0) for i in range(33)]  # one unit per image, 33 images
    _check([(d, C.jpeg_decode_host(d)[2], _pil(d)) for d in tiny], compact)


def test_ragged_refuses_oriented_uploads(device):
    """No oriented ragged kernel: the binding says so instead of writing unrotated pixels (the executor keeps the
    rectangular pair for such a batch)."""
    import struct

    C = native()
    data = _jpeg(_scene(16, 24))
    tiff = b"II*\x00\x08\x00\x00\x00" + struct.pack("<H", 1) + struct.pack("<HHII", 0x0112, 3, 1, 6) + b"\0\0\0\0"
    app1 = b"Exif\x00\x00" + tiff
    tagged = data[:2] + b"\xff\xe1" + struct.pack(">H", len(app1) + 2) + app1 + data[2:]
    assert C.jpeg_coefs(tagged)["orientation"] == 6
    with pytest.raises(ValueError):
        C.jpeg_decode_device([tagged], 0, ragged=True)


# ---- classifier program -------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def ragged_classifier():
    import torch

    from inference_arena_amd.engine.pipeline import GpuClassifier
    from inference_arena_amd.models.zoo import make_mobilenet
    from inference_arena_amd.server.batching import AsyncBatcher

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    # one bucket: a crop's answer does not depend on how the batcher happened to group the requests
    runner = GpuClassifier(make_mobilenet(1), device=0, buckets=[8], jpeg_ragged=True)
    assert runner.ex.jpeg_ragged
    b = AsyncBatcher([runner], max_batch=8, max_queue_delay_us=2000)
    yield b
    b.close()


def _crop_bytes():
    """Five JPEG crops of one frame: from encode_crop and (same boxes) from the GPU crop encoder."""
    from inference_arena_amd.data.curator import workload_images

    C = native()
    frame = np.ascontiguousarray(workload_images(1)[0])
    H, W = frame.shape[:2]
    boxes = [(3, 5, 67, 101), (40, 30, 41 + 9, 30 + 7), (0, 0, min(W, 300), min(H, 200)), (100, 90, 133, 107),
             (W - 120, H - 90, W, H)]
    pil = [encode_crop(frame[y1:y2, x1:x2], "jpeg") for x1, y1, x2, y2 in boxes]
    gpu = list(C.jpeg_encode_device(frame, [tuple(map(float, b)) for b in boxes])) if hasattr(C, "jpeg_encode_device") else []
    return pil, gpu


def _same(a: dict, b: dict):
    for k in ("topk_idx", "topk_logit", "topk_prob"):
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)


def test_classifier_on_jpeg_crops_matches_decoded_pixels(ragged_classifier):
    b = ragged_classifier
    pil, gpu = _crop_bytes()

    async def decode(data):
        raise AssertionError("a baseline 4:2:0 crop must not fall back")

    async def go(crops):
        got = await asyncio.gather(*(b.run_jpeg(c, decode) for c in crops))
        ref = await asyncio.gather(*(b.run(decode_crop(c)) for c in crops))
        return got, ref

    for source in (pil, gpu):
        for n in (1, 3, 5):
            got, ref = asyncio.run(go(source[:n]))
            assert len(got) == min(n, len(source))
            for x, y in zip(got, ref):
                _same(x, y)
    # the answers tell crops apart (the comparison is not of constants)
    got, _ = asyncio.run(go(pil))
    assert len({tuple(np.asarray(g["topk_logit"]).ravel().tolist()) for g in got}) > 1
    st = b.ingest_stats()
    assert st["fallback"] == 0 and st["errors"] == 0 and st["native"] >= 5


def test_classifier_on_a_batch_mixing_jpeg_and_raw_crops(ragged_classifier):
    b = ragged_classifier
    pil, _ = _crop_bytes()
    raw = decode_crop(pil[2])

    async def decode(data):
        raise AssertionError("a baseline 4:2:0 crop must not fall back")

    async def go():
        got = await asyncio.gather(b.run_jpeg(pil[0], decode), b.run(raw), b.run_jpeg(pil[1], decode))
        ref = await asyncio.gather(b.run(decode_crop(pil[0])), b.run(raw), b.run(decode_crop(pil[1])))
        return got, ref

    got, ref = asyncio.run(go())
    for x, y in zip(got, ref):
        _same(x, y)


# ---- service --------------------------------------------------------------------------------------------------------


def test_service_answers_are_those_of_the_pil_path(device, monkeypatch):
    """start_server with ARENA_CROP_DECODE=gpu and with pil, the same crops one after the other (so every batch is
    one crop in both runs): four JPEG, one PNG, one truncated JPEG — and a progressive JPEG.  The PNG does not start
    with FF D8, so the servicer keeps it on the thread-pool PIL path and the ingest never sees it; the progressive
    crop is the one the split decoder hands back (the switch is off), which makes the ingest's counters 4 native,
    1 fallback, 1 error."""
    from inference_arena_amd.data.curator import workload_images
    from inference_arena_amd.proto import inference_api as pb
    from inference_arena_amd.server.classification_service import start_server
    from inference_arena_amd.server.service_backends import CROP_DECODE_RAGGED
    from inference_arena_amd.utils.settings import Settings

    monkeypatch.setenv("ARENA_CLS_MAX_BATCH", "8")  # four buckets to capture instead of eight
    frame = workload_images(1)[0]
    crops = [frame[10:100, 20:140], frame[50:58, 60:68], frame[0:201, 0:133], frame[200:233, 300:317]]
    jpegs = [encode_crop(c, "jpeg") for c in crops]
    blobs = jpegs + [encode_crop(frame[30:90, 40:100], "png"), jpegs[0][: len(jpegs[0]) // 2],
                     _jpeg(np.ascontiguousarray(frame[60:150, 80:170]), progressive=True)]
    good = [0, 1, 2, 3, 4, 6]

    async def go(mode):
        s = Settings(LOG_LEVEL="WARNING", HOST="127.0.0.1", ARENA_CROP_DECODE=mode)
        server, servicer, _ = await start_server(s, port=0)
        try:
            out = [await servicer.Classify(pb.ClassificationRequest(request_id=str(i), image_crop=d))
                   for i, d in enumerate(blobs)]
            return out, servicer.backend.stats(), [r.ex.jpeg_ragged for r in servicer.backend.runners]
        finally:
            await server.stop(0)
            servicer.backend.close()
            servicer.close()

    gpu, gst, gflags = asyncio.run(go("gpu"))
    pil, pst, pflags = asyncio.run(go("pil"))
    assert gflags == [CROP_DECODE_RAGGED] and pflags == [False]
    for a, b in ((gpu[i], pil[i]) for i in good):
        assert a.error == "" and b.error == ""
        assert [t.class_id for t in a.top_k] == [t.class_id for t in b.top_k]
        assert [t.confidence for t in a.top_k] == [t.confidence for t in b.top_k]
    assert gpu[5].error and pil[5].error
    ing = gst["ingest"]
    assert (ing["native"], ing["fallback"], ing["errors"]) == (4, 1, 1)
    assert "ingest" not in pst
