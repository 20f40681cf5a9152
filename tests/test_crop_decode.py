"""``ARENA_CROP_DECODE=gpu`` on CPU: arm B's JPEG crops through the split decoder in the classification service.

The reference decodes every crop with PIL inside ``Classify`` (architectures/microservices/classification/app/
servicer.py:65-76).  With the switch on, a JPEG crop goes as bytes to ``GpuClassifierBackend.classify_bytes``
(Huffman decode on C++ threads, pixels reconstructed on the GPU inside the classifier batch); everything else keeps
its path.  Checked here without a GPU: the routing of ``ClassificationServicer.Classify``, the setting,
``classify_bytes`` over a host-only instance (the pixels the instance receives are ``decode_crop``'s), and the
launch plan of the ragged reconstruction kernels (``_C.jpeg_ragged_plan``).  GPU half: test_crop_decode_gpu.py."""
from __future__ import annotations

import asyncio
import io
import threading
import types
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

from inference_arena_amd.ops import native
from inference_arena_amd.proto import inference_api as pb
from inference_arena_amd.server import classification_service as cs
from inference_arena_amd.server.crop_codec import decode_crop, encode_crop
from inference_arena_amd.server.service_backends import ClassifierBackend, GpuClassifierBackend
from inference_arena_amd.utils.settings import Settings

ROOT = Path(__file__).resolve().parents[1]
TOP = (np.array([7, 1, 2, 3, 4], np.int32), np.array([5, 4, 3, 2, 1], np.float32),
       np.array([0.6, 0.2, 0.1, 0.05, 0.05], np.float32))


def _scene(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([x / max(w, 1) * 200, y / max(h, 1) * 180, (x + y) / max(h + w, 1) * 150], -1)
    img += rng.normal(0, 12, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def _jpeg(arr, **kw) -> bytes:
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "JPEG", **{"quality": 95, **kw})
    return b.getvalue()


# ---- routing ------------------------------------------------------------------------------------------------------


class PlainBackend(ClassifierBackend):
    """Records classify() calls; no classify_bytes (the CPU backend's shape)."""

    def __init__(self):
        self.calls = []

    async def classify(self, crop):
        self.calls.append(("classify", crop.shape))
        return TOP


class BytesBackend(PlainBackend):
    async def classify_bytes(self, data, decode):
        self.calls.append(("classify_bytes", len(data)))
        self.decode = decode
        return TOP


def _classify(servicer, data, monkeypatch):
    """One Classify call; returns (response, names of the threads decode_crop ran on)."""
    threads = []

    def recording_decode(d):
        threads.append(threading.current_thread().name)
        return decode_crop(d)

    monkeypatch.setattr(cs, "decode_crop", recording_decode)
    try:
        resp = asyncio.run(servicer.Classify(pb.ClassificationRequest(request_id="r", image_crop=data)))
    finally:
        servicer.close()
    return resp, threads


CROP = _scene(37, 53)


def test_jpeg_crop_goes_to_classify_bytes(monkeypatch):
    be = BytesBackend()
    data = encode_crop(CROP, "jpeg")
    resp, threads = _classify(cs.ClassificationServicer(be, [], crop_decode="gpu"), data, monkeypatch)
    assert resp.error == "" and resp.result.class_id == 7 and len(resp.top_k) == 5
    assert be.calls == [("classify_bytes", len(data))] and threads == []  # no PIL decode anywhere
    # the fallback handed to the backend is the thread-pool PIL decode
    sv = cs.ClassificationServicer(be, [], crop_decode="gpu")
    try:
        np.testing.assert_array_equal(asyncio.run(sv._decode(data)), decode_crop(data))
    finally:
        sv.close()


def test_raw_crop_keeps_the_no_hop_path(monkeypatch):
    be = BytesBackend()
    resp, threads = _classify(cs.ClassificationServicer(be, [], crop_decode="gpu"), encode_crop(CROP, "raw"),
                              monkeypatch)
    assert resp.error == "" and be.calls == [("classify", CROP.shape)]
    assert threads == [threading.current_thread().name]  # decoded inline on the event loop's thread


def test_png_crop_keeps_the_pool_decode(monkeypatch):
    be = BytesBackend()
    resp, threads = _classify(cs.ClassificationServicer(be, [], crop_decode="gpu"), encode_crop(CROP, "png"),
                              monkeypatch)
    assert resp.error == "" and be.calls == [("classify", CROP.shape)]
    assert len(threads) == 1 and threads[0].startswith("crop-decode")


def test_backend_without_classify_bytes_keeps_the_pil_path(monkeypatch):
    be = PlainBackend()
    resp, threads = _classify(cs.ClassificationServicer(be, [], crop_decode="gpu"), encode_crop(CROP, "jpeg"),
                              monkeypatch)
    assert resp.error == "" and be.calls == [("classify", CROP.shape)]
    assert len(threads) == 1 and threads[0].startswith("crop-decode")


@pytest.mark.parametrize("kw", [{}, {"crop_decode": "pil"}])
def test_switch_off_is_todays_path(monkeypatch, kw):
    be = BytesBackend()
    resp, threads = _classify(cs.ClassificationServicer(be, [], **kw), encode_crop(CROP, "jpeg"), monkeypatch)
    assert resp.error == "" and be.calls == [("classify", CROP.shape)]
    assert len(threads) == 1 and threads[0].startswith("crop-decode")


def test_corrupt_crop_answers_in_band(monkeypatch):
    class Failing(BytesBackend):
        async def classify_bytes(self, data, decode):
            raise ValueError("Failed to decode image: truncated")

    sv = cs.ClassificationServicer(Failing(), [], crop_decode="gpu")
    resp, _ = _classify(sv, encode_crop(CROP, "jpeg")[:200], monkeypatch)
    assert "truncated" in resp.error and resp.request_id == "r" and sv.n_errors == 1


def test_start_server_hands_the_setting_to_the_servicer():
    async def go(mode):
        s = Settings(LOG_LEVEL="WARNING", HOST="127.0.0.1", **({"ARENA_CROP_DECODE": mode} if mode else {}))
        server, servicer, _ = await cs.start_server(s, BytesBackend(), port=0)
        await server.stop(0)
        servicer.close()
        return servicer.crop_decode

    assert asyncio.run(go(None)) == "pil" and asyncio.run(go("gpu")) == "gpu"


# ---- settings -----------------------------------------------------------------------------------------------------


def test_setting_default_and_env_template():
    assert Settings().ARENA_CROP_DECODE == "pil"
    keys = [ln.split("=", 1)[0].strip() for ln in (ROOT / ".env.example").read_text().splitlines() if "=" in ln]
    assert "ARENA_CROP_DECODE" in keys
    assert keys.index("ARENA_CROP_DECODE") == keys.index("ARENA_CROP_ENCODE") + 1


# ---- classify_bytes over a host-only instance ------------------------------------------------------------------


def test_classify_bytes_pixels_and_ingest_stats():
    """GpuClassifierBackend.classify_bytes with an EchoInstance in place of the GPU sessions: the instance
    reconstructs split-decoded JPEGs with the kernels' arithmetic (jpeg_coefs_to_rgb) and records what it got."""
    from inference_arena_amd.server.batching import AsyncBatcher

    C = native()
    echo = C.EchoInstance(2, 8, 4, 0)
    echo.set_record(True)
    be = GpuClassifierBackend.__new__(GpuClassifierBackend)
    be.runners = [types.SimpleNamespace(ex=echo)]
    be.batcher = AsyncBatcher(be.runners, max_batch=8, max_queue_delay_us=200)
    assert "ingest" not in be.stats()  # no ingest before the first classify_bytes

    gray = np.asarray(Image.fromarray(_scene(9, 9, 5)).convert("L"))
    native_crops = [encode_crop(_scene(37, 53, 1), "jpeg"), encode_crop(_scene(8, 8, 2), "jpeg"),
                    _jpeg(_scene(17, 33, 3), subsampling=0), _jpeg(_scene(16, 16, 4), subsampling=1), _jpeg(gray)]
    fallback_crops = [encode_crop(_scene(20, 31, 6), "png"), encode_crop(_scene(11, 3, 7), "jpeg"),
                      _jpeg(_scene(40, 40, 8), progressive=True)]
    truncated = native_crops[0][: len(native_crops[0]) // 2]
    decoded = []

    async def decode(data):
        decoded.append(data)
        return decode_crop(data)

    async def go():
        out = []
        for data in native_crops + fallback_crops:  # one at a time: the record is in this order
            out.append(await be.classify_bytes(data, decode))
        with pytest.raises(ValueError):
            await be.classify_bytes(truncated, decode)
        return out

    try:
        out = asyncio.run(go())
        st = be.stats()
        got = echo.take_recorded()
    finally:
        be.close()
    assert decoded == fallback_crops  # only what the split decoder handed back went through the caller's decoder
    assert len(got) == len(native_crops) + len(fallback_crops)
    for data, rgb in zip(native_crops + fallback_crops, got):
        np.testing.assert_array_equal(rgb, decode_crop(data))
    assert got[4].shape == (9, 9, 3) and (got[4][..., 0] == got[4][..., 1]).all()  # gray crop: R = G = B
    for idx, logit, prob in out:  # the triple classify returns
        assert idx.shape == logit.shape == prob.shape == (5,)
    ing = st["ingest"]
    assert (ing["native"], ing["fallback"], ing["errors"]) == (len(native_crops), len(fallback_crops), 1)
    assert st["requests"] == len(native_crops) + len(fallback_crops)  # the batcher's own counters stay


# ---- launch plan of the ragged reconstruction ----------------------------------------------------------------------


def _ceil(a, b):
    return -(-a // b)


def _blocks(data):
    d = native().jpeg_coefs(data)
    assert d["status"] == "ok", d["error"]
    return sum(c["bw"] * c["bh"] for c in d["comps"]), d["width"], d["height"]


def test_ragged_plan_prefixes_and_totals():
    C = native()
    sizes = [(600, 400), (64, 96), (1, 5), (8, 8), (9, 7), (17, 33), (250, 180), (64, 96)]
    batch = [_jpeg(_scene(h, w, i), subsampling=(2, 0, 1)[i % 3]) for i, (h, w) in enumerate(sizes)]
    p = C.jpeg_ragged_plan(batch)
    geo = [_blocks(b) for b in batch]
    iu = [_ceil(nb, 32) for nb, _, _ in geo]
    cu = [_ceil(_ceil(w, 4) * h, 256) for _, w, h in geo]
    assert list(p["idct_first"]) == [sum(iu[:i]) for i in range(len(iu))]
    assert list(p["color_first"]) == [sum(cu[:i]) for i in range(len(cu))]
    for first in (p["idct_first"], p["color_first"]):
        assert first[0] == 0 and all(a <= b for a, b in zip(first, first[1:]))
    assert p["idct_units"] == sum(iu) and p["color_units"] == sum(cu)
    assert p["rect_idct_units"] == len(batch) * max(iu)
    assert p["rect_color_units"] == len(batch) * max(_ceil(w * h, 1024) for _, w, h in geo)
    assert p["idct_units"] < p["rect_idct_units"] and p["color_units"] < p["rect_color_units"]


def test_ragged_plan_of_one_image_is_the_rectangular_launch():
    C = native()
    for h, w, sub in [(130, 96, 2), (37, 52, 0), (8, 8, 1)]:  # widths that are multiples of 4: quads = pixels / 4
        p = C.jpeg_ragged_plan([_jpeg(_scene(h, w), subsampling=sub)])
        assert list(p["idct_first"]) == [0] and list(p["color_first"]) == [0]
        assert p["idct_units"] == p["rect_idct_units"] and p["color_units"] == p["rect_color_units"]


def test_ragged_plan_of_33_single_mcu_crops():
    """33 crops of 8x8 in 4:4:4: 3 blocks and 2 x 8 = 16 quads each, so one IDCT unit and one colour unit per crop
    (a unit never spans two images), where the rectangular pair launches the same 33 + 33."""
    C = native()
    p = C.jpeg_ragged_plan([_jpeg(_scene(8, 8, i), subsampling=0) for i in range(33)])
    assert list(p["idct_first"]) == list(range(33)) == list(p["color_first"])
    assert (p["idct_units"], p["color_units"], p["rect_idct_units"], p["rect_color_units"]) == (33, 33, 33, 33)


def test_ragged_plan_rejects_what_the_decoder_does_not_take():
    C = native()
    assert C.jpeg_ragged_plan([])["idct_units"] == 0
    with pytest.raises(ValueError):
        C.jpeg_ragged_plan([encode_crop(CROP, "png")])


def test_ragged_flag_reaches_the_backend_from_the_setting(monkeypatch):
    """build_classifier_backend builds the sessions of ARENA_CROP_DECODE=gpu with jpeg_ragged (and only those)."""
    from inference_arena_amd.server import service_backends as sb

    seen = []

    class Rec:
        def __init__(self, mnet, **kw):
            seen.append(kw.get("jpeg_ragged"))

    monkeypatch.setattr(sb, "GpuClassifierBackend", Rec)
    import inference_arena_amd.models.zoo as zoo

    monkeypatch.setattr(zoo, "resolve_models", lambda *a, **k: (None, None))
    sb.build_classifier_backend(Settings(LOG_LEVEL="WARNING"))
    sb.build_classifier_backend(Settings(LOG_LEVEL="WARNING", ARENA_CROP_DECODE="gpu"))
    assert seen == [False, sb.CROP_DECODE_RAGGED]
