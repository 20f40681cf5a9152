"""The split JPEG crop encoder on the CPU: host half, shared arithmetic and service wiring.

* ``jpeg_encode_host`` (csrc/runtime/jpeg_encode.cpp: the kernel's arithmetic from kernels/jpeg_enc_math.h, the
  Huffman pass and the markers) gives PIL's quality-95 bytes on the smallest shapes at which each edge rule can go
  wrong, for contents from noise to the 0/255 checkerboards that drive the DCT accumulators to their extremes;
* the quantisation tables are PIL's, and the encoder's coefficients are the ones the repository's own decoder
  reads back out of its files;
* ``ARENA_CROP_ENCODE=gpu`` in the detection service: the RPCs carry the bytes the ``pil`` setting sends, the
  upload is never decoded on the host, the frame slot goes back after success, errors and cancellation — and never
  before the encode has completed; requests the path does not cover take the PIL path;
* the host half runs clean under AddressSanitizer + UBSan (stand-alone csrc/tests/jpeg_encode_check.cpp).
"""
from __future__ import annotations

import asyncio
import io
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from fastapi.testclient import TestClient
from PIL import Image

from inference_arena_amd.data.synthetic import encode_jpeg, synthetic_images
from inference_arena_amd.ops import native
from inference_arena_amd.processing import extract_crop
from inference_arena_amd.processing.transforms import load_image_from_bytes
from inference_arena_amd.proto import inference_api as pb
from inference_arena_amd.server.crop_codec import JPEG_QUALITY, GpuCropEncoder, encode_crop
from inference_arena_amd.server.device_transport import DeviceImageRing
from inference_arena_amd.server.grpc_client import ClassificationClient
from inference_arena_amd.server.multipart import encode_multipart
from inference_arena_amd.server.service_backends import DetectorBackend
from inference_arena_amd.utils.settings import Settings

SHAPES = [(1, 1), (1, 9), (2, 2), (3, 12), (12, 3), (8, 8), (9, 7), (10, 10), (16, 16), (17, 33), (31, 16), (40, 5),
          (5, 40), (24, 40), (40, 24), (23, 23), (37, 53), (100, 75)]  # h x w
CONTENTS = ["random", "gradient", "two-tone", "checker", "checker-green-inverted", "zeros", "ones"]

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
      28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
      47, 55, 62, 63]  # zigzag index -> natural index


def _crop(h: int, w: int, content: str) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    ck = (((yy + xx) & 1) * 255).astype(np.uint8)
    if content == "random":
        return np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "gradient":
        return np.stack([(yy * 7 + xx * 3) % 256, (xx * 5) % 256, (yy * 11 + 40) % 256], -1).astype(np.uint8)
    if content == "two-tone":
        a = np.full((h, w, 3), [255, 0, 128], np.uint8)
        a[h // 2:] = [3, 250, 9]
        return a
    if content == "checker":
        return np.stack([ck, ck, ck], -1)
    if content == "checker-green-inverted":
        return np.stack([ck, 255 - ck, ck], -1)
    return np.full((h, w, 3), 0 if content == "zeros" else 255, np.uint8)


@pytest.fixture(scope="module")
def corpus():
    """(h, w, content) -> (crop, PIL's bytes), computed once."""
    out = {}
    for h, w in SHAPES:
        for content in CONTENTS:
            c = _crop(h, w, content)
            out[(h, w, content)] = (c, encode_crop(c, "jpeg"))
    return out


def _scan(data: bytes) -> bytes:
    i = data.index(b"\xff\xda")
    n = int.from_bytes(data[i + 2:i + 4], "big")
    return data[i + 2 + n:-2]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_encoder_bytes_equal_pil(corpus, shape):
    C = native()
    for content in CONTENTS:
        crop, want = corpus[(*shape, content)]
        got = C.jpeg_encode_host(crop)
        assert got == want, f"{shape} {content}: {len(got)} bytes, PIL {len(want)}"


def test_corpus_exercises_byte_stuffing(corpus):
    assert any(b"\xff\x00" in _scan(want) for _, want in corpus.values())


def test_host_encoder_accepts_non_contiguous_crops_and_rejects_other_shapes():
    C = native()
    frame = synthetic_images(1, 4)[0]
    view = frame[3:40, 5:58]  # a view: the binding packs it
    assert C.jpeg_encode_host(view) == encode_crop(view.copy(), "jpeg")
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((0, 4, 3), np.uint8), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            C.jpeg_encode_host(bad)


def _dqt_payloads(data: bytes) -> dict[int, bytes]:
    out, pos = {}, 2
    while data[pos + 1] != 0xDA:
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        if data[pos + 1] == 0xDB:
            seg = data[pos + 4:pos + 2 + n]
            while seg:
                assert seg[0] >> 4 == 0  # 8-bit
                out[seg[0] & 15] = seg[1:65]
                seg = seg[65:]
        pos += 2 + n
    return out


@pytest.mark.parametrize("quality", [JPEG_QUALITY, 50, 75, 100])
def test_tables_equal_pil(quality):
    buf = io.BytesIO()
    Image.fromarray(_crop(16, 16, "gradient")).save(buf, format="JPEG", quality=quality)
    dqt = _dqt_payloads(buf.getvalue())
    t = native().jpeg_enc_tables(quality, zigzag=True)
    assert bytes(t[0].astype(np.uint8)) == dqt[0] and bytes(t[1].astype(np.uint8)) == dqt[1]
    nat = native().jpeg_enc_tables(quality)
    assert np.array_equal(t[:, np.arange(64)], nat[:, ZZ])


def _scan_blocks(C, data: bytes, w: int, h: int):
    """The coefficients the repository's decoder reads from ``data`` in the encoder's layout (int16[blocks][64],
    zigzag, scan order MCU by MCU) and the mask of real (not dummy) block slots."""
    d = C.jpeg_coefs(data)
    assert d["status"] == "ok", d["error"]
    mcux, mcuy, ybw, ybh = (w + 15) // 16, (h + 15) // 16, (w + 7) // 8, (h + 7) // 8
    out = np.zeros((mcux * mcuy * 6, 64), np.int16)
    real = np.zeros(len(out), bool)
    for my in range(mcuy):
        for mx in range(mcux):
            for s in range(6):
                c = 0 if s < 4 else s - 3
                by, bx = (2 * my + (s >> 1), 2 * mx + (s & 1)) if s < 4 else (my, mx)
                k = d["comps"][c]
                off = k["coef_off"] + (by * k["bw"] + bx) * 64
                i = (my * mcux + mx) * 6 + s
                out[i] = d["coef"][off:off + 64][ZZ]
                real[i] = s >= 4 or (by < ybh and bx < ybw)
    return out, real


def test_round_trip_through_the_repository_decoder(corpus):
    """jpeg_coefs(jpeg_encode_host(x)) == jpeg_encode_coefs_host(x) on the real blocks; a dummy slot of a partial
    MCU decodes to zero AC and the DC of the block coded before it.  (The split decoder leaves files with fewer than
    three chroma columns, i.e. crops up to 4 pixels wide, to PIL: those report 'unsupported' and are skipped.)"""
    C = native()
    decoded = dummies = 0
    for (h, w, content), (crop, _) in corpus.items():
        if content not in ("random", "checker-green-inverted"):
            continue
        data = C.jpeg_encode_host(crop)
        want = C.jpeg_encode_coefs_host(crop)
        assert want.shape == (((w + 15) // 16) * ((h + 15) // 16) * 6, 64)
        assert np.array_equal(C.jpeg_encode_coefs_host(crop, zigzag=False)[:, ZZ], want)
        assert C.jpeg_write(w, h, want) == data
        if w <= 4:
            assert C.jpeg_coefs(data)["status"] == "unsupported"
            continue
        got, real = _scan_blocks(C, data, w, h)
        np.testing.assert_array_equal(got[real], want[real], err_msg=f"{h}x{w} {content}")
        for i in np.flatnonzero(~real):
            assert not got[i, 1:].any() and got[i, 0] == got[i - 1, 0], f"{h}x{w} {content}: dummy slot {i}"
        decoded += 1
        dummies += int((~real).sum())
    assert decoded >= 20 and dummies >= 20


# ---- service wiring -------------------------------------------------------------------------------------------------

class FakeDeviceMemory:
    """'Device' memory of the fakes: one host bytearray at a made-up base address."""

    def __init__(self, nbytes: int, tag: int = 3):
        self.data = bytearray(nbytes)
        self.ptr = (tag + 1) << 40

    def handle(self) -> bytes:
        return b"\x07" * 64

    def frame(self, ptr: int, h: int, w: int) -> np.ndarray:
        off = ptr - self.ptr
        assert 0 <= off and off + h * w * 3 <= len(self.data)
        return np.frombuffer(bytes(self.data[off:off + h * w * 3]), np.uint8).reshape(h, w, 3)


class ExportingDetector(DetectorBackend):
    """Stands in for the GPU detector: 'reconstructs' the upload into the slot it is given."""

    exports_frames = True

    def __init__(self, mem: FakeDeviceMemory):
        self.mem = mem
        self.bytes_calls = self.exports = 0

    def _export(self, image, export_to):
        if export_to:
            b = np.ascontiguousarray(image).tobytes()
            off = export_to - self.mem.ptr
            self.mem.data[off:off + len(b)] = b
            self.exports += 1

    async def detect(self, image, export_to=0):
        self._export(image, export_to)
        h, w = image.shape[:2]
        # a fixed box, one clipped by the frame with fractional corners, an empty one, an odd origin
        return np.array([[0, 0, 10, 20, 0.9, 1], [5.7, 5.2, w + 3.5, h + 0.5, 0.7, 2], [3, 3, 3, 9, 0.6, 4],
                         [7, 9, 24, 26, 0.55, 5]], np.float32), {}


class SplitDetector(ExportingDetector):
    """... and takes the upload's bytes, like the detector with the split decoder."""

    async def detect_bytes(self, data, decode, export_to=0):
        self.bytes_calls += 1
        return await self.detect(load_image_from_bytes(data), export_to)


class HostEncoder:
    """The injected encoder: GpuCropEncoder's interface over jpeg_encode_host on the fake device memory.  With
    ``hold`` the encode completes only when the test calls ``finish()``."""

    def __init__(self, mem: FakeDeviceMemory, hold: bool = False, fail: bool = False):
        self.mem, self.hold, self.fail = mem, hold, fail
        self.calls = 0
        self.pending: list = []

    def submit(self, frame_ptr, h, w, det, frame_bytes=0):
        self.calls += 1
        assert h * w * 3 <= frame_bytes
        frame = self.mem.frame(frame_ptr, h, w)
        fut = asyncio.get_running_loop().create_future()

        def complete():
            if self.fail:
                fut.set_exception(RuntimeError("HIP error (injected)"))
            else:
                fut.set_result([native().jpeg_encode_host(extract_crop(frame, d)) for d in det])

        if self.hold:
            self.pending.append(complete)
        else:
            complete()
        return fut

    def finish(self):
        for c in self.pending:
            c()
        self.pending.clear()


class RecordingStub:
    def __init__(self):
        self.sent: list[tuple[str, bytes, tuple]] = []
        self.raise_error = False
        self.gate: asyncio.Event | None = None
        self.waiting = 0

    async def _one(self, req):
        b = req.source_box
        self.sent.append((req.request_id.rsplit("_", 1)[1], bytes(req.image_crop),
                          (b.x1, b.y1, b.x2, b.y2, round(b.confidence, 4), b.class_id)))
        r = pb.ClassificationResponse(request_id=req.request_id)
        r.result.class_id = len(req.image_crop) % 1000
        r.result.class_name = "x"
        r.result.confidence = 0.5
        return r

    async def Classify(self, req, timeout=None):
        if self.gate is not None:
            self.waiting += 1
            await self.gate.wait()
        if self.raise_error:
            raise RuntimeError("classification exploded")
        return await self._one(req)

    async def ClassifyBatch(self, breq, timeout=None):
        if self.raise_error:
            raise RuntimeError("classification exploded")
        return pb.BatchClassificationResponse(responses=[await self._one(r) for r in breq.requests])


def _client() -> ClassificationClient:
    cl = ClassificationClient("fake:0")
    cl.stub = RecordingStub()  # connected; no channel
    return cl


class CountingDecode:
    def __init__(self, pool):
        self.pool, self.calls = pool, 0

    async def decode(self, data):
        self.calls += 1
        return await self.pool.decode(data)

    def close(self):
        self.pool.close()


def _ring(mem: FakeDeviceMemory, slots: int, slot_bytes: int) -> DeviceImageRing:
    return DeviceImageRing(slots, slot_bytes, buffer=mem)


def _post(app, body, ctype, n=1):
    """n posts through the app; returns the responses and the counting decode pool."""
    with TestClient(app) as c:
        dec = app.state.arena["decode"] = CountingDecode(app.state.arena["decode"])
        return [c.post("/predict", content=body, headers={"content-type": ctype}) for _ in range(n)], dec


@pytest.fixture(scope="module")
def upload():
    img = synthetic_images(1, 5)[0]
    return encode_multipart("file", encode_jpeg(img))


def _sent(cl):
    return sorted(cl.stub.sent)


@pytest.mark.parametrize("fanout", ["parallel", "batch"])
@pytest.mark.parametrize("split", [True, False], ids=["split-decoder", "exported-upload"])
def test_gpu_setting_sends_the_bytes_of_the_pil_setting(upload, fanout, split, monkeypatch):
    from inference_arena_amd.server.detection_service import create_app

    if not split:
        monkeypatch.setenv("ARENA_NATIVE_DECODE", "0")
    body, ctype = upload
    slot_bytes = 640 * 640 * 3
    det_cls = SplitDetector if split else ExportingDetector
    # today's path: the default setting
    mem0 = FakeDeviceMemory(slot_bytes)
    cl0, enc0 = _client(), HostEncoder(mem0)
    s0 = Settings(LOG_LEVEL="WARNING", ARENA_FANOUT=fanout)
    assert s0.ARENA_CROP_ENCODE == "pil"
    out0, dec0 = _post(create_app(s0, detector=det_cls(mem0), client=cl0, encoder=enc0), body, ctype)
    assert out0[0].status_code == 200, out0[0].text
    assert enc0.calls == 0 and dec0.calls == 1  # the encoder is never touched
    # the gpu setting
    mem = FakeDeviceMemory(2 * slot_bytes)
    ring, enc, cl, det = _ring(mem, 2, slot_bytes), HostEncoder(mem), _client(), det_cls(mem)
    s = Settings(LOG_LEVEL="WARNING", ARENA_FANOUT=fanout, ARENA_CROP_ENCODE="gpu")
    out, dec = _post(create_app(s, detector=det, client=cl, ring=ring, encoder=enc), body, ctype, n=3)
    for r in out:
        assert r.status_code == 200, r.text
        assert r.json()["detections"] == out0[0].json()["detections"]
    assert len(cl0.stub.sent) == 4 and _sent(cl) == sorted(cl0.stub.sent * 3)
    assert enc.calls == 3 and det.exports == 3
    assert dec.calls == (0 if split else 3) and det.bytes_calls == (3 if split else 0)
    assert sorted(ring._free) == [0, 1]


def test_requests_the_gpu_path_does_not_cover_take_the_pil_path(upload):
    from inference_arena_amd.server.detection_service import create_app

    body, ctype = upload
    s = Settings(LOG_LEVEL="WARNING", ARENA_CROP_ENCODE="gpu")
    want_mem = FakeDeviceMemory(16)
    cl0 = _client()
    _post(create_app(Settings(LOG_LEVEL="WARNING"), detector=SplitDetector(want_mem), client=cl0), body, ctype)

    # a frame larger than a slot
    mem = FakeDeviceMemory(2 * 300)
    ring, enc, cl, det = _ring(mem, 2, 300), HostEncoder(mem), _client(), SplitDetector(mem)
    out, dec = _post(create_app(s, detector=det, client=cl, ring=ring, encoder=enc), body, ctype)
    assert out[0].status_code == 200 and enc.calls == 0 and dec.calls == 1 and det.exports == 0
    assert _sent(cl) == _sent(cl0) and sorted(ring._free) == [0, 1]

    # no free slot
    mem = FakeDeviceMemory(640 * 640 * 3)
    ring, enc, cl, det = _ring(mem, 1, 640 * 640 * 3), HostEncoder(mem), _client(), SplitDetector(mem)
    assert ring.try_acquire() == 0
    out, dec = _post(create_app(s, detector=det, client=cl, ring=ring, encoder=enc), body, ctype)
    assert out[0].status_code == 200 and enc.calls == 0 and dec.calls == 1 and det.exports == 0
    assert _sent(cl) == _sent(cl0) and ring._free == []

    # a detector without frame export
    class Plain(DetectorBackend):
        async def detect(self, image):
            return await ExportingDetector(want_mem).detect(image)

    mem = FakeDeviceMemory(640 * 640 * 3)
    ring, enc, cl = _ring(mem, 1, 640 * 640 * 3), HostEncoder(mem), _client()
    out, dec = _post(create_app(s, detector=Plain(), client=cl, ring=ring, encoder=enc), body, ctype)
    assert out[0].status_code == 200 and enc.calls == 0 and dec.calls == 1
    assert _sent(cl) == _sent(cl0) and ring._free == [0]

    # another crop transport: ARENA_CROP_ENCODE only concerns jpeg crops
    mem = FakeDeviceMemory(640 * 640 * 3)
    enc, cl = HostEncoder(mem), _client()
    s_png = Settings(LOG_LEVEL="WARNING", ARENA_CROP_ENCODE="gpu", ARENA_CROP_TRANSPORT="png")
    out, dec = _post(create_app(s_png, detector=SplitDetector(mem), client=cl, encoder=enc), body, ctype)
    assert out[0].status_code == 200 and enc.calls == 0 and dec.calls == 1


def test_slot_is_released_after_errors(upload):
    from inference_arena_amd.server.detection_service import create_app

    body, ctype = upload
    s = Settings(LOG_LEVEL="WARNING", ARENA_CROP_ENCODE="gpu")
    slot_bytes = 640 * 640 * 3
    # a classification error
    mem = FakeDeviceMemory(slot_bytes)
    ring, enc, cl = _ring(mem, 1, slot_bytes), HostEncoder(mem), _client()
    cl.stub.raise_error = True
    out, _ = _post(create_app(s, detector=SplitDetector(mem), client=cl, ring=ring, encoder=enc), body, ctype, n=2)
    assert [r.status_code for r in out] == [500, 500] and enc.calls == 2  # the second request got the slot again
    assert ring._free == [0]
    # an encoder (HIP) error is reported in-band and not retried
    enc, cl = HostEncoder(mem, fail=True), _client()
    out, _ = _post(create_app(s, detector=SplitDetector(mem), client=cl, ring=ring, encoder=enc), body, ctype)
    assert out[0].status_code == 500 and "HIP error" in out[0].text and enc.calls == 1 and cl.stub.sent == []
    assert ring._free == [0]

    # a failed detection
    class Failing(SplitDetector):
        async def detect(self, image, export_to=0):
            raise RuntimeError("detector exploded")

    enc = HostEncoder(mem)
    out, _ = _post(create_app(s, detector=Failing(mem), client=_client(), ring=ring, encoder=enc), body, ctype)
    assert out[0].status_code == 500 and enc.calls == 0 and ring._free == [0]


def test_slot_is_held_until_the_encode_completes_after_cancellation():
    from inference_arena_amd.server.detection_service import create_app

    data = encode_jpeg(synthetic_images(1, 5)[0])
    s = Settings(LOG_LEVEL="WARNING", ARENA_CROP_ENCODE="gpu")
    slot_bytes = 640 * 640 * 3
    mem = FakeDeviceMemory(slot_bytes)
    ring, enc, cl = _ring(mem, 1, slot_bytes), HostEncoder(mem, hold=True), _client()
    app = create_app(s, detector=SplitDetector(mem), client=cl, ring=ring, encoder=enc)

    async def scenario():
        predict = app.state.arena["predict_bytes"]
        # cancelled while the encode is in flight: the slot stays taken until the encode has really completed
        t = asyncio.ensure_future(predict(data))
        while not enc.pending:
            await asyncio.sleep(0)
        t.cancel()
        with pytest.raises(asyncio.CancelledError):
            await t
        assert ring._free == [] and enc.pending
        enc.finish()
        await asyncio.sleep(0)
        assert ring._free == [0] and cl.stub.sent == []
        # cancelled while the classification is in flight: the encode is over, the slot is already back
        cl.stub.gate = asyncio.Event()
        enc.hold = False
        t = asyncio.ensure_future(predict(data))
        while not cl.stub.waiting:
            await asyncio.sleep(0)
        assert ring._free == [0]
        t.cancel()
        with pytest.raises(asyncio.CancelledError):
            await t
        assert ring._free == [0]
        # and the service still answers
        cl.stub.gate = None
        r = await predict(data)
        assert len(r.detections) == 4 and ring._free == [0]

    with TestClient(app):  # runs the lifespan (decode pool, metrics)
        asyncio.run(scenario())


def test_gpu_crop_encoder_wrapper_reports_native_errors_in_band():
    """GpuCropEncoder over a stand-in native encoder: blobs and errors arrive from another thread."""
    import threading

    class Native:
        def __init__(self):
            self.stopped = False

        def submit(self, ptr, h, w, boxes, done, frame_bytes):
            assert boxes == [(1.5, 2.0, 3.0, 4.0)] and (ptr, h, w, frame_bytes) == (4096, 5, 6, 90)
            threading.Thread(target=done, args=((None, "HIP error (injected)") if self.stopped else ([b"x"], ""))).start()

        def stop(self):
            self.stopped = True

    async def go():
        e = GpuCropEncoder(native_encoder=Native())
        det = np.array([[1.5, 2, 3, 4, 0.9, 1]], np.float32)
        assert await e.encode(4096, 5, 6, det, frame_bytes=90) == [b"x"]
        e.close()
        with pytest.raises(RuntimeError, match="HIP error"):
            await e.encode(4096, 5, 6, det, frame_bytes=90)

    asyncio.run(go())


# ---- memory safety of the host half ---------------------------------------------------------------------------------

def test_host_encoder_check_under_address_and_ub_sanitizers():
    """csrc/tests/jpeg_encode_check.cpp, built host-only with -fsanitize=address,undefined: 300 random crops of
    1..70 pixels a side through the host encoder and back through the repository's decoder, without a report."""
    root = Path(__file__).resolve().parents[1]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (Path(hipcc).exists() or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    srcs = [root / "csrc" / "tests" / "jpeg_encode_check.cpp", root / "csrc" / "runtime" / "jpeg_encode.cpp",
            root / "csrc" / "runtime" / "jpeg_decode.cpp"]
    hdrs = [root / "csrc" / "runtime" / "jpeg_encode.h", root / "csrc" / "runtime" / "jpeg_decode.h",
            root / "csrc" / "kernels" / "jpeg_enc_math.h", root / "csrc" / "kernels" / "jpeg_math.h",
            root / "csrc" / "kernels" / "jpeg_enc_desc.h"]
    exe = root / "build" / "jpeg_encode_check_asan"
    exe.parent.mkdir(parents=True, exist_ok=True)
    if not exe.exists() or exe.stat().st_mtime < max(p.stat().st_mtime for p in srcs + hdrs):
        cmd = [hipcc, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Xarch_host", "-fsanitize=address,undefined",
               "-I" + str(root / "csrc"), *map(str, srcs), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe), "300", "7"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    report = r.stdout + r.stderr
    assert "Sanitizer" not in report and "runtime error" not in report and r.returncode == 0, report[-6000:]
    assert "jpeg_encode_check: ok" in r.stdout
