"""EXIF orientation on every decode path, on CPU.

The reference decodes uploads with cv2.imdecode(..., IMREAD_COLOR) (src/shared/processing/transforms.py:103),
which turns a JPEG upright by its EXIF Orientation tag.  The native parser (csrc/runtime/jpeg_decode.cpp) and its
Python twin (processing/exif.py) must read the tag by one rule, and the host reconstruction, the PIL paths, the
ingest and the native front end must all return the upright pixels: PIL's unrotated decode rearranged with numpy
(exif_cases.expected)."""
from __future__ import annotations

import io
import json

import numpy as np
import pytest
from PIL import Image

import exif_cases as X
from inference_arena_amd.ops import native
from inference_arena_amd.processing.exif import jpeg_orientation
from inference_arena_amd.processing.transforms import decode_rgb, load_image, load_image_from_bytes

HOWS = ["pil", "le", "le_far"]
SIZE = (45, 67)  # h, w: odd, partial MCUs in every layout


def _native_orientation(data: bytes):
    d = native().jpeg_coefs(data)
    return d["status"], d["orientation"], (d["out_height"], d["out_width"]), (d["height"], d["width"])


def test_parsers_agree_on_wellformed_tags():
    arr = X.scene(*SIZE)
    for how in HOWS:
        for o in range(0, 10):
            data = X.tagged(arr, "420", o, how)
            want = o if 1 <= o <= 8 else 1
            st, no, out, stored = _native_orientation(data)
            assert st == "ok" and no == want == jpeg_orientation(data), (how, o, st, no)
            assert stored == SIZE and out == (SIZE[::-1] if want >= 5 else SIZE)
    plain = X.encode(arr, "420")
    assert _native_orientation(plain)[:2] == ("ok", 1) and jpeg_orientation(plain) == 1
    assert jpeg_orientation(b"") == 1 and jpeg_orientation(b"\x89PNG\r\n\x1a\n" + bytes(32)) == 1


def _hostile_cases(plain: bytes):
    A = X.app1
    xmp = X.segment(0xE1, b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta xmlns:tiff='http://ns.adobe.com/tiff/1.0/'>"
                          b"<tiff:Orientation>6</tiff:Orientation></x:xmpmeta>")
    cut = A(6)[:4 + 6 + 8]  # marker, length, "Exif\0\0", TIFF header; the length is rewritten below
    cut = cut[:2] + (len(cut) - 2).to_bytes(2, "big") + cut[4:]
    sos = plain.index(b"\xff\xda")
    sos_end = sos + 2 + int.from_bytes(plain[sos + 2:sos + 4], "big")
    return {
        "count beyond the segment": (X.splice(plain, A(6, n_entries=60000)), 1),
        "count one entry too many": (X.splice(plain, A(6, n_entries=2)), 1),
        "ifd offset past the end": (X.splice(plain, A(6, ifd=8).replace(b"II*\0\x08\0\0\0", b"II*\0\x00\x10\0\0")), 1),
        "ifd offset wrapping": (X.splice(plain, A(6, ifd=8).replace(b"II*\0\x08\0\0\0", b"II*\0\xfe\xff\xff\xff")), 1),
        "cut after the TIFF header": (X.splice(plain, cut), 1),
        "xmp only": (X.splice(plain, xmp), 1),
        "xmp then exif": (X.splice(plain, xmp + A(8)), 8),
        "type LONG": (X.splice(plain, A(6, typ=4)), 1),
        "count 2": (X.splice(plain, A(6, count=2)), 1),
        "big-endian, not first": (X.splice(plain, A(7, order=">", before=3)), 7),
        "bad magic": (X.splice(plain, A(6).replace(b"II*\0", b"II+\0")), 1),
        "mixed byte-order mark": (X.splice(plain, A(6).replace(b"II*\0", b"IM*\0")), 1),
        "first exif segment decides": (X.splice(plain, A(9) + A(6)), 1),
        "exif after SOS": (plain[:sos_end] + A(6) + plain[sos_end:], 1),
        "exif after EOI": (plain + A(6), 1),
    }


def test_parsers_agree_on_hostile_exif():
    plain = X.encode(X.scene(24, 40), "420")
    for name, (data, want) in _hostile_cases(plain).items():
        st, no, _, _ = _native_orientation(data)
        tw = jpeg_orientation(data)
        if name == "exif after SOS":  # inside the entropy-coded data: the scan may not survive, the tag is unseen
            assert no == tw == 1, name
            continue
        assert st == "ok", (name, st)
        assert no == tw, (name, no, tw)
        if want is not None:
            assert no == want, (name, no)


def test_parsers_agree_under_random_flips():
    plain = X.encode(X.scene(24, 40), "444")
    rng = np.random.default_rng(5)
    seen = set()
    for base in (X.app1(6, before=1, after=1), X.app1(3, order=">", ifd=12)):
        for _ in range(200):
            seg = bytearray(base)
            for k in rng.integers(4, len(seg), rng.integers(1, 4)):  # inside the payload: marker and length stay
                seg[k] ^= 1 << int(rng.integers(0, 8))
            data = X.splice(plain, bytes(seg))
            st, no, _, _ = _native_orientation(data)
            assert st == "ok" and 1 <= no <= 8 and no == jpeg_orientation(data)
            seen.add(no)
    assert len(seen) > 2  # the flips reach the tag, its type and its value, not only padding


@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_oriented_pixels_on_every_host_path(layout, tmp_path):
    from inference_arena_amd.server.app_common import probe_size

    C = native()
    arr = X.scene(*SIZE, seed=3)
    a = X.unrotated(X.encode(arr, layout))
    for o in range(1, 9):
        data = X.tagged(arr, layout, o, HOWS[o % 3])
        want = X.expected(a, o)
        st, err, rgb = C.jpeg_decode_host(data)
        assert st == "ok", err
        np.testing.assert_array_equal(rgb, want, err_msg=f"jpeg_decode_host {o}")
        np.testing.assert_array_equal(load_image_from_bytes(data), want, err_msg=f"load_image_from_bytes {o}")
        h, w, px = decode_rgb(data)
        assert (h, w) == want.shape[:2] and px == want.tobytes(), o
        assert probe_size(data) == want.shape[:2]
        p = tmp_path / f"o{o}.jpg"
        p.write_bytes(data)
        np.testing.assert_array_equal(load_image(p), want)
    # a PNG is untouched, whatever it carries
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "PNG", exif=X.pil_exif(6))
    np.testing.assert_array_equal(load_image_from_bytes(b.getvalue()), arr)
    assert probe_size(b.getvalue()) == SIZE


@pytest.mark.parametrize("jpeg_device", [True, False])
def test_ingest_answers_for_the_upright_image(jpeg_device):
    """AsyncBatcher.run_jpeg over the echo instance: a tagged baseline JPEG (split decoder) and a tagged
    progressive JPEG (PIL fallback) answer like run() of the expected pixels."""
    import asyncio
    import types

    from inference_arena_amd.server.batching import AsyncBatcher

    C = native()
    runner = types.SimpleNamespace(ex=C.EchoInstance(2, 8, 4, 200))
    b = AsyncBatcher([runner], max_batch=8, max_queue_delay_us=500)
    if not jpeg_device:
        b._ingest = C.JpegIngest(b._b, {"threads": 2, "jpeg_device": False})
    cases = []
    for i, o in enumerate([6, 3, 5, 8, 2, 7, 4]):
        arr = X.scene(30 + 5 * i, 41 + 3 * i, seed=i)
        layout = X.LAYOUTS[1 + i % 3]
        base = X.tagged(arr, layout, o, HOWS[i % 3])
        prog = X.encode(arr, layout, exif=X.pil_exif(o), progressive=True)
        cases.append((base, X.expected(X.unrotated(base), o)))
        cases.append((prog, X.expected(X.unrotated(prog), o)))
    calls = []

    async def decode(data):
        calls.append(data)
        return load_image_from_bytes(data)

    async def go():
        a = await asyncio.gather(*(b.run_jpeg(u, decode) for u, _ in cases))
        r = await asyncio.gather(*(b.run(w) for _, w in cases))
        return a, r

    try:
        a, r = asyncio.run(go())
    finally:
        b.close()
    for x, y in zip(a, r):
        assert x["det_count"] == y["det_count"]
        np.testing.assert_array_equal(x["det"], y["det"])
        np.testing.assert_array_equal(x["topk_idx"], y["topk_idx"])
    assert sorted(calls) == sorted(u for u, _ in cases[1::2])  # exactly the progressive ones fell back
    assert len({x["det_count"] for x in a}) > 1


def test_native_front_end_answers_for_the_upright_image():
    """/predict over the echo engine: a tagged JPEG answers like the PNG of its expected pixels (lossless, PIL
    path), whose boxes carry the upright width and height; oriented_decoded counts the tagged uploads."""
    from inference_arena_amd.labels import load_labels
    from inference_arena_amd.server.native_front import NativeFrontEnd
    from test_native_http import _multipart, _post

    C = native()
    batcher = C.DynamicBatcher([C.EchoInstance(2, 8, 4, 200)], {"max_batch": 8, "max_queue_delay_us": 200})
    fe = NativeFrontEnd(batcher, load_labels(None), port=0, host="127.0.0.1", io_threads=2, decode_procs=1, slots=16,
                        decode_threads=2)

    def ask(data):
        body, ct = _multipart(data)
        st, out, c = _post(fe.port, body, ct)
        c.close()
        assert st == 200, out
        return [(d["detection"], d["classification"]) for d in json.loads(out)["detections"]]

    try:
        answers = set()
        for i, o in enumerate([6, 8, 3]):
            arr = X.scene(40 + 8 * i, 72 + 4 * i, seed=10 + i)
            jpg = X.tagged(arr, "420", o, HOWS[i])
            want = X.expected(X.unrotated(jpg), o)
            png = io.BytesIO()
            Image.fromarray(want).save(png, "PNG")
            got = ask(jpg)
            assert got == ask(png.getvalue()), o
            # progressive: the PIL pool's decode is upright too
            assert ask(X.encode(arr, "420", exif=X.pil_exif(o), progressive=True))[0][0]["x2"] == got[0][0]["x2"]
            answers.add(json.dumps(got))
        assert ask(X.encode(X.scene(40, 72), "420"))  # untagged
        s = fe.stats()
        assert s["oriented_decoded"] == 3 and s["native_decoded"] == 4, s
        assert len(answers) == 3
    finally:
        fe.close()
        batcher.shutdown()


def test_exif_fuzz_under_sanitizers(tmp_path):
    """csrc/tests/exif_fuzz.cpp with the host decoder, built host-only with AddressSanitizer and UBSan: mutated
    APP1 segments never change the status, and the oriented RGB buffer is written exactly."""
    import os
    import shutil
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (Path(hipcc).exists() or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    srcs = [root / "csrc" / "tests" / "exif_fuzz.cpp", root / "csrc" / "runtime" / "jpeg_decode.cpp"]
    exe = root / "build" / "exif_fuzz_asan_ubsan"
    exe.parent.mkdir(parents=True, exist_ok=True)
    newest = max(p.stat().st_mtime for p in srcs + [root / "csrc" / "runtime" / "jpeg_decode.h",
                                                   root / "csrc" / "kernels" / "jpeg_math.h"])
    if not exe.exists() or exe.stat().st_mtime < newest:
        cmd = [hipcc, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Xarch_host",
               "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
               "-I" + str(root / "csrc"), *map(str, srcs), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
    for i, (layout, o, how) in enumerate([("420", 6, "pil"), ("422", 7, "le_far"), ("gray", 3, "le")]):
        seed = tmp_path / f"seed{i}.jpg"
        seed.write_bytes(X.tagged(X.scene(41, 54, seed=i), layout, o, how))
        r = subprocess.run([str(exe), str(seed), "1500"], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1"))
        report = r.stdout + r.stderr
        assert "Sanitizer" not in report and "runtime error" not in report and r.returncode == 0, report[-6000:]
        assert "exif_fuzz: ok" in r.stdout
