"""Progressive (SOF2) uploads through the host half of the split JPEG decoder (csrc/runtime/jpeg_decode.h) on CPU.

PIL's decode of a complete progressive file equals its decode of the baseline file of the same image, quality and
subsampling, so the split decoder's bit-exact reconstruction applies unchanged once the scans are entropy-decoded
(T.81 Annex G) into the coefficient blocks a baseline scan would give: the baseline twin is the coefficient oracle,
PIL the pixel oracle.  The switch is off by default (ARENA_JPEG_PROGRESSIVE=0): every test passes ``progressive=``
per call or per object and none touches the process default.  A file whose result is not certainly libjpeg's
warning-free one (incomplete or inconsistent progression, too many scans, DQT between scans) is handed back as
"unsupported", from the decode stage, and the callers send it to their PIL path."""
from __future__ import annotations

import io

import numpy as np
import pytest
from PIL import Image

from inference_arena_amd.ops import native

SIZES = [(427, 640), (37, 53), (17, 33), (16, 16), (9, 7), (13, 17)]
SMALL = SIZES[1:]


def _enc(arr, **kw) -> bytes:
    # libjpeg writes a progressive file in one go and PIL sizes the buffer for it by a guess (2 bytes per pixel at
    # q >= 95) that a noisy 4:4:4 q100 frame exceeds ("Suspension not allowed here"): give it room for any frame
    from PIL import ImageFile

    b = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 8 * arr.shape[0] * arr.shape[1] + 65536)
    try:
        Image.fromarray(arr).save(b, "JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return b.getvalue()


def _pil(data: bytes) -> np.ndarray:
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def _scene(h, w, seed=0):
    """A natural-ish frame: smooth gradients + blobs + noise (every DCT frequency band populated)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([x / max(w, 1) * 200, y / max(h, 1) * 180, (x + y) / max(h + w, 1) * 150], -1)
    for _ in range(6):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(3, max(4, min(h, w) / 3))
        img += (((y - cy) ** 2 + (x - cx) ** 2) < r * r)[..., None] * rng.uniform(-90, 90, 3)
    img += rng.normal(0, 12, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def _grey(arr):
    return np.asarray(Image.fromarray(arr).convert("L"))


def _segments(data: bytes):
    """[(marker, start, end)] of a JPEG file: each marker segment with the entropy-coded data that follows it (an
    SOS segment extends to the next marker that is neither a restart marker nor a stuffed 0xFF00)."""
    out, pos = [(0xD8, 0, 2)], 2
    while pos < len(data):
        assert data[pos] == 0xFF, pos
        m = data[pos + 1]
        if m == 0xD9:
            out.append((m, pos, pos + 2))
            break
        end = pos + 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
        if m == 0xDA:
            while not (data[end] == 0xFF and data[end + 1] != 0 and not 0xD0 <= data[end + 1] <= 0xD7):
                end += 1
        out.append((m, pos, end))
        pos = end
    return out


def _scans(data: bytes):
    """(index into _segments, Ns, first component selector, Ss, Se, Ah, Al) of every scan."""
    out = []
    for i, (m, a, _) in enumerate(_segments(data)):
        if m == 0xDA:
            ns = data[a + 4]
            t = a + 5 + 2 * ns
            out.append((i, ns, data[a + 5], data[t], data[t + 1], data[t + 2] >> 4, data[t + 2] & 15))
    return out


def _join(data: bytes, segs) -> bytes:
    return b"".join(data[a:b] for _, a, b in segs)


def test_control_progressive_is_unsupported_by_default():
    C = native()
    prog = _enc(_scene(37, 53), quality=90, progressive=True)
    assert b"\xff\xc2" in prog
    assert not C.jpeg_progressive_default()
    st, err, rgb = C.jpeg_decode_host(prog)
    assert st == "unsupported" and rgb is None and "progressive" in err
    st, err, rgb = C.jpeg_decode_host(prog, progressive=False)
    assert st == "unsupported" and rgb is None
    assert C.jpeg_coefs(prog)["status"] == "unsupported"


@pytest.mark.parametrize("quality", [50, 75, 90, 95, 100])
@pytest.mark.parametrize("subsampling", [0, 1, 2, "grey"])
def test_bit_exact_with_pil(quality, subsampling):
    C = native()
    for i, (h, w) in enumerate(SIZES + [(101, 3)]):
        img = _scene(h, w, i)
        kw = {} if subsampling == "grey" else {"subsampling": subsampling}
        data = _enc(_grey(img) if subsampling == "grey" else img, quality=quality, progressive=True, **kw)
        assert b"\xff\xc2" in data
        st, err, rgb = C.jpeg_decode_host(data, progressive=True)
        if subsampling in (1, 2) and w <= 4:  # chroma narrower than 3 samples: the same rule as for baseline files
            assert st == "unsupported"
            continue
        assert st == "ok", (h, w, err)
        np.testing.assert_array_equal(rgb, _pil(data))


@pytest.mark.parametrize("blocks", [1, 3, 7])
@pytest.mark.parametrize("subsampling", [0, 1, 2, "grey"])
def test_restart_intervals(blocks, subsampling):
    C = native()
    for i, (h, w) in enumerate([(120, 170)] + SMALL):
        img = _scene(h, w, 10 + i)
        kw = {} if subsampling == "grey" else {"subsampling": subsampling}
        data = _enc(_grey(img) if subsampling == "grey" else img, quality=88, progressive=True,
                    restart_marker_blocks=blocks, **kw)
        assert b"\xff\xdd" in data and b"\xff\xc2" in data
        st, err, rgb = C.jpeg_decode_host(data, progressive=True)
        assert st == "ok", (h, w, err)
        np.testing.assert_array_equal(rgb, _pil(data))
        twin = C.jpeg_coefs(_enc(_grey(img) if subsampling == "grey" else img, quality=88, **kw))
        np.testing.assert_array_equal(C.jpeg_coefs(data, progressive=True)["coef"], twin["coef"])


def test_exif_orientation_is_honoured():
    C = native()
    img = _scene(37, 53, 3)
    exif = Image.Exif()
    exif[0x0112] = 6
    data = _enc(img, quality=90, subsampling=2, progressive=True, exif=exif.tobytes())
    d = C.jpeg_coefs(data, progressive=True)
    assert d["status"] == "ok" and d["progressive"] and d["orientation"] == 6
    st, err, rgb = C.jpeg_decode_host(data, progressive=True)
    assert st == "ok", err
    assert rgb.shape == (53, 37, 3)
    np.testing.assert_array_equal(rgb, np.rot90(_pil(data), -1))  # PIL's convert() leaves the stored frame


@pytest.mark.parametrize("subsampling", [0, 1, 2, "grey"])
def test_coefficients_equal_the_baseline_twin(subsampling):
    """Every block of every component, the MCU padding of the grid included: libjpeg's encoder fills the padding
    from the same coefficient arrays in both modes (the last real block's DC, zero AC), and the progressive decoder
    takes the padding's DC from the interleaved DC scans and leaves its AC zero."""
    C = native()
    for i, (h, w) in enumerate(SIZES):
        img = _scene(h, w, 20 + i)
        for q in (50, 90, 100):
            kw = {} if subsampling == "grey" else {"subsampling": subsampling}
            arr = _grey(img) if subsampling == "grey" else img
            p = C.jpeg_coefs(_enc(arr, quality=q, progressive=True, **kw), progressive=True)
            b = C.jpeg_coefs(_enc(arr, quality=q, **kw))
            assert p["status"] == "ok" and b["status"] == "ok", (p["error"], b["error"])
            assert p["progressive"] and not b["progressive"]
            for key in ("width", "height", "layout", "mcux", "mcuy", "coef_count", "comps"):
                assert p[key] == b[key], key
            np.testing.assert_array_equal(p["coef"], b["coef"])


def test_all_zero_image_decodes_dense_and_compact():
    C = native()
    for arr in (np.full((16, 16), 128, np.uint8), np.full((16, 16, 3), 128, np.uint8)):
        data = _enc(arr, quality=90, progressive=True)
        dense = C.jpeg_coefs(data, progressive=True)
        compact = C.jpeg_coefs(data, progressive=True, compact=True)
        assert dense["status"] == "ok" and compact["status"] == "ok", (dense["error"], compact["error"])
        assert not dense["coef"].any() and not compact["coef"].any()
        st, err, rgb = C.jpeg_decode_host(data, progressive=True)
        assert st == "ok", err
        np.testing.assert_array_equal(rgb, _pil(data))
        # a block without coefficients still stores its DC, as the baseline producer's blocks do
        base = C.jpeg_coefs(_enc(arr, quality=90), compact=True)
        assert compact["compact_bytes"] == base["compact_bytes"]


@pytest.mark.parametrize("subsampling", [0, 1, 2, "grey"])
def test_compact_payload_expands_to_the_dense_blocks(subsampling):
    """jpeg_decode_compact on a progressive file: the payload fits jpeg_compact_capacity (the binding raises
    otherwise) and expands to the dense decode."""
    C = native()
    for i, (h, w) in enumerate(SMALL):
        img = _scene(h, w, 30 + i)
        kw = {} if subsampling == "grey" else {"subsampling": subsampling}
        arr = _grey(img) if subsampling == "grey" else img
        for q in (50, 100):
            data = _enc(arr, quality=q, progressive=True, **kw)
            dense = C.jpeg_coefs(data, progressive=True)
            compact = C.jpeg_coefs(data, progressive=True, compact=True)
            assert dense["status"] == "ok" and compact["status"] == "ok"
            np.testing.assert_array_equal(compact["coef"], dense["coef"])
            # never longer than the baseline twin's (whose scan decoder also stores the zero a ZRL code ends on)
            assert compact["compact_bytes"] <= C.jpeg_coefs(_enc(arr, quality=q, **kw), compact=True)["compact_bytes"]


def _hand_back_cases():
    prog = _enc(_scene(64, 80, 5), quality=90, subsampling=2, progressive=True)
    segs, scans = _segments(prog), _scans(prog)
    assert len(scans) == 10 and segs[-1][0] == 0xD9
    cases = {}
    # the last scan removed (EOI kept): some coefficients never reach bit 0 and libjpeg smooths
    last = scans[-1][0]
    dht_before = last - 1 if segs[last - 1][0] == 0xC4 else last
    cases["incomplete"] = _join(prog, segs[:dht_before] + segs[last + 1:])
    # two AC scans of one component swapped (with the DHT segments in front of each): a refinement comes before
    # the first scan of its band, or a band's first scan comes twice as far as Ah / Al tell
    ac = [s for s in scans if s[1] == 1 and s[3] > 0 and s[2] == scans[-1][2]]
    assert len(ac) >= 2
    a, b = ac[0][0], ac[-1][0]

    def unit(i):  # a scan with the DHT segment(s) right in front of it
        j = i
        while segs[j - 1][0] == 0xC4:
            j -= 1
        return j, i + 1

    (a0, a1), (b0, b1) = unit(a), unit(b)
    assert a1 <= b0
    cases["swapped"] = _join(prog, segs[:a0] + segs[b0:b1] + segs[a1:b0] + segs[a0:a1] + segs[b1:])
    # one refinement scan 40 times: the scan cap, answered without 40 passes' worth of time
    ref = [s for s in scans if s[5] > 0][-1][0]
    r0, r1 = unit(ref)
    cases["scan_cap"] = _join(prog, segs[:r1] + segs[r0:r1] * 39 + segs[r1:])
    # a DQT between scans: libjpeg would dequantise later scans' components differently
    dqt = next(s for s in segs if s[0] == 0xDB)
    second = scans[1][0]
    s0, _ = unit(second)
    cases["dqt_between_scans"] = _join(prog, segs[:s0] + [dqt] + segs[s0:])
    return prog, cases


@pytest.mark.parametrize("name", ["incomplete", "swapped", "scan_cap", "dqt_between_scans"])
def test_doubtful_files_are_handed_back(name):
    import time

    C = native()
    prog, cases = _hand_back_cases()
    st, err, rgb = C.jpeg_decode_host(prog, progressive=True)
    assert st == "ok", err
    np.testing.assert_array_equal(rgb, _pil(prog))
    data = cases[name]
    assert data != prog
    if name == "incomplete":  # PIL decodes it, with libjpeg's inter-block smoothing: not the exact reconstruction
        assert _pil(data).shape == (64, 80, 3)
    t0 = time.perf_counter()
    st, err, rgb = C.jpeg_decode_host(data, progressive=True)
    dt = time.perf_counter() - t0
    assert st != "ok", name
    assert st == "unsupported" and rgb is None, (name, st, err)
    assert C.jpeg_coefs(data, progressive=True, compact=True)["status"] == "unsupported"
    if name == "scan_cap":
        assert len(_scans(data)) == 49 and dt < 0.25, dt


def test_ok_always_means_pil_pixels():
    """Whatever the surgery, a file the decoder accepts has PIL's pixels."""
    C = native()
    prog, cases = _hand_back_cases()
    segs, scans = _segments(prog), _scans(prog)
    # further variants: every single scan dropped, every pair of neighbouring scans swapped
    for k, s in enumerate(scans):
        cases[f"drop{k}"] = _join(prog, segs[:s[0]] + segs[s[0] + 1:])
    for k in range(len(scans) - 1):
        i, j = scans[k][0], scans[k + 1][0]
        cases[f"swap{k}"] = _join(prog, segs[:i] + segs[i + 1:j + 1] + segs[i:i + 1] + segs[j + 1:])
    n_ok = 0
    for name, data in cases.items():
        st, err, rgb = C.jpeg_decode_host(data, progressive=True)
        assert st in ("ok", "corrupt", "unsupported"), name
        if st == "ok":
            n_ok += 1
            np.testing.assert_array_equal(rgb, _pil(data), err_msg=name)
    assert n_ok < len(cases)


def test_damaged_scan_data_is_handed_back_or_exact():
    """Byte flips inside the entropy-coded data of the scans.  Where libjpeg would warn (a code that matches
    nothing, a segment that ends early or leaves bytes over, a restart marker out of place, a refinement symbol
    of another magnitude than 1) the decoder hands the file back; what it accepts has PIL's pixels."""
    import warnings

    C = native()
    seeds = [_enc(_scene(40, 56, 1), quality=90, subsampling=2, progressive=True),
             _enc(_scene(33, 47, 2), quality=75, subsampling=0, progressive=True, restart_marker_blocks=3),
             _enc(_grey(_scene(40, 56, 3)), quality=90, progressive=True, restart_marker_blocks=1)]
    rng = np.random.default_rng(21)
    seen = {"ok": 0, "corrupt": 0, "unsupported": 0}
    for it in range(450):
        good = seeds[it % len(seeds)]
        spans = [(a + 2 + int.from_bytes(good[a + 2:a + 4], "big"), b) for m, a, b in _segments(good) if m == 0xDA]
        bad = bytearray(good)
        for _ in range(1 + it % 2):
            a, b = spans[int(rng.integers(0, len(spans)))]
            bad[int(rng.integers(a, b))] = int(rng.integers(0, 256))
        bad = bytes(bad)
        st, err, rgb = C.jpeg_decode_host(bad, progressive=True)
        seen[st] += 1
        if st == "ok":
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                np.testing.assert_array_equal(rgb, _pil(bad), err_msg=f"mutation {it}")
    assert seen["ok"] > 20 and seen["unsupported"] > 100, seen


def test_truncation_is_corrupt_like_pil():
    C = native()
    prog = _enc(_scene(64, 80, 6), quality=90, subsampling=2, progressive=True)
    segs, scans = _segments(prog), _scans(prog)
    _, a, b = segs[scans[2][0]]
    cut = prog[:(a + b) // 2 + 4]  # inside the third scan's entropy-coded data, no EOI
    st, err, rgb = C.jpeg_decode_host(cut, progressive=True)
    assert st == "corrupt" and "truncated" in err and rgb is None, (st, err)
    with pytest.raises(OSError):
        _pil(cut)
    # between two scans, no EOI: libjpeg waits for the rest, PIL raises
    cut = prog[:b]
    st, err, rgb = C.jpeg_decode_host(cut, progressive=True)
    assert st == "corrupt" and "truncated" in err, (st, err)
    with pytest.raises(OSError):
        _pil(cut)


def test_fuzz_random_byte_flips_never_crash():
    C = native()
    good = _enc(_scene(64, 80, 7), quality=90, subsampling=2, progressive=True, restart_marker_blocks=3)
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(300):
        bad = bytearray(good)
        for k in rng.integers(2, len(bad), 8):
            bad[k] = int(rng.integers(0, 256))
        for compact in (False, True):
            st = C.jpeg_coefs(bytes(bad), progressive=True, compact=compact)["status"]
            assert st in ("ok", "corrupt", "unsupported")
            seen.add(st)
    assert len(seen) >= 2


@pytest.mark.parametrize("progressive", [True, False])
def test_ingest_takes_progressive_uploads_when_switched_on(progressive):
    """csrc/runtime/jpeg_ingest.h behind AsyncBatcher.run_jpeg over the CPU echo instance: with the switch on,
    progressive uploads never reach the caller's decoder and count as native; with it off they all do.  The file
    whose last scan is missing passes jpeg_parse and is handed back by the entropy decode: it reaches the caller's
    decoder either way."""
    import asyncio
    import types

    from inference_arena_amd.processing.transforms import load_image_from_bytes
    from inference_arena_amd.server.batching import AsyncBatcher

    C = native()
    runner = types.SimpleNamespace(ex=C.EchoInstance(2, 8, 4, 200))
    b = AsyncBatcher([runner], max_batch=8, max_queue_delay_us=500)
    rng = np.random.default_rng(4)
    frames = [(rng.random((30 + 5 * i, 41 + 3 * i, 3)) * 255).astype(np.uint8) for i in range(6)]
    uploads = [_enc(f, quality=85, subsampling=i % 3, progressive=True) for i, f in enumerate(frames)]
    incomplete = _hand_back_cases()[1]["incomplete"]
    calls = []

    async def decode(data):
        calls.append(data)
        return load_image_from_bytes(data)

    async def go():
        a = await asyncio.gather(*(b.run_jpeg(u, decode, progressive=progressive) for u in uploads))
        r = await asyncio.gather(*(b.run(_pil(u)) for u in uploads))
        n_calls = len(calls)
        p = await b.run_jpeg(incomplete, decode)
        return a, r, n_calls, p

    try:
        a, r, n_calls, p = asyncio.run(go())
        st = b.ingest_stats()
    finally:
        b.close()
    for x, y in zip(a, r):
        np.testing.assert_array_equal(x["det"], y["det"])
        np.testing.assert_array_equal(x["topk_idx"], y["topk_idx"])
    assert len({x["det_count"] for x in a}) > 1
    assert n_calls == (0 if progressive else 6)
    assert calls[n_calls:] == [incomplete] and p["det_count"] >= 1
    if progressive:
        assert (st["native"], st["progressive_decoded"], st["fallback"], st["errors"]) == (6, 6, 1, 0)
    else:
        assert (st["native"], st["progressive_decoded"], st["fallback"], st["errors"]) == (0, 0, 7, 0)


def test_native_front_end_hands_a_doubtful_file_to_the_pil_pool():
    """/predict over the echo engine with the switch on: a complete progressive upload is split-decoded, the one
    whose last scan is missing passes jpeg_parse, is handed back by the entropy decode and answered through the PIL
    pool (200, not the 500 of a decode failure), and both answer like the PNG of PIL's pixels."""
    import json

    from inference_arena_amd.labels import load_labels
    from inference_arena_amd.server.native_front import NativeFrontEnd
    from test_native_http import _multipart, _post

    C = native()
    prog, cases = _hand_back_cases()
    batcher = C.DynamicBatcher([C.EchoInstance(2, 8, 4, 200)], {"max_batch": 8, "max_queue_delay_us": 200})
    fe = NativeFrontEnd(batcher, load_labels(None), port=0, host="127.0.0.1", io_threads=2, decode_procs=1, slots=16,
                        decode_threads=2, progressive=True)

    def ask(data):
        body, ct = _multipart(data)
        st, out, c = _post(fe.port, body, ct)
        c.close()
        assert st == 200, out
        return [(d["detection"], d["classification"]) for d in json.loads(out)["detections"]]

    def png(arr):
        b = io.BytesIO()
        Image.fromarray(arr).save(b, "PNG")
        return b.getvalue()

    try:
        got = ask(prog)
        s = fe.stats()
        assert (s["native_decoded"], s["progressive_decoded"], s["fallback_decoded"]) == (1, 1, 0), s
        assert got and got == ask(png(_pil(prog)))
        got = ask(cases["incomplete"])
        s = fe.stats()
        assert (s["native_decoded"], s["progressive_decoded"], s["fallback_decoded"]) == (1, 1, 2), s
        assert got and got == ask(png(_pil(cases["incomplete"])))
    finally:
        fe.close()
        batcher.shutdown()


def test_settings_know_the_switch():
    from inference_arena_amd.utils.settings import Settings

    assert Settings().ARENA_JPEG_PROGRESSIVE == 0
    assert Settings(ARENA_JPEG_PROGRESSIVE="1").ARENA_JPEG_PROGRESSIVE == 1


def test_decoder_fuzz_under_address_sanitizer(tmp_path):
    """csrc/tests/jpeg_progressive_fuzz.cpp: the host decoder built host-only with AddressSanitizer and
    UndefinedBehaviorSanitizer, run as a program of its own over PIL-written progressive seeds mutated in-process
    (dense and compact decode of every mutation, the compact payload checked against the dense blocks)."""
    import os
    import shutil
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (Path(hipcc).exists() or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    srcs = [root / "csrc" / "tests" / "jpeg_progressive_fuzz.cpp", root / "csrc" / "runtime" / "jpeg_decode.cpp"]
    exe = root / "build" / "jpeg_progressive_fuzz_asan"
    exe.parent.mkdir(parents=True, exist_ok=True)
    newest = max(p.stat().st_mtime for p in srcs + [root / "csrc" / "runtime" / "jpeg_decode.h",
                                                   root / "csrc" / "kernels" / "jpeg_math.h"])
    if not exe.exists() or exe.stat().st_mtime < newest:
        cmd = [hipcc, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Xarch_host",
               "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
               "-I" + str(root / "csrc"), *map(str, srcs), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
    seeds = []
    variants = [dict(subsampling=2), dict(subsampling=1, restart_marker_blocks=3), dict(subsampling=0, quality=100),
                dict(grey=True, restart_marker_blocks=1)]
    for i, kw in enumerate(variants):
        img = _scene(40 + 7 * i, 56 + 5 * i, i)
        if kw.pop("grey", False):
            img = _grey(img)
        p = tmp_path / f"seed{i}.jpg"
        p.write_bytes(_enc(img, **{"quality": 90, **kw}, progressive=True))
        seeds.append(str(p))
    r = subprocess.run([str(exe), "600", *seeds], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    report = r.stdout + r.stderr
    assert "Sanitizer" not in report and "runtime error" not in report and r.returncode == 0, report[-6000:]
    assert "jpeg_progressive_fuzz: ok" in r.stdout
