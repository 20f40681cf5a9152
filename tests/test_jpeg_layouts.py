"""4:4:0, 4:1:1 and the other integral chroma ratios, RGB-coded files and sequential files in several scans through
the host half of the split JPEG decoder (csrc/runtime/jpeg_decode.h) on CPU.

PIL cannot write these files, so jpeg_layout_cases.py does; PIL's decode of each file is the pixel oracle.  A file
the decoder accepts has PIL's pixels bit for bit; the files libjpeg would decode to something this decoder does not
vouch for (a component coded twice or never, a DQT between scans, luma below the maximum factor, unequal chroma
factors, narrow fancy chroma) are "unsupported" and go to the callers' PIL path."""
from __future__ import annotations

import io

import numpy as np
import pytest
from PIL import Image

import exif_cases as X
import jpeg_layout_cases as L
from inference_arena_amd.ops import native

CASES = L.cases()


def test_writer_self_test():
    """The writer's own check (passes without the layouts under test): PIL opens every case as RGB and the 4:2:0
    single-scan control is decoded exactly as PIL decodes it."""
    assert L.self_test() == len(CASES) >= 140


def test_every_case_is_exact_with_pil():
    C = native()
    seen = set()
    for name, data in CASES:
        st, err, rgb = C.jpeg_decode_host(data)
        assert st == "ok", (name, err)
        np.testing.assert_array_equal(rgb, L.pil(data), err_msg=name)
        info = C.jpeg_coefs(data)
        got = (info["layout"], info["rh"], info["rv"], info["rgb_coded"], info["multiscan"])
        assert got == L.expected_layout(name), name
        seen.add(got)
    assert len(seen) >= 11  # every sampling, both colour codings, walked and single scans


def test_compact_payload_expands_to_the_dense_blocks():
    C = native()
    for name, data in CASES:
        dense, compact = C.jpeg_coefs(data), C.jpeg_coefs(data, compact=True)
        assert dense["status"] == compact["status"] == "ok", name
        np.testing.assert_array_equal(compact["coef"], dense["coef"], err_msg=name)
        assert 0 < compact["compact_bytes"]


def test_scans_decode_to_the_single_scan_blocks():
    """The coefficient oracle of a multi-scan file: the same components written in one interleaved scan."""
    C = native()
    for si, (h, w) in enumerate(L.SIZES):
        img = L.scene(h, w, si)
        for sampling in (L.S444, L.S440, L.S411):
            one = C.jpeg_coefs(L.write(img, sampling))
            for script in L.SCAN_SCRIPTS.values():
                many = C.jpeg_coefs(L.write(img, sampling, scans=script, restart=2))
                assert one["status"] == many["status"] == "ok" and many["multiscan"] and not one["multiscan"]
                a, b = one["coef"], many["coef"]
                # the MCU padding of a component is coded by interleaved scans only; the walker leaves it zero
                for c, k in enumerate(one["comps"]):
                    blk = lambda x: x[k["coef_off"]:k["coef_off"] + k["bw"] * k["bh"] * 64].reshape(k["bh"], k["bw"], 64)
                    rb, cb = -(-k["ch"] // 8), -(-k["cw"] // 8)
                    np.testing.assert_array_equal(blk(a)[:rb, :cb], blk(b)[:rb, :cb])


def _negative_cases():
    img = L.scene(33, 47, 7)
    dqt = L.segment(0xDB, bytes([1]) + bytes([3] * 64))
    return {
        "coded_twice": L.write(img, L.S444, scans=[[0], [1], [2], [1]]),
        "never_coded": L.write(img, L.S444, scans=[[0], [1]]),
        "dqt_between_scans": L.write(img, L.S440, scans=[[0], [1], [2]], between={1: dqt}),
        "unequal_chroma": L.write(img, [(2, 2), (1, 1), (2, 1)]),
        "luma_below_max": L.write(img, [(1, 1), (2, 2), (2, 2)]),
        "narrow_422": L.write(L.scene(21, 4, 8), [(2, 1), (1, 1), (1, 1)]),
        "narrow_420": L.write(L.scene(21, 4, 9), L.S420),
        "narrow_420_scans": L.write(L.scene(21, 4, 9), L.S420, scans=[[0], [1, 2]]),
    }


@pytest.mark.parametrize("name", sorted(_negative_cases()))
def test_negative_cases_are_handed_back_and_open_in_pil(name):
    C = native()
    data = _negative_cases()[name]
    st, err, rgb = C.jpeg_decode_host(data)
    assert st == "unsupported" and rgb is None and err, (name, st, err)
    assert C.jpeg_coefs(data, compact=True)["status"] == "unsupported"
    assert L.pil(data).shape[2] == 3


def test_mcu_of_more_than_ten_blocks_is_handed_back():
    """libjpeg refuses such an interleaved scan; the message is PIL's to give."""
    C = native()
    data = L.write(L.scene(20, 20, 3), [(4, 4), (1, 1), (1, 1)])
    assert C.jpeg_decode_host(data)[0] == "unsupported"
    with pytest.raises(Exception):
        L.pil(data)
    # the same frame in three scans has no interleaved MCU and is exact
    data = L.write(L.scene(20, 20, 3), [(4, 4), (1, 1), (1, 1)], scans=[[0], [1], [2]])
    st, err, rgb = C.jpeg_decode_host(data)
    assert st == "ok", err
    np.testing.assert_array_equal(rgb, L.pil(data))


@pytest.mark.parametrize("sampling", ["440", "411", "410"])
def test_progressive_twins(sampling):
    """The same blocks as SOF2 files (a DC scan and one AC scan per component): exact with the switch on."""
    C = native()
    for si, (h, w) in enumerate(L.SIZES):
        img = L.scene(h, w, 20 + si)
        data = L.write(img, L.SAMPLINGS[sampling][0], progressive=True, restart=si % 3)
        assert b"\xff\xc2" in data
        assert C.jpeg_decode_host(data, progressive=False)[0] == "unsupported"
        st, err, rgb = C.jpeg_decode_host(data, progressive=True)
        assert st == "ok", (h, w, err)
        np.testing.assert_array_equal(rgb, L.pil(data))


@pytest.mark.parametrize("sampling", ["440", "411"])
@pytest.mark.parametrize("orientation", range(1, 9))
def test_exif_orientations(sampling, orientation):
    C = native()
    for h, w in ((37, 53), (9, 7), (16, 16)):
        data = X.splice(L.write(L.scene(h, w, orientation), L.SAMPLINGS[sampling][0]), X.app1(orientation))
        st, err, rgb = C.jpeg_decode_host(data)
        assert st == "ok", err
        np.testing.assert_array_equal(rgb, X.expected(X.unrotated(data), orientation))


def _pil_or_none(data):
    import warnings

    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with Image.open(io.BytesIO(data)) as im:
                return np.asarray(im.convert("RGB"))
    except Exception:  # noqa: BLE001
        return None


def test_ok_always_means_pil_pixels():
    """Scans dropped, swapped and repeated, and files cut inside a scan: what the decoder accepts has PIL's pixels,
    everything else is corrupt or handed back."""
    C = native()
    seeds = [L.write(L.scene(33, 47, 1), L.S440, scans=[[0], [1], [2]]),
             L.write(L.scene(25, 40, 2), L.S420, scans=[[0], [1, 2]], restart=2),
             L.write(L.scene(18, 35, 3), L.S411, scans=[[2], [0], [1]]),
             L.write(L.scene(18, 35, 4), L.S444, scans=[[0], [1], [2]], jfif=False, adobe=0)]
    n_ok = n = 0
    for s, good in enumerate(seeds):
        segs = L.segments(good)
        scans = [i for i, (m, _, _) in enumerate(segs) if m == 0xDA]
        variants = {"good": good}
        for k, i in enumerate(scans):
            variants[f"drop{k}"] = L.join(good, segs[:i] + segs[i + 1:])
            variants[f"twice{k}"] = L.join(good, segs[:i + 1] + segs[i:])
            a, b = segs[i][1] + 2 + int.from_bytes(good[segs[i][1] + 2:segs[i][1] + 4], "big"), segs[i][2]
            variants[f"cut{k}"] = good[:(a + b) // 2]
            variants[f"cut{k}_eoi"] = good[:(a + b) // 2] + b"\xff\xd9"
            variants[f"short{k}"] = L.join(good, segs[:i]) + good[segs[i][1]:(a + b) // 2] + L.join(good, segs[i + 1:])
        for k in range(len(scans) - 1):
            i, j = scans[k], scans[k + 1]
            variants[f"swap{k}"] = L.join(good, segs[:i] + segs[j:j + 1] + segs[i + 1:j] + segs[i:i + 1] + segs[j + 1:])
        for name, data in variants.items():
            st, err, rgb = C.jpeg_decode_host(data)
            assert st in ("ok", "corrupt", "unsupported"), (s, name)
            n += 1
            if st == "ok":
                n_ok += 1
                np.testing.assert_array_equal(rgb, _pil_or_none(data), err_msg=f"seed {s} {name}")
    assert len(seeds) < n_ok < n  # the swaps are exact too: the order of the scans is free


def test_random_byte_flips_never_crash():
    C = native()
    picks = [d for n, d in CASES if "37x53" in n or "33x17" in n]
    rng = np.random.default_rng(33)
    seen = {"ok": 0, "corrupt": 0, "unsupported": 0}
    for it in range(300):
        bad = bytearray(picks[it % len(picks)])
        for _ in range(1 + it % 4):
            bad[int(rng.integers(2, len(bad)))] = int(rng.integers(0, 256))
        st, err, rgb = C.jpeg_decode_host(bytes(bad), progressive=bool(it & 1))
        seen[st] += 1
        assert (rgb is not None) == (st == "ok")
        assert C.jpeg_coefs(bytes(bad), compact=True, progressive=bool(it & 1))["status"] == st
    assert seen["ok"] and seen["corrupt"] + seen["unsupported"]


@pytest.mark.parametrize("jpeg_device", [True, False])
def test_ingest_counts_the_new_layouts_as_native(jpeg_device):
    """AsyncBatcher.run_jpeg (the model server's IMAGE_BYTES path) over an echo instance: uploads in the new layouts
    are decoded by the ingest, not by the caller's decoder, and answer as their PIL pixels do."""
    import asyncio
    import types

    from inference_arena_amd.server.batching import AsyncBatcher

    C = native()
    runner = types.SimpleNamespace(ex=C.EchoInstance(2, 8, 4, 200))
    b = AsyncBatcher([runner], max_batch=8, max_queue_delay_us=500)
    if not jpeg_device:
        b._ingest = C.JpegIngest(b._b, {"threads": 2, "jpeg_device": False})
    want = ("440_37x53", "411_37x53", "410_33x17", "2x4_17x33", "rgb_adobe_37x53", "rgb_ids_9x7",
            "scans_y_cbcr_420_r0_37x53", "scans_cr_y_cb_440_r0_33x17")
    uploads = [dict(CASES)[k] for k in want]
    calls = []

    async def decode(data):
        calls.append(len(data))
        return L.pil(data)

    async def go():
        a = await asyncio.gather(*(b.run_jpeg(u, decode) for u in uploads))
        r = await asyncio.gather(*(b.run(L.pil(u)) for u in uploads))
        n = await b.run_jpeg(_negative_cases()["never_coded"], decode)
        return a, r, n

    try:
        a, r, n = asyncio.run(go())
        st = b.ingest_stats() if jpeg_device else None
    finally:
        b.close()
    for x, y in zip(a, r):
        np.testing.assert_array_equal(x["det"], y["det"])
        np.testing.assert_array_equal(x["topk_idx"], y["topk_idx"])
    assert calls == [len(_negative_cases()["never_coded"])] and n["det_count"] >= 1
    if st is not None:
        assert st["native"] == len(uploads) and st["fallback"] == 1 and st["errors"] == 0


def test_layout_check_under_address_sanitizer(tmp_path):
    """csrc/tests/jpeg_layout_check.cpp: jpeg_parse, the dense and the compact decode and jpeg_coefs_to_rgb built
    host-only with AddressSanitizer and UndefinedBehaviorSanitizer, run as a program of its own over files of every
    new layout and over seeded mutations of them (frame header, scan headers, scans dropped / repeated / swapped,
    truncation), every buffer at exactly its stated size.  The files with crafted coefficients of jpeg_range_cases.py
    are seeds too: the dense and the compact decode agree on which side of the coefficient range a file lies."""
    import os
    import shutil
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (Path(hipcc).exists() or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    srcs = [root / "csrc" / "tests" / "jpeg_layout_check.cpp", root / "csrc" / "runtime" / "jpeg_decode.cpp"]
    exe = root / "build" / "jpeg_layout_check_asan"
    exe.parent.mkdir(parents=True, exist_ok=True)
    newest = max(p.stat().st_mtime for p in srcs + [root / "csrc" / "runtime" / "jpeg_decode.h",
                                                   root / "csrc" / "kernels" / "jpeg_math.h",
                                                   root / "csrc" / "kernels" / "jpeg_desc.h"])
    if not exe.exists() or exe.stat().st_mtime < newest:
        cmd = [hipcc, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Xarch_host",
               "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
               "-I" + str(root / "csrc"), *map(str, srcs), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
    want = ("440_37x53", "440_h2_33x17", "411_37x53", "410_17x33", "311_9x7", "1x4_3x101", "2x4_101x3",
            "rgb_adobe_16x16", "rgb_ids_1x1", "scans_y_cb_cr_444_r3_37x53", "scans_y_cbcr_420_r0_33x17",
            "scans_cr_y_cb_440_r0_17x33", "411_r2_37x53")
    seeds = []
    for k in want:
        p = tmp_path / f"{k}.jpg"
        p.write_bytes(dict(CASES)[k])
        seeds.append(str(p))
    p = tmp_path / "prog_410.jpg"
    p.write_bytes(L.write(L.scene(37, 53, 5), L.SAMPLINGS["410"][0], progressive=True))
    seeds.append(str(p))
    import jpeg_range_cases as R

    crafted = [c for c in R.inside() if c.blocks is not None and not c.name.startswith("random_")]
    crafted += [c for c in R.inside() if c.name.endswith("_0") and c.name.startswith("random_")]
    crafted += list(R.outside())
    seeds.append("--range")
    for c in crafted:
        p = tmp_path / f"{c.name}.jpg"
        p.write_bytes(c.data)
        seeds.append(str(p))
    r = subprocess.run([str(exe), "240", *seeds], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    report = r.stdout + r.stderr
    assert "Sanitizer" not in report and "runtime error" not in report and r.returncode == 0, report[-6000:]
    assert "jpeg_layout_check: ok" in r.stdout
    n_out = len(R.outside())
    assert f"{len(crafted) - n_out} + {n_out} of them in and beyond the coefficient range" in r.stdout, r.stdout
