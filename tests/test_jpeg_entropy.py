"""Host side of the device entropy coder (``ARENA_CROP_ENTROPY=gpu``), without a GPU.

* the crafted cases (entropy_cases.py) have, on the oracle's bytes (``jpeg_write``), the properties the GPU tests rely
  on: heavy byte stuffing, a stuffed padded last byte, overflow of the default reserve, zero runs above 15, no EOB;
* ``jpeg_entropy_phased_host`` — the functions of csrc/kernels/jpeg_huff_math.h run through the device coder's size,
  scan, emit and stuff phases on the CPU — equals ``jpeg_write`` on every crafted case and on 50 random crops;
* the per-slot sizes (``block_bits``) sum to the oracle's unstuffed scan; header + scan + EOI is ``jpeg_write``;
* the setting, the env template, the Python wrapper and the detection service hand the mode through;
* the stand-alone check csrc/tests/jpeg_entropy_check.cpp runs clean under AddressSanitizer + UBSan.
"""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import entropy_cases as ec
from inference_arena_amd.ops import native
from inference_arena_amd.utils.settings import Settings

ROOT = Path(__file__).resolve().parents[1]
CASES = ec.cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def oracle():
    """id -> jpeg_write's bytes, computed once."""
    C = native()
    return {cid: C.jpeg_write(w, h, coefs) for cid, w, h, _, coefs in CASES}


def _unstuffed(scan: bytes) -> bytes:
    assert scan.count(b"\xff") == scan.count(b"\xff\x00")  # no marker inside the scan
    return scan.replace(b"\xff\x00", b"\xff")


# ---- the cases exercise what they are meant to ------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "sparse" and c[1] >= 16], ids=lambda c: c[0])
def test_sparse_mix_stuffs_adjacent_bytes_and_fits_the_reserve(case, oracle):
    cid, w, h, _, coefs = case
    scan = ec.scan_of(oracle[cid])
    pairs, per_slot = scan.count(b"\xff\x00\xff\x00"), len(scan) / ec.blocks(w, h)
    print(f"{cid}: {pairs} adjacent stuffed pairs, {per_slot:.1f} bytes per slot")
    assert pairs >= 5
    assert per_slot < 128


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "plus"], ids=lambda c: c[0])
def test_all_plus_1023_overflows_the_reserve_and_ends_in_a_stuffed_byte(case, oracle):
    cid, w, h, _, coefs = case
    scan = ec.scan_of(oracle[cid])
    per_slot = len(scan) / ec.blocks(w, h)
    print(f"{cid}: {per_slot:.1f} bytes per slot, last bytes {scan[-2:].hex()}")
    assert per_slot > 128
    assert scan[-2:] == b"\xff\x00"  # the padded last byte is 0xFF and stuffed: FF 00 right before EOI


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "runs"], ids=lambda c: c[0])
def test_runs_blocks_have_long_zero_runs_and_no_eob(case):
    _, _, _, _, coefs = case
    for blk in coefs:
        nz = np.flatnonzero(blk[1:]) + 1
        assert blk[63] != 0
        assert np.diff(np.concatenate([[0], nz])).max() - 1 >= 16


def test_cases_stay_in_the_domain_and_the_binding_rejects_what_does_not():
    C = native()
    for _, _, _, _, coefs in CASES:
        assert coefs.dtype == np.int16 and np.abs(coefs.astype(np.int32)).max() <= 1023
    bad = np.zeros((6, 64), np.int16)
    bad[3, 17] = 1024
    with pytest.raises(ValueError, match="1023"):
        C.jpeg_entropy_phased_host(16, 16, bad)
    with pytest.raises(ValueError, match="count"):
        C.jpeg_entropy_phased_host(17, 16, bad)


# ---- the phased coder against the serial one ----------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_phased_host_coder_equals_jpeg_write_on_crafted_coefficients(case, oracle):
    C = native()
    cid, w, h, _, coefs = case
    assert C.jpeg_entropy_phased_host(w, h, coefs) == oracle[cid]
    nat = np.zeros_like(coefs)
    nat[:, ZZ] = coefs
    assert C.jpeg_entropy_phased_host(w, h, nat, natural=True) == oracle[cid]


ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
      28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
      47, 55, 62, 63]  # zigzag index -> natural index


def test_phased_host_coder_equals_jpeg_write_on_random_crops():
    C = native()
    crops = ec.random_crops(50)
    assert len(crops) == 50
    for crop in crops:
        h, w = crop.shape[:2]
        coefs = C.jpeg_encode_coefs_host(crop)
        want = C.jpeg_write(w, h, coefs)
        assert want == C.jpeg_encode_host(crop)
        assert C.jpeg_entropy_phased_host(w, h, coefs) == want, f"{w}x{h}"
        assert C.jpeg_entropy_phased_host(w, h, C.jpeg_encode_coefs_host(crop, zigzag=False), natural=True) == want


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_block_bits_sum_to_the_oracles_unstuffed_scan(case, oracle):
    """The oracle's scan, unstuffed, is ceil(bits / 8) bytes long and ends in 8 * bytes - bits padding 1-bits."""
    C = native()
    cid, w, h, _, coefs = case
    bits = C.jpeg_block_bits(w, h, coefs)
    assert bits.shape == (ec.blocks(w, h),) and bits.min() >= 2  # the shortest slot: a 2-bit DC code and ... EOB
    total = int(bits.astype(np.int64).sum())
    raw = _unstuffed(ec.scan_of(oracle[cid]))
    assert len(raw) == (total + 7) // 8
    pad = 8 * len(raw) - total
    assert raw[-1] & ((1 << pad) - 1) == (1 << pad) - 1
    assert int(bits.max()) <= 1660  # jpeg_huff_math.h kMaxBlockBits sizes the device buffers


@pytest.mark.parametrize("case", CASES[:12], ids=IDS[:12])
def test_header_scan_and_eoi_make_jpeg_write(case, oracle):
    C = native()
    cid, w, h, _, _ = case
    head = C.jpeg_write_header(w, h)
    data = oracle[cid]
    assert data == head + ec.scan_of(data) + b"\xff\xd9"
    assert head[:2] == b"\xff\xd8" and head[-14:-12] == b"\xff\xda"
    # only the SOF0 size differs between crops (the device path patches a cached header)
    other = C.jpeg_write_header(640, 333)
    diff = [i for i, (a, b) in enumerate(zip(head, other)) if a != b]
    assert len(other) == len(head) and set(diff) <= {163, 164, 165, 166}
    assert other[163:167] == (333).to_bytes(2, "big") + (640).to_bytes(2, "big")


# ---- setting and wiring -------------------------------------------------------------------------------------------------

def test_setting_default_and_env_template():
    assert Settings().ARENA_CROP_ENTROPY == "host"
    assert Settings.from_env(PORT=None).ARENA_CROP_ENTROPY == os.environ.get("ARENA_CROP_ENTROPY", "host")
    lines = [ln for ln in (ROOT / ".env.example").read_text().splitlines() if "=" in ln]
    keys = [ln.split("=", 1)[0].strip() for ln in lines]
    assert keys.index("ARENA_CROP_ENTROPY") == keys.index("ARENA_CROP_DECODE") + 1
    assert lines[keys.index("ARENA_CROP_ENTROPY")].split("=", 1)[1].split()[0] == "host"


def test_wrapper_passes_the_mode_to_the_native_encoder(monkeypatch):
    from inference_arena_amd import ops
    from inference_arena_amd.server import crop_codec

    seen = []

    class FakeModule:
        @staticmethod
        def CropJpegEncoder(device, capacity_bytes, threads, entropy="host"):
            seen.append((device, capacity_bytes, threads, entropy))
            return object()

    monkeypatch.setattr(ops, "native", lambda: FakeModule)
    assert crop_codec.GpuCropEncoder(device=3, entropy="gpu").entropy == "gpu"
    assert crop_codec.GpuCropEncoder(device=1, capacity_bytes=512, threads=4).entropy == "host"
    assert seen == [(3, 0, 2, "gpu"), (1, 512, 4, "host")]
    with pytest.raises(ValueError, match="entropy"):
        crop_codec.GpuCropEncoder(entropy="fast")
    assert len(seen) == 2


def test_service_with_the_gpu_entropy_setting_sends_the_bytes_of_the_pil_setting(monkeypatch):
    """create_app with ARENA_CROP_ENCODE=gpu and ARENA_CROP_ENTROPY=gpu builds its encoder in that mode (a fake one
    here, over the host encoder) and the RPCs carry the bytes the default settings send."""
    import test_jpeg_encode as te
    from inference_arena_amd.data.synthetic import encode_jpeg, synthetic_images
    from inference_arena_amd.server import crop_codec
    from inference_arena_amd.server.detection_service import create_app
    from inference_arena_amd.server.multipart import encode_multipart

    body, ctype = encode_multipart("file", encode_jpeg(synthetic_images(1, 5)[0]))
    slot_bytes = 640 * 640 * 3
    mem0 = te.FakeDeviceMemory(slot_bytes)
    cl0 = te._client()
    out0, _ = te._post(create_app(Settings(LOG_LEVEL="WARNING"), detector=te.SplitDetector(mem0), client=cl0), body, ctype)
    assert out0[0].status_code == 200 and len(cl0.stub.sent) == 4

    mem = te.FakeDeviceMemory(2 * slot_bytes)
    built = []

    class FakeGpuCropEncoder(te.HostEncoder):
        def __init__(self, device=0, entropy="host"):
            super().__init__(mem)
            built.append((device, entropy))

        async def encode(self, frame_ptr, h, w, det, frame_bytes=0):
            return await self.submit(frame_ptr, h, w, det, frame_bytes)

        def close(self):
            built.append("closed")

    monkeypatch.setattr(crop_codec, "GpuCropEncoder", FakeGpuCropEncoder)
    s = Settings(LOG_LEVEL="WARNING", ARENA_CROP_ENCODE="gpu", ARENA_CROP_ENTROPY="gpu", ARENA_DEVICE="gpu", ARENA_GPU=0)
    ring, cl, det = te._ring(mem, 2, slot_bytes), te._client(), te.SplitDetector(mem)
    out, dec = te._post(create_app(s, detector=det, client=cl, ring=ring), body, ctype, n=2)
    for r in out:
        assert r.status_code == 200, r.text
        assert r.json()["detections"] == out0[0].json()["detections"]
    assert built == [(0, "gpu"), "closed"]
    assert te._sent(cl) == sorted(cl0.stub.sent * 2) and dec.calls == 0 and det.exports == 2
    # and the default mode is handed through as such
    built.clear()
    s = Settings(LOG_LEVEL="WARNING", ARENA_CROP_ENCODE="gpu", ARENA_DEVICE="gpu", ARENA_GPU=0)
    te._post(create_app(s, detector=te.SplitDetector(mem), client=te._client(), ring=te._ring(mem, 2, slot_bytes)), body, ctype)
    assert built == [(0, "host"), "closed"]


# ---- memory safety of the phased coder ------------------------------------------------------------------------------------

def test_entropy_check_under_address_and_ub_sanitizers():
    """csrc/tests/jpeg_entropy_check.cpp, built host-only with -fsanitize=address,undefined: the phased coder against
    jpeg_write on 300 random crops of 1..70 pixels a side and on the crafted coefficient sets, without a report."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (Path(hipcc).exists() or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    srcs = [ROOT / "csrc" / "tests" / "jpeg_entropy_check.cpp", ROOT / "csrc" / "runtime" / "jpeg_encode.cpp"]
    hdrs = [ROOT / "csrc" / "runtime" / "jpeg_encode.h", ROOT / "csrc" / "kernels" / "jpeg_enc_math.h",
            ROOT / "csrc" / "kernels" / "jpeg_huff_math.h", ROOT / "csrc" / "kernels" / "jpeg_math.h",
            ROOT / "csrc" / "kernels" / "jpeg_enc_desc.h"]
    exe = ROOT / "build" / "jpeg_entropy_check_asan"
    exe.parent.mkdir(parents=True, exist_ok=True)
    if not exe.exists() or exe.stat().st_mtime < max(p.stat().st_mtime for p in srcs + hdrs):
        cmd = [hipcc, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Xarch_host", "-fsanitize=address,undefined",
               "-I" + str(ROOT / "csrc"), *map(str, srcs), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe), "300", "7"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    report = r.stdout + r.stderr
    assert "Sanitizer" not in report and "runtime error" not in report and r.returncode == 0, report[-6000:]
    assert "jpeg_entropy_check: ok" in r.stdout
