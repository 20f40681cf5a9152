"""The coefficient range of the split JPEG decoder (kCoefRangeLimit, csrc/kernels/jpeg_math.h) on CPU.

Every other JPEG the suite decodes was encoded from pixels, and such coefficients stay in a narrow range.  A valid file
can carry any coefficients its Huffman tables can code; on large ones PIL (libjpeg-turbo's SIMD IDCT, 16-bit lanes),
exact arithmetic and the kernels' int32 arithmetic part ways.  The decode functions therefore hand back every file
with a block whose S = sum |c_k| * q_k passes the limit.  jpeg_range_cases.py writes files on both sides of it; here

* on every outside file the decoder's arithmetic without the check (a numpy port of jpeg_math.h) differs from PIL:
  what the decoder answered with before it had the check, and the reason the cases are not vacuous;
* on every inside file the same arithmetic, in int32 and in int64, equals PIL, and so does the decoder;
* both decode functions say "unsupported" for every outside file and "ok" for every inside one, single-scan,
  multi-scan and progressive alike, and the ingest sends the outside ones to the caller's decoder."""
from __future__ import annotations

import numpy as np
import pytest

import jpeg_layout_cases as L
import jpeg_range_cases as R
from inference_arena_amd.ops import native

INSIDE = R.inside()
OUTSIDE = R.outside()
CRAFTED = [c for c in INSIDE if c.blocks is not None]


def test_the_case_lists_are_complete():
    """PIL refuses none of the files, and the lists hold what they promise."""
    names = [c.name for c in INSIDE]
    assert len(OUTSIDE) == 8 and len(set(names)) == len(names)
    lim = R.limit()
    for kind in R.KINDS:  # at least 400 random blocks per kind, luma and chroma, 4:4:4 and 4:2:0, just under the limit
        for lay in ("444", "420"):
            files = [c for c in INSIDE if c.name.startswith(f"random_{kind}_{lay}_")]
            sums = np.concatenate([R.block_sums(b, c.qt[0 if k == 0 else 1]).ravel()
                                   for c in files for k, b in enumerate(c.blocks)])
            assert len(files) == 3 and (sums <= lim).all() and (sums > lim - 128).all()  # within one quantiser step
        assert sum(np.asarray(b).shape[0] * np.asarray(b).shape[1] for c in INSIDE
                   if c.name.startswith(f"random_{kind}_") for b in c.blocks) >= 400
    for c in INSIDE:
        if c.name.startswith("at_limit"):
            sums = [R.block_sums(b, c.qt[0 if k == 0 else 1]) for k, b in enumerate(c.blocks)]
            assert max(s.max() for s in sums) == lim
    assert R.worst_sum(dict((c.name, c) for c in OUTSIDE)["limit_plus_1"]) == lim + 1
    # the extreme real images: seven contents less the one that is beyond the range, five qualities, two samplings
    assert sum(c.blocks is None for c in INSIDE) == 6 * 5 * 2 and len(R.beyond()) == 5 * 2


def test_the_gain_the_proof_rests_on():
    """G of the proof in jpeg_math.h: the largest weight of an input in an output of idct8 before its descale."""
    unit = np.eye(8, dtype=np.int64) << 20  # large enough that the descale's rounding does not matter
    w = R.idct8(unit, 11).astype(np.float64) * 2048 / (1 << 20)
    assert round(float(np.abs(w).max())) == 11363
    assert R.limit() == ((1 << 15) - 2) * (1 << 11) // 11363


def test_the_writer_codes_the_blocks_it_is_given():
    C = native()
    for c in CRAFTED:
        got = C.jpeg_coefs(c.data)
        assert got["status"] == "ok", (c.name, got["error"])
        for k, comp in enumerate(got["comps"]):
            n = comp["bw"] * comp["bh"] * 64
            blk = got["coef"][comp["coef_off"]:comp["coef_off"] + n].reshape(comp["bh"], comp["bw"], 64)
            np.testing.assert_array_equal(blk[:, :, R._NAT_OF_ZZ], np.asarray(c.blocks[k]), err_msg=c.name)


@pytest.mark.parametrize("case", OUTSIDE, ids=[c.name for c in OUTSIDE])
def test_outside_files_differ_from_pil_without_the_check(case):
    """The one assertion that documents the bug: the decoder's arithmetic on these coefficients is not PIL's."""
    want = L.pil(case.data)
    assert (R.port_rgb(case, np.int32) != want).any(), "the kernels' int32 arithmetic equals PIL here"
    assert R.worst_sum(case) > R.limit()


@pytest.mark.parametrize("case", OUTSIDE, ids=[c.name for c in OUTSIDE])
def test_outside_files_are_handed_back(case):
    C = native()
    st, err, rgb = C.jpeg_decode_host(case.data)
    assert st == "unsupported" and rgb is None and "16-bit IDCT" in err, (st, err)
    dense, compact = C.jpeg_coefs(case.data), C.jpeg_coefs(case.data, compact=True)
    assert dense["status"] == compact["status"] == "unsupported"
    assert compact["error"] == dense["error"] == err


def test_inside_files_equal_pil_in_every_arithmetic():
    C = native()
    for c in INSIDE:
        want = L.pil(c.data)
        st, err, rgb = C.jpeg_decode_host(c.data)
        assert st == "ok", (c.name, err)
        np.testing.assert_array_equal(rgb, want, err_msg=c.name)
        dense, compact = C.jpeg_coefs(c.data), C.jpeg_coefs(c.data, compact=True)
        assert dense["status"] == compact["status"] == "ok", c.name
        np.testing.assert_array_equal(compact["coef"], dense["coef"], err_msg=c.name)
        if c.blocks is not None:
            np.testing.assert_array_equal(R.port_rgb(c, np.int32), want, err_msg=f"{c.name}: int32 port vs PIL")
            np.testing.assert_array_equal(R.port_rgb(c, np.int64), want, err_msg=f"{c.name}: int64 port vs PIL")


def test_the_clamp_files_reach_all_six_clamps():
    """Before its clamps ycc_to_rgb leaves 0..255 on both sides in every channel of every clamp file."""
    files = [c for c in INSIDE if c.name.startswith("clamps_")]
    assert [c.sampling[0] for c in files] == [(1, 1), (2, 1), (2, 2)]
    for c in files:
        y, cb, cr = (np.asarray(b)[..., 0].astype(np.int64) + 128 for b in c.blocks)  # DC-only, q = 8: the samples
        assert set(np.unique(y)) == set(np.unique(cb)) == set(np.unique(cr)) == {0, 255}
        rgb = L.pil(c.data).reshape(-1, 3)
        h, v = c.sampling[0]
        for my in range(cb.shape[0]):
            for mx in range(cb.shape[1]):  # the centre of every MCU is far enough from its neighbours' chroma
                yy, b, r = int(y[my * v, mx * h]), int(cb[my, mx]) - 128, int(cr[my, mx]) - 128
                raw = (yy + 1.402 * r, yy - 0.34414 * b - 0.71414 * r, yy + 1.772 * b)
                px = L.pil(c.data)[my * 8 * v + 4 * v, mx * 8 * h + 4 * h]
                assert [int(p) for p in px] == [min(255, max(0, round(t))) for t in raw], (c.name, my, mx)
        assert all({0, 255} <= set(np.unique(rgb[:, k])) for k in range(3))
    seen = set()
    for i in range(8):
        yy, b, r = 255 * (i & 1), 255 * (i >> 1 & 1) - 128, 255 * (i >> 2 & 1) - 128
        for k, t in enumerate((yy + 1.402 * r, yy - 0.34414 * b - 0.71414 * r, yy + 1.772 * b)):
            seen |= {(k, "low")} if t < 0 else {(k, "high")} if t > 255 else set()
    assert len(seen) == 6


def test_real_images_beyond_the_range_are_handed_back_not_wrong():
    """Grey 0 / 255 noise is the one PIL-encoded content here whose blocks pass the limit (S up to about 7000): it
    goes to the PIL path.  That is the price of a sufficient criterion, not a decode that would have been wrong: on
    these dense blocks the arithmetic without the check still equals PIL."""
    C = native()
    for c in R.beyond():
        assert C.jpeg_decode_host(c.data)[0] == "unsupported", c.name
        assert C.jpeg_coefs(c.data, compact=True)["status"] == "unsupported", c.name
        k = R.with_blocks(c, C.jpeg_coefs(c.data))
        assert R.limit() < R.worst_sum(k) < 8000, (c.name, R.worst_sum(k))
        np.testing.assert_array_equal(R.port_rgb(k, np.int32), L.pil(c.data), err_msg=c.name)


@pytest.mark.parametrize("how", ["scans", "progressive"])
def test_walked_files_take_the_same_check(how):
    """The same blocks in several scans and as a progressive file: checked scan by scan, or after the last scan."""
    C = native()
    kw = dict(scans=[[0], [1, 2]]) if how == "scans" else dict(progressive=True)
    by_name = {c.name: c for c in INSIDE + OUTSIDE}
    # a DC predictor that leaves int16 is the walker's own "coefficient value" hand-back in a progressive DC scan
    past = "coefficient value" if how == "progressive" else "16-bit IDCT"
    for name, want_status, message in (("at_limit_pairs", "ok", None), ("random_sparse_420_1", "ok", None),
                                       ("limit_plus_1", "unsupported", "16-bit IDCT"),
                                       ("row0_shortcut_shift", "unsupported", "16-bit IDCT"),
                                       ("dc_predictor_past_int16", "unsupported", past)):
        c = by_name[name]
        data = L.write_coefs(c.size, c.blocks, c.qt, c.sampling, pq=(1, 0) if name == "limit_plus_1" else (0, 0), **kw)
        st, err, rgb = C.jpeg_decode_host(data, progressive=True)
        assert st == want_status, (name, st, err)
        assert C.jpeg_coefs(data, compact=True, progressive=True)["status"] == want_status
        if st == "ok":
            np.testing.assert_array_equal(rgb, L.pil(data), err_msg=name)
        else:
            assert message in err, (name, err)


def test_a_damaged_file_stays_corrupt():
    """The range is reported once the scan has proved sound: a truncated outside file is corrupt, as for PIL."""
    C = native()
    c = OUTSIDE[0]
    cut = c.data[:len(c.data) - 40]
    assert C.jpeg_decode_host(cut)[0] == C.jpeg_coefs(cut, compact=True)["status"] == "corrupt"


@pytest.mark.parametrize("jpeg_device", [True, False])
def test_the_ingest_sends_outside_files_to_the_callers_decoder(jpeg_device):
    """AsyncBatcher.run_jpeg (the model server's IMAGE_BYTES path and the classification service's
    ARENA_CROP_DECODE=gpu path) over an echo instance: inside files are decoded by the ingest, outside files by the
    caller's decoder, and they answer as their PIL pixels do."""
    import asyncio
    import types

    from inference_arena_amd.server.batching import AsyncBatcher

    C = native()
    runner = types.SimpleNamespace(ex=C.EchoInstance(2, 8, 4, 200))
    b = AsyncBatcher([runner], max_batch=8, max_queue_delay_us=500)
    if not jpeg_device:
        b._ingest = C.JpegIngest(b._b, {"threads": 2, "jpeg_device": False})
    by_name = {c.name: c for c in INSIDE}
    native_uploads = [by_name[k].data for k in ("at_limit_pairs", "clamps_420", "random_dense_444_1")]
    handed_back = [c.data for c in OUTSIDE]
    calls = []

    async def decode(data):
        calls.append(data)
        return L.pil(data)

    async def go():
        a = await asyncio.gather(*(b.run_jpeg(u, decode) for u in native_uploads + handed_back))
        r = await asyncio.gather(*(b.run(L.pil(u)) for u in native_uploads + handed_back))
        return a, r

    try:
        a, r = asyncio.run(go())
        st = b.ingest_stats() if jpeg_device else None
    finally:
        b.close()
    for x, y in zip(a, r):
        np.testing.assert_array_equal(x["det"], y["det"])
        np.testing.assert_array_equal(x["topk_idx"], y["topk_idx"])
    assert sorted(calls) == sorted(handed_back)
    if st is not None:
        assert st["native"] == len(native_uploads) and st["fallback"] == len(handed_back) and st["errors"] == 0
