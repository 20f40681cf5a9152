"""Head split on the GPU: the cell-mark kernel against numpy, the windowed and mark-gated x3hp conv tile by tile
against the host oracle (head_marks_needed), the chain box window -> gated box conv against the dense chain, and
whole pipelines with the split on, off and the gate off.  All comparisons are bit-exact."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from inference_arena_amd.ops import functional as AF
from inference_arena_amd.ops import native

pytestmark = pytest.mark.gpu

SENTINEL = 12288.0
MARK_SENTINEL = 77
BOX, CLS = 64, 80
B, LIVE, H, W = 3, 2, 20, 24   # the map of tests/test_head_gate_gpu.py: partial 8 x 16 tiles on both axes
TH, TW = 8, 16                  # the x3hp tile of both windows
DENSE_IMPL = 198                # kF32X3HP + 7 = conv_x3hp_kernel<9, 8, 1>, the headline's ops 47 / 50
CONSUMERS = [(145, 8, 16), (181, 8, 8)]  # fused-1x1 box conv impl, its tile


def _bdev(dev):
    return torch.tensor([LIVE], dtype=torch.int32, device=dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _marks_numpy(logits, gm32):
    """[B, ncy, ncx] int32 from [B, H, W, n] float32; NaN compares false."""
    b, h, w, _ = logits.shape
    hot = (logits >= gm32).any(axis=-1)
    ncy, ncx = -(-h // 8), -(-w // 8)
    pad = np.zeros((b, ncy * 8, ncx * 8), dtype=bool)
    pad[:, :h, :w] = hot
    return pad.reshape(b, ncy, 8, ncx, 8).any(axis=(2, 4)).astype(np.int32)


def test_mark_kernel_against_numpy():
    dev = torch.device("cuda:0")
    gm = native().head_gate_min(0.5)
    gm32 = np.float32(gm)
    below = np.nextafter(gm32, np.float32(-np.inf))
    logits = np.full((B, H, W, CLS), -9.0, dtype=np.float32)
    logits[0, 7, 7, CLS - 1] = gm32           # cell (0, 0): exactly gate_min at its last pixel and channel
    logits[0, 2, 11, 5] = below               # cell (0, 1): one float32 below it
    logits[0, 9, 1, 17] = np.nan              # cell (1, 0): NaN
    logits[0, 10, 10, 40] = np.inf            # cell (1, 1): +inf
    logits[0, H - 1, W - 1, 0] = 3.0          # cell (2, 2), partial: hot only at the map's last pixel
    # image 1: hot at (row 0, column 0).  A read of image 0's partial cells (2, x) past the bottom edge would alias
    # the first rows of this image; (row 1, column 0) is what a read past the right edge of row 0 would alias
    logits[1, 0, 0, 3] = 0.25
    logits[1, 1, 0, 0] = 0.25
    logits[2] = 5.0                           # dead: hot everywhere
    D = torch.full((B, H, W, BOX + CLS), SENTINEL, dtype=torch.float32)
    D[..., BOX:] = torch.from_numpy(logits)
    # a second, smaller level in the same launch, partial on both axes, hot in its last partial cell only
    H2, W2 = 12, 9
    l2 = np.full((B, H2, W2, CLS), -9.0, dtype=np.float32)
    l2[1, H2 - 1, W2 - 1, 79] = 1.0
    l2[2] = 5.0
    D2 = torch.full((B, H2, W2, BOX + CLS), SENTINEL, dtype=torch.float32)
    D2[..., BOX:] = torch.from_numpy(l2)
    m1 = torch.full((B, 3, 3), MARK_SENTINEL, dtype=torch.int32, device=dev)
    m2 = torch.full((B, 2, 2), MARK_SENTINEL, dtype=torch.int32, device=dev)
    Dd, D2d = D.to(dev), D2.to(dev)
    out = AF.head_mark(Dd, BOX, CLS, gm, marks=m1, bdev=_bdev(dev), levels=[(D2d, m2)])
    torch.cuda.synchronize()
    got1, got2 = out[0].cpu().numpy(), out[1].cpu().numpy()
    want1, want2 = _marks_numpy(logits, gm32), _marks_numpy(l2, gm32)
    assert want1[0].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert want1[1].tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert want2[0].sum() == 0 and want2[1].tolist() == [[0, 0], [0, 1]]
    assert np.array_equal(got1[:LIVE], want1[:LIVE]) and np.array_equal(got2[:LIVE], want2[:LIVE])
    assert np.all(got1[LIVE:] == MARK_SENTINEL) and np.all(got2[LIVE:] == MARK_SENTINEL)  # the dead image
    assert np.array_equal(Dd.cpu().numpy(), D.numpy(), equal_nan=True)  # the logits are only read


def _f_case(cin, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, cin, generator=g)
    w = torch.randn(BOX + CLS, cin, 3, 3, generator=g) * 0.05
    b = torch.randn(BOX + CLS, generator=g) * 0.1
    return x, w, b


def _f_run(case, dev, impl, packed, out=None, **kw):
    x, w, b = case
    if out is None:
        out = torch.full((B, H, W, BOX + CLS), SENTINEL, dtype=torch.float32)
    out = out.to(dev)
    AF.conv2d_nhwc(x.to(dev), w, b, act="silu", impl=impl, out=out, bdev=_bdev(dev), packed=packed, **kw)
    torch.cuda.synchronize()
    return out


# marked cells per live image: a map corner (0, 0); the opposite corner, a partial cell of a partial tile; an inner
# cell next to the partial last tiles; one in the top right
MARK_PATTERNS = [
    [[(0, 0)], [(2, 2)]],
    [[(1, 1)], [(0, 2)]],
    [[], [(1, 0)]],
]


@pytest.mark.parametrize("cin", [64, 128])
def test_windowed_and_gated_x3hp(cin):
    C = native()
    dev = torch.device("cuda:0")
    case = _f_case(cin, 3 + cin)
    packed = AF.pack_weights(case[1], case[2], dev, "fp32")
    dense = _f_run(case, dev, DENSE_IMPL, packed).cpu().numpy()
    assert np.all(dense[:LIVE] != SENTINEL) and np.all(np.isfinite(dense[:LIVE])) and np.all(dense[LIVE:] == SENTINEL)

    cls_impl, box_impl = C.HEAD_SPLIT_CLS_IMPL, C.HEAD_SPLIT_BOX_IMPL
    for impl in (cls_impl, box_impl):  # the window kernels on the whole conv: the same bits whatever the tile
        assert np.array_equal(_bits(_f_run(case, dev, impl, packed).cpu().numpy()), _bits(dense))
    # the class window: channels [64, 144) of the dense conv, the box half untouched
    got = _f_run(case, dev, cls_impl, packed, window=(BOX, BOX + CLS)).cpu().numpy()
    assert np.array_equal(_bits(got[:LIVE, ..., BOX:]), _bits(dense[:LIVE, ..., BOX:]))
    assert np.all(got[..., :BOX] == SENTINEL) and np.all(got[LIVE:] == SENTINEL)
    # the box window without marks: channels [0, 64), the class half untouched
    got = _f_run(case, dev, box_impl, packed, window=(0, BOX)).cpu().numpy()
    assert np.array_equal(_bits(got[:LIVE, ..., :BOX]), _bits(dense[:LIVE, ..., :BOX]))
    assert np.all(got[..., BOX:] == SENTINEL) and np.all(got[LIVE:] == SENTINEL)

    nty, ntx = -(-H // TH), -(-W // TW)
    seen = set()
    for pattern in MARK_PATTERNS:
        marks = np.zeros((B, 3, 3), dtype=np.int32)
        for img, cells in enumerate(pattern):
            for cy, cx in cells:
                marks[img, cy, cx] = 1
        marks[LIVE:] = 1  # the dead image is marked everywhere and still not written
        md = torch.from_numpy(marks).to(dev)
        for _, uh, uw in CONSUMERS:
            got = _f_run(case, dev, box_impl, packed, window=(0, BOX), marks=(md, uh, uw, 1)).cpu().numpy()
            assert np.all(got[..., BOX:] == SENTINEL) and np.all(got[LIVE:] == SENTINEL)
            for img in range(LIVE):
                need = np.asarray(C.head_marks_needed(marks[img], H, W, TH, TW, uh, uw, 1))
                assert need.shape == (nty, ntx)
                for ty in range(nty):
                    for tx in range(ntx):
                        t = got[img, ty * TH:(ty + 1) * TH, tx * TW:(tx + 1) * TW, :BOX]
                        ref = dense[img, ty * TH:(ty + 1) * TH, tx * TW:(tx + 1) * TW, :BOX]
                        if need[ty, tx]:
                            assert np.array_equal(_bits(t), _bits(ref)), (pattern, uh, uw, img, ty, tx)
                        else:
                            assert np.all(t == SENTINEL), (pattern, uh, uw, img, ty, tx)
                        seen.add(bool(need[ty, tx]))
            assert np.array_equal(md.cpu().numpy(), marks)  # the marks are only read
    assert seen == {False, True}


def test_window_and_marks_need_an_x3hp_kernel():
    dev = torch.device("cuda:0")
    case = _f_case(64, 5)
    packed = AF.pack_weights(case[1], case[2], dev, "fp32")
    md = torch.zeros((B, 3, 3), dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):
        _f_run(case, dev, 101, packed, window=(0, BOX))
    with pytest.raises(RuntimeError):
        _f_run(case, dev, 0, packed, marks=(md, 8, 16, 1))
    with pytest.raises(RuntimeError):  # a window that does not start on a 16-channel fragment
        _f_run(case, dev, native().HEAD_SPLIT_BOX_IMPL, packed, window=(8, BOX))
    with pytest.raises(RuntimeError):  # consumer tiles must be whole cells
        _f_run(case, dev, native().HEAD_SPLIT_BOX_IMPL, packed, window=(0, BOX), marks=(md, 4, 16, 1))
    torch.cuda.synchronize()


@pytest.mark.parametrize("impl,uh,uw", CONSUMERS)
def test_chain_box_window_then_gated_box_conv(impl, uh, uw):
    """The box half of F pre-filled with NaN, the gated box window, then the gated fused-1x1 box conv: every tile
    that conv keeps is finite and bit-equal to the dense chain, so it read nothing the box window skipped."""
    C = native()
    dev = torch.device("cuda:0")
    gm = C.head_gate_min(0.5)
    gm32 = np.float32(gm)
    case = _f_case(64, 11)
    packed = AF.pack_weights(case[1], case[2], dev, "fp32")
    g = torch.Generator().manual_seed(12)
    w2 = torch.randn(64, 64, 3, 3, generator=g) * 0.05
    b2 = torch.randn(64, generator=g) * 0.1
    wp = torch.randn(BOX, 64, 1, 1, generator=g) * 0.1
    bp = torch.randn(BOX, generator=g) * 0.1
    logits = np.full((B, H, W, CLS), -9.0, dtype=np.float32)
    logits[0, 0, 0, 1] = 2.0            # the map's first pixel
    logits[0, H - 1, W - 1, 7] = gm32   # and its last, in the partial corner tile
    logits[1, 2, 17, 70] = 1.0          # top right: this image's last tile row is read by nothing
    logits[2] = 5.0
    L = torch.full((B, H, W, BOX + CLS), SENTINEL, dtype=torch.float32)
    L[..., BOX:] = torch.from_numpy(logits)

    def box_conv(f_out, gate):
        out = L.clone().to(dev)
        AF.conv2d_nhwc(f_out, w2, b2, act="silu", impl=impl, cin=64, pw=(wp, bp), pw_out=out,
                       gate=(out, BOX, CLS, gm) if gate else None, bdev=_bdev(dev))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    dense = box_conv(_f_run(case, dev, DENSE_IMPL, packed), gate=False)
    Ld = L.to(dev)
    marks = AF.head_mark(Ld, BOX, CLS, gm, bdev=_bdev(dev))
    f0 = torch.full((B, H, W, BOX + CLS), float("nan"), dtype=torch.float32)
    f = _f_run(case, dev, C.HEAD_SPLIT_CLS_IMPL, packed, out=f0, window=(BOX, BOX + CLS))
    f = _f_run(case, dev, C.HEAD_SPLIT_BOX_IMPL, packed, out=f, window=(0, BOX), marks=(marks, uh, uw, 1))
    fh = f.cpu().numpy()
    assert np.isnan(fh[:LIVE, ..., :BOX]).any() and np.isfinite(fh[:LIVE, ..., :BOX]).any()  # some tiles skipped
    got = box_conv(f, gate=True)
    kept = 0
    for img in range(LIVE):
        for y0 in range(0, H, uh):
            for x0 in range(0, W, uw):
                keep = bool(np.any(logits[img, y0:y0 + uh, x0:x0 + uw] >= gm32))
                t, ref = got[img, y0:y0 + uh, x0:x0 + uw, :BOX], dense[img, y0:y0 + uh, x0:x0 + uw, :BOX]
                if keep:
                    assert np.all(np.isfinite(t)), (img, y0, x0)
                    assert np.array_equal(_bits(t), _bits(ref)), (img, y0, x0)
                else:
                    assert np.all(t == SENTINEL), (img, y0, x0)
                kept += keep
    assert kept == 3
    assert np.all(got[LIVE:, ..., :BOX] == SENTINEL)


def _images():
    from inference_arena_amd.data.synthetic import synthetic_images

    return synthetic_images(5, 11) + synthetic_images(1, 12, hw=(360, 520))  # the images of test_head_gate_gpu.py


def _pipeline(gate: bool, split: int, buckets):
    from inference_arena_amd.engine.pipeline import GpuPipeline
    from inference_arena_amd.models.zoo import default_models

    C = native()
    before = C.get_head_gate(), C.get_head_split()
    C.set_head_gate(gate)  # both are read when the buckets are captured
    C.set_head_split(split)
    try:
        pipe = GpuPipeline(*default_models(0), device=0, dtype="fp32", buckets=buckets)
    finally:
        C.set_head_gate(before[0])
        C.set_head_split(before[1])
    Bk = buckets[0]
    imgs = _images()
    res = pipe.infer(imgs) if Bk >= len(imgs) else [r for im in imgs for r in pipe.infer([im])]
    info = {"gated": list(pipe.ex.gated_ops(Bk)), "order": list(pipe.ex.exec_order(Bk)),
            "launches": [tuple(x) for x in pipe.ex.launch_order(Bk)], "n_ops": len(pipe.program.ops),
            "pairs": [tuple(p) for p in C.head_gate_pairs(pipe.program.ops)],
            "first": list(C.head_gate_first_convs(pipe.program.ops))}
    del pipe
    return res, info


def _assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for key in ("boxes", "scores", "classes", "topk_idx", "topk_logit"):
            assert np.array_equal(getattr(x, key), getattr(y, key)), key
        assert x.det_count == y.det_count


def _check_order(info, on):
    """The invariants of tests/test_head_gate_gpu.py: program order with each gated pair swapped."""
    n = info["n_ops"]
    want = list(range(n))
    for box in info["gated"]:
        want[box], want[box + 1] = box + 1, box
    assert sorted(info["order"]) == list(range(n)) and info["order"] == want
    assert set(info["gated"]) <= {p[0] for p in info["pairs"]}
    if not on:
        assert info["gated"] == []


def _expected_launches(info, split_pairs):
    out = []
    split_f = {info["first"][i]: info["pairs"][i] for i in split_pairs}
    for op in info["order"]:
        pair = next((p for p in split_f.values() if p[0] == op), None)
        if op in split_f:
            out.append((op, 1))
        elif pair is not None:
            out += [(op, 3), (op - 1, 2), (op, 0)]
        else:
            out.append((op, 0))
    return out


@pytest.mark.parametrize("bucket", [1, 32])
def test_pipeline_split_on_off_gate_off(bucket):
    C = native()
    on, i_on = _pipeline(True, 1, [bucket])
    off, i_off = _pipeline(True, 0, [bucket])
    dense, i_dense = _pipeline(False, 1, [bucket])
    for info, gated in ((i_on, True), (i_off, True), (i_dense, False)):
        _check_order(info, gated)
    assert i_on["gated"] == [p[0] for p in i_on["pairs"]] == i_off["gated"]
    assert i_on["order"] == i_off["order"]
    assert i_off["launches"] == [(op, 0) for op in i_off["order"]]
    assert i_dense["launches"] == [(op, 0) for op in range(i_dense["n_ops"])]
    split = [0, 1] if bucket >= C.HEAD_SPLIT_MIN_BUCKET else []
    assert i_on["launches"] == _expected_launches(i_on, split)
    if bucket == 32:  # both levels split: two windows and one mark launch each
        assert sorted(k for _, k in i_on["launches"] if k) == [1, 1, 2, 2, 3, 3]
    assert sum(r.det_count for r in on) > 0
    _assert_same(on, off)
    _assert_same(on, dense)
    if not split:  # ARENA_HEAD_SPLIT=2 splits the small bucket as well, where its first convs run on x3hp tiles
        forced, i_forced = _pipeline(True, 2, [bucket])
        _check_order(i_forced, True)
        assert [op for op, k in i_forced["launches"] if k in (0, 1)] == i_forced["order"]
        _assert_same(forced, off)
