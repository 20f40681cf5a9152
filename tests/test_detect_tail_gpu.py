"""The detector's tail against exact host oracles (MI355X only): NMS and the crop plan on crafted candidates
(equality), decode and the raw [84, A] output on a tiny pyramid in both element types (fp64 oracle, measured
tolerance), the tensor-input rearrangement (bit for bit) and the fp32 crop gather against the host preprocessor
(same grey level at every pixel).  Inputs and oracles come from detect_cases.py; test_detect_cases.py proves on
the CPU that the NMS inputs cannot depend on fp32 rounding."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import detect_cases as dc
import tie_image as ti
from inference_arena_amd.ops import functional as AF
from inference_arena_amd.ops import native
from inference_arena_amd.processing import MobileNetPreprocessor
from inference_arena_amd.processing.mobilenet_preprocess import crop_bounds
from inference_arena_amd.processing.transforms import IMAGENET_MEAN, IMAGENET_STD, resize_bilinear

pytestmark = pytest.mark.gpu

S = dc.SENTINEL
UNTOUCHED = 12288.0  # fill of float outputs a kernel must leave alone (exact in bf16)
CAP = 8400  # the program's cand_cap: the sort pads to 16384 keys, 147 KB of LDS


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _meta(shapes, device):
    meta, _ = AF.image_meta_bytes(dc.zero_images(shapes), dc.T)
    return torch.frombuffer(bytearray(meta), dtype=torch.uint8).to(device)


def _shapes(n):
    return [dc.GEOMETRIES[i % len(dc.GEOMETRIES)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    cases = dc.nms_launch(name)
    return [dc.nms_oracle(c, hw) for c, hw in zip(cases, _shapes(len(cases)))]


# ------------------------------------------------------------------ 1. NMS
def _run_nms(name, device, max_det, n_images=None, counts=None, tail=64):
    """One nms launch over the images of NMS_LAUNCHES[name] -> det [B, max_det, 8] int32, the sentinel rows
    allocated behind the last image, det_count, and the device tensors."""
    cases = dc.nms_launch(name)
    B = len(cases)
    # 16384 sentinel records behind the last image: the sort key holds a 14-bit slot, so a sort gone wrong reads
    # sentinels (and fails the comparison), never past the allocation
    cand = np.concatenate([dc.pack_candidates(c, CAP, 40 + i) for i, c in enumerate(cases)] +
                          [np.full((16384, 8), S, np.int32)])
    cand = _dev(cand, device)
    cnt = _dev(np.asarray(counts if counts is not None else [len(c["boxes"]) for c in cases], np.int32), device)
    meta = _meta(_shapes(B), device)
    det = torch.full((B * max_det + tail, 8), S, dtype=torch.int32, device=device)
    dcnt = torch.full((B,), S, dtype=torch.int32, device=device)
    ctrl = AF.ctrl_tensor(B if n_images is None else n_images, device)
    native().nms({"cand": cand.data_ptr(), "cand_count": cnt.data_ptr(), "cand_cap": CAP, "meta": meta.data_ptr(),
                  "B": B, "iou_thr": dc.IOU_THR, "det": det.data_ptr(), "det_count": dcnt.data_ptr(),
                  "max_det": max_det, "ctrl": ctrl.data_ptr(), "stream": _stream()})
    torch.cuda.synchronize()
    d = det.cpu().numpy()
    return d[:B * max_det].reshape(B, max_det, 8), d[B * max_det:], dcnt.cpu().numpy(), (det, dcnt, meta, ctrl)


def _check_image(rows, count, want, max_det, what):
    """Equality of one image's detections with the oracle's [K, 6]; rows past the kept ones are untouched."""
    assert count == len(want), (what, count, len(want))
    k = min(len(want), max_det)
    got = rows[:k]
    assert np.array_equal(got[:, 5], want[:k, 5].astype(np.int32)), what
    assert np.array_equal(got[:, 4].view(np.float32), want[:k, 4]), what
    xy = got[:, :4].view(np.float32)
    bad = np.nonzero((xy != want[:k, :4]).any(1))[0]
    assert np.array_equal(xy, want[:k, :4]), (what, len(bad), xy[bad[:3]], want[bad[:3], :4])
    assert (got[:, 6:] == 0).all() and (rows[k:] == S).all(), what


@pytest.fixture(scope="module")
def counts_run(device):
    return _run_nms("counts", device, CAP)


def test_nms_counts_and_geometries(counts_run):
    """Candidate counts on both sides of every power of two the sort pads to, single classes above 1024 members,
    all 80 classes, five letterbox geometries with boxes reaching into the padding: every kept detection equals
    apply_nms + scale_boxes in class, score and all four coordinates."""
    det, tail, dcnt, _ = counts_run
    want = _oracle("counts")
    for b, hw in enumerate(_shapes(len(want))):
        _check_image(det[b], dcnt[b], want[b], CAP, (b, hw))
    assert (tail == S).all()
    big = want[-1]
    assert {0, 79} <= set(big[:, 5].astype(int))
    # both clamps fire at the 600x800, 300x200 and 1000x300 geometries: to 0 and to the limit of the padded side
    for b, axis in ((7, 1), (8, 0), (9, 0)):
        lim = _shapes(10)[b][1 - axis]
        assert (want[b][:, axis] == 0).any() and (want[b][:, axis + 2] == lim).any()


def test_nms_dense(device):
    """Box origins confined to a 64-px window: most candidates are suppressed."""
    det, tail, dcnt, _ = _run_nms("dense", device, CAP)
    want = _oracle("dense")
    for b, w in enumerate(want):
        _check_image(det[b], dcnt[b], w, CAP, b)
    assert (tail == S).all() and len(want[-1]) < CAP // 2


def test_nms_max_det_overflow_and_count_clamp(device):
    """max_det = 300 below every kept count; cand_count[1] above cand_cap must clamp to it.  det_count is the full
    kept count, the first 300 rows are exact, the next image's rows are its own, the tail is untouched."""
    want = _oracle("overflow")
    assert all(len(w) > 300 for w in want)
    det, tail, dcnt, _ = _run_nms("overflow", device, 300, counts=[2049, 9000, 1025])
    for b, w in enumerate(want):
        _check_image(det[b], dcnt[b], w, 300, b)
    assert (tail == S).all()


def test_nms_live_batch(device):
    """B = 3 with ctrl.n_images = 2: image 2's rows and count keep their sentinel."""
    want = _oracle("overflow")
    det, tail, dcnt, _ = _run_nms("overflow", device, 300, n_images=2)
    for b in range(2):
        _check_image(det[b], dcnt[b], want[b], 300, b)
    assert (det[2] == S).all() and dcnt[2] == S and (tail == S).all()


# ------------------------------------------------------------------ 2. crop plan
def _crop_plan(device, det, dcnt, meta, ctrl, B, max_det, rows, crop_cap, whole=0):
    crops = torch.full((rows, 8), S, dtype=torch.int32, device=device)
    native().crop_plan({"det": det.data_ptr(), "det_count": dcnt.data_ptr(), "max_det": max_det,
                        "meta": meta.data_ptr(), "B": B, "crops": crops.data_ptr(), "ctrl": ctrl.data_ptr(),
                        "crop_cap": crop_cap, "whole": whole, "stream": _stream()})
    torch.cuda.synchronize()
    return crops.cpu().numpy(), ctrl.cpu().numpy()


def test_nms_to_crop_plan_chain(device, counts_run):
    """The kept detections of the NMS launch through crop_plan: every rectangle is crop_bounds of the oracle's box
    (an ulp in the un-letterboxed coordinate becomes a different pixel rectangle here)."""
    _, _, _, (det, dcnt, meta, ctrl) = counts_run
    want = _oracle("counts")
    total = sum(len(w) for w in want)
    crops, c = _crop_plan(device, det, dcnt, meta, ctrl.clone(), len(want), CAP, total + 16, 1 << 20)
    assert c[3] == total and c[1] == total
    exp = [(b, *crop_bounds(box, *hw), d) for b, (w, hw) in enumerate(zip(want, _shapes(len(want))))
           for d, box in enumerate(w)]
    assert np.array_equal(crops[:total, :6], np.asarray(exp, np.int32))
    assert (crops[:total, 6:] == 0).all() and (crops[total:] == S).all()


def test_crop_plan_whole(device):
    """whole = 1: every live image is one crop of its full extent; the kernel writes det, det_count and crops."""
    shapes = [(300, 200), (1000, 300), (480, 640)]
    meta = _meta(shapes, device)
    det = torch.full((3, 4, 8), S, dtype=torch.int32, device=device)
    dcnt = torch.full((3,), S, dtype=torch.int32, device=device)
    crops, c = _crop_plan(device, det, dcnt, meta, AF.ctrl_tensor(2, device), 3, 4, 4, 8, whole=1)
    assert c[3] == 2 and c[1] == 2
    d = det.cpu().numpy()
    for b, (h, w) in enumerate(shapes[:2]):
        assert np.array_equal(d[b, 0, :5].view(np.float32), np.float32([0, 0, w, h, 1]))
        assert d[b, 0, 5] == -1 and (d[b, 0, 6:] == 0).all() and (d[b, 1:] == S).all()
        assert np.array_equal(crops[b], [b, 0, 0, w, h, 0, 0, 0])
    assert np.array_equal(dcnt.cpu().numpy(), [1, 1, S])
    assert (d[2] == S).all() and (crops[2:] == S).all()


@pytest.mark.parametrize("base,n_crops", [(3, 2), (6, 1), (9, 0)])
def test_crop_plan_overflow_pass(device, base, n_crops):
    """7 crops with room for 2 per pass: a later pass (ctrl.crop_base preset) gets what is left, never below 0."""
    shapes = [(300, 200), (1000, 300), (480, 640)]
    det = np.zeros((3, 4, 8), np.float32)
    det[:, :, 2:4] = 50.0
    dcnt = _dev(np.int32([3, 0, 4]), device)
    ctrl = AF.ctrl_tensor(3, device, crop_base=base)
    crops, c = _crop_plan(device, _dev(det, device), dcnt, _meta(shapes, device), ctrl, 3, 4, 12, 2)
    assert c[3] == 7 and c[1] == n_crops and c[2] == base
    assert np.array_equal(crops[:7, 0], [0, 0, 0, 2, 2, 2, 2]) and np.array_equal(crops[:7, 5], [0, 1, 2, 0, 1, 2, 3])
    assert (crops[7:] == S).all()


def test_crop_plan_truncates_toward_zero(device):
    """Coordinates below 0 and above the image: (int) truncates toward zero like Python's int() in crop_bounds."""
    shapes = [(300, 200), (1000, 300)]
    boxes = np.float32([[-3.7, -0.5, -2.2, -0.9], [-0.99, 0.99, 199.99, 299.5], [10.5, 20.5, 250.9, 1e6],
                        [199.5, 299.99, 200.0, 300.0], [-1e6, -7.5, 0.999, 1.0]])
    det = np.zeros((2, 8, 8), np.float32)
    det[:, :5, :4] = boxes
    crops, c = _crop_plan(device, _dev(det, device), _dev(np.int32([5, 5]), device), _meta(shapes, device),
                          AF.ctrl_tensor(2, device), 2, 8, 16, 16)
    assert c[3] == 10 and c[1] == 10
    exp = [(b, *crop_bounds(box, h, w), d) for b, (h, w) in enumerate(shapes) for d, box in enumerate(boxes)]
    assert np.array_equal(crops[:10, :6], np.asarray(exp, np.int32))
    assert crops[0, 3] == -2 and crops[0, 4] == 0  # x2 = int(-2.2), y2 = int(-0.9): not floored


# ------------------------------------------------------------------ 3. decode
DTYPES = [torch.float32, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def _decode_case(dtype):
    """Inputs, the fp64 oracle's raw output and the (score, pixel) bounds for `dtype`.

    The bound is a measurement: the largest |fp32 - fp64| of torch's Detect.decode on these inputs, times 4 for the
    fp32 kernel (another summation order, expf) and times 16 for the bf16 kernel (hardware exp approximation, whose
    argument scaling adds error proportional to |v - max|), never below one fp32 ulp of the largest value (2^-23 for
    a score, 2^-14 = 6.1e-5 px at 640).  Measured: fp32 inputs 6.5e-8 / 6.2e-5 px -> bounds 2.6e-7 / 2.5e-4 px;
    bf16 inputs 7.6e-8 / 8.2e-5 px -> bounds 1.2e-6 / 1.3e-3 px.  The kernels' largest errors on an MI355X were
    5.5e-8 / 4.6e-5 px (decode) and 6.5e-8 / 8.4e-5 px (yolo_raw) in fp32, 7.0e-8 / 4.0e-5 px and 7.6e-8 / 7.3e-5 px
    in bf16."""
    x, passing, exact = dc.decode_inputs(dtype)
    d_score, d_px = dc.decode_tolerances(x)
    k = 4 if dtype == torch.float32 else 16
    tol = (max(k * d_score, 2.0 ** -23), max(k * d_px, 2.0 ** -14))
    print(f"decode {dtype}: fp32-fp64 score {d_score:.3e} px {d_px:.3e} -> bounds {tol[0]:.3e} {tol[1]:.3e}")
    return x, passing, exact, dc.decode_oracle(x), tol


def _run_decode(x, dtype, xs, device, n_images=None, cap=64):
    B = x.shape[0]
    heads = dc.nhwc_heads(x, dtype, xs, device)
    cand = torch.full((B * cap + 1, 8), S, dtype=torch.int32, device=device)
    cnt = torch.zeros(B, dtype=torch.int32, device=device)
    ctrl = AF.ctrl_tensor(B if n_images is None else n_images, device)
    native().detect_decode({"head": [h.data_ptr() for h in heads], "hw": list(dc.HW), "xs": [xs] * 3,
                            "strides": list(dc.STRIDES), "B": B, "conf_thr": dc.CONF_THR, "cand": cand.data_ptr(),
                            "cand_count": cnt.data_ptr(), "cand_cap": cap, "ctrl": ctrl.data_ptr(),
                            "f32": int(dtype == torch.float32), "stream": _stream()})
    torch.cuda.synchronize()
    c = cand.cpu().numpy()
    return c[:B * cap].reshape(B, cap, 8), c[B * cap:], cnt.cpu().numpy()


def _check_records(rec, raw, tol):
    """Candidate records of one image against the fp64 oracle's raw [84, A] output, matched through the anchor."""
    a = rec[:, 6]
    assert np.array_equal(rec[:, 5], raw[4:, a].argmax(0)), "class (ties go to the lower index)"
    score = rec[:, 4].view(np.float32).astype(np.float64)
    xyxy = rec[:, :4].view(np.float32).astype(np.float64)
    e_score = np.abs(score - raw[4:, a].max(0)).max()
    e_px = np.abs(xyxy - dc.raw_to_xyxy(raw[None])[0][:, a].T).max()
    print(f"decode error: score {e_score:.3e} (bound {tol[0]:.3e}) px {e_px:.3e} (bound {tol[1]:.3e})")
    # bounds: 4x (fp32) / 16x (bf16) the measured fp32 - fp64 difference of the torch decode, see _decode_case
    assert e_score <= tol[0] and e_px <= tol[1], (e_score, e_px, tol)
    assert (rec[:, 7] == 0).all()


@pytest.mark.parametrize("xs", [144, 160])
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_tiny_pyramid(device, dtype, xs):
    x, passing, exact, raw, tol = _decode_case(dtype)
    cand, tail, cnt = _run_decode(x, dtype, xs, device)
    assert np.array_equal(cnt, dc.N_PASS)
    for b in range(3):
        rec = cand[b, :cnt[b]]
        assert np.array_equal(np.sort(rec[:, 6]), passing[b])
        _check_records(rec, raw[b], tol)
        assert (cand[b, cnt[b]:] == S).all()
    assert (tail == S).all()
    # one-hot DFL side -> its bin, flat side -> 7.5: both exact, so x1 and x2 of that anchor are exact
    r = cand[0][cand[0, :, 6] == exact][0]
    ax = exact % dc.HW[0] + 0.5
    assert r[0:1].view(np.float32)[0] == (ax - dc.ONE_HOT_BIN) * 8 and r[2:3].view(np.float32)[0] == (ax + 7.5) * 8
    best = cand[..., 4].view(np.float32)[cand[..., 6] != S]
    assert (best == 1.0).any()  # the +30 logit


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_capacity(device, dtype):
    """15 passing anchors, room for 8: the count is the full 15, the 8 stored records are distinct members of the
    passing set, the row after slot 7 is untouched."""
    x, passing, _, raw, tol = _decode_case(dtype)
    cand, tail, cnt = _run_decode(x[:1], dtype, 144, device, cap=8)
    assert cnt[0] == 15
    rec = cand[0]
    assert len(set(rec[:, 6])) == 8 and set(rec[:, 6]) <= set(passing[0])
    _check_records(rec, raw[0], tol)
    assert (tail == S).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_live_batch(device, dtype):
    x, passing, _, raw, tol = _decode_case(dtype)
    cand, tail, cnt = _run_decode(x, dtype, 144, device, n_images=2)
    assert np.array_equal(cnt, [dc.N_PASS[0], dc.N_PASS[1], 0])
    for b in range(2):
        assert np.array_equal(np.sort(cand[b, :cnt[b], 6]), passing[b])
    assert (cand[2] == S).all() and (tail == S).all()


# ------------------------------------------------------------------ 4. yolo_raw, tensor_in_s2d
@pytest.mark.parametrize("n_images", [3, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_yolo_raw(device, dtype, n_images):
    """The full [84, A] output per image against the fp64 oracle under the decode bounds; an out_stride 256 bytes
    above the image size leaves a gap that, like a dead image's rows, keeps its sentinel."""
    x, _, _, raw, tol = _decode_case(dtype)
    n = 84 * dc.A
    for xs in (144, 160):
        heads = dc.nhwc_heads(x, dtype, xs, device)
        out = torch.full((3, n + 64), S, dtype=torch.int32, device=device)
        ctrl = AF.ctrl_tensor(n_images, device)
        native().yolo_raw({"head": [h.data_ptr() for h in heads], "hw": list(dc.HW), "xs": [xs] * 3,
                           "strides": list(dc.STRIDES), "B": 3, "out": out.data_ptr(), "out_stride": (n + 64) * 4,
                           "ctrl": ctrl.data_ptr(), "f32": int(dtype == torch.float32), "stream": _stream()})
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        got = o[:n_images, :n].view(np.float32).reshape(n_images, 84, dc.A).astype(np.float64)
        e_px = np.abs(got[:, :4] - raw[:n_images, :4]).max()
        e_score = np.abs(got[:, 4:] - raw[:n_images, 4:]).max()
        print(f"yolo_raw error: score {e_score:.3e} (bound {tol[0]:.3e}) px {e_px:.3e} (bound {tol[1]:.3e})")
        assert e_score <= tol[0] and e_px <= tol[1], (e_score, e_px, tol)
        assert (o[:, n:] == S).all() and (o[n_images:] == S).all()


def test_yolo_raw_rejects_short_stride(device):
    with pytest.raises(RuntimeError, match="stride"):
        native().yolo_raw({"head": [0, 0, 0], "hw": list(dc.HW), "xs": [144] * 3, "strides": list(dc.STRIDES), "B": 1,
                           "out": 0, "out_stride": 84 * dc.A * 4 - 4, "ctrl": 0, "stream": _stream()})


@pytest.mark.parametrize("size", [8, 224])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_in_s2d(device, dtype, size):
    """fp32 NCHW tensors in the pool -> space-to-depth: the fp32 output is the host rearrangement bit for bit, the
    bf16 output its .to(bfloat16); channels 12..15 are zero; dead images are untouched."""
    x = torch.randn(3, 3, size, size, generator=torch.Generator().manual_seed(size))
    meta, pool = dc.tensor_pool(x)
    meta_t = torch.frombuffer(bytearray(meta), dtype=torch.uint8).to(device)
    pool_t = _dev(pool.copy(), device)
    want = dc.nchw_to_s2d(x).to(dtype)
    for n_images in (3, 2):
        out = torch.full((3, size // 2, size // 2, 16), UNTOUCHED, dtype=dtype, device=device)
        ctrl = AF.ctrl_tensor(n_images, device)
        native().tensor_in_s2d({"pool": pool_t.data_ptr(), "meta": meta_t.data_ptr(), "ctrl": ctrl.data_ptr(),
                                "out": out.data_ptr(), "B": 3, "S": size, "f32": int(dtype == torch.float32),
                                "stream": _stream()})
        torch.cuda.synchronize()
        got = out.cpu()
        assert torch.equal(got[:n_images], want[:n_images])
        assert (got[:n_images, ..., 12:] == 0).all() and (got[n_images:] == UNTOUCHED).all()


# ------------------------------------------------------------------ 5. crop gather
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


@pytest.fixture(scope="module")
def crop_env(device):
    """Images in a pool whose tail behind the last image is sentinel-filled, the hand-written CropRefs, the host
    oracle (resized uint8 crop and normalised tensor per crop) and the fp32 gather of all crops with ctrl null."""
    images = dc.crop_images()
    meta, pool = AF.image_meta_bytes(images, dc.T)
    last = images[-1]
    end = len(pool) - (-last.size) % 256
    pool = np.concatenate([pool[:end], np.full(len(pool) - end + 4096, 0xAB, np.uint8)])
    env = {"images": images, "pool": _dev(pool, device), "crops": _dev(dc.pack_crops(), device),
           "meta": torch.frombuffer(bytearray(meta), dtype=torch.uint8).to(device)}
    pre = MobileNetPreprocessor()
    assert pre.input_size == 224
    host = [dc.host_crop(images, c) for c in dc.CROPS]
    env["grey"] = np.stack([resize_bilinear(h, 224, 224).transpose(2, 0, 1) for h in host])
    env["norm"] = np.concatenate([pre(h).tensor for h in host])
    env["f32"] = _gather(env, torch.float32, len(dc.CROPS), None, len(dc.CROPS))
    return env


def _gather(env, dtype, cap, ctrl, rows):
    out = torch.full((rows, 112, 112, 16), UNTOUCHED, dtype=dtype, device=env["pool"].device)
    native().crop_gather_s2d({"pool": env["pool"].data_ptr(), "meta": env["meta"].data_ptr(),
                              "crops": env["crops"].data_ptr(), "ctrl": 0 if ctrl is None else ctrl.data_ptr(),
                              "out": out.data_ptr(), "cap": cap, "S": 224, "mean": MEAN,
                              "inv_std": [1 / v for v in STD], "f32": int(dtype == torch.float32),
                              "stream": _stream()})
    torch.cuda.synchronize()
    return out.cpu()


def _grey(got):
    """The uint8 level a normalised [N, 3, 224, 224] output came from."""
    std, mean = IMAGENET_STD.astype(np.float64)[:, None, None], IMAGENET_MEAN.astype(np.float64)[:, None, None]
    return np.rint((got.double().numpy() * std + mean) * 255).astype(np.int64)


def test_crop_gather_f32_equals_host(crop_env):
    """fp32 gather == MobileNetPreprocessor()(image[y1:y2, x1:x2]): the same grey level at every pixel, and the
    normalised value within 1e-6 (|v| <= 2.65, eps 1.19e-7, and the two sides round two operations differently —
    the kernel multiplies by inv_std where the host divides by std — so at most 2 * 2.65 * 1.19e-7 = 6.3e-7)."""
    out = crop_env["f32"]
    assert (out[..., 12:] == 0).all()
    got = AF.s2d_to_nchw(out)
    grey = _grey(got)
    for i, c in enumerate(dc.CROPS):
        bad = grey[i] != crop_env["grey"][i]
        assert not bad.any(), (c, int(bad.sum()), grey[i][bad][:4], crop_env["grey"][i][bad][:4])
    err = np.abs(got.numpy().astype(np.float64) - crop_env["norm"]).reshape(len(dc.CROPS), -1).max(1)
    assert (err <= 1e-6).all(), err
    # the checkerboard's 448x448 crop has every tap at weight 0.5; the identity crop returns the pixels themselves
    assert (crop_env["grey"][8] == 128).all()
    x1, y1, x2, y2 = dc.CROPS[6][1:]
    assert np.array_equal(grey[6], crop_env["images"][1][y1:y2, x1:x2].transpose(2, 0, 1))
    assert (crop_env["grey"][12:] == 0).all()  # the empty crops: extract_crop's 1x1 black
    # the tie image's crop is made of samples where fused multiply-adds round to the neighbouring grey level
    tie = crop_env["grey"][11].transpose(1, 2, 0)
    assert dc.CROPS[11][0] == 2 and (tie != ti.resize_fused(crop_env["images"][2], 224, 224)).sum() >= 20


def test_crop_gather_control_paths(crop_env):
    """ctrl.n_crops = 3 of cap = 8 leaves rows 3..7 alone; ctrl.crop_base = 2 makes row i crop 2 + i; a null ctrl
    (the fixture's launch) writes all cap rows."""
    dev = crop_env["pool"].device
    full = crop_env["f32"]
    assert (full[..., :12] != UNTOUCHED).all()
    out = _gather(crop_env, torch.float32, 8, AF.ctrl_tensor(3, dev, n_crops=3), 8)
    assert torch.equal(out[:3], full[:3]) and (out[3:] == UNTOUCHED).all()
    out = _gather(crop_env, torch.float32, 8, AF.ctrl_tensor(3, dev, n_crops=4, crop_base=2), 8)
    assert torch.equal(out[:4], full[2:6]) and (out[4:] == UNTOUCHED).all()
    out = _gather(crop_env, torch.float32, 8, None, 9)
    assert torch.equal(out[:8], full[:8]) and (out[8:] == UNTOUCHED).all()


def test_crop_gather_bf16_grey_level(crop_env):
    """bf16 gather of the same crops: the recovered grey level is within 1 of the host's (one bf16 ulp near 2.6 is
    about 0.9 grey levels)."""
    out = _gather(crop_env, torch.bfloat16, len(dc.CROPS), None, len(dc.CROPS))
    assert (out[..., 12:] == 0).all()
    diff = np.abs(_grey(AF.s2d_to_nchw(out)) - crop_env["grey"])
    assert diff.max() <= 1, diff.reshape(len(dc.CROPS), -1).max(1)
