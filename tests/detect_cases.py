"""Inputs and host oracles shared by the detector-tail tests (test_detect_cases.py, test_detect_tail_gpu.py):
crafted NMS candidates whose greedy pass cannot depend on fp32 rounding, a tiny decode pyramid with hand-placed
class and DFL logits, and the packing of the records the kernels read and write (csrc/kernels/launch.h)."""
from __future__ import annotations

import functools

import numpy as np
import torch

import tie_image as ti
from inference_arena_amd.models.yolov5nu import Detect
from inference_arena_amd.ops import functional as AF
from inference_arena_amd.postprocess import apply_nms
from inference_arena_amd.processing import scale_boxes
from inference_arena_amd.processing.transforms import letterbox_geometry

IOU_THR = 0.45
CONF_THR = 0.5
T = 640
SENTINEL = -0x5A5A5A5B  # int32 fill of buffers a kernel must leave alone (0xA5A5A5A5: a huge negative float)

# ------------------------------------------------------------------ NMS
SCORES = (0.5 + np.arange(17) / 32.0).astype(np.float32)  # 17 exact values in [0.5, 1.0]: heavy ties
GEOMETRIES = [(480, 640), (720, 1280), (600, 800), (300, 200), (1000, 300)]  # (h, w) of the original images
ALL_CLASSES = tuple(range(80))

# name -> per image (candidate count, classes drawn from); image i uses GEOMETRIES[i % 5].  The counts sit
# on both sides of the powers of two the bitonic sort pads to; a single class above 1024 members makes the
# suppression sweep stride; 8400 is the program's cand_cap.
NMS_LAUNCHES = {
    "counts": [(0, (0,)), (1, (79,)), (2, (0, 79)), (3, (0, 79)), (1023, (3, 4, 5)), (1024, (79,)), (1025, (0,)),
               (2048, (0, 79)), (2049, (17,)), (8400, ALL_CLASSES)],
    "overflow": [(2049, (0,)), (8400, ALL_CLASSES), (1025, (79,))],
    # box origins confined to a 64-px window, so that most candidates are suppressed.  Every member of a class then
    # overlaps every other, and the share of candidates with a partner near the IoU threshold grows with the size of
    # the class (11 % at 1100 members); at most ~130 members per class keep the margin filter below its 2 % limit.
    "dense": [(0, (0,)), (1, (79,)), (2, (79,)), (3, (0,)), (1023, tuple(range(0, 80, 8))),
              (1024, tuple(range(72, 80))), (1025, tuple(range(10))), (2048, tuple(range(0, 80, 4))),
              (2049, tuple(range(60, 80))), (8400, ALL_CLASSES)],
}


@functools.lru_cache(maxsize=None)
def nms_launch(name):
    """The cases of one launch, one per image, built once and shared by the tests (which leave them unchanged)."""
    base = 1000 * sorted(NMS_LAUNCHES).index(name)
    return [nms_case(n, classes, base + i, name == "dense") for i, (n, classes) in enumerate(NMS_LAUNCHES[name])]


def nms_case(n, classes, seed, dense=False):
    """n candidates in anchor order: xyxy boxes on a 4-px grid in [0, 640] (every product and sum of the IoU is
    then exact in fp32), scores from SCORES, unique ascending anchors.  dense: box origins confined to a 64-px
    window, so that most candidates are suppressed.  Pairs of one class whose fp64 IoU lies within 1e-4 of the
    threshold lose their later member (margin_keep) before anything is returned; `filtered` is the share of the
    draw that this removed."""
    rng = np.random.default_rng(seed)
    m = n + n // 16 + 8
    if dense:
        x1 = 288 + 4 * rng.integers(0, 16, m)
        y1 = 288 + 4 * rng.integers(0, 16, m)
    else:
        x1 = 4 * rng.integers(0, 159, m)
        y1 = 4 * rng.integers(0, 159, m)
    x2 = np.minimum(x1 + 4 * rng.integers(2, 25, m), T)
    y2 = np.minimum(y1 + 4 * rng.integers(2, 25, m), T)
    boxes = np.stack([x1, y1, x2, y2], 1).astype(np.float32)
    cls = np.asarray(classes, np.int32)[rng.integers(0, len(classes), m)]
    scores = SCORES[rng.integers(0, len(SCORES), m)]
    ok = margin_keep(boxes, cls)
    filtered = 1.0 - ok.sum() / m
    boxes, cls, scores = boxes[ok][:n], cls[ok][:n], scores[ok][:n]
    assert len(boxes) == n, "margin filter removed more than the spare candidates"
    anchors = np.sort(rng.choice(8400, n, replace=False)).astype(np.int32)
    return {"boxes": boxes, "cls": cls, "scores": scores, "anchors": anchors, "filtered": filtered}


def _pair_iou64(b, rows):
    iw = np.clip(np.minimum(b[rows, None, 2], b[None, :, 2]) - np.maximum(b[rows, None, 0], b[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(b[rows, None, 3], b[None, :, 3]) - np.maximum(b[rows, None, 1], b[None, :, 1]), 0, None)
    inter = iw * ih
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (area[rows, None] + area[None, :] - inter + 1e-6)


def margin_keep(boxes, cls, thr=IOU_THR, margin=1e-4):
    """Mask that drops the later member of every same-class pair with |IoU - thr| < margin (IoU in fp64)."""
    b = boxes.astype(np.float64)
    keep = np.ones(len(b), bool)
    for c in np.unique(cls):
        idx = np.nonzero(cls == c)[0]
        bb = b[idx]
        for s in range(0, len(idx), 512):
            rows = np.arange(s, min(s + 512, len(idx)))
            near = np.abs(_pair_iou64(bb, rows) - thr) < margin
            near &= np.arange(len(idx))[None, :] > rows[:, None]
            keep[idx[near.any(0)]] = False
    return keep


def to_cxcywh(xyxy):
    return np.stack([(xyxy[:, 0] + xyxy[:, 2]) / 2, (xyxy[:, 1] + xyxy[:, 3]) / 2, xyxy[:, 2] - xyxy[:, 0],
                     xyxy[:, 3] - xyxy[:, 1]], 1).astype(xyxy.dtype)


def nms_keep(case):
    """The project's host NMS on the case (candidates in anchor order), ordered by class, score, anchor."""
    keep = np.asarray(apply_nms(to_cxcywh(case["boxes"]), case["scores"], case["cls"], CONF_THR, IOU_THR), np.int64)
    if len(keep):
        keep = keep[np.lexsort((case["anchors"][keep], -case["scores"][keep], case["cls"][keep]))]
    return keep


def nms_keep_f64(case):
    """The same greedy pass written out in fp64."""
    b = case["boxes"].astype(np.float64)
    keep = []
    for c in np.unique(case["cls"]):
        order = np.nonzero(case["cls"] == c)[0]
        order = order[np.argsort(-case["scores"][order].astype(np.float64), kind="stable")]
        while order.size:
            i, order = order[0], order[1:]
            keep.append(int(i))
            if order.size:
                pair = np.concatenate([[i], order])
                order = order[_pair_iou64(b[pair], np.array([0]))[0, 1:] <= IOU_THR]
    return np.asarray(keep, np.int64)


def nms_oracle(case, hw):
    """[K, 6] fp32 = x1, y1, x2, y2 in the (h, w) original image, conf, class: apply_nms, then the xyxy form of
    the kept boxes through scale_boxes."""
    keep = nms_keep(case)
    c = to_cxcywh(case["boxes"])[keep]
    rows = np.column_stack([c[:, 0] - c[:, 2] / 2, c[:, 1] - c[:, 3] / 2, c[:, 0] + c[:, 2] / 2, c[:, 1] + c[:, 3] / 2,
                            case["scores"][keep], case["cls"][keep]]).astype(np.float32)
    if not len(rows):
        return rows.reshape(0, 6)
    scale, _, _, pw, ph = letterbox_geometry(hw[0], hw[1], T)
    return scale_boxes(rows, scale, (pw, ph), hw)


def pack_candidates(case, cap, seed):
    """[cap, 8] int32 Candidate records of the case in a random slot permutation (decode's atomics scramble the
    slots in production); slots past the case hold SENTINEL."""
    n = len(case["boxes"])
    assert n <= cap
    rec = np.full((cap, 8), SENTINEL, np.int32)
    slot = np.random.default_rng(seed).permutation(n)
    rec[slot, 0:4] = case["boxes"].view(np.int32)
    rec[slot, 4] = case["scores"].view(np.int32)
    rec[slot, 5] = case["cls"]
    rec[slot, 6] = case["anchors"]
    rec[slot, 7] = 0
    return rec


def zero_images(shapes):
    return [np.zeros((h, w, 3), np.uint8) for h, w in shapes]


# ------------------------------------------------------------------ decode
HW = (5, 3, 2)
STRIDES = (8.0, 16.0, 32.0)
A = sum(h * h for h in HW)  # 38 anchors
N_PASS = (15, 9, 6)  # passing anchors per image; image 0 overflows a cand_cap of 8
ONE_HOT_BIN = 11


def decode_inputs(dtype, seed=5):
    """[B=3, 144, A] head activations (64 DFL logits, 80 class logits) rounded to `dtype`, as fp64, and the
    anchors that carry the hand-placed cases.

    Class logits: background in [-8, -4]; chosen anchors get one or two logits of magnitude [0.25, 6], so no best
    sigmoid lies within 0.05 of the 0.5 threshold; anchors 0..3 of every image carry two classes with the same
    maximum logit (the lower index must win); one anchor holds +30 (sigmoid rounds to 1.0), one a best logit of
    -0.25 (rejected).  DFL logits: normal x 3; anchor `exact` of image 0 is one-hot (+-30) at ONE_HOT_BIN on its
    left side and flat on its right side, so its x1 and x2 are exact in fp32."""
    rng = np.random.default_rng(seed)
    x = np.empty((3, 144, A))
    x[:, :64] = rng.normal(0, 3, (3, 64, A))
    x[:, 64:] = rng.uniform(-8, -4, (3, 80, A))
    passing = []
    for b, n_pass in enumerate(N_PASS):
        chosen = rng.permutation(A)
        pos, neg = chosen[:n_pass], chosen[n_pass:n_pass + 6]
        for k, a in enumerate(pos):
            c = rng.choice(80, 2, replace=False)
            v = rng.uniform(0.25, 6)
            x[b, 64 + c[0], a] = v
            if k < 4:
                x[b, 64 + c[1], a] = v  # bit-identical maximum at two classes
            elif k % 2:
                x[b, 64 + c[1], a] = rng.uniform(0.25, v)
        for a in neg:
            x[b, 64 + rng.choice(80, 2, replace=False), a] = -rng.uniform(0.25, 6, 2)
        x[b, 64 + 79, pos[4]] = 30.0
        x[b, 64:, neg[0]] = rng.uniform(-8, -4, 80)
        x[b, 64 + 40, neg[0]] = -0.25
        passing.append(np.sort(pos))
    exact = int(passing[0][0])
    x[0, 0:16, exact] = -30.0
    x[0, ONE_HOT_BIN, exact] = 30.0
    x[0, 32:48, exact] = 1.5
    x[1, 16:32, passing[1][0]] = -30.0  # one-hot on a y side as well
    x[1, 16 + 3, passing[1][0]] = 30.0
    x[2, 48:64, passing[2][0]] = -2.25
    x = torch.from_numpy(x).to(dtype).double()
    return x, passing, exact


def split_levels(x):
    """[B, 144, A] -> the three NCHW maps [B, 144, h, h]."""
    out, o = [], 0
    for h in HW:
        out.append(x[:, :, o:o + h * h].reshape(x.shape[0], 144, h, h))
        o += h * h
    return out


_detect = None


def decode_oracle(x):
    """Detect().decode of the maps in the precision of `x`: [B, 84, A] = cx, cy, w, h, 80 sigmoid scores."""
    global _detect
    if _detect is None:
        _detect = Detect()
    det = _detect.double() if x.dtype == torch.float64 else _detect.float()
    with torch.no_grad():
        return det.decode(split_levels(x)).numpy()


def raw_to_xyxy(raw):
    cx, cy, w, h = raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3]
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)


def decode_tolerances(x):
    """(score, pixel) largest |fp32 - fp64| of torch's decode on these inputs, over the raw output and the xyxy
    boxes derived from it."""
    r64 = decode_oracle(x)
    r32 = decode_oracle(x.float())
    d_score = np.abs(r32[:, 4:].astype(np.float64) - r64[:, 4:]).max()
    d_px = max(np.abs(r32[:, :4].astype(np.float64) - r64[:, :4]).max(),
               np.abs(raw_to_xyxy(r32).astype(np.float64) - raw_to_xyxy(r64)).max())
    return float(d_score), float(d_px)


def nhwc_heads(x, dtype, xs, device):
    """Device head maps [B, h, h, xs] of element type `dtype`; channels past 144 hold a sentinel value."""
    out = []
    for m in split_levels(x):
        t = torch.full((m.shape[0], m.shape[2], m.shape[3], xs), 77.0, dtype=dtype)
        t[..., :144] = m.permute(0, 2, 3, 1).to(dtype)
        out.append(t.to(device))
    return out


# ------------------------------------------------------------------ space-to-depth
def nchw_to_s2d(x):
    """[B, 3, 2h, 2w] -> [B, h, w, 16] space-to-depth, channel (p * 2 + q) * 3 + c, 12..15 zero: the inverse of
    AF.s2d_to_nchw."""
    B, _, H, W = x.shape
    y = x.reshape(B, 3, H // 2, 2, W // 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(B, H // 2, W // 2, 12)
    return torch.cat([y, torch.zeros(B, H // 2, W // 2, 4, dtype=x.dtype)], 3)


def tensor_pool(x):
    """fp32 NCHW tensors in a byte pool at 256-byte-aligned offsets with a gap in front of each -> (meta, pool)."""
    B, _, S, _ = x.shape
    metas, chunks, off = [], [], 0
    for b in range(B):
        gap = 256 * (b + 1)
        data = x[b].contiguous().numpy().tobytes()
        pad = (-len(data)) % 256
        metas.append(AF.IMAGE_META.pack(off + gap, S, S, S, S, 0, 0, 1.0))
        chunks.append(b"\xa5" * gap + data + b"\xa5" * pad)
        off += gap + len(data) + pad
    return b"".join(metas), np.frombuffer(b"".join(chunks), dtype=np.uint8)


# ------------------------------------------------------------------ crops
def crop_images():
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:450, 0:450]
    checker = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    # image 2: the tie image (tie_image.py) of a 464 -> 224 resize (scale 29/14 on both axes)
    big = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    return [checker, big, np.array(ti.tie_image(464, 464, 224, 224, 0, 1)),
            rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)]


# (image, x1, y1, x2, y2): w x h = 1x1, 1x40, 40x1, 2x2, 3x5, 223, 224 (the identity), 225, 448 (every tap at weight
# 0.5: on the checkerboard, and on random pixels where the sums land on x.5 with even and odd x), a crop that ends
# at the last row and column of the last image of the pool, the whole tie image (about 1,500 of its 150,528 resized
# samples sit on a uint8 rounding tie of the host arithmetic), and the two kinds of empty crop
CROPS = [(1, 7, 9, 8, 10), (1, 601, 3, 602, 43), (1, 11, 470, 51, 471), (3, 51, 35, 53, 37), (3, 3, 5, 6, 10),
         (1, 100, 50, 323, 273), (1, 416, 256, 640, 480), (1, 1, 2, 226, 227), (0, 1, 1, 449, 449),
         (1, 33, 17, 481, 465), (3, 30, 20, 53, 37), (2, 0, 0, 464, 464), (1, 50, 10, 50, 30), (3, 5, 30, 25, 12)]


def pack_crops(crops=CROPS):
    rec = np.zeros((len(crops), 8), np.int32)
    for i, (img, x1, y1, x2, y2) in enumerate(crops):
        rec[i, :6] = (img, x1, y1, x2, y2, i)
    return rec


def host_crop(images, crop):
    img, x1, y1, x2, y2 = crop
    if x2 <= x1 or y2 <= y1:
        return np.zeros((1, 1, 3), np.uint8)  # extract_crop's black 1x1
    return images[img][y1:y2, x1:x2].copy()
