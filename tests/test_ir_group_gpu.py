"""The crop-group inverted-residual kernel (csrc/kernels/ir_group_x3.hip: stride-1 7x7 blocks, G crops per workgroup)
against fp64, against the whole-map kernel bit for bit, in a hidden-slice chain and in the fp32 pipeline."""
import numpy as np
import pytest
import torch

import fp32_bounds as fb
from inference_arena_amd.ops import functional as AF

pytestmark = pytest.mark.gpu
SENTINEL = -777.0


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("oup,res,G,B,live", [
    (160, True, 4, 5, None),   # a partial last group, tiles straddling crops
    (160, True, 4, 9, 6),      # a live count inside a group, and a wholly dead group
    (160, True, 2, 3, None),
    (320, False, 2, 5, 4),
    (160, True, 4, 1, None),   # one crop
])
def test_group_kernel_matches_fp64(device, oup, res, G, B, live):
    case = fb.ir_case(160, 960, oup, 1, 7, res, B=B)
    expand, dw, project = case.blocks[0][:3]
    out = torch.full((B, 7, 7, oup), SENTINEL, device=device)
    bdev = None if live is None else torch.tensor([live], dtype=torch.int32, device=device)
    y = AF.ir_block_nhwc(_nhwc(case.x).to(device), expand, dw, project, stride=1, res=res, group=G, bdev=bdev, out=out)
    fb.check(case, _nchw(y), f"group={G}", live=live, listed=False)
    if live is not None:
        assert torch.all(y[live:] == SENTINEL)


def test_group_kernel_honours_channel_strides(device):
    """``out`` wider than oup and an input read at a pixel stride above inp: the extra channels keep their contents."""
    case = fb.ir_case(160, 960, 160, 1, 7, True, B=5)
    expand, dw, project = case.blocks[0][:3]
    wide = torch.full((5, 7, 7, 200), SENTINEL, device=device)
    wide[..., :160] = _nhwc(case.x).to(device)
    out = torch.full((5, 7, 7, 176), SENTINEL, device=device)
    from inference_arena_amd.engine.planner import pack_ir_weights, split_bf16x3
    from inference_arena_amd.ops import native

    pk = pack_ir_weights(expand, dw, project, 160, k_align=16)
    dev = {k: pk[k].float().contiguous().to(device) for k in ("be", "wd", "bd", "bp")}
    dev["we"], dev["wp"] = split_bf16x3(pk["we"]).to(device), split_bf16x3(pk["wp"]).to(device)
    native().ir_block({"x": AF._ptr(wide), "x_cs": 200, "H": 7, "W": 7, "inp": 160, "inp_pad": 160, "hid_pad": 960,
                       "oup": 160, "oup_pad": 160, "stride": 1, "expand": 1, "res": 1,
                       **{k: AF._ptr(v) for k, v in dev.items()}, "y": AF._ptr(out), "y_cs": 176, "Ho": 7, "Wo": 7, "B": 5,
                       "bdev": 0, "stream": AF._stream(), "f32": 1, "x3w": 1, "group": 4})
    torch.cuda.synchronize(device)
    fb.check(case, _nchw(out[..., :160]), "strided", listed=False)
    assert torch.all(out[..., 160:] == SENTINEL) and torch.all(wide[..., 160:] == SENTINEL)


@pytest.mark.parametrize("oup,G", [(160, 4), (160, 2), (320, 2)])
def test_group_kernel_equals_the_whole_map_kernel(device, oup, G, monkeypatch, request):
    """Both kernels accumulate the same product chains in the same K and chunk order: the same bits."""
    from inference_arena_amd.ops import native

    case = fb.ir_case(160, 960, oup, 1, 7, oup == 160, B=5)
    expand, dw, project = case.blocks[0][:3]
    x = _nhwc(case.x).to(device)
    got = AF.ir_block_nhwc(x, expand, dw, project, stride=1, res=oup == 160, group=G)
    monkeypatch.setenv("ARENA_IRC_F32", "1")
    native().set_irx_parts(2)
    request.addfinalizer(lambda: native().set_irx_parts(-1))
    ref = AF.ir_block_nhwc(x, expand, dw, project, stride=1, res=oup == 160)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("parts", [3, 5])
def test_group_kernel_hidden_slice_chain(device, parts):
    """Block A (groups of 4) stores ``parts`` partial sums, block B (groups of 2) adds them while loading."""
    tail = fb.ir_tail_case(parts)
    (ea, da, pa), (eb, db, pb) = tail.blocks[1][:3], tail.blocks[2][:3]
    g = torch.Generator().manual_seed(parts + 170)
    x = torch.randn(6, 160, 7, 7, generator=g)
    case = fb._ir(f"ir_group_chain-{parts}", x, [(ea, da, pa, 1, True, parts), (eb, db, pb, 1, False, 1)])
    mid = AF.ir_block_nhwc(_nhwc(x).to(device), ea, da, pa, stride=1, res=True, y_parts=parts, group=4)
    assert mid.shape[-1] == 160 * parts
    y = AF.ir_block_nhwc(mid, eb, db, pb, stride=1, res=False, x_parts=parts, group=2)
    fb.check(case, _nchw(y), "chain", listed=False)


@pytest.fixture(scope="module")
def dense_models():
    from inference_arena_amd.models.zoo import make_mobilenet, make_yolo

    return make_yolo(0, cls_shift=-20.0), make_mobilenet(1)


def _iou(a, b):
    x1, y1 = np.maximum(a[:, None, 0], b[None, :, 0]), np.maximum(a[:, None, 1], b[None, :, 1])
    x2, y2 = np.minimum(a[:, None, 2], b[None, :, 2]), np.minimum(a[:, None, 3], b[None, :, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    area = lambda t: (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])  # noqa: E731
    return inter / (area(a)[:, None] + area(b)[None, :] - inter + 1e-9)


def test_fp32_pipeline_with_group_blocks_matches_reference(dense_models, device, monkeypatch):
    """ARENA_IRX_GROUP=4: the criteria of test_fp32_gpu.py::test_fp32_pipeline_matches_reference."""
    from inference_arena_amd.data.synthetic import synthetic_images
    from inference_arena_amd.engine.pipeline import GpuPipeline
    from inference_arena_amd.engine.reference import ReferencePipeline

    monkeypatch.setenv("ARENA_IRX_GROUP", "4")
    imgs = synthetic_images(10, 21) + synthetic_images(2, 22, hw=(333, 500)) + synthetic_images(2, 23, hw=(640, 427))
    pipe = GpuPipeline(*dense_models, device=0, buckets=[1, 8, 16], dtype="fp32")
    grouped = [i for i, o in enumerate(pipe.program.ops) if int(o[0]) == 14 and int(o[26]) > 1]
    assert [int(pipe.program.ops[i][26]) for i in grouped] == [4, 4, 2]
    got = pipe.infer(imgs)
    for Bk in (1, 8, 16):  # a group op that launches runs the group kernel or throws (ir_block_f32)
        assert set(grouped) <= {op for op, _ in pipe.ex.launch_order(Bk)}
    ref = ReferencePipeline(*dense_models, device="cpu")
    n_det, n_top1, rel = 0, 0, []
    for i, (im, g) in enumerate(zip(imgs, got)):
        r = ref(im)
        assert len(g) == len(r), f"image {i}: {len(g)} detections vs reference {len(r)}"
        iou = _iou(r.boxes, g.boxes) if len(r) else None
        for j in range(len(r)):
            k = int(np.argmax(iou[j]))
            assert iou[j, k] > 0.99, (i, j, iou[j, k])
            n_det += 1
            n_top1 += int(g.topk_idx[k, 0] == r.topk_idx[j, 0])
            if np.array_equal(np.trunc(g.boxes[k]), np.trunc(r.boxes[j])):  # the same int-truncated crop
                rel.append(abs(float(g.topk_logit[k, 0]) - float(r.topk_logit[j, 0]))
                           / (abs(float(r.topk_logit[j, 0])) + 1e-6))
    assert n_det >= 20 and n_top1 >= 0.99 * n_det, (n_top1, n_det)
    assert max(rel) < 1e-3, max(rel)
