// pybind11 module `inference_arena_amd._C`.
//
// Exposes (a) every kernel launcher with a dict of device pointers / sizes,
// used by the kernel-vs-oracle tests and the Python op wrappers, and (b) the
// native Executor (csrc/runtime/executor.h), which releases the GIL for host
// packing, graph launch and result waits.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <malloc.h>
#include <map>
#include <mutex>

#include "kernels/launch.h"
#include "runtime/executor.h"
#include "runtime/echo_instance.h"
#include "runtime/http_front.h"
#include "runtime/http_loadgen.h"
#include "runtime/ipc_buffer.h"
#include "runtime/peer.h"
#include "runtime/jpeg_decode.h"
#include "runtime/jpeg_ingest.h"
#include "runtime/batcher.h"
#include "runtime/split.h"
#include "runtime/crash_trace.h"

namespace py = pybind11;
using namespace arena;

namespace arena {
void bind_jpeg(py::module& m);  // bindings_jpeg.cpp
}

namespace {

template <typename T>
T get(const py::dict& d, const char* k, T dflt) {
  if (!d.contains(k)) return dflt;
  py::object o = d[k];
  if (o.is_none()) return dflt;
  return o.cast<T>();
}
template <typename T>
T req(const py::dict& d, const char* k) {
  if (!d.contains(k)) throw std::runtime_error(std::string("missing kernel parameter '") + k + "'");
  return d[k].cast<T>();
}
template <typename P>
P ptr(const py::dict& d, const char* k) {
  return reinterpret_cast<P>(get<uintptr_t>(d, k, 0));
}
hipStream_t stream_of(const py::dict& d) { return reinterpret_cast<hipStream_t>(get<uintptr_t>(d, "stream", 0)); }

void py_conv2d(const py::dict& d) {
  ConvParams p{};
  p.x = ptr<const void*>(d, "x");
  p.B = req<int>(d, "B");
  p.H = req<int>(d, "H");
  p.W = req<int>(d, "W");
  p.xs = req<int>(d, "xs");
  p.Cin = req<int>(d, "Cin");
  p.w = ptr<const void*>(d, "w");
  p.Kpad = req<int>(d, "Kpad");
  p.bias = ptr<const float*>(d, "bias");
  p.y = ptr<void*>(d, "y");
  p.Ho = req<int>(d, "Ho");
  p.Wo = req<int>(d, "Wo");
  p.ys = req<int>(d, "ys");
  p.Cout = req<int>(d, "Cout");
  p.Cout_pad = req<int>(d, "Cout_pad");
  p.KH = req<int>(d, "KH");
  p.KW = req<int>(d, "KW");
  p.stride = get<int>(d, "stride", 1);
  p.pad_t = get<int>(d, "pad_t", 0);
  p.pad_l = get<int>(d, "pad_l", 0);
  p.res = ptr<const void*>(d, "res");
  p.rs = get<int>(d, "rs", 0);
  p.y2 = ptr<void*>(d, "y2");
  p.y2s = get<int>(d, "y2s", 0);
  p.act = get<int>(d, "act", 0);
  p.f32out = get<int>(d, "f32out", 0);
  p.bdev = ptr<const int*>(d, "bdev");
  p.impl = get<int>(d, "impl", 0);
  p.pw_w = ptr<const void*>(d, "pw_w");
  p.pw_bias = ptr<const float*>(d, "pw_bias");
  p.pw_y = ptr<void*>(d, "pw_y");
  p.pw_ys = get<int>(d, "pw_ys", 0);
  p.pw_cout = get<int>(d, "pw_cout", 0);
  p.pw_kpad = get<int>(d, "pw_kpad", 0);
  p.pw_act = get<int>(d, "pw_act", 0);
  p.gate = ptr<const float*>(d, "gate");
  p.gate_n = get<int>(d, "gate_n", 0);
  p.gate_min = get<float>(d, "gate_min", 0.f);
  p.n_lo = get<int>(d, "n_lo", 0);
  p.n_hi = get<int>(d, "n_hi", 0);
  p.marks = ptr<const int*>(d, "marks");
  p.mark_uh = get<int>(d, "mark_uh", 0);
  p.mark_uw = get<int>(d, "mark_uw", 0);
  p.mark_halo = get<int>(d, "mark_halo", 0);
  p.w3 = ptr<const void*>(d, "w3");
  p.sk_ws = ptr<float*>(d, "sk_ws");
  p.sk_ws_bytes = get<int64_t>(d, "sk_ws_bytes", 0);
  prepare_kernels();  // dynamic-LDS limits of the x3 halo / fused kernels (before any launch)
  if (get<int>(d, "f32", 0))
    conv2d_f32(p, stream_of(d));
  else
    conv2d(p, stream_of(d));
}

void py_head_mark(const py::dict& d) {
  HeadMarkParams p{};
  const std::vector<uintptr_t> logits = req<std::vector<uintptr_t>>(d, "logits");
  const std::vector<uintptr_t> marks = req<std::vector<uintptr_t>>(d, "marks");
  const std::vector<int> H = req<std::vector<int>>(d, "H"), W = req<std::vector<int>>(d, "W");
  const std::vector<int> ps = req<std::vector<int>>(d, "ps");
  const size_t n = logits.size();
  if (n < 1 || n > (size_t)kMarkMaxLevels || marks.size() != n || H.size() != n || W.size() != n || ps.size() != n)
    throw std::runtime_error("head_mark: 1..3 levels, one entry per level in every list");
  p.n_levels = (int)n;
  for (size_t l = 0; l < n; ++l) {
    p.logits[l] = reinterpret_cast<const float*>(logits[l]);
    p.marks[l] = reinterpret_cast<int*>(marks[l]);
    p.H[l] = H[l];
    p.W[l] = W[l];
    p.ps[l] = ps[l];
  }
  p.n = req<int>(d, "n");
  p.gate_min = req<float>(d, "gate_min");
  p.B = req<int>(d, "B");
  p.bdev = ptr<const int*>(d, "bdev");
  head_mark(p, stream_of(d));
}

void py_dwconv(const py::dict& d) {
  DwParams p{};
  p.x = ptr<const void*>(d, "x");
  p.B = req<int>(d, "B");
  p.H = req<int>(d, "H");
  p.W = req<int>(d, "W");
  p.xs = req<int>(d, "xs");
  p.C = req<int>(d, "C");
  p.w = ptr<const void*>(d, "w");
  p.bias = ptr<const float*>(d, "bias");
  p.y = ptr<void*>(d, "y");
  p.Ho = req<int>(d, "Ho");
  p.Wo = req<int>(d, "Wo");
  p.ys = req<int>(d, "ys");
  p.stride = get<int>(d, "stride", 1);
  p.act = get<int>(d, "act", 0);
  p.bdev = ptr<const int*>(d, "bdev");
  if (get<int>(d, "f32", 0))
    dwconv3x3_f32(p, stream_of(d));
  else
    dwconv3x3(p, stream_of(d));
}

void py_ir_block(const py::dict& d) {
  IrParams p{};
  p.x = ptr<const void*>(d, "x");
  p.x_cs = req<int>(d, "x_cs");
  p.H = req<int>(d, "H");
  p.W = req<int>(d, "W");
  p.inp = req<int>(d, "inp");
  p.inp_pad = req<int>(d, "inp_pad");
  p.hid_pad = req<int>(d, "hid_pad");
  p.oup = req<int>(d, "oup");
  p.oup_pad = req<int>(d, "oup_pad");
  p.stride = req<int>(d, "stride");
  p.expand = req<int>(d, "expand");
  p.res = get<int>(d, "res", 0);
  p.we = ptr<const void*>(d, "we");
  p.be = ptr<const float*>(d, "be");
  p.wd = ptr<const void*>(d, "wd");
  p.bd = ptr<const float*>(d, "bd");
  p.wp = ptr<const void*>(d, "wp");
  p.bp = ptr<const float*>(d, "bp");
  p.y = ptr<void*>(d, "y");
  p.y_cs = req<int>(d, "y_cs");
  p.Ho = req<int>(d, "Ho");
  p.Wo = req<int>(d, "Wo");
  p.B = req<int>(d, "B");
  p.bdev = ptr<const int*>(d, "bdev");
  p.x3w = get<int>(d, "x3w", 0);
  p.x_parts = get<int>(d, "x_parts", 0);
  p.y_parts = get<int>(d, "y_parts", 0);
  prepare_kernels();
  if (get<int>(d, "f32", 0))
    ir_block_f32(p, stream_of(d));
  else
    ir_block(p, stream_of(d));
}

// one fused C3 block (fp32: c3_x3.hip over pre-split weights; bf16: c3_fused.hip)
void py_c3_block(const py::dict& d) {
  C3Params p{};
  p.x = ptr<const void*>(d, "x");
  p.xs = req<int>(d, "xs");
  p.B = req<int>(d, "B");
  p.H = req<int>(d, "H");
  p.W = req<int>(d, "W");
  p.bdev = ptr<const int*>(d, "bdev");
  p.C1 = req<int>(d, "C1");
  p.CH = req<int>(d, "CH");
  p.NB = req<int>(d, "NB");
  p.res = req<int>(d, "res");
  p.w12 = ptr<const void*>(d, "w12");
  p.b12 = ptr<const float*>(d, "b12");
  p.wb1[0] = p.wb1[1] = ptr<const void*>(d, "wb1");
  p.bb1[0] = p.bb1[1] = ptr<const float*>(d, "bb1");
  p.wb2[0] = p.wb2[1] = ptr<const void*>(d, "wb2");
  p.bb2[0] = p.bb2[1] = ptr<const float*>(d, "bb2");
  p.w3 = ptr<const void*>(d, "w3");
  p.b3 = ptr<const float*>(d, "b3");
  p.y = ptr<void*>(d, "y");
  p.ys = req<int>(d, "ys");
  prepare_kernels();
  if (get<int>(d, "f32", 0))
    c3_x3(p, stream_of(d));
  else
    c3_fused(p, stream_of(d));
}

void py_sppf(const py::dict& d) {
  SppfParams p{};
  p.buf = ptr<void*>(d, "buf");
  p.B = req<int>(d, "B");
  p.H = req<int>(d, "H");
  p.W = req<int>(d, "W");
  p.xs = req<int>(d, "xs");
  p.C = req<int>(d, "C");
  p.bdev = ptr<const int*>(d, "bdev");
  if (get<int>(d, "f32", 0))
    sppf_pool_f32(p, stream_of(d));
  else
    sppf_pool(p, stream_of(d));
}

void py_letterbox(const py::dict& d) {
  LetterboxParams p{};
  p.pool = ptr<const uint8_t*>(d, "pool");
  p.meta = ptr<const ImageMeta*>(d, "meta");
  p.ctrl = ptr<const Ctrl*>(d, "ctrl");
  p.out = ptr<void*>(d, "out");
  p.B = req<int>(d, "B");
  p.T = req<int>(d, "T");
  p.f32 = get<int>(d, "f32", 0);
  letterbox_s2d(p, stream_of(d));
}

void py_decode(const py::dict& d) {
  DecodeParams p{};
  auto heads = req<std::vector<uintptr_t>>(d, "head");
  auto hw = req<std::vector<int>>(d, "hw");
  auto xs = req<std::vector<int>>(d, "xs");
  auto st = req<std::vector<float>>(d, "strides");
  for (int l = 0; l < 3; ++l) {
    p.head[l] = (const void*)heads.at(l);
    p.hw[l] = hw.at(l);
    p.xs[l] = xs.at(l);
    p.stride[l] = st.at(l);
  }
  p.B = req<int>(d, "B");
  p.conf_thr = req<float>(d, "conf_thr");
  p.cand = ptr<Candidate*>(d, "cand");
  p.cand_count = ptr<int*>(d, "cand_count");
  p.cand_cap = req<int>(d, "cand_cap");
  p.ctrl = ptr<const Ctrl*>(d, "ctrl");
  p.f32 = get<int>(d, "f32", 0);
  detect_decode(p, stream_of(d));
}

void py_yolo_raw(const py::dict& d) {
  YoloRawParams p{};
  auto heads = req<std::vector<uintptr_t>>(d, "head");
  auto hw = req<std::vector<int>>(d, "hw");
  auto xs = req<std::vector<int>>(d, "xs");
  auto st = req<std::vector<float>>(d, "strides");
  for (int l = 0; l < 3; ++l) {
    p.head[l] = (const void*)heads.at(l);
    p.hw[l] = hw.at(l);
    p.xs[l] = xs.at(l);
    p.stride[l] = st.at(l);
  }
  p.B = req<int>(d, "B");
  p.out = ptr<void*>(d, "out");
  p.out_stride = req<size_t>(d, "out_stride");  // bytes
  p.ctrl = ptr<const Ctrl*>(d, "ctrl");
  p.f32 = get<int>(d, "f32", 0);
  yolo_raw(p, stream_of(d));
}

void py_tensor_in(const py::dict& d) {
  TensorInParams p{};
  p.pool = ptr<const uint8_t*>(d, "pool");
  p.meta = ptr<const ImageMeta*>(d, "meta");
  p.ctrl = ptr<const Ctrl*>(d, "ctrl");
  p.out = ptr<void*>(d, "out");
  p.B = req<int>(d, "B");
  p.S = req<int>(d, "S");
  p.f32 = get<int>(d, "f32", 0);
  tensor_in_s2d(p, stream_of(d));
}

// fp32 detector front end on its own (csrc/kernels/stem_x3.hip): src 0 letterbox, 2 request tensors.
void py_stem_s2_f32(const py::dict& d) {
  prepare_kernels();
  StemFusedParams p{};
  p.src = req<int>(d, "src");
  p.pool = ptr<const uint8_t*>(d, "pool");
  p.meta = ptr<const ImageMeta*>(d, "meta");
  p.ctrl = ptr<const Ctrl*>(d, "ctrl");
  p.cap = req<int>(d, "cap");
  p.S = req<int>(d, "S");
  p.KS = 3;
  p.w = ptr<const void*>(d, "w");
  p.bias = ptr<const float*>(d, "bias");
  p.Cout = 16;
  p.act = 1;
  p.w2 = ptr<const void*>(d, "w2");
  p.bias2 = ptr<const float*>(d, "bias2");
  p.Cout2 = 32;
  p.act2 = get<int>(d, "act2", 1);
  p.y2 = ptr<void*>(d, "y");
  p.y2s = req<int>(d, "ys");
  stem_s2_f32(p, stream_of(d));
}

// bf16 front ends on their own (csrc/kernels/stem_fused.hip): src 0 letterbox -> detector stem [-> 3x3 s2 conv with
// "w2"], src 1 crop gather -> classifier stem [-> MobileNetV2 block 1 with "ir_wd"].
void py_stem_fused(const py::dict& d) {
  StemFusedParams p{};
  p.src = req<int>(d, "src");
  p.pool = ptr<const uint8_t*>(d, "pool");
  p.meta = ptr<const ImageMeta*>(d, "meta");
  p.ctrl = ptr<const Ctrl*>(d, "ctrl");
  p.crops = ptr<const CropRef*>(d, "crops");
  p.cap = req<int>(d, "cap");
  p.S = req<int>(d, "S");
  const auto mean = get<std::vector<float>>(d, "mean", {0.f, 0.f, 0.f});
  const auto inv_std = get<std::vector<float>>(d, "inv_std", {1.f, 1.f, 1.f});
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = mean.at(c);
    p.inv_std[c] = inv_std.at(c);
  }
  p.KS = req<int>(d, "KS");
  p.w = ptr<const void*>(d, "w");
  p.Kpad = req<int>(d, "Kpad");
  p.bias = ptr<const float*>(d, "bias");
  p.Cout = req<int>(d, "Cout");
  p.y = ptr<void*>(d, "y");
  p.ys = get<int>(d, "ys", 0);
  p.act = get<int>(d, "act", 0);
  p.w2 = ptr<const void*>(d, "w2");
  p.Kpad2 = get<int>(d, "Kpad2", 0);
  p.bias2 = ptr<const float*>(d, "bias2");
  p.Cout2 = get<int>(d, "Cout2", 0);
  p.act2 = get<int>(d, "act2", 0);
  p.y2 = ptr<void*>(d, "y2");
  p.y2s = get<int>(d, "y2s", 0);
  p.ir_wd = ptr<const void*>(d, "ir_wd");
  p.ir_bd = ptr<const float*>(d, "ir_bd");
  p.ir_wp = ptr<const void*>(d, "ir_wp");
  p.ir_bp = ptr<const float*>(d, "ir_bp");
  p.ir_y = ptr<void*>(d, "ir_y");
  p.ir_ys = get<int>(d, "ir_ys", 0);
  stem_fused(p, stream_of(d));
}

// {"name", "input", "in_dims", "output", "out_dims", "max_batch_size", "platform", "versions"} -> the contract
KServeTensorModel tensor_model_of(const py::dict& d) {
  KServeTensorModel m;
  m.name = req<std::string>(d, "name");
  m.input = req<std::string>(d, "input");
  m.output = req<std::string>(d, "output");
  m.in_dims = req<std::vector<int64_t>>(d, "in_dims");
  m.out_dims = req<std::vector<int64_t>>(d, "out_dims");
  m.max_batch_size = get<int>(d, "max_batch_size", 0);
  m.platform = get<std::string>(d, "platform", m.platform);
  m.versions = get<std::vector<std::string>>(d, "versions", {});
  return m;
}

void py_nms(const py::dict& d) {
  prepare_kernels();
  NmsParams p{};
  p.cand = ptr<const Candidate*>(d, "cand");
  p.cand_count = ptr<const int*>(d, "cand_count");
  p.cand_cap = req<int>(d, "cand_cap");
  p.meta = ptr<const ImageMeta*>(d, "meta");
  p.B = req<int>(d, "B");
  p.iou_thr = req<float>(d, "iou_thr");
  p.det = ptr<Detection*>(d, "det");
  p.det_count = ptr<int*>(d, "det_count");
  p.max_det = req<int>(d, "max_det");
  p.ctrl = ptr<const Ctrl*>(d, "ctrl");
  nms(p, stream_of(d));
}

void py_crop_plan(const py::dict& d) {
  CropPlanParams p{};
  p.det = ptr<Detection*>(d, "det");
  p.det_count = ptr<int*>(d, "det_count");
  p.max_det = req<int>(d, "max_det");
  p.meta = ptr<const ImageMeta*>(d, "meta");
  p.B = req<int>(d, "B");
  p.crops = ptr<CropRef*>(d, "crops");
  p.ctrl = ptr<Ctrl*>(d, "ctrl");
  p.crop_cap = req<int>(d, "crop_cap");
  p.whole = get<int>(d, "whole", 0);
  crop_plan(p, stream_of(d));
}

void py_crop_gather(const py::dict& d) {
  CropGatherParams p{};
  p.pool = ptr<const uint8_t*>(d, "pool");
  p.meta = ptr<const ImageMeta*>(d, "meta");
  p.crops = ptr<const CropRef*>(d, "crops");
  p.ctrl = ptr<const Ctrl*>(d, "ctrl");
  p.out = ptr<void*>(d, "out");
  p.cap = req<int>(d, "cap");
  p.S = req<int>(d, "S");
  auto mean = req<std::vector<float>>(d, "mean");
  auto inv_std = req<std::vector<float>>(d, "inv_std");
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = mean.at(c);
    p.inv_std[c] = inv_std.at(c);
  }
  p.f32 = get<int>(d, "f32", 0);
  crop_gather_s2d(p, stream_of(d));
}

void py_head_pool(const py::dict& d) {
  HeadPoolParams p{};
  p.x = ptr<const void*>(d, "x");
  p.xs = req<int>(d, "xs");
  p.HW = req<int>(d, "HW");
  p.K = req<int>(d, "K");
  p.w = ptr<const void*>(d, "w");
  p.Kpad = req<int>(d, "Kpad");
  p.bias = ptr<const float*>(d, "bias");
  p.N = req<int>(d, "N");
  p.Npad = req<int>(d, "Npad");
  p.y = ptr<void*>(d, "y");
  p.ys = req<int>(d, "ys");
  p.act = get<int>(d, "act", 0);
  p.B = req<int>(d, "B");
  p.bdev = ptr<const int*>(d, "bdev");
  prepare_kernels();
  if (get<int>(d, "f32", 0))
    head_pool_f32(p, stream_of(d));
  else
    head_pool(p, stream_of(d));
}

void py_avgpool(const py::dict& d) {
  AvgPoolParams p{};
  p.x = ptr<const void*>(d, "x");
  p.B = req<int>(d, "B");
  p.HW = req<int>(d, "HW");
  p.C = req<int>(d, "C");
  p.y = ptr<void*>(d, "y");
  p.bdev = ptr<const int*>(d, "bdev");
  p.f32 = get<int>(d, "f32", 0);
  global_avgpool(p, stream_of(d));
}

void py_topk(const py::dict& d) {
  TopkParams p{};
  p.logits = ptr<const float*>(d, "logits");
  p.B = req<int>(d, "B");
  p.N = req<int>(d, "N");
  p.ld = req<int>(d, "ld");
  p.out = ptr<TopkResult*>(d, "out");
  p.ctrl = ptr<const Ctrl*>(d, "ctrl");
  p.bdev = ptr<const int*>(d, "bdev");
  topk_softmax(p, stream_of(d));
}

ExecutorConfig config_from(const py::dict& d) {
  ExecutorConfig c;
  c.device = get<int>(d, "device", c.device);
  c.max_batch = get<int>(d, "max_batch", c.max_batch);
  c.max_det = get<int>(d, "max_det", c.max_det);
  c.cand_cap = get<int>(d, "cand_cap", c.cand_cap);
  c.crop_cap_per_image = get<int>(d, "crop_cap_per_image", c.crop_cap_per_image);
  c.min_crop_cap = get<int>(d, "min_crop_cap", c.min_crop_cap);
  c.pool_bytes_per_image = get<int64_t>(d, "pool_bytes_per_image", c.pool_bytes_per_image);
  c.pool_factor = get<int>(d, "pool_factor", c.pool_factor);
  c.det_size = get<int>(d, "det_size", c.det_size);
  c.cls_size = get<int>(d, "cls_size", c.cls_size);
  c.host_threads = get<int>(d, "host_threads", c.host_threads);
  c.raw_out_bytes = get<int64_t>(d, "raw_out_bytes", c.raw_out_bytes);
  c.jpeg_ragged = get<bool>(d, "jpeg_ragged", c.jpeg_ragged);
  return c;
}

// A DynamicBatcher result callback that calls a Python function with the result dict (GIL taken on the batcher
// thread; the function's reference is dropped under the GIL too).
ResultCallback py_result_cb(py::function cb) {
  // The callback is released on a batcher thread: drop the Python reference under the GIL.
  std::shared_ptr<py::function> pycb(new py::function(std::move(cb)), [](py::function* fn) {
    py::gil_scoped_acquire gil;
    delete fn;
  });
  return [pycb](RequestResult&& r) {
    py::gil_scoped_acquire gil;
    py::dict d;
    d["id"] = r.id;
    d["error"] = r.error;
    d["det_count"] = r.det_count;
    const int k = (int)r.det.size();
    py::array_t<float> det({k, 8});
    if (k) std::memcpy(det.mutable_data(), r.det.data(), sizeof(Detection) * k);
    const int t = (int)r.topk.size();
    py::array_t<int32_t> ti({t, 5});
    py::array_t<float> tl({t, 5}), tp({t, 5});
    for (int i = 0; i < t; ++i)
      for (int j = 0; j < 5; ++j) {
        ti.mutable_at(i, j) = r.topk[i].idx[j];
        tl.mutable_at(i, j) = r.topk[i].logit[j];
        tp.mutable_at(i, j) = r.topk[i].prob[j];
      }
    d["det"] = det;
    d["topk_idx"] = ti;
    d["topk_logit"] = tl;
    d["topk_prob"] = tp;
    if (!r.raw.empty()) {
      py::array_t<uint8_t> raw((py::ssize_t)r.raw.size());
      std::memcpy(raw.mutable_data(), r.raw.data(), r.raw.size());
      d["raw"] = raw;
    }
    d["batch_size"] = r.batch_size;
    d["queue_us"] = r.queue_us;
    d["compute_us"] = r.compute_us;
    d["detection_ms"] = r.det_ms;       // device stage times of the batch (OP_STAMP); -1: none
    d["classification_ms"] = r.cls_ms;
    try {
      (*pycb)(d);
    } catch (py::error_already_set& e) {
      e.discard_as_unraisable("DynamicBatcher callback");
    }
  };
}

// JPEG uploads given to Executor.submit / run as `bytes`: entropy-decoded here (host half of the split decoder),
// reconstructed on the device by the executor.  The coefficients must outlive the asynchronous H2D copy, so a
// submitted batch's holders stay registered until its collect().
struct JpegHolder {
  JpegInfo info;
  std::vector<int16_t> coef;
};
using JpegKeep = std::vector<std::shared_ptr<JpegHolder>>;
std::mutex g_jkeep_mu;
std::map<std::pair<const void*, int>, JpegKeep> g_jkeep;
struct JpegSet;
std::map<std::pair<const void*, int>, std::shared_ptr<JpegSet>> g_jset_keep;  // sets of submitted batches

// Uploads entropy-decoded once into pinned host memory (what the HTTP front end's decode threads hand the batcher:
// coefficient blocks in a pinned HostBufferPool buffer, DMA'd by the executor), so a benchmark can replay the HTTP
// path's device inputs without paying the Huffman decode per batch (bench.py engine_req_s: the device ceiling of
// the split-decode path).
struct JpegSet {
  struct Item {
    JpegInfo info;
    int16_t* coef = nullptr;
    bool pinned = false;
    ~Item() {
      if (coef == nullptr) return;
      if (pinned) (void)hipHostFree(coef);
      else std::free(coef);
    }
  };
  std::vector<std::shared_ptr<Item>> items;
};

std::shared_ptr<JpegSet> make_jpeg_set(const py::list& uploads, bool pinned) {
  auto set = std::make_shared<JpegSet>();
  for (auto h : uploads) {
    const std::string data = h.cast<std::string>();
    auto it = std::make_shared<JpegSet::Item>();
    std::string err;
    JpegStatus st = jpeg_parse((const uint8_t*)data.data(), data.size(), it->info, err);
    if (st != JpegStatus::Ok) throw py::value_error("JpegSet: not decodable by the split decoder: " + err);
    const bool compact = jpeg_compact_enabled();  // the serving paths' payload (http_front.cpp native_decode)
    const size_t bytes =
        std::max<size_t>(2, compact ? (size_t)jpeg_compact_capacity(it->info) : (size_t)it->info.coef_count * 2);
    void* p = nullptr;
    if (pinned && hipHostMalloc(&p, bytes, hipHostMallocPortable) == hipSuccess) {
      it->pinned = true;
    } else {
      (void)hipGetLastError();
      p = std::malloc(bytes);
      if (p == nullptr) throw std::bad_alloc();
    }
    it->coef = (int16_t*)p;
    st = compact ? jpeg_decode_compact((const uint8_t*)data.data(), data.size(), it->info, (uint8_t*)it->coef, err)
                 : jpeg_decode_coefs((const uint8_t*)data.data(), data.size(), it->info, it->coef, err);
    if (st != JpegStatus::Ok) throw py::value_error("JpegSet: entropy decode failed: " + err);
    set->items.push_back(it);
  }
  return set;
}

std::vector<InputImage> images_from(const py::list& imgs, std::vector<py::array>& keep, JpegKeep* jkeep = nullptr) {
  std::vector<InputImage> v;
  v.reserve(imgs.size());
  for (auto h : imgs) {
    if (py::isinstance<py::bytes>(h)) {
      if (jkeep == nullptr) throw std::runtime_error("JPEG inputs are not accepted here");
      const std::string data = h.cast<std::string>();
      auto jh = std::make_shared<JpegHolder>();
      std::string err;
      JpegStatus st = jpeg_parse((const uint8_t*)data.data(), data.size(), jh->info, err);
      if (st == JpegStatus::Ok) {
        jh->coef.assign((size_t)jh->info.coef_count, 0);
        st = jpeg_decode_coefs((const uint8_t*)data.data(), data.size(), jh->info, jh->coef.data(), err);
      }
      if (st != JpegStatus::Ok) throw py::value_error("JPEG input not decodable by the split decoder: " + err);
      InputImage im{(const uint8_t*)jh->coef.data(), jh->info.out_height, jh->info.out_width};
      im.jpeg = &jh->info;
      jkeep->push_back(jh);
      v.push_back(im);
      continue;
    }
    py::array a = py::array::ensure(h, py::array::c_style);
    if (!a) throw std::runtime_error("inputs must be numpy arrays");
    InputImage im;
    if (a.ndim() == 3 && a.shape(2) == 3 && a.itemsize() == 1) {  // RGB uint8 HWC image
      im.h = (int)a.shape(0);
      im.w = (int)a.shape(1);
    } else if (a.ndim() == 3 && a.shape(0) == 3 && a.itemsize() == 4 && a.shape(1) == a.shape(2)) {
      im.h = im.w = (int)a.shape(1);  // fp32 CHW [3, S, S] tensor (reference tensor contract)
      im.bytes = (int64_t)a.nbytes();
    } else {
      throw std::runtime_error("inputs must be uint8 HxWx3 images or float32 [3,S,S] tensors");
    }
    keep.push_back(a);
    im.data = (const uint8_t*)a.data();
    v.push_back(im);
  }
  return v;
}

py::dict result_to_py(const BatchResult& r, int max_det) {
  py::dict out;
  const int n = r.n_images;
  py::array_t<int32_t> cnt(n);
  std::memcpy(cnt.mutable_data(), r.det_count.data(), sizeof(int) * n);
  py::array_t<float> det({n, max_det, 8});
  static_assert(sizeof(Detection) == 32, "Detection layout");
  if (n) std::memcpy(det.mutable_data(), r.det.data(), sizeof(Detection) * (size_t)n * max_det);
  py::array_t<int32_t> offs(n + 1);
  std::memcpy(offs.mutable_data(), r.crop_offset.data(), sizeof(int) * (n + 1));
  static_assert(sizeof(TopkResult) == 64, "TopkResult layout");
  py::array_t<int32_t> tk_idx({(int)r.topk.size(), 5});
  py::array_t<float> tk_logit({(int)r.topk.size(), 5});
  py::array_t<float> tk_prob({(int)r.topk.size(), 5});
  for (size_t i = 0; i < r.topk.size(); ++i)
    for (int k = 0; k < 5; ++k) {
      tk_idx.mutable_at(i, k) = r.topk[i].idx[k];
      tk_logit.mutable_at(i, k) = r.topk[i].logit[k];
      tk_prob.mutable_at(i, k) = r.topk[i].prob[k];
    }
  out["det_count"] = cnt;
  out["det"] = det;
  out["crop_offset"] = offs;
  out["topk_idx"] = tk_idx;
  out["topk_logit"] = tk_logit;
  out["topk_prob"] = tk_prob;
  out["gpu_ms"] = r.gpu_ms;
  out["detection_ms"] = r.det_ms;
  out["classification_ms"] = r.cls_ms;
  out["bucket"] = r.bucket;
  out["total_crops"] = r.total_crops;
  if (!r.raw.empty()) {
    py::array_t<uint8_t> raw((py::ssize_t)r.raw.size());
    std::memcpy(raw.mutable_data(), r.raw.data(), r.raw.size());
    out["raw"] = raw;
  }
  return out;
}

}  // namespace

PYBIND11_MODULE(_C, m) {
  m.doc() = "MI355X-native kernels and runtime of inference_arena_amd (gfx950)";
  // native stack of a fault on a thread Python's faulthandler cannot see (ARENA_CRASH_TRACE=0 disables)
  {
    const char* e = std::getenv("ARENA_CRASH_TRACE");
    if (e == nullptr || std::strcmp(e, "0") != 0) arena::install_crash_trace();
  }
  m.def("install_crash_trace", &arena::install_crash_trace);
  m.def("crash_trace_installed", &arena::crash_trace_installed);
  m.def("dump_thread_stack", &arena::dump_thread_stack, py::arg("tid"));
  // glibc: hand free heap pages of every arena back to the kernel (buffers allocated on one thread and freed on
  // another leave per-thread arenas holding pages; the serving processes call this periodically)
  m.def("malloc_trim", []() {
    py::gil_scoped_release nogil;
    return malloc_trim(0) != 0;
  });
  // glibc heap totals (mallinfo2): RSS growth with flat in_use bytes is free pages the heap holds (fragmentation);
  // growth of in_use is live allocations; growth outside both is mmap'd memory of someone other than malloc
  m.def("malloc_info", []() {
    const struct mallinfo2 mi = mallinfo2();
    py::dict d;
    d["arena"] = (uint64_t)mi.arena;        // bytes of the main and thread heaps (sbrk / heap mmaps)
    d["mmapped"] = (uint64_t)mi.hblkhd;     // bytes in malloc's own per-chunk mmaps
    d["in_use"] = (uint64_t)mi.uordblks;    // allocated bytes inside the heaps
    d["free"] = (uint64_t)mi.fordblks;      // free bytes inside the heaps
    d["releasable"] = (uint64_t)mi.keepcost;
    return d;
  });
  bind_jpeg(m);
  m.def("conv2d", &py_conv2d);
  m.def("set_conv_impl", &set_conv_impl);
  m.def("get_conv_impl", &get_conv_impl);
  m.def("dwconv3x3", &py_dwconv);
  m.def("sppf_pool", &py_sppf);
  m.def("ir_block", &py_ir_block);
  m.def("c3_block", &py_c3_block);
  m.def("set_conv_pw", &set_conv_pw);
  m.def("set_conv_v3", &set_conv_v3);
  m.def("set_ir_wave", &set_ir_wave);
  m.def("set_irx_parts", &set_irx_parts);
  m.def("set_irx_slices_big", &set_irx_slices_big);
  m.def("set_ir_t14", &set_ir_t14);
  m.def("set_ir_crop", &set_ir_crop);
  m.def("set_ir_s2k16", &set_ir_s2k16);
  m.def("set_ir_crop_split", &set_ir_crop_split);
  // Detect-head tile gate (runtime/head_gate.h)
  m.def("set_head_gate", &set_head_gate);
  m.def("get_head_gate", &get_head_gate);
  m.def(
      "head_gate_min",
      [](float conf_thr) -> py::object {
        float g;
        if (!head_gate_min(conf_thr, &g)) return py::none();
        return py::float_(g);
      },
      py::arg("conf_thr"), "the gate's logit threshold for a confidence threshold (float32); None: the gate is off");
  m.def(
      "head_gate_pairs",
      [](py::array_t<int64_t, py::array::c_style> ops) {
        if (ops.ndim() != 2 || ops.shape(1) != kOpFields) throw std::runtime_error("ops must be int64 [n, OP_FIELDS]");
        py::list out;
        for (const HeadGatePair& gp : head_gate_pairs(ops.data(), (int)ops.shape(0), kOpFields))
          out.append(py::make_tuple(gp.box, gp.cls, gp.level));
        return out;
      },
      py::arg("ops"), "[(box conv op, class conv op, level)] of a program's records");
  // Head split (runtime/head_marks.h)
  m.def("set_head_split", &set_head_split);
  m.def("get_head_split", &get_head_split);
  m.attr("HEAD_SPLIT_MIN_BUCKET") = kHeadSplitMinBucket;
  m.attr("HEAD_SPLIT_BOX_IMPL") = kF32X3HP + kHeadSplitBoxVariant;
  m.attr("HEAD_SPLIT_CLS_IMPL") = kF32X3HP + kHeadSplitClsVariant;
  m.attr("MARK_CELL") = kMarkCell;
  m.def("head_mark", &py_head_mark);
  m.def(
      "head_gate_first_convs",
      [](py::array_t<int64_t, py::array::c_style> ops) {
        if (ops.ndim() != 2 || ops.shape(1) != kOpFields) throw std::runtime_error("ops must be int64 [n, OP_FIELDS]");
        py::list out;
        for (const HeadGatePair& gp : head_gate_pairs(ops.data(), (int)ops.shape(0), kOpFields))
          out.append(head_gate_first_conv(ops.data(), (int)ops.shape(0), kOpFields, gp));
        return out;
      },
      py::arg("ops"), "per head-gate pair of a program's records: the op of its first head conv, or -1");
  m.def(
      "head_marks_needed",
      [](py::array_t<int, py::array::c_style | py::array::forcecast> marks, int H, int W, int th, int tw, int uh,
         int uw, int halo) {
        if (H <= 0 || W <= 0 || th <= 0 || tw <= 0 || uh <= 0 || uw <= 0 || halo < 0 || marks.ndim() != 2 ||
            marks.shape(0) != head_mark_cells(H) || marks.shape(1) != head_mark_cells(W))
          throw std::runtime_error("head_marks_needed: marks must be int32 [ceil(H / 8), ceil(W / 8)], sizes > 0");
        const int nty = (H + th - 1) / th, ntx = (W + tw - 1) / tw;
        py::array_t<bool> out({nty, ntx});
        auto o = out.mutable_unchecked<2>();
        for (int ty = 0; ty < nty; ++ty)
          for (int tx = 0; tx < ntx; ++tx)
            o(ty, tx) = head_marks_needed(marks.data(), H, W, ty, tx, th, tw, uh, uw, halo);
        return out;
      },
      py::arg("marks"), py::arg("H"), py::arg("W"), py::arg("th"), py::arg("tw"), py::arg("uh"), py::arg("uw"),
      py::arg("halo"),
      "bool [tiles_y, tiles_x]: the th x tw producer tiles of one image that a continuing uh x uw consumer tile, "
      "grown by halo pixels, reads (the host oracle of the x3hp mark gate)");
  m.attr("HEAD_BOX_CHANNELS") = kHeadBoxChannels;
  m.attr("HEAD_CLS_CHANNELS") = kHeadClsChannels;
  m.def("letterbox_s2d", &py_letterbox);
  m.def("detect_decode", &py_decode);
  m.def("yolo_raw", &py_yolo_raw);
  m.def("tensor_in_s2d", &py_tensor_in);
  m.def("stem_s2_f32", &py_stem_s2_f32);
  m.def("stem_fused", &py_stem_fused);
  m.def("nms", &py_nms);
  m.def("crop_plan", &py_crop_plan);
  m.def("crop_gather_s2d", &py_crop_gather);
  m.def("global_avgpool", &py_avgpool);
  m.def("head_pool", &py_head_pool);
  m.def("topk_softmax", &py_topk);
  m.attr("SIZEOF_IMAGE_META") = (int)sizeof(ImageMeta);
  m.attr("SIZEOF_CTRL") = (int)sizeof(Ctrl);
  m.attr("SIZEOF_CANDIDATE") = (int)sizeof(Candidate);
  m.attr("SIZEOF_DETECTION") = (int)sizeof(Detection);
  m.attr("SIZEOF_CROPREF") = (int)sizeof(CropRef);
  m.attr("SIZEOF_TOPK") = (int)sizeof(TopkResult);
  m.attr("OP_FIELDS") = kOpFields;

  py::class_<Executor, std::shared_ptr<Executor>>(m, "Executor")
      .def(py::init([](const py::dict& cfg) { return std::make_shared<Executor>(config_from(cfg)); }))
      .def("set_weights",
           [](Executor& e, py::array_t<uint8_t, py::array::c_style> blob) { e.set_weights(blob.data(), blob.size()); })
      .def("set_weights_device",
           [](Executor& e, uintptr_t ptr, size_t bytes) {
             py::gil_scoped_release nogil;
             e.set_weights_device((const void*)ptr, bytes);
           })
      .def("weights_host",
           [](Executor& e) {
             std::vector<uint8_t> v;
             {
               py::gil_scoped_release nogil;
               v = e.weights_host();
             }
             return py::bytes((const char*)v.data(), v.size());
           })
      .def("set_program",
           [](Executor& e, py::array_t<int64_t, py::array::c_style> ops, py::array_t<int64_t, py::array::c_style> cls) {
             if (ops.ndim() != 2 || ops.shape(1) != kOpFields || cls.ndim() != 2 || cls.shape(1) != kOpFields)
               throw std::runtime_error("programs must be int64 [n, OP_FIELDS]");
             e.set_program(ops.data(), (int)ops.shape(0), cls.data(), (int)cls.shape(0));
           })
      .def("add_bucket",
           [](Executor& e, int B, py::array_t<int64_t, py::array::c_style> offs, int64_t arena_bytes,
              py::object impl) {
             if (impl.is_none()) {
               e.add_bucket(B, offs.data(), (int)offs.size(), arena_bytes);
             } else {
               const std::vector<int> v = impl.cast<std::vector<int>>();
               e.add_bucket(B, offs.data(), (int)offs.size(), arena_bytes, &v);
             }
           },
           py::arg("B"), py::arg("offsets"), py::arg("arena_bytes"), py::arg("impl") = py::none())
      .def("buckets", &Executor::buckets)
      .def("crop_cap_for", &Executor::crop_cap_for)
      .def_property_readonly("jpeg_ragged", [](const Executor& e) { return e.config().jpeg_ragged; })
      .def("submit",
           [](Executor& e, const py::list& imgs) {
             std::vector<py::array> keep;
             JpegKeep jkeep;
             auto v = images_from(imgs, keep, &jkeep);
             int slot;
             {
               py::gil_scoped_release nogil;
               slot = e.submit(v);
             }
             if (!jkeep.empty()) {
               std::lock_guard<std::mutex> lk(g_jkeep_mu);
               g_jkeep[{(const void*)&e, slot}] = std::move(jkeep);
             }
             return slot;
           })
      .def("submit_jpeg_set",
           // images idx[0..n) of a JpegSet: pre-decoded coefficients, reconstructed on the device like an HTTP upload
           [](Executor& e, std::shared_ptr<JpegSet> set, const std::vector<int>& idx) {
             std::vector<InputImage> v;
             v.reserve(idx.size());
             for (int i : idx) {
               if (i < 0 || i >= (int)set->items.size()) throw py::index_error("submit_jpeg_set: index out of range");
               const auto& it = set->items[i];
               InputImage im{(const uint8_t*)it->coef, it->info.out_height, it->info.out_width};
               im.jpeg = &it->info;
               v.push_back(im);
             }
             int slot;
             {
               py::gil_scoped_release nogil;
               slot = e.submit(v);
             }
             std::lock_guard<std::mutex> lk(g_jkeep_mu);
             g_jset_keep[{(const void*)&e, slot}] = set;
             return slot;
           })
      .def("collect",
           [](Executor& e, int slot) {
             BatchResult r;
             {
               py::gil_scoped_release nogil;
               r = e.collect(slot);
             }
             {
               std::lock_guard<std::mutex> lk(g_jkeep_mu);
               g_jkeep.erase({(const void*)&e, slot});
               g_jset_keep.erase({(const void*)&e, slot});
             }
             return result_to_py(r, e.config().max_det);
           })
      .def("run",
           [](Executor& e, const py::list& imgs) {
             std::vector<py::array> keep;
             JpegKeep jkeep;
             auto v = images_from(imgs, keep, &jkeep);
             BatchResult r;
             {
               py::gil_scoped_release nogil;
               r = e.run(v);
             }
             return result_to_py(r, e.config().max_det);
           })
      .def("replay",
           [](Executor& e, int B, int slot, int iters) {
             py::gil_scoped_release nogil;
             e.replay(B, slot, iters);
           })
      .def("num_slots", &Executor::num_slots)
      .def("synchronize",
           [](Executor& e) {
             py::gil_scoped_release nogil;
             e.synchronize();
           })
      .def("arena_ptr", &Executor::arena_ptr)
      .def("read_arena",
           [](Executor& e, int B, int64_t offset, size_t bytes) {
             py::array_t<uint8_t> out(bytes);
             {
               py::gil_scoped_release nogil;
               e.read_arena(B, offset, out.mutable_data(), bytes);
             }
             return out;
           })
      .def("weights_ptr", &Executor::weights_ptr)
      .def("set_peer_stage", &Executor::set_peer_stage)
      .def("device", &Executor::device)
      .def("submit_peer",
           [](Executor& e, Executor& src, int slot) {
             py::gil_scoped_release nogil;
             return e.submit_peer(src, slot);
           })
      .def("submit_device",
           // images: [(device_ptr, h, w, device)], boxes: per image a float32 [k, 6] array (x1, y1, x2, y2, conf,
           // class) in image coordinates
           [](Executor& e, const std::vector<std::tuple<uintptr_t, int, int, int>>& images,
              const std::vector<py::array_t<float, py::array::c_style | py::array::forcecast>>& boxes) {
             if (images.size() != boxes.size()) throw std::runtime_error("submit_device: one box array per image");
             std::vector<Executor::DeviceImage> imgs;
             std::vector<std::vector<Detection>> dets(images.size());
             for (size_t i = 0; i < images.size(); ++i) {
               Executor::DeviceImage d;
               d.ptr = std::get<0>(images[i]);
               d.h = std::get<1>(images[i]);
               d.w = std::get<2>(images[i]);
               d.device = std::get<3>(images[i]);
               imgs.push_back(d);
               const auto& b = boxes[i];
               if (b.size() == 0) continue;
               if (b.ndim() != 2 || b.shape(1) != 6) throw std::runtime_error("submit_device: boxes must be [k, 6]");
               const float* q = b.data();
               for (ssize_t k = 0; k < b.shape(0); ++k, q += 6) {
                 Detection dd{};
                 dd.x1 = q[0];
                 dd.y1 = q[1];
                 dd.x2 = q[2];
                 dd.y2 = q[3];
                 dd.conf = q[4];
                 dd.cls = (int)q[5];
                 dets[i].push_back(dd);
               }
             }
             py::gil_scoped_release nogil;
             return e.submit_device(imgs, dets);
           })
      .def("conv_choices", &Executor::conv_choices)
      .def("exec_order", &Executor::exec_order, py::arg("B"),
           "program op indices in the order bucket B's graphs launch them")
      .def("gated_ops", &Executor::gated_ops, py::arg("B"), "ops of bucket B that run with a tile gate")
      .def("launch_order", &Executor::launch_order, py::arg("B"),
           "every kernel launch of bucket B's graphs in order as (op, kind): 0 the whole op, 1 / 2 the class / "
           "box window of a split first head conv, 3 the cell marks launched before op's box conv")
      .def("stream", &Executor::stream);

  py::class_<SplitInstance, std::shared_ptr<SplitInstance>>(m, "SplitInstance")
      .def(py::init([](std::shared_ptr<Executor> det, std::shared_ptr<Executor> cls) {
        return std::make_shared<SplitInstance>(det, cls);
      }))
      .def("submit",
           [](SplitInstance& s, const py::list& imgs) {
             std::vector<py::array> keep;
             auto v = images_from(imgs, keep);
             py::gil_scoped_release nogil;
             return s.submit(v);
           })
      .def("collect",
           [](SplitInstance& s, int slot) {
             BatchResult r;
             {
               py::gil_scoped_release nogil;
               r = s.collect(slot);
             }
             return result_to_py(r, s.max_det());
           })
      .def("num_slots", &SplitInstance::num_slots)
      .def("buckets", &SplitInstance::buckets);

  py::class_<JpegSet, std::shared_ptr<JpegSet>>(m, "JpegSet")
      .def(py::init(&make_jpeg_set), py::arg("uploads"), py::arg("pinned") = true,
           "JPEG uploads entropy-decoded once into (pinned) host buffers, for Executor.submit_jpeg_set")
      .def("__len__", [](const JpegSet& s) { return s.items.size(); })
      .def("coef_bytes", [](const JpegSet& s, int i) { return (int64_t)jpeg_payload_bytes(s.items.at(i)->info); })
      .def_property_readonly("pinned", [](const JpegSet& s) {
        for (const auto& it : s.items)
          if (!it->pinned) return false;
        return true;
      });

  py::class_<EchoInstance, std::shared_ptr<EchoInstance>>(m, "EchoInstance")
      .def(py::init<int, int, int, int, int64_t, int64_t>(), py::arg("slots") = 2, py::arg("max_batch") = 32,
           py::arg("max_det") = 4, py::arg("latency_us") = 0, py::arg("staging_cap") = 0,
           py::arg("raw_out_bytes") = 0)
      .def("set_record", &EchoInstance::set_record, py::arg("on"),
           "Tests: keep the RGB pixels of every uint8 image submitted from now on (split-decoded JPEGs reconstructed).")
      .def("take_recorded", [](EchoInstance& e) {
        py::list out;
        for (auto& r : e.take_recorded()) {
          py::array_t<uint8_t> a({(py::ssize_t)r.h, (py::ssize_t)r.w, (py::ssize_t)3});
          std::memcpy(a.mutable_data(), r.rgb.data(), r.rgb.size());
          out.append(a);
        }
        return out;
      }, "The recorded HxWx3 uint8 images in submission order; the record is emptied.");

  py::class_<DynamicBatcher>(m, "DynamicBatcher")
      .def(py::init([](py::list executors, const py::dict& cfg) {
             std::vector<std::shared_ptr<BatchInstance>> inst;
             for (auto h : executors) {
               if (py::isinstance<SplitInstance>(h))
                 inst.push_back(h.cast<std::shared_ptr<SplitInstance>>());
               else if (py::isinstance<EchoInstance>(h))
                 inst.push_back(h.cast<std::shared_ptr<EchoInstance>>());
               else
                 inst.push_back(h.cast<std::shared_ptr<Executor>>());
             }
             BatcherConfig c;
             c.max_batch = get<int>(cfg, "max_batch", c.max_batch);
             c.preferred = get<std::vector<int>>(cfg, "preferred", {});
             c.max_queue_delay_us = get<int64_t>(cfg, "max_queue_delay_us", c.max_queue_delay_us);
             c.idle_queue_delay_us = get<int64_t>(cfg, "idle_queue_delay_us", c.idle_queue_delay_us);
             c.max_queue_size = get<int64_t>(cfg, "max_queue_size", c.max_queue_size);
             c.overlap = get<int>(cfg, "overlap", c.overlap);
             return new DynamicBatcher(inst, c);
           }),
           py::keep_alive<1, 2>())
      .def("enqueue",
           [](DynamicBatcher& b, py::array img_in, py::function cb, uintptr_t export_to) {
             py::array img = py::array::ensure(img_in, py::array::c_style);
             int h = 0, w = 0;
             int64_t bytes = 0;
             if (img && img.ndim() == 3 && img.shape(2) == 3 && img.itemsize() == 1) {
               h = (int)img.shape(0);
               w = (int)img.shape(1);
             } else if (img && img.ndim() == 3 && img.shape(0) == 3 && img.itemsize() == 4 &&
                        img.shape(1) == img.shape(2)) {
               h = w = (int)img.shape(1);
               bytes = (int64_t)img.nbytes();
             } else {
               throw std::runtime_error("input must be a uint8 HxWx3 image or a float32 [3,S,S] tensor");
             }
             ResultCallback f = py_result_cb(std::move(cb));
             const uint8_t* data = (const uint8_t*)img.data();
             py::gil_scoped_release nogil;
             return b.enqueue(data, h, w, std::move(f), bytes, (uint8_t*)export_to);
           },
           py::arg("img"), py::arg("cb"), py::arg("export_to") = 0)
      .def("stats",
           [](DynamicBatcher& b) {
             BatcherStats s = b.stats();
             py::dict d;
             d["requests"] = s.requests;
             d["batches"] = s.batches;
             d["rejected"] = s.rejected;
             d["failed"] = s.failed;
             d["queue_depth"] = s.queue_depth;
             d["mean_batch"] = s.batches ? s.sum_batch / s.batches : 0.0;
             d["mean_queue_us"] = s.requests ? s.sum_queue_us / s.requests : 0.0;
             d["mean_compute_us"] = s.batches ? s.sum_compute_us / s.batches : 0.0;
             d["batch_hist"] = s.batch_hist;
             d["device_faults"] = s.device_faults;
             d["last_error"] = s.last_error;
             return d;
           })
      .def("shutdown", [](DynamicBatcher& b) {
        py::gil_scoped_release nogil;
        b.shutdown();
      });

  // closed-loop HTTP load generator (bench.py --path http, serving sweeps)
  py::class_<JpegIngest>(m, "JpegIngest")
      .def(py::init([](DynamicBatcher& batcher, const py::dict& cfg) {
             IngestConfig c;
             c.threads = get<int>(cfg, "threads", c.threads);
             c.jpeg_device = get<bool>(cfg, "jpeg_device", c.jpeg_device);
             c.max_image_pixels = get<int64_t>(cfg, "max_image_pixels", c.max_image_pixels);
             if (cfg.contains("progressive") && !cfg["progressive"].is_none())  // absent: the process default
               c.progressive = cfg["progressive"].cast<bool>() ? 1 : 0;
             c.buffer_cap = get<int64_t>(cfg, "buffer_cap", c.buffer_cap);
             int ndev = 0;
             const bool gpu = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
             (void)hipGetLastError();
             if (get<bool>(cfg, "pinned", gpu)) {
               c.host_alloc = [](size_t n) -> void* {
                 void* p = nullptr;
                 if (hipHostMalloc(&p, n, hipHostMallocPortable) != hipSuccess) {
                   (void)hipGetLastError();
                   return nullptr;
                 }
                 return p;
               };
               c.host_free = [](void* p) { (void)hipHostFree(p); };
             }
             py::gil_scoped_release nogil;
             return new JpegIngest(&batcher, c);
           }),
           py::keep_alive<1, 2>())
      .def(
          "submit",
          [](JpegIngest& g, py::bytes upload, py::function done, py::function fallback, uintptr_t export_to) {
            std::string u = upload;
            std::shared_ptr<py::function> fb(new py::function(std::move(fallback)), [](py::function* fn) {
              py::gil_scoped_acquire gil;
              delete fn;
            });
            ResultCallback cb = py_result_cb(std::move(done));
            py::gil_scoped_release nogil;
            g.submit(std::move(u), std::move(cb), [fb](std::string&&) {
              py::gil_scoped_acquire gil;
              try {
                (*fb)();
              } catch (py::error_already_set& e) {
                e.discard_as_unraisable("JpegIngest fallback");
              }
            }, (uint8_t*)export_to);
          },
          py::arg("upload"), py::arg("done"), py::arg("fallback"), py::arg("export_to") = 0,
          "Split-decode `upload` into the batcher: done(result dict) after its batch; fallback() (no arguments) "
          "when the split decoder does not cover the format (the caller decodes and enqueues it itself).")
      .def("stats",
           [](JpegIngest& g) {
             IngestStats s = g.stats();
             py::dict d;
             d["native"] = s.native;
             d["fallback"] = s.fallback;
             d["errors"] = s.errors;
             d["progressive_decoded"] = s.progressive_decoded;
             d["cpu_decode_ms"] = s.cpu_decode_ms;
             return d;
           })
      .def("stop", [](JpegIngest& g) {
        py::gil_scoped_release nogil;
        g.stop();
      });

  py::class_<IpcBuffer>(m, "IpcBuffer")
      .def(py::init<size_t, int>(), py::arg("bytes"), py::arg("device") = 0)
      .def("handle", [](const IpcBuffer& b) { return py::bytes(b.handle()); })
      .def_property_readonly("ptr", &IpcBuffer::ptr)
      .def_property_readonly("size", &IpcBuffer::size)
      .def_property_readonly("device", &IpcBuffer::device)
      .def("write",
           [](IpcBuffer& b, size_t off, py::buffer data) {
             py::buffer_info bi = data.request();
             const size_t n = (size_t)bi.size * (size_t)bi.itemsize;
             py::gil_scoped_release nogil;
             b.write(off, bi.ptr, n);
           })
      .def("read", [](const IpcBuffer& b, size_t off, size_t n) {
        std::string out(n, '\0');
        {
          py::gil_scoped_release nogil;
          b.read(off, out.data(), n);
        }
        return py::bytes(out);
      });
  m.def("ipc_open", [](py::bytes handle, int device, int src_device) {
    return ipc_open(std::string(handle), device, src_device);
  }, py::arg("handle"), py::arg("device") = 0, py::arg("src_device") = -1);
  m.def("ipc_close", &ipc_close);
  m.def("ipc_open_range", [](py::bytes handle, int device, int src_device) {
    const uintptr_t p = ipc_open(std::string(handle), device, src_device);
    return py::make_tuple(p, ipc_mapped_bytes(p));
  }, py::arg("handle"), py::arg("device") = 0, py::arg("src_device") = -1,
     "ipc_open + the mapped size: (device pointer, bytes); src_device >= 0 is checked for peer access first");
  m.def("can_access_peer", &hip_can_access_peer, py::arg("dst"), py::arg("src"), "hipDeviceCanAccessPeer");
  m.def("require_peer_access", [](int dst, int src, const std::string& what, py::object can) {
    PeerQuery q = hip_can_access_peer;
    if (!can.is_none()) q = [can](int d, int s) { py::gil_scoped_acquire g; return can(d, s).cast<int>(); };
    require_peer_access(dst, src, what.c_str(), q);
  }, py::arg("dst"), py::arg("src"), py::arg("what") = "peer copy", py::arg("can_access") = py::none(),
     "runtime/peer.h policy; can_access(dst, src) -> int overrides hipDeviceCanAccessPeer (tests)");

  // BodyCapture -> {"body": [bytes per request], "at": int64 completion index of each (-1: none)}
  auto bodies_py = [](const BodyCapture& c) {
    py::list body;
    for (const std::string& b : c.body) body.append(py::bytes(b));
    py::array_t<int64_t> at((py::ssize_t)c.at.size());
    for (size_t i = 0; i < c.at.size(); ++i) at.mutable_data()[i] = c.at[i];
    py::dict d;
    d["body"] = body;
    d["at"] = at;
    return d;
  };
  py::class_<HttpLoadGen>(m, "HttpLoadGen")
      .def(py::init([](const py::dict& cfg, const py::list& requests) {
             LoadGenConfig c;
             c.host = get<std::string>(cfg, "host", c.host);
             c.port = get<int>(cfg, "port", c.port);
             c.users = get<int>(cfg, "users", c.users);
             c.threads = get<int>(cfg, "threads", c.threads);
             c.max_requests = get<int64_t>(cfg, "max_requests", c.max_requests);
             c.keep_bodies = get<bool>(cfg, "keep_bodies", c.keep_bodies);
             std::vector<std::string> reqs;
             for (auto r : requests) reqs.push_back(r.cast<std::string>());
             return new HttpLoadGen(c, std::move(reqs));
           }))
      .def("start", [](HttpLoadGen& g) {
        py::gil_scoped_release nogil;
        g.start();
      })
      .def(
          "stop",
          [](HttpLoadGen& g, double timeout_s) {
            py::gil_scoped_release nogil;
            g.stop(timeout_s);
          },
          py::arg("timeout_s") = 30.0)
      .def("completed", &HttpLoadGen::completed)
      .def("connect_failures", &HttpLoadGen::connect_failures)
      .def("capture_until", &HttpLoadGen::capture_until, py::arg("n"))
      .def("bodies", [bodies_py](HttpLoadGen& g) { return bodies_py(g.bodies()); })
      .def(
          "wait_completed",
          [](HttpLoadGen& g, int64_t n, double timeout_s) {
            py::gil_scoped_release nogil;
            return g.wait_completed(n, timeout_s);
          },
          py::arg("n"), py::arg("timeout_s") = 600.0)
      .def(
          "records",
          [](HttpLoadGen& g, int64_t from, int64_t to) {
            std::vector<LoadGenRecord> r = g.records(from, to);
            py::array_t<double> t((py::ssize_t)r.size());
            py::array_t<float> lat((py::ssize_t)r.size());
            py::array_t<int16_t> st((py::ssize_t)r.size()), dets((py::ssize_t)r.size());
            for (size_t i = 0; i < r.size(); ++i) {
              t.mutable_data()[i] = r[i].t_done;
              lat.mutable_data()[i] = r[i].latency;
              st.mutable_data()[i] = r[i].status;
              dets.mutable_data()[i] = r[i].dets;
            }
            py::dict d;
            d["t_done"] = t;
            d["latency"] = lat;
            d["status"] = st;
            d["dets"] = dets;
            return d;
          },
          py::arg("from") = 0, py::arg("to") = -1);

  auto records_py = [](const std::vector<LoadGenRecord>& r) {
    py::array_t<double> t((py::ssize_t)r.size());
    py::array_t<float> lat((py::ssize_t)r.size());
    py::array_t<int16_t> st((py::ssize_t)r.size()), dets((py::ssize_t)r.size());
    for (size_t i = 0; i < r.size(); ++i) {
      t.mutable_data()[i] = r[i].t_done;
      lat.mutable_data()[i] = r[i].latency;
      st.mutable_data()[i] = r[i].status;
      dets.mutable_data()[i] = r[i].dets;
    }
    py::dict d;
    d["t_done"] = t;
    d["latency"] = lat;
    d["status"] = st;
    d["dets"] = dets;
    return d;
  };
  py::class_<LocalLoadGen>(m, "LocalLoadGen")
      .def(py::init([](HttpFrontEnd& fe, const py::list& uploads, int users) {
             std::vector<std::string> u;
             for (auto r : uploads) u.push_back(r.cast<std::string>());
             return new LocalLoadGen(&fe, std::move(u), users);
           }),
           py::keep_alive<1, 2>())
      .def("start", [](LocalLoadGen& g) {
        py::gil_scoped_release nogil;
        g.start();
      })
      .def(
          "stop",
          [](LocalLoadGen& g, double timeout_s) {
            py::gil_scoped_release nogil;
            g.stop(timeout_s);
          },
          py::arg("timeout_s") = 30.0)
      .def("completed", &LocalLoadGen::completed)
      .def("keep_bodies", &LocalLoadGen::keep_bodies)
      .def("capture_until", &LocalLoadGen::capture_until, py::arg("n"))
      .def("bodies", [bodies_py](LocalLoadGen& g) { return bodies_py(g.bodies()); })
      .def(
          "wait_completed",
          [](LocalLoadGen& g, int64_t n, double timeout_s) {
            py::gil_scoped_release nogil;
            return g.wait_completed(n, timeout_s);
          },
          py::arg("n"), py::arg("timeout_s") = 600.0)
      .def(
          "records", [records_py](LocalLoadGen& g, int64_t from, int64_t to) { return records_py(g.records(from, to)); },
          py::arg("from") = 0, py::arg("to") = -1);

  py::class_<HttpFrontEnd>(m, "HttpFrontEnd")
      .def(py::init([](DynamicBatcher& batcher, const py::dict& ch, std::vector<std::string> labels,
                       const py::dict& cfg) {
             DecodeChannel dc;
             dc.shm = (uint8_t*)(uintptr_t)get<int64_t>(ch, "shm_addr", 0);
             dc.stride = get<int64_t>(ch, "stride", 0);
             dc.in_bytes = get<int64_t>(ch, "in_bytes", 0);
             dc.slot_bytes = get<int64_t>(ch, "slot_bytes", 0);
             dc.slots = get<int>(ch, "slots", 0);
             dc.task_fds = get<std::vector<int>>(ch, "task_fds", {});
             dc.big_fds = get<std::vector<int>>(ch, "big_fds", {});
             dc.result_fd = get<int>(ch, "result_fd", -1);
             dc.result_wfd = get<int>(ch, "result_wfd", -1);
             FrontConfig c;
             c.host = get<std::string>(cfg, "host", c.host);
             c.port = get<int>(cfg, "port", c.port);
             c.io_threads = get<int>(cfg, "io_threads", c.io_threads);
             c.reuse_port = get<bool>(cfg, "reuse_port", c.reuse_port);
             c.softmax_confidence = get<bool>(cfg, "softmax_confidence", c.softmax_confidence);
             c.max_body = get<int64_t>(cfg, "max_body", c.max_body);
             c.replica_tag = get<std::string>(cfg, "replica_tag", c.replica_tag);
             c.idle_timeout_ms = get<int64_t>(cfg, "idle_timeout_ms", c.idle_timeout_ms);
             c.read_timeout_ms = get<int64_t>(cfg, "read_timeout_ms", c.read_timeout_ms);
             c.decode_threads = get<int>(cfg, "decode_threads", c.decode_threads);
             c.jpeg_device = get<bool>(cfg, "jpeg_device", c.jpeg_device);
             c.max_image_pixels = get<int64_t>(cfg, "max_image_pixels", c.max_image_pixels);
             if (cfg.contains("progressive") && !cfg["progressive"].is_none())  // absent: the process default
               c.progressive = cfg["progressive"].cast<bool>() ? 1 : 0;
             c.decode_buffer_cap = get<int64_t>(cfg, "decode_buffer_cap", c.decode_buffer_cap);
             c.kserve_model = get<std::string>(cfg, "kserve_model", c.kserve_model);
             c.body_pool_depth = get<int>(cfg, "body_pool_depth", c.body_pool_depth);
             if (cfg.contains("tensor_models"))  // dicts as tensor_model_of + "batcher" (kept alive with cfg)
               for (auto h : cfg["tensor_models"].cast<py::list>()) {
                 const py::dict td = h.cast<py::dict>();
                 TensorModelEntry e;
                 e.model = tensor_model_of(td);
                 e.batcher = &td["batcher"].cast<DynamicBatcher&>();
                 c.tensor_models.push_back(std::move(e));
               }
             // decoded uploads live in pinned memory when a GPU is present (the executor DMAs from them)
             int ndev = 0;
             const bool gpu = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
             (void)hipGetLastError();
             if (get<bool>(cfg, "pinned", gpu)) {
               c.host_alloc = [](size_t n) -> void* {
                 void* p = nullptr;
                 if (hipHostMalloc(&p, n, hipHostMallocPortable) != hipSuccess) {
                   (void)hipGetLastError();
                   return nullptr;
                 }
                 return p;
               };
               c.host_free = [](void* p) { (void)hipHostFree(p); };
             }
             py::gil_scoped_release nogil;
             return new HttpFrontEnd(&batcher, dc, std::move(labels), c);
           }),
           py::keep_alive<1, 2>(), py::keep_alive<1, 5>())
      // handler mode: HTTP/multipart natively, the request handler in Python (take / complete)
      .def(py::init([](const py::dict& cfg) {
        FrontConfig c;
        c.host = get<std::string>(cfg, "host", c.host);
        c.port = get<int>(cfg, "port", c.port);
        c.io_threads = get<int>(cfg, "io_threads", c.io_threads);
        c.reuse_port = get<bool>(cfg, "reuse_port", c.reuse_port);
        c.max_body = get<int64_t>(cfg, "max_body", c.max_body);
        c.replica_tag = get<std::string>(cfg, "replica_tag", c.replica_tag);
        c.max_handler_queue = get<int>(cfg, "max_queue", c.max_handler_queue);
        c.idle_timeout_ms = get<int64_t>(cfg, "idle_timeout_ms", c.idle_timeout_ms);
        c.read_timeout_ms = get<int64_t>(cfg, "read_timeout_ms", c.read_timeout_ms);
        c.handler_mode = true;
        py::gil_scoped_release nogil;
        return new HttpFrontEnd(nullptr, DecodeChannel{}, {}, c);
      }))
      .def_property_readonly("handler_mode", &HttpFrontEnd::handler_mode)
      .def("drain", [](HttpFrontEnd& f) {
        py::gil_scoped_release nogil;
        f.drain();
      })
      .def("handler_pending", &HttpFrontEnd::handler_pending)
      .def(
          "take",
          [](HttpFrontEnd& f, int max_n, int timeout_ms) {
            std::vector<HandlerRequest> v;
            {
              py::gil_scoped_release nogil;
              v = f.take(max_n, timeout_ms);
            }
            py::list out;
            for (auto& r : v) out.append(py::make_tuple(r.key, py::bytes(r.data)));
            return out;
          },
          py::arg("max_n") = 64, py::arg("timeout_ms") = 100)
      .def(
          "complete",
          [](HttpFrontEnd& f, uint64_t key, int code, const std::string& body, int n_det) {
            py::gil_scoped_release nogil;
            return f.complete(key, code, body, n_det);
          },
          py::arg("key"), py::arg("code"), py::arg("body"), py::arg("n_det") = 0)
      .def_property_readonly("port", &HttpFrontEnd::port)
      .def("set_healthy", &HttpFrontEnd::set_healthy)
      .def("upstream_forwarded", &HttpFrontEnd::upstream_forwarded)
      .def("set_metrics_text", &HttpFrontEnd::set_metrics_text)
      .def("stats",
           [](HttpFrontEnd& f) {
             FrontStats s = f.stats();
             py::dict d;
             d["requests"] = s.requests;
             d["ok"] = s.ok;
             d["bad_request"] = s.bad_request;
             d["too_large"] = s.too_large;
             d["unavailable"] = s.unavailable;
             d["errors"] = s.errors;
             d["not_found"] = s.not_found;
             d["connections"] = s.connections;
             d["open_connections"] = s.open_connections;
             d["detections"] = s.detections;
             d["timeouts"] = s.timeouts;
             d["sum_total_ms"] = s.sum_total_ms;
             d["sum_decode_ms"] = s.sum_decode_ms;
             d["sum_queue_ms"] = s.sum_queue_ms;
             d["sum_gpu_ms"] = s.sum_gpu_ms;
             d["native_decoded"] = s.native_decoded;
             d["fallback_decoded"] = s.fallback_decoded;
             d["oriented_decoded"] = s.oriented_decoded;
             d["layout_decoded"] = s.layout_decoded;
             d["progressive_decoded"] = s.progressive_decoded;
             d["bodies_recycled"] = s.bodies_recycled;
             d["bodies_allocated"] = s.bodies_allocated;
             d["bodies_retained_bytes"] = s.bodies_retained_bytes;
             d["bodies_budget_bytes"] = s.bodies_budget_bytes;
             d["bodies_over_budget"] = s.bodies_over_budget;
             py::dict tms;
             for (const TensorModelStats& t : s.tensor_models) {
               py::dict e;
               e["requests"] = t.requests;
               e["items"] = t.items;
               e["ok"] = t.ok;
               e["failed"] = t.failed;
               e["request_us"] = t.request_us;
               e["queue_us"] = t.queue_us;
               e["compute_us"] = t.compute_us;
               tms[py::str(t.name)] = e;
             }
             d["tensor_models"] = tms;
             d["cpu_parse_ms"] = s.cpu_parse_ms;
             d["cpu_decode_ms"] = s.cpu_decode_ms;
             d["cpu_json_ms"] = s.cpu_json_ms;
             py::dict st;
             for (size_t k = 0; k < kStages.size() && k < s.stage_hist.size(); ++k)
               st[py::str(kStages[k])] = py::make_tuple(s.stage_hist[k], s.stage_sum_ms[k]);
             d["stages"] = st;
             d["latency_hist"] = s.latency_hist;
             d["latency_buckets_ms"] = kLatencyBucketsMs;
             return d;
           })
      .def("stop", [](HttpFrontEnd& f) {
        py::gil_scoped_release nogil;
        f.stop();
      });
  // tensor-model wire layer (runtime/kserve.h) on its own, for tests: the parser raises ValueError with the
  // message a client would get in the 400 body
  m.def("kserve_parse_tensor_input", [](const std::string& body, int64_t ihcl, const py::dict& model) {
    KServeTensorRequest r;
    std::string err;
    if (!kserve_parse_tensor_input(body, ihcl, tensor_model_of(model), r, err)) throw py::value_error(err);
    py::dict d;
    d["id"] = r.id;
    d["off"] = r.off;
    d["n"] = r.n;
    d["item_bytes"] = r.item_bytes;
    d["batch_dim"] = r.batch_dim;
    return d;
  });
  m.def("kserve_build_tensor_response",
        [](const py::dict& model, const std::string& id, bool batch_dim, const std::vector<std::string>& items) {
          std::vector<std::vector<uint8_t>> raw;
          for (const std::string& s : items) raw.emplace_back(s.begin(), s.end());
          std::vector<const std::vector<uint8_t>*> ptrs;
          for (const auto& v : raw) ptrs.push_back(&v);
          int64_t ihcl = -1;
          const std::string out = kserve_build_tensor_response(tensor_model_of(model), id, batch_dim, ptrs, &ihcl);
          return py::make_tuple(py::bytes(out), ihcl);
        });
  m.def("kserve_tensor_model_metadata",
        [](const py::dict& model) { return kserve_tensor_model_metadata(tensor_model_of(model)); });
  // native gateway: /predict forwarded to a model server's KServe endpoint (FrontConfig upstream_*)
  m.def(
      "http_proxy_front",
      [](std::vector<std::string> labels, const py::dict& cfg) {
        FrontConfig c;
        c.host = get<std::string>(cfg, "host", c.host);
        c.port = get<int>(cfg, "port", c.port);
        c.io_threads = get<int>(cfg, "io_threads", c.io_threads);
        c.reuse_port = get<bool>(cfg, "reuse_port", c.reuse_port);
        c.softmax_confidence = get<bool>(cfg, "softmax_confidence", c.softmax_confidence);
        c.max_body = get<int64_t>(cfg, "max_body", c.max_body);
        c.replica_tag = get<std::string>(cfg, "replica_tag", c.replica_tag);
        c.idle_timeout_ms = get<int64_t>(cfg, "idle_timeout_ms", c.idle_timeout_ms);
        c.read_timeout_ms = get<int64_t>(cfg, "read_timeout_ms", c.read_timeout_ms);
        c.upstream_host = get<std::string>(cfg, "upstream_host", c.upstream_host);
        c.upstream_port = get<int>(cfg, "upstream_port", 0);
        c.upstream_model = get<std::string>(cfg, "upstream_model", c.upstream_model);
        c.upstream_conns = get<int>(cfg, "upstream_conns", c.upstream_conns);
        c.upstreams = get<std::string>(cfg, "upstreams", c.upstreams);
        if (c.upstream_port <= 0) throw std::runtime_error("http_proxy_front: upstream_port required");
        py::gil_scoped_release nogil;
        return new HttpFrontEnd(nullptr, DecodeChannel{}, std::move(labels), c);
      },
      py::return_value_policy::take_ownership, py::arg("labels"), py::arg("cfg"));
}
