// pybind11 bindings of the split JPEG decoder (runtime/jpeg_decode.h, kernels/jpeg_idct.hip): the host
// entropy decoder and reference reconstruction for tests / host-only decoding, and a stand-alone device
// reconstruction of a list of uploads (the kernel-vs-reference tests; the serving path runs the same kernels
// inside Executor::submit) — and of the split JPEG crop encoder (runtime/jpeg_encode.h, kernels/jpeg_fdct.hip): the
// host encoder and reference arithmetic, a stand-alone device encode of the crops of one frame, the device entropy
// coder (kernels/jpeg_huff.hip) alone and its phases on the host, and the CropJpegEncoder the detection service drives.
#include <hip/hip_runtime.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <future>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "kernels/jpeg_desc.h"
#include "kernels/jpeg_huff_math.h"
#include "kernels/launch.h"
#include "runtime/jpeg_decode.h"
#include "runtime/jpeg_encode.h"

namespace py = pybind11;

namespace arena {

namespace {

const char* status_name(JpegStatus s) {
  return s == JpegStatus::Ok ? "ok" : (s == JpegStatus::Unsupported ? "unsupported" : "corrupt");
}

py::dict info_dict(const JpegInfo& in) {
  py::dict d;
  d["width"] = in.width;
  d["height"] = in.height;
  d["ncomp"] = in.ncomp;
  d["layout"] = in.layout;
  d["rh"] = in.rh;
  d["rv"] = in.rv;
  d["rgb_coded"] = in.rgb_coded;
  d["multiscan"] = in.multiscan;
  d["orientation"] = in.orientation;
  d["out_width"] = in.out_width;
  d["out_height"] = in.out_height;
  d["mcux"] = in.mcux;
  d["mcuy"] = in.mcuy;
  d["restart_interval"] = in.restart_interval;
  d["progressive"] = in.progressive;
  d["coef_count"] = in.coef_count;
  py::list comps;
  for (int c = 0; c < in.ncomp; ++c) {
    const JpegCompDesc& k = in.comp[c];
    py::dict e;
    e["h"] = k.h;
    e["v"] = k.v;
    e["bw"] = k.bw;
    e["bh"] = k.bh;
    e["cw"] = k.cw;
    e["ch"] = k.ch;
    e["coef_off"] = k.coef_off;
    comps.append(e);
  }
  d["comps"] = comps;
  return d;
}

struct Parsed {
  JpegInfo info;
  std::vector<int16_t> coef;
};

// progressive: None = the process default (jpeg_progressive_enabled), else the per-call switch of jpeg_parse
int progressive_arg(const py::object& o) { return o.is_none() ? -1 : (o.cast<bool>() ? 1 : 0); }

JpegStatus parse_decode(const std::string& data, Parsed& p, std::string& err, int64_t max_pixels, int progressive) {
  const uint8_t* b = (const uint8_t*)data.data();
  JpegStatus st = jpeg_parse(b, data.size(), p.info, err, max_pixels, progressive);
  if (st != JpegStatus::Ok) return st;
  p.coef.assign((size_t)p.info.coef_count, 0);
  return jpeg_decode_coefs(b, data.size(), p.info, p.coef.data(), err);
}

void check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e) + " (" + what + ")");
}

int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// ---- crop encoder ---------------------------------------------------------------------------------------------

using U8Array = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>;

void check_rgb(const U8Array& a, const char* what) {
  if (a.ndim() != 3 || a.shape(2) != 3 || a.shape(0) < 1 || a.shape(1) < 1)
    throw std::invalid_argument(std::string(what) + " must be HxWx3 uint8 with H, W >= 1");
  if (a.shape(0) > 65535 || a.shape(1) > 65535) throw std::invalid_argument(std::string(what) + " is too large for a JPEG");
}

py::bytes to_bytes(const std::vector<uint8_t>& v) { return py::bytes((const char*)v.data(), v.size()); }

// rows of at least four numbers (x1, y1, x2, y2, ...): a list of sequences or an N x >=4 array
std::vector<CropBox> to_boxes(const py::object& boxes) {
  std::vector<CropBox> out;
  for (py::handle h : boxes) {
    py::sequence r = py::reinterpret_borrow<py::sequence>(h);
    if (py::len(r) < 4) throw std::invalid_argument("a box needs x1, y1, x2, y2");
    out.push_back({r[0].cast<double>(), r[1].cast<double>(), r[2].cast<double>(), r[3].cast<double>()});
  }
  return out;
}

constexpr uint8_t kZigzagToNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                          12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                          58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Upload `frame`, encode `boxes` with a CropJpegEncoder of its own, check the guards around its device buffer.
py::dict encode_device(const U8Array& frame, const py::object& boxes, int device, int64_t capacity_bytes,
                       bool want_coefs, const std::string& entropy) {
  check_rgb(frame, "frame");
  const int h = (int)frame.shape(0), w = (int)frame.shape(1);
  std::vector<CropBox> bx = to_boxes(boxes);
  const size_t bytes = (size_t)h * w * 3;
  CropJpegEncoder::Blobs blobs;
  std::vector<std::vector<int16_t>> coefs;
  std::string err;
  int64_t launches = 0, d2h_bytes = 0, fallbacks = 0;
  if (entropy != "host" && entropy != "gpu") throw std::invalid_argument("entropy is 'host' or 'gpu'");
  {
    py::gil_scoped_release nogil;
    check(hipSetDevice(device), "hipSetDevice");
    uint8_t* d_frame = nullptr;
    check(hipMalloc((void**)&d_frame, bytes), "hipMalloc frame");
    try {
      check(hipMemcpy(d_frame, frame.data(), bytes, hipMemcpyHostToDevice), "H2D frame");
      CropJpegEncoder enc(device, capacity_bytes, 2, kCropJpegQuality, entropy);
      enc.keep_coefs = want_coefs;
      std::promise<void> p;
      enc.submit(d_frame, h, w, std::move(bx), [&](CropJpegEncoder::Blobs&& b, std::string&& e) {
        blobs = std::move(b);
        err = std::move(e);
        p.set_value();
      }, (int64_t)bytes);
      p.get_future().wait();
      enc.stop();
      if (err.empty()) err = enc.check_guards();
      coefs = std::move(enc.last_coefs);
      launches = enc.launches();
      d2h_bytes = enc.d2h_bytes();
      fallbacks = enc.entropy_fallbacks();
    } catch (...) {
      (void)hipFree(d_frame);
      throw;
    }
    (void)hipFree(d_frame);
  }
  if (!err.empty()) throw std::runtime_error("jpeg_encode_device: " + err);
  py::dict out;
  py::list bl;
  for (const auto& b : blobs) bl.append(to_bytes(b));
  out["blobs"] = bl;
  out["launches"] = launches;
  out["d2h_bytes"] = d2h_bytes;
  out["entropy_fallbacks"] = fallbacks;
  if (want_coefs) {
    py::list cl;
    for (const auto& c : coefs) {  // device layout: natural order; handed out in zigzag order like the host oracle
      py::array_t<int16_t> a({(py::ssize_t)(c.size() / 64), (py::ssize_t)64});
      int16_t* dst = a.mutable_data();
      for (size_t b = 0; b < c.size() / 64; ++b)
        for (int z = 0; z < 64; ++z) dst[b * 64 + z] = c[b * 64 + kZigzagToNatural[z]];
      cl.append(a);
    }
    out["coefs"] = cl;
  }
  return out;
}

using I16Array = py::array_t<int16_t, py::array::c_style | py::array::forcecast>;

void check_coefs(int w, int h, const I16Array& coefs, bool domain) {
  if (w < 1 || h < 1 || w > 65535 || h > 65535) throw std::invalid_argument("bad size");
  if (coefs.size() != jpeg_enc_blocks(w, h) * 64) throw std::invalid_argument("coefficient count does not match the size");
  if (!domain) return;
  const int16_t* p = coefs.data();
  for (py::ssize_t i = 0; i < coefs.size(); ++i)
    if (p[i] > jpegh::kMaxCoef || p[i] < -jpegh::kMaxCoef)
      throw std::invalid_argument("a coefficient lies outside +-1023, the entropy coder's domain");
}

// The entropy kernels alone over one crop's coefficient blocks, with buffers of their own between guards.
py::dict entropy_device(int w, int h, const I16Array& coefs, int device, int reserve_per_block, bool natural) {
  check_coefs(w, h, coefs, true);
  const int64_t slots = jpeg_enc_blocks(w, h), cbytes = slots * 128;
  if (slots > 9600) throw std::invalid_argument("more block slots than a 640 x 640 frame slot has");
  const JpegEncTables t = jpeg_enc_tables(kCropJpegQuality);
  std::vector<uint8_t> blob;
  JpegEntResult rec{};
  int64_t fallbacks = 0;
  std::string err;
  {
    py::gil_scoped_release nogil;
    constexpr int64_t kGuard = JpegEntropyDevice::kGuard;
    constexpr int kGuardByte = JpegEntropyDevice::kGuardByte;
    check(hipSetDevice(device), "hipSetDevice");
    uint8_t* d_alloc = nullptr;
    hipStream_t s = nullptr;
    check(hipMalloc((void**)&d_alloc, (size_t)(cbytes + 2 * kGuard)), "hipMalloc coefficients");
    try {
      check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
      check(hipMemset(d_alloc, kGuardByte, (size_t)(cbytes + 2 * kGuard)), "hipMemset guards");
      check(hipMemcpy(d_alloc + kGuard, coefs.data(), (size_t)cbytes, hipMemcpyHostToDevice), "H2D coefficients");
      JpegEncDesc e{};
      e.w = w;
      e.h = h;
      e.mcux = (w + 15) / 16;
      e.total_blocks = (int32_t)slots;
      std::vector<JpegEntDesc> descs;
      JpegEntropyDevice ent(slots, align256(slots * std::max(reserve_per_block, 1)), 1);
      err = ent.plan({e}, reserve_per_block, descs);
      if (err.empty()) err = ent.launch(descs, d_alloc + kGuard, natural, s);
      if (err.empty()) {
        check(hipMemcpyAsync(&rec, ent.d_res(), sizeof(rec), hipMemcpyDeviceToHost, s), "D2H record");
        check(hipStreamSynchronize(s), "jpeg_entropy");
        if (rec.status == jpegh::kEntropyOk) {
          if (rec.scan_bytes > (uint32_t)descs[0].reserve) throw std::runtime_error("inconsistent entropy record");
          blob = jpeg_write_header(w, h, t);
          const size_t at = blob.size();
          blob.resize(at + rec.scan_bytes + 2);
          check(hipMemcpy(blob.data() + at, ent.d_out(), rec.scan_bytes, hipMemcpyDeviceToHost), "D2H scan");
          blob[at + rec.scan_bytes] = 0xFF;
          blob[at + rec.scan_bytes + 1] = 0xD9;
        } else {  // overflow: the coefficients come back and the host codes them
          std::vector<int16_t> back((size_t)slots * 64);
          check(hipMemcpy(back.data(), d_alloc + kGuard, (size_t)cbytes, hipMemcpyDeviceToHost), "D2H coefficients");
          blob = jpeg_write(w, h, back.data(), t, natural);
          fallbacks = 1;
        }
        err = ent.check_guards();
        uint8_t g[2 * kGuard];
        check(hipMemcpy(g, d_alloc, (size_t)kGuard, hipMemcpyDeviceToHost), "D2H guards");
        check(hipMemcpy(g + kGuard, d_alloc + kGuard + cbytes, (size_t)kGuard, hipMemcpyDeviceToHost), "D2H guards");
        for (int64_t k = 0; k < 2 * kGuard && err.empty(); ++k)
          if (g[k] != kGuardByte) err = "the entropy kernels wrote outside the coefficient buffer";
      }
    } catch (...) {
      if (s) (void)hipStreamDestroy(s);
      (void)hipFree(d_alloc);
      throw;
    }
    (void)hipStreamDestroy(s);
    (void)hipFree(d_alloc);
  }
  if (!err.empty()) throw std::runtime_error("jpeg_entropy_device: " + err);
  py::dict out;
  out["blob"] = to_bytes(blob);
  out["status"] = rec.status == jpegh::kEntropyOk ? "ok" : "overflow";
  out["bits"] = (int64_t)rec.total_bits;
  out["scan_bytes"] = (int64_t)rec.scan_bytes;
  out["fallbacks"] = fallbacks;
  return out;
}

}  // namespace

void bind_jpeg(py::module& m) {
  m.attr("SIZEOF_JPEG_DESC") = (int)sizeof(JpegDesc);

  m.def("jpeg_progressive_default", &jpeg_progressive_enabled,
        "Process default of the progressive switch (ARENA_JPEG_PROGRESSIVE, default 0): what progressive=None means.");
  m.def("set_jpeg_progressive_default", &jpeg_set_progressive_enabled, py::arg("on"),
        "Replace the process default of the progressive switch; returns the previous value.  Executor.run on encoded\n"
        "bytes and every config without a \"progressive\" key follow it.");

  m.def(
      "jpeg_coefs",
      [](py::bytes data, int64_t max_pixels, py::object progressive, bool compact) {
        std::string s = data;
        Parsed p;
        std::string err;
        JpegStatus st;
        const int prog = progressive_arg(progressive);
        bool fits = true;
        {
          py::gil_scoped_release nogil;
          if (!compact) {
            st = parse_decode(s, p, err, max_pixels, prog);
          } else {  // through the serving paths' payload: jpeg_decode_compact, expanded again
            st = jpeg_parse((const uint8_t*)s.data(), s.size(), p.info, err, max_pixels, prog);
            if (st == JpegStatus::Ok) {
              std::vector<uint8_t> payload((size_t)jpeg_compact_capacity(p.info));
              st = jpeg_decode_compact((const uint8_t*)s.data(), s.size(), p.info, payload.data(), err);
              if (st == JpegStatus::Ok) {
                fits = p.info.compact_bytes <= (int64_t)payload.size();
                p.coef.assign((size_t)p.info.coef_count, 0);
                jpeg_compact_to_dense(p.info, payload.data(), p.coef.data());
              }
            }
          }
        }
        if (!fits) throw std::runtime_error("jpeg_coefs: the compact payload exceeds jpeg_compact_capacity");
        py::dict out = info_dict(p.info);
        if (compact) out["compact_bytes"] = p.info.compact_bytes;
        out["status"] = status_name(st);
        out["error"] = err;
        py::array_t<int16_t> a((py::ssize_t)p.coef.size());
        if (!p.coef.empty()) std::memcpy(a.mutable_data(), p.coef.data(), p.coef.size() * sizeof(int16_t));
        out["coef"] = a;
        return out;
      },
      py::arg("data"), py::arg("max_pixels") = 0, py::arg("progressive") = py::none(), py::arg("compact") = false,
      "Host entropy decode: dict(status, error, geometry, comps, coef=int16 natural-order blocks).  layout: 0 grey,\n"
      "1 4:4:4, 2 4:2:2, 3 4:2:0, 4 4:4:0 (h1v2 fancy), 5 box (each chroma sample over rh x rv pixels); rgb_coded:\n"
      "no YCbCr step; multiscan: a sequential file whose scans are walked.  progressive:\n"
      "accept SOF2 files (None = the process default, ARENA_JPEG_PROGRESSIVE).  compact=True decodes into the\n"
      "compact payload and expands it (adds compact_bytes).");

  m.def(
      "jpeg_decode_host",
      [](py::bytes data, int64_t max_pixels, py::object progressive) -> py::object {
        std::string s = data;
        Parsed p;
        std::string err;
        JpegStatus st;
        std::vector<uint8_t> rgb;
        const int prog = progressive_arg(progressive);
        {
          py::gil_scoped_release nogil;
          st = parse_decode(s, p, err, max_pixels, prog);
          if (st == JpegStatus::Ok) {
            rgb.resize((size_t)p.info.width * p.info.height * 3);
            jpeg_coefs_to_rgb(p.info, p.coef.data(), rgb.data());
          }
        }
        if (st != JpegStatus::Ok) return py::make_tuple(status_name(st), err, py::none());
        py::array_t<uint8_t> a({(py::ssize_t)p.info.out_height, (py::ssize_t)p.info.out_width, (py::ssize_t)3});
        std::memcpy(a.mutable_data(), rgb.data(), rgb.size());
        return py::make_tuple("ok", std::string(), a);
      },
      py::arg("data"), py::arg("max_pixels") = 0, py::arg("progressive") = py::none(),
      "Whole decode on the host with the device kernels' arithmetic: (status, error, HxWx3 uint8 in the EXIF\n"
      "orientation, or None).  progressive: accept SOF2 files (None = the process default).");

  m.def(
      "jpeg_decode_device",
      [](std::vector<py::bytes> uploads, int device, bool guard, py::object progressive, bool compact, bool ragged) {
        const int n = (int)uploads.size();
        const int prog = progressive_arg(progressive);
        std::vector<Parsed> ps(n);
        std::vector<std::vector<uint8_t>> payload(n);  // compact=True: what the serving paths ship
        std::vector<JpegDesc> descs(n);
        int64_t off = 0, max_blocks = 0, max_pix = 0;
        bool oriented = false, general = false;
        // guard: kGuard bytes of kGuardByte right before and right after every RGB region (not rounded up to the
        // pool's alignment, so one byte past the frame already lands in them), checked after the kernels
        constexpr int64_t kGuard = 256;
        constexpr int kGuardByte = 0xA5;
        std::vector<int64_t> coef_base(n), rgb_off(n);
        for (int i = 0; i < n; ++i) {
          std::string err;
          const std::string s = uploads[i];
          JpegStatus st;
          if (!compact) {
            st = parse_decode(s, ps[i], err, 0, prog);
          } else {
            st = jpeg_parse((const uint8_t*)s.data(), s.size(), ps[i].info, err, 0, prog);
            if (st == JpegStatus::Ok) {
              payload[i].resize((size_t)jpeg_compact_capacity(ps[i].info));
              st = jpeg_decode_compact((const uint8_t*)s.data(), s.size(), ps[i].info, payload[i].data(), err);
            }
            if (st == JpegStatus::Ok && ps[i].info.compact_bytes > (int64_t)payload[i].size())
              throw std::runtime_error("jpeg_decode_device: the compact payload exceeds jpeg_compact_capacity");
          }
          if (st != JpegStatus::Ok) throw std::invalid_argument("upload " + std::to_string(i) + ": " + err);
          const JpegInfo& in = ps[i].info;
          if (guard) off += kGuard;
          rgb_off[i] = off;
          off = align256(off + (int64_t)in.width * in.height * 3 + (guard ? kGuard : 0));
          oriented |= in.orientation > 1;
          general |= in.orientation > 1 || jpeg_needs_general(in.layout, in.rgb_coded);
          coef_base[i] = off;
          off = align256(off + jpeg_payload_bytes(in));
          descs[i] = jpeg_device_desc(in, coef_base[i], off, rgb_off[i]);
          off = align256(off + in.plane_bytes);
          max_blocks = std::max<int64_t>(max_blocks, descs[i].total_blocks);
          max_pix = std::max<int64_t>(max_pix, (int64_t)in.width * in.height);
        }
        JpegRaggedPlan rplan;
        if (ragged) rplan = jpeg_ragged_plan(descs.data(), n);
        py::list out;
        if (n == 0) return out;
        check(hipSetDevice(device), "hipSetDevice");
        uint8_t* pool = nullptr;
        JpegDesc* dd = nullptr;
        check(hipMalloc(&pool, (size_t)off), "hipMalloc pool");
        check(hipMalloc(&dd, sizeof(JpegDesc) * n), "hipMalloc descs");
        std::vector<std::vector<uint8_t>> rgb(n);
        try {
          check(hipMemset(pool, 0xCD, (size_t)off), "hipMemset");
          for (int i = 0; i < n; ++i)
            check(hipMemcpy(pool + coef_base[i], compact ? (const void*)payload[i].data() : (const void*)ps[i].coef.data(),
                            (size_t)jpeg_payload_bytes(ps[i].info), hipMemcpyHostToDevice), "H2D coef");
          check(hipMemcpy(dd, descs.data(), sizeof(JpegDesc) * n, hipMemcpyHostToDevice), "H2D desc");
          if (guard)
            for (int i = 0; i < n; ++i) {
              check(hipMemset(pool + rgb_off[i] - kGuard, kGuardByte, (size_t)kGuard), "guard");
              check(hipMemset(pool + rgb_off[i] + (int64_t)ps[i].info.width * ps[i].info.height * 3, kGuardByte, (size_t)kGuard), "guard");
            }
          if (ragged) {
            if (oriented) throw std::invalid_argument("jpeg_decode_device: ragged=True takes no EXIF-oriented upload");
            jpeg_reconstruct_ragged(dd, pool, n, rplan.idct_units, rplan.color_units, nullptr);
          } else {
            jpeg_reconstruct(dd, pool, n, (int)max_blocks, max_pix, nullptr, general);
          }
          check(hipGetLastError(), "jpeg_reconstruct launch");
          check(hipDeviceSynchronize(), "jpeg_reconstruct");
          for (int i = 0; i < n; ++i) {
            rgb[i].resize((size_t)ps[i].info.width * ps[i].info.height * 3);
            check(hipMemcpy(rgb[i].data(), pool + rgb_off[i], rgb[i].size(), hipMemcpyDeviceToHost), "D2H rgb");
            if (!guard) continue;
            uint8_t g[2 * kGuard];
            check(hipMemcpy(g, pool + rgb_off[i] - kGuard, (size_t)kGuard, hipMemcpyDeviceToHost), "D2H guard");
            check(hipMemcpy(g + kGuard, pool + rgb_off[i] + (int64_t)rgb[i].size(), (size_t)kGuard, hipMemcpyDeviceToHost), "D2H guard");
            for (int64_t k = 0; k < 2 * kGuard; ++k)
              if (g[k] != kGuardByte)
                throw std::runtime_error("jpeg_decode_device: the kernels wrote " + std::string(k < kGuard ? "before" : "past") +
                                         " the RGB region of upload " + std::to_string(i));
          }
        } catch (...) {
          hipFree(pool);
          hipFree(dd);
          throw;
        }
        hipFree(pool);
        hipFree(dd);
        for (int i = 0; i < n; ++i) {
          py::array_t<uint8_t> a({(py::ssize_t)ps[i].info.out_height, (py::ssize_t)ps[i].info.out_width, (py::ssize_t)3});
          std::memcpy(a.mutable_data(), rgb[i].data(), rgb[i].size());
          out.append(a);
        }
        return out;
      },
      py::arg("uploads"), py::arg("device") = 0, py::arg("guard") = false, py::arg("progressive") = py::none(),
      py::arg("compact") = false, py::arg("ragged") = false,
      "Entropy-decode on the host, reconstruct on the GPU (jpeg_idct.hip): list of HxWx3 uint8 in the EXIF\n"
      "orientation.  guard=True surrounds each RGB region with guard bytes and raises if the kernels touched them.\n"
      "progressive: accept SOF2 files (None = the process default).  compact=True ships the compact payload\n"
      "(jpeg_decode_compact) instead of dense blocks.  ragged=True launches the ragged kernels\n"
      "(jpeg_reconstruct_ragged; no EXIF-oriented upload) instead of the rectangular pair.");

  m.def(
      "jpeg_ragged_plan",
      [](std::vector<py::bytes> uploads) {
        const int n = (int)uploads.size();
        std::vector<JpegDesc> descs(n);
        int64_t max_blocks = 0, max_pix = 0;
        for (int i = 0; i < n; ++i) {
          const std::string s = uploads[i];
          JpegInfo in;
          std::string err;
          if (jpeg_parse((const uint8_t*)s.data(), s.size(), in, err, 0, -1) != JpegStatus::Ok)
            throw std::invalid_argument("upload " + std::to_string(i) + ": " + err);
          descs[i] = jpeg_device_desc(in, 0, 0, 0);
          max_blocks = std::max<int64_t>(max_blocks, descs[i].total_blocks);
          max_pix = std::max<int64_t>(max_pix, (int64_t)in.width * in.height);
        }
        const JpegRaggedPlan p = jpeg_ragged_plan(descs.data(), n);
        py::list fi, fc;
        for (int i = 0; i < n; ++i) {
          fi.append(descs[i].pad_[0]);
          fc.append(descs[i].pad_[1]);
        }
        py::dict out;
        out["idct_first"] = fi;
        out["color_first"] = fc;
        out["idct_units"] = p.idct_units;
        out["color_units"] = p.color_units;
        // the grids of jpeg_reconstruct over the same batch
        out["rect_idct_units"] = (int64_t)n * ((max_blocks + kJpegBlocksPerUnit - 1) / kJpegBlocksPerUnit);
        out["rect_color_units"] = n == 0 ? (int64_t)0 : (int64_t)n * std::max<int64_t>(1, (max_pix + 1023) / 1024);
        return out;
      },
      py::arg("uploads"),
      "Launch plan of the ragged reconstruction over a batch of uploads (host only; headers are parsed, nothing is\n"
      "decoded): dict(idct_first, color_first = each upload's first unit, idct_units, color_units = the ragged grids,\n"
      "rect_idct_units, rect_color_units = the workgroups the rectangular pair launches for the same batch).");
  // ---- crop encoder ----
  m.attr("SIZEOF_JPEG_ENC_DESC") = (int)sizeof(JpegEncDesc);

  m.def(
      "jpeg_enc_tables",
      [](int quality, bool zigzag) {
        const JpegEncTables t = jpeg_enc_tables(quality);
        py::array_t<uint16_t> a({(py::ssize_t)2, (py::ssize_t)64});
        for (int c = 0; c < 2; ++c)
          for (int k = 0; k < 64; ++k) a.mutable_at(c, k) = t.q[c][zigzag ? kZigzagToNatural[k] : k];
        return a;
      },
      py::arg("quality") = kCropJpegQuality, py::arg("zigzag") = false,
      "Annex K luminance / chrominance tables under IJG quality scaling: uint16[2][64], natural order (zigzag=True:\n"
      "the order of a DQT segment).");

  m.def(
      "jpeg_encode_coefs_host",
      [](U8Array crop, bool zigzag) {
        check_rgb(crop, "crop");
        const int h = (int)crop.shape(0), w = (int)crop.shape(1);
        py::array_t<int16_t> a({(py::ssize_t)jpeg_enc_blocks(w, h), (py::ssize_t)64});
        jpeg_encode_coefs_host<int32_t>(crop.data(), (int64_t)w * 3, w, h, jpeg_enc_tables(kCropJpegQuality),
                                        a.mutable_data(), zigzag);
        return a;
      },
      py::arg("crop"), py::arg("zigzag") = true,
      "Host oracle of the encoder kernel: int16[blocks][64] quantised coefficients of a 4:2:0 quality-95 JPEG, blocks\n"
      "in scan order MCU by MCU (Y00 Y01 Y10 Y11 Cb Cr), each in zigzag (default) or natural order.  Dummy slots of\n"
      "partial MCUs hold the transform of edge-clamped pixels; jpeg_write replaces them.");

  m.def(
      "jpeg_write",
      [](int w, int h, py::array_t<int16_t, py::array::c_style | py::array::forcecast> coefs, bool natural) {
        if (w < 1 || h < 1 || w > 65535 || h > 65535) throw std::invalid_argument("bad size");
        if (coefs.size() != jpeg_enc_blocks(w, h) * 64) throw std::invalid_argument("coefficient count does not match the size");
        return to_bytes(jpeg_write(w, h, coefs.data(), jpeg_enc_tables(kCropJpegQuality), natural));
      },
      py::arg("w"), py::arg("h"), py::arg("coefs"), py::arg("natural") = false,
      "Markers + Huffman scan of a w x h crop from its coefficient blocks (layout of jpeg_encode_coefs_host).");

  m.def(
      "jpeg_encode_host",
      [](U8Array crop) {
        check_rgb(crop, "crop");
        const int h = (int)crop.shape(0), w = (int)crop.shape(1);
        std::vector<uint8_t> out;
        {
          py::gil_scoped_release nogil;
          out = jpeg_encode_host(crop.data(), (int64_t)w * 3, w, h, jpeg_enc_tables(kCropJpegQuality));
        }
        return to_bytes(out);
      },
      py::arg("crop"), "Whole encode on the host: the bytes of PIL's quality-95 JPEG of an HxWx3 uint8 crop.");

  m.def(
      "jpeg_encode_device",
      [](U8Array frame, py::object boxes, int device, int64_t capacity_bytes, std::string entropy) -> py::object {
        // the dict outlives the lookup: an item accessor of a temporary dict would be read after the dict is gone
        const py::dict out = encode_device(frame, boxes, device, capacity_bytes, false, entropy);
        return out["blobs"];
      },
      py::arg("frame"), py::arg("boxes"), py::arg("device") = 0, py::arg("capacity_bytes") = 0,
      py::arg("entropy") = "host",
      "Upload an HxWx3 uint8 frame and encode the crops of `boxes` (x1, y1, x2, y2 floats, clipped like\n"
      "crop_bounds) on the GPU: list of bytes.  The encoder's device buffer (capacity_bytes, 0 = default) lies\n"
      "between guard bytes; raises if the kernel touched them.  entropy: \"host\" (C++ threads Huffman-code the\n"
      "coefficients) or \"gpu\" (kernels/jpeg_huff.hip; its buffers lie between guard bytes too).");
  m.def(
      "jpeg_encode_device_coefs",
      [](U8Array frame, py::object boxes, int device, int64_t capacity_bytes, std::string entropy, bool keep_coefs) {
        return encode_device(frame, boxes, device, capacity_bytes, keep_coefs, entropy);
      },
      py::arg("frame"), py::arg("boxes"), py::arg("device") = 0, py::arg("capacity_bytes") = 0,
      py::arg("entropy") = "host", py::arg("keep_coefs") = true,
      "jpeg_encode_device that also returns what the kernel wrote: dict(blobs, coefs = int16[blocks][64] per box in\n"
      "zigzag order (empty for an empty box), launches, d2h_bytes = bytes the encoder copied device to host,\n"
      "entropy_fallbacks = crops whose device-coded scan overflowed its reserve and the host coded).\n"
      "keep_coefs=False leaves `coefs` out, and with it the copy of the coefficients entropy=\"gpu\" does not need.");

  m.def(
      "jpeg_write_header",
      [](int w, int h) {
        if (w < 1 || h < 1 || w > 65535 || h > 65535) throw std::invalid_argument("bad size");
        return to_bytes(jpeg_write_header(w, h, jpeg_enc_tables(kCropJpegQuality)));
      },
      py::arg("w"), py::arg("h"), "What jpeg_write puts before the scan: SOI up to and including the SOS header.");
  m.def(
      "jpeg_block_bits",
      [](int w, int h, I16Array coefs, bool natural) {
        check_coefs(w, h, coefs, true);
        const std::vector<uint32_t> b = jpeg_block_bits_host(w, h, coefs.data(), natural);
        py::array_t<uint32_t> a((py::ssize_t)b.size());
        std::memcpy(a.mutable_data(), b.data(), b.size() * sizeof(uint32_t));
        return a;
      },
      py::arg("w"), py::arg("h"), py::arg("coefs"), py::arg("natural") = false,
      "Size phase of the entropy coder on the host (kernels/jpeg_huff_math.h block_bits): the bits jpeg_write emits\n"
      "for every block slot, uint32[blocks].");
  m.def(
      "jpeg_entropy_phased_host",
      [](int w, int h, I16Array coefs, bool natural) {
        check_coefs(w, h, coefs, true);
        return to_bytes(jpeg_entropy_phased_host(w, h, coefs.data(), jpeg_enc_tables(kCropJpegQuality), natural));
      },
      py::arg("w"), py::arg("h"), py::arg("coefs"), py::arg("natural") = false,
      "jpeg_write's bytes made on the CPU through the device entropy coder's phases (size, scan, emit, stuff) with\n"
      "the functions of kernels/jpeg_huff_math.h.  Coefficients must lie in +-1023.");
  m.def("jpeg_entropy_device", &entropy_device, py::arg("w"), py::arg("h"), py::arg("coefs"), py::arg("device") = 0,
        py::arg("reserve_per_block") = jpegh::kEntropyReserve, py::arg("natural") = false,
        "Upload one crop's coefficient blocks (jpeg_write's layout) and run only the entropy kernels\n"
        "(kernels/jpeg_huff.hip): dict(blob = the whole file, status = ok | overflow, bits = scan bits before padding,\n"
        "scan_bytes, fallbacks).  A scan that does not fit reserve_per_block bytes per block slot is coded by\n"
        "jpeg_write instead (status overflow, fallbacks 1).  Raises if a guard byte around the kernels' buffers was\n"
        "touched or a coefficient lies outside +-1023.");

  py::class_<CropJpegEncoder>(m, "CropJpegEncoder")
      .def(py::init([](int device, int64_t capacity_bytes, int threads, std::string entropy) {
             py::gil_scoped_release nogil;
             return new CropJpegEncoder(device, capacity_bytes, threads, kCropJpegQuality, entropy);
           }),
           py::arg("device") = 0, py::arg("capacity_bytes") = 0, py::arg("threads") = 2, py::arg("entropy") = "host")
      .def(
          "submit",
          [](CropJpegEncoder& e, uintptr_t frame_ptr, int frame_h, int frame_w, py::object boxes, py::function done,
             int64_t frame_bytes) {
            std::vector<CropBox> bx = to_boxes(boxes);
            std::shared_ptr<py::function> cb(new py::function(std::move(done)), [](py::function* fn) {
              py::gil_scoped_acquire gil;
              delete fn;
            });
            py::gil_scoped_release nogil;
            e.submit((const uint8_t*)frame_ptr, frame_h, frame_w, std::move(bx),
                     [cb](CropJpegEncoder::Blobs&& blobs, std::string&& err) {
                       py::gil_scoped_acquire gil;
                       try {
                         if (!err.empty()) {
                           (*cb)(py::none(), err);
                         } else {
                           py::list bl;
                           for (const auto& b : blobs) bl.append(to_bytes(b));
                           (*cb)(bl, std::string());
                         }
                       } catch (py::error_already_set& ex) {
                         ex.discard_as_unraisable("CropJpegEncoder done");
                       }
                     },
                     frame_bytes);
          },
          py::arg("frame_ptr"), py::arg("frame_h"), py::arg("frame_w"), py::arg("boxes"), py::arg("done"),
          py::arg("frame_bytes") = 0,
          "Encode the crops of `boxes` from the packed RGB frame at device address frame_ptr (frame_bytes: size of the\n"
          "buffer there, 0 = the frame's).  done(list of bytes, '') or done(None, error) is called from an encoder\n"
          "thread; the frame must stay valid until then.")
      .def_property_readonly("capacity", &CropJpegEncoder::capacity)
      .def_property_readonly("launches", &CropJpegEncoder::launches)
      .def_property_readonly("d2h_bytes", &CropJpegEncoder::d2h_bytes)
      .def_property_readonly("entropy_fallbacks", &CropJpegEncoder::entropy_fallbacks)
      .def_property_readonly("entropy", [](const CropJpegEncoder& e) { return e.entropy_gpu() ? "gpu" : "host"; })
      .def("stop", [](CropJpegEncoder& e) {
        py::gil_scoped_release nogil;
        e.stop();
      });
}

}  // namespace arena
