// CropJpegEncoder: the device-owning part of the JPEG crop encoder (see jpeg_encode.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "../kernels/jpeg_huff_math.h"
#include "../kernels/launch.h"
#include "jpeg_encode.h"

namespace arena {

namespace {

constexpr int kMaxCropsPerLaunch = 4096;  // bounds the descriptor buffer (and gridDim.y)

std::string hip_err(hipError_t e, const char* what) {
  return std::string("HIP error ") + hipGetErrorString(e) + " (" + what + ")";
}

int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

constexpr size_t kHeaderSizeAt = 163;  // SOI + APP0 (20), two DQT (2 x 69), then FF C0 00 11 08 | hh hh ww ww

}  // namespace

// ---- JpegEntropyDevice ---------------------------------------------------------------------------------------------

JpegEntropyDevice::JpegEntropyDevice(int64_t max_slots, int64_t out_capacity, int max_crops)
    : max_slots_(std::max<int64_t>(max_slots, 6)), out_capacity_(align256(std::max<int64_t>(out_capacity, 256))),
      max_crops_(std::max(max_crops, 1)) {
  auto check = [](hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(hip_err(e, what));
  };
  // a crop has at least 6 slots and stuff_segments(slots) <= slots / 16 + 1 segments
  max_segs_ = max_slots_ / 16 + std::min<int64_t>(max_crops_, max_slots_ / 6) + 1;
  struct Part {
    const char* name;
    int64_t bytes, off;
  } parts[5] = {{"scan buffer", out_capacity_, 0},
                {"bit buffer", max_slots_ * jpegh::kBitBufBytesPerSlot, 0},
                {"slot sizes", align256(max_slots_ * 4), 0},
                {"segment counts", align256(max_segs_ * 4), 0},
                {"result records", align256((int64_t)max_crops_ * (int64_t)sizeof(JpegEntResult)), 0}};
  int64_t off = 0;
  guards_.emplace_back(off, "scan buffer (before)");
  off += kGuard;
  for (Part& p : parts) {
    p.off = off;
    off += p.bytes;
    guards_.emplace_back(off, p.name);
    off += kGuard;
  }
  alloc_bytes_ = off;
  check(hipMalloc((void**)&d_alloc_, (size_t)alloc_bytes_), "hipMalloc entropy buffers");
  check(hipMemset(d_alloc_, kGuardByte, (size_t)alloc_bytes_), "hipMemset entropy guards");
  d_out_ = d_alloc_ + parts[0].off;
  d_bitbuf_ = d_alloc_ + parts[1].off;
  d_slot_bits_ = (uint32_t*)(d_alloc_ + parts[2].off);
  d_seg_ff_ = (uint32_t*)(d_alloc_ + parts[3].off);
  d_res_ = (JpegEntResult*)(d_alloc_ + parts[4].off);
  check(hipMalloc((void**)&d_desc_, sizeof(JpegEntDesc) * (size_t)max_crops_), "hipMalloc entropy descriptors");
  const size_t tb = sizeof(uint32_t) * 4 * jpegh::kCodeTableEntries;
  check(hipMalloc((void**)&d_tables_, tb), "hipMalloc code tables");
  check(hipMemcpy(d_tables_, jpeg_enc_code_tables(), tb, hipMemcpyHostToDevice), "H2D code tables");
}

JpegEntropyDevice::~JpegEntropyDevice() {
  if (d_alloc_) (void)hipFree(d_alloc_);
  if (d_desc_) (void)hipFree(d_desc_);
  if (d_tables_) (void)hipFree(d_tables_);
}

std::string JpegEntropyDevice::plan(const std::vector<JpegEncDesc>& enc, int reserve_per_block,
                                    std::vector<JpegEntDesc>& out) const {
  out.clear();
  if (enc.empty() || (int64_t)enc.size() > max_crops_) return "entropy coder: crop count";
  if (reserve_per_block < 1 || reserve_per_block > 4096) return "entropy coder: reserve per block";
  int64_t slots = 0, segs = 0, bytes = 0;
  for (const JpegEncDesc& e : enc) {
    if (e.w < 1 || e.h < 1 || e.mcux != (e.w + 15) / 16 || e.total_blocks != jpeg_enc_blocks(e.w, e.h) ||
        e.out_off < 0 || e.out_off % 16 != 0)
      return "entropy coder: inconsistent descriptor";
    JpegEntDesc d;
    d.coef_off = e.out_off;
    d.out_off = bytes;
    d.w = e.w;
    d.h = e.h;
    d.mcux = e.mcux;
    d.total_blocks = e.total_blocks;
    d.slot_base = (int32_t)slots;
    d.seg_base = (int32_t)segs;
    const int64_t reserve = align256((int64_t)e.total_blocks * reserve_per_block);
    d.reserve = (int32_t)reserve;
    d.pad_ = 0;
    slots += e.total_blocks;
    segs += jpegh::stuff_segments(e.total_blocks);
    bytes += reserve;
    if (slots > max_slots_ || segs > max_segs_ || bytes > out_capacity_) return "entropy coder: the crops do not fit its buffers";
    out.push_back(d);
  }
  return "";
}

std::string JpegEntropyDevice::launch(const std::vector<JpegEntDesc>& descs, const uint8_t* d_coef, bool natural,
                                      void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (descs.empty() || (int64_t)descs.size() > max_crops_) return "entropy coder: crop count";
  int max_blocks = 0;
  const JpegEntDesc& last = descs.back();
  for (const JpegEntDesc& d : descs) max_blocks = std::max(max_blocks, d.total_blocks);
  const int64_t slots = (int64_t)last.slot_base + last.total_blocks;
  if (slots > max_slots_) return "entropy coder: the crops do not fit its buffers";
  hipError_t e = hipMemcpyAsync(d_desc_, descs.data(), sizeof(JpegEntDesc) * descs.size(), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_err(e, "H2D entropy descriptors");
  // the emit kernel ORs the words two workgroups share into zeroed memory
  if ((e = hipMemsetAsync(d_bitbuf_, 0, (size_t)(slots * jpegh::kBitBufBytesPerSlot), s)) != hipSuccess)
    return hip_err(e, "hipMemsetAsync bit buffer");
  JpegEntBuffers b;
  b.coef = d_coef;
  b.tables = d_tables_;
  b.slot_bits = d_slot_bits_;
  b.bitbuf = d_bitbuf_;
  b.seg_ff = d_seg_ff_;
  b.out = d_out_;
  b.res = d_res_;
  jpeg_entropy((const JpegEntDesc*)d_desc_, b, (int)descs.size(), max_blocks, natural, s);
  if ((e = hipGetLastError()) != hipSuccess) return hip_err(e, "jpeg_entropy launch");
  return "";
}

std::string JpegEntropyDevice::check_guards() const {
  uint8_t g[kGuard];
  for (const auto& gd : guards_) {
    const hipError_t e = hipMemcpy(g, d_alloc_ + gd.first, (size_t)kGuard, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_err(e, "D2H entropy guards");
    for (int64_t k = 0; k < kGuard; ++k)
      if (g[k] != kGuardByte) return std::string("the entropy kernels wrote outside the ") + gd.second;
  }
  return "";
}

// ---- CropJpegEncoder -----------------------------------------------------------------------------------------------

CropJpegEncoder::CropJpegEncoder(int device, int64_t capacity_bytes, int threads, int quality, const std::string& entropy)
    : device_(device), tables_(jpeg_enc_tables(quality)) {
  if (entropy != "host" && entropy != "gpu") throw std::invalid_argument("CropJpegEncoder: entropy is 'host' or 'gpu'");
  // a crop is no larger than a frame slot (640 x 640 x 3 bytes), so one crop always fits the default
  capacity_ = capacity_bytes > 0 ? (capacity_bytes + 255) / 256 * 256 : jpeg_enc_coef_bytes(640, 640);
  const uint8_t zero[3] = {0, 0, 0};
  black_ = jpeg_encode_host(zero, 3, 1, 1, tables_);
  auto check = [](hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(hip_err(e, what));
  };
  check(hipSetDevice(device_), "hipSetDevice");
  hipStream_t s = nullptr;
  check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
  stream_ = s;
  // guard bytes right before and right after the coefficient buffer, checked by check_guards()
  check(hipMalloc((void**)&d_alloc_, (size_t)(capacity_ + 2 * kGuard)), "hipMalloc coefficients");
  check(hipMemset(d_alloc_, kGuardByte, (size_t)(capacity_ + 2 * kGuard)), "hipMemset guards");
  d_coef_ = d_alloc_ + kGuard;
  check(hipHostMalloc((void**)&h_coef_, (size_t)capacity_, hipHostMallocPortable), "hipHostMalloc coefficients");
  check(hipMalloc((void**)&d_desc_, sizeof(JpegEncDesc) * kMaxCropsPerLaunch), "hipMalloc descriptors");
  check(hipMalloc((void**)&d_qt_, sizeof(tables_.q)), "hipMalloc tables");
  check(hipMemcpy(d_qt_, tables_.q, sizeof(tables_.q), hipMemcpyHostToDevice), "H2D tables");
  if (entropy == "gpu") {
    // every crop reserves what its coefficients take (kEntropyReserve = 128 bytes per slot), so what fits the
    // coefficient buffer fits the scan buffer
    static_assert(jpegh::kEntropyReserve == 128, "the scan reserve equals the coefficient bytes");
    ent_.reset(new JpegEntropyDevice(capacity_ / 128, capacity_, kMaxCropsPerLaunch));
    const size_t recs = sizeof(JpegEntResult) * kMaxCropsPerLaunch;
    check(hipHostMalloc((void**)&h_scan_, (size_t)capacity_ + recs, hipHostMallocPortable), "hipHostMalloc scans");
    h_res_ = (JpegEntResult*)(h_scan_ + capacity_);
    header_ = jpeg_write_header(1, 1, tables_);
    const uint8_t sof[9] = {0xFF, 0xC0, 0, 17, 8, 0, 1, 0, 1};
    if (header_.size() < kHeaderSizeAt + 4 || std::memcmp(&header_[kHeaderSizeAt - 5], sof, 9) != 0)
      throw std::runtime_error("CropJpegEncoder: unexpected header layout");
  }
  for (int i = 1; i < std::max(1, threads); ++i) pool_.emplace_back([this] { work(); });
  driver_ = std::thread([this] { drive(); });
}

CropJpegEncoder::~CropJpegEncoder() {
  stop();
  if (d_alloc_) (void)hipFree(d_alloc_);
  if (h_coef_) (void)hipHostFree(h_coef_);
  if (h_scan_) (void)hipHostFree(h_scan_);
  ent_.reset();
  if (d_desc_) (void)hipFree(d_desc_);
  if (d_qt_) (void)hipFree(d_qt_);
  if (stream_) (void)hipStreamDestroy((hipStream_t)stream_);
}

std::string CropJpegEncoder::check_guards() {
  uint8_t g[2 * kGuard];
  hipError_t e = hipMemcpy(g, d_alloc_, (size_t)kGuard, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(g + kGuard, d_coef_ + capacity_, (size_t)kGuard, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_err(e, "D2H guards");
  for (int64_t k = 0; k < 2 * kGuard; ++k)
    if (g[k] != kGuardByte)
      return std::string("the kernel wrote ") + (k < kGuard ? "before" : "past") + " the coefficient buffer";
  if (ent_) return ent_->check_guards();
  return "";
}

void CropJpegEncoder::stop() {
  {
    std::lock_guard<std::mutex> lk(mu_);
    if (stop_) return;
    stop_ = true;
  }
  cv_.notify_all();
  if (driver_.joinable()) driver_.join();  // finishes the queued jobs first
  {
    std::lock_guard<std::mutex> lk(pmu_);
    pstop_ = true;
  }
  pcv_.notify_all();
  for (auto& t : pool_) t.join();
  pool_.clear();
}

void CropJpegEncoder::submit(const uint8_t* frame_ptr, int frame_h, int frame_w, std::vector<CropBox> boxes, Done done,
                             int64_t frame_bytes) {
  Job j{frame_ptr, frame_h, frame_w, frame_bytes > 0 ? frame_bytes : (int64_t)frame_h * frame_w * 3, std::move(boxes),
        std::move(done)};
  {
    std::lock_guard<std::mutex> lk(mu_);
    if (!stop_) {
      jobs_.push_back(std::move(j));
      cv_.notify_one();
      return;
    }
  }
  j.done(Blobs(), "the crop encoder is stopped");
}

void CropJpegEncoder::drive() {
  (void)hipSetDevice(device_);
  for (;;) {
    Job j;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [this] { return stop_ || !jobs_.empty(); });
      if (jobs_.empty()) return;
      j = std::move(jobs_.front());
      jobs_.pop_front();
    }
    Blobs out;
    std::string err;
    try {
      err = run(j, out);
    } catch (const std::exception& e) {
      err = e.what();
    }
    if (!err.empty()) out.clear();
    j.done(std::move(out), std::move(err));
  }
}

std::string CropJpegEncoder::run(Job& j, Blobs& out) {
  const size_t n = j.boxes.size();
  out.assign(n, {});
  if (keep_coefs) last_coefs.assign(n, {});
  if (n == 0) return "";
  if (j.frame == nullptr) return "no frame";
  // windows of the non-empty boxes; an empty box is the 1x1 black crop extract_crop gives
  std::vector<CropWindow> win;
  std::vector<size_t> owner;
  for (size_t i = 0; i < n; ++i) {
    CropWindow c;
    if (jpeg_crop_window(j.boxes[i], j.h, j.w, c.x0, c.y0, c.w, c.h)) {
      win.push_back(c);
      owner.push_back(i);
    } else {
      out[i] = black_;
    }
  }
  hipStream_t s = (hipStream_t)stream_;
  std::vector<JpegEncDesc> descs;
  for (size_t first = 0; first < win.size();) {
    int64_t bytes = 0;
    int max_blocks = 0;
    const size_t next = jpeg_enc_plan_chunk(win, first, j.w, capacity_, kMaxCropsPerLaunch, descs, bytes, max_blocks);
    const std::string bad = jpeg_enc_validate(descs, j.h, j.w, j.frame_bytes, capacity_);
    if (!bad.empty()) return "crop encoder: " + bad;
    hipError_t e = hipMemcpyAsync(d_desc_, descs.data(), sizeof(JpegEncDesc) * descs.size(), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_err(e, "H2D descriptors");
    jpeg_forward((const JpegEncDesc*)d_desc_, j.frame, d_coef_, d_qt_, (int)descs.size(), max_blocks, s);
    if ((e = hipGetLastError()) != hipSuccess) return hip_err(e, "jpeg_forward launch");
    const std::string err = ent_ ? finish_gpu(descs, bytes, first, owner, out) : finish_host(descs, bytes, first, owner, out);
    if (!err.empty()) return err;
    first = next;
  }
  return "";
}

// entropy = "host": all coefficients come back, the pool Huffman-codes them.
std::string CropJpegEncoder::finish_host(const std::vector<JpegEncDesc>& descs, int64_t bytes, size_t first,
                                         const std::vector<size_t>& owner, Blobs& out) {
  hipStream_t s = (hipStream_t)stream_;
  hipError_t e;
  if ((e = hipMemcpyAsync(h_coef_, d_coef_, (size_t)bytes, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_err(e, "D2H coefficients");
  // descs is read by the async copy until here
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_err(e, "jpeg_forward");
  ++launches_;
  d2h_bytes_ += bytes;
  const std::function<void(size_t)> code = [&](size_t k) {
    const JpegEncDesc& d = descs[k];
    const int16_t* cf = (const int16_t*)(h_coef_ + d.out_off);
    out[owner[first + k]] = jpeg_write(d.w, d.h, cf, tables_, true);
    if (keep_coefs) last_coefs[owner[first + k]].assign(cf, cf + (size_t)d.total_blocks * 64);
  };
  parallel_for(descs.size(), code);
  return "";
}

// entropy = "gpu": the records come back, then each scan at its exact length; overflowed crops take the host path.
std::string CropJpegEncoder::finish_gpu(const std::vector<JpegEncDesc>& descs, int64_t bytes, size_t first,
                                        const std::vector<size_t>& owner, Blobs& out) {
  hipStream_t s = (hipStream_t)stream_;
  hipError_t e;
  const size_t n = descs.size();
  std::string err = ent_->plan(descs, jpegh::kEntropyReserve, ent_descs_);
  if (!err.empty()) return "crop encoder: " + err;
  if (!(err = ent_->launch(ent_descs_, d_coef_, true, stream_)).empty()) return err;
  if ((e = hipMemcpyAsync(h_res_, ent_->d_res(), sizeof(JpegEntResult) * n, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return hip_err(e, "D2H entropy records");
  d2h_bytes_ += (int64_t)(sizeof(JpegEntResult) * n);
  if (keep_coefs) {
    if ((e = hipMemcpyAsync(h_coef_, d_coef_, (size_t)bytes, hipMemcpyDeviceToHost, s)) != hipSuccess)
      return hip_err(e, "D2H coefficients");
    d2h_bytes_ += bytes;
  }
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_err(e, "jpeg_entropy");
  ++launches_;
  std::vector<size_t> fallback;
  for (size_t k = 0; k < n; ++k) {
    const JpegEntResult& r = h_res_[k];
    const JpegEntDesc& d = ent_descs_[k];
    if (r.status == jpegh::kEntropyOk) {
      if (r.scan_bytes < 1 || r.scan_bytes > (uint32_t)d.reserve) return "crop encoder: inconsistent entropy record";
      if ((e = hipMemcpyAsync(h_scan_ + d.out_off, ent_->d_out() + d.out_off, r.scan_bytes, hipMemcpyDeviceToHost, s)) !=
          hipSuccess)
        return hip_err(e, "D2H scan");
      d2h_bytes_ += r.scan_bytes;
    } else if (r.status == jpegh::kEntropyOverflow) {
      fallback.push_back(k);
      if (keep_coefs) continue;  // they are here already
      const size_t cb = (size_t)d.total_blocks * 128;
      if ((e = hipMemcpyAsync(h_coef_ + d.coef_off, d_coef_ + d.coef_off, cb, hipMemcpyDeviceToHost, s)) != hipSuccess)
        return hip_err(e, "D2H coefficients");
      d2h_bytes_ += (int64_t)cb;
    } else {
      return "crop encoder: inconsistent entropy record";
    }
  }
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_err(e, "D2H scans");
  entropy_fallbacks_ += (int64_t)fallback.size();
  for (size_t k = 0; k < n; ++k) {
    const JpegEntDesc& d = ent_descs_[k];
    const int16_t* cf = (const int16_t*)(h_coef_ + d.coef_off);
    if (keep_coefs) last_coefs[owner[first + k]].assign(cf, cf + (size_t)d.total_blocks * 64);
    if (h_res_[k].status != jpegh::kEntropyOk) continue;
    std::vector<uint8_t>& o = out[owner[first + k]];
    const size_t len = h_res_[k].scan_bytes;
    o.resize(header_.size() + len + 2);
    std::memcpy(o.data(), header_.data(), header_.size());
    o[kHeaderSizeAt] = (uint8_t)(d.h >> 8);
    o[kHeaderSizeAt + 1] = (uint8_t)d.h;
    o[kHeaderSizeAt + 2] = (uint8_t)(d.w >> 8);
    o[kHeaderSizeAt + 3] = (uint8_t)d.w;
    std::memcpy(o.data() + header_.size(), h_scan_ + d.out_off, len);
    o[header_.size() + len] = 0xFF;
    o[header_.size() + len + 1] = 0xD9;
  }
  const std::function<void(size_t)> code = [&](size_t i) {
    const JpegEntDesc& d = ent_descs_[fallback[i]];
    out[owner[first + fallback[i]]] = jpeg_write(d.w, d.h, (const int16_t*)(h_coef_ + d.coef_off), tables_, true);
  };
  parallel_for(fallback.size(), code);
  return "";
}

// The driver and the pool threads take indices from a shared counter until none is left.
void CropJpegEncoder::parallel_for(size_t n, const std::function<void(size_t)>& fn) {
  if (pool_.empty() || n < 2) {
    for (size_t i = 0; i < n; ++i) fn(i);
    return;
  }
  {
    std::lock_guard<std::mutex> lk(pmu_);
    pfn_ = &fn;
    pn_ = n;
    pnext_ = 0;
    pleft_ = n;
  }
  pcv_.notify_all();
  for (;;) {
    size_t i;
    {
      std::lock_guard<std::mutex> lk(pmu_);
      if (pnext_ >= pn_) break;
      i = pnext_++;
    }
    fn(i);
    std::lock_guard<std::mutex> lk(pmu_);
    --pleft_;
  }
  std::unique_lock<std::mutex> lk(pmu_);
  pdone_.wait(lk, [this] { return pleft_ == 0; });
  pfn_ = nullptr;
  pn_ = 0;
}

void CropJpegEncoder::work() {
  std::unique_lock<std::mutex> lk(pmu_);
  for (;;) {
    pcv_.wait(lk, [this] { return pstop_ || (pfn_ != nullptr && pnext_ < pn_); });
    if (pstop_) return;
    while (pfn_ != nullptr && pnext_ < pn_) {
      const size_t i = pnext_++;
      const std::function<void(size_t)>* fn = pfn_;
      lk.unlock();
      (*fn)(i);
      lk.lock();
      if (--pleft_ == 0) pdone_.notify_all();
    }
  }
}

}  // namespace arena
