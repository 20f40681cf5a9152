// CropJpegEncoder: the device-owning part of the JPEG crop encoder (see jpeg_encode.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "../kernels/launch.h"
#include "jpeg_encode.h"

namespace arena {

namespace {

constexpr int kMaxCropsPerLaunch = 4096;  // bounds the descriptor buffer (and gridDim.y)

std::string hip_err(hipError_t e, const char* what) {
  return std::string("HIP error ") + hipGetErrorString(e) + " (" + what + ")";
}

}  // namespace

CropJpegEncoder::CropJpegEncoder(int device, int64_t capacity_bytes, int threads, int quality)
    : device_(device), tables_(jpeg_enc_tables(quality)) {
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
  for (int i = 1; i < std::max(1, threads); ++i) pool_.emplace_back([this] { work(); });
  driver_ = std::thread([this] { drive(); });
}

CropJpegEncoder::~CropJpegEncoder() {
  stop();
  if (d_alloc_) (void)hipFree(d_alloc_);
  if (h_coef_) (void)hipHostFree(h_coef_);
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
    if ((e = hipMemcpyAsync(h_coef_, d_coef_, (size_t)bytes, hipMemcpyDeviceToHost, s)) != hipSuccess)
      return hip_err(e, "D2H coefficients");
    // descs is read by the async copy until here
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_err(e, "jpeg_forward");
    ++launches_;
    const std::function<void(size_t)> code = [&](size_t k) {
      const JpegEncDesc& d = descs[k];
      const int16_t* cf = (const int16_t*)(h_coef_ + d.out_off);
      out[owner[first + k]] = jpeg_write(d.w, d.h, cf, tables_, true);
      if (keep_coefs) last_coefs[owner[first + k]].assign(cf, cf + (size_t)d.total_blocks * 64);
    };
    parallel_for(descs.size(), code);
    first = next;
  }
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
