// Host half of the split JPEG crop encoder, the mirror image of jpeg_decode.h: the GPU gathers each crop from a
// device-resident frame and does colour conversion, chroma downsampling, forward DCT and quantisation
// (csrc/kernels/jpeg_fdct.hip); a host thread does the bit-serial Huffman pass and writes the markers, or, in the
// encoder's entropy = "gpu" mode, the GPU codes the scan too (csrc/kernels/jpeg_huff.hip) and the host adds markers.
//
// The reference's arm B sends each crop as a PIL JPEG at quality 95 (architectures/microservices/detection/app/
// grpc_client.py:99-103).  The files written here are byte-identical to PIL's (libjpeg-turbo defaults: baseline,
// 4:2:0, the Annex K Huffman tables, JFIF 1.01 header), so the classification service and the wire contract see
// no difference.  Scope: quality >= 50 tables, 4:2:0, standard Huffman tables.
#pragma once
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../kernels/jpeg_enc_desc.h"

namespace arena {

constexpr int kCropJpegQuality = 95;  // server/crop_codec.py JPEG_QUALITY

struct JpegEncTables {
  uint16_t q[2][64];  // luminance, chrominance; natural order
};

// Annex K tables under IJG quality scaling (jcparam.c): scale = 200 - 2q for q >= 50 (5000 / q below), each entry
// (base * scale + 50) / 100 clamped to 1..255.
JpegEncTables jpeg_enc_tables(int quality);

// Blocks of a w x h crop: jpeg_enc_blocks(w, h) (jpeg_enc_desc.h), in scan order MCU by MCU, Y00 Y01 Y10 Y11 Cb Cr.

// The bit-exact host reference of the kernel: quantised int16 coefficients of a packed RGB crop (row pitch in
// bytes), jpeg_enc_blocks(w, h) * 64 of them.  zigzag = true writes each block in zigzag order (what jpeg_write
// reads by default), false in natural order (the kernel's layout).  Every block slot is computed from
// edge-clamped pixels, the dummy slots of partial MCUs too; jpeg_write replaces those.  Acc is the DCT accumulator
// type: int32_t is what the GPU runs, int64_t is libjpeg's JLONG.
template <typename Acc = int32_t>
void jpeg_encode_coefs_host(const uint8_t* rgb, int64_t pitch, int w, int h, const JpegEncTables& t, int16_t* out,
                            bool zigzag = true);

// Markers + Huffman-coded scan of a w x h crop from its coefficient blocks (layout as above; `natural` = the
// blocks are in natural order).  A block slot beyond the component's real ceil(cw / 8) x ceil(ch / 8) grid is coded
// as libjpeg's compress_data codes dummy blocks: all-zero AC, DC = the DC of the block coded just before it in the
// same MCU.
std::vector<uint8_t> jpeg_write(int w, int h, const int16_t* coefs, const JpegEncTables& t, bool natural = false);

// jpeg_write in its parts: everything up to and including the SOS header; jpeg_write appends the scan and EOI.
std::vector<uint8_t> jpeg_write_header(int w, int h, const JpegEncTables& t);
// The four Huffman code tables jpeg_write codes with, symbol -> code | length << 16: uint32[4][256] in the DHT order
// DC0, AC0, DC1, AC1 (the layout of kernels/jpeg_huff_math.h; the device entropy coder uploads them).
const uint32_t* jpeg_enc_code_tables();
// The bytes of jpeg_write, made the way the device entropy coder (kernels/jpeg_huff.hip) makes them, with the
// functions of kernels/jpeg_huff_math.h: size every slot on its own, prefix-sum the sizes, emit every slot at its bit
// offset into a zeroed buffer, pad, count the 0xFF bytes per segment, prefix-sum, place every byte.  Coefficients
// must lie in +-1023.  jpeg_block_bits_host: the size phase alone, bits per block slot.
std::vector<uint8_t> jpeg_entropy_phased_host(int w, int h, const int16_t* coefs, const JpegEncTables& t,
                                              bool natural = false);
std::vector<uint32_t> jpeg_block_bits_host(int w, int h, const int16_t* coefs, bool natural = false);

// Whole encode on the host.
std::vector<uint8_t> jpeg_encode_host(const uint8_t* rgb, int64_t pitch, int w, int h, const JpegEncTables& t);

// Integer crop window of a float box, the rule of processing/mobilenet_preprocess.crop_bounds: truncate towards
// zero, clip to the frame.  Returns false for an empty window (the caller sends a 1x1 black crop, as extract_crop).
struct CropBox {
  double x1, y1, x2, y2;
};
bool jpeg_crop_window(const CropBox& b, int frame_h, int frame_w, int& x0, int& y0, int& w, int& h);

// One launch's worth of crops: descriptors whose coefficient ranges are packed (256-byte aligned) from offset 0.
// plan_chunk takes windows [first, n) while they fit `capacity` bytes and `max_crops`; at least one (the caller
// guarantees a single crop fits).  Returns the index after the last one taken; `bytes` is the buffer range used.
struct CropWindow {
  int x0, y0, w, h;
};
size_t jpeg_enc_plan_chunk(const std::vector<CropWindow>& win, size_t first, int frame_w, int64_t capacity,
                           int max_crops, std::vector<JpegEncDesc>& descs, int64_t& bytes, int& max_blocks);
// Every descriptor's source window inside a frame of frame_h x frame_w pixels held by a buffer of frame_bytes,
// every output range inside `capacity` bytes and 16-byte aligned: "" or what is wrong.
std::string jpeg_enc_validate(const std::vector<JpegEncDesc>& descs, int frame_h, int frame_w, int64_t frame_bytes,
                              int64_t capacity);

// Device buffers of the entropy coder (kernels/jpeg_huff.hip) and its launch.  One allocation holds, each between
// kGuard bytes of kGuardByte: the scan buffer, the bit buffer (256 bytes per block slot), the per-slot sizes, the
// per-segment 0xFF counts and the result records.  plan() lays the crops of one launch out in them, launch() uploads
// the descriptors, zeroes the bit buffer and queues the five kernels on the caller's stream; nothing synchronises.
class JpegEntropyDevice {
 public:
  static constexpr int64_t kGuard = 256;
  static constexpr int kGuardByte = 0xA5;
  // max_slots: block slots of one launch; out_capacity: bytes of the scan buffer; max_crops: crops of one launch
  JpegEntropyDevice(int64_t max_slots, int64_t out_capacity, int max_crops);
  ~JpegEntropyDevice();
  JpegEntropyDevice(const JpegEntropyDevice&) = delete;
  JpegEntropyDevice& operator=(const JpegEntropyDevice&) = delete;

  // Descriptors for crops whose coefficient blocks lie at enc[i].out_off of the coefficient buffer, each reserving
  // reserve_per_block bytes per block slot (rounded up to 256) of the scan buffer: "" or why they do not fit.
  std::string plan(const std::vector<JpegEncDesc>& enc, int reserve_per_block, std::vector<JpegEntDesc>& out) const;
  // "" or the HIP error.  `descs` must stay alive until the stream has passed the upload.
  std::string launch(const std::vector<JpegEntDesc>& descs, const uint8_t* d_coef, bool natural, void* stream);
  const uint8_t* d_out() const { return d_out_; }
  const JpegEntResult* d_res() const { return d_res_; }
  std::string check_guards() const;  // "" while every guard is intact

 private:
  int64_t max_slots_, out_capacity_, max_segs_;
  int max_crops_;
  uint8_t* d_alloc_ = nullptr;
  int64_t alloc_bytes_ = 0;
  std::vector<std::pair<int64_t, const char*>> guards_;  // offsets of the guard ranges, the buffer each follows
  uint8_t* d_out_ = nullptr;
  uint8_t* d_bitbuf_ = nullptr;
  uint32_t* d_slot_bits_ = nullptr;
  uint32_t* d_seg_ff_ = nullptr;
  JpegEntResult* d_res_ = nullptr;
  uint8_t* d_desc_ = nullptr;
  uint32_t* d_tables_ = nullptr;
};

// Encoder of the crops of device-resident frames.  Owns one stream, a device coefficient buffer, a pinned copy of
// it and a small pool of Huffman threads.  submit() queues a job; a driver thread launches the kernel over as many
// crops as fit the buffer, copies the coefficients back, has the pool Huffman-code them and repeats for the rest,
// then calls done(blobs, error) from that thread: one byte string per box and "" on success, no blobs and the
// message on failure (a HIP error is reported in-band and never retried).  The frame must stay valid until done.
//
// entropy = "gpu": the Huffman pass runs on the device too (JpegEntropyDevice).  Per launch the encoder copies back
// the result records, then each crop's scan at its exact length, and assembles header + scan + EOI; only a crop
// whose scan overflowed its reserve (kEntropyReserve bytes per block slot) has its coefficients copied and coded by
// jpeg_write as in "host" mode.  Same bytes either way.
class CropJpegEncoder {
 public:
  using Blobs = std::vector<std::vector<uint8_t>>;
  using Done = std::function<void(Blobs&&, std::string&&)>;

  // capacity_bytes <= 0: room for one 640 x 640 frame slot's worth of crops.
  CropJpegEncoder(int device, int64_t capacity_bytes, int threads, int quality = kCropJpegQuality,
                  const std::string& entropy = "host");
  ~CropJpegEncoder();
  CropJpegEncoder(const CropJpegEncoder&) = delete;
  CropJpegEncoder& operator=(const CropJpegEncoder&) = delete;

  // frame_bytes: size of the buffer at frame_ptr (0: exactly frame_h * frame_w * 3).
  void submit(const uint8_t* frame_ptr, int frame_h, int frame_w, std::vector<CropBox> boxes, Done done,
              int64_t frame_bytes = 0);
  void stop();
  int64_t capacity() const { return capacity_; }
  int64_t launches() const { return launches_; }
  int64_t d2h_bytes() const { return d2h_bytes_; }                  // bytes copied device to host by the jobs so far
  int64_t entropy_fallbacks() const { return entropy_fallbacks_; }  // crops whose scan overflowed and the host coded
  bool entropy_gpu() const { return ent_ != nullptr; }
  // The device coefficient buffer lies between kGuard bytes of kGuardByte; "" while they are intact (call it with
  // no job in flight).
  static constexpr int64_t kGuard = 256;
  static constexpr int kGuardByte = 0xA5;
  std::string check_guards();
  // device coefficients of the last job, crop after crop in natural order (tests; set keep_coefs before submit)
  bool keep_coefs = false;
  std::vector<std::vector<int16_t>> last_coefs;

 private:
  struct Job {
    const uint8_t* frame;
    int h, w;
    int64_t frame_bytes;
    std::vector<CropBox> boxes;
    Done done;
  };
  void drive();
  void work();
  std::string run(Job& j, Blobs& out);
  std::string finish_host(const std::vector<JpegEncDesc>& descs, int64_t bytes, size_t first,
                          const std::vector<size_t>& owner, Blobs& out);
  std::string finish_gpu(const std::vector<JpegEncDesc>& descs, int64_t bytes, size_t first,
                         const std::vector<size_t>& owner, Blobs& out);
  void parallel_for(size_t n, const std::function<void(size_t)>& fn);

  int device_;
  int64_t capacity_;
  JpegEncTables tables_;
  std::vector<uint8_t> black_;  // the 1x1 black crop of an empty box
  void* stream_ = nullptr;
  uint8_t* d_alloc_ = nullptr;  // guard | coefficients | guard
  uint8_t* d_coef_ = nullptr;
  uint8_t* h_coef_ = nullptr;
  uint8_t* d_desc_ = nullptr;
  uint16_t* d_qt_ = nullptr;
  int64_t launches_ = 0, d2h_bytes_ = 0, entropy_fallbacks_ = 0;
  // entropy = "gpu"
  std::unique_ptr<JpegEntropyDevice> ent_;
  std::vector<JpegEntDesc> ent_descs_;
  std::vector<uint8_t> header_;  // jpeg_write_header of a 1x1 crop: only the SOF0 size differs between crops
  uint8_t* h_scan_ = nullptr;    // pinned: capacity_ bytes of scans, then the result records
  JpegEntResult* h_res_ = nullptr;

  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<Job> jobs_;
  bool stop_ = false;
  std::thread driver_;

  // Huffman pool: the driver publishes (n, fn) and takes part itself
  std::mutex pmu_;
  std::condition_variable pcv_, pdone_;
  const std::function<void(size_t)>* pfn_ = nullptr;
  size_t pn_ = 0, pnext_ = 0, pleft_ = 0;
  bool pstop_ = false;
  std::vector<std::thread> pool_;
};

}  // namespace arena
