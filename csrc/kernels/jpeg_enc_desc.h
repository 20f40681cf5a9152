// Device-side description of one crop the GPU half of the JPEG encoder transforms (csrc/kernels/jpeg_fdct.hip);
// the host half (csrc/runtime/jpeg_encode.h) builds and validates it.
#pragma once
#include <cstdint>

namespace arena {

struct JpegEncDesc {
  int64_t src_off;   // bytes from the frame's base to the crop's top-left pixel (packed RGB)
  int64_t out_off;   // bytes from the coefficient buffer's base to this crop's blocks (16-byte aligned)
  int32_t pitch;     // bytes per frame row
  int32_t w, h;      // crop size in pixels, both >= 1; the window lies inside the frame
  int32_t mcux;      // 16x16 MCUs per row
  int32_t total_blocks;  // mcux * mcuy * 6
  int32_t pad_;
};
static_assert(sizeof(JpegEncDesc) == 40, "JpegEncDesc layout is shared with the kernel");

// One crop of the device entropy coder (csrc/kernels/jpeg_huff.hip): where its coefficient blocks lie and which
// ranges of the coder's buffers are its own.  JpegEntropyDevice::plan (csrc/runtime/jpeg_encode.h) builds these.
struct JpegEntDesc {
  int64_t coef_off;      // bytes from the coefficient buffer's base to this crop's blocks (16-byte aligned)
  int64_t out_off;       // bytes from the scan buffer's base to this crop's reserved range
  int32_t w, h;          // crop size in pixels
  int32_t mcux;          // 16x16 MCUs per row
  int32_t total_blocks;  // block slots: mcux * mcuy * 6
  int32_t slot_base;     // first entry of the per-slot size array; the crop's bits start at byte slot_base * 256
  int32_t seg_base;      // first entry of the per-segment 0xFF counts
  int32_t reserve;       // bytes of the scan buffer reserved for this crop
  int32_t pad_;
};
static_assert(sizeof(JpegEntDesc) == 48, "JpegEntDesc layout is shared with the kernels");

// What the entropy coder reports per crop.
struct JpegEntResult {
  uint32_t scan_bytes;  // length of the stuffed scan (written only when it fits the reserve)
  uint32_t total_bits;  // bits of the scan before padding and stuffing
  uint32_t status;      // jpegh::kEntropyOk | kEntropyOverflow
  uint32_t raw_bytes;   // (total_bits + 7) / 8
};

constexpr int kJpegEncBlocksPerMcu = 6;  // 4:2:0: Y00 Y01 Y10 Y11 Cb Cr

// Blocks / bytes of a w x h crop's coefficients (int16[blocks][64]).
inline int64_t jpeg_enc_blocks(int w, int h) { return (int64_t)((w + 15) / 16) * ((h + 15) / 16) * kJpegEncBlocksPerMcu; }
inline int64_t jpeg_enc_coef_bytes(int w, int h) { return jpeg_enc_blocks(w, h) * 128; }

}  // namespace arena
