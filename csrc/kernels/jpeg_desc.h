// Device-side description of one entropy-decoded baseline JPEG (the split decoder's hand-off from the host
// Huffman decoder, csrc/runtime/jpeg_decode.h, to the reconstruction kernels, csrc/kernels/jpeg_idct.hip).
// Offsets are bytes from the base of a staging slot's image pool (Executor d_in), so one descriptor array
// describes a whole batch.
#pragma once
#include <cstdint>

namespace arena {

constexpr int kJpegMaxComp = 3;

// Chroma layouts the split decoder reconstructs on the device; anything else goes to the PIL fallback.  The ratio
// luma : chroma sampling factors decides: (1,1), (2,1) and (2,2) are the first three colour layouts, (1,2) is
// JPEG_440 (libjpeg's h1v2 fancy upsampling: 4:4:0, what a losslessly rotated 4:2:2 file becomes), and every other
// integral pair of ratios 1..4 is JPEG_BOX (libjpeg's integral upsampling: each chroma sample replicated over
// rh x rv pixels; 4:1:1, 4:1:0, ...), which reads JpegDesc::rh / rv.
enum JpegLayout : int32_t { JPEG_GRAY = 0, JPEG_444 = 1, JPEG_422 = 2, JPEG_420 = 3, JPEG_440 = 4, JPEG_BOX = 5 };

// jpeg_color_kernel knows the layouts up to JPEG_420 and the YCbCr transform only; an image beyond them needs the
// kernels built on color_quad (jpeg_idct.hip).
inline bool jpeg_needs_general(int layout, bool rgb_coded) { return layout > JPEG_420 || rgb_coded; }

struct JpegCompDesc {
  int32_t h, v;       // sampling factors
  int32_t bw, bh;     // stored 8x8 blocks per row / block rows (the MCU grid's coverage of this component)
  int32_t cw, ch;     // component size in samples (ceil(width * h / hmax), ceil(height * v / vmax))
  int64_t coef_off;   // int16[bh][bw][64] quantized coefficients, natural order
  int64_t plane_off;  // uint8 reconstructed samples, row stride bw * 8
};

struct JpegDesc {
  int32_t ncomp, layout, width, height;
  int32_t total_blocks;  // sum over components of bw * bh
  int32_t orientation;   // EXIF orientation 1..8 of the output (0 reads as 1): see jpeg_idct.hip for the placement
  int32_t pad_[2];       // ragged launch only (jpeg_ragged_plan below): first IDCT unit, first colour unit; else 0
  int64_t rgb_off;      // packed RGB output in the oriented geometry (the ImageMeta offset the pipeline reads)
  JpegCompDesc comp[kJpegMaxComp];
  uint16_t qt[kJpegMaxComp][64];  // dequantization table per component, natural order
  // compact payload (runtime/jpeg_decode.h jpeg_decode_compact; comp[].coef_off unused): per block a uint64
  // zigzag mask at cmask_off, a uint32 first-value index at cvoff_off, int16 values in zigzag order at cval_off
  int64_t cmask_off, cvoff_off, cval_off;
  int32_t compact;
  uint8_t rh, rv;        // JPEG_BOX: pixels per chroma sample along x / y (1..4); other layouts imply theirs
  uint8_t no_transform;  // 1: the three components are R, G, B (libjpeg's JCS_RGB); 0: YCbCr -> RGB
  uint8_t pad2_;
};
static_assert(sizeof(JpegDesc) == 576, "JpegDesc layout is shared with the kernels");

// Ragged launch of the reconstruction (jpeg_reconstruct_ragged, jpeg_idct.hip): a 1-D grid with one workgroup per
// unit of real work, where the rectangular launch sizes every image's share by the largest image of the batch.
// A unit is up to kJpegBlocksPerUnit 8x8 blocks of one image for the IDCT, and up to kJpegQuadsPerUnit 4-pixel row
// quads (ceil(width / 4) per row) of one image for the colour pass.
constexpr int kJpegBlocksPerUnit = 32;
constexpr int kJpegQuadsPerUnit = 256;

inline int jpeg_idct_units(const JpegDesc& d) { return (d.total_blocks + kJpegBlocksPerUnit - 1) / kJpegBlocksPerUnit; }
inline int jpeg_color_units(const JpegDesc& d) {
  const int64_t quads = (int64_t)((d.width + 3) >> 2) * d.height;
  return (int)((quads + kJpegQuadsPerUnit - 1) / kJpegQuadsPerUnit);
}

struct JpegRaggedPlan {
  int idct_units = 0, color_units = 0;  // grid sizes of the two ragged kernels
};

// Write each descriptor's first IDCT unit and first colour unit (exclusive prefix sums over the batch, so both
// sequences are monotone) into pad_[0] / pad_[1], where a workgroup of the ragged kernels searches for its image.
inline JpegRaggedPlan jpeg_ragged_plan(JpegDesc* descs, int n) {
  JpegRaggedPlan p;
  for (int i = 0; i < n; ++i) {
    descs[i].pad_[0] = p.idct_units;
    descs[i].pad_[1] = p.color_units;
    p.idct_units += jpeg_idct_units(descs[i]);
    p.color_units += jpeg_color_units(descs[i]);
  }
  return p;
}

}  // namespace arena
