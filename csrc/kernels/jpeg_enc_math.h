// Integer compression arithmetic of a baseline JPEG, shared by the host reference encoder
// (csrc/runtime/jpeg_encode.cpp) and the device kernel (csrc/kernels/jpeg_fdct.hip): the mirror image of
// jpeg_math.h.
//
// The reference's arm B sends every crop as a PIL JPEG at quality 95 (architectures/microservices/detection/app/
// grpc_client.py:99-103), i.e. libjpeg(-turbo) with its default compression settings: table-driven RGB->YCbCr,
// h2v2 box-filter chroma downsampling with the alternating bias, the accurate integer forward DCT (JDCT_ISLOW) and
// division-with-rounding quantisation.  This header reproduces exactly that arithmetic, so the coefficients, and
// with the standard Huffman tables the bytes, are PIL's (tests/test_jpeg_encode.py pins that).
//
// Attribution: the colour conversion follows libjpeg's jccolor.c (rgb_ycc_convert and its rgb_ycc_start tables),
// the downsampling jcsample.c (h2v2_downsample, expand_right_edge), the forward DCT the structure and fixed-point
// constants of jfdctint.c (jpeg_fdct_islow), the quantisation jcdctmgr.c (forward_DCT).  The host half
// (runtime/jpeg_encode.cpp) follows jchuff.c (encode_one_block), jcmarker.c (marker layout) and jcparam.c (quality
// scaling, the Annex K tables).  This software is based in part on the work of the Independent JPEG Group (see
// NOTICE at the repository root).
//
// As in jpeg_math.h there is no table and no memory access: the same functions run per lane in the HIP kernel and
// per sample in the host reference.
#pragma once
#include "jpeg_math.h"

namespace arena {
namespace jpegm {

// RGB -> YCbCr (jccolor.c, SCALEBITS 16, FIX(x) = round(x * 65536)).  The chroma bias is CBCR_OFFSET +
// ONE_HALF - 1: libjpeg folds "one half minus one" into the B->Cb / R->Cr tables so that 255,255,255 maps to 128.
ARENA_JHD void rgb_to_ycc(int r, int g, int b, int& y, int& cb, int& cr) {
  y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;                          // .299 .587 .114
  cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;         // .16874 .33126 .5
  cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;           // .5 .41869 .08131
}

// h2v2 downsampling (jcsample.c): the four input samples under output column `c`; the bias alternates 1, 2, 1, 2
// along a row so that the rounding does not drift.
ARENA_JHD int h2v2_down(int a, int b, int c_, int d, int c) { return (a + b + c_ + d + ((c & 1) ? 2 : 1)) >> 2; }

// The 1-D forward DCT of jpeg_fdct_islow over d[0..7] (samples minus 128 in pass 1).  Pass 1 (rows) leaves its
// outputs scaled up by 2^kPass1Bits, pass 2 (columns) removes that scale again; both leave the factor 8 of the 2-D
// transform, which the quantiser divides out (quantize: step q * 8).
//
// int32 holds every intermediate for |sample - 128| <= 128:
//   pass 1: |d| <= 128, so |tmp0..7| <= 256, |tmp10..13| <= 512 and |z1..z4| <= 512; the largest product is
//           z5 = (z3 + z4) * 9633 with |z3 + z4| <= 1024, under 2^24, and the sums of at most four such terms stay
//           under 2^27.  An output is 4 * sqrt(2) * sum d[x] cos(..) (k > 0) or 4 * sum d[x] (k = 0), so
//           |out| <= max(4 * 1.4143 * 128 * 5.126, 4 * 8 * 128) = 4096.
//   pass 2: |d| <= 4096, so |tmp0..7| <= 8192, |z1..z4| <= 16384, |z3 + z4| <= 32768: z5 <= 32768 * 9633 < 3.2e8,
//           z3 * 16069 and z4 * 3196 < 2.7e8, so |z3|, |z4| after adding z5 < 5.9e8; an output sums one tmp product
//           (<= 8192 * 25172 < 2.1e8), one of z1 / z2 (<= 16384 * 20995 < 3.5e8) and one of z3 / z4: < 1.15e9 < 2^31.
// The 0/255 checkerboards of the tests are the extreme inputs; the stand-alone check (csrc/tests/
// jpeg_encode_check.cpp) compares the int32 and int64 instantiations on them.
template <typename T>
ARENA_JHD void fdct8(const T d[8], T out[8], bool first) {
  T tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  T tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const T tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  const int n = first ? kConstBits - kPass1Bits : kConstBits + kPass1Bits;
  if (first) {
    out[0] = (tmp10 + tmp11) * ((T)1 << kPass1Bits);
    out[4] = (tmp10 - tmp11) * ((T)1 << kPass1Bits);
  } else {
    out[0] = descale<T>(tmp10 + tmp11, kPass1Bits);
    out[4] = descale<T>(tmp10 - tmp11, kPass1Bits);
  }
  T z1 = (tmp12 + tmp13) * F_0_541196100;
  out[2] = descale<T>(z1 + tmp13 * F_0_765366865, n);
  out[6] = descale<T>(z1 + tmp12 * (-F_1_847759065), n);
  z1 = tmp4 + tmp7;
  T z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const T z5 = (z3 + z4) * F_1_175875602;
  tmp4 = tmp4 * F_0_298631336;
  tmp5 = tmp5 * F_2_053119869;
  tmp6 = tmp6 * F_3_072711026;
  tmp7 = tmp7 * F_1_501321110;
  z1 = z1 * (-F_0_899976223);
  z2 = z2 * (-F_2_562915447);
  z3 = z3 * (-F_1_961570560) + z5;
  z4 = z4 * (-F_0_390180644) + z5;
  out[7] = descale<T>(tmp4 + z1 + z3, n);
  out[5] = descale<T>(tmp5 + z2 + z4, n);
  out[3] = descale<T>(tmp6 + z2 + z3, n);
  out[1] = descale<T>(tmp7 + z1 + z4, n);
}

template <typename T>
ARENA_JHD void fdct8_rows(const T d[8], T out[8]) { fdct8<T>(d, out, true); }
template <typename T>
ARENA_JHD void fdct8_cols(const T d[8], T out[8]) { fdct8<T>(d, out, false); }

// Quantise a pass-2 output by table entry q (jcdctmgr.c: the divisor is q << 3, rounding half away from zero).
ARENA_JHD int quantize(int coef, int q) {
  const int step = q << 3;
  const int a = coef < 0 ? -coef : coef;
  const int m = (a + (step >> 1)) / step;
  return coef < 0 ? -m : m;
}

// Geometry of a W x H crop coded 4:2:0: which source pixels a sample reads.  Luma sample (y, x) is the pixel at
// (min(y, H - 1), min(x, W - 1)).  Chroma sample (r, c) averages rows chroma_row0/1 and columns min(2c, W - 1),
// min(2c + 1, W - 1): horizontally libjpeg edge-extends the input before it downsamples (c is not clamped),
// vertically it replicates only the odd last row before and the last downsampled row after (r is clamped first).
ARENA_JHD int enc_clamp(int v, int hi) { return v < hi ? v : hi; }
ARENA_JHD int chroma_row0(int r, int H) { return enc_clamp(2 * enc_clamp(r, (H + 1) / 2 - 1), H - 1); }
ARENA_JHD int chroma_row1(int r, int H) { return enc_clamp(2 * enc_clamp(r, (H + 1) / 2 - 1) + 1, H - 1); }

}  // namespace jpegm
}  // namespace arena
