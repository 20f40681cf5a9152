// Device half of the JPEG crop encoder (host half: csrc/runtime/jpeg_encode.h), the mirror image of
// jpeg_idct.hip.
//
// One launch turns a list of crop windows of a device-resident packed RGB frame into the quantised DCT
// coefficient blocks of their 4:2:0 baseline JPEGs; the host only Huffman-codes them.  There are no intermediate
// planes in global memory: a lane produces its samples straight from the frame.
//
//   jpeg_fdct_kernel   one 8x8 block per 8 lanes, 32 blocks per 256-lane workgroup, grid (block groups, crops).
//                      Blocks are numbered in scan order, MCU by MCU: Y00 Y01 Y10 Y11 Cb Cr.  Lane l makes row l
//                      of its block: a luma lane converts 8 pixels, a chroma lane converts the 16x2 pixels under
//                      its 8 samples and downsamples them.  Pass 1 of the islow forward DCT runs on that row in
//                      registers, an LDS transpose ([8][9] padded) hands each lane a column for pass 2, a second
//                      transpose hands it row l of the result, which it quantises.
//
// Output order: natural (row-major) order, not zigzag.  A lane then owns 8 adjacent coefficients and a block is
// eight 16-byte stores to 128 contiguous bytes (a wave writes 1 KiB contiguously); in zigzag order the same lane
// would scatter eight 2-byte stores.  The host Huffman pass reads each block through the zigzag table instead.
//
// Every pixel read is clamped into the crop window (jpeg_enc_math.h: libjpeg's edge replication is exactly that
// clamp), and the host validated that the window lies inside the frame, so nothing outside the frame is read.
// Block slots beyond a component's real grid (the dummy blocks of partial MCUs) are computed from clamped pixels
// like any other and ignored by the host writer, which codes them as libjpeg does.
//
// The arithmetic is kernels/jpeg_enc_math.h, the functions the host reference (jpeg_encode_coefs_host) runs, in
// int32 (the bound is derived there), so the coefficients are bit-identical to it and to PIL / libjpeg-turbo
// (tests/test_jpeg_encode_gpu.py).
#include <hip/hip_runtime.h>

#include "jpeg_enc_desc.h"
#include "jpeg_enc_math.h"
#include "launch.h"

namespace arena {

namespace {

constexpr int kBlocksPerGroup = 32;  // 8x8 blocks per 256-lane workgroup

__device__ __forceinline__ void load_ycc(const uint8_t* __restrict__ p, int& y, int& cb, int& cr) {
  jpegm::rgb_to_ycc((int)p[0], (int)p[1], (int)p[2], y, cb, cr);
}

__global__ __launch_bounds__(256) void jpeg_fdct_kernel(const JpegEncDesc* __restrict__ descs,
                                                        const uint8_t* __restrict__ frame,
                                                        uint8_t* __restrict__ coef,
                                                        const uint16_t* __restrict__ qt) {
  // +1 column: the column accesses of the transposes hit distinct banks (bank = 8g + 9r + l mod 32 over the four
  // blocks of a 32-lane group)
  __shared__ int32_t ws[kBlocksPerGroup][8][9];
  const JpegEncDesc d = descs[blockIdx.y];
  const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
  const int blk = (int)blockIdx.x * kBlocksPerGroup + g;
  const bool live = blk < d.total_blocks;
  const int W = d.w, H = d.h;
  const int mcu = blk / kJpegEncBlocksPerMcu, s = blk - mcu * kJpegEncBlocksPerMcu;
  const int my = mcu / d.mcux, mx = mcu - my * d.mcux;
  const bool chroma = s >= 4;
  const uint8_t* src = frame + d.src_off;
  int32_t v[8], o[8];
  if (!live) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0;
  } else if (!chroma) {
    const int y = min(my * 16 + (s >> 1) * 8 + l, H - 1);
    const int x0 = mx * 16 + (s & 1) * 8;
    const uint8_t* row = src + (int64_t)y * d.pitch;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int yy, cb, cr;
      load_ycc(row + 3 * min(x0 + k, W - 1), yy, cb, cr);
      v[k] = yy - 128;
    }
  } else {
    const int r = my * 8 + l;
    const uint8_t* row0 = src + (int64_t)jpegm::chroma_row0(r, H) * d.pitch;
    const uint8_t* row1 = src + (int64_t)jpegm::chroma_row1(r, H) * d.pitch;
    const bool want_cr = s == 5;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = mx * 8 + k;
      const int xa = 3 * min(2 * c, W - 1), xb = 3 * min(2 * c + 1, W - 1);
      int yy, cb[4], cr[4];
      load_ycc(row0 + xa, yy, cb[0], cr[0]);
      load_ycc(row0 + xb, yy, cb[1], cr[1]);
      load_ycc(row1 + xa, yy, cb[2], cr[2]);
      load_ycc(row1 + xb, yy, cb[3], cr[3]);
      const int sb = jpegm::h2v2_down(cb[0], cb[1], cb[2], cb[3], c);
      const int sr = jpegm::h2v2_down(cr[0], cr[1], cr[2], cr[3], c);
      v[k] = (want_cr ? sr : sb) - 128;
    }
  }
  // pass 1: row l
  jpegm::fdct8_rows<int32_t>(v, o);
#pragma unroll
  for (int k = 0; k < 8; ++k) ws[g][l][k] = o[k];
  __syncthreads();
  // pass 2: column l; the outputs go back to the column this lane just read, so no barrier in between
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = ws[g][r][l];
  jpegm::fdct8_cols<int32_t>(v, o);
#pragma unroll
  for (int r = 0; r < 8; ++r) ws[g][r][l] = o[r];
  __syncthreads();
  if (!live) return;
  // row l of the coefficients and of the component's table: quantise, one 16-byte store
  const uint4 qv = *reinterpret_cast<const uint4*>(qt + (chroma ? 64 : 0) + l * 8);
  const uint32_t qw[4] = {qv.x, qv.y, qv.z, qv.w};
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int a = jpegm::quantize(ws[g][l][2 * k], (int)(qw[k] & 0xFFFF));
    const int b = jpegm::quantize(ws[g][l][2 * k + 1], (int)(qw[k] >> 16));
    w[k] = (uint32_t)(uint16_t)(int16_t)a | ((uint32_t)(uint16_t)(int16_t)b << 16);
  }
  uint4* dst = reinterpret_cast<uint4*>(coef + d.out_off + (int64_t)blk * 128 + l * 16);
  *dst = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace

void jpeg_forward(const JpegEncDesc* d_descs, const uint8_t* d_frame, uint8_t* d_coef, const uint16_t* d_qt,
                  int n_crops, int max_blocks, hipStream_t s) {
  if (n_crops <= 0 || max_blocks <= 0) return;
  const dim3 grid((unsigned)((max_blocks + kBlocksPerGroup - 1) / kBlocksPerGroup), (unsigned)n_crops);
  hipLaunchKernelGGL(jpeg_fdct_kernel, grid, dim3(256), 0, s, d_descs, d_frame, d_coef, d_qt);
}

}  // namespace arena
