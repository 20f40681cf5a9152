// Device half of the split JPEG decoder (host half: csrc/runtime/jpeg_decode.h).
//
// A batch of entropy-decoded images (quantized int16 coefficient blocks + one JpegDesc each) becomes packed
// HxWx3 RGB in the staging slot's image pool, where the fused letterbox/stem kernel and the crop gather read
// it — exactly the bytes the host path used to upload after a PIL decode.  Two launches per batch:
//
//   jpeg_idct_kernel    one 8x8 block per 8 lanes: dequantize (row loads of 16 B), islow pass 1 over the
//                       columns and pass 2 over the rows through an LDS transpose, 8 samples (one 8-byte store)
//                       per lane into the component's sample plane.  grid (blocks / 32, images).
//   jpeg_color_kernel   4 horizontally adjacent output pixels per lane: one dword of luma, each chroma sample
//                       loaded once per lane, fancy upsampling (h2v2 / h2v1 / none) + YCbCr->RGB, three 4-byte
//                       stores.  grid (pixels / 1024, images), grid-stride over rows x quads.
//
// A batch that holds an image with an EXIF orientation other than 1, a layout beyond JPEG_420 (4:4:0, 4:1:1, ...:
// jpeg_desc.h) or RGB-coded components launches jpeg_color_oriented_kernel in place of jpeg_color_kernel (the host
// knows from the descriptors it built); every other batch launches exactly the two kernels above.  The oriented kernel computes each quad with the same color_quad and only places it
// differently (see its comment), so its pixels are those of the plain kernel, moved.
//
// jpeg_reconstruct_ragged launches the same two stages as jpeg_idct_ragged_kernel and jpeg_color_ragged_kernel over
// 1-D grids with one workgroup per unit of real work, for batches of crops of very different sizes (see "ragged
// launch" below); same arithmetic, same bytes.
//
// The arithmetic is kernels/jpeg_math.h, the same functions the host reference (jpeg_coefs_to_rgb) uses, so
// the result is bit-identical to it and to PIL / libjpeg-turbo (tests/test_jpeg_native_gpu.py).  The work is
// a few MB of traffic per batch of 32 frames: latency, not throughput, is what the layout optimises (every
// lane of a wave does useful work; no divergent per-component loops).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "jpeg_desc.h"
#include "jpeg_math.h"
#include "launch.h"

namespace arena {

namespace {

constexpr int kBlocksPerGroup = 32;  // 8x8 blocks per 256-lane workgroup

// natural index -> zigzag index (the compact payload stores each block's coded coefficients in zigzag order),
// packed for the lanes of a block: byte l of kZigzagCol[k] is the zigzag index of natural (row l, column k).  The
// row is a lane's, so an indexed table would be one divergent memory load per coefficient; as 64-bit literals
// the lookup is a shift of an immediate.
constexpr uint64_t kZigzagCol[8] = {0x2315140a09030200ull, 0x242216130b080401ull, 0x30252117120c0705ull,
                                    0x312f262018110d06ull, 0x39322e271f19100eull, 0x3a38332d281e1a0full,
                                    0x3e3b37342c291d1bull, 0x3f3d3c36352b2a1cull};

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegDesc* __restrict__ descs, uint8_t* __restrict__ pool) {
  __shared__ int32_t ws[kBlocksPerGroup][8][9];  // +1 column: pass-1 column reads hit distinct banks
  const JpegDesc& d = descs[blockIdx.y];
  const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
  const int blk = (int)blockIdx.x * kBlocksPerGroup + g;
  const bool live = blk < d.total_blocks;
  // component of this block: at most 3 ranges
  int c = 0, b = blk;
  const int n0 = d.comp[0].bw * d.comp[0].bh;
  if (d.ncomp > 1 && b >= n0) {
    c = 1;
    b -= n0;
    const int n1 = d.comp[1].bw * d.comp[1].bh;
    if (b >= n1) {
      c = 2;
      b -= n1;
    }
  }
  const JpegCompDesc& cd = d.comp[c];
  // row l of the block: 8 int16 coefficients (16 B) and the matching 8 quantizer steps
  int32_t row[8];
  if (live && d.compact) {
    // compact payload (runtime/jpeg_decode.h jpeg_decode_compact): the block's zigzag mask and first value; the
    // coefficient at natural (l, k) is value popcount(mask below its zigzag bit) when its bit is set
    const uint64_t mask = reinterpret_cast<const uint64_t*>(pool + d.cmask_off)[blk];
    const int32_t v0 = (int32_t)reinterpret_cast<const uint32_t*>(pool + d.cvoff_off)[blk];
    const int16_t* vals = reinterpret_cast<const int16_t*>(pool + d.cval_off);
    const uint4 qv = *reinterpret_cast<const uint4*>(&d.qt[c][l * 8]);
    const uint32_t qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int z = (int)((kZigzagCol[k] >> (8 * l)) & 0xFF);
      const int idx = v0 + __popcll(mask & ((1ull << z) - 1ull));
      int32_t cf = 0;
      if ((mask >> z) & 1ull) cf = (int32_t)vals[idx];  // zero coefficients issue no load
      const int32_t q = (int32_t)((k & 1) ? (qw[k >> 1] >> 16) : (qw[k >> 1] & 0xFFFF));
      row[k] = cf * q;
    }
  } else if (live) {
    const uint4 cv = *reinterpret_cast<const uint4*>(pool + cd.coef_off + (int64_t)b * 128 + l * 16);
    const uint4 qv = *reinterpret_cast<const uint4*>(&d.qt[c][l * 8]);
    const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      row[2 * k] = (int32_t)(int16_t)(cw[k] & 0xFFFF) * (int32_t)(qw[k] & 0xFFFF);
      row[2 * k + 1] = (int32_t)(int16_t)(cw[k] >> 16) * (int32_t)(qw[k] >> 16);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = 0;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) ws[g][l][k] = row[k];
  __syncthreads();
  // pass 1: column l
  int32_t v[8], o[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = ws[g][r][l];
  jpegm::idct8<int32_t>(v, o, jpegm::kPass1Shift);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) ws[g][r][l] = o[r];
  __syncthreads();
  // pass 2: row l -> 8 samples
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = ws[g][l][k];
  jpegm::idct8<int32_t>(v, o, jpegm::kPass2Shift);
  if (!live) return;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    lo |= (uint32_t)jpegm::idct_sample<int32_t>(o[k]) << (8 * k);
    hi |= (uint32_t)jpegm::idct_sample<int32_t>(o[k + 4]) << (8 * k);
  }
  const int by = b / cd.bw, bx = b - by * cd.bw;
  const int64_t stride = (int64_t)cd.bw * 8;
  uint2* dst = reinterpret_cast<uint2*>(pool + cd.plane_off + (int64_t)(by * 8 + l) * stride + bx * 8);
  *dst = make_uint2(lo, hi);
}

// One lane = 4 horizontally adjacent output pixels x0 .. x0 + 3 (x0 = 4q) of one row.  Their luma is one aligned
// dword of the Y plane (row stride bw * 8, x0 % 4 == 0, planes 8-byte aligned: the IDCT's uint2 stores); with
// 2x horizontal chroma subsampling the four pixels need chroma columns cx0 - 1 .. cx0 + 2 (cx0 = 2q) of each
// chroma row they read, so every chroma sample is loaded once per lane instead of once per pixel and tap.  The
// per-pixel formulas (clamped neighbours, fancy upsampling, fixed-point YCbCr) are exactly chroma_at's of the
// host reference (jpeg_math.h), so the output stays bit-identical.  Rows of a width that is a multiple of 4 store
// 12-byte aligned dword triples; other widths store bytes.
struct ChromaRow {
  int v[4];  // columns max(cx0 - 1, 0), cx0, min(cx0 + 1, cw - 1), min(cx0 + 2, cw - 1)
};

__device__ __forceinline__ ChromaRow chroma_row(const uint8_t* __restrict__ row, int cx0, int cw) {
  ChromaRow r;
  r.v[0] = row[max(cx0 - 1, 0)];
  r.v[1] = row[cx0];
  r.v[2] = row[min(cx0 + 1, cw - 1)];
  r.v[3] = row[min(cx0 + 2, cw - 1)];
  return r;
}

// (cx, nx) of pixel i of the quad as indices into ChromaRow: i = 0 (cx0, cx0 - 1), 1 (cx0, cx0 + 1),
// 2 (cx0 + 1, cx0), 3 (cx0 + 1, cx0 + 2)
__device__ __forceinline__ int quad_c(int i) { return i < 2 ? 1 : 2; }
__device__ __forceinline__ int quad_n(int i) { return i == 0 ? 0 : i == 1 ? 2 : i == 2 ? 1 : 3; }

// The kernel of every batch without an EXIF orientation, a layout beyond JPEG_420 or an RGB-coded image, i.e. of
// the whole benchmark workload.  It is kept as one self-contained body, so its code object does not move when the
// oriented kernel below changes; color_quad is the same per-quad code as a function, for the oriented kernel, plus
// the layouts and the identity transform that only that kernel and the ragged one serve.
__global__ __launch_bounds__(256) void jpeg_color_kernel(const JpegDesc* __restrict__ descs, uint8_t* __restrict__ pool) {
  const JpegDesc& d = descs[blockIdx.y];
  const int W = d.width, H = d.height, layout = d.layout;
  const int qpr = (W + 3) >> 2;  // quads per row
  const int total = qpr * H;
  const uint8_t* yp = pool + d.comp[0].plane_off;
  const int ys = d.comp[0].bw * 8;
  uint8_t* out_img = pool + d.rgb_off;
  for (int t = (int)blockIdx.x * 256 + (int)threadIdx.x; t < total; t += (int)gridDim.x * 256) {
    const int y = t / qpr, q = t - y * qpr;
    const int x0 = 4 * q;
    const int n = min(4, W - x0);
    const uint32_t yw = *reinterpret_cast<const uint32_t*>(yp + (int64_t)y * ys + x0);
    uint8_t px[12];
    if (layout == JPEG_GRAY) {
#pragma unroll
      for (int i = 0; i < 4; ++i) px[3 * i] = px[3 * i + 1] = px[3 * i + 2] = (uint8_t)(yw >> (8 * i));
    } else {
      int cb[4], cr[4];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const JpegCompDesc& C = d.comp[1 + k];
        const uint8_t* cp = pool + C.plane_off;
        const int cs = C.bw * 8;
        int* dst = k == 0 ? cb : cr;
        if (layout == JPEG_444) {
          const uint32_t w = *reinterpret_cast<const uint32_t*>(cp + (int64_t)y * cs + x0);
#pragma unroll
          for (int i = 0; i < 4; ++i) dst[i] = (int)((w >> (8 * i)) & 0xFF);
        } else if (layout == JPEG_422) {
          const ChromaRow r = chroma_row(cp + (int64_t)y * cs, 2 * q, C.cw);
#pragma unroll
          for (int i = 0; i < 4; ++i) dst[i] = jpegm::fancy_h2v1(r.v[quad_c(i)], r.v[quad_n(i)], i & 1);
        } else {
          const int cy = y >> 1;
          const int ny = (y & 1) ? min(cy + 1, C.ch - 1) : max(cy - 1, 0);
          const ChromaRow a = chroma_row(cp + (int64_t)cy * cs, 2 * q, C.cw);
          const ChromaRow b = chroma_row(cp + (int64_t)ny * cs, 2 * q, C.cw);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            dst[i] = jpegm::fancy_h2v2(a.v[quad_c(i)], a.v[quad_n(i)], b.v[quad_c(i)], b.v[quad_n(i)], i & 1);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) jpegm::ycc_to_rgb((int)((yw >> (8 * i)) & 0xFF), cb[i], cr[i], px + 3 * i);
    }
    uint8_t* out = out_img + ((int64_t)y * W + x0) * 3;
    if (n == 4 && (W & 3) == 0) {
      uint32_t w[3];
#pragma unroll
      for (int k = 0; k < 3; ++k)
        w[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) |
               ((uint32_t)px[4 * k + 3] << 24);
      uint32_t* o32 = reinterpret_cast<uint32_t*>(out);
      o32[0] = w[0];
      o32[1] = w[1];
      o32[2] = w[2];
    } else {
      for (int k = 0; k < 3 * n; ++k) out[k] = px[k];
    }
  }
}

// RGB of the quad q of source row y (px: 4 pixels x 3 bytes).  All four pixels are computed whatever the width:
// the luma dword lies inside the plane's 8-sample padded row and the chroma columns are clamped.
__device__ __forceinline__ void color_quad(const JpegDesc& d, const uint8_t* __restrict__ pool,
                                           const uint8_t* __restrict__ yp, int ys, int layout, int y, int q,
                                           uint8_t* px) {
  const int x0 = 4 * q;
  const uint32_t yw = *reinterpret_cast<const uint32_t*>(yp + (int64_t)y * ys + x0);
  if (layout == JPEG_GRAY) {
#pragma unroll
    for (int i = 0; i < 4; ++i) px[3 * i] = px[3 * i + 1] = px[3 * i + 2] = (uint8_t)(yw >> (8 * i));
  } else {
    int cb[4], cr[4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const JpegCompDesc& C = d.comp[1 + k];
      const uint8_t* cp = pool + C.plane_off;
      const int cs = C.bw * 8;
      int* dst = k == 0 ? cb : cr;
      if (layout == JPEG_444) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(cp + (int64_t)y * cs + x0);
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[i] = (int)((w >> (8 * i)) & 0xFF);
      } else if (layout == JPEG_422) {
        const ChromaRow r = chroma_row(cp + (int64_t)y * cs, 2 * q, C.cw);
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[i] = jpegm::fancy_h2v1(r.v[quad_c(i)], r.v[quad_n(i)], i & 1);
      } else if (layout == JPEG_420) {
        const int cy = y >> 1;
        const int ny = (y & 1) ? min(cy + 1, C.ch - 1) : max(cy - 1, 0);
        const ChromaRow a = chroma_row(cp + (int64_t)cy * cs, 2 * q, C.cw);
        const ChromaRow b = chroma_row(cp + (int64_t)ny * cs, 2 * q, C.cw);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          dst[i] = jpegm::fancy_h2v2(a.v[quad_c(i)], a.v[quad_n(i)], b.v[quad_c(i)], b.v[quad_n(i)], i & 1);
      } else if (layout == JPEG_440) {
        // chroma as wide as luma (equal h, so the same row stride): the quad's columns are one aligned dword of
        // the nearest chroma row and one of its vertical neighbour, both rows clamped into the component
        const int cy = y >> 1;
        const int ny = (y & 1) ? min(cy + 1, C.ch - 1) : max(cy - 1, 0);
        const uint32_t wa = *reinterpret_cast<const uint32_t*>(cp + (int64_t)cy * cs + x0);
        const uint32_t wb = *reinterpret_cast<const uint32_t*>(cp + (int64_t)ny * cs + x0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          dst[i] = jpegm::fancy_h1v2((int)((wa >> (8 * i)) & 0xFF), (int)((wb >> (8 * i)) & 0xFF), y & 1);
      } else {
        // JPEG_BOX: one chroma byte per rh pixels of row y / rv; the column is clamped into the component like
        // chroma_row's, which only the pixels past the width (computed, never stored) can need
        const int rh = d.rh, rv = d.rv;
        const uint8_t* row = cp + (int64_t)min(jpegm::box_coord(y, rv), C.ch - 1) * cs;
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[i] = row[min(jpegm::box_coord(x0 + i, rh), C.cw - 1)];
      }
    }
    if (d.no_transform) {  // RGB-coded: uniform per image, like the layout
#pragma unroll
      for (int i = 0; i < 4; ++i) jpegm::rgb_identity((int)((yw >> (8 * i)) & 0xFF), cb[i], cr[i], px + 3 * i);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) jpegm::ycc_to_rgb((int)((yw >> (8 * i)) & 0xFF), cb[i], cr[i], px + 3 * i);
    }
  }
}

// One image in its stored orientation, as jpeg_color_kernel reconstructs it: the oriented kernel's path for the
// untagged images of a mixed batch.
__device__ __forceinline__ void color_plain(const JpegDesc& d, uint8_t* __restrict__ pool) {
  const int W = d.width, H = d.height, layout = d.layout;
  const int qpr = (W + 3) >> 2;  // quads per row
  const int total = qpr * H;
  const uint8_t* yp = pool + d.comp[0].plane_off;
  const int ys = d.comp[0].bw * 8;
  uint8_t* out_img = pool + d.rgb_off;
  for (int t = (int)blockIdx.x * 256 + (int)threadIdx.x; t < total; t += (int)gridDim.x * 256) {
    const int y = t / qpr, q = t - y * qpr;
    const int x0 = 4 * q;
    const int n = min(4, W - x0);
    uint8_t px[12];
    color_quad(d, pool, yp, ys, layout, y, q, px);
    uint8_t* out = out_img + ((int64_t)y * W + x0) * 3;
    if (n == 4 && (W & 3) == 0) {
      uint32_t w[3];
#pragma unroll
      for (int k = 0; k < 3; ++k)
        w[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) |
               ((uint32_t)px[4 * k + 3] << 24);
      uint32_t* o32 = reinterpret_cast<uint32_t*>(out);
      o32[0] = w[0];
      o32[1] = w[1];
      o32[2] = w[2];
    } else {
      for (int k = 0; k < 3 * n; ++k) out[k] = px[k];
    }
  }
}

// ---- EXIF-oriented output ----------------------------------------------------------------------------------------
//
// Source pixel (y, x) of a W x H image goes to (row, column) of the output:
//   2 (y, W-1-x)   3 (H-1-y, W-1-x)   4 (H-1-y, x)                        output W x H
//   5 (x, y)       6 (x, H-1-y)       7 (W-1-x, H-1-y)   8 (W-1-x, y)     output H wide, W high
// A quad is four pixels packed one per dword (r | g << 8 | b << 16) in source order; store_quad writes the first
// n of them at `out`, last pixel first when `rev` (a mirrored axis), as the plain kernel's 12-byte aligned dword
// triple when `aligned` (n == 4 and the output width a multiple of 4, so a quad's first column is too, mirrored
// or not) and as bytes otherwise.
__device__ __forceinline__ uint32_t pick4(const uint32_t* p, int i) {
  return i == 0 ? p[0] : i == 1 ? p[1] : i == 2 ? p[2] : p[3];
}

__device__ __forceinline__ void store_quad(uint8_t* __restrict__ out, const uint32_t* p, int n, bool rev,
                                           bool aligned) {
  if (aligned) {
    const uint32_t a = rev ? p[3] : p[0], b = rev ? p[2] : p[1], c = rev ? p[1] : p[2], e = rev ? p[0] : p[3];
    uint32_t* o32 = reinterpret_cast<uint32_t*>(out);
    o32[0] = a | (b << 24);
    o32[1] = (b >> 8) | (c << 16);
    o32[2] = (c >> 16) | (e << 8);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < n) {
        const uint32_t v = pick4(p, rev ? n - 1 - j : j);
        out[3 * j] = (uint8_t)v;
        out[3 * j + 1] = (uint8_t)(v >> 8);
        out[3 * j + 2] = (uint8_t)(v >> 16);
      }
    }
  }
}

// Orientations 5-8 turn a source row into an output column, so a source tile of kTile x kTile pixels is staged in
// LDS and stored transposed.  kTile = 64: a 256-lane workgroup computes the tile's 16 x 64 quads in 4 steps and
// then stores its 64 output rows x 16 quads in 4 steps; per step a wave covers 4 output rows with 16 adjacent
// lanes each, i.e. four contiguous 192-byte segments (one 12-byte store per lane).
//
// LDS: one dword per pixel, row pitch kTilePitch = 65 dwords.  Both accesses are ds_*_b32, which CDNA4's LDS
// serves in two groups of 32 lanes over 32 banks (bank = (addr / 4) mod 32).  A lane's (a, b) = (its index along
// the fast axis 0..15, along the slow axis 0..63) is laid out so that each 32-lane group holds a in 8g .. 8g + 7
// and four consecutive b:
//   write of pixel i of quad a in source row b:   dword b * 65 + 4a + i  -> bank (b + 4a + i) mod 32; 4a takes the
//     8 multiples of 4 and b the 4 residues between them: 32 distinct banks;
//   read of row 4a + i of source column b:        dword (4a + i) * 65 + b -> bank (4a + i + b) mod 32: the same set.
// Under the plain model of 64 banks x 4 B over a whole wave the same holds (a in 0..15, four consecutive b: 64
// distinct values of b + 4a mod 64), because the pitch is 1 mod 64 as well; 65 is the smallest such pitch that
// holds a 64-pixel row.  16.25 KB per workgroup.
constexpr int kTile = 64;
constexpr int kTilePitch = kTile + 1;

__global__ __launch_bounds__(256) void jpeg_color_oriented_kernel(const JpegDesc* __restrict__ descs,
                                                                  uint8_t* __restrict__ pool) {
  __shared__ uint32_t tile[kTile * kTilePitch];
  const JpegDesc& d = descs[blockIdx.y];
  const int orient = d.orientation;  // block-uniform: one image per blockIdx.y
  if (orient <= 1) {
    color_plain(d, pool);
    return;
  }
  const int W = d.width, H = d.height, layout = d.layout;
  const uint8_t* yp = pool + d.comp[0].plane_off;
  const int ys = d.comp[0].bw * 8;
  uint8_t* out_img = pool + d.rgb_off;
  if (orient <= 4) {
    // rows stay rows: the plain kernel's row-quad stores, on a flipped row and / or from a mirrored column
    const int qpr = (W + 3) >> 2;
    const int total = qpr * H;
    const bool rev = orient != 4, flip = orient != 2;
    for (int t = (int)blockIdx.x * 256 + (int)threadIdx.x; t < total; t += (int)gridDim.x * 256) {
      const int y = t / qpr, q = t - y * qpr;
      const int x0 = 4 * q;
      const int n = min(4, W - x0);
      uint8_t px[12];
      color_quad(d, pool, yp, ys, layout, y, q, px);
      uint32_t p[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        p[i] = (uint32_t)px[3 * i] | ((uint32_t)px[3 * i + 1] << 8) | ((uint32_t)px[3 * i + 2] << 16);
      const int row = flip ? H - 1 - y : y, col = rev ? W - x0 - n : x0;
      store_quad(out_img + ((int64_t)row * W + col) * 3, p, n, rev, n == 4 && (W & 3) == 0);
    }
    return;
  }
  const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
  const int wave = (int)threadIdx.x >> 6, l = (int)threadIdx.x & 63;
  const int a = (l & 7) | ((l >> 5) << 3);  // 0..15, 8 per 32-lane group
  const int b0 = ((l >> 3) & 3) + 4 * wave;  // + 16 per step
  const bool rev = orient == 6 || orient == 7;  // output columns run against the source rows
  const bool mirror = orient == 7 || orient == 8;  // output rows run against the source columns
  // the trip count is uniform over the workgroup (it depends on blockIdx alone), as the barriers need
  for (int t = (int)blockIdx.x; t < tiles_x * tiles_y; t += (int)gridDim.x) {
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int sy = ty * kTile, sx = tx * kTile;
#pragma unroll
    for (int step = 0; step < 4; ++step) {
      const int b = b0 + 16 * step;  // source row within the tile, quad a of it
      const int y = sy + b, x0 = sx + 4 * a;
      if (y < H && x0 < W) {
        uint8_t px[12];
        color_quad(d, pool, yp, ys, layout, y, x0 >> 2, px);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          tile[b * kTilePitch + 4 * a + i] =
              (uint32_t)px[3 * i] | ((uint32_t)px[3 * i + 1] << 8) | ((uint32_t)px[3 * i + 2] << 16);
      }
    }
    __syncthreads();
#pragma unroll
    for (int step = 0; step < 4; ++step) {
      const int b = b0 + 16 * step;  // source column within the tile, rows 4a .. 4a + 3 of it
      const int x = sx + b, y0 = sy + 4 * a;
      if (x < W && y0 < H) {
        const int n = min(4, H - y0);
        uint32_t p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = tile[(4 * a + i) * kTilePitch + b];  // rows >= n: stale, never stored
        const int row = mirror ? W - 1 - x : x, col = rev ? H - y0 - n : y0;
        store_quad(out_img + ((int64_t)row * H + col) * 3, p, n, rev, n == 4 && (H & 3) == 0);
      }
    }
    __syncthreads();
  }
}

// ---- ragged launch -----------------------------------------------------------------------------------------------
//
// The two kernels above run over (units of the largest image) x (images): right for a batch of similar uploads, but
// in a batch of arm B's crops, whose sizes spread over two orders of magnitude, almost every workgroup reads a
// descriptor and exits.  The ragged kernels run over a 1-D grid with one workgroup per unit of real work
// (jpeg_desc.h: 32 blocks of one image, 256 row quads of one image); the descriptors carry the exclusive prefix of
// the unit counts (pad_[0] IDCT, pad_[1] colour, written by jpeg_ragged_plan).  They are separate kernels after the
// ones above, whose code objects stay as they are; the per-block and per-quad code is the same, as functions.
static_assert(kJpegBlocksPerUnit == kBlocksPerGroup && kJpegQuadsPerUnit == 256, "unit sizes are the workgroup's");

// Image of unit u: the last descriptor whose first unit is <= u.  The prefix is monotone, so that is the number of
// descriptors with first unit <= u, less one.  The workgroup counts them 256 at a time, one load per lane (each
// descriptor is a cache line of its own, so a batch of 128 costs the workgroup 128 lines, read once) and a ballot
// per wave; the four partial counts meet in LDS (`part`, 4 ints).  No dependent chain of loads.  The result is
// uniform over the workgroup; first[0] = 0 <= u, so it is >= 0 for every unit of the grid.
template <int kField>
__device__ __forceinline__ int ragged_image(const JpegDesc* __restrict__ descs, int n, int u, int* part) {
  int count = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + (int)threadIdx.x;
    const bool below = i < n && descs[i].pad_[kField] <= u;
    count += __popcll(__ballot(below));
  }
  if (((int)threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = count;
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(part[0] + part[1] + part[2] + part[3]) - 1;
}

// Blocks group * 32 .. group * 32 + 31 of image d: the body of jpeg_idct_kernel (same loads, same LDS layout, same
// jpeg_math.h calls), with the group and the descriptor as arguments.
__device__ __forceinline__ void idct_group(const JpegDesc& d, uint8_t* __restrict__ pool, int group,
                                           int32_t (*ws)[8][9]) {
  const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
  const int blk = group * kBlocksPerGroup + g;
  const bool live = blk < d.total_blocks;
  int c = 0, b = blk;
  const int n0 = d.comp[0].bw * d.comp[0].bh;
  if (d.ncomp > 1 && b >= n0) {
    c = 1;
    b -= n0;
    const int n1 = d.comp[1].bw * d.comp[1].bh;
    if (b >= n1) {
      c = 2;
      b -= n1;
    }
  }
  const JpegCompDesc& cd = d.comp[c];
  int32_t row[8];
  if (live && d.compact) {
    const uint64_t mask = reinterpret_cast<const uint64_t*>(pool + d.cmask_off)[blk];
    const int32_t v0 = (int32_t)reinterpret_cast<const uint32_t*>(pool + d.cvoff_off)[blk];
    const int16_t* vals = reinterpret_cast<const int16_t*>(pool + d.cval_off);
    const uint4 qv = *reinterpret_cast<const uint4*>(&d.qt[c][l * 8]);
    const uint32_t qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int z = (int)((kZigzagCol[k] >> (8 * l)) & 0xFF);
      const int idx = v0 + __popcll(mask & ((1ull << z) - 1ull));
      int32_t cf = 0;
      if ((mask >> z) & 1ull) cf = (int32_t)vals[idx];  // zero coefficients issue no load
      const int32_t q = (int32_t)((k & 1) ? (qw[k >> 1] >> 16) : (qw[k >> 1] & 0xFFFF));
      row[k] = cf * q;
    }
  } else if (live) {
    const uint4 cv = *reinterpret_cast<const uint4*>(pool + cd.coef_off + (int64_t)b * 128 + l * 16);
    const uint4 qv = *reinterpret_cast<const uint4*>(&d.qt[c][l * 8]);
    const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      row[2 * k] = (int32_t)(int16_t)(cw[k] & 0xFFFF) * (int32_t)(qw[k] & 0xFFFF);
      row[2 * k + 1] = (int32_t)(int16_t)(cw[k] >> 16) * (int32_t)(qw[k] >> 16);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = 0;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) ws[g][l][k] = row[k];
  __syncthreads();
  // pass 1: column l
  int32_t v[8], o[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = ws[g][r][l];
  jpegm::idct8<int32_t>(v, o, jpegm::kPass1Shift);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) ws[g][r][l] = o[r];
  __syncthreads();
  // pass 2: row l -> 8 samples
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = ws[g][l][k];
  jpegm::idct8<int32_t>(v, o, jpegm::kPass2Shift);
  if (!live) return;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    lo |= (uint32_t)jpegm::idct_sample<int32_t>(o[k]) << (8 * k);
    hi |= (uint32_t)jpegm::idct_sample<int32_t>(o[k + 4]) << (8 * k);
  }
  const int by = b / cd.bw, bx = b - by * cd.bw;
  const int64_t stride = (int64_t)cd.bw * 8;
  uint2* dst = reinterpret_cast<uint2*>(pool + cd.plane_off + (int64_t)(by * 8 + l) * stride + bx * 8);
  *dst = make_uint2(lo, hi);
}

__global__ __launch_bounds__(256) void jpeg_idct_ragged_kernel(const JpegDesc* __restrict__ descs,
                                                               uint8_t* __restrict__ pool, int n_images) {
  __shared__ int32_t ws[kBlocksPerGroup][8][9];  // jpeg_idct_kernel's layout
  __shared__ int part[4];
  const int u = (int)blockIdx.x;
  const int img = ragged_image<0>(descs, n_images, u, part);
  if (img < 0) return;  // never for a grid of jpeg_ragged_plan's size; uniform over the workgroup
  const JpegDesc& d = descs[img];
  idct_group(d, pool, u - d.pad_[0], ws);
}

// Quads unit * 256 .. unit * 256 + 255 of an image's rows x quads, one per lane: color_quad and jpeg_color_kernel's
// stores.  The units of an image cover its ceil(W / 4) * H quads exactly, so there is no grid-stride loop.
__global__ __launch_bounds__(256) void jpeg_color_ragged_kernel(const JpegDesc* __restrict__ descs,
                                                                uint8_t* __restrict__ pool, int n_images) {
  __shared__ int part[4];
  const int u = (int)blockIdx.x;
  const int img = ragged_image<1>(descs, n_images, u, part);
  if (img < 0) return;
  const JpegDesc& d = descs[img];
  const int W = d.width, H = d.height, layout = d.layout;
  const int qpr = (W + 3) >> 2;  // quads per row
  const int total = qpr * H;
  const int t = (u - d.pad_[1]) * 256 + (int)threadIdx.x;
  if (t >= total) return;
  const uint8_t* yp = pool + d.comp[0].plane_off;
  const int ys = d.comp[0].bw * 8;
  const int y = t / qpr, q = t - y * qpr;
  const int x0 = 4 * q;
  const int n = min(4, W - x0);
  uint8_t px[12];
  color_quad(d, pool, yp, ys, layout, y, q, px);
  uint8_t* out = pool + d.rgb_off + ((int64_t)y * W + x0) * 3;
  if (n == 4 && (W & 3) == 0) {
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      w[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) |
             ((uint32_t)px[4 * k + 3] << 24);
    uint32_t* o32 = reinterpret_cast<uint32_t*>(out);
    o32[0] = w[0];
    o32[1] = w[1];
    o32[2] = w[2];
  } else {
    for (int k = 0; k < 3 * n; ++k) out[k] = px[k];
  }
}

}  // namespace

void jpeg_reconstruct_ragged(const JpegDesc* d_descs, uint8_t* d_pool, int n_images, int idct_units, int color_units,
                             hipStream_t s) {
  if (n_images <= 0) return;
  if (idct_units > 0)
    hipLaunchKernelGGL(jpeg_idct_ragged_kernel, dim3((unsigned)idct_units), dim3(256), 0, s, d_descs, d_pool, n_images);
  if (color_units > 0)
    hipLaunchKernelGGL(jpeg_color_ragged_kernel, dim3((unsigned)color_units), dim3(256), 0, s, d_descs, d_pool,
                       n_images);
}

void jpeg_reconstruct(const JpegDesc* d_descs, uint8_t* d_pool, int n_images, int max_blocks, int64_t max_pixels,
                      hipStream_t s, bool general) {
  if (n_images <= 0) return;
  const dim3 g1((unsigned)((max_blocks + kBlocksPerGroup - 1) / kBlocksPerGroup), (unsigned)n_images);
  if (max_blocks > 0) hipLaunchKernelGGL(jpeg_idct_kernel, g1, dim3(256), 0, s, d_descs, d_pool);
  // one lane per 4-pixel quad of a row, grid-stride over the image's rows x quads
  const dim3 g2((unsigned)std::max<int64_t>(1, (max_pixels + 1023) / 1024), (unsigned)n_images);
  if (max_pixels <= 0) return;
  if (general) hipLaunchKernelGGL(jpeg_color_oriented_kernel, g2, dim3(256), 0, s, d_descs, d_pool);
  else hipLaunchKernelGGL(jpeg_color_kernel, g2, dim3(256), 0, s, d_descs, d_pool);
}

}  // namespace arena
