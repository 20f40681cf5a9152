// Device helpers shared by the tiled x3 inverted-residual kernels (ir_tile_x3.hip, ir_s2k16_x3.hip): the E / D
// LDS layouts, the bf16 plane splits, the packed depthwise accumulator and the six-product MFMA chain.
#pragma once

#include "common.h"

namespace arena {

constexpr int ITX_HC = 32;                    // hidden channels per chunk
constexpr int ITX_DPB = 3 * ITX_HC * 2 + 32;  // bytes per D pixel row: [h|m|l][32] bf16 + pad (14 slots)

__host__ __device__ constexpr int itx_ep(int S) { return S == 1 ? ITX_HC : ITX_HC + 4; }  // E pixel pitch

template <int S>
__device__ __forceinline__ int itx_eswz(int pix, int g) {
  const int f = S == 1 ? ((pix ^ (4 * (pix >> 2))) & 7) : 0;
  return (g & ~7) | ((g & 7) ^ f);
}

// v = h + m + l planes of 8 / 4 values, two at a time (common.h split_bf16x3_pair)
__device__ __forceinline__ void itx_split8(const float* v, bf16x8& h, bf16x8& m, bf16x8& l) {
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    bf16x2 th, tm, tl;
    split_bf16x3_pair(f32x2{v[i], v[i + 1]}, th, tm, tl);
    h[i] = th[0]; h[i + 1] = th[1];
    m[i] = tm[0]; m[i + 1] = tm[1];
    l[i] = tl[0]; l[i + 1] = tl[1];
  }
}

__device__ __forceinline__ void itx_split4(f32x2 v0, f32x2 v1, bf16x4& h, bf16x4& m, bf16x4& l) {
  bf16x2 h0, m0, l0, h1, m1, l1;
  split_bf16x3_pair(v0, h0, m0, l0);
  split_bf16x3_pair(v1, h1, m1, l1);
  h = __builtin_shufflevector(h0, h1, 0, 1, 2, 3);
  m = __builtin_shufflevector(m0, m1, 0, 1, 2, 3);
  l = __builtin_shufflevector(l0, l1, 0, 1, 2, 3);
}

// Depthwise accumulator of one output pixel's 4 channels as two channel pairs: every tap is two v_pk_fma_f32
// (each lane rounds like fmaf, so the result is that of the scalar chain bias, tap 0, .. tap 8).
struct ItxDw {
  f32x2 a0, a1;
  __device__ __forceinline__ explicit ItxDw(const float4 b) : a0{b.x, b.y}, a1{b.z, b.w} {}
  __device__ __forceinline__ void tap(const float4 v, const float4 w) {
    a0 = __builtin_elementwise_fma(f32x2{v.x, v.y}, f32x2{w.x, w.y}, a0);
    a1 = __builtin_elementwise_fma(f32x2{v.z, v.w}, f32x2{w.z, w.w}, a1);
  }
  // ReLU6, split, the three bf16 planes of D (d: the pixel's row + 8 * channel group)
  __device__ __forceinline__ void store(uint8_t* d) const {
    bf16x4 dh, dm, dl;
    itx_split4(f32x2{relu6f(a0[0]), relu6f(a0[1])}, f32x2{relu6f(a1[0]), relu6f(a1[1])}, dh, dm, dl);
    *(bf16x4*)d = dh;
    *(bf16x4*)(d + 64) = dm;
    *(bf16x4*)(d + 128) = dl;
  }
};

__device__ __forceinline__ f32x4 itx_mfma(const bf16x8& ah, const bf16x8& am, const bf16x8& al, const bf16x8& bh,
                                          const bf16x8& bm, const bf16x8& bl, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bm, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bm, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
}

__device__ __forceinline__ float4 itx_relu6x4(float4 v) {
  return make_float4(relu6f(v.x), relu6f(v.y), relu6f(v.z), relu6f(v.w));
}

}  // namespace arena
