// Device helpers shared by the tiled x3 inverted-residual kernels (ir_tile_x3.hip, ir_s2k16_x3.hip): the E / D
// LDS layouts and the packed depthwise accumulator.  The plane splits and the six-product MFMA chain are x3.h's.
#pragma once

#include "x3.h"

namespace arena {

constexpr int ITX_HC = 32;                    // hidden channels per chunk
constexpr int ITX_DPB = 3 * ITX_HC * 2 + 32;  // bytes per D pixel row: [h|m|l][32] bf16 + pad (14 slots)

__host__ __device__ constexpr int itx_ep(int S) { return S == 1 ? ITX_HC : ITX_HC + 4; }  // E pixel pitch

template <int S>
__device__ __forceinline__ int itx_eswz(int pix, int g) {
  const int f = S == 1 ? ((pix ^ (4 * (pix >> 2))) & 7) : 0;
  return (g & ~7) | ((g & 7) ^ f);
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
    x3_split4_pair(f32x2{relu6f(a0[0]), relu6f(a0[1])}, f32x2{relu6f(a1[0]), relu6f(a1[1])}, dh, dm, dl);
    *(bf16x4*)d = dh;
    *(bf16x4*)(d + 64) = dm;
    *(bf16x4*)(d + 128) = dl;
  }
};

__device__ __forceinline__ float4 itx_relu6x4(float4 v) {
  return make_float4(relu6f(v.x), relu6f(v.y), relu6f(v.z), relu6f(v.w));
}

}  // namespace arena
