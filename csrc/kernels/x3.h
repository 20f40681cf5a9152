// The triple-bf16 ("x3") scheme of the fp32 pipeline: fp32-level error from the bf16 matrix cores.
//
// Every fp32 operand is split into three bf16 planes,
//   h = bf16(v),  m = bf16(v - h),  l = bf16(v - h - m)        (each conversion rounds to nearest even),
// both residuals are exact in fp32 and 3 x 8 significant bits cover fp32's 24, so v = h + m + l.  Of the nine
// plane products of a * b six are kept and accumulated in fp32, smallest first:
//   am*bm, al*bh, ah*bl   (<= 2^-16 |a||b|),   am*bh, ah*bm   (<= 2^-8 |a||b|),   ah*bh.
// The dropped three (am*bl, al*bm, al*bl) are below 2^-24 |a||b|, the size of fp32's own product rounding, and
// a bf16 product is exact in the fp32 accumulator.  Smallest first because the small terms then meet a small
// partial sum and keep their low bits; added last they would be rounded at the size of ah*bh.  When one operand
// is exactly bf16 (one plane) three products remain: al*x, am*x, ah*x.
//
// The planes a kernel computes must equal the planes the planner packs for the weights: the host twin of the
// split is engine/planner.py split_bf16x3.  The split has two forms that give the same bits but not the same
// instructions (csrc/tests/x3_split_check.cpp compares them on the host, tests/test_x3_split.py against the
// planner): element by element (x3_split, x3_split_at, x3_split4, x3_split8) and two values at a time
// (split_bf16x3_pair, x3_split4_pair, x3_split8_pair).  Which one a kernel uses is part of its measured
// instruction stream, and so is the spelling within a form: the compiler schedules a loop over x3_split (planes
// stored after all three are known) differently from one over x3_split_at (h and m stored before l is formed).
// Move a kernel from one to another only with a measurement.
//
// The split compiles as plain host C++ too (clang: __bf16 and ext_vector_type); the product chains, the tile
// remap and everything else of common.h are device code.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#include "common.h"
#define ARENA_X3HD __host__ __device__ __forceinline__
#else
typedef __bf16 bf16;  // the vector types of common.h that the split needs
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define ARENA_X3HD inline
#endif

namespace arena {

// ---- the split, element by element
ARENA_X3HD void x3_split(float v, bf16& h, bf16& m, bf16& l) {
  h = (bf16)v;
  const float r = v - (float)h;
  m = (bf16)r;
  l = (bf16)(r - (float)m);
}

// the same into element i of the plane vectors
template <typename V>
ARENA_X3HD void x3_split_at(float v, int i, V& h, V& m, V& l) {
  const bf16 th = (bf16)v;
  const float r = v - (float)th;
  const bf16 tm = (bf16)r;
  h[i] = th;
  m[i] = tm;
  l[i] = (bf16)(r - (float)tm);
}
ARENA_X3HD void x3_split4(const float* v, bf16x4& h, bf16x4& m, bf16x4& l) {
#pragma unroll
  for (int i = 0; i < 4; ++i) x3_split_at(v[i], i, h, m, l);
}
ARENA_X3HD void x3_split8(const float* v, bf16x8& h, bf16x8& m, bf16x8& l) {
#pragma unroll
  for (int i = 0; i < 8; ++i) x3_split_at(v[i], i, h, m, l);
}

// ---- the split, two values at a time: 10 VALU per pair instead of 12-13.  One v_cvt_pk_bf16_f32 converts both
// values, the packed word is widened back with one shift (low half) and one mask (high half), and the residual
// is one v_pk_add_f32.
ARENA_X3HD f32x2 widen_bf16x2(bf16x2 v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  return f32x2{__builtin_bit_cast(float, u << 16), __builtin_bit_cast(float, u & 0xffff0000u)};
}
ARENA_X3HD void split_bf16x3_pair(f32x2 v, bf16x2& h, bf16x2& m, bf16x2& l) {
  h = __builtin_convertvector(v, bf16x2);
  const f32x2 r = v - widen_bf16x2(h);
  m = __builtin_convertvector(r, bf16x2);
  l = __builtin_convertvector(r - widen_bf16x2(m), bf16x2);
}
ARENA_X3HD void x3_split4_pair(f32x2 v0, f32x2 v1, bf16x4& h, bf16x4& m, bf16x4& l) {
  bf16x2 h0, m0, l0, h1, m1, l1;
  split_bf16x3_pair(v0, h0, m0, l0);
  split_bf16x3_pair(v1, h1, m1, l1);
  h = __builtin_shufflevector(h0, h1, 0, 1, 2, 3);
  m = __builtin_shufflevector(m0, m1, 0, 1, 2, 3);
  l = __builtin_shufflevector(l0, l1, 0, 1, 2, 3);
}
ARENA_X3HD void x3_split8_pair(const float* v, bf16x8& h, bf16x8& m, bf16x8& l) {
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    bf16x2 th, tm, tl;
    split_bf16x3_pair(f32x2{v[i], v[i + 1]}, th, tm, tl);
    h[i] = th[0]; h[i + 1] = th[1];
    m[i] = tm[0]; m[i + 1] = tm[1];
    l[i] = tl[0]; l[i + 1] = tl[1];
  }
}

#if defined(__HIPCC__) || defined(__HIP__)

// ---- the six-product chain c += a * b, one overload per MFMA shape (told apart by fragment and accumulator)
// v_mfma_f32_16x16x32_bf16
__device__ __forceinline__ f32x4 x3_mfma(const bf16x8& ah, const bf16x8& am, const bf16x8& al, const bf16x8& bh,
                                         const bf16x8& bm, const bf16x8& bl, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bm, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bm, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
}
// v_mfma_f32_32x32x16_bf16
__device__ __forceinline__ f32x16 x3_mfma(const bf16x8& ah, const bf16x8& am, const bf16x8& al, const bf16x8& bh,
                                          const bf16x8& bm, const bf16x8& bl, f32x16 c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
}
// v_mfma_f32_16x16x16_bf16 (16-deep K without padding)
__device__ __forceinline__ f32x4 x3_mfma(const bf16x4& ah, const bf16x4& am, const bf16x4& al, const bf16x4& bh,
                                         const bf16x4& bm, const bf16x4& bl, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(am, bm, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ah, bl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(am, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ah, bm, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ah, bh, c, 0, 0, 0);
}
// b is exactly bf16: three products (16x16x32)
__device__ __forceinline__ f32x4 x3_mfma_b1(const bf16x8& ah, const bf16x8& am, const bf16x8& al, const bf16x8& b,
                                            f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, b, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, b, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b, c, 0, 0, 0);
}

// Bijective XCD-aware block remap (8 XCDs, round-robin dispatch): consecutive
// logical tiles land on the same XCD so neighbouring pixel tiles share its L2.
__device__ __forceinline__ int xcd_remap(int bx, int nx) {
  const int q = nx / 8, r = nx % 8, x = bx % 8, y = bx / 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + y;
}

#endif

}  // namespace arena
