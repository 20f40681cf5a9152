// Detect-head cell marks (runtime/head_marks.h): one int per 8 x 8-pixel cell and image, 1 iff a class logit of an
// in-map pixel of the cell is >= gate_min.
//
// One wave per cell, four cells per workgroup, all gated levels of a program in one launch (cells numbered level by
// level, image by image).  A cell is 64 pixels x 80 logits = 1280 float4 items, 20 per lane, lane-consecutive items
// being the consecutive 16-byte pieces of a pixel's 320 bytes; all 20 loads are issued before the first compare.  An
// item outside the map holds NaN, which passes nothing, as does a NaN logit.  Lane 0 writes the cell's mark (a plain
// vector store of 0 or 1, so no zero-fill pass and no atomics); the cells of images at or past the live count are
// not touched.  The kernel is the class-logit read that the gated box convs do per tile today, done once per level.
#include <stdexcept>
#include <string>

#include "../runtime/head_marks.h"
#include "common.h"
#include "launch.h"

namespace arena {

namespace {
constexpr int HM_WAVES = 4;
}

template <int NQ>  // float4 pieces per pixel
__global__ __launch_bounds__(HM_WAVES * 64) void head_mark_kernel(const HeadMarkParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int g = blockIdx.x * HM_WAVES + wave;  // cell number over levels, images and cells (wave-uniform)
  const int live = live_batch(p.B, p.bdev);
  int l = 0, ncy = 0, ncx = 0;
  for (; l < p.n_levels; ++l) {
    ncy = head_mark_cells(p.H[l]);
    ncx = head_mark_cells(p.W[l]);
    if (g < p.B * ncy * ncx) break;
    g -= p.B * ncy * ncx;
  }
  if (l >= p.n_levels) return;
  // kMarkMaxLevels is small: select by compare, so that the arrays stay in the kernel-argument segment
  const float* logits = l == 0 ? p.logits[0] : l == 1 ? p.logits[1] : p.logits[2];
  int* marks = l == 0 ? p.marks[0] : l == 1 ? p.marks[1] : p.marks[2];
  const int H = l == 0 ? p.H[0] : l == 1 ? p.H[1] : p.H[2];
  const int W = l == 0 ? p.W[0] : l == 1 ? p.W[1] : p.W[2];
  const int ps = l == 0 ? p.ps[0] : l == 1 ? p.ps[1] : p.ps[2];
  const int cells = ncy * ncx;
  const int b = g / cells;
  if (b >= live) return;
  const int c = g - b * cells;
  const int cy = c / ncx, cx = c - cy * ncx;
  const float nan = __builtin_nanf("");
  const float* img = logits + (size_t)b * H * W * ps;
  float4 v[NQ];
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const int i = lane + 64 * j;
    const int px = i / NQ, q = i - px * NQ;
    const int y = cy * kMarkCell + (px >> 3), x = cx * kMarkCell + (px & 7);
    v[j] = make_float4(nan, nan, nan, nan);
    if (y < H && x < W) v[j] = *(const float4*)(img + ((size_t)y * W + x) * ps + 4 * q);
  }
  const float gm = p.gate_min;
  int any = 0;
#pragma unroll
  for (int j = 0; j < NQ; ++j) any |= (v[j].x >= gm) | (v[j].y >= gm) | (v[j].z >= gm) | (v[j].w >= gm);
  const int hot = __any(any);
  if (lane == 0) marks[(size_t)b * cells + c] = hot ? 1 : 0;
}

void head_mark(const HeadMarkParams& p, hipStream_t s) {
  if (p.n_levels <= 0 || p.n_levels > kMarkMaxLevels || p.B <= 0 || p.n != 80)
    throw std::runtime_error("head_mark: 1..3 levels of 80 logits per pixel");
  long total = 0;
  for (int l = 0; l < p.n_levels; ++l) {
    if (p.logits[l] == nullptr || p.marks[l] == nullptr || p.H[l] <= 0 || p.W[l] <= 0 || p.ps[l] < p.n ||
        p.ps[l] % 4 != 0 || (uintptr_t)p.logits[l] % 16 != 0 || (uintptr_t)p.marks[l] % 4 != 0)
      throw std::runtime_error("head_mark: level " + std::to_string(l) + ": pointers, map size or pixel stride");
    total += (long)p.B * head_mark_cells(p.H[l]) * head_mark_cells(p.W[l]);
  }
  if (total > 0x7fffffffL - HM_WAVES) throw std::runtime_error("head_mark: too many cells");
  const unsigned grid = (unsigned)((total + HM_WAVES - 1) / HM_WAVES);
  hipLaunchKernelGGL((head_mark_kernel<20>), dim3(grid), dim3(HM_WAVES * 64), 0, s, p);
}

}  // namespace arena
