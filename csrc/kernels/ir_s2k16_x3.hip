// Fused MobileNetV2 inverted residual, fp32-accurate on the bf16 matrix cores, for the stride-2 expanding block
// with a 16-channel input (torchvision mobilenet_v2 features[2]: 112x112x16 -> 56x56x24, hidden 96).  It takes
// the geometry and the operands of ir_f32_kernel<2, 4, 8, 2, true, 1> (ir_f32.hip): fp32 we [hid_pad][16],
// wd [9][hid_pad], wp [32][hid_pad], fp32 biases, IrParams.x3w == 0; one workgroup = a 4 x 8 output tile of one
// crop (9 x 17 input halo, 10 pixel tiles of 16).
//
// Structure and LDS layout are those of ir_tile_x3_kernel<2, 4, 8, ..> (ir_tile_x3.hip): per chunk of 32 hidden
// channels, expand GEMM -> fp32 E tile in LDS -> depthwise (v_pk_fma_f32, one output pixel per thread) -> split D
// planes in LDS -> project GEMM into register accumulators.  Three differences:
//
//   * K-packed expand.  With K = 16 a 32-deep x3 step would be half zero padding.  Instead the six products of the
//     triple-bf16 split pair up along K: with A = [p | q] and B = [r | s] (16-wide halves) one
//     v_mfma_f32_16x16x32_bf16 yields p.r + q.s, so
//         [am | al].[bm | bh],  [ah | am].[bl | bh],  [ah | ah].[bm | bh]
//     are the six terms of x3_mfma (x3.h), smallest first, in three MFMAs.  A lane's 8-element fragment covers k = 8 kq
//     .. + 7 of the 32, so the packing is only a choice of plane per lane: lanes kq < 2 take the first plane of each
//     pair, lanes kq >= 2 the second, both for channels 8 (kq & 1) .. + 7.
//   * The input halo is loaded and split once per workgroup, into bf16 planes in the LDS region that later holds E;
//     the waves then keep the B fragments of their pixel tiles in registers for all chunks.  (With every wave
//     loading and splitting its own pixels, each value four times per workgroup, the prologue was as long as the
//     three chunks together.)
//   * fp32 weights.  The plan keeps this block's weights unsplit (x3w == 0), so every lane splits the weight
//     fragments it feeds to the MFMAs itself, once per chunk, from a prefetch issued in the chunk before.
//
// 124 VGPRs, no scratch, 34 KB of LDS at hidden 96: four workgroups per CU (ir_f32_kernel: three).  Block 2 per
// batch of 32 requests 201.2 -> 146.3 us, at batch 1 11.0 -> 9.8 us; SQ_INSTS_MFMA 4.73e6 -> 3.54e6, MFMA busy
// 31 -> 16 %, SQ_INSTS_VALU 4.08e7 -> 5.21e7 (the splits) (profiles/r9_s2k16).
#include <cstdlib>
#include <stdexcept>

#include "ir_tile_x3.h"
#include "launch.h"

namespace arena {

namespace {

constexpr int ISK_TH = 4, ISK_TW = 8;                           // output tile
constexpr int ISK_PH = (ISK_TH - 1) * 2 + 3, ISK_PW = (ISK_TW - 1) * 2 + 3;
constexpr int ISK_PIN = ISK_PH * ISK_PW, ISK_MT_IN = (ISK_PIN + 15) / 16, ISK_ROWS = ISK_MT_IN * 16;
constexpr int ISK_POUT = ISK_TH * ISK_TW;
constexpr int ISK_ET = (ISK_MT_IN * 2 + 3) / 4;                 // expand tiles per wave (pixel tile x hidden half)
constexpr int ISK_EP = itx_ep(2);
static_assert(ISK_POUT == 32, "one depthwise pass of 32 pixels, two project pixel tiles");

__device__ __forceinline__ bf16x8 isk_sel(bool second, const bf16x8& a, const bf16x8& b) { return second ? b : a; }

}  // namespace

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void ir_s2k16_x3_kernel(const IrParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t isk_lds[];
  float* Es = (float*)isk_lds;                                  // [ROWS][EP] fp32
  uint8_t* Ds = isk_lds + ISK_ROWS * ISK_EP * sizeof(float);    // [POUT][ITX_DPB] bf16 planes
  float* Wd = (float*)(Ds + ISK_POUT * ITX_DPB);                // [10][hid_pad]: depthwise taps 0..8, bias

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: what derives from it stays scalar
  const int col = lane & 15, kq = lane >> 4;
  const bool second = kq >= 2;  // this lane's half of the packed K
  const int kc = 8 * (kq & 1);  // and its input channels kc .. kc + 7
  const int tiles_x = (p.Wo + ISK_TW - 1) / ISK_TW, tiles_y = (p.Ho + ISK_TH - 1) / ISK_TH;
  const int tiles = tiles_x * tiles_y;
  const int b = blockIdx.x / tiles;
  if (b >= live_batch(p.B, p.bdev)) return;
  const int t = blockIdx.x - b * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int oy0 = ty * ISK_TH, ox0 = tx * ISK_TW;
  const int iy0 = oy0 * 2 - 1, ix0 = ox0 * 2 - 1;
  const float* xb = (const float*)p.x + (size_t)b * p.H * p.W * p.x_cs;
  const float* we = (const float*)p.we;
  const float* wp = (const float*)p.wp;
  const float* wd = (const float*)p.wd;
  const int hid_pad = p.hid_pad;

  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};  // one project pair per wave: pixel tile wave >> 1, channel tile wave & 1

  // fp32 weight fragments of chunk c + 1 are fetched while chunk c runs (expand: A operand, hidden row h0 +
  // 16 nt_e + col, input channels kc .. + 7; project: A operand, output row 16 nt_p + col, hidden k h0 + 8 kq
  // .. + 7) and split at the head of their chunk.  The prefetch is unconditional (the last chunk re-fetches
  // itself), as in ir_tile_x3_kernel.  The depthwise taps and bias of every chunk are staged in LDS once.
  const int nt_e = wave & 1, nt_p = wave & 1, mt_p = wave >> 1;
  float4 wef[2], wpf[2], bexp;
  auto load_weights = [&](int h0) {
    const float* er = we + (size_t)(h0 + nt_e * 16 + col) * 16 + kc;
    wef[0] = *(const float4*)er;
    wef[1] = *(const float4*)(er + 4);
    const float* pr = wp + (size_t)(nt_p * 16 + col) * hid_pad + h0 + 8 * kq;
    wpf[0] = *(const float4*)pr;
    wpf[1] = *(const float4*)(pr + 4);
    bexp = *(const float4*)((const float*)p.be + h0 + nt_e * 16 + 4 * kq);
  };
  load_weights(0);
  for (int r = tid >> 5; r < 10; r += 8) {  // 32 threads per row of Wd
    const float* src = r < 9 ? wd + (size_t)r * hid_pad : (const float*)p.bd;
    for (int c = 4 * (tid & 31); c < hid_pad; c += 128) *(float4*)&Wd[r * hid_pad + c] = *(const float4*)(src + c);
  }

  // ---- X: the halo pixels' 16 channels, loaded and split once per workgroup (item = pixel x 8-channel group)
  // into bf16 planes in LDS, in the E region, which is free until the first expand.  A pixel row is [h|m|l][16]
  // bf16, then its inside flag: 112 B = 7 slots of 16 B, so 16 consecutive pixels start in 16 different slots.
  constexpr int XPB = 112;
  static_assert(ISK_ROWS * XPB <= ISK_ROWS * ISK_EP * (int)sizeof(float), "the X planes fit the E region");
  uint8_t* Xs = isk_lds;
  for (int it = tid; it < ISK_ROWS * 2; it += 256) {
    const int r = it >> 1, c0 = 8 * (it & 1);
    const int iy = iy0 + r / ISK_PW, ix = ix0 + r % ISK_PW;
    const bool in = r < ISK_PIN && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    const float* src = xb + ((size_t)(in ? iy : 0) * p.W + (in ? ix : 0)) * p.x_cs;
    // channels past inp are padding (inp % 4 == 0): zero, and never read (they may lie past the tensor)
    const bool lo = in && c0 < p.inp, up = in && c0 + 4 < p.inp;
    const float4 a = *(const float4*)(src + (lo ? c0 : 0)), c = *(const float4*)(src + (up ? c0 + 4 : 0));
    float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (j < 4 ? lo : up) ? v[j] : 0.f;
    bf16x8 h, m, l;
    x3_split8_pair(v, h, m, l);
    uint8_t* d = Xs + r * XPB + 2 * c0;
    *(bf16x8*)d = h;
    *(bf16x8*)(d + 32) = m;
    *(bf16x8*)(d + 64) = l;
    if (c0 == 0) *(unsigned*)(d + 96) = in ? 1u : 0u;
  }
  __syncthreads();

  // ---- this wave's expand tiles: tile tt = wave + 4 i covers halo pixels 16 (tt >> 1) .. + 15 and hidden half
  // tt & 1 = wave & 1.  The lane keeps the two B fragments of the packed products of its pixel ([bm | bh] serves
  // the first and the third MFMA, [bl | bh] the second) in registers for all chunks.
  static_assert(ISK_ET * 4 == ISK_MT_IN * 2, "every wave runs ISK_ET expand tiles");
  bf16x8 xb1[ISK_ET], xb2[ISK_ET];
  unsigned xin = 0;  // bit i: the lane's halo pixel of tile i is inside the image (the expanded map is zero-padded)
#pragma unroll
  for (int i = 0; i < ISK_ET; ++i) {
    const int tt = wave + 4 * i;
    const uint8_t* sx = Xs + ((tt >> 1) * 16 + col) * XPB;
    xb1[i] = *(const bf16x8*)(sx + 2 * kc + (second ? 0 : 32));
    xb2[i] = *(const bf16x8*)(sx + 2 * kc + (second ? 0 : 64));
    xin |= *(const unsigned*)(sx + 96) << i;
  }
  __syncthreads();  // every wave holds its fragments: the region becomes E

  const int g = tid & 7;  // depthwise channel group (4 channels) of this thread
  // The depthwise reads do not depend on the chunk, and the stride-2 E layout has no swizzle: one address (the
  // window's first pixel), the nine taps at constant offsets from it
  static_assert(itx_ep(2) != ITX_HC, "the unswizzled stride-2 E pitch");
  const int q = tid >> 3;
  const float* etap = Es + (((q / ISK_TW) * 2) * ISK_PW + (q % ISK_TW) * 2) * ISK_EP + 4 * g;

  for (int h0 = 0; h0 < hid_pad; h0 += ITX_HC) {
    const int hn = h0 + ITX_HC < hid_pad ? h0 + ITX_HC : h0;
    // ---- this chunk's weight fragments as bf16 planes; then the next chunk's fetch
    bf16x8 a1, a2, a3, ph, pm, pl;
    {
      const float ev[8] = {wef[0].x, wef[0].y, wef[0].z, wef[0].w, wef[1].x, wef[1].y, wef[1].z, wef[1].w};
      bf16x8 h, m, l;
      x3_split8_pair(ev, h, m, l);
      a1 = isk_sel(second, m, l);  // [am | al]
      a2 = isk_sel(second, h, m);  // [ah | am]
      a3 = h;                      // [ah | ah]
      const float pv[8] = {wpf[0].x, wpf[0].y, wpf[0].z, wpf[0].w, wpf[1].x, wpf[1].y, wpf[1].z, wpf[1].w};
      x3_split8_pair(pv, ph, pm, pl);
    }
    const float4 be = bexp;

    // ---- expand: E = relu6(We . X + be) * inside, fp32 into LDS; three K-packed MFMAs per tile
#pragma unroll
    for (int i = 0; i < ISK_ET; ++i) {
      const int tt = wave + 4 * i;
      f32x4 e = f32x4{0.f, 0.f, 0.f, 0.f};
      e = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, xb1[i], e, 0, 0, 0);  // am.bm + al.bh
      e = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, xb2[i], e, 0, 0, 0);  // ah.bl + am.bh
      e = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, xb1[i], e, 0, 0, 0);  // ah.bm + ah.bh
      // the lane holds hidden channels hc .. hc + 3 of pixel `pix` (16x16 output layout); its own inside flag
      // belongs to the same pixel
      const int pix = (tt >> 1) * 16 + col;
      const int hc = nt_e * 16 + 4 * kq;
      const float m = (xin >> i) & 1u ? 1.f : 0.f;
      const float4 v = make_float4(relu6f(e[0] + be.x) * m, relu6f(e[1] + be.y) * m, relu6f(e[2] + be.z) * m,
                                   relu6f(e[3] + be.w) * m);
      *(float4*)&Es[pix * ISK_EP + hc] = v;
    }
    __syncthreads();

    // ---- depthwise 3x3 stride 2 + bias + ReLU6 -> split planes of D; one output pixel per thread, all nine
    // taps' LDS reads issued before the FMAs (tap order of ir_f32.hip: bias, tap 0, .. tap 8)
    {
      float4 wk[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) wk[k] = *(const float4*)&Wd[k * hid_pad + h0 + 4 * g];
      const float4 bdw = *(const float4*)&Wd[9 * hid_pad + h0 + 4 * g];
      float4 v[9];
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) v[tp] = *(const float4*)(etap + ((tp / 3) * ISK_PW + tp % 3) * ISK_EP);
      ItxDw dw(bdw);
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) dw.tap(v[tp], wk[tp]);
      dw.store(Ds + q * ITX_DPB + 8 * g);
    }
    load_weights(hn);
    __syncthreads();

    // ---- project GEMM accumulate (rows = output channels, columns = output pixels), six products over K = 32
    {
      const uint8_t* d = Ds + (mt_p * 16 + col) * ITX_DPB + 16 * kq;
      acc = x3_mfma(ph, pm, pl, *(const bf16x8*)d, *(const bf16x8*)(d + 64), *(const bf16x8*)(d + 128), acc);
    }
    // no barrier here: the next chunk's expand writes E, which every wave finished reading before the barrier
    // above, and its depthwise writes D only after the next expand barrier, which every wave reaches after
    // this project
  }

  // ---- epilogue: + bias -> NHWC fp32
  float* yb = (float*)p.y + (size_t)b * p.Ho * p.Wo * p.y_cs;
  const int qo = mt_p * 16 + col;
  const int oy = oy0 + qo / ISK_TW, ox = ox0 + qo % ISK_TW;
  const int co = nt_p * 16 + 4 * kq;
  if (oy >= p.Ho || ox >= p.Wo || co >= p.oup) return;
  const float4 bp = *(const float4*)((const float*)p.bp + co);
  *(float4*)(yb + ((size_t)oy * p.Wo + ox) * p.y_cs + co) =
      make_float4(acc[0] + bp.x, acc[1] + bp.y, acc[2] + bp.z, acc[3] + bp.w);
}

static bool g_ir_s2k16 = [] {
  const char* e = std::getenv("ARENA_IR_S2K16");
  return e ? std::atoi(e) != 0 : true;
}();
void set_ir_s2k16(bool v) { g_ir_s2k16 = v; }

// The geometry of ir_f32_kernel<2, 4, 8, 2, true, 1>; the caller (ir_block_f32) has checked the channel
// alignment and the output size.
bool ir_s2k16_x3(const IrParams& p, hipStream_t s) {
  if (!g_ir_s2k16 || p.x3w || p.stem || p.stride != 2 || !p.expand || p.res || p.inp_pad != 16 ||
      p.hid_pad % ITX_HC || p.hid_pad <= 0 || p.oup_pad != 32)
    return false;
  const size_t lds = (size_t)ISK_ROWS * ISK_EP * 4 + (size_t)ISK_POUT * ITX_DPB + (size_t)10 * p.hid_pad * 4;
  if (lds > 64 * 1024) return false;
  const int tiles = ((p.Wo + ISK_TW - 1) / ISK_TW) * ((p.Ho + ISK_TH - 1) / ISK_TH);
  hipLaunchKernelGGL(ir_s2k16_x3_kernel, dim3((unsigned)(p.B * tiles)), dim3(256), lds, s, p);
  return true;
}

}  // namespace arena
