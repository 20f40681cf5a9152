// Split-K x3g second pass with the Detect head's 1x1 conv applied to the reduced tile ("x3g-sk-pw").
//
// A fused-1x1 record (3x3 stride 1 -> act -> 1x1, ConvParams.pw_*) ran on x3hg / x3hr / x3hc tiles only: one
// workgroup walks all 9 x Cin / 32 K chunks of its tile, and at batch 1 / 2 the Detect-head levels are 15-100 such
// workgroups on 256 CUs, so the op costs one workgroup's serial chain.  Here the 3x3 conv is the split-K first pass
// of gemm_x3.hip (XG_SK_VARIANTS row v: raw fp32 partial tiles ws[split][pixel][Cout_pad]), and this kernel is the
// second pass: for TP consecutive output pixels (linear over live_batch x Ho x Wo) and all pw_cout channels
//
//   pw_y = act2(W2 . act(sum_s ws[s] + bias) + pw_bias).
//
//   * Reduce: a lane owns (pixel, 4-channel) items and sums their partials in split order, adds the bias and applies
//     the activation in fp32: the arithmetic of x3g_sk_reduce_kernel, so the 3x3 value has the bits the unfused
//     split-K conv stores, whatever TP is.
//   * The activated value is split once into h / m / l bf16 planes (x3.h) and stored into LDS as pixel rows
//     [h K2 | m K2 | l K2] (K2 = pw_kpad), with the K columns in the order of the fused-1x1 weight blob
//     (halo_x3g.hip: column 16 ks + 8 h + i is channel 16 ks + 4 h + (i & 3) + 8 (i >> 2)); a lane's four channels
//     are four consecutive columns, one 8-byte store per plane.  Channels Cout .. K2 - 1 are stored as zeros.
//   * W2's pre-split planes (the blob as the planner packs it, rows [h | m | l] of K2 columns) are staged into LDS
//     once per workgroup by plain 16-byte copies; their loads are issued before the partial loads, so the
//     workgroup pays one memory latency for both.
//   * LDS rows are 6 K2 + 32 bytes (224 / 416 / 608): the 16-byte fragment reads of v_mfma_f32_16x16x32_bf16 (lane
//     l: row l & 15, columns 8 (l >> 4) .. + 7 of a 32-deep step) are conflict-free in every ds_read_b128 lane group
//     (tools/lds_bank_model.py's group table), for the pixel rows and the weight rows alike.
//   * Each wave owns 16 pixels: K2 / 32 steps x pw_cout / 16 channel fragments of the six-product chain of x3.h,
//     smallest first.  W2 is the MFMA's row operand and the pixels its columns, so a lane's accumulator holds four
//     consecutive channels of one pixel: the epilogue (pw_bias, pw_act) ends in one float4 store per fragment of the
//     pw_cout channels at stride pw_ys.
//
// Tile gate (ConvParams.gate): a workgroup whose TP pixels hold no logit >= gate_min among their first gate_n
// channels returns first and writes nothing.  The first pass applies the same rule to its BM-pixel linear tile; BM
// of every XG_SK_VARIANTS row is a multiple of 64 and tiles are aligned, so a second-pass tile that continues lies
// in a first-pass tile that continued.  Invariant: every pixel whose gate logits pass is written with exactly the
// ungated bits; other pixels may or may not be written (decode reads box values only at cells whose class logit
// passes).
#include <stdexcept>
#include <string>

#include "launch.h"
#include "x3.h"

namespace arena {

namespace {

constexpr int SP_GATE_MAX_N = 80;  // gating channels per pixel at most (ConvParams.gate_n): the Detect head's classes
constexpr int SP_MAX_C = 96;       // 3x3 channels (K of the 1x1) and 1x1 output channels at most
int g_sp_cus = 256;

__host__ __device__ constexpr int sp_pitch(int KS) { return 96 * KS + 16; }  // bf16 per LDS row: 3 planes x 32 KS + pad
// TP pixel rows and 16 weight rows per output-channel fragment
__host__ __device__ constexpr int sp_lds_bytes(int KS, int TP, int nf) { return (TP + 16 * nf) * sp_pitch(KS) * 2; }

}  // namespace

// KS: 32-deep K steps of the 1x1 (pw_kpad / 32); TP: pixels per workgroup, 16 per wave
template <int KS, int TP>
__global__ __launch_bounds__(TP * 4) void sk_pw_x3_kernel(const ConvParams p) {
  constexpr int NT = TP * 4, K2 = 32 * KS, P = sp_pitch(KS);
  constexpr int Q = K2 / 4;                              // 4-channel groups of a pixel row
  constexpr int VJ = TP * Q / NT;                        // (pixel, 4-channel) items per thread: 2 KS
  constexpr int RP = 12 * KS;                            // 16-byte pieces of a weight row (three planes of K2)
  constexpr int WI = (SP_MAX_C * RP + NT - 1) / NT;      // weight pieces per thread at most
  constexpr int NF = SP_MAX_C / 16;                      // output-channel fragments at most
  extern __shared__ __attribute__((aligned(16))) bf16 sp_lds[];
  bf16* sV = sp_lds;           // [TP][P] activated 3x3 values
  bf16* sW = sp_lds + TP * P;  // [16 nf][P] W2

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HWo = p.Ho * p.Wo;
  const int M = live_batch(p.B, p.bdev) * HWo, Mcap = p.B * HWo;
  const int m0 = (int)blockIdx.x * TP;
  if (m0 >= M) return;

  if (p.gate != nullptr) {
    constexpr int GJ = TP * (SP_GATE_MAX_N / 4) / NT;  // float4 items per thread at most
    const int nq = p.gate_n >> 2;  // host: gate_n % 4 == 0, 0 < gate_n <= SP_GATE_MAX_N
    const int items = (M - m0 < TP ? M - m0 : TP) * nq;
    const float gm = p.gate_min;
    const float nan = __builtin_nanf("");  // an item outside the tile passes nothing
    float4 gv[GJ];
#pragma unroll
    for (int j = 0; j < GJ; ++j) {  // all loads first, then the compares
      const int i = tid + NT * j;
      const int px = i / nq, q = i - px * nq;
      gv[j] = make_float4(nan, nan, nan, nan);
      if (i < items) gv[j] = *(const float4*)(p.gate + (size_t)(m0 + px) * p.pw_ys + 4 * q);
    }
    int any = 0;
#pragma unroll
    for (int j = 0; j < GJ; ++j) any |= gv[j].x >= gm || gv[j].y >= gm || gv[j].z >= gm || gv[j].w >= gm;
    if (!__syncthreads_or(any)) return;
  }

  // ---- W2: the blob's rows are the LDS rows without the pad, so piece i of the blob is piece i % RP of row i / RP
  const int nf = (p.pw_cout + 15) >> 4;
  const int wpieces = 16 * nf * RP;  // <= the blob's round32(pw_cout) rows
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.pw_w), (short)0, ((p.pw_cout + 31) & ~31) * RP * 16, 0x00020000);
  constexpr int kOob = 0x7fffffff & ~15;  // past the buffer: the load returns zeros
  u32x4 rw[WI];
#pragma unroll
  for (int j = 0; j < WI; ++j) {
    const int i = tid + NT * j;
    rw[j] = __builtin_amdgcn_raw_buffer_load_b128(wr, i < wpieces ? i * 16 : kOob, 0, 0);
  }

  // ---- reduce: this thread's items, summed in split order.  An item past the live pixels or the 3x3 channels
  // reads a valid address (its value is replaced by zero below).
  const size_t sstride = (size_t)Mcap * p.Cout_pad;
  const float* src[VJ];
  bool ok[VJ];
  int ch[VJ];
#pragma unroll
  for (int j = 0; j < VJ; ++j) {
    const int i = tid + NT * j;
    const int px = i / Q;
    ch[j] = 4 * (i - px * Q);
    ok[j] = m0 + px < M && ch[j] < p.Cout;
    src[j] = p.sk_ws + (size_t)(ok[j] ? m0 + px : m0) * p.Cout_pad + (ok[j] ? ch[j] : 0);
  }
  float4 a[VJ];
#pragma unroll
  for (int j = 0; j < VJ; ++j) a[j] = *(const float4*)src[j];
#pragma unroll 4
  for (int k = 1; k < p.sk_splits; ++k) {
    float4 v[VJ];
#pragma unroll
    for (int j = 0; j < VJ; ++j) v[j] = *(const float4*)(src[j] + k * sstride);
#pragma unroll
    for (int j = 0; j < VJ; ++j) {
      a[j].x += v[j].x; a[j].y += v[j].y; a[j].z += v[j].z; a[j].w += v[j].w;
    }
  }

  // ---- bias, activation, split, into the pixel rows at the blob's K columns
#pragma unroll
  for (int j = 0; j < VJ; ++j) {
    const int i = tid + NT * j;
    const int px = i / Q, c = ch[j];
    const float4 bias = *(const float4*)(p.bias + (ok[j] ? c : 0));
    const float v0 = ok[j] ? apply_act(a[j].x + bias.x, p.act) : 0.f;
    const float v1 = ok[j] ? apply_act(a[j].y + bias.y, p.act) : 0.f;
    const float v2 = ok[j] ? apply_act(a[j].z + bias.z, p.act) : 0.f;
    const float v3 = ok[j] ? apply_act(a[j].w + bias.w, p.act) : 0.f;
    bf16x4 h, m, l;
    x3_split4_pair(f32x2{v0, v1}, f32x2{v2, v3}, h, m, l);
    const int r = c & 15;
    bf16* d = sV + px * P + (c & ~15) + 8 * ((r >> 2) & 1) + 4 * (r >> 3);
    *(bf16x4*)d = h;
    *(bf16x4*)(d + K2) = m;
    *(bf16x4*)(d + 2 * K2) = l;
  }
#pragma unroll
  for (int j = 0; j < WI; ++j) {
    const int i = tid + NT * j;
    if (i < wpieces) {
      const int row = i / RP, part = i - row * RP;
      *(u32x4*)(sW + row * P + part * 8) = rw[j];
    }
  }
  __syncthreads();

  // ---- 1x1: wave's 16 pixels x 16 nf channels
  const int fr = lane & 15, fq = lane >> 4;
  bf16x8 vh[KS], vm[KS], vl[KS];
  {
    const bf16* r = sV + (wave * 16 + fr) * P + 8 * fq;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      vh[kk] = *(const bf16x8*)(r + 32 * kk);
      vm[kk] = *(const bf16x8*)(r + K2 + 32 * kk);
      vl[kk] = *(const bf16x8*)(r + 2 * K2 + 32 * kk);
    }
  }
  const int m = m0 + wave * 16 + fr;
  float* yrow = (float*)p.pw_y + (size_t)m * p.pw_ys;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    if (f >= nf) break;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const bf16* r = sW + (16 * f + fr) * P + 8 * fq;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const bf16x8 wh = *(const bf16x8*)(r + 32 * kk), wmid = *(const bf16x8*)(r + K2 + 32 * kk),
                   wl = *(const bf16x8*)(r + 2 * K2 + 32 * kk);
      acc = x3_mfma(wh, wmid, wl, vh[kk], vm[kk], vl[kk], acc);
    }
    const int c = 16 * f + 4 * fq;  // accumulator lane: pixel fr, channels c .. c + 3
    if (m < M && c < p.pw_cout) {
      const float4 bias = *(const float4*)(p.pw_bias + c);
      *(float4*)(yrow + c) = make_float4(apply_act(acc[0] + bias.x, p.pw_act), apply_act(acc[1] + bias.y, p.pw_act),
                                         apply_act(acc[2] + bias.z, p.pw_act), apply_act(acc[3] + bias.w, p.pw_act));
    }
  }
}

namespace {

template <int KS, int TP>
void sp_launch(const ConvParams& p, hipStream_t s) {
  const long M = (long)p.B * p.Ho * p.Wo;
  hipLaunchKernelGGL((sk_pw_x3_kernel<KS, TP>), dim3((unsigned)((M + TP - 1) / TP)), dim3(TP * 4),
                     sp_lds_bytes(KS, TP, (p.pw_cout + 15) / 16), s, p);
}

template <int KS>
void sp_launch_ks(const ConvParams& p, hipStream_t s) {
  // 64-pixel tiles where they fill the device, 32-pixel tiles (two waves) below that; same bits either way
  const long M = (long)p.B * p.Ho * p.Wo;
  if ((M + 63) / 64 >= g_sp_cus)
    sp_launch<KS, 64>(p, s);
  else
    sp_launch<KS, 32>(p, s);
}

template <int KS, int TP>
void sp_prepare() {
  ARENA_HIP_CHECK(hipFuncSetAttribute((const void*)sk_pw_x3_kernel<KS, TP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      sp_lds_bytes(KS, TP, SP_MAX_C / 16)));
}

}  // namespace

void conv_x3g_sk_pw(const ConvParams& p, hipStream_t s, int v) {
  auto no = [](const std::string& what) {
    throw std::runtime_error("conv2d_f32: split-K x3g with a fused 1x1 (impl 171 + v, pw) " + what);
  };
  if (p.KH != 3 || p.KW != 3 || p.stride != 1 || p.pad_t != 1 || p.pad_l != 1 || p.w3 == nullptr)
    no("takes a 3x3 stride-1 pad-1 conv with pre-split weights");
  if (p.res != nullptr || p.y2 != nullptr) no("takes no res / y2");
  if (p.n_lo != 0 || p.n_hi != 0 || p.marks != nullptr) no("takes no output-channel window and no marks");
  if (p.x_planes != 0 || p.y3 != nullptr) no("takes no x3 planes");
  if (p.Cout != p.Cout_pad || p.Cout > SP_MAX_C) no("needs Cout == Cout_pad <= 96");
  if (p.pw_cout <= 0 || p.pw_cout > SP_MAX_C || p.pw_cout % 4 != 0) no("needs pw_cout <= 96, a multiple of 4");
  if (p.pw_kpad % 32 != 0 || p.pw_kpad < p.Cout || p.pw_kpad > SP_MAX_C) no("needs pw_kpad = Cout rounded up to 32");
  if (p.pw_y == nullptr || p.pw_ys % 4 != 0 || (uintptr_t)p.pw_y % 16 != 0) no("needs a 16-byte aligned pw_y, pw_ys % 4");
  if (p.gate != nullptr && !(p.gate_n > 0 && p.gate_n <= SP_GATE_MAX_N && p.gate_n % 4 == 0 && p.gate_n <= p.pw_ys &&
                             (uintptr_t)p.gate % 16 == 0))
    no("needs gate_n a multiple of 4, <= 80, and 16-byte aligned gate logits");
  if (v < 0 || v >= kF32X3GSKVariants) no("names no variant");
  const int splits = x3g_sk_pass1(p, s, v);
  if (splits == 0) {  // the workspace cannot hold the partial tiles: the fused variant impl 0 picks
    if (!conv_x3hg_pw(p, s, x3hg_pw_variant(0, p.Cout_pad))) throw std::runtime_error(f32_family(F32Family::X3HGPw).reject);
    return;
  }
  ConvParams q = p;
  q.sk_splits = splits;
  switch (p.pw_kpad / 32) {
    case 1: sp_launch_ks<1>(q, s); break;
    case 2: sp_launch_ks<2>(q, s); break;
    default: sp_launch_ks<3>(q, s); break;
  }
}

void x3g_sk_pw_prepare() {
  sp_prepare<1, 32>();
  sp_prepare<1, 64>();
  sp_prepare<2, 32>();
  sp_prepare<2, 64>();
  sp_prepare<3, 32>();
  sp_prepare<3, 64>();
  int dev = 0, cus = 0;
  ARENA_HIP_CHECK(hipGetDevice(&dev));
  ARENA_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  if (cus > 0) g_sp_cus = cus;
}

}  // namespace arena
