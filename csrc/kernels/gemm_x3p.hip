// x3gp: the x3g implicit GEMM (gemm_x3.hip) over activations kept as pre-split bf16 planes ("x3 planes").
//
// conv_x3g_kernel splits every activation element into its three bf16 planes while it stages it (x3_split8, about
// 40 VALU per 8 values), once per workgroup that stages the element: a 3x3 conv splits each element 9 taps x
// ceil(Cout_pad / BN) times.  Here the producer of an activation stores the planes once and every consumer loads
// matrix operands directly.
//
// The layout: an NHWC map with C % 32 == 0 is [B][H][W][C / 32] chunks of 192 bytes, each [h 32 | m 32 | l 32] bf16:
// the planes of x3.h's split for 32 consecutive channels.  That is the row format of ConvParams.w3
// (engine/planner.py pack_conv_weight_x3), so a staged activation row in LDS is the image conv_x3g_kernel builds
// (XG_PITCH rows, planes at +0 / +32 / +64), and all-zero planes are the split of 0.0f: an out-of-range buffer load
// (padding, pixels past the live batch) stays correct.
//
//   * PIN: x is planes.  Staging a pixel row is a plain copy of 12 16-byte pieces, the path of the weights, with no
//     split VALU.  A thread's pieces are `NT` apart in (row, piece) order, so a wave reads 1 KiB runs of consecutive
//     chunks of consecutive pixels (a 1x1 conv over 32 channels reads its whole input as one run).
//     Without PIN x is fp32 and is split while staging, exactly as x3g does: that is how a chain is entered.
//   * POUT: after bias, activation and the fp32 residual, the value y receives is split with the pair form of x3.h
//     (the bits of x3_split8: csrc/tests/x3_split_check.cpp) and stored to y3 as one 8-byte piece per plane per g
//     (accumulator lane l holds channels 8g + 4(l >> 5) + 0..3 of pixel l & 31).  y is stored as well when non-null.
//   * The tiles, the K order (taps row-major, 32-channel chunks ascending, the two 16-deep steps ascending), the
//     v_mfma_f32_32x32x16_bf16 k-to-lane map and the six-product chain are x3g's: the fp32 output has x3g's bits.
//
// Pipeline: two LDS stages (one barrier per 32-deep chunk) and two register sets, so chunk kc + 2's loads are issued
// before chunk kc's MFMAs and land in LDS after chunk kc + 1's.  With PIN a set is at most 6 + 6 16-byte pieces a
// thread (48 VGPRs), about x3g's own 16 + 24 plus its split temporaries, so the depth stays at two sets; there is
// no split to interleave, so the kernel has no sched_group_barrier shaping (x3g's IL twins map to the same tile).
#include <stdexcept>
#include <string>

#include "launch.h"
#include "x3.h"

namespace arena {

namespace {

constexpr int XP_PITCH = 104;  // bf16 per LDS row, as XG_PITCH: 3 planes x 32 k + 8 pad (208 B = 13 slots, odd)

__host__ __device__ constexpr int xp_lds_bytes(int BM, int BN) { return 2 * (BM + BN) * XP_PITCH * 2; }

}  // namespace

template <int WM, int WN, int TM, int TN, bool PIN, bool POUT>
__global__ __launch_bounds__(WM * WN * 64) void conv_x3gp_kernel(const ConvParams p) {
  constexpr int NT = WM * WN * 64;  // 4 or 8 waves
  static_assert(WM * WN == 4 || WM * WN == 8, "four or eight waves");
  static_assert(PIN || POUT, "fp32 in, fp32 out is conv_x3g_kernel");
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  // activation items per thread: PIN 16-byte pieces (12 per row), else (row, 8-k group) items of two float4
  constexpr int AI = PIN ? BM * 12 / NT : BM * 4 / NT;
  constexpr int AR = PIN ? 1 : 2;                // 16-byte registers per item
  constexpr int WI = (BN * 12 + NT - 1) / NT;  // 16-B weight pieces per thread
  static_assert(BM * 12 % NT == 0 && BM * 4 % NT == 0, "every thread stages the same number of activation items");
  extern __shared__ __attribute__((aligned(16))) bf16 xp_lds[];
  bf16* sA = xp_lds;                     // [2][BM][XP_PITCH] activations
  bf16* sB = xp_lds + 2 * BM * XP_PITCH;  // [2][BN][XP_PITCH] weights

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int HWo = p.Ho * p.Wo;
  const int M = live_batch(p.B, p.bdev) * HWo;
  const int ntn = (p.Cout_pad + BN - 1) / BN;
  const int bx = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int mt = bx / ntn, nt = bx - mt * ntn;
  const int m0 = mt * BM, n0 = nt * BN;
  if (m0 >= M) return;

  // Raw buffer loads: an out-of-range offset (conv padding, pixels past the live batch, channels past Cin of an fp32
  // input) returns zeros; offsets are 32-bit (launcher: every tensor < 2 GiB).
  const int Cin32 = (p.Cin + 31) & ~31;
  const int cpp = Cin32 >> 5;                            // 32-channel chunks per pixel and per tap
  const int xpix = PIN ? cpp * 192 : p.xs * 4;           // bytes from a pixel to the next
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.x), (short)0, (int)((size_t)p.B * p.H * p.W * xpix), 0x00020000);
  const int nk = p.KH * p.KW * cpp;
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.w3), (short)0, (int)((size_t)nk * p.Cout_pad * 192), 0x00020000);
  const int Cin = p.Cin, H = p.H, W = p.W, S = p.stride;
  constexpr int kOob = 0x7fffffff & ~15;  // past every buffer: the load returns zeros

  // per staged item: the input pixel of tap (0, 0) and the item's byte offset there, fixed over the K loop
  int a_iy[AI], a_ix[AI], a_off[AI];
#pragma unroll
  for (int j = 0; j < AI; ++j) {
    const int i = tid + NT * j;
    const int row = PIN ? i / 12 : i >> 2;
    const int sub = PIN ? (i - row * 12) * 16 : (i & 3) * 32;  // byte offset of the item within its chunk
    const int m = m0 + row;
    if (m < M) {
      const int b = m / HWo, r = m - b * HWo;
      const int oy = r / p.Wo, ox = r - oy * p.Wo;
      a_iy[j] = oy * S - p.pad_t;
      a_ix[j] = ox * S - p.pad_l;
      a_off[j] = ((b * H + a_iy[j]) * W + a_ix[j]) * xpix + sub;
    } else {
      a_iy[j] = -0x40000000;  // never inside the map
      a_ix[j] = 0;
      a_off[j] = 0;
    }
  }
  int w_off[WI];  // byte offset of this thread's 16-B weight pieces within a chunk
#pragma unroll
  for (int j = 0; j < WI; ++j) {
    const int i = tid + NT * j;
    const int row = i / 12, part = i - (i / 12) * 12;
    w_off[j] = i < BN * 12 ? ((n0 + row) * 96 + part * 8) * 2 : kOob;
  }

  u32x4 ra0[AI][AR], ra1[AI][AR];
  u32x4 rw0[WI], rw1[WI];
  // (ky, kx, c0) of the next chunk to load: chunks are loaded strictly in order (a chunk never straddles two taps)
  int ld_ky = 0, ld_kx = 0, ld_c0 = 0;
  auto load = [&](int kc, u32x4 (&ra)[AI][AR], u32x4 (&rw)[WI]) {
    const int ky = ld_ky, kx = ld_kx, c0 = ld_c0;
    ld_c0 += 32;  // advanced with selects, not branches: the K step stays one scheduling region
    const bool wrap = ld_c0 >= Cin32;
    ld_c0 = wrap ? 0 : ld_c0;
    ld_kx += wrap ? 1 : 0;
    const bool wrap2 = ld_kx == p.KW;
    ld_kx = wrap2 ? 0 : ld_kx;
    ld_ky += wrap2 ? 1 : 0;
    const int step = (ky * W + kx) * xpix + (PIN ? (c0 >> 5) * 192 : c0 * 4);  // uniform
#pragma unroll
    for (int j = 0; j < AI; ++j) {
      const bool in = (unsigned)(a_iy[j] + ky) < (unsigned)H && (unsigned)(a_ix[j] + kx) < (unsigned)W;
      if constexpr (PIN) {
        ra[j][0] = __builtin_amdgcn_raw_buffer_load_b128(xr, in ? a_off[j] + step : kOob, 0, 0);
      } else {
        const int c = c0 + 8 * ((tid + NT * j) & 3);
        ra[j][0] = __builtin_amdgcn_raw_buffer_load_b128(xr, in && c < Cin ? a_off[j] + step : kOob, 0, 0);
        ra[j][1] = __builtin_amdgcn_raw_buffer_load_b128(xr, in && c + 4 < Cin ? a_off[j] + step + 16 : kOob, 0, 0);
      }
    }
    const int wstep = kc * p.Cout_pad * 192;  // uniform: chunk kc's rows
#pragma unroll
    for (int j = 0; j < WI; ++j) rw[j] = __builtin_amdgcn_raw_buffer_load_b128(wr, w_off[j], wstep, 0);
  };
  auto store = [&](int buf, const u32x4 (&ra)[AI][AR], const u32x4 (&rw)[WI]) {
    bf16* a = sA + buf * BM * XP_PITCH;
    bf16* bw = sB + buf * BN * XP_PITCH;
#pragma unroll
    for (int j = 0; j < AI; ++j) {
      const int i = tid + NT * j;
      if constexpr (PIN) {
        const int row = i / 12, part = i - (i / 12) * 12;
        *(u32x4*)(a + row * XP_PITCH + part * 8) = ra[j][0];
      } else {
        const f32x4 v0 = __builtin_bit_cast(f32x4, ra[j][0]), v1 = __builtin_bit_cast(f32x4, ra[j][AR - 1]);
        const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        bf16x8 h, m, l;
        x3_split8(v, h, m, l);
        bf16* d = a + (i >> 2) * XP_PITCH + 8 * (i & 3);
        *(bf16x8*)d = h;
        *(bf16x8*)(d + 32) = m;
        *(bf16x8*)(d + 64) = l;
      }
    }
#pragma unroll
    for (int j = 0; j < WI; ++j) {
      const int i = tid + NT * j;
      if (BN * 12 % NT == 0 || i < BN * 12) {
        const int row = i / 12, part = i - (i / 12) * 12;
        *(u32x4*)(bw + row * XP_PITCH + part * 8) = rw[j];
      }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int fr = lane & 31, fk = 8 * (lane >> 5);
  auto compute = [&](int buf) {
    const bf16* a = sA + buf * BM * XP_PITCH;
    const bf16* bw = sB + buf * BN * XP_PITCH;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 wh[TN], wmid[TN], wl[TN];
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        const bf16* r = bw + ((wn * TN + tn) * 32 + fr) * XP_PITCH + ks * 16 + fk;
        wh[tn] = *(const bf16x8*)r;
        wmid[tn] = *(const bf16x8*)(r + 32);
        wl[tn] = *(const bf16x8*)(r + 64);
      }
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        const bf16* r = a + ((wm * TM + tm) * 32 + fr) * XP_PITCH + ks * 16 + fk;
        const bf16x8 xh = *(const bf16x8*)r, xm = *(const bf16x8*)(r + 32), xl = *(const bf16x8*)(r + 64);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = x3_mfma(wh[tn], wmid[tn], wl[tn], xh, xm, xl, acc[tm][tn]);
      }
    }
  };

  load(0, ra0, rw0);
  if (nk > 1) load(1, ra1, rw1);
  store(0, ra0, rw0);
  __syncthreads();
  int kc = 0;
  // Branch-free body: loads past the last chunk read zeros (the weight offset leaves its buffer; the activation
  // bytes they fetch are never used) and the stage they are stored into is not read again.
  for (; kc + 1 < nk; kc += 2) {  // chunk kc in stage 0, kc + 1 in register set 1
    load(kc + 2, ra0, rw0);
    compute(0);
    store(1, ra1, rw1);
    __syncthreads();
    load(kc + 3, ra1, rw1);
    compute(1);
    store(0, ra0, rw0);
    __syncthreads();
  }
  if (kc < nk) compute(0);  // odd chunk count: the last chunk is in stage 0

  // ---- epilogue: bias, activation, fp32 residual; NHWC fp32 and / or x3 planes
  const int kh4 = 4 * (lane >> 5);
  const int ych = p.Cout >> 5;  // chunks per output pixel (POUT: Cout % 32 == 0)
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int m = m0 + (wm * TM + tm) * 32 + fr;
    if (m >= M) continue;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int cb = n0 + (wn * TN + tn) * 32;  // this tile's 32 channels: one output chunk
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = cb + 8 * g + kh4;
        if (c >= p.Cout) continue;
        const float4 bias = *(const float4*)(p.bias + c);
        float v[4] = {acc[tm][tn][4 * g] + bias.x, acc[tm][tn][4 * g + 1] + bias.y, acc[tm][tn][4 * g + 2] + bias.z,
                      acc[tm][tn][4 * g + 3] + bias.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = apply_act(v[r], p.act);
        if (p.res != nullptr) {
          const float4 rv = *(const float4*)((const float*)p.res + (size_t)m * p.rs + c);
          v[0] += rv.x; v[1] += rv.y; v[2] += rv.z; v[3] += rv.w;
        }
        if (!POUT || p.y != nullptr)
          *(float4*)((float*)p.y + (size_t)m * p.ys + c) = make_float4(v[0], v[1], v[2], v[3]);
        if constexpr (POUT) {
          bf16x4 h, mid, l;
          x3_split4_pair(f32x2{v[0], v[1]}, f32x2{v[2], v[3]}, h, mid, l);
          bf16* d = (bf16*)p.y3 + ((size_t)m * ych + (cb >> 5)) * 96 + 8 * g + kh4;
          *(bf16x4*)d = h;
          *(bf16x4*)(d + 32) = mid;
          *(bf16x4*)(d + 64) = l;
        }
      }
    }
  }
}

namespace {

template <int WM, int WN, int TM, int TN, bool PIN, bool POUT>
void xp_launch(const ConvParams& p, hipStream_t s) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  const long M = (long)p.B * p.Ho * p.Wo;
  const long tiles = ((M + BM - 1) / BM) * ((p.Cout_pad + BN - 1) / BN);
  hipLaunchKernelGGL((conv_x3gp_kernel<WM, WN, TM, TN, PIN, POUT>), dim3((unsigned)tiles), dim3(WM * WN * 64),
                     xp_lds_bytes(BM, BN), s, p);
}

template <int WM, int WN, int TM, int TN>
void xp_launch_io(const ConvParams& p, hipStream_t s) {
  if (p.x_planes && p.y3 != nullptr)
    xp_launch<WM, WN, TM, TN, true, true>(p, s);
  else if (p.x_planes)
    xp_launch<WM, WN, TM, TN, true, false>(p, s);
  else
    xp_launch<WM, WN, TM, TN, false, true>(p, s);
}

// the tiles of gemm_x3.hip's XG_VARIANTS, in its order: impl 111 + v and 111 + v + 10 run tile v
#define XP_TILES(X) \
  X(0, 2, 2, 2, 1)     /* 128 px x  64 ch */ \
  X(1, 2, 2, 2, 2)     /* 128 px x 128 ch */ \
  X(2, 4, 1, 1, 1)     /* 128 px x  32 ch */ \
  X(3, 4, 1, 1, 2)     /* 128 px x  64 ch, one 32-px row per wave */ \
  X(4, 2, 2, 1, 2)     /*  64 px x 128 ch */ \
  X(5, 2, 2, 1, 1)     /*  64 px x  64 ch */ \
  X(6, 2, 4, 2, 1)     /* 128 px x 128 ch, 8 waves */ \
  X(7, 4, 2, 1, 2)     /* 128 px x 128 ch, 8 waves */ \
  X(8, 4, 2, 2, 1)     /* 256 px x  64 ch, 8 waves */ \
  X(9, 4, 2, 1, 1)     /* 128 px x  64 ch, 8 waves */

static_assert(2 * F32_TABLE_ROWS(XP_TILES) == kF32X3GVariants, "XP_TILES rows != the X3G family's tiles (f32_impl.h)");

void xp_refuse(const char* why) { throw std::runtime_error(std::string("conv_x3gp: ") + why); }

}  // namespace

void conv_x3gp(const ConvParams& p, hipStream_t s, int v) {
  constexpr size_t kMax = (1u << 31) - (1u << 20);
  const bool pin = p.x_planes != 0, pout = p.y3 != nullptr;
  if (!pin && !pout) xp_refuse("neither x_planes nor y3 is set");
  if (p.w3 == nullptr) xp_refuse("needs pre-split weights (w3)");
  if (p.y2 != nullptr) xp_refuse("an upsampled second output (y2) is not supported");
  if (p.pw_w != nullptr || p.pw_y != nullptr) xp_refuse("a fused pointwise conv (pw_*) is not supported");
  if (p.gate != nullptr) xp_refuse("a tile gate is not supported");
  if (p.n_lo != 0 || p.n_hi != 0) xp_refuse("an output-channel window is not supported");
  if (p.marks != nullptr) xp_refuse("a mark gate is not supported");
  if (p.sk_splits != 0) xp_refuse("split-K is not supported");
  if (p.lb_meta != nullptr) xp_refuse("a letterbox source is not supported");
  if (!((p.KH == 1 && p.KW == 1) || (p.KH == 3 && p.KW == 3))) xp_refuse("only 1x1 and 3x3 convs");
  if (p.stride != 1 && p.stride != 2) xp_refuse("only stride 1 and 2");
  if (pin && p.Cin % 32 != 0) xp_refuse("a planes input needs Cin % 32 == 0");
  if (pout && p.Cout % 32 != 0) xp_refuse("a planes output needs Cout % 32 == 0");
  if (!pout && p.y == nullptr) xp_refuse("no output");
  if (p.Cin % 4 != 0 || p.Cout % 4 != 0 || p.Cout > p.Cout_pad || p.Kpad < p.KH * p.KW * p.Cin ||
      (!pin && p.xs % 4 != 0) || (p.y != nullptr && p.ys % 4 != 0) || (p.res != nullptr && p.rs % 4 != 0))
    xp_refuse("unsupported geometry (Cin / Cout / strides % 4, Kpad >= KH*KW*Cin)");
  const size_t px_in = (size_t)p.B * p.H * p.W, px_out = (size_t)p.B * p.Ho * p.Wo;
  const size_t cin32 = (size_t)(p.Cin + 31) / 32;
  if (px_in * (pin ? cin32 * 192 : (size_t)p.xs * 4) >= kMax || (size_t)p.KH * p.KW * cin32 * p.Cout_pad * 192 >= kMax ||
      px_out * (size_t)(p.y != nullptr ? p.ys : 0) * 4 >= kMax || px_out * (size_t)(pout ? p.Cout : 0) * 6 >= kMax ||
      px_out * (size_t)(p.res != nullptr ? p.rs : 0) * 4 >= kMax)
    xp_refuse("a tensor of 2 GiB or more");
  if (px_out == 0) return;
  switch (v >= 10 ? v - 10 : v) {
#define XP_CASE(V, WM, WN, TM, TN) \
  case V: xp_launch_io<WM, WN, TM, TN>(p, s); return;
    XP_TILES(XP_CASE)
#undef XP_CASE
    default: xp_refuse("unknown tile variant");
  }
}

void x3gp_prepare() {
#define XP_ATTR1(WM, WN, TM, TN, PIN, POUT)                                                          \
  ARENA_HIP_CHECK(hipFuncSetAttribute((const void*)conv_x3gp_kernel<WM, WN, TM, TN, PIN, POUT>,      \
                                      hipFuncAttributeMaxDynamicSharedMemorySize,                    \
                                      xp_lds_bytes(WM * TM * 32, WN * TN * 32)));
#define XP_ATTR(V, WM, WN, TM, TN)        \
  XP_ATTR1(WM, WN, TM, TN, true, true)    \
  XP_ATTR1(WM, WN, TM, TN, true, false)   \
  XP_ATTR1(WM, WN, TM, TN, false, true)
  XP_TILES(XP_ATTR)
#undef XP_ATTR
#undef XP_ATTR1
}

}  // namespace arena
