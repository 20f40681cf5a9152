// fp32-accurate 3x3 stride-1 pad-1 convolution to exactly 80 output channels, with the Detect head's final 1x1
// optionally fused: exact 80-wide halo tiles on the 16x16 bf16 matrix cores over pre-split weights ("x3hc", the
// class branch of the Detect head).
//
// The class branch's convs (80x80x64 / 40x40x128 -> 80 of the stacked first head conv, 80 -> 80 with the 1x1 -> 80
// fused) ran on tiles that do not fit 80 channels: x3hg's 32-wide fragments pad N 80 -> 96 in the 3x3 and K2 80 -> 96
// in the fused 1x1 (PWN = 3, 16 accumulator registers per fragment), and the 16-wide x3hp family has no fused 1x1.
// 80 = 5 x 16, so here:
//
//   * N: five 16-channel fragments of v_mfma_f32_16x16x32_bf16 (A = weights, row = channel; B = pixels, column =
//     pixel of one 16-pixel tile row).  No padded output channel anywhere, 4 accumulator registers per fragment.
//   * K of the 3x3: one tap x 32 input channels per step; a last chunk of 16 channels (Cin 80: 2.5 steps per tap)
//     runs on v_mfma_f32_16x16x16_bf16 over the first half of each staged plane.  Per 16 pixels and tap that is
//     3 steps x 6 products x 5 fragments = 90 MFMA instructions (810 over the nine taps), the same number as with a
//     zero-padded third step; what the half step saves is depth: 30 of the 90 are 16-deep, K multiplied is 80 per
//     tap instead of 96.  Packing (tap, channel) linearly (720 = 22.5 steps) multiplies the same K and would cost a
//     per-step (tap, channel) lookup for every halo read.  Padding left: none in the arithmetic; the staged weight
//     rows of a half chunk carry 16 zero k per plane that are copied and never read.
//   * Weights: the plan's pre-split planes as every x3g / x3h kernel reads them (ConvParams.w3, engine/planner.py
//     pack_conv_weight_x3: [tap * Cin32 / 32 + c / 32][80][h 32 | m 32 | l 32]).  A stage is one contiguous run of 80
//     192-byte rows = 960 plain 16-byte copies, so the family needs no layout of its own.
//   * Halo: 32 input channels of the (TH + 2) x 18 halo pixels are split once (x3.h) into h | m | l planes on the
//     way into LDS and feed all nine taps.  The weight stage is double-buffered: one barrier per tap, two where the
//     halo chunk is replaced, the next stage's global loads (and the next chunk's halo, during tap 0) in flight
//     during the current MFMAs.
//   * Fused 1x1 (ConvParams.pw_*, the contract of the x3hg fused-1x1 kernels): register remap, no LDS exchange and
//     no LDS in the budget for it.  Accumulator lane (pixel p, quarter q) of fragment j holds channels 16 j + 4 q +
//     {0..3} of pixel p, which is exactly the B operand of a 16-deep step (lane (p, q) supplies k = 4 q .. 4 q + 3):
//     the remap is the identity.  K2 = 80 is run exactly as five steps of v_mfma_f32_16x16x16_bf16, fragment j being
//     step j: 5 x 6 = 30 MFMA instructions per output fragment, 150 per 16 pixels, K multiplied 80.  Three 32-deep
//     steps over K2 = 96 are 90 instructions, K multiplied 96, and need a zero sixth fragment.  By instruction count
//     the 32-deep form is lower (90 against 150, beside the 3x3's 810 at Cin 80); the 16-deep form was taken for the
//     identity remap, no padded K, one load shape and one
//     split per accumulator register.  The 1x1 weights are x3hg's operand unchanged (pack_pw_weight_x3,
//     [rows][h | m | l][96]): there the four channels 16 j + 4 q + {0..3} are the four consecutive columns
//     16 j + 8 (q & 1) + 4 (q >> 1), so a lane reads one 8-byte piece per plane and step straight from global
//     memory (L1 / L2-resident, 55 KB).  Columns 80..95 are never read.  The 3x3 result is not stored.
//   * Grid: one workgroup per pixel tile and image, all 80 channels, blocks remapped per XCD (x3.h) so neighbouring
//     tiles share an L2; rows and columns past the map are masked in the epilogue, their halo reads return zeros.
//     Images at or past the live count (ConvParams.bdev) are not touched.
//
// Workgroup: NW waves, tile TH x 16 pixels; wave w computes rows w + NW f, f < MF = TH / NW (MF x 5 fragments).
// LDS: a halo pixel is [h 32 | m 32 | l 32 | 8 pad] bf16 = 208 B = 13 16-byte slots, a weight row the same; 13 is
// odd, so the 16 consecutive rows (pixels of a tile row, channels of a fragment) that a ds_read_b128 lane group
// reads at one k offset land on 16 distinct slots of the 16.  Bytes: ((TH + 2) x 18 + 2 x 80) x 208.
//
// Variants <TH, NW>, compiled for gfx950 (VGPRs + AGPRs / scratch bytes / LDS bytes / waves per SIMD the compiler
// reports; plain, fused 1x1):
//   <8, 4>   8 x 16 px, 256 threads: 155 + 40 / 0 / 70720 / 2,  156 + 40 / 0 / 70720 / 2    (two workgroups per CU)
//   <16, 8> 16 x 16 px, 512 threads: 172 + 0 / 0 / 100672 / 2,  174 + 0 / 0 / 100672 / 2    (one workgroup per CU: LDS)
//   <4, 4>   4 x 16 px, 256 threads: 113 + 20 / 0 / 55744 / 3,  114 + 20 / 0 / 55744 / 3    (two per CU: LDS)
//
// Measured on MI355X, fp32 headline program at batch 32 (profiles/r12_x3hc/, two passes each, us): **x3hc loses**.
//   80x80x80 -> 80 + 1x1 -> 80 (op 49): conv_x3hg_kernel<16,4,1,1,3,3> 181.3 / 180.1; x3hc <8, 4> 224.8 / 223.8,
//                                       <16, 8> 281.5 / 288.2, <4, 4> 260.2 / 274.6
//   40x40x80 -> 80 + 1x1 -> 80 (op 52): x3hg 60.9 / 60.0; x3hc <8, 4> 66.8 / 66.8, <16, 8> 135.1 / 135.7, <4, 4> 84.6 / 86.8
// The shipped tuning table therefore does not name the family; it is selectable (impl 211 + v) and an autotune
// candidate.  The class windows of the split first head convs (ops 47 / 50) need an output-channel window and stay
// on x3hp.  Buckets below 32 and the unfused conv were not measured.
#include <stdexcept>
#include <string>

#include "launch.h"
#include "x3.h"

namespace arena {

namespace {

constexpr int HC_N = 80;            // output channels, exactly
constexpr int HC_TW = 16, HC_HC = HC_TW + 2;
constexpr int HC_P = 3 * 32 + 8;    // bf16 per LDS row (halo pixel or weight row): 208 B
constexpr int HC_K2 = 96;           // columns per plane row of the 1x1 operand (pack_pw_weight_x3 of 80 channels)
__host__ __device__ constexpr int hc_lds_bytes(int TH) { return ((TH + 2) * HC_HC + 2 * HC_N) * HC_P * 2; }

}  // namespace

template <int TH, int NW, bool PW>
__global__ __launch_bounds__(NW * 64) void conv_x3hc_kernel(const ConvParams p) {
  static_assert(TH % NW == 0, "every wave computes TH / NW tile rows");
  constexpr int NT = NW * 64, MF = TH / NW, NF = HC_N / 16;
  constexpr int HPIX = (TH + 2) * HC_HC;
  constexpr int XI = (HPIX * 8 + NT - 1) / NT;  // halo float4 items (pixel, 4-channel group) per thread
  constexpr int WPC = HC_N * 12;                // 16-B weight pieces per stage (12 per row)
  constexpr int WI = (WPC + NT - 1) / NT;
  extern __shared__ __attribute__((aligned(16))) bf16 hc_lds[];
  bf16* sX = hc_lds;                 // [HPIX][HC_P]
  bf16* sW = hc_lds + HPIX * HC_P;   // [2][HC_N][HC_P]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int tiles_x = (p.Wo + HC_TW - 1) / HC_TW, tiles_y = (p.Ho + TH - 1) / TH;
  const int tiles = tiles_x * tiles_y;
  const int bx = xcd_remap(blockIdx.x, gridDim.x);
  const int b = bx / tiles;
  if (b >= live_batch(p.B, p.bdev)) return;
  const int t = bx - b * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int oy0 = ty * TH, ox0 = tx * HC_TW;
  const int iy0 = oy0 - 1, ix0 = ox0 - 1;
  const int H = p.H, W = p.W, Cin = p.Cin;

  // raw buffer loads: out-of-range offsets (halo outside the map, channels past Cin) read zeros; every weight
  // piece of a stage is inside the operand; host: both tensors < 2 GiB (x3hc_supported)
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.x), (short)0, (int)((size_t)p.B * H * W * p.xs * 4), 0x00020000);
  const int cin32 = (Cin + 31) >> 5;  // 32-deep chunks per tap in the w3 layout
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.w3), (short)0, (int)((size_t)9 * cin32 * HC_N * 192), 0x00020000);
  constexpr int kOob = 0x7fffffff & ~15;

  // per halo item: byte offset of its (pixel, group) at channel chunk 0, or kOob
  int x_off[XI];
  const size_t img = (size_t)b * H * W;
#pragma unroll
  for (int j = 0; j < XI; ++j) {
    const int i = tid + NT * j;
    const int px = i >> 3, g = i & 7;
    const int hy = px / HC_HC, hx = px - hy * HC_HC;
    const int iy = iy0 + hy, ix = ix0 + hx;
    const bool in = i < HPIX * 8 && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
    x_off[j] = in ? (int)(((img + (size_t)iy * W + ix) * p.xs + 4 * g) * 4) : kOob;
  }

  f32x4 rx[XI];
  u32x4 rw[WI];
  auto load_x = [&](int c0) {  // input channels c0 + 4 g .. + 3 of every halo pixel
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      const int c = c0 + 4 * ((tid + NT * j) & 7);
      const int o = (x_off[j] != kOob && c < Cin) ? x_off[j] + 4 * c0 : kOob;
      rx[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, o, 0, 0));
    }
  };
  auto store_x = [&]() {
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      const int i = tid + NT * j;
      if (HPIX * 8 % NT == 0 || i < HPIX * 8) {
        bf16x2 h0, m0, l0, h1, m1, l1;  // split two values at a time (x3.h)
        split_bf16x3_pair(f32x2{rx[j][0], rx[j][1]}, h0, m0, l0);
        split_bf16x3_pair(f32x2{rx[j][2], rx[j][3]}, h1, m1, l1);
        bf16* d = sX + (i >> 3) * HC_P + 4 * (i & 7);
        *(bf16x4*)d = __builtin_shufflevector(h0, h1, 0, 1, 2, 3);
        *(bf16x4*)(d + 32) = __builtin_shufflevector(m0, m1, 0, 1, 2, 3);
        *(bf16x4*)(d + 64) = __builtin_shufflevector(l0, l1, 0, 1, 2, 3);
      }
    }
  };
  auto load_w = [&](int st) {  // stage st = (chunk, tap): the 80 rows of row block tap * cin32 + chunk, piece by piece
    const int chunk = st / 9, tap = st - chunk * 9;
    const int step = (tap * cin32 + chunk) * HC_N * 192;  // wave-uniform
#pragma unroll
    for (int j = 0; j < WI; ++j) {
      const int i = tid + NT * j;
      rw[j] = __builtin_amdgcn_raw_buffer_load_b128(wr, (WPC % NT == 0 || i < WPC) ? i * 16 : kOob, step, 0);
    }
  };
  auto store_w = [&](int buf) {
    bf16* d = sW + buf * HC_N * HC_P;
#pragma unroll
    for (int j = 0; j < WI; ++j) {
      const int i = tid + NT * j;
      if (WPC % NT == 0 || i < WPC) *(u32x4*)(d + (i / 12) * HC_P + (i % 12) * 8) = rw[j];
    }
  };

  f32x4 acc[MF][NF];
#pragma unroll
  for (int f = 0; f < MF; ++f)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[f][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // one tap of one chunk: `half` = the chunk holds 16 channels (wave-uniform)
  auto compute = [&](int buf, int tap, bool half) {
    const int ky = tap / 3, kx = tap - ky * 3;
    const bf16* wb = sW + buf * HC_N * HC_P;
    if (!half) {
      bf16x8 bh[MF], bm[MF], bl[MF];
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        const bf16* r = sX + ((wave + NW * f + ky) * HC_HC + col + kx) * HC_P + 8 * kq;
        bh[f] = *(const bf16x8*)r;
        bm[f] = *(const bf16x8*)(r + 32);
        bl[f] = *(const bf16x8*)(r + 64);
      }
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const bf16* r = wb + (j * 16 + col) * HC_P + 8 * kq;
        const bf16x8 ah = *(const bf16x8*)r, am = *(const bf16x8*)(r + 32), al = *(const bf16x8*)(r + 64);
#pragma unroll
        for (int f = 0; f < MF; ++f) acc[f][j] = x3_mfma(ah, am, al, bh[f], bm[f], bl[f], acc[f][j]);
      }
    } else {
      bf16x4 bh[MF], bm[MF], bl[MF];
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        const bf16* r = sX + ((wave + NW * f + ky) * HC_HC + col + kx) * HC_P + 4 * kq;
        bh[f] = *(const bf16x4*)r;
        bm[f] = *(const bf16x4*)(r + 32);
        bl[f] = *(const bf16x4*)(r + 64);
      }
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const bf16* r = wb + (j * 16 + col) * HC_P + 4 * kq;
        const bf16x4 ah = *(const bf16x4*)r, am = *(const bf16x4*)(r + 32), al = *(const bf16x4*)(r + 64);
#pragma unroll
        for (int f = 0; f < MF; ++f) acc[f][j] = x3_mfma(ah, am, al, bh[f], bm[f], bl[f], acc[f][j]);
      }
    }
  };

  const int ns = cin32 * 9;
  load_x(0);
  load_w(0);
  store_x();
  store_w(0);
  __syncthreads();
  for (int st = 0; st < ns; ++st) {
    const int chunk = st / 9, tap = st - chunk * 9;
    const bool more = st + 1 < ns;
    if (more) load_w(st + 1);
    if (tap == 0 && chunk + 1 < cin32) load_x((chunk + 1) * 32);  // lands during this chunk's nine taps
    compute(st & 1, tap, Cin - chunk * 32 < 32);
    if (more) {
      if (tap == 8) {  // every wave is done with this chunk's halo before it is replaced
        __syncthreads();
        store_x();
      }
      store_w((st + 1) & 1);
      __syncthreads();
    }
  }

  const size_t HWo = (size_t)p.Ho * p.Wo;
  if constexpr (PW) {
    // ---- fused 1x1: out2 = W2 . act(conv + bias) + b2 (+ act2); the 3x3 result is not stored
    const bf16* __restrict__ w2 = (const bf16*)p.pw_w;
    const int kc = 8 * (kq & 1) + 4 * (kq >> 1);  // this lane's four columns within a fragment's 16 (pack_pw_weight_x3)
    const int nf2 = (p.pw_cout + 15) >> 4;
#pragma unroll
    for (int f = 0; f < MF; ++f) {
      // B operand: fragment j as the 16-deep step j, straight from the accumulators
      bf16x4 bh[NF], bm[NF], bl[NF];
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const float4 bias = *(const float4*)(p.bias + j * 16 + kq * 4);
        const float bb[4] = {bias.x, bias.y, bias.z, bias.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) x3_split_at(apply_act(acc[f][j][e] + bb[e], p.act), e, bh[j], bm[j], bl[j]);
      }
      const int oy = oy0 + wave + NW * f, ox = ox0 + col;
      const bool live = oy < p.Ho && ox < p.Wo;
      const size_t pix = (size_t)b * HWo + (size_t)oy * p.Wo + ox;
#pragma unroll
      for (int t2 = 0; t2 < NF; ++t2) {
        if (t2 >= nf2) break;  // uniform: no row of this fragment is an output channel
        const bf16* wrow = w2 + (size_t)((t2 * 16 + col) * 3) * HC_K2 + kc;
        f32x4 a2 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NF; ++j)
          a2 = x3_mfma(*(const bf16x4*)(wrow + 16 * j), *(const bf16x4*)(wrow + HC_K2 + 16 * j),
                       *(const bf16x4*)(wrow + 2 * HC_K2 + 16 * j), bh[j], bm[j], bl[j], a2);
        const int c2 = t2 * 16 + kq * 4;
        if (!live || c2 >= p.pw_cout) continue;
        const float4 b2 = *(const float4*)(p.pw_bias + c2);
        const float4 o = make_float4(apply_act(a2[0] + b2.x, p.pw_act), apply_act(a2[1] + b2.y, p.pw_act),
                                     apply_act(a2[2] + b2.z, p.pw_act), apply_act(a2[3] + b2.w, p.pw_act));
        *(float4*)((float*)p.pw_y + pix * p.pw_ys + c2) = o;
      }
    }
  } else {
    // ---- epilogue: bias, activation, NHWC fp32
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int cb = j * 16 + kq * 4;
      const float4 bias = *(const float4*)(p.bias + cb);
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        const int oy = oy0 + wave + NW * f, ox = ox0 + col;
        if (oy >= p.Ho || ox >= p.Wo) continue;
        const size_t pix = (size_t)b * HWo + (size_t)oy * p.Wo + ox;
        const float4 o = make_float4(apply_act(acc[f][j][0] + bias.x, p.act), apply_act(acc[f][j][1] + bias.y, p.act),
                                     apply_act(acc[f][j][2] + bias.z, p.act), apply_act(acc[f][j][3] + bias.w, p.act));
        *(float4*)((float*)p.y + pix * p.ys + cb) = o;
      }
    }
  }
}

namespace {

// variant v: (TH, NW) -> tile TH x 16 pixels x 80 channels on NW waves
#define HC_VARIANTS(X) \
  X(0, 8, 4)   /*  8 x 16 px, 4 waves */ \
  X(1, 16, 8)  /* 16 x 16 px, 8 waves */ \
  X(2, 4, 4)   /*  4 x 16 px, 4 waves: small buckets */

static_assert(F32_TABLE_ROWS(HC_VARIANTS) == kF32X3HCVariants, "HC_VARIANTS rows != the family's count (f32_impl.h)");

template <int TH, int NW>
void hc_launch(const ConvParams& p, hipStream_t s) {
  const long tiles = (long)p.B * ((p.Ho + TH - 1) / TH) * ((p.Wo + HC_TW - 1) / HC_TW);
  if (p.pw_w != nullptr)
    hipLaunchKernelGGL((conv_x3hc_kernel<TH, NW, true>), dim3((unsigned)tiles), dim3(NW * 64), hc_lds_bytes(TH), s, p);
  else
    hipLaunchKernelGGL((conv_x3hc_kernel<TH, NW, false>), dim3((unsigned)tiles), dim3(NW * 64), hc_lds_bytes(TH), s, p);
}

}  // namespace

// The family's eligibility: 3x3 stride 1 pad 1 over Cin % 16 == 0 channels to exactly 80, pre-split weights, bias and
// activation only (no residual, upsampled copy, window, marks or gate); the fused 1x1 as x3hg's operand over K2 96.
bool x3hc_supported(const ConvParams& p) {
  const size_t x_bytes = (size_t)p.B * p.H * p.W * p.xs * 4;
  const size_t w_bytes = (size_t)9 * ((p.Cin + 31) / 32) * HC_N * 192;
  const bool conv = p.w3 != nullptr && p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad_t == 1 && p.pad_l == 1 &&
                    p.Ho == p.H && p.Wo == p.W && p.Cin >= 16 && p.Cin % 16 == 0 && p.xs % 4 == 0 &&
                    p.Cout == HC_N && p.Cout_pad == HC_N && x_bytes < (1u << 31) - (1u << 20) &&
                    w_bytes < (1u << 31) - (1u << 20) && p.res == nullptr && p.y2 == nullptr &&
                    p.lb_meta == nullptr && p.n_lo == 0 && p.n_hi == 0 && p.marks == nullptr && p.gate == nullptr;
  // float4 / b128 accesses: 16-byte aligned bases (a channel offset that is no multiple of 4 fails here)
  auto al16 = [](const void* q) { return q != nullptr && (uintptr_t)q % 16 == 0; };
  if (!conv || !al16(p.x) || !al16(p.w3) || !al16(p.bias)) return false;
  if (p.pw_w == nullptr) return al16(p.y) && p.ys % 4 == 0;
  return al16(p.pw_y) && al16(p.pw_bias) && (uintptr_t)p.pw_w % 8 == 0 && p.pw_kpad == HC_K2 && p.pw_cout > 0 &&
         p.pw_cout % 4 == 0 && p.pw_cout <= HC_N && p.pw_ys % 4 == 0;
}

bool conv_x3hc(const ConvParams& p, hipStream_t s, int v) {
  if (!x3hc_supported(p)) return false;
  switch (v) {
#define HC_CASE(V, TH, NW) \
  case V: hc_launch<TH, NW>(p, s); return true;
    HC_VARIANTS(HC_CASE)
#undef HC_CASE
    default: return false;
  }
}

void x3hc_prepare() {
#define HC_ATTR(V, TH, NW)                                                                                     \
  ARENA_HIP_CHECK(hipFuncSetAttribute((const void*)conv_x3hc_kernel<TH, NW, false>,                            \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, hc_lds_bytes(TH)));          \
  ARENA_HIP_CHECK(hipFuncSetAttribute((const void*)conv_x3hc_kernel<TH, NW, true>,                             \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, hc_lds_bytes(TH)));
  HC_VARIANTS(HC_ATTR)
#undef HC_ATTR
}

}  // namespace arena
