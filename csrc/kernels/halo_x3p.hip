// fp32-accurate 3x3 stride-1 convolution: 16x16x32 halo tiles over pre-split weights ("x3hp").
//
// conv_x3_halo_kernel (conv_f32.hip) with its weight staging replaced: the same output tile (TH rows x 16
// columns of one image x BN = NF*16 channels, wave w computing rows w and w + TH/2), the same 32-channel input
// chunks, the same K order (chunk, ky, kx) and the same six products per 32-deep step (x3.h), so every output
// is bit-identical to impl 101 / 102 / 103 / 108 / 109 whatever the tile.
// What differs is how a stage reaches LDS:
//
//   * weights are the plan's pre-split bf16 planes (ConvParams.w3, engine/planner.py pack_conv_weight_x3:
//     [tap * Cin32/32 + c/32][Cout_pad][h 32 | m 32 | l 32], one 192-byte row per output channel and 32-deep
//     K step).  A stage's rows go global -> registers -> LDS as plain 16-byte pieces: no convert, no subtract.
//     The old kernel split the fp32 weights again in every workgroup and every launch (three bf16 converts and
//     two subtracts per element: ~70 % of its staging work at NF 3).  Per-thread piece offsets are computed
//     once; a stage adds one wave-uniform offset (raw buffer loads, rows past Cout_pad read zeros);
//   * the input halo's per-thread offsets are computed once per kernel as well, and the chunk is split two
//     values at a time (split_bf16x3_pair, x3.h);
//   * TS = taps per weight stage: 3 stages one kernel row (ky) as the old kernel does (608-B rows); 1 stages a
//     single tap (224-B rows), which lets one workgroup hold all nine 16-channel fragments of the 144-channel
//     Detect-head convs (NF 9: 32 KB of weights per stage) so that their halo is staged and split once, not
//     once per 48-channel tile.
//
// Two optional additions for the split Detect-head convs (runtime/head_marks.h): an output-channel window
// (ConvParams.n_lo / n_hi: the workgroup's first channel is n_lo + blockIdx.y * BN, the epilogue stops at n_hi, the
// grid covers the window only; weight rows, bias and output addresses stay absolute) and a mark gate
// (ConvParams.marks: a workgroup whose tile no continuing consumer tile reads returns before any load).  A tile that
// runs computes exactly what it computes in the whole conv.  <5, 8, 1> holds the 80-channel class window on per-tap
// stages: 58 KB of LDS, two workgroups per CU, where <5, 8, 3> needs 89 KB and runs one (117 vs 176 us for the
// 80x80x64 class window at batch 32, profiles/r11_head_split/README.md).
//
// LDS rows: halo pixels [h 32 | m 32 | l 32 | 16 pad] bf16 = 224 B, weight rows TS x 96 + 16 bf16 = 608 / 224 B;
// both pitches keep the ds_read_b128 fragment reads of 16 consecutive rows conflict-free (tools/lds_bank_model.py).
// The next stage's global loads are issued before the current stage's MFMAs, as in the old kernel.
//
// Measured on MI355X, fp32 headline program at batch 32 (profiles/r8_x3hp/, parent = conv_x3_halo_kernel):
//   80x80x64 -> 144  <3, 8> x 3 tiles -> <9, 8, 1>: 194.9 -> 170.3 us, SQ_INSTS_VALU 5.03e7 -> 2.19e7,
//                    SQ_INSTS_LDS 6.66e6 -> 4.73e6, MFMA busy 42.6 -> 49.2 %
//   40x40x128 -> 144 <3, 8> x 3 tiles -> <9, 8, 1>: 116.6 ->  96.9 us, VALU 2.69e7 -> 1.10e7, MFMA busy 41.7 -> 49.5 %
//   80x80x32 -> 32   <2, 8> -> <2, 8, 3>: 40.9 / 39.7 / 36.6 -> 37.6 / 35.9 / 33.4 us, VALU 7.79e6 -> 5.07e6
//   40x40x64 -> 64   <4, 8> -> <4, 8, 3>: 31.8 / 30.8 -> 28.8 / 28.4 us, VALU 6.19e6 -> 3.55e6
// SQ_INSTS_MFMA is unchanged everywhere.  The 48-channel tile <3, 8, 3> runs the two 144-channel convs as fast as
// <9, 8, 1> within the run-to-run spread (178.1 vs 183.4 and 105.1 vs 105.1 us in one trace, 170.8 vs 172.0 and
// 99.6 vs 94.2 us stand-alone) with 3 x the halo staging; the 16-row all-N tile <9, 16, 1> is slower (190 / 158 us
// stand-alone: 105 KB of LDS, one workgroup per CU).  Registers and LDS per variant: profiles/r8_x3hp/README.md.
#include <stdexcept>
#include <string>

#include "../runtime/head_marks.h"
#include "launch.h"
#include "x3.h"

namespace arena {

namespace {

constexpr int HP_TW = 16, HP_HC = HP_TW + 2;
constexpr int HP_XP = 3 * 32 + 16;  // bf16 per halo pixel (224 B)
__host__ __device__ constexpr int hp_wp(int TS) { return TS * 96 + 16; }  // bf16 per weight row of one stage
__host__ __device__ constexpr int hp_lds_bytes(int NF, int TH, int TS) {
  return ((TH + 2) * HP_HC * HP_XP + NF * 16 * hp_wp(TS)) * 2;
}

}  // namespace

template <int NF, int TH, int TS>
__global__ __launch_bounds__(TH * 32) void conv_x3hp_kernel(const ConvParams p) {
  static_assert(TS == 1 || TS == 3, "a weight stage is one tap or one kernel row");
  constexpr int NT = TH * 32, NW = TH / 2;  // threads, waves (wave w: rows w and w + NW)
  constexpr int HR = TH + 2, HPIX = HR * HP_HC;
  constexpr int XI = (HPIX * 8 + NT - 1) / NT;  // halo float4 items (pixel, 4-channel group) per thread
  constexpr int BN = NF * 16, MF = 2;
  constexpr int WP = hp_wp(TS);
  constexpr int WPC = TS * BN * 12;             // 16-B weight pieces per stage (12 per row and tap)
  constexpr int WI = (WPC + NT - 1) / NT;       // ... per thread
  constexpr int SPC = 9 / TS;                   // stages per 32-channel chunk
  extern __shared__ __attribute__((aligned(16))) bf16 hp_lds[];
  bf16* sX = hp_lds;                  // [HPIX][HP_XP]
  bf16* sW = hp_lds + HPIX * HP_XP;   // [BN][WP]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int tiles_x = (p.Wo + HP_TW - 1) / HP_TW, tiles_y = (p.Ho + TH - 1) / TH;
  const int tiles = tiles_x * tiles_y;
  const int bx = xcd_remap(blockIdx.x, gridDim.x);
  const int b = bx / tiles;
  if (b >= live_batch(p.B, p.bdev)) return;
  const int t = bx - b * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int oy0 = ty * TH, ox0 = tx * HP_TW;
  // ---- mark gate (ConvParams.marks): nothing reads this tile unless a continuing consumer tile touches it; before
  // any halo or weight load.  Wave-uniform: at most 18 mark reads for 8 x 16 tiles on both sides.
  if (p.marks != nullptr) {
    const int* m = p.marks + (size_t)b * head_mark_cells(p.Ho) * head_mark_cells(p.Wo);
    if (!head_marks_needed(m, p.Ho, p.Wo, ty, tx, TH, HP_TW, p.mark_uh, p.mark_uw, p.mark_halo)) return;
  }
  const int iy0 = oy0 - p.pad_t, ix0 = ox0 - p.pad_l;
  const int n0 = p.n_lo + blockIdx.y * BN;  // the launcher sets n_hi (the whole conv: [0, Cout))
  const int H = p.H, W = p.W, Cin = p.Cin;

  // raw buffer loads: out-of-range offsets (halo outside the map, channels past Cin, weight rows past
  // Cout_pad) read zeros; host: both tensors < 2 GiB (x3hp_supported)
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.x), (short)0, (int)((size_t)p.B * H * W * p.xs * 4), 0x00020000);
  const int cin32 = (Cin + 31) >> 5;  // 32-deep chunks per tap in the w3 layout
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.w3), (short)0, (int)((size_t)9 * cin32 * p.Cout_pad * 192), 0x00020000);
  constexpr int kOob = 0x7fffffff & ~15;

  // per halo item: byte offset of its (pixel, group) at channel chunk 0, or kOob
  int x_off[XI];
  const size_t img = (size_t)b * H * W;
#pragma unroll
  for (int j = 0; j < XI; ++j) {
    const int i = tid + NT * j;
    const int px = i >> 3, g = i & 7;
    const int hy = px / HP_HC, hx = px - hy * HP_HC;
    const int iy = iy0 + hy, ix = ix0 + hx;
    const bool in = i < HPIX * 8 && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
    x_off[j] = in ? (int)(((img + (size_t)iy * W + ix) * p.xs + 4 * g) * 4) : kOob;
  }
  // per weight piece (tap of the stage, row, 16-B piece of the row): byte offset from the stage's first row
  // block, or kOob; and its place in LDS
  int w_off[WI], w_dst[WI];
  const int tap_bytes = cin32 * p.Cout_pad * 192;  // one tap's row blocks
#pragma unroll
  for (int j = 0; j < WI; ++j) {
    const int i = tid + NT * j;
    const int kxl = i / (BN * 12), r = i - kxl * (BN * 12);
    const int row = r / 12, piece = r - row * 12;
    const int n = n0 + row;
    w_off[j] = (i < WPC && n < p.Cout_pad) ? kxl * tap_bytes + n * 192 + piece * 16 : kOob;
    w_dst[j] = row * WP + kxl * 96 + piece * 8;
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
        bf16* d = sX + (i >> 3) * HP_XP + 4 * (i & 7);
        *(bf16x4*)d = __builtin_shufflevector(h0, h1, 0, 1, 2, 3);
        *(bf16x4*)(d + 32) = __builtin_shufflevector(m0, m1, 0, 1, 2, 3);
        *(bf16x4*)(d + 64) = __builtin_shufflevector(l0, l1, 0, 1, 2, 3);
      }
    }
  };
  auto load_w = [&](int st) {  // stage st = (chunk, s): taps s * TS .. + TS - 1 of the chunk's 32 channels
    const int chunk = st / SPC, s = st - chunk * SPC;
    const int step = (s * TS * cin32 + chunk) * p.Cout_pad * 192;  // wave-uniform
#pragma unroll
    for (int j = 0; j < WI; ++j) rw[j] = __builtin_amdgcn_raw_buffer_load_b128(wr, w_off[j], step, 0);
  };
  auto store_w = [&]() {
#pragma unroll
    for (int j = 0; j < WI; ++j)
      if (WPC % NT == 0 || tid + NT * j < WPC) *(u32x4*)(sW + w_dst[j]) = rw[j];
  };

  f32x4 acc[MF][NF];
#pragma unroll
  for (int f = 0; f < MF; ++f)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[f][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nstage = cin32 * SPC;
  load_x(0);
  load_w(0);
  for (int st = 0; st < nstage; ++st) {
    const int chunk = st / SPC, s = st - chunk * SPC;
    if (s == 0) store_x();
    store_w();
    __syncthreads();
    if (st + 1 < nstage) {  // next stage's global loads overlap this stage's MFMAs
      if (s == SPC - 1) load_x((chunk + 1) * 32);
      load_w(st + 1);
    }
    const int ky = TS == 3 ? s : s / 3;
#pragma unroll
    for (int kxl = 0; kxl < TS; ++kxl) {
      const int kx = TS == 3 ? kxl : s - ky * 3;
      bf16x8 bh[MF], bm[MF], bl[MF];
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        const int oy = wave + NW * f;
        const bf16* r = &sX[((oy + ky) * HP_HC + col + kx) * HP_XP + 8 * kq];
        bh[f] = *(const bf16x8*)r;
        bm[f] = *(const bf16x8*)(r + 32);
        bl[f] = *(const bf16x8*)(r + 64);
      }
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const bf16* r = &sW[(j * 16 + col) * WP + kxl * 96 + 8 * kq];
        const bf16x8 ah = *(const bf16x8*)r;
        const bf16x8 am = *(const bf16x8*)(r + 32);
        const bf16x8 al = *(const bf16x8*)(r + 64);
#pragma unroll
        for (int f = 0; f < MF; ++f) acc[f][j] = x3_mfma(ah, am, al, bh[f], bm[f], bl[f], acc[f][j]);
      }
    }
    __syncthreads();
  }

  const int HWo = p.Ho * p.Wo;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int cb = n0 + j * 16 + kq * 4;
    if (cb >= p.n_hi) continue;
    const float4 bias = *(const float4*)(p.bias + cb);
#pragma unroll
    for (int f = 0; f < MF; ++f) {
      const int oy = oy0 + wave + NW * f, ox = ox0 + col;
      if (oy >= p.Ho || ox >= p.Wo) continue;
      const size_t pix = (size_t)b * HWo + (size_t)oy * p.Wo + ox;
      float v[4] = {acc[f][j][0] + bias.x, acc[f][j][1] + bias.y, acc[f][j][2] + bias.z, acc[f][j][3] + bias.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = apply_act(v[r], p.act);
      if (p.res != nullptr) {
        const float4 rv = *(const float4*)((const float*)p.res + pix * p.rs + cb);
        v[0] += rv.x; v[1] += rv.y; v[2] += rv.z; v[3] += rv.w;
      }
      const float4 o = make_float4(v[0], v[1], v[2], v[3]);
      *(float4*)((float*)p.y + pix * p.ys + cb) = o;
      if (p.y2 != nullptr) {
        const int W2 = 2 * p.Wo;
        float* y2 = (float*)p.y2;
        const size_t base = ((size_t)(b * 2 * p.Ho + 2 * oy) * W2 + 2 * ox);
        *(float4*)(y2 + base * p.y2s + cb) = o;
        *(float4*)(y2 + (base + 1) * p.y2s + cb) = o;
        *(float4*)(y2 + (base + W2) * p.y2s + cb) = o;
        *(float4*)(y2 + (base + W2 + 1) * p.y2s + cb) = o;
      }
    }
  }
}

namespace {

template <int NF, int TH, int TS>
void hp_launch(const ConvParams& p0, hipStream_t s) {
  constexpr int BN = NF * 16;
  ConvParams p = p0;
  const bool whole = p.n_lo == 0 && p.n_hi == 0;
  if (whole) p.n_hi = p.Cout;
  const int tiles = ((p.Wo + HP_TW - 1) / HP_TW) * ((p.Ho + TH - 1) / TH);
  // the whole conv covers the padded rows as before; a window covers [n_lo, n_hi) only
  const int span = whole ? p.Cout_pad : p.n_hi - p.n_lo;
  dim3 grid((unsigned)(p.B * tiles), (unsigned)((span + BN - 1) / BN));
  hipLaunchKernelGGL((conv_x3hp_kernel<NF, TH, TS>), grid, dim3(TH * 32), hp_lds_bytes(NF, TH, TS), s, p);
}

// variant v: (NF, TH, TS) -> tile TH x 16 pixels x NF * 16 channels, TS taps per weight stage
#define HP_VARIANTS(X) \
  X(0, 2, 8, 3)   /*  8 x 16 px x  32 ch (the tile of impl 103) */ \
  X(1, 3, 8, 3)   /*  8 x 16 px x  48 ch (102) */ \
  X(2, 4, 8, 3)   /*  8 x 16 px x  64 ch (101 on multiples of 64) */ \
  X(3, 5, 8, 3)   /*  8 x 16 px x  80 ch (101 on 80) */ \
  X(4, 2, 16, 3)  /* 16 x 16 px x  32 ch, 8 waves (108 on <= 32) */ \
  X(5, 3, 16, 3)  /* 16 x 16 px x  48 ch (109) */ \
  X(6, 4, 16, 3)  /* 16 x 16 px x  64 ch (108) */ \
  X(7, 9, 8, 1)   /*  8 x 16 px x 144 ch, per-tap stages: the halo staged once for a Detect-head pair */ \
  X(8, 9, 16, 1)  /* 16 x 16 px x 144 ch, 8 waves */ \
  X(9, 5, 8, 1)   /*  8 x 16 px x  80 ch, per-tap stages: the class window of a split Detect-head conv */

static_assert(F32_TABLE_ROWS(HP_VARIANTS) == kF32X3HPVariants, "HP_VARIANTS rows != the family's count (f32_impl.h)");

}  // namespace

bool x3hp_supported(const ConvParams& p) {
  const size_t x_bytes = (size_t)p.B * p.H * p.W * p.xs * 4;
  const size_t w_bytes = (size_t)9 * ((p.Cin + 31) / 32) * p.Cout_pad * 192;
  return p.w3 != nullptr && p.KH == 3 && p.KW == 3 && p.stride == 1 && p.Cin % 4 == 0 && p.xs % 4 == 0 &&
         x_bytes < (1u << 31) - (1u << 20) && w_bytes < (1u << 31) - (1u << 20) && p.Cout % 4 == 0 &&
         p.Cout_pad % 16 == 0 && p.ys % 4 == 0 && (p.res == nullptr || p.rs % 4 == 0) &&
         (p.y2 == nullptr || p.y2s % 4 == 0) && p.lb_meta == nullptr && p.pw_w == nullptr &&
         // window: 16-aligned start, 4-aligned end inside the conv; (0, 0) = the whole conv
         ((p.n_lo == 0 && p.n_hi == 0) ||
          (p.n_lo >= 0 && p.n_lo % 16 == 0 && p.n_hi > p.n_lo && p.n_hi <= p.Cout && p.n_hi % 4 == 0)) &&
         // marks: the consumer's tiles are whole cells, so that the cells of a tile are exactly its pixels
         (p.marks == nullptr || ((uintptr_t)p.marks % 4 == 0 && p.mark_uh > 0 && p.mark_uw > 0 &&
                                 p.mark_uh % kMarkCell == 0 && p.mark_uw % kMarkCell == 0 && p.mark_halo >= 0));
}

bool conv_x3hp(const ConvParams& p, hipStream_t s, int v) {
  if (!x3hp_supported(p)) return false;
  switch (v) {
#define HP_CASE(V, NF, TH, TS) \
  case V: hp_launch<NF, TH, TS>(p, s); return true;
    HP_VARIANTS(HP_CASE)
#undef HP_CASE
    default: return false;
  }
}

void x3hp_prepare() {
#define HP_ATTR(V, NF, TH, TS)                                                                      \
  ARENA_HIP_CHECK(hipFuncSetAttribute((const void*)conv_x3hp_kernel<NF, TH, TS>,                     \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, hp_lds_bytes(NF, TH, TS)));
  HP_VARIANTS(HP_ATTR)
#undef HP_ATTR
}

}  // namespace arena
