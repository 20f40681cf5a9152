// fp32-accurate C3 bottleneck as one kernel: y = silu(conv3x3_p1(silu(x W1 + b1), W2) + b2) [+ x]  ("c3_bneck_x3").
//
// The unfused fp32 program runs a Bottleneck as two convs: the 1x1 writes a [B, H, W, c_] fp32 map that the 3x3
// reads straight back (engine/plans.py _c3).  Here the 1x1 is recomputed on the 3x3's one-pixel halo and its
// result only exists in LDS, already split into the bf16 planes the 3x3 multiplies.
//
// Work split.  A workgroup (4 waves) owns one 8 x 16 pixel tile of one live image and one slice of the c_ / 32
// mid-channel chunks (blockIdx.y).  A mid chunk of the 1x1's outputs is a K chunk of the 3x3, so a slice is a
// split-K part of the 3x3 that recomputes nothing of another slice's 1x1: one slice is the whole bottleneck in
// one launch, several slices are the split-K form for grids that do not fill the device (the launcher's rule).
// Per mid chunk of 32 channels:
//
//   stage 1  mid = silu(x W1[chunk] + b1) on the tile's 10 x 18 halo pixels, zero outside the map (the 3x3's
//            padding).  180 halo pixels = three passes of 64 rows (wave w: rows 16 w .. 16 w + 15 of the pass, both
//            16-channel fragments), x streamed in 32-channel K chunks and split once per element as it enters LDS
//            (split_bf16x3_pair), W1's rows copied from the plan's pre-split planes (pack_conv_weight_x3 of the 1x1:
//            [c / 32][c_][h 32 | m 32 | l 32]).  The next K chunk's global loads are issued before this chunk's
//            MFMAs.  The activated result is split once into h | m | l and stored to the mid planes in LDS.
//   stage 2  acc += conv3x3(mid, W2[:, chunk]) with the six-product chain of x3.h on v_mfma_f32_16x16x32_bf16,
//            wave w computing tile rows w and w + 4 for all c_ output channels.  W2's K slice comes from the
//            pre-split planes the planner packs for the 3x3 ([tap * c_ / 32 + chunk][c_][192 B]), one stage per
//            tap and per 64 output channels, double-buffered: stage s + 1 is loaded while stage s multiplies and
//            lands in the other buffer, one barrier per stage.
//
// Epilogue.  One slice: + b2, SiLU, + x (the shortcut, read from the source), fp32 store.  Several slices: the raw
// partial tile goes to the split-K workspace ([slice][pixel][c_], the layout of gemm_x3.hip's split-K kernels) and
// x3g_sk_reduce sums the slices in order and applies bias, SiLU and the shortcut: deterministic, slices - 1 more
// fp32 adds per output (tests/fp32_bounds.py adds).
//
// LDS.  Every row (mid pixel, staged x pixel, weight row) is [h 32 | m 32 | l 32 | 16 pad] bf16 = 224 B = 56
// dwords, the pitch of halo_x3p.hip / stem_x3.hip.  Every fragment read of both stages is a ds_read_b128 by lane
// (col, kq) of row r0 + col at byte 16 kq of a plane: 16 consecutive rows per kq.  Row starts fall on banks
// 56 r mod 64 = 0, 56, 48, ..., 8, eight distinct 8-bank windows before they repeat, and the second eight rows of a
// 16-lane group of the read (tools/lds_bank_model.py G128 pairs lanes of two kq values) sit 16 B further on, in the
// half of the window the first eight leave free: 1.0 x the conflict-free cycles in that model, against 2.0 x for
// 192-, 208- and 240-byte rows.  The 8-byte plane stores of the two splits are the patterns of halo_x3p.hip.
// Stage 1's staging area (64 x rows + 32 W1 rows = 21.0 KB) and stage 2's two weight buffers (2 x min(c_, 64) rows:
// 14 / 28 / 28 KB) share one region, the 180 mid rows (39.4 KB) live beside it: 60.4 / 67.4 / 67.4 KB for c_ = 32 /
// 64 / 128, two workgroups per CU at every c_.
#include <stdexcept>
#include <string>

#include "launch.h"
#include "x3.h"

namespace arena {

namespace {

constexpr int BK_TH = 8, BK_TW = 16;                    // output tile
constexpr int BK_HC = BK_TW + 2, BK_HR = BK_TH + 2;     // its halo
constexpr int BK_HPIX = BK_HR * BK_HC;                  // 180 halo pixels
constexpr int BK_PASS = 64;                             // halo rows per stage-1 pass (one 16-row fragment per wave)
constexpr int BK_NPASS = (BK_HPIX + BK_PASS - 1) / BK_PASS;
constexpr int BK_P = 3 * 32 + 16;                       // bf16 per LDS row (224 B)
constexpr int BK_NT = 256;

__host__ __device__ constexpr int bk_ns(int C) { return C < 64 ? C : 64; }  // output channels per W2 stage
__host__ __device__ constexpr int bk_region(int C) {
  return (BK_PASS + 32) * BK_P > 2 * bk_ns(C) * BK_P ? (BK_PASS + 32) * BK_P : 2 * bk_ns(C) * BK_P;
}
__host__ __device__ constexpr int bk_lds_bytes(int C) { return (BK_HPIX * BK_P + bk_region(C)) * 2; }

int g_bk_cus = 0;  // compute units of the device (c3_bneck_x3_prepare)

}  // namespace

template <int C>
__global__ __launch_bounds__(BK_NT) void c3_bneck_x3_kernel(const BneckParams p, const int slices) {
  constexpr int NT = BK_NT, KC = C / 32, NF = C / 16, NS = bk_ns(C), NH = C / NS, NFS = NS / 16;
  constexpr int XI = BK_PASS * 8 / NT;             // staged x items (row, 4-channel group) per thread and stage
  constexpr int W1I = (32 * 12 + NT - 1) / NT;     // 16-B W1 pieces per thread and stage
  constexpr int W2I = (NS * 12 + NT - 1) / NT;     // 16-B W2 pieces per thread and stage
  constexpr int NST2 = 9 * NH;                     // W2 stages per mid chunk
  static_assert(C == 32 || C == 64 || C == 128, "c_ is 32, 64 or 128");
  extern __shared__ __attribute__((aligned(16))) bf16 bk_lds[];
  bf16* sM = bk_lds;                     // [BK_HPIX][BK_P] mid planes
  bf16* sX = bk_lds + BK_HPIX * BK_P;    // stage 1: [BK_PASS][BK_P] x planes
  bf16* sW1 = sX + BK_PASS * BK_P;       // stage 1: [32][BK_P] W1 rows
  bf16* sW2 = sX;                        // stage 2: [2][NS][BK_P] W2 rows (over sX / sW1)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int H = p.H, W = p.W;
  const int tiles_x = (W + BK_TW - 1) / BK_TW, tiles_y = (H + BK_TH - 1) / BK_TH;
  const int tiles = tiles_x * tiles_y;
  const int bx = xcd_remap(blockIdx.x, gridDim.x);
  const int b = bx / tiles;
  if (b >= live_batch(p.B, p.bdev)) return;
  const int t = bx - b * tiles;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int oy0 = ty * BK_TH, ox0 = tx * BK_TW;
  const int slice = blockIdx.y;
  const int mc_begin = slice * KC / slices, mc_end = (slice + 1) * KC / slices;  // this workgroup's mid chunks

  // raw buffer loads: an out-of-range offset (halo outside the map, rows past a pass) reads zeros; host: every
  // tensor < 2 GiB (c3_bneck_x3_supported)
  const float* x = p.x + p.x_coff;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(x), (short)0, (int)(((size_t)p.B * H * W - 1) * p.xs + C) * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t w1r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w1), (short)0, KC * C * 192, 0x00020000);
  const __amdgpu_buffer_rsrc_t w2r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w2), (short)0, 9 * KC * C * 192, 0x00020000);
  constexpr int kOob = 0x7fffffff & ~15;
  const size_t img = (size_t)b * H * W;

  // halo pixel hp (row-major in the 10 x 18 halo) -> inside the map?
  auto halo_in = [&](int hp, int& iy, int& ix) {
    const int hy = hp / BK_HC, hx = hp - hy * BK_HC;
    iy = oy0 - 1 + hy;
    ix = ox0 - 1 + hx;
    return hp < BK_HPIX && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
  };

  int x_off[XI];  // this pass's items: byte offset of (pixel, group) at channel 0, or kOob
  auto pass_offsets = [&](int ps) {
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      const int i = tid + NT * j;
      int iy, ix;
      const bool in = halo_in(ps * BK_PASS + (i >> 3), iy, ix);
      x_off[j] = in ? (int)(((img + (size_t)iy * W + ix) * p.xs + 4 * (i & 7)) * 4) : kOob;
    }
  };
  int w1_off[W1I], w1_dst[W1I], w2_off[W2I], w2_dst[W2I];  // per 16-B piece: byte offset in a stage's rows, LDS place
#pragma unroll
  for (int j = 0; j < W1I; ++j) {
    const int i = tid + NT * j, row = i / 12, piece = i - row * 12;
    w1_off[j] = i < 32 * 12 ? row * 192 + piece * 16 : kOob;
    w1_dst[j] = row * BK_P + piece * 8;
  }
#pragma unroll
  for (int j = 0; j < W2I; ++j) {
    const int i = tid + NT * j, row = i / 12, piece = i - row * 12;
    w2_off[j] = i < NS * 12 ? row * 192 + piece * 16 : kOob;
    w2_dst[j] = row * BK_P + piece * 8;
  }

  f32x4 rx[XI];
  u32x4 rw1[W1I], rw2[W2I];
  auto load_1 = [&](int mc, int kc) {  // x channels 32 kc .. + 31 of this pass's rows; W1 rows of mid chunk mc
#pragma unroll
    for (int j = 0; j < XI; ++j)
      rx[j] = __builtin_bit_cast(
          f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, x_off[j] != kOob ? x_off[j] + kc * 128 : kOob, 0, 0));
    const int step = (kc * C + mc * 32) * 192;  // wave-uniform
#pragma unroll
    for (int j = 0; j < W1I; ++j) rw1[j] = __builtin_amdgcn_raw_buffer_load_b128(w1r, w1_off[j], step, 0);
  };
  auto store_1 = [&]() {
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      const int i = tid + NT * j;
      bf16x4 h, m, l;
      x3_split4_pair(f32x2{rx[j][0], rx[j][1]}, f32x2{rx[j][2], rx[j][3]}, h, m, l);
      bf16* d = sX + (i >> 3) * BK_P + 4 * (i & 7);
      *(bf16x4*)d = h;
      *(bf16x4*)(d + 32) = m;
      *(bf16x4*)(d + 64) = l;
    }
#pragma unroll
    for (int j = 0; j < W1I; ++j)
      if (32 * 12 % NT == 0 || tid + NT * j < 32 * 12) *(u32x4*)(sW1 + w1_dst[j]) = rw1[j];
  };
  auto load_2 = [&](int mc, int st) {  // stage st = tap * NH + half: rows half * NS .. + NS - 1 of (tap, mc)
    const int tap = st / NH, half = st - tap * NH;
    const int step = ((tap * KC + mc) * C + half * NS) * 192;  // wave-uniform
#pragma unroll
    for (int j = 0; j < W2I; ++j) rw2[j] = __builtin_amdgcn_raw_buffer_load_b128(w2r, w2_off[j], step, 0);
  };
  auto store_2 = [&](int buf) {
#pragma unroll
    for (int j = 0; j < W2I; ++j)
      if (NS * 12 % NT == 0 || tid + NT * j < NS * 12) *(u32x4*)(sW2 + buf * NS * BK_P + w2_dst[j]) = rw2[j];
  };

  f32x4 acc[2][NF];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[f][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  pass_offsets(0);
  load_1(mc_begin, 0);
  for (int mc = mc_begin; mc < mc_end; ++mc) {
    // ---- stage 1: mid chunk mc on the halo, three passes of 64 rows
    for (int ps = 0; ps < BK_NPASS; ++ps) {
      f32x4 a1[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      for (int kc = 0; kc < KC; ++kc) {
        store_1();
        __syncthreads();
        // the next stage's global loads overlap this stage's MFMAs
        if (kc + 1 < KC) {
          load_1(mc, kc + 1);
        } else if (ps + 1 < BK_NPASS) {
          pass_offsets(ps + 1);
          load_1(mc, 0);
        } else {
          load_2(mc, 0);
        }
        const bf16* r = &sX[(wave * 16 + col) * BK_P + 8 * kq];
        const bf16x8 bh = *(const bf16x8*)r, bm = *(const bf16x8*)(r + 32), bl = *(const bf16x8*)(r + 64);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const bf16* wr = &sW1[(j * 16 + col) * BK_P + 8 * kq];
          a1[j] = x3_mfma(*(const bf16x8*)wr, *(const bf16x8*)(wr + 32), *(const bf16x8*)(wr + 64), bh, bm, bl, a1[j]);
        }
        __syncthreads();
      }
      // bias, SiLU, zero outside the map, split once into the mid planes (lane: halo pixel col, 4 channels)
      const int hp = ps * BK_PASS + wave * 16 + col;
      int iy, ix;
      const bool in = halo_in(hp, iy, ix);
      if (hp < BK_HPIX) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int ch = j * 16 + kq * 4;
          const float4 bias = *(const float4*)(p.b1 + mc * 32 + ch);
          const float v0 = in ? silu(a1[j][0] + bias.x) : 0.f, v1 = in ? silu(a1[j][1] + bias.y) : 0.f;
          const float v2 = in ? silu(a1[j][2] + bias.z) : 0.f, v3 = in ? silu(a1[j][3] + bias.w) : 0.f;
          bf16x4 h, m, l;
          x3_split4_pair(f32x2{v0, v1}, f32x2{v2, v3}, h, m, l);
          bf16* d = sM + hp * BK_P + ch;
          *(bf16x4*)d = h;
          *(bf16x4*)(d + 32) = m;
          *(bf16x4*)(d + 64) = l;
        }
      }
    }
    // ---- stage 2: the 3x3 over the mid planes, W2 stages double-buffered
    store_2(0);
    __syncthreads();  // the mid planes and stage 0 are in LDS; stage 1's staging area is free (barrier above)
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
      for (int half = 0; half < NH; ++half) {
        const int st = tap * NH + half;
        const int buf = st & 1;
        if (st + 1 < NST2) {
          load_2(mc, st + 1);
        } else if (mc + 1 < mc_end) {  // the next mid chunk's first stage-1 loads
          pass_offsets(0);
          load_1(mc + 1, 0);
        }
        bf16x8 bh[2], bm[2], bl[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const bf16* r = &sM[((wave + 4 * f + ky) * BK_HC + col + kx) * BK_P + 8 * kq];
          bh[f] = *(const bf16x8*)r;
          bm[f] = *(const bf16x8*)(r + 32);
          bl[f] = *(const bf16x8*)(r + 64);
        }
#pragma unroll
        for (int j = 0; j < NFS; ++j) {
          const bf16* r = &sW2[buf * NS * BK_P + (j * 16 + col) * BK_P + 8 * kq];
          const bf16x8 ah = *(const bf16x8*)r, am = *(const bf16x8*)(r + 32), al = *(const bf16x8*)(r + 64);
#pragma unroll
          for (int f = 0; f < 2; ++f)
            acc[f][half * NFS + j] = x3_mfma(ah, am, al, bh[f], bm[f], bl[f], acc[f][half * NFS + j]);
        }
        if (st + 1 < NST2) store_2(buf ^ 1);  // last read before the previous stage's barrier
        __syncthreads();
      }
    }
  }

  // ---- epilogue
  const int HW = H * W;
  const bool partial = slices > 1;
  float* ws = partial ? p.sk_ws + (size_t)slice * p.B * HW * C : nullptr;
  float* y = p.y + p.y_coff;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int cb = j * 16 + kq * 4;
    const float4 bias = *(const float4*)(p.b2 + cb);
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int oy = oy0 + wave + 4 * f, ox = ox0 + col;
      if (oy >= H || ox >= W) continue;
      const size_t pix = img + (size_t)oy * W + ox;
      if (partial) {  // raw partial sums: ws[slice][pixel][C]
        *(float4*)(ws + pix * C + cb) = make_float4(acc[f][j][0], acc[f][j][1], acc[f][j][2], acc[f][j][3]);
        continue;
      }
      float v[4] = {silu(acc[f][j][0] + bias.x), silu(acc[f][j][1] + bias.y), silu(acc[f][j][2] + bias.z),
                    silu(acc[f][j][3] + bias.w)};
      if (p.res) {
        const float4 rv = *(const float4*)(x + pix * p.xs + cb);
        v[0] += rv.x; v[1] += rv.y; v[2] += rv.z; v[3] += rv.w;
      }
      *(float4*)(y + pix * p.ys + cb) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

namespace {

template <int C>
void bk_launch(const BneckParams& p, int slices, hipStream_t s) {
  const int tiles = ((p.W + BK_TW - 1) / BK_TW) * ((p.H + BK_TH - 1) / BK_TH);
  hipLaunchKernelGGL((c3_bneck_x3_kernel<C>), dim3((unsigned)(p.B * tiles), (unsigned)slices), dim3(BK_NT),
                     bk_lds_bytes(C), s, p, slices);
}

// byte ranges [a, a + an) and [b, b + bn) of two channel slices with pixel strides as / bs: true unless the slices can
// be shown disjoint (separate memory, or the same pixel grid with channel windows that do not meet)
bool bk_overlap(const float* a, size_t an, int as, const float* b, size_t bn, int bs, int C) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  if (a0 + an * 4 <= b0 || b0 + bn * 4 <= a0) return false;
  if (as != bs || (a0 > b0 ? a0 - b0 : b0 - a0) % 4) return true;
  const size_t d = (a0 > b0 ? (a0 - b0) / 4 : as - ((b0 - a0) / 4) % as) % as;  // a's channel offset past b's
  return !(d >= (size_t)C && d + C <= (size_t)as);
}

}  // namespace

bool c3_bneck_x3_supported(int C, int B, int H, int W, int xs, int x_coff, int ys, int y_coff) {
  if (!(C == 32 || C == 64 || C == 128) || B < 1 || H < 1 || W < 1) return false;
  if (xs % 4 || ys % 4 || x_coff % 4 || y_coff % 4 || x_coff < 0 || y_coff < 0 || x_coff + C > xs || y_coff + C > ys)
    return false;
  const size_t lim = (1u << 31) - (1u << 20);
  return (size_t)B * H * W * xs * 4 < lim && (size_t)B * H * W * ys * 4 < lim;
}

// Slices for a bottleneck of c / 32 mid chunks over B x tiles workgroups: one once the grid fills the device,
// doubled below that while a slice still holds a whole chunk.
int c3_bneck_x3_slices(int C, int B, int H, int W) {
  const int tiles = ((W + BK_TW - 1) / BK_TW) * ((H + BK_TH - 1) / BK_TH);
  const int cus = g_bk_cus > 0 ? g_bk_cus : 256;
  int s = 1;
  while (2 * s <= C / 32 && (long)B * tiles * s < cus) s *= 2;
  return s;
}

int c3_bneck_x3(const BneckParams& p, hipStream_t s) {
  if (!c3_bneck_x3_supported(p.C, p.B, p.H, p.W, p.xs, p.x_coff, p.ys, p.y_coff))
    throw std::invalid_argument("c3_bneck_x3: c_ must be 32, 64 or 128, over 4-aligned channel slices of maps < 2 GiB");
  const size_t span = (size_t)p.B * p.H * p.W - 1;
  if (bk_overlap(p.x + p.x_coff, span * p.xs + p.C, p.xs, p.y + p.y_coff, span * p.ys + p.C, p.ys, p.C))
    throw std::invalid_argument("c3_bneck_x3: the destination slice overlaps the source slice (every workgroup reads "
                                "its neighbours' pixels)");
  const int kc = p.C / 32;
  int slices = p.slices > 0 ? p.slices : c3_bneck_x3_slices(p.C, p.B, p.H, p.W);
  if (slices > kc) throw std::invalid_argument("c3_bneck_x3: more slices than 32-channel mid chunks");
  if (p.slices <= 0)  // the rule never asks for more than the workspace holds
    while (slices > 1 && (p.sk_ws == nullptr || (int64_t)slices * (int64_t)(span + 1) * p.C * 4 > p.sk_ws_bytes))
      slices /= 2;
  if (slices > 1 && (p.sk_ws == nullptr || (int64_t)slices * (int64_t)(span + 1) * p.C * 4 > p.sk_ws_bytes))
    throw std::invalid_argument("c3_bneck_x3: the split-K workspace does not hold the forced slices");
  switch (p.C) {
    case 32: bk_launch<32>(p, slices, s); break;
    case 64: bk_launch<64>(p, slices, s); break;
    default: bk_launch<128>(p, slices, s); break;
  }
  if (slices > 1) {  // the x3g split-K second pass: sum in slice order, + b2, SiLU, + x
    ConvParams q{};
    q.B = p.B;
    q.Ho = p.H;
    q.Wo = p.W;
    q.Cout = q.Cout_pad = p.C;
    q.bias = p.b2;
    q.act = ACT_SILU;
    q.res = p.res ? p.x + p.x_coff : nullptr;
    q.rs = p.xs;
    q.y = p.y + p.y_coff;
    q.ys = p.ys;
    q.bdev = p.bdev;
    q.sk_ws = p.sk_ws;
    q.sk_splits = slices;
    x3g_sk_reduce(q, s);
  }
  return slices;
}

void c3_bneck_x3_prepare() {
  ARENA_HIP_CHECK(hipFuncSetAttribute((const void*)c3_bneck_x3_kernel<32>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      bk_lds_bytes(32)));
  ARENA_HIP_CHECK(hipFuncSetAttribute((const void*)c3_bneck_x3_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      bk_lds_bytes(64)));
  ARENA_HIP_CHECK(hipFuncSetAttribute((const void*)c3_bneck_x3_kernel<128>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      bk_lds_bytes(128)));
  int dev = 0, cus = 0;
  ARENA_HIP_CHECK(hipGetDevice(&dev));
  ARENA_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  g_bk_cus = cus;
}

}  // namespace arena
