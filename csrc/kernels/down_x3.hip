// fp32-accurate downsampling pair as one kernel: y = silu(W2 . silu(conv3x3_s2_p1(x, W1) + b1) + b2)  ("x3ds").
//
// In the fp32 detector each backbone downsampling conv (3x3 stride 2) is read only by the merged cv1|cv2 1x1 of the
// C3 block behind it.  Unfused the pair is two launches and the [B, Ho, Wo, C] map between them goes out to memory
// and comes straight back; here it only exists in registers and, one 32-channel chunk at a time, in LDS.
// (Cin, C) = (32, 64), (64, 128), (128, 256) with C2 == C; any H, W >= 1.
//
// Work split.  A workgroup (4 waves) owns one TH x TW tile of output pixels of one live image and ALL C mid channels
// and all C output channels of it.  Both GEMMs are split over the waves by channel: wave w owns channels
// [w C / 4, (w + 1) C / 4) as C / 64 fragments of 16, for every pixel fragment (M = TH TW pixels, row-major in the
// tile, 16 to a fragment), on v_mfma_f32_16x16x32_bf16 (A = 16 weight rows, B = 16 pixels): the 16-pixel fragment
// shape lets a 20-wide tile pack 4 x 20 = 80 pixels into five fragments without waste, which 32-pixel fragments do
// not.  Every wave therefore reads every pixel fragment but only its own weight rows: per 32-deep K step a wave
// issues 3 (MF + NS) ds_read_b128 for 6 MF NS MFMAs (NS = 1 or 2 weight fragments per stage).
//
//   GEMM 1  per 32-channel chunk of Cin: the tile's input patch, (2 TH + 1) x (2 TW + 1) pixels, is read from global
//           ONCE (raw buffer loads, zeros outside the map = the conv's padding), split ONCE per element into
//           h | m | l (x3.h) and stored to LDS; the nine taps then read the planes.  W1's K slices (tap, chunk) come
//           from the planner's pre-split operand (pack_conv_weight_x3: [tap Cin / 32 + chunk][C][192 B]) in stages of
//           64 NS rows (fragment j of every wave), double-buffered: stage s + 1 is loaded to registers before stage
//           s multiplies and lands in the other buffer after it, one barrier per stage.
//   mid     + b1, SiLU, one split of each mid value, stored to LDS in chunks of 32 mid channels (a chunk is the
//           fragment of one or two waves; 128 px x 256 ch x 6 B would not fit, a chunk of M x 32 does twice).
//   GEMM 2  per mid chunk: acc2 += W2[:, chunk] . mid[chunk], W2's slices from pack_pw_weight_x3's operand
//           ([C][h | m | l][C], K columns of each 16 in the order 0-3, 8-11, 4-7, 12-15, which is the order the mid
//           planes are stored in), staged and double-buffered exactly as W1's; the next chunk's mid planes are
//           written into the other mid buffer during the chunk's last stage.
//   out     + b2, SiLU, one 16-byte fp32 store per lane and fragment into the destination's channel slice.
//
// LDS.  Every row (patch pixel, mid pixel, weight row) is [h 32 | m 32 | l 32 | 16 pad] bf16 = 224 B = 56 dwords,
// the pitch of halo_x3p.hip / c3_bneck_x3.hip, and every fragment read is a ds_read_b128 by lane (col, kq) of row
// r0 + col at byte 16 kq of a plane.  Row starts fall on banks 56 r mod 64 = 0, 56, 48, ..., 8: eight distinct
// 8-bank windows before they repeat, and rows 8 .. 15 of a fragment read the other half of each window (the second
// kq of the 16-lane group, tools/lds_bank_model.py G128): conflict-free as long as the 16 lanes' rows are
// CONSECUTIVE.  A stride-2 tap over a row-major patch would read rows r0 + 2 col, i.e. banks 48 col mod 64: four
// windows, a 2-way conflict on every read.  So the patch rows are de-interleaved: patch row py holds its even
// columns first (TW + 1 of them), then the odd ones (TW), and tap kx of output column tx reads patch column
// 2 tx + kx = entry tx of the even run (kx 0), entry tx of the odd run (kx 1) or entry tx + 1 of the even run
// (kx 2): consecutive LDS rows for consecutive tx at every tap.  With TW = 16 a fragment is one output row and the
// argument holds as it stands.  With TW = 20 a fragment wraps into the next output row once (lanes c .. 15 sit
// 2 (2 TW + 1) - 20 = 62 rows further on, window index + 6 mod 8): up to four of the sixteen lanes meet a window
// that is already taken, at most a 2-way conflict on that read.  The 8-byte plane stores of the two splits are the
// patterns of halo_x3p.hip.  Patch (later the two mid buffers) + two weight buffers:
//   (2 TH + 1)(2 TW + 1) + 2 * 64 NS rows of 224 B = 93 / 121 / 121 KB (4 x 16), 109 / 137 / 137 KB (4 x 20),
//   73 / 101 / 101 KB (2 x 20) for C = 64 / 128 / 256: one workgroup per CU in every instantiation.
//
// Tiles (conv impl 145 + v, the X3HGPw numbers; any other impl: the launcher's rule).  v0 4 x 16, v1 4 x 20 (no
// waste on 20-wide maps), v2 2 x 20 (three fragments of 16 for 40 pixels: 320 workgroups at 32 x 20 x 20, where v1
// has 160).  The rule: among the tiles whose B x tiles fill the CUs the one with the fewest padded pixels, else the
// one with the most workgroups.
#include <stdexcept>
#include <string>
#include <type_traits>

#include "launch.h"
#include "x3.h"

namespace arena {

namespace {

constexpr int DS_NT = 256;
constexpr int DS_P = 3 * 32 + 16;  // bf16 per LDS row (224 B)
constexpr int DS_VARIANTS = 3;
constexpr int DS_TH[DS_VARIANTS] = {4, 4, 2}, DS_TW[DS_VARIANTS] = {16, 20, 20};

__host__ __device__ constexpr int ds_ns(int C) { return C >= 128 ? 2 : 1; }  // weight fragments per wave and stage
__host__ __device__ constexpr int ds_patch_rows(int TH, int TW) { return (2 * TH + 1) * (2 * TW + 1); }
__host__ __device__ constexpr int ds_lds_bytes(int C, int TH, int TW) {
  return (ds_patch_rows(TH, TW) + 2 * 64 * ds_ns(C)) * DS_P * 2;
}

int g_ds_cus = 0;  // compute units of the device (down_x3_prepare)

}  // namespace

template <int CIN, int C, int TH, int TW>
__global__ __launch_bounds__(DS_NT) void down_x3_kernel(const ConvParams p) {
  constexpr int NT = DS_NT, M = TH * TW, MF = (M + 15) / 16, PW = 2 * TW + 1, PR = ds_patch_rows(TH, TW);
  constexpr int KC1 = CIN / 32, KC2 = C / 32, CW = C / 4, NFW = C / 64, NS = ds_ns(C), NH = NFW / NS;
  constexpr int WR = 64 * NS;            // weight rows per stage
  constexpr int WI = WR * 12 / NT;       // 16-byte weight pieces per thread and stage
  constexpr int PI = (PR * 8 + NT - 1) / NT;  // patch items (pixel, 4-channel group) per thread and Cin chunk
  constexpr int NST1 = KC1 * 9 * NH;
  static_assert(WR * 12 % NT == 0 && 2 * MF * 16 <= PR && NFW % NS == 0, "stage / mid buffer geometry");
  extern __shared__ __attribute__((aligned(16))) bf16 ds_lds[];
  bf16* sP = ds_lds;             // GEMM 1: [PR][DS_P] patch planes; GEMM 2: [2][MF * 16][DS_P] mid planes
  bf16* sW = ds_lds + PR * DS_P;  // [2][WR][DS_P] weight rows

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int H = p.H, W = p.W, Ho = p.Ho, Wo = p.Wo;
  const int tiles_x = (Wo + TW - 1) / TW, tiles_y = (Ho + TH - 1) / TH;
  const int tiles = tiles_x * tiles_y;
  const int bx = xcd_remap(blockIdx.x, gridDim.x);
  const int b = bx / tiles;
  if (b >= live_batch(p.B, p.bdev)) return;
  const int t = bx - b * tiles;
  const int tyi = t / tiles_x, txi = t - tyi * tiles_x;
  const int oy0 = tyi * TH, ox0 = txi * TW;

  // raw buffer loads: an out-of-range offset (padding, rows past the patch) reads zeros; host: every tensor < 2 GiB
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.x), (short)0, (int)(((size_t)p.B * H * W - 1) * p.xs + CIN) * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t w1r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w3), (short)0, 9 * KC1 * C * 192, 0x00020000);
  const __amdgpu_buffer_rsrc_t w2r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.pw_w), (short)0, C * 3 * C * 2, 0x00020000);
  constexpr int kOob = 0x7fffffff & ~15;
  const size_t img = (size_t)b * H * W;

  // ---- the patch of Cin chunk kc: one global read and one split per element
  auto fill_patch = [&](int kc) {
    for (int j0 = 0; j0 < PI; j0 += 4) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = tid + NT * (j0 + u), lr = i >> 3;
        const int py = lr / PW, rem = lr - py * PW;
        const int pc = rem <= TW ? 2 * rem : 2 * (rem - TW - 1) + 1;  // even columns first, then the odd ones
        const int iy = 2 * oy0 - 1 + py, ix = 2 * ox0 - 1 + pc;
        const bool in = lr < PR && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        const int off = in ? (int)(((img + (size_t)iy * W + ix) * p.xs + kc * 32 + 4 * (i & 7)) * 4) : kOob;
        v[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = tid + NT * (j0 + u), lr = i >> 3;
        if (lr >= PR) continue;
        bf16x4 h, m, l;
        x3_split4_pair(f32x2{v[u][0], v[u][1]}, f32x2{v[u][2], v[u][3]}, h, m, l);
        bf16* d = sP + lr * DS_P + 4 * (i & 7);
        *(bf16x4*)d = h;
        *(bf16x4*)(d + 32) = m;
        *(bf16x4*)(d + 64) = l;
      }
    }
  };

  // ---- weight stages: stage row sr = (wave w, fragment j, row r) is channel w CW + (half NS + j) 16 + r
  int w_ch[WI], w_piece[WI], w_dst[WI];
#pragma unroll
  for (int j = 0; j < WI; ++j) {
    const int i = tid + NT * j, sr = i / 12;
    w_piece[j] = i - sr * 12;
    w_ch[j] = (sr / (16 * NS)) * CW + (sr % (16 * NS));
    w_dst[j] = sr * DS_P + w_piece[j] * 8;
  }
  u32x4 rw[WI];
  auto load_w1 = [&](int st) {  // st = (kc * 9 + tap) * NH + half; w3 rows [(tap KC1 + kc)][C][192 B]
    const int half = st % NH, kt = st / NH, kc = kt / 9, tap = kt - kc * 9;
    const int step = ((tap * KC1 + kc) * C + half * NS * 16) * 192;  // wave-uniform
#pragma unroll
    for (int j = 0; j < WI; ++j)
      rw[j] = __builtin_amdgcn_raw_buffer_load_b128(w1r, w_ch[j] * 192 + w_piece[j] * 16, step, 0);
  };
  auto load_w2 = [&](int c, int half) {  // W2 rows [C][h | m | l][C]: 64 B of each plane at mid chunk c
    const int step = half * NS * 16 * (3 * C * 2) + c * 64;  // wave-uniform
#pragma unroll
    for (int j = 0; j < WI; ++j)
      rw[j] = __builtin_amdgcn_raw_buffer_load_b128(
          w2r, w_ch[j] * (3 * C * 2) + (w_piece[j] >> 2) * (C * 2) + (w_piece[j] & 3) * 16, step, 0);
  };
  auto store_w = [&](int buf) {
#pragma unroll
    for (int j = 0; j < WI; ++j) *(u32x4*)(sW + buf * WR * DS_P + w_dst[j]) = rw[j];
  };

  // this lane's pixel of every fragment (past M: the last pixel again, never stored)
  int prow[MF];
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    const int pi = f * 16 + col < M ? f * 16 + col : M - 1;
    const int ty = pi / TW, tx = pi - ty * TW;
    prow[f] = 2 * ty * PW + tx;
  }

  f32x4 acc[MF][NFW];
#pragma unroll
  for (int f = 0; f < MF; ++f)
#pragma unroll
    for (int j = 0; j < NFW; ++j) acc[f][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- GEMM 1: the 3x3 stride-2 conv
  load_w1(0);
  for (int kc = 0; kc < KC1; ++kc) {
    fill_patch(kc);  // the last stage's barrier freed the patch
    if (kc == 0) store_w(0);
    __syncthreads();
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - ky * 3;
      const int toff = ky * PW + (kx == 1 ? TW + 1 : kx >> 1);
#pragma unroll
      for (int half = 0; half < NH; ++half) {
        const int st = (kc * 9 + tap) * NH + half, buf = st & 1;
        if (st + 1 < NST1) load_w1(st + 1);
        bf16x8 bh[MF], bm[MF], bl[MF];
#pragma unroll
        for (int f = 0; f < MF; ++f) {
          const bf16* r = &sP[(prow[f] + toff) * DS_P + 8 * kq];
          bh[f] = *(const bf16x8*)r;
          bm[f] = *(const bf16x8*)(r + 32);
          bl[f] = *(const bf16x8*)(r + 64);
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          const bf16* r = &sW[buf * WR * DS_P + ((wave * NS + j) * 16 + col) * DS_P + 8 * kq];
          const bf16x8 ah = *(const bf16x8*)r, am = *(const bf16x8*)(r + 32), al = *(const bf16x8*)(r + 64);
#pragma unroll
          for (int f = 0; f < MF; ++f)
            acc[f][half * NS + j] = x3_mfma(ah, am, al, bh[f], bm[f], bl[f], acc[f][half * NS + j]);
        }
        if (st + 1 < NST1) store_w(buf ^ 1);  // last read before the previous stage's barrier
        __syncthreads();
      }
    }
  }

  // ---- mid: + b1, SiLU, one split; chunk c = mid channels 32 c .. 32 c + 31 = two fragments of their owner waves
  f32x4 mid[MF][NFW];
#pragma unroll
  for (int j = 0; j < NFW; ++j) {
    const float4 bias = *(const float4*)(p.bias + wave * CW + j * 16 + 4 * kq);
#pragma unroll
    for (int f = 0; f < MF; ++f) {
      mid[f][j] = f32x4{silu(acc[f][j][0] + bias.x), silu(acc[f][j][1] + bias.y), silu(acc[f][j][2] + bias.z),
                        silu(acc[f][j][3] + bias.w)};
      acc[f][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  auto write_mid = [&](auto cc) {
    constexpr int c = decltype(cc)::value;
    bf16* sM = sP + (c & 1) * MF * 16 * DS_P;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int ch = 32 * c + 16 * g;       // first mid channel of the fragment
      if (wave != ch / CW) continue;        // wave-uniform
      const int jf = (ch % CW) / 16;
      const int kcol = 16 * g + 8 * (kq & 1) + 4 * (kq >> 1);  // pack_pw_weight_x3's column of channel 4 kq
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        bf16x4 h, m, l;
        const f32x4 v = mid[f][jf];
        x3_split4_pair(f32x2{v[0], v[1]}, f32x2{v[2], v[3]}, h, m, l);
        bf16* d = sM + (f * 16 + col) * DS_P + kcol;
        *(bf16x4*)d = h;
        *(bf16x4*)(d + 32) = m;
        *(bf16x4*)(d + 64) = l;
      }
    }
  };

  // ---- GEMM 2: the 1x1 over the mid chunks (the barrier that ended GEMM 1 freed the patch and both weight buffers)
  write_mid(std::integral_constant<int, 0>{});
  load_w2(0, 0);
  store_w(0);
  __syncthreads();
  auto gemm2 = [&](auto cc, auto self) {
    constexpr int c = decltype(cc)::value;
    if constexpr (c < KC2) {
      const bf16* sM = sP + (c & 1) * MF * 16 * DS_P;
#pragma unroll
      for (int half = 0; half < NH; ++half) {
        const int st = c * NH + half, buf = st & 1;
        const bool more = st + 1 < KC2 * NH;
        if (more) load_w2((st + 1) / NH, (st + 1) % NH);
        bf16x8 bh[MF], bm[MF], bl[MF];
#pragma unroll
        for (int f = 0; f < MF; ++f) {
          const bf16* r = &sM[(f * 16 + col) * DS_P + 8 * kq];
          bh[f] = *(const bf16x8*)r;
          bm[f] = *(const bf16x8*)(r + 32);
          bl[f] = *(const bf16x8*)(r + 64);
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          const bf16* r = &sW[buf * WR * DS_P + ((wave * NS + j) * 16 + col) * DS_P + 8 * kq];
          const bf16x8 ah = *(const bf16x8*)r, am = *(const bf16x8*)(r + 32), al = *(const bf16x8*)(r + 64);
#pragma unroll
          for (int f = 0; f < MF; ++f)
            acc[f][half * NS + j] = x3_mfma(ah, am, al, bh[f], bm[f], bl[f], acc[f][half * NS + j]);
        }
        if (more) store_w(buf ^ 1);
        if constexpr (c + 1 < KC2)
          if (half == NH - 1) write_mid(std::integral_constant<int, c + 1>{});  // read last during chunk c - 1
        __syncthreads();
      }
      self(std::integral_constant<int, c + 1>{}, self);
    }
  };
  gemm2(std::integral_constant<int, 0>{}, gemm2);

  // ---- out: + b2, SiLU, 16-byte stores into the destination's channel slice
  float* y = (float*)p.pw_y;
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    const int pi = f * 16 + col;
    const int ty = pi / TW, tx = pi - ty * TW;
    const int oy = oy0 + ty, ox = ox0 + tx;
    if (pi >= M || oy >= Ho || ox >= Wo) continue;
    const size_t pix = ((size_t)b * Ho + oy) * Wo + ox;
#pragma unroll
    for (int j = 0; j < NFW; ++j) {
      const int ch = wave * CW + j * 16 + 4 * kq;
      const float4 bias = *(const float4*)(p.pw_bias + ch);
      *(float4*)(y + pix * p.pw_ys + ch) = make_float4(silu(acc[f][j][0] + bias.x), silu(acc[f][j][1] + bias.y),
                                                       silu(acc[f][j][2] + bias.z), silu(acc[f][j][3] + bias.w));
    }
  }
}

namespace {

template <int CIN, int C, int TH, int TW>
void ds_launch(const ConvParams& p, hipStream_t s) {
  const int tiles = ((p.Wo + TW - 1) / TW) * ((p.Ho + TH - 1) / TH);
  hipLaunchKernelGGL((down_x3_kernel<CIN, C, TH, TW>), dim3((unsigned)(p.B * tiles)), dim3(DS_NT),
                     ds_lds_bytes(C, TH, TW), s, p);
}

template <int CIN, int C>
void ds_launch_v(const ConvParams& p, int v, hipStream_t s) {
  switch (v) {
    case 0: ds_launch<CIN, C, 4, 16>(p, s); break;
    case 1: ds_launch<CIN, C, 4, 20>(p, s); break;
    default: ds_launch<CIN, C, 2, 20>(p, s); break;
  }
}

template <int CIN, int C>
void ds_prepare_c() {
  ARENA_HIP_CHECK(hipFuncSetAttribute((const void*)down_x3_kernel<CIN, C, 4, 16>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, ds_lds_bytes(C, 4, 16)));
  ARENA_HIP_CHECK(hipFuncSetAttribute((const void*)down_x3_kernel<CIN, C, 4, 20>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, ds_lds_bytes(C, 4, 20)));
  ARENA_HIP_CHECK(hipFuncSetAttribute((const void*)down_x3_kernel<CIN, C, 2, 20>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, ds_lds_bytes(C, 2, 20)));
}

}  // namespace

int down_x3_variants() { return DS_VARIANTS; }

// The launcher's tile for B images of Ho x Wo outputs: among the tiles whose B x tiles fill the CUs the one with the
// fewest padded pixels (tiles x fragments x 16), else the one with the most workgroups (ties: fewer padded pixels).
int down_x3_tile(int B, int Ho, int Wo) {
  const long cus = g_ds_cus > 0 ? g_ds_cus : 256;
  int best = 0;
  long best_wg = -1, best_px = 0;
  for (int v = 0; v < DS_VARIANTS; ++v) {
    const long tiles = (long)((Wo + DS_TW[v] - 1) / DS_TW[v]) * ((Ho + DS_TH[v] - 1) / DS_TH[v]);
    const long wg = (long)B * tiles, px = tiles * ((DS_TH[v] * DS_TW[v] + 15) / 16 * 16);
    const bool full = wg >= cus, best_full = best_wg >= cus;
    const bool better = best_wg < 0 || (full && !best_full) || (full && best_full && px < best_px) ||
                        (!full && !best_full && (wg > best_wg || (wg == best_wg && px < best_px)));
    if (better) best = v, best_wg = wg, best_px = px;
  }
  return best;
}

bool down_x3_supported(const ConvParams& p) {
  const bool pair = (p.Cin == 32 && p.Cout == 64) || (p.Cin == 64 && p.Cout == 128) || (p.Cin == 128 && p.Cout == 256);
  if (!pair || p.pw_cout != p.Cout || p.pw_kpad != p.Cout || p.Cout_pad != p.Cout) return false;
  if (p.KH != 3 || p.KW != 3 || p.stride != 2 || p.pad_t != 1 || p.pad_l != 1 || p.B < 1 || p.H < 1 || p.W < 1 ||
      p.Ho != (p.H - 1) / 2 + 1 || p.Wo != (p.W - 1) / 2 + 1)
    return false;
  if (p.act != ACT_SILU || p.pw_act != ACT_SILU) return false;  // SiLU after both convs
  if (p.res != nullptr || p.y2 != nullptr || p.gate != nullptr || p.marks != nullptr || p.n_lo != 0 || p.n_hi != 0 ||
      p.lb_meta != nullptr || p.x_planes != 0 || p.y3 != nullptr)
    return false;
  if (p.x == nullptr || p.w3 == nullptr || p.bias == nullptr || p.pw_w == nullptr || p.pw_bias == nullptr ||
      p.pw_y == nullptr)
    return false;
  if (p.xs % 4 || p.pw_ys % 4 || p.xs < p.Cin || p.pw_ys < p.Cout || (uintptr_t)p.x % 16 || (uintptr_t)p.pw_y % 16 ||
      (uintptr_t)p.w3 % 16 || (uintptr_t)p.pw_w % 16 || (uintptr_t)p.bias % 16 || (uintptr_t)p.pw_bias % 16)
    return false;
  const size_t lim = (1u << 31) - (1u << 20);
  return (size_t)p.B * p.H * p.W * p.xs * 4 < lim && (size_t)p.B * p.Ho * p.Wo * p.pw_ys * 4 < lim;
}

int conv_down_x3(const ConvParams& p, hipStream_t s) {
  if (!down_x3_supported(p))
    throw std::invalid_argument(
        "down_x3: needs a 3x3 stride-2 pad-1 fp32 conv (Cin, C) = (32, 64), (64, 128) or (128, 256) with SiLU, pre-split "
        "weights and a fused 1x1 C -> C with SiLU, over 4-aligned channel slices of maps < 2 GiB");
  // every workgroup reads its neighbours' input pixels: the two byte ranges must not meet
  const uintptr_t x0 = (uintptr_t)p.x, x1 = x0 + (((size_t)p.B * p.H * p.W - 1) * p.xs + p.Cin) * 4;
  const uintptr_t y0 = (uintptr_t)p.pw_y, y1 = y0 + (((size_t)p.B * p.Ho * p.Wo - 1) * p.pw_ys + p.Cout) * 4;
  if (x0 < y1 && y0 < x1) throw std::invalid_argument("down_x3: the destination overlaps the source");
  const int v = f32_conv_impl_in(p.impl, F32Family::X3HGPw) && p.impl - kF32X3HGPw < DS_VARIANTS
                    ? p.impl - kF32X3HGPw
                    : down_x3_tile(p.B, p.Ho, p.Wo);
  switch (p.Cin) {
    case 32: ds_launch_v<32, 64>(p, v, s); break;
    case 64: ds_launch_v<64, 128>(p, v, s); break;
    default: ds_launch_v<128, 256>(p, v, s); break;
  }
  return v;
}

void down_x3_prepare() {
  ds_prepare_c<32, 64>();
  ds_prepare_c<64, 128>();
  ds_prepare_c<128, 256>();
  int dev = 0, cus = 0;
  ARENA_HIP_CHECK(hipGetDevice(&dev));
  ARENA_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  g_ds_cus = cus;
}

}  // namespace arena
