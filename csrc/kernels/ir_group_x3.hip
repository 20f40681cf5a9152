// Fused MobileNetV2 inverted residual at fp32 accuracy for the stride-1 7x7 blocks (torchvision mobilenet_v2
// features[15..17]: 160 -> 960 -> 160 with residual, twice, and 160 -> 960 -> 320), split over GROUPS OF CROPS.
//
// The whole-map kernel (ir_crop_f32.hip) gives one workgroup a row band of one crop: at 7x7 that is 21-28 output
// pixels per pass over the block's 1.8-2.8 MB of split weights, and the planner leaves it off there (149 / 194 us
// fused against 97 / 120 us as expand GEMM + depthwise + project GEMM; engine/planner.py ir_crop_f32_policy).  Here
// a workgroup owns G consecutive crops, G x 49 pixels per weight pass (G = 4: 196), so the weight stream per pixel
// is 7-9 times smaller.  The arithmetic is ir_x3_kernel's, product chain by product chain in its K and chunk order
// (the two kernels give the same bits, tests/test_ir_group_gpu.py); where X lives and how far ahead the weights are
// staged differ, as the register budget below demands:
//
//   * one workgroup = G crops x one hidden slice, 8 waves; grid = ceil(B / G) x y_parts.  A group whose first crop
//     is at or past the live count returns; inside a live group the crops past the live count are padding: their X
//     is zero, their E pixels stay zero, their outputs are not stored;
//   * pixel tiles of 16 run over the group's G x 49 pixels, so a tile may straddle two crops; a lane derives
//     (crop, y, x) of its pixel once.  Stride 1: an output pixel is the input pixel, so wave w owns tiles w, w + 8
//     for the expand, the depthwise and the project (accumulators resident for the whole chunk loop): each
//     depthwise tile is computed once.  X of the first tile is split once and resident in registers; the part of X
//     that does not fit (a second tile, G = 4; two K-steps at 320 outputs) waits as fp32 in LDS and is split per
//     chunk;
//   * E (fp32, LDS) holds G separate 9x9 maps per 8-channel plane, each with its own zero border: the border is the
//     depthwise padding and keeps a crop's taps off its neighbour; odd-slot plane stride as in ir_x3_kernel;
//   * per chunk of 32 hidden channels: E = relu6(We . X + be) (x3 MFMA 16x16x32), barrier, D = relu6(dw3x3(E) + bd)
//     straight into the project B operand, acc += Wp . D, barrier; chunk weights fetched into registers one phase
//     ahead (We during the expand before, Wp during the depthwise + project before: one staging array live at a
//     time) and stored to LDS by all threads;
//   * y = acc + bp (+ x), NHWC fp32; hidden slices (x_parts / y_parts) as in ir_x3_kernel: partial sums added in
//     order while loading X and the residual, slice j > 0 stores its bare partial sum at channel offset j * oup.
//
// Registers decide G: at 512 threads a wave has 256 (VGPR + AGPR); a split X tile at 160 input channels is 60, an
// accumulator tile 4, the staging of one weight chunk 20 (36 for Wp at 320 outputs).  G = 4, 160 outputs: one X
// tile + 20 accumulator tiles + staging = 160, the second X tile in LDS.  320 outputs at G = 4 would need 40
// accumulator tiles and are instantiated at G = 2 only.  No instantiation uses scratch (228 / 253 / 252 VGPRs,
// profiles/r13_ir_group/README.md).
#include <stdexcept>
#include <string>

#include "launch.h"
#include "x3.h"

namespace arena {

namespace {

constexpr int IRG_THREADS = 512, IRG_WAVES = IRG_THREADS / 64;

// GC: crops per workgroup; NOT: oup_pad / 16.  7x7 map, stride 1, 160 input channels, hidden chunks of 32.
template <int GC, int NOT>
struct IrgGeom {
  static constexpr int HO = 7, HW = HO * HO, EW = HO + 2, KS = 5, INP = KS * 32, HC = 32;
  static constexpr int NPIX = GC * HW;                // pixels of a group
  static constexpr int NT = (NPIX + 15) / 16;         // pixel tiles (expand columns == project columns)
  static constexpr int TPW = (NT + IRG_WAVES - 1) / IRG_WAVES;  // pixel tiles per wave
  static constexpr int NEP = GC * EW * EW;            // E pixels: GC maps with their zero borders
  static constexpr int NKG = HC / 8;                  // 8-channel groups of a chunk
  static constexpr int EPS = (2 * NEP + 1) * 16;      // bytes per E channel-group plane (odd slot count)
  static constexpr int NHT = HC / 16;                 // expand hidden tiles per chunk
  static constexpr int WEB = 6 * INP + 32;            // bytes per We row: [h|m|l][INP] bf16 + pad
  static constexpr int WPB = 6 * HC + 32;             // bytes per Wp row: [h|m|l][HC] bf16 + pad
  static constexpr int E_BYTES = NKG * EPS, WE_BYTES = HC * WEB, WBE_BYTES = HC * 4;
  static constexpr int WP_BYTES = NOT * 16 * WPB, WD_BYTES = 10 * HC * 4;  // WD: 9 taps + bias
  // The part of X that does not fit the registers, as fp32 rows of an odd number of 16-byte slots: the first KL0
  // K-steps of a wave's first tile ([wave][16 pixels][32 KL0 + 4]; 320 outputs: 20 accumulator tiles and eight Wp
  // staging pieces leave room for three of the five split K-steps) and all of its second tile (tiles 8 .. NT - 1,
  // [tile][16 pixels][INP + 4])
  static constexpr int KL0 = NOT > 10 ? 2 : 0;
  static constexpr int XP0 = KL0 ? (KL0 * 32 + 4) * 4 : 0, X0_BYTES = IRG_WAVES * 16 * XP0;
  static constexpr int XSP = (INP + 4) * 4, XS_BYTES = (TPW > 1 ? NT - IRG_WAVES : 0) * 16 * XSP;
  static constexpr int LDS = E_BYTES + WE_BYTES + WBE_BYTES + WP_BYTES + WD_BYTES + X0_BYTES + XS_BYTES;
  static_assert(TPW <= 2, "a wave owns at most two pixel tiles");
  // 16-byte staging pieces of one chunk
  static constexpr int WE_PPR = 3 * INP / 8, WE_PIECES = HC * WE_PPR;  // the expand bias: 8 pieces of their own
  static constexpr int WP_PPR = 3 * HC / 8, WP_PIECES = NOT * 16 * WP_PPR;  // taps, dw bias: 80 pieces of their own
  static constexpr int WE_PT = (WE_PIECES + IRG_THREADS - 1) / IRG_THREADS;
  static constexpr int WP_PT = (WP_PIECES + IRG_THREADS - 1) / IRG_THREADS;
};

// Weights as ir_x3_kernel (IrParams.x3w, engine/planner.py::split_bf16x3): we bf16 [hid_pad][3][160] and wp bf16
// [oup_pad][3][hid_pad] (planes h, m, l), wd fp32 [9][hid_pad], biases fp32.
template <int GC, int NOT>
__global__ __launch_bounds__(IRG_THREADS) void ir_group_x3_kernel(const IrParams p) {
  using G = IrgGeom<GC, NOT>;
  constexpr int HW = G::HW, HO = G::HO, INP = G::INP, EW = G::EW, KS = G::KS, HC = G::HC, TPW = G::TPW;
  extern __shared__ __align__(16) uint8_t lds[];
  uint8_t* Es = lds;
  uint8_t* WEs = Es + G::E_BYTES;
  float* WBEs = (float*)(WEs + G::WE_BYTES);
  uint8_t* WPs = (uint8_t*)WBEs + G::WBE_BYTES;
  float* WDs = (float*)(WPs + G::WP_BYTES);  // [10][HC]: taps 0..8, bias
  uint8_t* Xs = (uint8_t*)WDs + G::WD_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int xparts = p.x_parts > 1 ? p.x_parts : 1, yparts = p.y_parts > 1 ? p.y_parts : 1;
  const int slice = blockIdx.x % yparts, b0 = (blockIdx.x / yparts) * GC;
  const int live = live_batch(p.B, p.bdev);
  if (b0 >= live) return;
  const float* __restrict__ x = (const float*)p.x;
  const bf16* __restrict__ we = (const bf16*)p.we;
  const bf16* __restrict__ wp = (const bf16*)p.wp;
  const float* __restrict__ wd = (const float*)p.wd;
  const int hid_pad = p.hid_pad, nch_all = hid_pad / HC;
  const int cb = slice * nch_all / yparts, ce = (slice + 1) * nch_all / yparts;  // this slice's hidden chunks

  // ---- chunk weight staging (global -> registers -> LDS by all threads).  Every global address is a uniform
  // base plus one 32-bit lane offset shared by all pieces of a thread (the We chunk is contiguous, piece e at
  // e * 16; Wp piece e is 16-byte part e % 4 of row-plane e / 4): per-piece 64-bit pointers, loop invariant and
  // kept live by the compiler, do not fit next to the resident X and accumulator tiles.  Plain unrolled loops
  // over native vectors; out-of-range slots re-read offset 0 (as ir_x3_kernel: anything else went to scratch).
  // The expand bias (8 pieces) rides with We, the taps and the depthwise bias (80 pieces) with Wp.
  const unsigned we_vo = tid * 16u, wp_vo = (unsigned)(tid >> 2) * hid_pad * 2u + (tid & 3) * 16u;
  const int bi = tid < 8 ? tid : 0, di = tid < 10 * HC / 4 ? tid : 0;  // bias piece; tap row di / 8, part di % 8
  const float* dsrc = (di / (HC / 4) < 9 ? wd + (size_t)(di / (HC / 4)) * hid_pad : p.bd) + 4 * (di % (HC / 4));
  u32x4 rwe[G::WE_PT], rwp[G::WP_PT], rbe, rwd;
#define IRG_FETCH_WE(h0_)                                                                       \
  {                                                                                             \
    const uint8_t* base = (const uint8_t*)(we + (size_t)(h0_) * (3 * INP));                     \
    _Pragma("unroll") for (int j = 0; j < G::WE_PT; ++j) {                                     \
      const bool in = IRG_THREADS * (j + 1) <= G::WE_PIECES || tid + IRG_THREADS * j < G::WE_PIECES; \
      rwe[j] = *(const u32x4*)(base + IRG_THREADS * 16 * j + (in ? we_vo : 0u));                \
    }                                                                                           \
    rbe = *(const u32x4*)(p.be + (h0_) + 4 * bi);                                               \
  }
#define IRG_STORE_WE()                                                                          \
  {                                                                                             \
    _Pragma("unroll") for (int j = 0; j < G::WE_PT; ++j) {                                     \
      const int e = tid + IRG_THREADS * j;                                                      \
      if (e < G::WE_PIECES) *(u32x4*)(WEs + e * 16 + (e / G::WE_PPR) * (G::WEB - G::WE_PPR * 16)) = rwe[j]; \
    }                                                                                           \
    if (tid < HC / 4) *(u32x4*)(WBEs + 4 * tid) = rbe;                                          \
  }
#define IRG_FETCH_WP(h0_, j0_, j1_)                                                             \
  {                                                                                             \
    const uint8_t* base = (const uint8_t*)(wp + (h0_));                                         \
    _Pragma("unroll") for (int j = (j0_); j < (j1_); ++j) {                                    \
      const bool in = IRG_THREADS * (j + 1) <= G::WP_PIECES || tid + IRG_THREADS * j < G::WP_PIECES; \
      rwp[j] = *(const u32x4*)(base + (size_t)(IRG_THREADS / 4 * j) * hid_pad * 2 + (in ? wp_vo : 0u)); \
    }                                                                                           \
    if ((j0_) == 0) rwd = *(const u32x4*)(dsrc + (h0_));                                        \
  }
#define IRG_STORE_WP(j0_, j1_)                                                                  \
  {                                                                                             \
    _Pragma("unroll") for (int j = (j0_); j < (j1_); ++j) {                                    \
      const int e = tid + IRG_THREADS * j;                                                      \
      if (e < G::WP_PIECES) *(u32x4*)(WPs + e * 16 + (e / G::WP_PPR) * (G::WPB - G::WP_PPR * 16)) = rwp[j]; \
    }                                                                                           \
    if ((j0_) == 0 && tid < 10 * HC / 4) *(u32x4*)(WDs + 4 * tid) = rwd;                        \
  }
  IRG_FETCH_WE(cb * HC)
  IRG_FETCH_WP(cb * HC, 0, G::WP_PT)

  // ---- E: zero everywhere (the borders and the padding crops' maps stay zero)
  for (int i = tid; i < G::E_BYTES / 16; i += IRG_THREADS) ((uint4*)Es)[i] = make_uint4(0u, 0u, 0u, 0u);

  // ---- this wave's pixel tiles (tile = wave + 8 t), the same pixels for the expand, the depthwise and the project.
  // The block input of the first tile is split once and stays in registers for the whole kernel (60); what does
  // not fit next to the accumulator tiles (a second tile at G = 4, two K-steps of the first at 320 outputs: IrgGeom)
  // is kept as fp32 in LDS, private to the wave, and read and split per chunk, the same planes every time.
  bf16x8 xh[KS], xm[KS], xl[KS];
  int pix_off[TPW];  // pixel index in x / y (crop * 49 + y * 7 + x), -1: no pixel, or a padding crop's
  int e_off[TPW];    // byte offset of the pixel in an E plane (a padding lane: the first pixel's, read only)
  uint8_t* xs0 = Xs + (wave * 16 + col) * G::XP0 + 8 * kq * 4;  // this lane's rows of the first / second tile in LDS
  uint8_t* xs1 = Xs + G::X0_BYTES + (wave * 16 + col) * G::XSP + 8 * kq * 4;
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int q = (wave + IRG_WAVES * t) * 16 + col;
    const int g = q / HW, r = q - g * HW;
    const bool ok = q < G::NPIX && b0 + g < live;
    const int qy = r / HO, qx = r - qy * HO;
    pix_off[t] = ok ? (b0 + g) * HW + r : -1;
    e_off[t] = ok ? ((g * EW + qy + 1) * EW + qx + 1) * 32 : (EW + 1) * 32;
    if (t > 0 && wave + IRG_WAVES * t >= G::NT) continue;  // no such tile: nothing to keep
    const float* src = x + (size_t)(ok ? pix_off[t] : b0 * HW) * p.x_cs;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = ks * 32 + 8 * kq;
      float v[8];
      const bool kk = ok && k < p.inp;
      float4 a = *(const float4*)(src + (kk ? k : 0)), c = *(const float4*)(src + (kk ? k + 4 : 0));
      for (int j = 1; j < xparts; ++j) {  // partial sums of a hidden-sliced producer, added in order
        const float* sj = src + j * p.inp + (kk ? k : 0);
        const float4 a2 = *(const float4*)sj, c2 = *(const float4*)(sj + 4);
        a.x += a2.x; a.y += a2.y; a.z += a2.z; a.w += a2.w;
        c.x += c2.x; c.y += c2.y; c.z += c2.z; c.w += c2.w;
      }
      if (!kk) a = c = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t == 0 && ks >= G::KL0) {
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = c.x; v[5] = c.y; v[6] = c.z; v[7] = c.w;
        x3_split8(v, xh[ks], xm[ks], xl[ks]);
      } else {
        uint8_t* xs = (t > 0 ? xs1 : xs0) + ks * 128;
        *(float4*)xs = a;
        *(float4*)(xs + 16) = c;
      }
    }
  }

  f32x4 acc[TPW][NOT];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int j = 0; j < NOT; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  IRG_STORE_WE()
  IRG_STORE_WP(0, G::WP_PT)
  if (ce - cb > 1) {
    IRG_FETCH_WE((cb + 1) * HC)
  }
  __syncthreads();

  for (int c = cb; c < ce; ++c) {
    // ---- expand: E[pix][chunk] = relu6(We[chunk] . X + be) for this wave's pixel tiles
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      if (wave + IRG_WAVES * t >= G::NT) continue;  // (a break would keep the loop from unrolling: arrays in scratch)
      f32x4 e[G::NHT];
#pragma unroll
      for (int ht = 0; ht < G::NHT; ++ht) e[ht] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {  // K ascending per hidden tile, as ir_x3_kernel
        bf16x8 bh = xh[ks], bm = xm[ks], bl = xl[ks];
        if (t > 0 || ks < G::KL0) {
          const uint8_t* xs = (t > 0 ? xs1 : xs0) + ks * 128;
          const float4 a = *(const float4*)xs, c = *(const float4*)(xs + 16);
          const float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
          x3_split8(v, bh, bm, bl);
        }
#pragma unroll
        for (int ht = 0; ht < G::NHT; ++ht) {
          const uint8_t* ra = WEs + (ht * 16 + col) * G::WEB + (ks * 32 + 8 * kq) * 2;
          e[ht] = x3_mfma(*(const bf16x8*)ra, *(const bf16x8*)(ra + INP * 2), *(const bf16x8*)(ra + INP * 4), bh, bm,
                          bl, e[ht]);
        }
      }
      if (pix_off[t] >= 0) {
#pragma unroll
        for (int ht = 0; ht < G::NHT; ++ht) {
          const int ch = ht * 16 + 4 * kq;
          const float4 be = *(const float4*)(WBEs + ch);
          const float4 v = make_float4(relu6f(e[ht][0] + be.x), relu6f(e[ht][1] + be.y), relu6f(e[ht][2] + be.z),
                                       relu6f(e[ht][3] + be.w));
          *(float4*)(Es + (ch >> 3) * G::EPS + e_off[t] + (ch & 7) * 4) = v;
        }
      }
    }
    __syncthreads();  // A: E complete; every wave is past its reads of We / be
    if (c + 1 < ce) {
      IRG_STORE_WE()
      __builtin_amdgcn_sched_barrier(0);  // likewise We before the Wp loads
      IRG_FETCH_WP((c + 1) * HC, 0, G::WP_PT)
    }

    // ---- depthwise (into the project B operand) + project; HC == 32: one K-step, lane's channel group = kq
    const float* wk = WDs + kq * 8;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      if (wave + IRG_WAVES * t >= G::NT) continue;  // (a break would keep the loop from unrolling: arrays in scratch)
      float a[8];
      {
        const float4 c0 = *(const float4*)(wk + 9 * HC), c1 = *(const float4*)(wk + 9 * HC + 4);
        a[0] = c0.x; a[1] = c0.y; a[2] = c0.z; a[3] = c0.w; a[4] = c1.x; a[5] = c1.y; a[6] = c1.z; a[7] = c1.w;
      }
      const uint8_t* eb = Es + kq * G::EPS + e_off[t] - (EW + 1) * 32;  // tap (0, 0)
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) {
        const uint8_t* ep = eb + ((tp / 3) * EW + (tp % 3)) * 32;
        const float4 v0 = *(const float4*)ep, v1 = *(const float4*)(ep + 16);
        const float4 w0 = *(const float4*)(wk + tp * HC), w1 = *(const float4*)(wk + tp * HC + 4);
        a[0] = fmaf(v0.x, w0.x, a[0]);
        a[1] = fmaf(v0.y, w0.y, a[1]);
        a[2] = fmaf(v0.z, w0.z, a[2]);
        a[3] = fmaf(v0.w, w0.w, a[3]);
        a[4] = fmaf(v1.x, w1.x, a[4]);
        a[5] = fmaf(v1.y, w1.y, a[5]);
        a[6] = fmaf(v1.z, w1.z, a[6]);
        a[7] = fmaf(v1.w, w1.w, a[7]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] = relu6f(a[i]);
      bf16x8 dh, dm, dl;
      x3_split8(a, dh, dm, dl);
#pragma unroll
      for (int j = 0; j < NOT; ++j) {
        const uint8_t* ra = WPs + (j * 16 + col) * G::WPB + 8 * kq * 2;
        acc[t][j] = x3_mfma(*(const bf16x8*)ra, *(const bf16x8*)(ra + HC * 2), *(const bf16x8*)(ra + HC * 4), dh, dm,
                            dl, acc[t][j]);
      }
    }
    __syncthreads();  // B: every wave is past its reads of E, Wp and the taps
    if (c + 1 < ce) {
      IRG_STORE_WP(0, G::WP_PT)
      __builtin_amdgcn_sched_barrier(0);  // the staged Wp leaves its registers before the next We loads take theirs
      if (c + 2 < ce) {
        IRG_FETCH_WE((c + 2) * HC)
      }
    }
  }

#undef IRG_FETCH_WE
#undef IRG_STORE_WE
#undef IRG_FETCH_WP
#undef IRG_STORE_WP

  // ---- epilogue: + bp (+ residual: the block input at the same pixel) -> NHWC fp32; a hidden slice > 0 writes
  // its bare partial sum at channel offset slice * oup; padding crops store nothing
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    if (pix_off[t] < 0) continue;
    float* yp = (float*)p.y + (size_t)pix_off[t] * p.y_cs + slice * p.oup;
    const float* xr = x + (size_t)pix_off[t] * p.x_cs;
#pragma unroll
    for (int j = 0; j < NOT; ++j) {
      const int co = j * 16 + 4 * kq;
      if (co >= p.oup) continue;
      float4 v = make_float4(acc[t][j][0], acc[t][j][1], acc[t][j][2], acc[t][j][3]);
      if (slice == 0) {
        const float4 bp = *(const float4*)(p.bp + co);
        v.x += bp.x;
        v.y += bp.y;
        v.z += bp.z;
        v.w += bp.w;
        if (p.res) {
          float4 r = *(const float4*)(xr + co);
          for (int jp = 1; jp < xparts; ++jp) {  // the block input: its partial sums in the load's order
            const float4 r2 = *(const float4*)(xr + jp * p.inp + co);
            r.x += r2.x; r.y += r2.y; r.z += r2.z; r.w += r2.w;
          }
          v.x += r.x;
          v.y += r.y;
          v.z += r.z;
          v.w += r.w;
        }
      }
      *(float4*)(yp + co) = v;
    }
  }
}

}  // namespace

// (crops per workgroup, oup_pad / 16)
#define ARENA_IRG_CONFIGS(X) \
  X(2, 10)                   \
  X(4, 10)                   \
  X(2, 20)

void ir_group_x3_prepare() {
#define X(GC_, NOT_)                                                                              \
  static_assert(IrgGeom<GC_, NOT_>::LDS <= 160 * 1024, "ir_group_x3: LDS budget");                \
  ARENA_HIP_CHECK(hipFuncSetAttribute((const void*)ir_group_x3_kernel<GC_, NOT_>,                 \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  ARENA_IRG_CONFIGS(X)
#undef X
}

// Shapes the group kernel takes (mirrored by engine/validate.py::ir_group_x3_supported): an expanding stride-1
// block on a 7x7 map, 160 padded input channels, 160 or 320 padded output channels.
bool ir_group_x3_supported(int H, int stride, int inp_pad, int hid_pad, int oup_pad, int expand) {
  return expand && H == 7 && stride == 1 && inp_pad == 160 && (oup_pad == 160 || oup_pad == 320) && hid_pad % 32 == 0;
}

// false, with nothing launched: not a group block (IrParams.group <= 1, no split-plane weights) or not its shape
bool ir_group_x3(const IrParams& p, hipStream_t s) {
  if (!p.x3w || p.group <= 1) return false;
  if (p.H != p.W || p.Ho != p.Wo || !ir_group_x3_supported(p.H, p.stride, p.inp_pad, p.hid_pad, p.oup_pad, p.expand))
    return false;
  if (p.inp % 8 || p.oup % 4 || p.inp > p.inp_pad || p.oup > p.oup_pad || p.x_cs % 4 || p.y_cs % 4)
    throw std::runtime_error("ir_group_x3: unsupported channel geometry");
  if (p.res && p.inp != p.oup) throw std::runtime_error("ir_group_x3: residual needs inp == oup");
  if (p.Ho != p.H) throw std::runtime_error("ir_group_x3: output size mismatch");
  if ((p.x_parts > 1 ? p.x_parts : 1) * p.inp > p.x_cs || (p.y_parts > 1 ? p.y_parts : 1) * p.oup > p.y_cs)
    throw std::runtime_error("ir_group_x3: partial-sum tensor narrower than its planned parts");
  const int xparts = irx_effective_parts(p.x_parts, p.B), yparts = irx_effective_parts(p.y_parts, p.B);
  IrParams q = p;  // the kernel reads the effective counts
  q.x_parts = xparts;
  q.y_parts = yparts;
  if (xparts > 8 || yparts > 8 || yparts > p.hid_pad / 32)
    throw std::runtime_error("ir_group_x3: unsupported partial-sum geometry (<= 8 parts, <= 1 per hidden chunk)");
#define X(GC_, NOT_)                                                                                       \
  if (p.group == GC_ && p.oup_pad == NOT_ * 16) {                                                          \
    if (p.B > 0)                                                                                           \
      hipLaunchKernelGGL((ir_group_x3_kernel<GC_, NOT_>), dim3((unsigned)((p.B + GC_ - 1) / GC_ * yparts)), \
                         dim3(IRG_THREADS), (IrgGeom<GC_, NOT_>::LDS), s, q);                              \
    return true;                                                                                           \
  }
  ARENA_IRG_CONFIGS(X)
#undef X
  throw std::runtime_error("ir_group_x3: no kernel for groups of " + std::to_string(p.group) + " crops at oup_pad " +
                           std::to_string(p.oup_pad));
}

}  // namespace arena
