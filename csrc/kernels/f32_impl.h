// The fp32 conv kernel families: the one definition of the ConvParams.impl numbers of fp32 convs, which
// data/tuning/conv_tuning.json persists.  Host-only (no HIP): conv2d_f32's dispatch (conv_f32.hip), the executor's
// table check and autotune candidates (runtime/executor.cpp) and csrc/tests/f32_impl_check.cpp all read this table.
#pragma once
#include <array>
#include <cstdint>

namespace arena {

// variants -> candidate mask (bit v = variant v of the family)
template <class... V>
constexpr uint32_t f32_vs(V... v) {
  return ((1u << v) | ... | 0u);
}
constexpr uint32_t f32_all(int n) { return (1u << n) - 1u; }

// X(name, first impl, variants, variants autotune tries, what conv2d_f32 throws when the conv does not fit).
// Impl first + v runs variant v.  The rows stand in autotune's candidate order; 0 / 1 / 2 never reject a conv.
#define F32_CONV_FAMILIES(X)                                                                                          \
  X(Policy, 0, 1, f32_all(1), "")  /* FC / 3x3 halo / LDS tile by shape, or direct with ARENA_F32_CONV=direct */      \
  X(Direct, 1, 1, 0, "")           /* exact fp32, direct global->VGPR loads */                                        \
  X(Lds, 2, 1, 0, "")              /* exact fp32, 3x3 halo tiles or LDS implicit GEMM, tile by channel count */       \
  /* exact-fp32 LDS implicit-GEMM tile variants (conv_f32.hip LDS_VARIANTS) */                                        \
  X(LdsTile, 10, 16, f32_vs(2, 3, 4, 7, 9, 10, 11, 13, 14), "conv2d_f32: unknown variant")                            \
  X(Halo, 100, 1, f32_all(1), "conv2d_f32: not a halo-eligible conv")  /* exact-fp32 3x3 halo tiles */                \
  /* x3: fp32-accurate triple-bf16-split implicit GEMM tile variants (conv_f32.hip X3_VARIANTS) */                    \
  X(X3, 40, 12, f32_vs(0, 1, 4, 5, 6, 7, 8), "conv2d_f32: unknown x3 variant")                                        \
  /* x3 3x3 stride-1 halo tiles of 8 x 16 pixels; with 48-channel tiles; with 32-channel tiles */                     \
  X(X3Halo, 101, 1, f32_all(1), "conv2d_f32: not an x3-halo-eligible conv")                                           \
  X(X3HaloN3, 102, 1, f32_all(1), "conv2d_f32: not an x3-halo-eligible conv")                                         \
  X(X3HaloN2, 103, 1, f32_all(1), "conv2d_f32: not an x3-halo-eligible conv")                                         \
  /* x3 weight-stationary streaming conv; with 32-channel tiles */                                                    \
  X(Stream, 104, 1, f32_all(1), "conv2d_f32: not a stream-eligible conv (Cin % 8, Kpad <= 192)")                      \
  X(StreamN2, 105, 1, f32_all(1), "conv2d_f32: not a stream-eligible conv (Cin % 8, Kpad <= 192)")                    \
  /* exact-fp32 split-K FC over a 1x1 map (fc_splitk.hip) */                                                          \
  X(Fc, 106, 1, f32_all(1), "conv2d_f32: not an FC-eligible conv (1x1 map, Kpad 1280)")                               \
  /* streaming small-K conv on exact fp32 MFMA (no split) */                                                          \
  X(StreamExact, 107, 1, f32_all(1), "conv2d_f32: not a stream-eligible conv (Cin % 4, Kpad <= 192)")                 \
  /* x3 halo tiles of 16 x 16 pixels (8 waves); with 48-channel tiles */                                              \
  X(X3Halo16, 108, 1, f32_all(1), "conv2d_f32: not an x3-halo-eligible conv")                                         \
  X(X3Halo16N3, 109, 1, f32_all(1), "conv2d_f32: not an x3-halo-eligible conv")                                       \
  /* x3 3x3 stride-1 conv over exactly 16 input channels (s2d stems; the one kernel with a letterbox source) */       \
  X(X3H16, 110, 1, f32_all(1), "conv2d_f32: not an x3-h16-eligible conv (3x3 s1 over 16 channels)")                   \
  /* x3g: 32x32x16 MFMA implicit GEMM over pre-split weights (gemm_x3.hip XG_VARIANTS; v >= 10: v - 10 with the     \
     interleaved schedule); tried: the variants that won a layer in tools/bench_x3g.py */                             \
  X(X3G, 111, 20, f32_vs(5, 6, 7, 9, 15, 16, 17, 19),                                                                 \
    "conv2d_f32: not an x3g-eligible conv (needs pre-split weights)")                                                 \
  /* x3hg: 3x3 stride-1 halo tiles on 32x32x16 MFMAs over the same weights (halo_x3g.hip HG_VARIANTS) */              \
  X(X3HG, 131, 14, f32_vs(0, 1, 2, 4, 6, 7, 8, 9, 10),                                                                \
    "conv2d_f32: not an x3hg-eligible conv (3x3 s1 with pre-split weights)")                                          \
  /* ... with the Detect head's final 1x1 fused into the epilogue (ConvParams.pw_*; HG_PW_VARIANTS 0..5), and two    \
     more such tiles of 8 x 8 pixels on 2 waves for buckets 1 / 2 (HG_PW_VARIANTS 6, 7) */                            \
  X(X3HGPw, 145, 6, f32_all(6), "conv2d_f32: a fused pointwise epilogue needs an x3hg-pw variant that fits the conv") \
  X(X3HGPwSmall, 181, 2, f32_all(2),                                                                                  \
    "conv2d_f32: a fused pointwise epilogue needs an x3hg-pw variant that fits the conv")                             \
  /* x3hr: the x3hg tiles with per-wave register weights (HR_VARIANTS); and with the fused 1x1 (HR_PW_VARIANTS) */    \
  X(X3HR, 151, 10, f32_all(10), "conv2d_f32: not an x3hr-eligible conv (3x3 s1 with pre-split weights)")              \
  X(X3HRPw, 161, 6, f32_all(6), "conv2d_f32: a fused pointwise epilogue needs an x3hr-pw variant that fits the conv") \
  /* x3hp: the 16x16x32 halo tiles of X3Halo* over the pre-split weights (halo_x3p.hip HP_VARIANTS), bit-identical   \
     to impl 101 / 102 / 103 / 108 / 109 on every conv they take; variant 9 serves the head split only */             \
  X(X3HP, 191, 10, f32_all(9), "conv2d_f32: not an x3hp-eligible conv (3x3 s1 with pre-split weights)")               \
  /* split-K x3g for small grids (XG_SK_VARIANTS: tile x splits); needs ConvParams.sk_ws */                           \
  X(X3GSK, 171, 9, f32_all(9), "conv2d_f32: not a split-K x3g-eligible conv (pre-split weights, workspace)")

enum class F32Family {
#define F32_FAMILY_ID(name, first, count, tuned, reject) name,
  F32_CONV_FAMILIES(F32_FAMILY_ID)
#undef F32_FAMILY_ID
  Invalid
};

struct F32FamilyRow {
  const char* name;
  int first, count;
  uint32_t tuned;
  const char* reject;
};
inline constexpr F32FamilyRow kF32Families[] = {
#define F32_FAMILY_ROW(name, first, count, tuned, reject) {#name, first, count, tuned, reject},
    F32_CONV_FAMILIES(F32_FAMILY_ROW)
#undef F32_FAMILY_ROW
};
constexpr int kF32FamilyCount = (int)(sizeof(kF32Families) / sizeof(kF32Families[0]));

// kF32<name>: the family's first impl, kF32<name>Variants: its variant count
#define F32_FAMILY_ALIAS(name, first, count, tuned, reject) constexpr int kF32##name = first, kF32##name##Variants = count;
F32_CONV_FAMILIES(F32_FAMILY_ALIAS)
#undef F32_FAMILY_ALIAS

constexpr const F32FamilyRow& f32_family(F32Family f) { return kF32Families[(int)f]; }

constexpr bool f32_conv_impl_in(int impl, F32Family f) {
  return impl >= f32_family(f).first && impl < f32_family(f).first + f32_family(f).count;
}

// family and variant of an impl; {Invalid, 0} for a number that no family owns
struct F32Impl {
  F32Family family;
  int v;
};
constexpr F32Impl f32_conv_impl_find(int impl) {
  for (int f = 0; f < kF32FamilyCount; ++f)
    if (f32_conv_impl_in(impl, (F32Family)f)) return {(F32Family)f, impl - kF32Families[f].first};
  return {F32Family::Invalid, 0};
}
constexpr bool f32_conv_impl_valid(int impl) { return f32_conv_impl_find(impl).family != F32Family::Invalid; }

// the impls autotune times, in its order
constexpr int f32_conv_candidate_count() {
  int n = 0;
  for (const F32FamilyRow& r : kF32Families)
    for (int v = 0; v < r.count; ++v) n += (int)(r.tuned >> v & 1u);
  return n;
}
constexpr std::array<int, f32_conv_candidate_count()> f32_conv_candidates() {
  std::array<int, f32_conv_candidate_count()> a{};
  int n = 0;
  for (const F32FamilyRow& r : kF32Families)
    for (int v = 0; v < r.count; ++v)
      if (r.tuned >> v & 1u) a[n++] = r.first + v;
  return a;
}
inline constexpr auto kF32Candidates = f32_conv_candidates();

// rows of a kernel file's X-macro variant table, for its static_assert against the family's count
#define F32_TABLE_ROW(...) +1
#define F32_TABLE_ROWS(TABLE) (0 TABLE(F32_TABLE_ROW))

}  // namespace arena
