// Host check of the triple-bf16 split (csrc/kernels/x3.h), plain C++17 without HIP; needs clang (__bf16 and
// ext_vector_type).  Built and run by tests/test_x3_split.py.
//
//   x3_split_check            run the checks, print "x3_split_check: ok ..." and the counts
//   x3_split_check FILE       also write the edge values and their planes to FILE: per value one little-endian record
//                             {uint32 fp32 bits, uint16 h, uint16 m, uint16 l} (the Python test compares them with
//                             engine/planner.py split_bf16x3)
//
// 1. The two forms of the split give the same plane bits: element by element (the scalar x3_split, the
//    yardstick) against two at a time (x3_split8_pair) on every value; their other spellings (x3_split_at,
//    x3_split4, x3_split8; split_bf16x3_pair, x3_split4_pair) on the fixed values and one random block in eight.
//    Two NaN planes count as equal whatever their payload (an input whose h overflows to inf has NaN m and l).
// 2. h + m + l == v exactly in fp32, in both summation orders.  What the arithmetic guarantees, with u the fp32
//    quantum of v: r = v - h is a multiple of u with |r| <= 2^15 u, exact in fp32 (gradual underflow included);
//    r2 = r - m is a multiple of u with |r2| <= 2^6 u or a power of two, i.e. at most 8 significant bits, again
//    exact.  So l = bf16(r2) equals r2 whenever r2 fits bf16's exponent range, which is fp32's for normal numbers
//    but ends at the quantum 2^-133 below 2^-126.  Left out therefore, and counted:
//      * h not finite (|v| rounds past bf16's largest finite value: the residuals are inf - inf);
//      * 0 < |r2| < 2^-126 (l would be a bf16 subnormal or zero and may drop bits of r2).
//    Every input whose l is normal is checked: a normal l means |r2| >= 2^-126.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "kernels/x3.h"

namespace {

using namespace arena;

float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
uint32_t to_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
uint16_t bits(bf16 b) {
  uint16_t u;
  std::memcpy(&u, &b, 2);
  return u;
}
bool is_nan(uint16_t b) { return (b & 0x7fffu) > 0x7f80u; }
bool same(bf16 a, bf16 b) { return bits(a) == bits(b) || (is_nan(bits(a)) && is_nan(bits(b))); }
// exactly half-way between two bf16 values (x normal)
bool is_tie(float x) { return (to_bits(x) & 0xffffu) == 0x8000u; }

// ±0, smallest / largest normals, denormals (with bf16-denormal ties), ±inf, around bf16's largest finite value
const uint32_t kEdges[] = {
    0x00000000u, 0x80000000u, 0x00800000u, 0x80800000u, 0x7f7fffffu, 0xff7fffffu, 0x7f7f7fffu, 0x7f7f8000u,
    0x7f7f0000u, 0xff7f7fffu, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00008000u, 0x00018000u,
    0x00010000u, 0x80018000u, 0x00008001u, 0x00400000u, 0x7f800000u, 0xff800000u, 0x00ffffffu, 0x3f800000u,
    0x3fffffffu, 0x40490fdbu, 0xc0490fdbu, 0x3eaaaaabu, 0x00808080u, 0x01000001u, 0x0c7fffffu, 0x0c800001u,
};
// values exactly half-way between two bf16: the lower neighbour even (rounds down), then odd (rounds up)
const uint32_t kTies[] = {0x3f808000u, 0x3f818000u, 0xbf808000u, 0xbf818000u, 0x00808000u, 0x00818000u,
                          0x7e008000u, 0x7e018000u};
// values whose residual v - h is itself a tie: positive residual (even, odd), negative residual (even, odd)
const uint32_t kResidualTies[] = {0x3f804040u, 0x3f8040c0u, 0x3f80dfe0u, 0x3f80dfa0u,
                                  0xbf804040u, 0xbf8040c0u, 0xbf80dfe0u, 0xbf80dfa0u};

struct Counts {
  long values = 0, exact = 0, left_out_overflow = 0, left_out_subnormal = 0, normal_l = 0;
};

int fail(const char* what, float v) {
  std::printf("x3_split_check: FAILED %s at bits %08x\n", what, to_bits(v));
  return 1;
}

// the other spellings of the two forms against the scalar planes of 8 values
int check_wrappers(const float* v, const bf16* h, const bf16* m, const bf16* l) {
  bf16x8 h8, m8, l8, ha, ma, la;
  x3_split8(v, h8, m8, l8);
  for (int i = 0; i < 8; ++i) x3_split_at(v[i], i, ha, ma, la);
  for (int i = 0; i < 8; ++i) {
    if (!same(h8[i], h[i]) || !same(m8[i], m[i]) || !same(l8[i], l[i])) return fail("x3_split8", v[i]);
    if (!same(ha[i], h[i]) || !same(ma[i], m[i]) || !same(la[i], l[i])) return fail("x3_split_at", v[i]);
  }
  bf16x4 h4, m4, l4, hp4, mp4, lp4;
  x3_split4(v, h4, m4, l4);
  x3_split4_pair(f32x2{v[0], v[1]}, f32x2{v[2], v[3]}, hp4, mp4, lp4);
  for (int i = 0; i < 4; ++i) {
    if (!same(h4[i], h[i]) || !same(m4[i], m[i]) || !same(l4[i], l[i])) return fail("x3_split4", v[i]);
    if (!same(hp4[i], h[i]) || !same(mp4[i], m[i]) || !same(lp4[i], l[i])) return fail("x3_split4_pair", v[i]);
  }
  bf16x2 h2, m2, l2;
  split_bf16x3_pair(f32x2{v[6], v[7]}, h2, m2, l2);
  for (int i = 0; i < 2; ++i)
    if (!same(h2[i], h[6 + i]) || !same(m2[i], m[6 + i]) || !same(l2[i], l[6 + i]))
      return fail("split_bf16x3_pair", v[6 + i]);
  return 0;
}

// element by element (x3_split) against two at a time (x3_split8_pair) on 8 values, then the exactness of each;
// the other spellings on request
int check8(const float* v, Counts& n, bool wrappers) {
  bf16 h[8], m[8], l[8];
  for (int i = 0; i < 8; ++i) x3_split(v[i], h[i], m[i], l[i]);
  bf16x8 hp8, mp8, lp8;
  x3_split8_pair(v, hp8, mp8, lp8);
  for (int i = 0; i < 8; ++i)
    if (!same(hp8[i], h[i]) || !same(mp8[i], m[i]) || !same(lp8[i], l[i])) return fail("x3_split8_pair", v[i]);
  if (wrappers && check_wrappers(v, h, m, l)) return 1;

  for (int i = 0; i < 8; ++i) {
    ++n.values;
    const float fh = (float)h[i], fm = (float)m[i], fl = (float)l[i];
    const bool l_normal = std::isnormal(fl);
    n.normal_l += l_normal;
    if (!std::isfinite(fh)) {
      if (l_normal) return fail("normal l with h not finite", v[i]);
      ++n.left_out_overflow;
      continue;
    }
    const float r2 = (v[i] - fh) - fm;
    if (r2 != 0.f && std::fabs(r2) < 0x1p-126f) {
      if (l_normal) return fail("normal l left out", v[i]);
      ++n.left_out_subnormal;
      continue;
    }
    if ((fh + fm) + fl != v[i]) return fail("(h + m) + l != v", v[i]);
    if ((fl + fm) + fh != v[i]) return fail("(l + m) + h != v", v[i]);
    ++n.exact;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  constexpr int NE = sizeof(kEdges) / 4, NT = sizeof(kTies) / 4, NR = sizeof(kResidualTies) / 4;
  static_assert(NE % 8 == 0 && NT % 8 == 0 && NR % 8 == 0, "the fixed values are checked in blocks of 8");
  float fixed[NE + NT + NR];
  for (int i = 0; i < NE; ++i) fixed[i] = from_bits(kEdges[i]);
  for (int i = 0; i < NT; ++i) fixed[NE + i] = from_bits(kTies[i]);
  for (int i = 0; i < NR; ++i) fixed[NE + NT + i] = from_bits(kResidualTies[i]);

  // the tie lists are what they claim to be, and round to even
  for (int i = 0; i < NT; ++i) {
    const float v = fixed[NE + i];
    bf16 h, m, l;
    x3_split(v, h, m, l);
    const uint16_t down = (uint16_t)(kTies[i] >> 16);
    if (!is_tie(v) || bits(h) != ((down & 1) ? down + 1 : down)) return fail("tie list", v);
  }
  for (int i = 0; i < NR; ++i) {
    const float v = fixed[NE + NT + i];
    bf16 h, m, l;
    x3_split(v, h, m, l);
    const float r = v - (float)h;
    const uint16_t down = (uint16_t)(to_bits(r) >> 16);
    if (!is_tie(r) || bits(m) != ((down & 1) ? down + 1 : down)) return fail("residual tie list", v);
  }

  Counts n;
  for (int i = 0; i < NE + NT + NR; i += 8)
    if (check8(fixed + i, n, true)) return 1;

  // 1.3e6 blocks of 8 random bit patterns (1.04e7 values), NaNs replaced by the next pattern; the other spellings
  // of the forms on every 8th block
  std::mt19937 gen(20240607u);
  long nan_skipped = 0;
  for (long b = 0; b < 1300000; ++b) {
    float v[8];
    for (int i = 0; i < 8;) {
      const float f = from_bits((uint32_t)gen());
      if (f != f) {
        ++nan_skipped;
        continue;
      }
      v[i++] = f;
    }
    if (check8(v, n, b % 8 == 0)) return 1;
  }

  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "wb");
    if (f == nullptr) return fail("cannot write the planes file", 0.f);
    for (int i = 0; i < NE + NT + NR; ++i) {
      bf16 h, m, l;
      x3_split(fixed[i], h, m, l);
      const uint32_t vb = to_bits(fixed[i]);
      const uint16_t p[3] = {bits(h), bits(m), bits(l)};
      std::fwrite(&vb, 4, 1, f);
      std::fwrite(p, 2, 3, f);
    }
    std::fclose(f);
  }
  std::printf("x3_split_check: ok values=%ld exact=%ld normal_l=%ld left_out_overflow=%ld left_out_subnormal=%ld "
              "nan_skipped=%ld\n",
              n.values, n.exact, n.normal_l, n.left_out_overflow, n.left_out_subnormal, nan_skipped);
  return 0;
}
