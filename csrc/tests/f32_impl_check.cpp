// Stand-alone check of the fp32 conv family table (csrc/kernels/f32_impl.h) against the impl numbers and the
// autotune order that data/tuning/conv_tuning.json and its tuning runs were written with.  The literals below are
// that on-disk format, written out here on purpose: a change of the table that moves one of them fails.
//   c++ -std=c++17 -Icsrc csrc/tests/f32_impl_check.cpp -o f32_impl_check && ./f32_impl_check
#include <cstdio>
#include <vector>

#include "kernels/f32_impl.h"

using namespace arena;

static int fails = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      std::printf("FAIL %s: ", #cond);       \
      std::printf(__VA_ARGS__);              \
      std::printf("\n");                     \
      ++fails;                               \
    }                                        \
  } while (0)

int main() {
  // 1. the valid set: 119 numbers
  static const int kRanges[][2] = {{0, 3},     {10, 26},   {40, 52},   {100, 111}, {111, 131}, {131, 145},
                                   {145, 151}, {151, 161}, {161, 167}, {171, 180}, {181, 183}, {191, 201}};
  int n_valid = 0;
  for (int v = -1; v < 400; ++v) {
    bool want = false;
    for (const auto& r : kRanges) want = want || (v >= r[0] && v < r[1]);
    CHECK(f32_conv_impl_valid(v) == want, "impl %d: valid %d, expected %d", v, (int)f32_conv_impl_valid(v), (int)want);
    n_valid += f32_conv_impl_valid(v) ? 1 : 0;
  }
  CHECK(n_valid == 119, "%d valid impls", n_valid);
  for (int v : {-1, 3, 9, 26, 39, 52, 99, 167, 168, 169, 170, 180, 183, 190, 201})
    CHECK(!f32_conv_impl_valid(v), "impl %d must be invalid", v);

  // 2. the autotune candidates, in order: 87 numbers
  std::vector<int> want = {0,   12,  13,  14,  17,  19,  20,  21,  23,  24,  100, 40,  41,  44,  45,
                           46,  47,  48,  101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 116, 117,
                           118, 120, 126, 127, 128, 130, 131, 132, 133, 135, 137, 138, 139, 140, 141};
  for (int v = 145; v <= 150; ++v) want.push_back(v);
  want.push_back(181);
  want.push_back(182);
  for (int v = 151; v <= 160; ++v) want.push_back(v);
  for (int v = 161; v <= 166; ++v) want.push_back(v);
  for (int v = 191; v <= 199; ++v) want.push_back(v);
  for (int v = 171; v <= 179; ++v) want.push_back(v);
  CHECK(want.size() == 87, "%zu expected candidates", want.size());
  CHECK(kF32Candidates.size() == want.size(), "%zu candidates", kF32Candidates.size());
  for (size_t i = 0; i < want.size() && i < kF32Candidates.size(); ++i)
    CHECK(kF32Candidates[i] == want[i], "candidate %zu is %d, expected %d", i, kF32Candidates[i], want[i]);

  // 3. candidates are valid, families are disjoint, (family, variant) round-trips
  for (int c : kF32Candidates) CHECK(f32_conv_impl_valid(c), "candidate %d", c);
  for (int v = -1; v < 400; ++v) {
    int owners = 0;
    for (int f = 0; f < kF32FamilyCount; ++f) owners += f32_conv_impl_in(v, (F32Family)f) ? 1 : 0;
    CHECK(owners == (f32_conv_impl_valid(v) ? 1 : 0), "impl %d is in %d families", v, owners);
    const F32Impl fv = f32_conv_impl_find(v);
    if (!f32_conv_impl_valid(v)) {
      CHECK(fv.family == F32Family::Invalid, "impl %d", v);
      continue;
    }
    const F32FamilyRow& row = f32_family(fv.family);
    CHECK(fv.v >= 0 && fv.v < row.count && row.first + fv.v == v && f32_conv_impl_in(v, fv.family),
          "impl %d -> family %s variant %d", v, row.name, fv.v);
    if (v >= 10) CHECK(row.reject[0] != '\0', "family %s has no text", row.name);
  }
  CHECK(kF32FamilyCount == 24, "%d families", kF32FamilyCount);
  for (const F32FamilyRow& r : kF32Families)
    CHECK(r.count >= 1 && r.count <= 32 && (r.count == 32 || r.tuned >> r.count == 0), "family %s: tuned mask", r.name);

  if (fails) return 1;
  std::printf("f32_impl_check: ok\n");
  return 0;
}
