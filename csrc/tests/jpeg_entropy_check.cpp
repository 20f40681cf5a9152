// Stand-alone check of the phased entropy coder's host form (csrc/runtime/jpeg_encode.cpp:
// jpeg_entropy_phased_host over csrc/kernels/jpeg_huff_math.h, the arithmetic the device coder
// csrc/kernels/jpeg_huff.hip runs), meant to be built host-only with -fsanitize=address,undefined
// (tests/test_jpeg_entropy.py):
//   - random crops of 1..70 x 1..70 pixels (random, flat and 0/255 checkerboard contents) through
//     jpeg_encode_coefs_host: the phased coder's bytes equal jpeg_write's, in zigzag and in natural block order;
//   - crafted coefficient sets at 1x1, 16x16, 17x9, 40x24 and 33x47: all zero, all +1023, all -1023, a sparse mix of
//     +-1023 and +-1 (heavy byte stuffing), uniform in +-1023, and blocks with zero runs above 15 and no EOB;
//   - the per-slot sizes sum to the scan's unstuffed length, and header + scan + EOI is jpeg_write.
//
//   jpeg_entropy_check [iterations = 300] [seed = 1]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../runtime/jpeg_encode.h"

using namespace arena;

namespace {

uint64_t rng_state = 1;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

int fail(const char* what, int w, int h, int kind) {
  std::fprintf(stderr, "jpeg_entropy_check: FAILED %s (w=%d h=%d kind=%d)\n", what, w, h, kind);
  return 1;
}

// both block orders against jpeg_write, the sizes against the scan; returns the scan's bytes through `scan_bytes`
int compare(int w, int h, const std::vector<int16_t>& zz, const JpegEncTables& t, int kind, long& scan_bytes) {
  constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  std::vector<int16_t> nat(zz.size());
  for (size_t b = 0; b < zz.size() / 64; ++b)
    for (int k = 0; k < 64; ++k) nat[b * 64 + kNatural[k]] = zz[b * 64 + k];
  const std::vector<uint8_t> want = jpeg_write(w, h, zz.data(), t, false);
  if (want != jpeg_write(w, h, nat.data(), t, true)) return fail("natural-order writer differs", w, h, kind);
  if (jpeg_entropy_phased_host(w, h, zz.data(), t, false) != want) return fail("phased coder differs", w, h, kind);
  if (jpeg_entropy_phased_host(w, h, nat.data(), t, true) != want) return fail("phased coder differs (natural)", w, h, kind);
  const std::vector<uint8_t> head = jpeg_write_header(w, h, t);
  if (want.size() < head.size() + 3 || std::memcmp(want.data(), head.data(), head.size()) != 0 ||
      want[want.size() - 2] != 0xFF || want[want.size() - 1] != 0xD9)
    return fail("header + scan + EOI", w, h, kind);
  // unstuffed length of the oracle's scan against the sizes
  long unstuffed = 0;
  for (size_t i = head.size(); i + 2 < want.size(); ++i) {
    ++unstuffed;
    if (want[i] == 0xFF) ++i;  // skip the stuffed 0x00
  }
  uint64_t bits = 0;
  for (uint32_t b : jpeg_block_bits_host(w, h, zz.data(), false)) bits += b;
  if ((long)((bits + 7) / 8) != unstuffed) return fail("sizes do not sum to the scan's length", w, h, kind);
  scan_bytes = (long)(want.size() - head.size() - 2);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 300;
  rng_state = argc > 2 ? (uint64_t)std::atoll(argv[2]) : 1;
  const JpegEncTables t = jpeg_enc_tables(kCropJpegQuality);
  long bytes = 0, crafted = 0, n;
  for (int it = 0; it < iters; ++it) {
    const int w = 1 + (int)(rnd() % 70), h = 1 + (int)(rnd() % 70), kind = (int)(rnd() % 4);
    std::vector<uint8_t> crop((size_t)w * h * 3);
    for (auto& b : crop) b = (uint8_t)rnd();
    const uint8_t flat[3] = {(uint8_t)rnd(), (uint8_t)rnd(), (uint8_t)rnd()};
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        uint8_t* p = &crop[((size_t)y * w + x) * 3];
        if (kind == 1) std::memcpy(p, flat, 3);
        if (kind >= 2) {
          const uint8_t v = ((x + y) & 1) ? 255 : 0;
          p[0] = p[2] = v;
          p[1] = kind == 3 ? (uint8_t)(255 - v) : v;
        }
      }
    std::vector<int16_t> zz((size_t)jpeg_enc_blocks(w, h) * 64);
    jpeg_encode_coefs_host<int32_t>(crop.data(), (int64_t)w * 3, w, h, t, zz.data(), true);
    if (compare(w, h, zz, t, kind, n)) return 1;
    bytes += n;
  }
  const int sizes[5][2] = {{1, 1}, {16, 16}, {17, 9}, {40, 24}, {33, 47}};
  for (const auto& sz : sizes)
    for (int kind = 10; kind < 16; ++kind) {
      const int w = sz[0], h = sz[1];
      std::vector<int16_t> zz((size_t)jpeg_enc_blocks(w, h) * 64, 0);
      for (size_t i = 0; i < zz.size(); ++i) {
        const size_t b = i / 64, k = i % 64;
        if (kind == 11) zz[i] = 1023;
        if (kind == 12) zz[i] = -1023;
        if (kind == 13) {
          const uint32_t r = rnd() % 8;
          zz[i] = r == 0 ? 1023 : r == 1 ? -1023 : r == 2 ? 1 : r == 3 ? -1 : 0;
        }
        if (kind == 14) zz[i] = (int16_t)((int)(rnd() % 2047) - 1023);
        if (kind == 15) zz[i] = k == 0 ? (b & 1 ? -1023 : 1023) : k == 63 ? (b & 2 ? -1 : 1) : (k == 35 && b % 3 == 0) ? 5 : 0;
      }
      if (compare(w, h, zz, t, kind, n)) return 1;
      bytes += n;
      ++crafted;
    }
  std::printf("jpeg_entropy_check: ok (%d crops, %ld crafted sets, %ld scan bytes)\n", iters, crafted, bytes);
  return 0;
}
