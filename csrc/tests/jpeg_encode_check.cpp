// Stand-alone check of the host half of the JPEG crop encoder (csrc/runtime/jpeg_encode.cpp), meant to be built
// host-only with -fsanitize=address,undefined (tests/test_jpeg_encode.py):
//   - random crops of 1..70 x 1..70 pixels (random, flat and 0/255 checkerboard contents) are encoded, parsed and
//     entropy-decoded with the repository's own decoder (jpeg_parse + jpeg_decode_coefs); every real block must come
//     back with the coefficients that went in, every dummy block with zero AC (crops up to 4 pixels wide are
//     encoded too, but the decoder reports their 1-2 chroma columns as Unsupported, so they are not decoded);
//   - the int32 DCT accumulators (the GPU's) agree with int64 (libjpeg's JLONG) on every crop, the checkerboards
//     being the extreme inputs;
//   - crops are read from inside a larger pitched frame whose other bytes differ, and descriptor planning /
//     validation accepts what it planned and rejects windows and ranges that leave their buffers.
//
//   jpeg_encode_check [iterations = 300] [seed = 1]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../runtime/jpeg_decode.h"
#include "../runtime/jpeg_encode.h"

using namespace arena;

namespace {

uint64_t rng_state = 1;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

int fail(const char* what, int w, int h, int kind) {
  std::fprintf(stderr, "jpeg_encode_check: FAILED %s (w=%d h=%d kind=%d)\n", what, w, h, kind);
  return 1;
}

constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 300;
  rng_state = argc > 2 ? (uint64_t)std::atoll(argv[2]) : 1;
  const JpegEncTables t = jpeg_enc_tables(kCropJpegQuality);
  long blocks = 0, dummies = 0, narrow = 0;
  for (int it = 0; it < iters; ++it) {
    const int w = 1 + (int)(rnd() % 70), h = 1 + (int)(rnd() % 70), kind = (int)(rnd() % 4);
    // the crop sits at (x0, y0) of a larger frame filled with another pattern
    const int x0 = (int)(rnd() % 5), y0 = (int)(rnd() % 5), fw = w + x0 + (int)(rnd() % 5), fh = h + y0 + (int)(rnd() % 5);
    const int64_t pitch = (int64_t)fw * 3;
    std::vector<uint8_t> frame((size_t)fh * pitch);
    for (auto& b : frame) b = (uint8_t)rnd();
    const uint8_t flat[3] = {(uint8_t)rnd(), (uint8_t)rnd(), (uint8_t)rnd()};
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        uint8_t* p = &frame[(size_t)(y0 + y) * pitch + (size_t)(x0 + x) * 3];
        if (kind == 1) std::memcpy(p, flat, 3);
        if (kind >= 2) {
          const uint8_t v = ((x + y) & 1) ? 255 : 0;
          p[0] = p[2] = v;
          p[1] = kind == 3 ? (uint8_t)(255 - v) : v;
        }
      }
    const uint8_t* crop = &frame[(size_t)y0 * pitch + (size_t)x0 * 3];
    const size_t n = (size_t)jpeg_enc_blocks(w, h) * 64;
    std::vector<int16_t> c32(n), c64(n), nat(n);
    jpeg_encode_coefs_host<int32_t>(crop, pitch, w, h, t, c32.data(), true);
    jpeg_encode_coefs_host<int64_t>(crop, pitch, w, h, t, c64.data(), true);
    jpeg_encode_coefs_host<int32_t>(crop, pitch, w, h, t, nat.data(), false);
    if (c32 != c64) return fail("int32 and int64 accumulators differ", w, h, kind);
    const std::vector<uint8_t> file = jpeg_write(w, h, c32.data(), t, false);
    if (file != jpeg_write(w, h, nat.data(), t, true)) return fail("natural-order writer differs", w, h, kind);
    if (file != jpeg_encode_host(crop, pitch, w, h, t)) return fail("jpeg_encode_host differs", w, h, kind);

    JpegInfo info;
    std::string err;
    const JpegStatus st = jpeg_parse(file.data(), file.size(), info, err);
    if (w <= 4) {
      // the split decoder leaves 4:2:0 files with fewer than 3 chroma columns to PIL: nothing to decode with
      if (st != JpegStatus::Unsupported) return fail("a narrow crop should be outside the decoder's scope", w, h, kind);
      ++narrow;
      continue;
    }
    if (st != JpegStatus::Ok) return fail(err.c_str(), w, h, kind);
    if (info.width != w || info.height != h || info.layout != JPEG_420) return fail("parsed geometry", w, h, kind);
    std::vector<int16_t> dec((size_t)info.coef_count);
    if (jpeg_decode_coefs(file.data(), file.size(), info, dec.data(), err) != JpegStatus::Ok)
      return fail(err.c_str(), w, h, kind);
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < 64; ++i)
        if (info.qt[c][i] != t.q[c ? 1 : 0][i]) return fail("quantisation table", w, h, kind);
    const int mcux = (w + 15) / 16, mcuy = (h + 15) / 16;
    const int ybw = (w + 7) / 8, ybh = (h + 7) / 8;
    for (int my = 0; my < mcuy; ++my)
      for (int mx = 0; mx < mcux; ++mx)
        for (int s = 0; s < kJpegEncBlocksPerMcu; ++s) {
          const int c = s < 4 ? 0 : s - 3;
          const int by = s < 4 ? 2 * my + (s >> 1) : my, bx = s < 4 ? 2 * mx + (s & 1) : mx;
          const JpegCompDesc& k = info.comp[c];
          if (by >= k.bh || bx >= k.bw) return fail("decoder grid smaller than the MCU grid", w, h, kind);
          const int16_t* got = &dec[(size_t)k.coef_off + ((size_t)by * k.bw + bx) * 64];  // natural order
          const int16_t* want = &c32[((size_t)(my * mcux + mx) * kJpegEncBlocksPerMcu + s) * 64];  // zigzag
          const bool real = s >= 4 || (by < ybh && bx < ybw);
          ++blocks;
          if (real) {
            for (int z = 0; z < 64; ++z)
              if (got[kNatural[z]] != want[z]) return fail("decoded coefficients differ", w, h, kind);
          } else {
            ++dummies;
            for (int z = 1; z < 64; ++z)
              if (got[z] != 0) return fail("dummy block with AC", w, h, kind);
          }
        }

    // descriptors: what plan_chunk makes validates; a window or range moved out of its buffer does not
    std::vector<CropWindow> win = {{x0, y0, w, h}, {0, 0, fw, fh}};
    std::vector<JpegEncDesc> descs;
    int64_t bytes = 0;
    int max_blocks = 0;
    const int64_t cap = jpeg_enc_coef_bytes(fw, fh) * 3;
    if (jpeg_enc_plan_chunk(win, 0, fw, cap, 16, descs, bytes, max_blocks) != 2 || bytes > cap)
      return fail("plan_chunk", w, h, kind);
    if (!jpeg_enc_validate(descs, fh, fw, (int64_t)frame.size(), cap).empty()) return fail("validate rejects", w, h, kind);
    if (jpeg_enc_validate(descs, fh, fw, (int64_t)frame.size() - 1, cap).empty()) return fail("short frame", w, h, kind);
    if (jpeg_enc_validate(descs, fh, fw, (int64_t)frame.size(), bytes - 256).empty()) return fail("short output", w, h, kind);
    std::vector<JpegEncDesc> moved = descs;
    moved[0].src_off += (int64_t)(fw - x0 - w + 1) * 3;
    // (a 1-pixel-wide window moved past the right edge is the valid window at the start of the next row)
    if (w > 1 && jpeg_enc_validate(moved, fh, fw, (int64_t)frame.size(), cap).empty())
      return fail("window past the right", w, h, kind);
    moved = descs;
    moved[0].src_off += (int64_t)(fh - y0 - h + 1) * pitch;
    if (jpeg_enc_validate(moved, fh, fw, (int64_t)frame.size(), cap).empty()) return fail("window past the bottom", w, h, kind);
    // a one-crop capacity splits the list
    if (jpeg_enc_plan_chunk(win, 0, fw, 1, 16, descs, bytes, max_blocks) != 1) return fail("plan_chunk split", w, h, kind);
    int bx0, by0, bw, bh;
    if (!jpeg_crop_window({-3.7, -0.2, fw + 9.5, fh + 0.9}, fh, fw, bx0, by0, bw, bh) || bx0 || by0 || bw != fw || bh != fh)
      return fail("crop window clip", w, h, kind);
    if (jpeg_crop_window({2.9, 1.0, 2.1, 5.0}, fh, fw, bx0, by0, bw, bh)) return fail("empty crop window", w, h, kind);
  }
  std::printf("jpeg_encode_check: ok (%d crops, %ld not decodable, %ld blocks, %ld dummy)\n", iters, narrow, blocks,
              dummies);
  return 0;
}
