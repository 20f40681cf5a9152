// Fuzz of the EXIF orientation parse (runtime/jpeg_decode.cpp), built host-only under sanitizers by
// tests/test_jpeg_orientation.py:  exif_fuzz seed.jpg [iterations]
//
// The seed is a baseline JPEG with an EXIF APP1.  Each round mutates bytes inside the APP1 segments (random
// flips, a random 16/32-bit field set to an extreme, or the segment cut short with its length rewritten), then
// runs jpeg_parse, jpeg_decode_coefs and jpeg_coefs_to_rgb into a buffer of exactly the oriented size: broken
// EXIF must never change the status, leave the orientation outside 1..8 or the oriented size inconsistent.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "runtime/jpeg_decode.h"

using namespace arena;

namespace {

struct Seg {
  size_t at, len;  // payload offset and length
};

std::vector<Seg> app1_segments(const std::vector<uint8_t>& d) {
  std::vector<Seg> v;
  size_t pos = 2;
  while (pos + 4 <= d.size() && d[pos] == 0xFF) {
    const int m = d[pos + 1];
    const size_t len = ((size_t)d[pos + 2] << 8) | d[pos + 3];
    if (m == 0xDA || len < 2 || pos + 2 + len > d.size()) break;
    if (m == 0xE1) v.push_back({pos + 4, len - 2});
    pos += 2 + len;
  }
  return v;
}

int fail(const char* what, int round) {
  std::printf("exif_fuzz: FAILED (%s) in round %d\n", what, round);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: exif_fuzz seed.jpg [iterations]\n");
    return 2;
  }
  std::ifstream f(argv[1], std::ios::binary);
  const std::vector<uint8_t> seed((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const int iters = argc > 2 ? std::atoi(argv[2]) : 2000;
  const std::vector<Seg> segs = app1_segments(seed);
  if (segs.empty()) return fail("the seed has no APP1 segment", -1);
  JpegInfo base;
  std::string err;
  if (jpeg_parse(seed.data(), seed.size(), base, err) != JpegStatus::Ok) return fail("the seed does not parse", -1);
  std::mt19937 rng(1234);
  int oriented = 0;
  for (int r = 0; r < iters; ++r) {
    std::vector<uint8_t> d = seed;
    const Seg s = segs[rng() % segs.size()];
    const int kind = (int)(rng() % 4);
    if (kind == 0) {
      for (int k = 1 + (int)(rng() % 8); k > 0; --k) d[s.at + rng() % s.len] ^= (uint8_t)(1u << (rng() % 8));
    } else if (kind == 1) {
      for (int k = 1 + (int)(rng() % 4); k > 0; --k) d[s.at + rng() % s.len] = (uint8_t)rng();
    } else if (kind == 2) {  // an offset or count field at its extremes
      const size_t at = s.at + rng() % s.len;
      const uint8_t fill = (rng() & 1) ? 0xFF : 0x00;
      for (size_t k = at; k < at + 4 && k < s.at + s.len; ++k) d[k] = (rng() % 4) ? fill : (uint8_t)rng();
    } else {  // the segment cut short: drop its tail and rewrite its length
      const size_t keep = rng() % (s.len + 1);
      d.erase(d.begin() + (long)(s.at + keep), d.begin() + (long)(s.at + s.len));
      d[s.at - 2] = (uint8_t)((keep + 2) >> 8);
      d[s.at - 1] = (uint8_t)((keep + 2) & 0xFF);
    }
    JpegInfo info;
    if (jpeg_parse(d.data(), d.size(), info, err) != JpegStatus::Ok) return fail("EXIF damage changed the status", r);
    if (info.orientation < 1 || info.orientation > 8) return fail("orientation outside 1..8", r);
    const bool swap = info.orientation >= 5;
    if (info.width != base.width || info.height != base.height ||
        info.out_width != (swap ? info.height : info.width) || info.out_height != (swap ? info.width : info.height))
      return fail("inconsistent geometry", r);
    oriented += info.orientation > 1;
    std::vector<int16_t> coef((size_t)info.coef_count);
    if (jpeg_decode_coefs(d.data(), d.size(), info, coef.data(), err) != JpegStatus::Ok)
      return fail("EXIF damage changed the entropy decode", r);
    std::vector<uint8_t> rgb((size_t)info.out_width * info.out_height * 3);  // exact: ASan sees any overrun
    jpeg_coefs_to_rgb(info, coef.data(), rgb.data());
  }
  std::printf("exif_fuzz: ok (%d rounds, %d still oriented)\n", iters, oriented);
  return 0;
}
