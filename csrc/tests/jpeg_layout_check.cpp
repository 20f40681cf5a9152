// Check and fuzz driver for the layouts of the host JPEG decoder beyond 4:4:4 / 4:2:2 / 4:2:0 in one scan
// (csrc/runtime/jpeg_decode.cpp): 4:4:0 and the integral ("box") chroma ratios, RGB-coded components and sequential
// files whose components come in several scans.  Built host-only under AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_jpeg_layouts.py, which writes the seed files (tests/jpeg_layout_cases.py).
// Such uploads reach jpeg_parse, the scan walker and jpeg_coefs_to_rgb from untrusted HTTP bodies: whatever a
// damaged frame header claims about sampling factors, scans and component lists, every block must stay inside the
// coefficient buffer, every chroma read inside its plane and every pixel inside the output, all of which are
// allocated here at exactly their stated sizes.
//
//   jpeg_layout_check <iterations per seed> <seed.jpg>... [--range <seed.jpg>...]
//
// Every seed must decode (dense and compact, equal) and reconstruct.  The seeds after --range are files with crafted
// coefficients on both sides of the decoder's coefficient range (tests/jpeg_range_cases.py), in today's layouts: they
// must parse, and the dense and the compact decode must agree on "ok" or "unsupported" for them as for their
// mutations.  Every mutation is decoded both ways: same status, the payload within jpeg_compact_capacity, and
// expanded equal to the dense blocks.  Mutations: random byte flips anywhere; byte flips in the frame header's
// sampling factors and component ids; byte flips inside scan headers; truncation; a scan dropped, duplicated or
// swapped with its neighbour; a restart interval inserted in front of a scan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "runtime/jpeg_decode.h"

using arena::JpegInfo;
using arena::JpegStatus;

namespace {

using Bytes = std::vector<uint8_t>;

int mismatches = 0;
int new_layouts = 0;

JpegStatus run(const Bytes& d) {
  JpegInfo info;
  std::string err;
  JpegStatus st = arena::jpeg_parse(d.data(), d.size(), info, err, 64 << 20, 1);
  if (st != JpegStatus::Ok) return st;
  std::vector<int16_t> coef((size_t)info.coef_count);
  st = arena::jpeg_decode_coefs(d.data(), d.size(), info, coef.data(), err);
  JpegInfo ci = info;
  Bytes payload((size_t)arena::jpeg_compact_capacity(ci));
  std::string cerr;
  const JpegStatus cs = arena::jpeg_decode_compact(d.data(), d.size(), ci, payload.data(), cerr);
  if (cs != st) {
    ++mismatches;
  } else if (cs == JpegStatus::Ok) {
    if (ci.compact_bytes > (int64_t)payload.size()) ++mismatches;
    std::vector<int16_t> dense((size_t)ci.coef_count);
    arena::jpeg_compact_to_dense(ci, payload.data(), dense.data());
    if (dense != coef) ++mismatches;
  }
  if (st != JpegStatus::Ok) return st;
  new_layouts += info.multiscan || info.rgb_coded || info.layout > arena::JPEG_420;
  Bytes rgb((size_t)info.width * info.height * 3);
  arena::jpeg_coefs_to_rgb(info, coef.data(), rgb.data());
  // the device descriptor carries the ratios in single bytes
  const arena::JpegDesc dd = arena::jpeg_device_desc(info, 0, 0, 0);
  if (dd.rh != info.rh || dd.rv != info.rv || dd.rh < 1 || dd.rh > 4 || dd.rv < 1 || dd.rv > 4) ++mismatches;
  return st;
}

struct Segment {
  int marker;
  size_t begin, end;  // an SOS segment includes its entropy-coded data
};

// marker segments of a well-formed file
std::vector<Segment> segments(const Bytes& d) {
  std::vector<Segment> out;
  size_t p = 2;
  while (p + 4 <= d.size() && d[p] == 0xFF) {
    const int m = d[p + 1];
    if (m == 0xD9) break;
    size_t e = p + 2 + (((size_t)d[p + 2] << 8) | d[p + 3]);
    if (m == 0xDA)
      while (e + 1 < d.size() && !(d[e] == 0xFF && d[e + 1] != 0 && !(d[e + 1] >= 0xD0 && d[e + 1] <= 0xD7))) ++e;
    if (e > d.size()) break;
    out.push_back({m, p, e});
    p = e;
  }
  return out;
}

Bytes join(const Bytes& d, const std::vector<Segment>& segs) {
  Bytes out = {0xFF, 0xD8};
  for (const Segment& s : segs) out.insert(out.end(), d.begin() + (long)s.begin, d.begin() + (long)s.end);
  out.push_back(0xFF);
  out.push_back(0xD9);
  return out;
}

Bytes read_file(const char* path) {
  Bytes out;
  FILE* f = std::fopen(path, "rb");
  if (!f) return out;
  for (int c; (c = std::fgetc(f)) != EOF;) out.push_back((uint8_t)c);
  std::fclose(f);
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: jpeg_layout_check iterations seed.jpg... [--range seed.jpg...]\n");
    return 2;
  }
  const int iters = std::atoi(argv[1]);
  std::mt19937 rng(9157);
  int counts[3] = {0, 0, 0};
  int range_seeds[2] = {0, 0};  // ok, unsupported
  bool range = false;
  for (int a = 2; a < argc; ++a) {
    if (std::strcmp(argv[a], "--range") == 0) {
      range = true;
      continue;
    }
    const Bytes seed = read_file(argv[a]);
    const int before = new_layouts;
    if (range) {
      const JpegStatus st = seed.size() < 4 ? JpegStatus::Corrupt : run(seed);
      if (st == JpegStatus::Corrupt) {
        std::fprintf(stderr, "seed %s is not a well-formed file\n", argv[a]);
        return 1;
      }
      range_seeds[(int)st]++;
    } else if (seed.size() < 4 || run(seed) != JpegStatus::Ok || new_layouts == before) {
      std::fprintf(stderr, "seed %s does not decode as one of the layouts under test\n", argv[a]);
      return 1;
    }
    const std::vector<Segment> segs = segments(seed);
    std::vector<size_t> scans;
    size_t sof = segs.size();
    for (size_t i = 0; i < segs.size(); ++i) {
      if (segs[i].marker == 0xDA) scans.push_back(i);
      if (segs[i].marker >= 0xC0 && segs[i].marker <= 0xC2) sof = i;
    }
    if (scans.empty() || sof == segs.size() || join(seed, segs) != seed) {
      std::fprintf(stderr, "seed %s is not a file this driver can take apart\n", argv[a]);
      return 1;
    }
    for (int it = 0; it < iters; ++it) {
      Bytes d = seed;
      const size_t si = scans[rng() % scans.size()];
      switch (it % 6) {
        case 0:  // byte flips anywhere
          for (int k = 0; k < 6; ++k) d[2 + rng() % (d.size() - 2)] = (uint8_t)rng();
          break;
        case 1: {  // the frame header's component table: ids, sampling factors, table selectors
          const size_t b = segs[sof].begin + 10, n = segs[sof].end - b;
          for (int k = 0; k < 1 + (int)(rng() % 3); ++k) {
            const int h = 1 + (int)(rng() % 4), v = 1 + (int)(rng() % 4);
            d[b + rng() % n] = (uint8_t)(rng() % 4 ? (h << 4) | v : rng());
          }
          break;
        }
        case 2: {  // one scan header
          const size_t b = segs[si].begin + 4, n = (((size_t)seed[b - 2] << 8) | seed[b - 1]) - 2;
          for (int k = 0; k < 1 + (int)(rng() % 3); ++k) d[b + rng() % n] = (uint8_t)(rng() % 3 ? rng() % 16 : rng());
          break;
        }
        case 3:  // truncation
          d.resize(2 + rng() % (d.size() - 2));
          break;
        case 4: {  // a scan dropped, repeated, or swapped with the next one
          std::vector<Segment> s2 = segs;
          const int what = (int)(rng() % 3);
          if (what == 0) {
            s2.erase(s2.begin() + (long)si);
          } else if (what == 1) {
            for (int k = 0, n = 1 + (int)(rng() % 40); k < n; ++k) s2.insert(s2.begin() + (long)si, segs[si]);
          } else if (scans.size() > 1) {
            const size_t k = rng() % (scans.size() - 1);
            std::swap(s2[scans[k]], s2[scans[k + 1]]);
          }
          d = join(seed, s2);
          break;
        }
        default: {  // a restart interval that does not match the data, defined in front of a scan
          std::vector<Segment> s2 = segs;
          const uint8_t dri[6] = {0xFF, 0xDD, 0x00, 0x04, (uint8_t)(rng() % 2 ? 0 : rng()), (uint8_t)rng()};
          const size_t at = d.size();
          d.insert(d.end(), dri, dri + 6);
          s2.insert(s2.begin() + (long)si, Segment{0xDD, at, at + 6});
          d = join(d, s2);
          break;
        }
      }
      counts[(int)run(d)]++;
    }
  }
  if (mismatches) {
    std::printf("jpeg_layout_check: %d decodes are inconsistent (compact vs dense, or the descriptor)\n", mismatches);
    return 1;
  }
  std::printf("jpeg_layout_check: ok (%d seeds, %d + %d of them in and beyond the coefficient range; %d ok, "
              "%d unsupported, %d corrupt; compact == dense on all)\n",
              argc - 2 - (range ? 1 : 0), range_seeds[0], range_seeds[1], counts[0], counts[1], counts[2]);
  return 0;
}
