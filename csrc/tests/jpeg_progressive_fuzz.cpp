// Fuzz driver for the progressive (SOF2) half of the host JPEG decoder (csrc/runtime/jpeg_decode.cpp), built
// host-only under AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_jpeg_progressive.py.  Progressive
// uploads reach the scan walk of decode_progressive from untrusted HTTP bodies once ARENA_JPEG_PROGRESSIVE is on:
// every scan header, table redefinition, restart interval, EOB run and correction bit of a damaged file must stay
// inside the coefficient buffer and the file.
//
//   jpeg_progressive_fuzz <iterations per seed> <seed.jpg>...
//
// The seeds are progressive files (each must decode).  Every mutation is decoded twice, dense (jpeg_decode_coefs)
// and compact (jpeg_decode_compact): same status, the payload within jpeg_compact_capacity, and expanded equal to
// the dense blocks.  Mutations: random byte flips anywhere; byte flips inside scan headers only (Ns, selectors,
// table ids, Ss, Se, Ah / Al); truncation; a scan (with its entropy-coded data) duplicated, dropped or swapped with
// its neighbour; a DRI segment's interval rewritten or a new one inserted between scans; DHT count rewrites.
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
  Bytes rgb((size_t)info.width * info.height * 3);
  arena::jpeg_coefs_to_rgb(info, coef.data(), rgb.data());
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
    std::fprintf(stderr, "usage: jpeg_progressive_fuzz iterations seed.jpg...\n");
    return 2;
  }
  const int iters = std::atoi(argv[1]);
  std::mt19937 rng(4321);
  int counts[3] = {0, 0, 0};
  for (int a = 2; a < argc; ++a) {
    const Bytes seed = read_file(argv[a]);
    if (seed.size() < 4 || run(seed) != JpegStatus::Ok) {
      std::fprintf(stderr, "seed %s does not decode\n", argv[a]);
      return 1;
    }
    const std::vector<Segment> segs = segments(seed);
    std::vector<size_t> scans, dhts;
    for (size_t i = 0; i < segs.size(); ++i) {
      if (segs[i].marker == 0xDA) scans.push_back(i);
      if (segs[i].marker == 0xC4) dhts.push_back(i);
    }
    if (scans.size() < 2 || dhts.empty() || join(seed, segs) != seed) {
      std::fprintf(stderr, "seed %s is not a progressive file this driver can take apart\n", argv[a]);
      return 1;
    }
    for (int it = 0; it < iters; ++it) {
      Bytes d = seed;
      const size_t si = scans[rng() % scans.size()];
      switch (it % 8) {
        case 0:  // byte flips anywhere
          for (int k = 0; k < 8; ++k) d[2 + rng() % (d.size() - 2)] = (uint8_t)rng();
          break;
        case 1: {  // one scan header
          const size_t b = segs[si].begin + 4, n = (((size_t)seed[b - 2] << 8) | seed[b - 1]) - 2;
          for (int k = 0; k < 1 + (int)(rng() % 3); ++k) d[b + rng() % n] = (uint8_t)(rng() % 3 ? rng() % 16 : rng());
          break;
        }
        case 2:  // truncation
          d.resize(2 + rng() % (d.size() - 2));
          break;
        case 3: {  // a scan several times
          std::vector<Segment> s2(segs.begin(), segs.begin() + (long)si + 1);
          for (int k = 0, n = 1 + (int)(rng() % 40); k < n; ++k) s2.push_back(segs[si]);
          s2.insert(s2.end(), segs.begin() + (long)si + 1, segs.end());
          d = join(seed, s2);
          break;
        }
        case 4: {  // a scan dropped, or swapped with the next one
          std::vector<Segment> s2 = segs;
          const size_t k = rng() % (scans.size() - 1);
          if (rng() & 1) s2.erase(s2.begin() + (long)scans[k]);
          else std::swap(s2[scans[k]], s2[scans[k + 1]]);
          d = join(seed, s2);
          break;
        }
        case 5: {  // a restart interval that does not match the data, defined in front of a scan
          std::vector<Segment> s2 = segs;
          d = seed;
          const uint8_t dri[6] = {0xFF, 0xDD, 0x00, 0x04, (uint8_t)(rng() % 2 ? 0 : rng()), (uint8_t)rng()};
          const size_t at = d.size();
          d.insert(d.end(), dri, dri + 6);
          s2.insert(s2.begin() + (long)si, Segment{0xDD, at, at + 6});
          d = join(d, s2);
          break;
        }
        default: {  // DHT count rewrites (tables between scans included), some with a byte flip
          const Segment& h = segs[dhts[rng() % dhts.size()]];
          for (int k = 0; k < 3; ++k) d[h.begin + 5 + rng() % 16] = (uint8_t)(rng() % 8);
          if (it % 8 == 7) d[2 + rng() % (d.size() - 2)] = (uint8_t)rng();
          break;
        }
      }
      counts[(int)run(d)]++;
    }
  }
  if (mismatches) {
    std::printf("jpeg_progressive_fuzz: %d compact decodes differ from the dense decode\n", mismatches);
    return 1;
  }
  std::printf("jpeg_progressive_fuzz: ok (%d seeds; %d ok, %d unsupported, %d corrupt; compact == dense on all)\n",
              argc - 2, counts[0], counts[1], counts[2]);
  return 0;
}
