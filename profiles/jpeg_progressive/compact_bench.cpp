// Host time per file of jpeg_decode_compact (the serving paths' producer), in the manner of
// csrc/tests/jpeg_entropy_bench.cpp, which times jpeg_decode_coefs: files parsed once, then the fastest of 40
// passes into reused buffers.  SOF2 files are accepted whatever the process default.
// build: g++ -O2 -std=c++17 -Icsrc profiles/jpeg_progressive/compact_bench.cpp csrc/runtime/jpeg_decode.cpp
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "runtime/jpeg_decode.h"

int main(int argc, char** argv) {
  using namespace arena;
  std::vector<std::string> files;
  for (int i = 1; i < argc; ++i) {
    std::ifstream f(argv[i], std::ios::binary);
    files.emplace_back(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  }
  if (files.empty()) return 2;
  std::vector<JpegInfo> infos(files.size());
  std::vector<std::vector<uint8_t>> out(files.size());
  for (size_t i = 0; i < files.size(); ++i) {
    std::string err;
    if (jpeg_parse((const uint8_t*)files[i].data(), files[i].size(), infos[i], err, 0, 1) != JpegStatus::Ok) {
      std::fprintf(stderr, "%s: %s\n", argv[i + 1], err.c_str());
      return 1;
    }
    out[i].resize((size_t)jpeg_compact_capacity(infos[i]));
  }
  double best = 1e30;
  int64_t payload = 0;
  for (int r = 0; r < 40; ++r) {
    auto t0 = std::chrono::steady_clock::now();
    payload = 0;
    for (size_t i = 0; i < files.size(); ++i) {
      std::string err;
      if (jpeg_decode_compact((const uint8_t*)files[i].data(), files[i].size(), infos[i], out[i].data(), err) !=
          JpegStatus::Ok)
        return 1;
      payload += infos[i].compact_bytes;
    }
    best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  std::printf("%.1f us per image, %.0f payload bytes per image (%zu files, best of 40 passes)\n",
              best / files.size() * 1e6, (double)payload / files.size(), files.size());
  return 0;
}
