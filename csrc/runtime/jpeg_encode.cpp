// Host half of the JPEG crop encoder: tables, the host reference of the kernel's arithmetic, the Huffman pass and
// the marker writer.  Pure host code (the stand-alone check csrc/tests/jpeg_encode_check.cpp builds it without a
// GPU); the device-owning CropJpegEncoder is in jpeg_encode_device.cpp.
#include "jpeg_encode.h"

#include <algorithm>
#include <cstring>

#include "../kernels/jpeg_enc_math.h"
#include "../kernels/jpeg_huff_math.h"

namespace arena {

namespace {

// zigzag index -> natural index
constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ITU-T T.81 Annex K.1 quantisation tables, natural order
constexpr uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                   14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                   18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                     99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// ITU-T T.81 Annex K.3 Huffman tables: codes per length 1..16, then the symbols in code order
struct HuffSpec {
  uint8_t bits[16];
  const uint8_t* vals;
  int nvals;
};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
// DHT order of the file: DC0, AC0, DC1, AC1
constexpr HuffSpec kHuff[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, kDcVals, 12},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, kAcLumaVals, 162},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, kDcVals, 12},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}, kAcChromaVals, 162},
};
constexpr uint8_t kHuffClassId[4] = {0x00, 0x10, 0x01, 0x11};

// symbol -> (code, length), derived once from the specs (jchuff.c jpeg_make_c_derived_tbl)
struct CodeTable {
  uint16_t code[256];
  uint8_t len[256];
};
struct Codes {
  CodeTable t[4];
  Codes() {
    for (int k = 0; k < 4; ++k) {
      std::memset(&t[k], 0, sizeof(CodeTable));
      unsigned code = 0;
      int p = 0;
      for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < kHuff[k].bits[l - 1]; ++i, ++p) {
          t[k].code[kHuff[k].vals[p]] = (uint16_t)code++;
          t[k].len[kHuff[k].vals[p]] = (uint8_t)l;
        }
        code <<= 1;
      }
    }
  }
};
const Codes& codes() {
  static const Codes c;
  return c;
}

// Bit writer of the entropy-coded segment: MSB first, a 0xFF byte is followed by a stuffed 0x00.  It writes
// through a raw pointer into a buffer the caller sized for the worst case (kMaxBlockBytes per block): pending bits
// collect in a 64-bit accumulator and leave four bytes at a time, as one store when none of them is 0xFF.
constexpr size_t kMaxBlockBytes = 512;  // 27 bits of DC + 63 x (16-bit code + 15 value bits) = 248 bytes, all stuffed
struct BitWriter {
  uint8_t* p;
  uint64_t acc = 0;
  int n = 0;  // pending bits, < 32 between calls
  explicit BitWriter(uint8_t* dst) : p(dst) {}
  void byte(uint8_t b) {
    *p++ = b;
    if (b == 0xFF) *p++ = 0;
  }
  void put(uint32_t bits, int len) {  // len <= 31; bits above len are ignored
    acc = (acc << len) | (bits & ((1u << len) - 1u));
    n += len;
    if (n >= 32) {
      const uint32_t w = (uint32_t)(acc >> (n - 32));
      n -= 32;
      if ((((~w) - 0x01010101u) & w & 0x80808080u) == 0) {  // no byte of w is 0xFF
        p[0] = (uint8_t)(w >> 24);
        p[1] = (uint8_t)(w >> 16);
        p[2] = (uint8_t)(w >> 8);
        p[3] = (uint8_t)w;
        p += 4;
      } else {
        byte((uint8_t)(w >> 24));
        byte((uint8_t)(w >> 16));
        byte((uint8_t)(w >> 8));
        byte((uint8_t)w);
      }
    }
  }
  void flush() {  // whole pending bytes, then the last one padded with 1-bits
    while (n >= 8) {
      byte((uint8_t)(acc >> (n - 8)));
      n -= 8;
    }
    if (n > 0) byte((uint8_t)(((acc << (8 - n)) | ((1u << (8 - n)) - 1u)) & 0xFF));
    n = 0;
  }
};

inline int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

// jchuff.c encode_one_block over zz[0..63], the block in zigzag order (zz[0] is ignored: `dc` is coded), with `nz`
// the mask of its non-zero AC coefficients (bit k: zz[k] != 0), so the loop visits only those: the run before a
// coefficient is the gap to the previous set bit.
void encode_block(BitWriter& bw, const int16_t* zz, uint64_t nz, int dc, int pred, const CodeTable& dct,
                  const CodeTable& act) {
  const int diff = dc - pred;
  int nb = bit_length((unsigned)(diff < 0 ? -diff : diff));
  bw.put(dct.code[nb], dct.len[nb]);
  if (nb) bw.put((uint32_t)(diff < 0 ? diff - 1 : diff), nb);
  int prev = 0;
  for (uint64_t m = nz & ~1ull; m; m &= m - 1) {
    const int k = __builtin_ctzll(m);
    int run = k - prev - 1;
    prev = k;
    while (run > 15) {
      bw.put(act.code[0xF0], act.len[0xF0]);
      run -= 16;
    }
    const int v = zz[k];
    nb = bit_length((unsigned)(v < 0 ? -v : v));
    const int sym = (run << 4) | nb;
    bw.put(act.code[sym], act.len[sym]);
    bw.put((uint32_t)(v < 0 ? v - 1 : v), nb);
  }
  if (prev != 63) bw.put(act.code[0], act.len[0]);
}

void put16(std::vector<uint8_t>& o, int v) {
  o.push_back((uint8_t)(v >> 8));
  o.push_back((uint8_t)v);
}

}  // namespace

JpegEncTables jpeg_enc_tables(int quality) {
  quality = std::min(100, std::max(1, quality));
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  JpegEncTables t;
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < 64; ++i) {
      const int v = ((c ? kBaseChroma[i] : kBaseLuma[i]) * scale + 50) / 100;
      t.q[c][i] = (uint16_t)std::min(255, std::max(1, v));
    }
  return t;
}

template <typename Acc>
void jpeg_encode_coefs_host(const uint8_t* rgb, int64_t pitch, int w, int h, const JpegEncTables& t, int16_t* out,
                            bool zigzag) {
  const int mcux = (w + 15) / 16, mcuy = (h + 15) / 16;
  for (int my = 0; my < mcuy; ++my)
    for (int mx = 0; mx < mcux; ++mx)
      for (int s = 0; s < kJpegEncBlocksPerMcu; ++s, out += 64) {
        const bool chroma = s >= 4;
        Acc ws[8][8], col[8], o[8];
        for (int l = 0; l < 8; ++l) {
          Acc v[8];
          if (!chroma) {
            const int y = jpegm::enc_clamp(my * 16 + (s >> 1) * 8 + l, h - 1);
            for (int k = 0; k < 8; ++k) {
              const uint8_t* p = rgb + y * pitch + 3 * jpegm::enc_clamp(mx * 16 + (s & 1) * 8 + k, w - 1);
              int yy, cb, cr;
              jpegm::rgb_to_ycc(p[0], p[1], p[2], yy, cb, cr);
              v[k] = yy - 128;
            }
          } else {
            const int r = my * 8 + l;
            const uint8_t* row[2] = {rgb + jpegm::chroma_row0(r, h) * pitch, rgb + jpegm::chroma_row1(r, h) * pitch};
            for (int k = 0; k < 8; ++k) {
              const int c = mx * 8 + k;
              const int xs[2] = {3 * jpegm::enc_clamp(2 * c, w - 1), 3 * jpegm::enc_clamp(2 * c + 1, w - 1)};
              int cb[4], cr[4], yy;
              for (int i = 0; i < 4; ++i) {
                const uint8_t* p = row[i >> 1] + xs[i & 1];
                jpegm::rgb_to_ycc(p[0], p[1], p[2], yy, cb[i], cr[i]);
              }
              const int* q = s == 5 ? cr : cb;
              v[k] = jpegm::h2v2_down(q[0], q[1], q[2], q[3], c) - 128;
            }
          }
          jpegm::fdct8_rows<Acc>(v, ws[l]);
        }
        int16_t nat[64];
        for (int l = 0; l < 8; ++l) {
          for (int r = 0; r < 8; ++r) col[r] = ws[r][l];
          jpegm::fdct8_cols<Acc>(col, o);
          for (int r = 0; r < 8; ++r) nat[r * 8 + l] = (int16_t)jpegm::quantize((int)o[r], t.q[chroma][r * 8 + l]);
        }
        for (int k = 0; k < 64; ++k) out[k] = nat[zigzag ? kNatural[k] : k];
      }
}
template void jpeg_encode_coefs_host<int32_t>(const uint8_t*, int64_t, int, int, const JpegEncTables&, int16_t*, bool);
template void jpeg_encode_coefs_host<int64_t>(const uint8_t*, int64_t, int, int, const JpegEncTables&, int16_t*, bool);

std::vector<uint8_t> jpeg_write_header(int w, int h, const JpegEncTables& t) {
  std::vector<uint8_t> o;
  o.reserve(1024);
  // SOI, APP0 JFIF 1.01 (no units, density 1x1, no thumbnail)
  const uint8_t head[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  o.insert(o.end(), head, head + sizeof(head));
  for (int c = 0; c < 2; ++c) {  // DQT: 8-bit, zigzag
    o.push_back(0xFF);
    o.push_back(0xDB);
    put16(o, 67);
    o.push_back((uint8_t)c);
    for (int k = 0; k < 64; ++k) o.push_back((uint8_t)t.q[c][kNatural[k]]);
  }
  o.push_back(0xFF);  // SOF0
  o.push_back(0xC0);
  put16(o, 17);
  o.push_back(8);
  put16(o, h);
  put16(o, w);
  o.push_back(3);
  const uint8_t comps[] = {1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};
  o.insert(o.end(), comps, comps + sizeof(comps));
  for (int k = 0; k < 4; ++k) {  // DHT: DC0, AC0, DC1, AC1
    o.push_back(0xFF);
    o.push_back(0xC4);
    put16(o, 2 + 1 + 16 + kHuff[k].nvals);
    o.push_back(kHuffClassId[k]);
    o.insert(o.end(), kHuff[k].bits, kHuff[k].bits + 16);
    o.insert(o.end(), kHuff[k].vals, kHuff[k].vals + kHuff[k].nvals);
  }
  const uint8_t sos[] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  o.insert(o.end(), sos, sos + sizeof(sos));
  return o;
}

const uint32_t* jpeg_enc_code_tables() {
  struct Packed {
    uint32_t e[4 * jpegh::kCodeTableEntries];
    Packed() {
      const Codes& cd = codes();
      for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 256; ++i) e[k * 256 + i] = (uint32_t)cd.t[k].code[i] | ((uint32_t)cd.t[k].len[i] << 16);
    }
  };
  static const Packed p;
  return p.e;
}

std::vector<uint8_t> jpeg_write(int w, int h, const int16_t* coefs, const JpegEncTables& t, bool natural) {
  std::vector<uint8_t> o = jpeg_write_header(w, h, t);
  const int mcux = (w + 15) / 16, mcuy = (h + 15) / 16;
  const Codes& cd = codes();
  // real block grid per component: luma ceil(w / 8) x ceil(h / 8), chroma ceil(cw / 8) x ceil(ch / 8)
  const int ybw = (w + 7) / 8, ybh = (h + 7) / 8;
  const int cbw = ((w + 1) / 2 + 7) / 8, cbh = ((h + 1) / 2 + 7) / 8;
  // the scan is written into a per-thread buffer that holds its worst case, then appended
  static thread_local std::vector<uint8_t> scan;
  const size_t worst = (size_t)mcux * mcuy * kJpegEncBlocksPerMcu * kMaxBlockBytes + 16;
  if (scan.size() < worst) scan.resize(worst);
  BitWriter bw(scan.data());
  static const int16_t kZeroBlock[64] = {};
  int pred[3] = {0, 0, 0};
  const int16_t* blk = coefs;
  int16_t zz[64];
  for (int my = 0; my < mcuy; ++my)
    for (int mx = 0; mx < mcux; ++mx) {
      int last_dc = 0;  // DC of the block coded just before in this MCU (slot 0 of a component is always real)
      for (int s = 0; s < kJpegEncBlocksPerMcu; ++s, blk += 64) {
        const int c = s < 4 ? 0 : s - 3;
        const bool real = s < 4 ? (2 * my + (s >> 1) < ybh && 2 * mx + (s & 1) < ybw) : (my < cbh && mx < cbw);
        const CodeTable& dct = cd.t[c ? 2 : 0];
        const CodeTable& act = cd.t[c ? 3 : 1];
        if (real) {
          // the block in zigzag order and the mask of its non-zero coefficients
          uint64_t nz = 0;
          for (int k = 0; k < 64; ++k) {
            const int16_t v = blk[natural ? kNatural[k] : k];
            zz[k] = v;
            nz |= (uint64_t)(v != 0) << k;
          }
          encode_block(bw, zz, nz, zz[0], pred[c], dct, act);
          last_dc = zz[0];
        } else {
          encode_block(bw, kZeroBlock, 0, last_dc, pred[c], dct, act);
        }
        pred[c] = last_dc;
      }
    }
  bw.flush();
  o.insert(o.end(), scan.data(), bw.p);
  o.push_back(0xFF);
  o.push_back(0xD9);
  return o;
}

namespace {

constexpr bool zigzag_of_inverts_natural() {
  for (int k = 0; k < 64; ++k)
    if (jpegh::kZigzagOf[kNatural[k]] != k) return false;
  return true;
}
static_assert(zigzag_of_inverts_natural(), "jpeg_huff_math.h kZigzagOf is the inverse of kNatural");

}  // namespace

std::vector<uint32_t> jpeg_block_bits_host(int w, int h, const int16_t* coefs, bool natural) {
  const int mcux = (w + 15) / 16, slots = (int)jpeg_enc_blocks(w, h);
  const uint32_t* tables = jpeg_enc_code_tables();
  const auto dc_at = [&](int slot) { return (int)coefs[(size_t)slot * 64]; };  // index 0 in either order
  std::vector<uint32_t> bits((size_t)slots);
  int16_t zz[64] = {};
  for (int i = 0; i < slots; ++i) {
    const int mcu = i / kJpegEncBlocksPerMcu, s = i - mcu * kJpegEncBlocksPerMcu;
    const bool real = jpegh::slot_real(w, h, mcux, mcu, s);
    uint64_t nz = 0;
    if (real) {
      for (int k = 0; k < 64; ++k) zz[k] = coefs[(size_t)i * 64 + (natural ? kNatural[k] : k)];
      nz = jpegh::nonzero_mask(zz);
    }
    const int diff = jpegh::effective_dc(w, h, mcux, mcu, s, dc_at) - jpegh::predictor(w, h, mcux, mcu, s, dc_at);
    const uint32_t* tb = jpegh::slot_tables(tables, s);
    bits[(size_t)i] = (uint32_t)jpegh::block_bits(zz, nz, diff, tb, tb + jpegh::kCodeTableEntries);
  }
  return bits;
}

std::vector<uint8_t> jpeg_entropy_phased_host(int w, int h, const int16_t* coefs, const JpegEncTables& t, bool natural) {
  const int mcux = (w + 15) / 16, slots = (int)jpeg_enc_blocks(w, h);
  const uint32_t* tables = jpeg_enc_code_tables();
  const auto dc_at = [&](int slot) { return (int)coefs[(size_t)slot * 64]; };
  // size, scan
  std::vector<uint32_t> off = jpeg_block_bits_host(w, h, coefs, natural);
  uint32_t total = 0;
  for (uint32_t& b : off) {
    const uint32_t n = b;
    b = total;
    total += n;
  }
  // emit: every slot on its own, into a zeroed buffer
  const uint32_t nbytes = (total + 7) / 8;
  std::vector<uint32_t> words((size_t)nbytes / 4 + 2, 0u);
  const auto or_word = [&](uint32_t i, uint32_t v) { words[i] |= v; };
  int16_t zz[64] = {};
  for (int i = slots - 1; i >= 0; --i) {  // any order gives the same buffer
    const int mcu = i / kJpegEncBlocksPerMcu, s = i - mcu * kJpegEncBlocksPerMcu;
    const uint32_t* tb = jpegh::slot_tables(tables, s);
    const uint32_t* act = tb + jpegh::kCodeTableEntries;
    uint64_t nz = 0, code;
    int len;
    if (jpegh::slot_real(w, h, mcux, mcu, s)) {
      for (int k = 0; k < 64; ++k) zz[k] = coefs[(size_t)i * 64 + (natural ? kNatural[k] : k)];
      nz = jpegh::nonzero_mask(zz);
    }
    uint32_t pos = off[(size_t)i];
    jpegh::dc_symbol(jpegh::effective_dc(w, h, mcux, mcu, s, dc_at) - jpegh::predictor(w, h, mcux, mcu, s, dc_at), tb,
                     code, len);
    jpegh::put_bits(pos, code, len, or_word);
    pos += (uint32_t)len;
    for (uint64_t m = nz & ~1ull; m; m &= m - 1) {
      const int k = __builtin_ctzll(m);
      jpegh::ac_symbol(nz, k, zz[k], act, code, len);
      jpegh::put_bits(pos, code, len, or_word);
      pos += (uint32_t)len;
    }
    jpegh::eob_symbol(nz, act, code, len);
    jpegh::put_bits(pos, code, len, or_word);
  }
  {
    uint64_t code;
    int len;
    jpegh::pad_symbol(total, code, len);
    jpegh::put_bits(total, code, len, or_word);
  }
  std::vector<uint8_t> raw((size_t)words.size() * 4);
  for (size_t i = 0; i < words.size(); ++i) {
    const uint32_t be = jpegh::store_be32(words[i]);
    std::memcpy(&raw[i * 4], &be, 4);
  }
  // stuff: 0xFF bytes per segment, their prefix sum, then every byte at its own position
  const uint32_t nseg = (nbytes + jpegh::kStuffSegment - 1) / jpegh::kStuffSegment;
  std::vector<uint32_t> ff((size_t)nseg + 1, 0u);
  for (uint32_t i = 0; i < nbytes; ++i) ff[(size_t)i / jpegh::kStuffSegment + 1] += raw[i] == 0xFF;
  for (uint32_t g = 0; g < nseg; ++g) ff[(size_t)g + 1] += ff[g];
  std::vector<uint8_t> o = jpeg_write_header(w, h, t);
  const size_t base = o.size();
  o.resize(base + nbytes + ff[nseg], 0);
  for (uint32_t g = 0; g < nseg; ++g) {
    uint32_t before = ff[g];
    for (uint32_t i = g * jpegh::kStuffSegment; i < std::min(nbytes, (g + 1) * (uint32_t)jpegh::kStuffSegment); ++i) {
      o[base + jpegh::stuffed_at(i, before)] = raw[i];  // the stuffed 0x00 after it is already there
      before += raw[i] == 0xFF;
    }
  }
  o.push_back(0xFF);
  o.push_back(0xD9);
  return o;
}

std::vector<uint8_t> jpeg_encode_host(const uint8_t* rgb, int64_t pitch, int w, int h, const JpegEncTables& t) {
  std::vector<int16_t> coefs((size_t)jpeg_enc_blocks(w, h) * 64);
  jpeg_encode_coefs_host<int32_t>(rgb, pitch, w, h, t, coefs.data(), true);
  return jpeg_write(w, h, coefs.data(), t, false);
}

bool jpeg_crop_window(const CropBox& b, int frame_h, int frame_w, int& x0, int& y0, int& w, int& h) {
  // int(v) of Python: truncation towards zero; out-of-range floats are clipped first so the cast is defined
  auto trunc = [](double v) {
    if (!(v == v)) return 0;
    if (v > 1e9) return 1000000000;
    if (v < -1e9) return -1000000000;
    return (int)v;
  };
  const int x1 = std::max(0, trunc(b.x1)), y1 = std::max(0, trunc(b.y1));
  const int x2 = std::min(frame_w, trunc(b.x2)), y2 = std::min(frame_h, trunc(b.y2));
  if (x2 <= x1 || y2 <= y1) return false;
  x0 = x1;
  y0 = y1;
  w = x2 - x1;
  h = y2 - y1;
  return true;
}

size_t jpeg_enc_plan_chunk(const std::vector<CropWindow>& win, size_t first, int frame_w, int64_t capacity,
                           int max_crops, std::vector<JpegEncDesc>& descs, int64_t& bytes, int& max_blocks) {
  descs.clear();
  bytes = 0;
  max_blocks = 0;
  size_t i = first;
  for (; i < win.size() && (int)descs.size() < max_crops; ++i) {
    const CropWindow& c = win[i];
    const int64_t need = (jpeg_enc_coef_bytes(c.w, c.h) + 255) / 256 * 256;
    if (!descs.empty() && bytes + need > capacity) break;
    JpegEncDesc d;
    d.pitch = frame_w * 3;
    d.src_off = (int64_t)c.y0 * d.pitch + (int64_t)c.x0 * 3;
    d.out_off = bytes;
    d.w = c.w;
    d.h = c.h;
    d.mcux = (c.w + 15) / 16;
    d.total_blocks = (int32_t)jpeg_enc_blocks(c.w, c.h);
    d.pad_ = 0;
    descs.push_back(d);
    bytes += need;
    max_blocks = std::max(max_blocks, d.total_blocks);
  }
  return i;
}

std::string jpeg_enc_validate(const std::vector<JpegEncDesc>& descs, int frame_h, int frame_w, int64_t frame_bytes,
                              int64_t capacity) {
  if (frame_h <= 0 || frame_w <= 0) return "empty frame";
  if ((int64_t)frame_h * frame_w * 3 > frame_bytes) return "the frame does not fit the buffer it lies in";
  for (size_t i = 0; i < descs.size(); ++i) {
    const JpegEncDesc& d = descs[i];
    const std::string at = "crop " + std::to_string(i) + ": ";
    if (d.pitch != frame_w * 3 || d.w < 1 || d.h < 1 || d.mcux != (d.w + 15) / 16 ||
        d.total_blocks != jpeg_enc_blocks(d.w, d.h))
      return at + "inconsistent descriptor";
    if (d.src_off < 0) return at + "window starts before the frame";
    const int64_t y0 = d.src_off / d.pitch, xb = d.src_off % d.pitch;
    if (xb % 3 != 0 || xb / 3 + d.w > frame_w || y0 + d.h > frame_h) return at + "window leaves the frame";
    if (d.out_off < 0 || d.out_off % 16 != 0 || d.out_off + (int64_t)d.total_blocks * 128 > capacity)
      return at + "coefficients leave the output buffer";
  }
  return "";
}

}  // namespace arena
