// See jpeg_decode.h.
#include "runtime/jpeg_decode.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../kernels/jpeg_math.h"

namespace arena {

namespace {

// zig-zag index -> natural index, with 16 guard entries so a corrupt run past coefficient 63 stays in the block
// (libjpeg's jpeg_natural_order has the same padding)
constexpr uint8_t kNatural[64 + 16] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
    6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
    39, 46, 53, 60, 61, 54, 47, 55, 62, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

// Kraft check of a DHT's code-length counts (JPEG Annex C): the canonical code assigns codes of length l in order,
// so after each length the next code must still fit in l bits.  An over-subscribed table is corrupt data.
bool huff_lengths_valid(const uint8_t* bits) {
  int64_t code = 0;
  for (int l = 1; l <= 16; ++l) {
    code += bits[l];
    if (code > (int64_t(1) << l)) return false;
    code <<= 1;
  }
  return true;
}

uint16_t be16(const uint8_t* p) { return (uint16_t)((p[0] << 8) | p[1]); }

// The tables of one DHT segment into dc[4] / ac[4]; false for a malformed segment or an over-subscribed code.
bool read_dht(const uint8_t* seg, size_t sl, JpegHuffSpec* dc, JpegHuffSpec* ac) {
  size_t q = 0;
  while (q < sl) {
    const int tc = seg[q] >> 4, th = seg[q] & 15;
    if (tc > 1 || th > 3 || q + 17 > sl) return false;
    JpegHuffSpec& h = tc == 0 ? dc[th] : ac[th];
    int count = 0;
    h.bits[0] = 0;
    for (int l = 1; l <= 16; ++l) {
      h.bits[l] = seg[q + l];
      count += h.bits[l];
    }
    if (count > 256 || q + 17 + count > sl || !huff_lengths_valid(h.bits)) return false;
    std::memset(h.vals, 0, sizeof h.vals);
    std::memcpy(h.vals, seg + q + 17, count);
    h.present = true;
    q += 17 + count;
  }
  return true;
}

constexpr int kFastBits = 11;
constexpr int kEobRun = 127;  // ac_fast run of an EOB entry

inline int extend(uint32_t v, int s) { return (int)v - ((v < (1u << (s - 1))) ? (int)((1u << s) - 1) : 0); }

// Decoding tables of one Huffman code (JPEG Annex C / F.2.2.3): an 11-bit lookahead table resolves every code of
// up to 11 bits with one lookup; longer codes walk maxcode / valoff by length.  AC tables also get `ac_fast`:
// when a code and the magnitude bits that follow it fit in the 11-bit lookahead, one lookup yields the run,
// the signed coefficient and the total bit count (most coefficients of a q90 frame).
struct HuffTable {
  uint16_t fast[1 << kFastBits];  // (length << 8) | symbol, 0 = longer than kFastBits
  int32_t ac_fast[1 << kFastBits];  // (value << 16) | (run << 8) | total length, 0 = no shortcut
  int32_t maxcode[18];            // largest code of each length (-1: none); [17] sentinel
  int32_t valoff[17];             // symbol index of the first code of each length minus that code
  uint8_t vals[256];

  bool build(const JpegHuffSpec& s, bool ac) {
    std::memset(fast, 0, sizeof fast);
    std::memset(ac_fast, 0, sizeof ac_fast);
    std::memcpy(vals, s.vals, sizeof vals);
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
      const int n = s.bits[l];
      valoff[l] = k - code;
      if (n) {
        for (int i = 0; i < n; ++i, ++k, ++code) {
          // over-subscribed code (too many codes of this or a shorter length): reject it before any table
          // write, as libjpeg's jdhuff.c does; (code << shift) | j would otherwise index past fast / ac_fast
          if (code >= (1 << l) || k >= 256) return false;
          if (l <= kFastBits) {
            const int shift = kFastBits - l;
            const uint8_t sym = s.vals[k];
            const uint16_t e = (uint16_t)((l << 8) | sym);
            for (int j = 0; j < (1 << shift); ++j) {
              const int idx = (code << shift) | j;
              fast[idx] = e;
              const int run = sym >> 4, mag = sym & 15;
              if (ac && mag && l + mag <= kFastBits) {
                const uint32_t bitsv = (uint32_t)(j >> (shift - mag)) & ((1u << mag) - 1);
                const int v = extend(bitsv, mag);
                ac_fast[idx] = (int32_t)((uint32_t)v << 16) | (run << 8) | (l + mag);
              } else if (ac && sym == 0x00) {
                ac_fast[idx] = (kEobRun << 8) | l;  // EOB: the run pushes k past the block
              } else if (ac && sym == 0xF0) {
                ac_fast[idx] = (15 << 8) | l;       // ZRL: 15 zeros + a stored zero = 16 positions
              }
            }
          }
        }
        maxcode[l] = code - 1;
      } else {
        maxcode[l] = -1;
      }
      code <<= 1;
    }
    maxcode[17] = 0x7fffffff;
    return true;
  }
};

// MSB-first bit reader over the entropy-coded segment: removes the 0xFF00 stuffing, stops at a marker and
// then feeds zero bits (libjpeg's behaviour on truncated data).  The fast refill takes up to 7 bytes at once
// when none of them is 0xFF.
struct BitReader {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t buf = 0;
  int bits = 0;
  bool marker = false;
  int64_t pad = 0;         // zero bytes fed because the data ended without a marker
  int64_t zfill = 0;       // zero bytes fed after a marker cut the segment short
  bool truncated = false;  // some of the `pad` bits were consumed (PIL: "image file is truncated")
  bool bad_code = false;   // decode() met bits that match no code (libjpeg warns)

  __attribute__((always_inline)) inline void refill() {
    if (!marker && end - p >= 8) {
      uint64_t x;
      std::memcpy(&x, p, 8);
      x = __builtin_bswap64(x);
      const int k = (63 - bits) >> 3;  // whole bytes that fit
      const uint64_t keep = ~0ULL << (64 - 8 * k);
      const uint64_t nx = ~x;          // 0xFF bytes -> 0x00
      const uint64_t ff = (nx - 0x0101010101010101ULL) & ~nx & 0x8080808080808080ULL;
      if ((ff & keep) == 0) {
        buf |= (x & keep) >> bits;
        bits += 8 * k;
        p += k;
        return;
      }
    }
    refill_slow();
  }
  void refill_slow() {
    while (bits <= 56) {
      uint32_t b = 0;
      if (marker) ++zfill;
      else if (p >= end) ++pad;
      if (!marker && p < end) {
        b = *p;
        if (b == 0xFF) {
          const uint32_t nb = p + 1 < end ? p[1] : 0xD9;
          if (nb == 0x00) {
            p += 2;
          } else {
            marker = true;  // p stays on the marker
            ++zfill;
            b = 0;
          }
        } else {
          ++p;
        }
      }
      buf |= (uint64_t)b << (56 - bits);
      bits += 8;
    }
  }
  __attribute__((always_inline)) inline void need(int n) {
    if (bits < n) refill();
  }
  __attribute__((always_inline)) inline void skip(int n) {
    buf <<= n;
    bits -= n;
  }
  __attribute__((always_inline)) inline uint32_t get(int n) {  // 1 <= n <= 16, after need()
    const uint32_t v = (uint32_t)(buf >> (64 - n));
    buf <<= n;
    bits -= n;
    return v;
  }
  // one Huffman symbol; needs 16 valid bits
  __attribute__((always_inline)) inline int decode(const HuffTable& t) {
    const uint32_t e = t.fast[buf >> (64 - kFastBits)];
    if (e) {
      skip((int)(e >> 8));
      return (int)(e & 0xFF);
    }
    return decode_slow(t);
  }
  int decode_slow(const HuffTable& t) {
    const uint32_t code16 = (uint32_t)(buf >> 48);
    for (int l = kFastBits + 1; l <= 16; ++l) {
      const int32_t c = (int32_t)(code16 >> (16 - l));
      if (c <= t.maxcode[l]) {
        skip(l);
        return t.vals[(t.valoff[l] + c) & 0xFF];
      }
    }
    // no code matches (corrupt data): libjpeg warns and yields symbol 0; consume 16 bits so the scan advances
    bad_code = true;
    skip(16);
    return 0;
  }
  // Restart marker: drop the bits of the finished interval and step over RSTn (scanning forward if the
  // encoder left padding or the marker is missing, as libjpeg's resync does).
  bool overran() const { return pad * 8 > bits; }
  // libjpeg's insufficient_data: a bit past a marker was consumed; the rest of the segment decodes as zero
  // blocks (uniform grey) instead of reading the zero fill
  bool starved() const { return zfill * 8 > bits; }
  void restart() {
    truncated |= overran();
    pad = 0;
    zfill = 0;
    buf = 0;
    bits = 0;
    marker = false;
    while (p + 1 < end) {
      if (p[0] == 0xFF && p[1] >= 0xD0 && p[1] <= 0xD7) {
        p += 2;
        return;
      }
      if (p[0] == 0xFF && p[1] != 0x00 && p[1] != 0xFF) return;  // some other marker: leave it for the reader
      ++p;
    }
  }
};

// The coefficient range (kernels/jpeg_math.h, kCoefRangeLimit), S = sum |c_k| * q_k <= limit per block.  The block
// decoders pay one addition per coded coefficient for it: they add up |c_k| over the AC coefficients the stream
// codes, bound S by |DC| * q_0 + max(q_1..63) * sum |c_k|, and only a block that fails this bound (about one in a
// hundred of a noisy q90 upload) has its exact sum taken.  That addition is not free: profiles/jpeg_range/README.md
// has the cost and the cheaper-looking variants that were no cheaper.  The DC enters as the predictor itself, not as
// the int16 stored: a predictor that has left int16 is far beyond the limit (or meets a zero quantizer, which makes
// it zero in every arithmetic).
struct RangeQuant {
  uint16_t qz[64];  // the component's quantization table in zigzag order
  uint32_t ac_max;  // its largest AC entry
};
inline uint64_t range_term(int v, uint16_t q) { return (uint64_t)(uint32_t)(v < 0 ? -v : v) * q; }
inline uint64_t range_dc(int pred, uint16_t q) { return (uint64_t)(pred < 0 ? -(int64_t)pred : (int64_t)pred) * q; }
inline bool range_wide(uint64_t sum) { return sum > (uint64_t)jpegm::kCoefRangeLimit; }
const char* const kRangeMessage = "coefficients beyond the range in which libjpeg's 16-bit IDCT is exact";

void range_quant(const JpegInfo& info, RangeQuant rq[kJpegMaxComp]) {
  for (int c = 0; c < info.ncomp; ++c) {
    rq[c].ac_max = 0;
    for (int k = 0; k < 64; ++k) {
      rq[c].qz[k] = info.qt[c][kNatural[k]];
      if (k) rq[c].ac_max = std::max<uint32_t>(rq[c].ac_max, rq[c].qz[k]);
    }
  }
}

// the exact sum of a dense block (natural order) whose DC predictor is `pred`
__attribute__((noinline)) bool range_wide_block(const int16_t* blk, int pred, const RangeQuant& rq) {
  uint64_t sum = range_dc(pred, rq.qz[0]);
  for (int k = 1; k < 64; ++k) sum += range_term(blk[kNatural[k]], rq.qz[k]);
  return range_wide(sum);
}

// the same of a compact block: `vals` are the values of the coefficients `mask` names, in zigzag order, the DC first
__attribute__((noinline)) bool range_wide_compact(uint64_t mask, const int16_t* vals, int pred, const RangeQuant& rq) {
  uint64_t sum = range_dc(pred, rq.qz[0]);
  ++vals;
  for (uint64_t m = mask & ~1ull; m; m &= m - 1) sum += range_term(*vals++, rq.qz[__builtin_ctzll(m)]);
  return range_wide(sum);
}

// One 8x8 block: DC difference + AC run/size symbols, coefficients written in natural order.  `wide` is set (never
// cleared) when the block is outside the coefficient range.
__attribute__((always_inline)) inline bool decode_block(BitReader& br, const HuffTable& dc, const HuffTable& ac,
                                                        int& pred, int16_t* blk, const RangeQuant& rq, bool& wide) {
  std::memset(blk, 0, 64 * sizeof(int16_t));
  br.need(32);
  const int s = br.decode(dc);
  if (s) {
    if (s > 15) return false;
    pred += extend(br.get(s), s);
  }
  blk[0] = (int16_t)pred;
  uint32_t mags = 0;  // sum |c_k| over the coded AC coefficients: at most 63 * 2^15
  for (int k = 1; k < 64;) {
    br.need(32);  // a code (<= 16 bits) and its magnitude (<= 15 bits)
    const int32_t f = ac.ac_fast[br.buf >> (64 - kFastBits)];
    if (f) {  // one lookup: coefficient, ZRL or EOB
      br.skip(f & 0xFF);
      k += (f >> 8) & 0xFF;
      if (k > 63) break;  // EOB (or a corrupt run past the block)
      const int v = f >> 16;
      blk[kNatural[k]] = (int16_t)v;
      mags += (uint32_t)(v < 0 ? -v : v);
      ++k;
      continue;
    }
    const int rs = br.decode(ac);
    const int r = rs >> 4, sz = rs & 15;
    if (sz) {
      k += r;
      const int v = extend(br.get(sz), sz);
      blk[kNatural[k]] = (int16_t)v;
      mags += (uint32_t)(v < 0 ? -v : v);
      ++k;
    } else {
      if (r != 15) break;  // EOB
      k += 16;
    }
  }
  if (__builtin_expect(range_wide(range_dc(pred, rq.qz[0]) + (uint64_t)mags * rq.ac_max), 0))
    wide |= range_wide_block(blk, pred, rq);
  return true;
}


// The same block in the compact layout (jpeg_decode.h, jpeg_decode_compact): bit k of *mask set for every coded
// coefficient at zigzag index k, their values appended to vals in zigzag order (the DC always, even when 0).
__attribute__((always_inline)) inline bool decode_block_compact(BitReader& br, const HuffTable& dc, const HuffTable& ac,
                                                                int& pred, uint64_t* mask, int16_t* vals, int64_t& nv,
                                                                const RangeQuant& rq, bool& wide) {
  br.need(32);
  const int s = br.decode(dc);
  if (s) {
    if (s > 15) return false;
    pred += extend(br.get(s), s);
  }
  uint64_t m = 1;
  int64_t n = nv;
  vals[n++] = (int16_t)pred;
  uint32_t mags = 0;  // as in decode_block
  for (int k = 1; k < 64;) {
    br.need(32);
    const int32_t f = ac.ac_fast[br.buf >> (64 - kFastBits)];
    if (f) {
      br.skip(f & 0xFF);
      k += (f >> 8) & 0xFF;
      if (k > 63) break;
      m |= 1ull << k;
      const int v = f >> 16;
      vals[n++] = (int16_t)v;
      mags += (uint32_t)(v < 0 ? -v : v);
      ++k;
      continue;
    }
    const int rs = br.decode(ac);
    const int r = rs >> 4, sz = rs & 15;
    if (sz) {
      k += r;
      const int16_t v = (int16_t)extend(br.get(sz), sz);
      mags += (uint32_t)(v < 0 ? -(int)v : (int)v);
      if (k > 63) {  // a corrupt run past the block: the dense decoder's kNatural pad stores it at 63
        if (m >> 63) vals[n - 1] = v;  // zigzag 63 is the last value appended
        else {
          m |= 1ull << 63;
          vals[n++] = v;
        }
      } else {
        m |= 1ull << k;
        vals[n++] = v;
      }
      ++k;
    } else {
      if (r != 15) break;
      k += 16;
    }
  }
  *mask = m;
  if (__builtin_expect(range_wide(range_dc(pred, rq.qz[0]) + (uint64_t)mags * rq.ac_max), 0))
    wide |= range_wide_compact(m, vals + nv, pred, rq);
  nv = n;
  return true;
}

// EXIF orientation of an APP1 payload (rule in jpeg_decode.h); 0 when the payload is not EXIF at all
int exif_orientation(const uint8_t* seg, size_t sl) {
  if (sl < 6 || std::memcmp(seg, "Exif\0\0", 6) != 0) return 0;
  const uint8_t* t = seg + 6;
  const uint64_t L = sl - 6;
  if (L < 8) return 1;
  const bool le = t[0] == 'I' && t[1] == 'I';
  if (!le && !(t[0] == 'M' && t[1] == 'M')) return 1;
  auto u16 = [&](uint64_t o) -> uint32_t { return le ? (uint32_t)(t[o] | (t[o + 1] << 8)) : (uint32_t)((t[o] << 8) | t[o + 1]); };
  auto u32 = [&](uint64_t o) -> uint64_t { return le ? ((uint64_t)u16(o + 2) << 16) | u16(o) : ((uint64_t)u16(o) << 16) | u16(o + 2); };
  if (u16(2) != 42) return 1;
  const uint64_t ifd = u32(4);
  if (ifd + 2 > L) return 1;
  const uint64_t count = u16(ifd);
  if (ifd + 2 + 12 * count > L) return 1;  // 64-bit: neither term can wrap
  for (uint64_t i = 0; i < count; ++i) {
    const uint64_t e = ifd + 2 + 12 * i;
    if (u16(e) != 0x0112) continue;
    if (u16(e + 2) != 3 || u32(e + 4) != 1) return 1;
    const uint32_t v = u16(e + 8);
    return v >= 1 && v <= 8 ? (int)v : 1;
  }
  return 1;
}

}  // namespace

namespace {
std::atomic<int>& progressive_default() {
  static std::atomic<int> on{[] {
    const char* e = std::getenv("ARENA_JPEG_PROGRESSIVE");
    return e != nullptr && std::atoi(e) != 0 ? 1 : 0;
  }()};
  return on;
}
}  // namespace

bool jpeg_progressive_enabled() { return progressive_default().load(std::memory_order_relaxed) != 0; }
bool jpeg_set_progressive_enabled(bool on) { return progressive_default().exchange(on ? 1 : 0) != 0; }

JpegStatus jpeg_parse(const uint8_t* data, size_t n, JpegInfo& info, std::string& err, int64_t max_pixels,
                      int progressive) {
  info = JpegInfo{};
  if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) {
    err = "not a JPEG stream";
    return JpegStatus::Unsupported;  // PNG, WebP, ... : the fallback identifies it
  }
  uint16_t qtab[4][64];
  bool qpresent[4] = {false, false, false, false};
  bool saw_sof = false, saw_jfif = false, adobe = false, saw_exif = false;
  int adobe_transform = -1;
  size_t pos = 2;
  while (true) {
    while (pos < n && data[pos] != 0xFF) ++pos;  // tolerate garbage between markers (libjpeg warns)
    while (pos < n && data[pos] == 0xFF) ++pos;
    if (pos >= n) {
      err = "Failed to decode image: no scan before the end of data";
      return JpegStatus::Corrupt;
    }
    const int m = data[pos++];
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // standalone markers
    if (m == 0xD9) {
      err = "Failed to decode image: end of image before the first scan";
      return JpegStatus::Corrupt;
    }
    if (pos + 2 > n) {
      err = "Failed to decode image: truncated marker";
      return JpegStatus::Corrupt;
    }
    const size_t len = be16(data + pos);
    if (len < 2 || pos + len > n) {
      err = "Failed to decode image: truncated marker segment";
      return JpegStatus::Corrupt;
    }
    const uint8_t* seg = data + pos + 2;
    const size_t sl = len - 2;
    pos += len;
    if (m == 0xC0 || m == 0xC1 ||
        (m == 0xC2 && (progressive < 0 ? jpeg_progressive_enabled() : progressive != 0))) {
      info.progressive = m == 0xC2;
      if (saw_sof || sl < 6) {
        err = "Failed to decode image: bad SOF";
        return JpegStatus::Corrupt;
      }
      saw_sof = true;
      if (seg[0] != 8) {
        err = "12-bit JPEG";
        return JpegStatus::Unsupported;
      }
      info.height = be16(seg + 1);
      info.width = be16(seg + 3);
      info.ncomp = seg[5];
      if (info.height == 0) {
        err = "height from DNL";
        return JpegStatus::Unsupported;
      }
      if (info.width == 0 || sl < 6 + 3 * (size_t)info.ncomp) {
        err = "Failed to decode image: bad SOF";
        return JpegStatus::Corrupt;
      }
      if (info.ncomp != 1 && info.ncomp != 3) {
        err = "component count";
        return JpegStatus::Unsupported;
      }
      if (max_pixels > 0 && (int64_t)info.width * info.height > max_pixels) {
        err = "Failed to decode image: image too large (" + std::to_string(info.width) + "x" +
              std::to_string(info.height) + " pixels > " + std::to_string(max_pixels) + ")";
        return JpegStatus::Corrupt;
      }
      for (int c = 0; c < info.ncomp; ++c) {
        info.comp_id[c] = seg[6 + 3 * c];
        info.comp[c].h = seg[7 + 3 * c] >> 4;
        info.comp[c].v = seg[7 + 3 * c] & 15;
        info.tq[c] = seg[8 + 3 * c];
        if (info.comp[c].h < 1 || info.comp[c].h > 4 || info.comp[c].v < 1 || info.comp[c].v > 4 || info.tq[c] > 3) {
          err = "Failed to decode image: bad sampling factors";
          return JpegStatus::Corrupt;
        }
      }
    } else if (m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) ||
               (m >= 0xCD && m <= 0xCF)) {
      err = "progressive, lossless or arithmetic-coded JPEG";
      return JpegStatus::Unsupported;
    } else if (m == 0xC4) {
      if (!read_dht(seg, sl, info.dc, info.ac)) {
        err = "Failed to decode image: bad DHT";
        return JpegStatus::Corrupt;
      }
    } else if (m == 0xDB) {
      size_t q = 0;
      while (q < sl) {
        const int pq = seg[q] >> 4, tq = seg[q] & 15;
        const size_t need = 1 + (pq ? 128 : 64);
        if (pq > 1 || tq > 3 || q + need > sl) {
          err = "Failed to decode image: bad DQT";
          return JpegStatus::Corrupt;
        }
        for (int k = 0; k < 64; ++k)
          qtab[tq][kNatural[k]] = pq ? be16(seg + q + 1 + 2 * k) : seg[q + 1 + k];
        qpresent[tq] = true;
        q += need;
      }
    } else if (m == 0xDD) {
      if (sl < 2) {
        err = "Failed to decode image: bad DRI";
        return JpegStatus::Corrupt;
      }
      info.restart_interval = be16(seg);
    } else if (m == 0xE0) {
      if (sl >= 5 && std::memcmp(seg, "JFIF\0", 5) == 0) saw_jfif = true;
    } else if (m == 0xE1) {
      if (!saw_exif) {  // the first EXIF segment decides, well-formed or not
        const int o = exif_orientation(seg, sl);
        if (o) {
          saw_exif = true;
          info.orientation = o;
        }
      }
    } else if (m == 0xEE) {
      if (sl >= 12 && std::memcmp(seg, "Adobe", 5) == 0) {
        adobe = true;
        adobe_transform = seg[11];
      }
    } else if (m == 0xDA) {
      if (!saw_sof) {
        err = "Failed to decode image: scan before frame header";
        return JpegStatus::Corrupt;
      }
      if (info.progressive) {  // the scans are walked by the decode functions (decode_scans)
        info.first_sos = pos - len;
        info.scan_begin = pos;
        break;
      }
      const int ns = sl >= 1 ? seg[0] : 0;
      // a first scan that is not all components in the frame's order: the walker takes every scan, as for a
      // progressive file, and decides there what it cannot vouch for
      bool in_order = ns == info.ncomp && sl >= 1 + 2 * (size_t)ns + 3;
      for (int i = 0; in_order && i < ns; ++i) in_order = seg[1 + 2 * i] == info.comp_id[i];
      if (!in_order && info.ncomp > 1 && ns >= 1 && ns <= info.ncomp && sl >= 1 + 2 * (size_t)ns + 3) {
        info.multiscan = true;
        info.first_sos = pos - len;
        info.scan_begin = pos;
        break;
      }
      if (ns != info.ncomp) {
        err = "scan component count";
        return JpegStatus::Unsupported;
      }
      if (sl < 1 + 2 * (size_t)ns + 3) {
        err = "Failed to decode image: bad SOS";
        return JpegStatus::Corrupt;
      }
      for (int i = 0; i < ns; ++i) {
        const int cs = seg[1 + 2 * i];
        if (cs != info.comp_id[i]) {
          err = "scan component order differs from the frame";
          return JpegStatus::Unsupported;
        }
        info.td[i] = seg[2 + 2 * i] >> 4;
        info.ta[i] = seg[2 + 2 * i] & 15;
        if (info.td[i] > 3 || info.ta[i] > 3 || !info.dc[info.td[i]].present || !info.ac[info.ta[i]].present) {
          err = "Failed to decode image: missing Huffman table";
          return JpegStatus::Corrupt;
        }
      }
      const uint8_t* t = seg + 1 + 2 * ns;
      if (t[0] != 0 || t[1] != 63 || t[2] != 0) {
        err = "Failed to decode image: bad spectral selection for a sequential scan";
        return JpegStatus::Corrupt;
      }
      info.scan_begin = pos;
      break;
    }
    // every other marker (APPn, COM, ...) is skipped by its length
  }
  // colour space as libjpeg guesses it (jdapimin.c default_decompress_parms): JFIF means YCbCr; else an Adobe
  // segment decides by its transform (0: RGB); else the component ids R, G, B mean RGB; everything else is YCbCr
  if (info.ncomp == 3 && !saw_jfif)
    info.rgb_coded = adobe ? adobe_transform == 0
                           : info.comp_id[0] == 'R' && info.comp_id[1] == 'G' && info.comp_id[2] == 'B';
  for (int c = 0; c < info.ncomp; ++c) {
    if (!qpresent[info.tq[c]]) {
      err = "Failed to decode image: missing quantization table";
      return JpegStatus::Corrupt;
    }
    std::memcpy(info.qt[c], qtab[info.tq[c]], sizeof info.qt[c]);
    info.hmax = std::max(info.hmax, info.comp[c].h);
    info.vmax = std::max(info.vmax, info.comp[c].v);
  }
  if (info.ncomp == 1) {
    info.layout = JPEG_GRAY;
  } else {
    const JpegCompDesc &y = info.comp[0], &cb = info.comp[1], &cr = info.comp[2];
    if (cb.h != cr.h || cb.v != cr.v || y.h != info.hmax || y.v != info.vmax || y.h % cb.h || y.v % cb.v) {
      err = "chroma sampling";
      return JpegStatus::Unsupported;
    }
    // the upsampler libjpeg picks (jdsample.c jinit_upsampler): fancy for 2:1 horizontally with 1:1 or 2:1
    // vertically and for 1:1 with 2:1, integral replication for every other ratio
    const int rh = y.h / cb.h, rv = y.v / cb.v;
    info.rh = rh;
    info.rv = rv;
    if (rh == 1 && rv == 1) info.layout = JPEG_444;
    else if (rh == 2 && rv == 1) info.layout = JPEG_422;
    else if (rh == 2 && rv == 2) info.layout = JPEG_420;
    else if (rh == 1 && rv == 2) info.layout = JPEG_440;
    else info.layout = JPEG_BOX;
    // libjpeg refuses an interleaved scan whose MCU holds more than 10 blocks (D_MAX_BLOCKS_IN_MCU); PIL reports
    // it.  A file whose scans are walked is checked scan by scan.
    if (!info.progressive && !info.multiscan && y.h * y.v + cb.h * cb.v + cr.h * cr.v > 10) {
      err = "MCU larger than 10 blocks";
      return JpegStatus::Unsupported;
    }
  }
  info.mcux = (info.width + 8 * info.hmax - 1) / (8 * info.hmax);
  info.mcuy = (info.height + 8 * info.vmax - 1) / (8 * info.vmax);
  int64_t off = 0, planes = 0;
  for (int c = 0; c < info.ncomp; ++c) {
    JpegCompDesc& d = info.comp[c];
    d.cw = (int)(((int64_t)info.width * d.h + info.hmax - 1) / info.hmax);
    d.ch = (int)(((int64_t)info.height * d.v + info.vmax - 1) / info.vmax);
    if (info.ncomp == 1) {  // a single-component scan is not interleaved: one block per MCU
      d.bw = (d.cw + 7) / 8;
      d.bh = (d.ch + 7) / 8;
    } else {
      d.bw = info.mcux * d.h;
      d.bh = info.mcuy * d.v;
    }
    if ((info.layout == JPEG_422 || info.layout == JPEG_420) && c > 0 && d.cw <= 2) {
      err = "chroma narrower than 3 samples (libjpeg switches to box upsampling)";
      return JpegStatus::Unsupported;
    }
    d.coef_off = off;
    d.plane_off = planes;
    off += (int64_t)d.bw * d.bh * 64;
    planes += (int64_t)d.bw * d.bh * 64;
  }
  info.coef_count = off;
  info.plane_bytes = planes;
  const bool swap = info.orientation >= 5;
  info.out_width = swap ? info.height : info.width;
  info.out_height = swap ? info.width : info.height;
  return JpegStatus::Ok;
}

namespace {
// Built decoding tables are ~12 KB each and nearly every upload carries the same few Huffman specs (the
// standard tables of libjpeg encoders), so each decode thread keeps the tables it built last.
struct TableCache {
  struct Entry {
    JpegHuffSpec spec;
    bool ac = false;
    bool valid = false;
    uint64_t used = 0;  // generation (image) that last used the entry: never evicted while that image decodes
    HuffTable table;
  };
  static constexpr int kEntries = 8;  // > the 6 tables one 3-component image can name
  Entry e[kEntries];
  int next = 0;
  uint64_t gen = 0;
  const HuffTable* get(const JpegHuffSpec& s, bool ac) {
    for (Entry& x : e)
      if (x.valid && x.ac == ac && std::memcmp(x.spec.bits, s.bits, sizeof s.bits) == 0 &&
          std::memcmp(x.spec.vals, s.vals, sizeof s.vals) == 0) {
        x.used = gen;
        return &x.table;
      }
    while (e[next].valid && e[next].used == gen) next = (next + 1) % kEntries;
    Entry& x = e[next];
    next = (next + 1) % kEntries;
    x.valid = false;
    if (!x.table.build(s, ac)) return nullptr;
    x.spec = s;
    x.ac = ac;
    x.valid = true;
    x.used = gen;
    return &x.table;
  }
};

// ---- progressive files (SOF2, T.81 Annex G; the behaviour matched is libjpeg's jdphuff.c) -----------------------

inline bool fits16(int v) { return v >= -32768 && v <= 32767; }

// One Huffman symbol as BitReader::decode reads it, but -1 where no code matches (libjpeg warns and goes on with a
// zero: not a result to vouch for).
__attribute__((always_inline)) inline int prog_symbol(BitReader& br, const HuffTable& t) {
  const uint32_t e = t.fast[br.buf >> (64 - kFastBits)];
  if (e) {
    br.skip((int)(e >> 8));
    return (int)(e & 0xFF);
  }
  const uint32_t code16 = (uint32_t)(br.buf >> 48);
  for (int l = kFastBits + 1; l <= 16; ++l) {
    const int32_t c = (int32_t)(code16 >> (16 - l));
    if (c <= t.maxcode[l]) {
      br.skip(l);
      return t.vals[(t.valoff[l] + c) & 0xFF];
    }
  }
  return -1;
}

// What is left of the data loaded so far, zero fill not counted: a well-formed segment ends within its last byte.
inline bool prog_leftover(const BitReader& br) { return br.bits - 8 * (br.zfill + br.pad) >= 8; }

// One block of each of the four scan kinds.  They return false where libjpeg would warn or a value leaves int16:
// the file is handed back.  Runs that a corrupt stream sends past coefficient 63 land on kNatural's guard entries,
// as in libjpeg.
inline bool prog_dc_first(BitReader& br, const HuffTable& t, int& pred, int al, int16_t* blk) {
  br.need(32);
  const int s = prog_symbol(br, t);
  if (s) {
    if (s < 0 || s > 15) return false;
    pred += extend(br.get(s), s);
    if (!fits16(pred)) return false;
  }
  const int v = pred * (1 << al);
  if (!fits16(v)) return false;
  blk[0] = (int16_t)v;
  return true;
}

inline void prog_dc_refine(BitReader& br, int al, int16_t* blk) {
  br.need(1);
  if (br.get(1)) blk[0] = (int16_t)(blk[0] | (1 << al));
}

inline bool prog_ac_first(BitReader& br, const HuffTable& t, int ss, int se, int al, int& eobrun, int16_t* blk) {
  if (eobrun > 0) {  // inside a run of blocks whose band is all zero
    --eobrun;
    return true;
  }
  for (int k = ss; k <= se; ++k) {
    br.need(32);  // a code (<= 16 bits) and its magnitude or run-length bits (<= 15)
    const int32_t f = t.ac_fast[br.buf >> (64 - kFastBits)];
    if (f) {  // one lookup, as in decode_block: a coefficient, ZRL or EOB0 (a run of this block only)
      br.skip(f & 0xFF);
      const int r = (f >> 8) & 0xFF;
      if (r == kEobRun) break;
      k += r;
      const int v = (f >> 16) * (1 << al);
      if (!fits16(v)) return false;
      if (v) blk[kNatural[k]] = (int16_t)v;  // ZRL's zero is not stored: a corrupt run may end in another band
      continue;
    }
    const int rs = prog_symbol(br, t);
    if (rs < 0) return false;
    const int r = rs >> 4, s = rs & 15;
    if (s) {
      k += r;
      const int v = extend(br.get(s), s) * (1 << al);
      if (!fits16(v)) return false;
      blk[kNatural[k]] = (int16_t)v;
    } else if (r == 15) {
      k += 15;  // ZRL
    } else {    // EOBr: this block's band ends here and so do the next (1 << r) + bits - 1 blocks'
      eobrun = 1 << r;
      if (r) eobrun += (int)br.get(r);
      --eobrun;
      break;
    }
  }
  return true;
}

// the correction bit of a coefficient that earlier scans made nonzero
inline void prog_correct(BitReader& br, int16_t& c, int p1) {
  br.need(1);
  if (br.get(1) && (c & p1) == 0) c = (int16_t)(c >= 0 ? c + p1 : c - p1);
}

inline bool prog_ac_refine(BitReader& br, const HuffTable& t, int ss, int se, int al, int& eobrun, int16_t* blk) {
  const int p1 = 1 << al;
  int k = ss;
  if (eobrun == 0) {
    for (; k <= se; ++k) {
      br.need(32);
      const int rs = prog_symbol(br, t);
      if (rs < 0) return false;
      int r = rs >> 4, s = rs & 15;
      if (s) {
        if (s != 1) return false;  // a new coefficient has magnitude 1 at this bit (libjpeg warns)
        s = br.get(1) ? p1 : -p1;
      } else if (r != 15) {
        eobrun = 1 << r;
        if (r) eobrun += (int)br.get(r);
        break;  // the rest of the band is handled as the first block of the run, below
      }
      // pass r still-zero coefficients (16 for ZRL), correcting every nonzero one on the way
      do {
        int16_t& c = blk[kNatural[k]];
        if (c != 0) prog_correct(br, c, p1);
        else if (--r < 0) break;
        ++k;
      } while (k <= se);
      if (s) blk[kNatural[k]] = (int16_t)s;
    }
  }
  if (eobrun > 0) {
    for (; k <= se; ++k) {
      int16_t& c = blk[kNatural[k]];
      if (c != 0) prog_correct(br, c, p1);
    }
    --eobrun;
  }
  return true;
}

// All scans of a progressive file, or of a sequential one that comes in several scans (info.multiscan: every scan
// codes whole blocks of its components), into dense blocks (contract in jpeg_decode.h, jpeg_decode_coefs).
JpegStatus decode_scans(const uint8_t* data, size_t n, const JpegInfo& info, int16_t* coef, std::string& err) {
  const bool seq = !info.progressive;
  auto hand_back = [seq](std::string& e, const char* why) {
    e = std::string(seq ? "multi-scan" : "progressive") + " JPEG outside the split decoder: " + why;
    return JpegStatus::Unsupported;
  };
  thread_local std::unique_ptr<TableCache> cache;
  if (!cache) cache.reset(new TableCache());
  std::memset(coef, 0, (size_t)info.coef_count * sizeof(int16_t));
  RangeQuant rq[kJpegMaxComp];
  range_quant(info, rq);
  JpegHuffSpec dc[4], ac[4];  // DHT between scans redefines them
  for (int i = 0; i < 4; ++i) {
    dc[i] = info.dc[i];
    ac[i] = info.ac[i];
  }
  int ri = info.restart_interval;
  // successive-approximation bit each coefficient is down to: -1 = never sent
  int8_t sent[kJpegMaxComp][64];
  std::memset(sent, -1, sizeof sent);
  bool coded[kJpegMaxComp] = {false, false, false};  // sequential: the component had its scan
  const char* const kTruncated = "Failed to decode image: image file is truncated";
  size_t pos = info.first_sos;
  for (int nscan = 1;; ++nscan) {
    if (nscan > kJpegMaxScans) return hand_back(err, "too many scans");
    // ---- scan header (pos: its length field) ----
    if (pos + 2 > n) {
      err = "Failed to decode image: truncated marker";
      return JpegStatus::Corrupt;
    }
    const size_t len = be16(data + pos);
    if (len < 2 || pos + len > n) {
      err = "Failed to decode image: truncated marker segment";
      return JpegStatus::Corrupt;
    }
    const uint8_t* seg = data + pos + 2;
    const size_t sl = len - 2;
    const int ns = sl >= 1 ? seg[0] : 0;
    if (ns < 1 || ns > info.ncomp) return hand_back(err, "scan component count");
    if (sl < 1 + 2 * (size_t)ns + 3) {
      err = "Failed to decode image: bad SOS";
      return JpegStatus::Corrupt;
    }
    if (sl != 1 + 2 * (size_t)ns + 3) return hand_back(err, "SOS length");
    int ci[kJpegMaxComp] = {}, td[kJpegMaxComp] = {}, ta[kJpegMaxComp] = {};
    int mcu_blocks = 0;
    for (int i = 0; i < ns; ++i) {
      const int cs = seg[1 + 2 * i];
      int c = i ? ci[i - 1] + 1 : 0;  // in the frame's order, none twice
      while (c < info.ncomp && info.comp_id[c] != cs) ++c;
      if (c >= info.ncomp) return hand_back(err, "scan component selector");
      ci[i] = c;
      td[i] = seg[2 + 2 * i] >> 4;
      ta[i] = seg[2 + 2 * i] & 15;
      mcu_blocks += info.comp[c].h * info.comp[c].v;
    }
    const uint8_t* sp = seg + 1 + 2 * ns;
    const int ss = sp[0], se = sp[1], ah = sp[2] >> 4, al = sp[2] & 15;
    if (seq) {
      // libjpeg only warns about other parameters in a sequential scan and decodes whole blocks all the same
      if (ss != 0 || se != 63 || ah != 0 || al != 0) return hand_back(err, "spectral selection of a sequential scan");
      // it outputs whatever the scans left in a component: exact only when each had exactly one
      for (int i = 0; i < ns; ++i) {
        if (coded[ci[i]]) return hand_back(err, "component coded twice");
        coded[ci[i]] = true;
      }
    } else {
      // G.1.1.1.1
      if (ss == 0 ? se != 0 : (ns != 1 || ss > se || se > 63)) return hand_back(err, "spectral selection");
      if ((ah != 0 && ah != al + 1) || al > 13) return hand_back(err, "successive approximation");
    }
    if (ns > 1 && mcu_blocks > 10) return hand_back(err, "MCU larger than 10 blocks");
    for (int i = 0; !seq && i < ns; ++i) {
      int8_t* s = sent[ci[i]];
      if (ss > 0 && s[0] < 0) return hand_back(err, "AC scan before the component's DC");
      for (int k = ss; k <= se; ++k) {
        // first scan of a coefficient sent before, refinement of one never sent, or Ah that is not the last Al
        if (ah == 0 ? s[k] >= 0 : s[k] != ah) return hand_back(err, "inconsistent progression");
        s[k] = (int8_t)al;
      }
    }
    const HuffTable* tab[kJpegMaxComp] = {};
    const HuffTable* actab[kJpegMaxComp] = {};  // sequential: a block takes both tables
    ++cache->gen;
    if (seq) {
      for (int i = 0; i < ns; ++i) {
        if (td[i] > 3 || ta[i] > 3 || !dc[td[i]].present || !ac[ta[i]].present) {
          err = "Failed to decode image: missing Huffman table";
          return JpegStatus::Corrupt;
        }
        tab[i] = cache->get(dc[td[i]], false);
        actab[i] = tab[i] ? cache->get(ac[ta[i]], true) : nullptr;
        if (!tab[i] || !actab[i]) {
          err = "Failed to decode image: bad Huffman table";
          return JpegStatus::Corrupt;
        }
      }
    } else if (ss > 0 || ah == 0) {  // a DC refinement scan carries raw bits only
      for (int i = 0; i < ns; ++i) {
        const int th = ss > 0 ? ta[i] : td[i];
        if (th > 3 || !(ss > 0 ? ac : dc)[th].present) {
          err = "Failed to decode image: missing Huffman table";
          return JpegStatus::Corrupt;
        }
        tab[i] = cache->get((ss > 0 ? ac : dc)[th], ss > 0);
        if (!tab[i]) {
          err = "Failed to decode image: bad Huffman table";
          return JpegStatus::Corrupt;
        }
      }
    }
    pos += len;
    // ---- entropy-coded segment ----
    // A scan of one component is not interleaved: it covers the component's real blocks, row by row, and its
    // restart interval counts them; the MCU padding of the grid (bw x bh) belongs to interleaved scans only.
    const bool single = ns == 1;
    const JpegCompDesc& d0 = info.comp[ci[0]];
    const int sbw = single ? (d0.cw + 7) / 8 : info.mcux, sbh = single ? (d0.ch + 7) / 8 : info.mcuy;
    const int64_t n_mcu = (int64_t)sbw * sbh;
    const int kind = seq ? 4 : ss == 0 ? (ah == 0 ? 0 : 1) : (ah == 0 ? 2 : 3);
    BitReader br{data + pos, data + n};
    int pred[kJpegMaxComp] = {0, 0, 0};
    int eobrun = 0;
    int todo = ri;
    bool wide = false;  // sequential scans: a block outside the coefficient range
    auto block = [&](int i, int16_t* blk) -> bool {
      switch (kind) {
        case 0: return prog_dc_first(br, *tab[i], pred[i], al, blk);
        case 1: prog_dc_refine(br, al, blk); return true;
        case 2: return prog_ac_first(br, *tab[i], ss, se, al, eobrun, blk);
        case 3: return prog_ac_refine(br, *tab[i], ss, se, al, eobrun, blk);
        // a whole block as a baseline scan codes it; bits that match no code make libjpeg warn
        default: return decode_block(br, *tab[i], *actab[i], pred[i], blk, rq[ci[i]], wide) && !br.bad_code;
      }
    };
    int next_rst = 0;
    for (int64_t m = 0; m < n_mcu; ++m) {
      if (ri) {
        if (todo == 0) {
          // the interval used up its bytes and RSTn, the expected n, follows at once; anything else makes libjpeg
          // warn and resynchronise by guesswork
          if (br.overran() || br.end - br.p < 2) {  // the file ends here
            err = kTruncated;
            return JpegStatus::Corrupt;
          }
          if (prog_leftover(br) || br.p[0] != 0xFF || br.p[1] != 0xD0 + next_rst)
            return hand_back(err, "restart marker out of place");
          next_rst = (next_rst + 1) & 7;
          br.restart();
          pred[0] = pred[1] = pred[2] = 0;
          eobrun = 0;
          todo = ri;
        }
        --todo;
      }
      const int my = (int)(m / sbw), mx = (int)(m % sbw);
      if (single) {
        if (!block(0, coef + d0.coef_off + ((int64_t)my * d0.bw + mx) * 64)) return hand_back(err, "coefficient value");
      } else {
        for (int i = 0; i < ns; ++i) {
          const JpegCompDesc& d = info.comp[ci[i]];
          for (int v = 0; v < d.v; ++v) {
            int16_t* row = coef + d.coef_off + (((int64_t)my * d.v + v) * d.bw + (int64_t)mx * d.h) * 64;
            for (int h = 0; h < d.h; ++h)
              if (!block(i, row + h * 64)) return hand_back(err, "coefficient value");
          }
        }
      }
      // a marker cut the segment short and zero bits were read past it: libjpeg warns, and skips what follows
      if (br.starved()) return hand_back(err, "scan data ends early");
      if (wide) return hand_back(err, kRangeMessage);
    }
    if (br.truncated || br.overran()) {
      err = kTruncated;
      return JpegStatus::Corrupt;
    }
    if (prog_leftover(br)) return hand_back(err, "scan data left over");
    // ---- markers up to the next scan or EOI ----
    size_t q = (size_t)(br.p - data);
    bool eoi = false;
    for (;;) {
      if (q < n && data[q] != 0xFF) return hand_back(err, "bytes between a scan and the next marker");
      while (q < n && data[q] == 0xFF) ++q;
      if (q >= n) {  // no EOI: libjpeg waits for more data, PIL raises
        err = kTruncated;
        return JpegStatus::Corrupt;
      }
      const int m = data[q++];
      if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
      if (m == 0xD9) {
        eoi = true;
        break;
      }
      if (m == 0xD8) return hand_back(err, "SOI between scans");
      if (q + 2 > n) {
        err = "Failed to decode image: truncated marker";
        return JpegStatus::Corrupt;
      }
      const size_t ml = be16(data + q);
      if (ml < 2 || q + ml > n) {
        err = "Failed to decode image: truncated marker segment";
        return JpegStatus::Corrupt;
      }
      if (m == 0xDA) break;
      if (m == 0xC4) {
        if (!read_dht(data + q + 2, ml - 2, dc, ac)) {
          err = "Failed to decode image: bad DHT";
          return JpegStatus::Corrupt;
        }
      } else if (m == 0xDD) {
        if (ml < 4) {
          err = "Failed to decode image: bad DRI";
          return JpegStatus::Corrupt;
        }
        ri = be16(data + q + 2);
      } else if (!((m >= 0xE0 && m <= 0xEF) || m == 0xFE)) {
        return hand_back(err, m == 0xDB ? "DQT between scans" : "marker between scans");
      }
      q += ml;
    }
    if (eoi) break;
    pos = q;
  }
  if (seq) {
    for (int c = 0; c < info.ncomp; ++c)
      if (!coded[c]) return hand_back(err, "component never coded");
    return JpegStatus::Ok;
  }
  // libjpeg smooths (and PIL returns the smoothed image) when the file ends before every coefficient is exact
  for (int c = 0; c < info.ncomp; ++c)
    for (int k = 0; k < 64; ++k)
      if (sent[c][k] != 0) return hand_back(err, "incomplete progression");
  // the coefficient range, now that every scan has had its say
  for (int c = 0; c < info.ncomp; ++c) {
    const JpegCompDesc& d = info.comp[c];
    const int16_t* blk = coef + d.coef_off;
    for (int64_t b = 0, nb = (int64_t)d.bw * d.bh; b < nb; ++b, blk += 64) {
      uint64_t sum = 0;
      for (int k = 0; k < 64; ++k) sum += range_term(blk[k], info.qt[c][k]);
      if (range_wide(sum)) return hand_back(err, kRangeMessage);
    }
  }
  return JpegStatus::Ok;
}
}  // namespace

JpegStatus jpeg_decode_coefs(const uint8_t* data, size_t n, const JpegInfo& info, int16_t* coef, std::string& err) {
  if (info.progressive || info.multiscan) return decode_scans(data, n, info, coef, err);
  thread_local std::unique_ptr<TableCache> cache;
  if (!cache) cache.reset(new TableCache());
  const HuffTable* dcp[kJpegMaxComp] = {};
  const HuffTable* acp[kJpegMaxComp] = {};
  ++cache->gen;
  for (int c = 0; c < info.ncomp; ++c) {
    dcp[c] = cache->get(info.dc[info.td[c]], false);
    acp[c] = dcp[c] ? cache->get(info.ac[info.ta[c]], true) : nullptr;
    if (!dcp[c] || !acp[c]) {
      err = "Failed to decode image: bad Huffman table";
      return JpegStatus::Corrupt;
    }
  }
  RangeQuant rq[kJpegMaxComp];
  range_quant(info, rq);
  bool wide = false;  // some block is outside the coefficient range: reported once the scan has proved sound
  BitReader br{data + info.scan_begin, data + n};
  int pred[kJpegMaxComp] = {0, 0, 0};
  const bool single = info.ncomp == 1;
  const int64_t n_mcu = single ? (int64_t)info.comp[0].bw * info.comp[0].bh : (int64_t)info.mcux * info.mcuy;
  const int ri = info.restart_interval;
  int todo = ri;
  bool starved = false;
  for (int64_t m = 0; m < n_mcu; ++m) {
    if (ri) {
      if (todo == 0) {
        br.restart();
        pred[0] = pred[1] = pred[2] = 0;
        todo = ri;
        // a segment that starts right at another marker stays starved (libjpeg process_restart)
        starved = br.p + 1 < br.end && br.p[0] == 0xFF && br.p[1] != 0x00 && !(br.p[1] >= 0xD0 && br.p[1] <= 0xD7)
                      ? starved : false;
      }
      --todo;
    }
    if (starved) {  // insufficient data: zero blocks, predictions untouched (jdhuff.c decode_mcu)
      if (single) {
        std::memset(coef + m * 64, 0, 64 * sizeof(int16_t));
      } else {
        const int my = (int)(m / info.mcux), mx = (int)(m % info.mcux);
        for (int c = 0; c < info.ncomp; ++c) {
          const JpegCompDesc& d = info.comp[c];
          for (int v = 0; v < d.v; ++v)
            std::memset(coef + d.coef_off + (((int64_t)my * d.v + v) * d.bw + (int64_t)mx * d.h) * 64, 0,
                        (size_t)d.h * 64 * sizeof(int16_t));
        }
      }
      continue;
    }
    if (single) {
      if (!decode_block(br, *dcp[0], *acp[0], pred[0], coef + m * 64, rq[0], wide)) {
        err = "Failed to decode image: bad DC magnitude";
        return JpegStatus::Corrupt;
      }
      starved = br.starved();
      continue;
    }
    const int my = (int)(m / info.mcux), mx = (int)(m % info.mcux);
    for (int c = 0; c < info.ncomp; ++c) {
      const JpegCompDesc& d = info.comp[c];
      for (int v = 0; v < d.v; ++v) {
        int16_t* row = coef + d.coef_off + (((int64_t)my * d.v + v) * d.bw + (int64_t)mx * d.h) * 64;
        for (int h = 0; h < d.h; ++h) {
          if (!decode_block(br, *dcp[c], *acp[c], pred[c], row + h * 64, rq[c], wide)) {
            err = "Failed to decode image: bad DC magnitude";
            return JpegStatus::Corrupt;
          }
        }
      }
    }
    starved = br.starved();
  }
  if (br.truncated || br.overran()) {
    err = "Failed to decode image: image file is truncated";
    return JpegStatus::Corrupt;
  }
  if (wide) {
    err = kRangeMessage;
    return JpegStatus::Unsupported;
  }
  return JpegStatus::Ok;
}

int64_t jpeg_total_blocks(const JpegInfo& info) {
  int64_t t = 0;
  for (int c = 0; c < info.ncomp; ++c) t += (int64_t)info.comp[c].bw * info.comp[c].bh;
  return t;
}

int64_t jpeg_compact_capacity(const JpegInfo& info) {
  const int64_t tb = jpeg_total_blocks(info);
  return ((tb * 12 + 15) & ~(int64_t)15) + tb * 128;
}

bool jpeg_compact_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("ARENA_JPEG_COMPACT");
    return e == nullptr || std::atoi(e) != 0;
  }();
  return on;
}

int64_t jpeg_payload_bytes(const JpegInfo& info) { return info.compact_bytes >= 0 ? info.compact_bytes : info.coef_count * 2; }

namespace {
// Dense blocks into the compact payload, with the scan decoder's convention: the DC is always coded (bit 0 set,
// its value stored even when 0), every other coefficient when it is not zero.
void dense_to_compact(JpegInfo& info, const int16_t* coef, uint8_t* out) {
  const int64_t tb = jpeg_total_blocks(info);
  uint64_t* masks = (uint64_t*)out;
  uint32_t* voff = (uint32_t*)(out + tb * 8);
  const int64_t val_at = (tb * 12 + 15) & ~(int64_t)15;
  int16_t* vals = (int16_t*)(out + val_at);
  int64_t nv = 0;
  uint8_t zigzag_of[64];  // natural index -> zigzag index
  for (int k = 0; k < 64; ++k) zigzag_of[kNatural[k]] = (uint8_t)k;
  for (int64_t b = 0; b < tb; ++b) {
    const int16_t* blk = coef + b * 64;
    voff[b] = (uint32_t)nv;
    // most coefficients are zero: find the others four at a time, then visit only them, in zigzag order
    uint64_t m = 1;
    for (int w = 0; w < 16; ++w) {
      uint64_t four;
      std::memcpy(&four, blk + 4 * w, sizeof four);
      if (four == 0) continue;
      for (int j = 4 * w; j < 4 * w + 4; ++j) m |= (uint64_t)(blk[j] != 0) << zigzag_of[j];
    }
    masks[b] = m;
    do {
      vals[nv++] = blk[kNatural[__builtin_ctzll(m)]];
      m &= m - 1;
    } while (m);
  }
  info.compact_bytes = val_at + nv * 2;
  info.cmask_off = 0;
  info.cvoff_off = tb * 8;
  info.cval_off = val_at;
}
}  // namespace

JpegStatus jpeg_decode_compact(const uint8_t* data, size_t n, JpegInfo& info, uint8_t* out, std::string& err) {
  if (info.progressive || info.multiscan) {  // the scans fill dense blocks; the payload is packed after the last one
    thread_local std::vector<int16_t> dense;
    dense.resize((size_t)info.coef_count);
    const JpegStatus st = decode_scans(data, n, info, dense.data(), err);
    if (st == JpegStatus::Ok) dense_to_compact(info, dense.data(), out);
    if (dense.capacity() > ((size_t)16 << 20)) std::vector<int16_t>().swap(dense);  // do not pin a huge frame's
    return st;
  }
  thread_local std::unique_ptr<TableCache> cache;
  if (!cache) cache.reset(new TableCache());
  const HuffTable* dcp[kJpegMaxComp] = {};
  const HuffTable* acp[kJpegMaxComp] = {};
  ++cache->gen;
  for (int c = 0; c < info.ncomp; ++c) {
    dcp[c] = cache->get(info.dc[info.td[c]], false);
    acp[c] = dcp[c] ? cache->get(info.ac[info.ta[c]], true) : nullptr;
    if (!dcp[c] || !acp[c]) {
      err = "Failed to decode image: bad Huffman table";
      return JpegStatus::Corrupt;
    }
  }
  const int64_t tb = jpeg_total_blocks(info);
  uint64_t* masks = (uint64_t*)out;
  uint32_t* voff = (uint32_t*)(out + tb * 8);
  const int64_t val_at = (tb * 12 + 15) & ~(int64_t)15;
  int16_t* vals = (int16_t*)(out + val_at);
  int64_t nv = 0;
  RangeQuant rq[kJpegMaxComp];
  range_quant(info, rq);
  bool wide = false;  // as in jpeg_decode_coefs
  BitReader br{data + info.scan_begin, data + n};
  int pred[kJpegMaxComp] = {0, 0, 0};
  const bool single = info.ncomp == 1;
  const int64_t n_mcu = single ? (int64_t)info.comp[0].bw * info.comp[0].bh : (int64_t)info.mcux * info.mcuy;
  const int ri = info.restart_interval;
  int todo = ri;
  bool starved = false;
  auto block = [&](int c, int64_t gb) -> bool {
    voff[gb] = (uint32_t)nv;
    if (starved) {  // insufficient data: an all-zero block, predictions untouched (jdhuff.c decode_mcu)
      masks[gb] = 0;
      return true;
    }
    return decode_block_compact(br, *dcp[c], *acp[c], pred[c], masks + gb, vals, nv, rq[c], wide);
  };
  for (int64_t m = 0; m < n_mcu; ++m) {
    if (ri) {
      if (todo == 0) {
        br.restart();
        pred[0] = pred[1] = pred[2] = 0;
        todo = ri;
        starved = br.p + 1 < br.end && br.p[0] == 0xFF && br.p[1] != 0x00 && !(br.p[1] >= 0xD0 && br.p[1] <= 0xD7)
                      ? starved : false;
      }
      --todo;
    }
    const bool was_starved = starved;
    if (single) {
      if (!block(0, m)) {
        err = "Failed to decode image: bad DC magnitude";
        return JpegStatus::Corrupt;
      }
    } else {
      const int my = (int)(m / info.mcux), mx = (int)(m % info.mcux);
      for (int c = 0; c < info.ncomp; ++c) {
        const JpegCompDesc& d = info.comp[c];
        for (int v = 0; v < d.v; ++v)
          for (int h = 0; h < d.h; ++h) {
            const int64_t gb = d.coef_off / 64 + ((int64_t)my * d.v + v) * d.bw + (int64_t)mx * d.h + h;
            if (!block(c, gb)) {
              err = "Failed to decode image: bad DC magnitude";
              return JpegStatus::Corrupt;
            }
          }
      }
    }
    if (!was_starved) starved = br.starved();
  }
  if (br.truncated || br.overran()) {
    err = "Failed to decode image: image file is truncated";
    return JpegStatus::Corrupt;
  }
  if (wide) {
    err = kRangeMessage;
    return JpegStatus::Unsupported;
  }
  info.compact_bytes = val_at + nv * 2;
  info.cmask_off = 0;
  info.cvoff_off = tb * 8;
  info.cval_off = val_at;
  return JpegStatus::Ok;
}

void jpeg_compact_to_dense(const JpegInfo& info, const uint8_t* payload, int16_t* coef) {
  const int64_t tb = jpeg_total_blocks(info);
  const uint64_t* masks = (const uint64_t*)(payload + info.cmask_off);
  const uint32_t* voff = (const uint32_t*)(payload + info.cvoff_off);
  const int16_t* vals = (const int16_t*)(payload + info.cval_off);
  for (int64_t b = 0; b < tb; ++b) {
    int16_t* blk = coef + b * 64;
    std::memset(blk, 0, 64 * sizeof(int16_t));
    uint64_t m = masks[b];
    int64_t i = voff[b];
    while (m) {
      const int k = __builtin_ctzll(m);
      blk[kNatural[k]] = vals[i++];
      m &= m - 1;
    }
  }
}

const int16_t* jpeg_dense_coefs(const JpegInfo& info, const uint8_t* payload, std::vector<int16_t>& scratch) {
  if (info.compact_bytes < 0) return (const int16_t*)payload;
  scratch.resize((size_t)info.coef_count);
  jpeg_compact_to_dense(info, payload, scratch.data());
  return scratch.data();
}

void jpeg_coefs_to_rgb(const JpegInfo& info, const int16_t* coef, uint8_t* rgb) {
  using namespace jpegm;
  std::vector<uint8_t> planes((size_t)info.plane_bytes);
  for (int c = 0; c < info.ncomp; ++c) {
    const JpegCompDesc& d = info.comp[c];
    const int stride = d.bw * 8;
    for (int by = 0; by < d.bh; ++by) {
      for (int bx = 0; bx < d.bw; ++bx) {
        const int16_t* in = coef + d.coef_off + ((int64_t)by * d.bw + bx) * 64;
        int64_t ws[64];
        for (int col = 0; col < 8; ++col) {
          int64_t v[8], o[8];
          for (int r = 0; r < 8; ++r) v[r] = (int64_t)in[r * 8 + col] * info.qt[c][r * 8 + col];
          idct8<int64_t>(v, o, kPass1Shift);
          for (int r = 0; r < 8; ++r) ws[r * 8 + col] = o[r];
        }
        for (int r = 0; r < 8; ++r) {
          int64_t o[8];
          idct8<int64_t>(ws + r * 8, o, kPass2Shift);
          uint8_t* dst = planes.data() + d.plane_off + (int64_t)(by * 8 + r) * stride + bx * 8;
          for (int k = 0; k < 8; ++k) dst[k] = idct_sample<int64_t>(o[k]);
        }
      }
    }
  }
  const JpegCompDesc& Y = info.comp[0];
  const uint8_t* yp = planes.data() + Y.plane_off;
  const int ys = Y.bw * 8;
  const int W = info.width, H = info.height, ori = info.orientation;
  for (int y = 0; y < info.height; ++y) {
    for (int x = 0; x < info.width; ++x) {
      int64_t at;  // output pixel index of source (y, x)
      switch (ori) {
        case 2: at = (int64_t)y * W + (W - 1 - x); break;
        case 3: at = (int64_t)(H - 1 - y) * W + (W - 1 - x); break;
        case 4: at = (int64_t)(H - 1 - y) * W + x; break;
        case 5: at = (int64_t)x * H + y; break;
        case 6: at = (int64_t)x * H + (H - 1 - y); break;
        case 7: at = (int64_t)(W - 1 - x) * H + (H - 1 - y); break;
        case 8: at = (int64_t)(W - 1 - x) * H + y; break;
        default: at = (int64_t)y * W + x; break;
      }
      uint8_t* o = rgb + at * 3;
      const int yy = yp[(int64_t)y * ys + x];
      if (info.layout == JPEG_GRAY) {
        o[0] = o[1] = o[2] = (uint8_t)yy;
        continue;
      }
      int cc[2];
      for (int k = 0; k < 2; ++k) {
        const JpegCompDesc& C = info.comp[1 + k];
        const uint8_t* cp = planes.data() + C.plane_off;
        const int cs = C.bw * 8;
        if (info.layout == JPEG_444) {
          cc[k] = cp[(int64_t)y * cs + x];
        } else if (info.layout == JPEG_422) {
          const int cx = x >> 1, xo = x & 1;
          const int nx = xo ? std::min(cx + 1, C.cw - 1) : std::max(cx - 1, 0);
          cc[k] = fancy_h2v1(cp[(int64_t)y * cs + cx], cp[(int64_t)y * cs + nx], xo);
        } else if (info.layout == JPEG_420) {
          const int cx = x >> 1, xo = x & 1, cy = y >> 1;
          const int nx = xo ? std::min(cx + 1, C.cw - 1) : std::max(cx - 1, 0);
          const int ny = (y & 1) ? std::min(cy + 1, C.ch - 1) : std::max(cy - 1, 0);
          cc[k] = fancy_h2v2(cp[(int64_t)cy * cs + cx], cp[(int64_t)cy * cs + nx], cp[(int64_t)ny * cs + cx],
                             cp[(int64_t)ny * cs + nx], xo);
        } else if (info.layout == JPEG_440) {
          const int cy = y >> 1;
          const int ny = (y & 1) ? std::min(cy + 1, C.ch - 1) : std::max(cy - 1, 0);
          cc[k] = fancy_h1v2(cp[(int64_t)cy * cs + x], cp[(int64_t)ny * cs + x], y & 1);
        } else {  // JPEG_BOX
          const int cx = std::min(box_coord(x, info.rh), C.cw - 1), cy = std::min(box_coord(y, info.rv), C.ch - 1);
          cc[k] = cp[(int64_t)cy * cs + cx];
        }
      }
      if (info.rgb_coded) rgb_identity(yy, cc[0], cc[1], o);
      else ycc_to_rgb(yy, cc[0], cc[1], o);
    }
  }
}

JpegDesc jpeg_device_desc(const JpegInfo& info, int64_t coef_base, int64_t plane_base, int64_t rgb_off) {
  JpegDesc d;
  std::memset(&d, 0, sizeof d);
  d.ncomp = info.ncomp;
  d.layout = info.layout;
  d.width = info.width;
  d.height = info.height;
  d.orientation = info.orientation;
  d.rh = (uint8_t)info.rh;
  d.rv = (uint8_t)info.rv;
  d.no_transform = info.rgb_coded ? 1 : 0;
  d.rgb_off = rgb_off;
  int64_t total = 0;
  for (int c = 0; c < info.ncomp; ++c) {
    d.comp[c] = info.comp[c];
    d.comp[c].coef_off = coef_base + info.comp[c].coef_off * 2;
    d.comp[c].plane_off = plane_base + info.comp[c].plane_off;
    total += (int64_t)info.comp[c].bw * info.comp[c].bh;
    std::memcpy(d.qt[c], info.qt[c], sizeof d.qt[c]);
  }
  d.total_blocks = (int32_t)total;
  if (info.compact_bytes >= 0) {  // compact payload at coef_base (jpeg_decode_compact)
    d.compact = 1;
    d.cmask_off = coef_base + info.cmask_off;
    d.cvoff_off = coef_base + info.cvoff_off;
    d.cval_off = coef_base + info.cval_off;
  }
  return d;
}

}  // namespace arena
