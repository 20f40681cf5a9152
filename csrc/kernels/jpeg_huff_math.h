// Huffman-coding arithmetic of a baseline 4:2:0 JPEG scan, shared by the host (csrc/runtime/jpeg_encode.cpp:
// jpeg_entropy_phased_host) and the device entropy coder (csrc/kernels/jpeg_huff.hip).  It restates what jpeg_write
// and its encode_block (jchuff.c encode_one_block) do serially as functions of a slot's own data, so that every
// block slot can be sized and coded independently:
//
//   slot rules   a slot of an MCU (Y00 Y01 Y10 Y11 Cb Cr) is real or dummy (slot_real).  Its effective DC is its own
//                coefficient 0 if it is real, else the effective DC of the slot before it in the same MCU (slot 0 is
//                always real).  Its predictor is the effective DC of the previous slot of the same component in scan
//                order, 0 at the start of the scan.
//   symbols      dc_symbol: the code of the DC difference.  ac_symbol: everything encode_block emits when it reaches
//                the non-zero coefficient at zigzag index k, i.e. the ZRL symbols of a run above 15, the (run, size)
//                code and the value bits; the run comes from the mask of non-zero coefficients alone.  eob_symbol:
//                the end-of-block code, unless coefficient 63 is non-zero.
//   block_bits   the sum of the symbols' lengths: exactly the bits encode_block emits for the slot.
//   put_bits     the emit step: OR a symbol into a bit buffer of 32-bit words, MSB first (bit p of the stream is bit
//                31 - (p & 31) of word p >> 5; store_be32 gives the word's bytes in stream order).
//   stuffing     pad_bits / stuffed_at: the last byte is padded with 1-bits, then every 0xFF byte is followed by 0x00.
//
// Domain: |coefficient| <= kMaxCoef (1023), which the forward DCT meets at quality 95.  The symbol functions clamp
// the magnitude to the domain, so a coefficient outside it gives wrong bits but never more than kMaxBlockBits of
// them: the device buffers are sized by that bound.
//
// Code tables: symbol -> code | length << 16, 256 entries each, in the DHT order DC0, AC0, DC1, AC1
// (jpeg_enc_code_tables in jpeg_encode.cpp defines them once).  As in jpeg_enc_math.h nothing here owns memory.
#pragma once
#include "jpeg_math.h"

namespace arena {
namespace jpegh {

constexpr int kMaxCoef = 1023;
// DC: an 11-bit code at most (chroma, size 11) + 11 value bits; AC: 63 x (16-bit code + 10 value bits).
constexpr int kMaxBlockBits = 22 + 63 * 26;                     // 1660
constexpr int kBitBufBytesPerSlot = 256;                        // >= kMaxBlockBits / 8, a power of two
constexpr int kEntropyReserve = 128;                            // scan bytes reserved per block slot
constexpr int kStuffSegment = 4096;                             // unstuffed bytes one workgroup stuffs
constexpr int kCodeTableEntries = 256;

// zigzag index of natural index
constexpr uint8_t kZigzagOf[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                   41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                   46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

ARENA_JHD int bit_length(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

// Is slot s of MCU `mcu` inside its component's real block grid?  Luma: ceil(w / 8) x ceil(h / 8) blocks; the chroma
// grid ceil(cw / 8) x ceil(ch / 8) equals the MCU grid, so a chroma slot is always real, and so is luma slot 0.
ARENA_JHD bool slot_real(int w, int h, int mcux, int mcu, int s) {
  if (s >= 4) return true;
  const int my = mcu / mcux, mx = mcu - my * mcux;
  return 2 * my + (s >> 1) < (h + 7) / 8 && 2 * mx + (s & 1) < (w + 7) / 8;
}

// dc_at(slot index in scan order) reads coefficient 0 of a slot.
template <typename DcAt>
ARENA_JHD int effective_dc(int w, int h, int mcux, int mcu, int s, const DcAt& dc_at) {
  while (s > 0 && !slot_real(w, h, mcux, mcu, s)) --s;
  return dc_at(mcu * 6 + s);
}

template <typename DcAt>
ARENA_JHD int predictor(int w, int h, int mcux, int mcu, int s, const DcAt& dc_at) {
  if (s >= 1 && s <= 3) return effective_dc(w, h, mcux, mcu, s - 1, dc_at);
  if (mcu == 0) return 0;
  return effective_dc(w, h, mcux, mcu - 1, s == 0 ? 3 : s, dc_at);
}

// tables of slot s within the four: DC at [0], AC at [kCodeTableEntries]
ARENA_JHD const uint32_t* slot_tables(const uint32_t* tables, int s) {
  return tables + (s >= 4 ? 2 * kCodeTableEntries : 0);
}

ARENA_JHD void dc_symbol(int diff, const uint32_t* dct, uint64_t& code, int& len) {
  int a = diff < 0 ? -diff : diff;
  if (a > 2 * kMaxCoef + 1) a = 2 * kMaxCoef + 1;
  const int nb = bit_length((uint32_t)a);
  const uint32_t e = dct[nb];
  const uint32_t v = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u);
  code = ((uint64_t)(e & 0xFFFF) << nb) | v;
  len = (int)(e >> 16) + nb;
}

// The non-zero coefficient v at zigzag index k (1..63) of a block whose mask of non-zero coefficients is nz (bit j:
// zigzag coefficient j != 0; bit 0 is ignored).  At most 3 ZRL codes (33 bits) + 16 + 10 bits = 59 bits.
ARENA_JHD void ac_symbol(uint64_t nz, int k, int v, const uint32_t* act, uint64_t& code, int& len) {
  const uint64_t below = ((nz & ~1ull) | 1ull) & ((1ull << k) - 1ull);  // bit 0 stands for "no coefficient before"
  const int prev = 63 - __builtin_clzll(below);
  const int run = k - prev - 1;
  int a = v < 0 ? -v : v;
  if (a > kMaxCoef) a = kMaxCoef;
  const int nb = bit_length((uint32_t)a);
  const uint32_t zrl = act[0xF0], e = act[((run & 15) << 4) | nb];
  const int zl = (int)(zrl >> 16);
  code = 0;
  len = 0;
  for (int i = run >> 4; i > 0; --i) {
    code = (code << zl) | (zrl & 0xFFFF);
    len += zl;
  }
  const int el = (int)(e >> 16);
  code = (((code << el) | (e & 0xFFFF)) << nb) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u));
  len += el + nb;
}

ARENA_JHD void eob_symbol(uint64_t nz, const uint32_t* act, uint64_t& code, int& len) {
  const bool none = (nz >> 63) & 1;
  code = none ? 0 : (act[0] & 0xFFFF);
  len = none ? 0 : (int)(act[0] >> 16);
}

// Mask of the non-zero coefficients of a block in zigzag order.
ARENA_JHD uint64_t nonzero_mask(const int16_t* zz) {
  uint64_t nz = 0;
  for (int k = 0; k < 64; ++k) nz |= (uint64_t)(zz[k] != 0) << k;
  return nz;
}

// Bits of one slot: zz / nz of a real slot (zz[0] is not read: the DC enters through diff), nz = 0 for a dummy.
ARENA_JHD int block_bits(const int16_t* zz, uint64_t nz, int diff, const uint32_t* dct, const uint32_t* act) {
  uint64_t code;
  int len, bits;
  dc_symbol(diff, dct, code, bits);
  for (uint64_t m = nz & ~1ull; m; m &= m - 1) {
    const int k = __builtin_ctzll(m);
    ac_symbol(nz, k, zz[k], act, code, len);
    bits += len;
  }
  eob_symbol(nz, act, code, len);
  return bits + len;
}

// OR the low `len` (0..64) bits of `code` into the stream at bit position pos.  or_word(word index, bits) ORs into
// a 32-bit word of a zeroed buffer; it is called for at most 3 words, never with 0.
template <typename OrWord>
ARENA_JHD void put_bits32(uint32_t pos, uint32_t code, int len, const OrWord& or_word) {  // len 1..32
  const int sh = (int)(pos & 31);
  const uint64_t t = ((uint64_t)code << (32 - len)) << (32 - sh);  // left-aligned at bit sh of a 64-bit window
  const uint32_t hi = (uint32_t)(t >> 32), lo = (uint32_t)t;
  if (hi) or_word(pos >> 5, hi);
  if (lo) or_word((pos >> 5) + 1, lo);
}
template <typename OrWord>
ARENA_JHD void put_bits(uint32_t pos, uint64_t code, int len, const OrWord& or_word) {
  if (len > 32) {
    put_bits32(pos, (uint32_t)(code >> 32) & (uint32_t)((1ull << (len - 32)) - 1ull), len - 32, or_word);
    put_bits32(pos + (uint32_t)(len - 32), (uint32_t)code, 32, or_word);
  } else if (len > 0) {
    put_bits32(pos, (uint32_t)code & (uint32_t)((1ull << len) - 1ull), len, or_word);
  }
}

// The 1-bits that pad a scan of total_bits to a whole byte (BitWriter::flush): symbol for put_bits at total_bits.
ARENA_JHD void pad_symbol(uint32_t total_bits, uint64_t& code, int& len) {
  len = (int)((8 - (total_bits & 7)) & 7);
  code = (1u << len) - 1u;
}

// A word of the bit buffer in stream (big-endian) byte order.
ARENA_JHD uint32_t store_be32(uint32_t w) { return __builtin_bswap32(w); }

// Position of unstuffed byte i in the stuffed stream when ff_before of the bytes before it are 0xFF.
ARENA_JHD uint32_t stuffed_at(uint32_t i, uint32_t ff_before) { return i + ff_before; }

// Segments of kStuffSegment unstuffed bytes a crop of `slots` block slots can need.
ARENA_JHD int stuff_segments(int slots) {
  return (int)(((int64_t)slots * kBitBufBytesPerSlot + kStuffSegment - 1) / kStuffSegment);
}

// Status of a crop's result record.
constexpr uint32_t kEntropyOk = 0, kEntropyOverflow = 1;

}  // namespace jpegh
}  // namespace arena
