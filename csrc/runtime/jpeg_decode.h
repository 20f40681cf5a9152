// Host half of the split JPEG decoder: marker parsing + baseline Huffman entropy decoding into quantized DCT
// coefficient blocks.  The device half (dequantisation, islow IDCT, fancy chroma upsampling, YCbCr->RGB) runs
// as HIP kernels on the batch (csrc/kernels/jpeg_idct.hip), so the host spends only the entropy decode per
// upload; everything after it is a few microseconds of GPU time per image.
//
// The reference decodes every upload entirely on the CPU (cv2.imdecode, src/shared/processing/transforms.py:
// 77-110; PIL for arm B crops, architectures/microservices/classification/app/servicer.py:65-76).  Here the
// work PIL does in one call is cut where the data is smallest and the arithmetic least parallel: the bit
// serial Huffman stream stays on a host thread, the per-pixel math moves to the GPU.
//
// Scope: baseline / extended-sequential Huffman (SOF0, SOF1), 8-bit samples, 1 (grayscale) or 3 components (YCbCr,
// or RGB-coded as libjpeg recognises it) whose chroma factors are equal and divide the luma's (4:4:4, 4:2:2, 4:2:0,
// 4:4:0, 4:1:1, 4:1:0, ...: JpegLayout), one interleaved scan or several scans that code every component exactly
// once, restart intervals; and, when the progressive switch is on (ARENA_JPEG_PROGRESSIVE, default 0, or the
// `progressive` argument of jpeg_parse), progressive Huffman files (SOF2, T.81 Annex G) of the same frame geometry
// whose scans send every coefficient of every component down to bit 0.  Everything else — arithmetic-coded,
// lossless, 12-bit, CMYK / YCCK, a height from DNL, luma below the maximum factor or unequal chroma factors, 4:2:2
// / 4:2:0 chroma narrower than 3 samples, an interleaved MCU of more than 10 blocks, progressive files with the
// switch off, with an incomplete or inconsistent progression, more than kJpegMaxScans scans or a DQT between scans
// — is reported as Unsupported and the caller sends the upload to the PIL fallback (server/decode_pool.py).  For a
// file whose scans are walked (progressive, or sequential in several scans) Unsupported can also come from the
// decode functions, after jpeg_parse said Ok, and for every file when its coefficients are beyond the range in which
// libjpeg's 16-bit IDCT is exact: some block with sum |c_k| * q_k > kCoefRangeLimit (kernels/jpeg_math.h), where PIL's
// SIMD decode, exact arithmetic and the kernels' int32 arithmetic are no longer proved to agree.  Photographs stay
// well within it; blocks of full-swing noise or dither in luma (0 / 255 in all three channels) reach S of about 7000
// at any quality and are handed back although they come from pixels (and although PIL and the kernels' arithmetic
// still agree on such dense blocks: the criterion is sufficient, not necessary); a crafted file can carry anything.
// Callers route either to the same fallback.  The same reconstruction arithmetic is available on the host (jpeg_coefs_to_rgb) as the
// bit-exact reference of the kernels and as a host-only decode.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../kernels/jpeg_desc.h"

namespace arena {

struct JpegHuffSpec {
  bool present = false;
  uint8_t bits[17] = {};   // codes per length 1..16
  uint8_t vals[256] = {};  // symbols in code order
};

struct JpegInfo {
  int width = 0, height = 0, ncomp = 0;
  int hmax = 1, vmax = 1, mcux = 0, mcuy = 0;
  int layout = -1;
  // luma : chroma sampling ratio (1..4 each; 1 for grey), and whether the components are R, G, B (no YCbCr step)
  int rh = 1, rv = 1;
  bool rgb_coded = false;
  // EXIF orientation (1..8; 1 when absent or not well-formed, see jpeg_parse) and the size of the oriented
  // output: width and height swapped for 5..8.  width / height stay the stored frame's.
  int orientation = 1;
  int out_width = 0, out_height = 0;
  int restart_interval = 0;
  int comp_id[kJpegMaxComp] = {};
  int tq[kJpegMaxComp] = {}, td[kJpegMaxComp] = {}, ta[kJpegMaxComp] = {};
  JpegCompDesc comp[kJpegMaxComp] = {};  // coef_off: element (int16) offsets into the coefficient buffer
  uint16_t qt[kJpegMaxComp][64] = {};    // per component, natural order
  int64_t coef_count = 0;                // int16 coefficients of all components
  int64_t plane_bytes = 0;               // reconstructed sample planes of all components
  size_t scan_begin = 0;                 // first byte of the entropy-coded segment
  // SOF2: the decode functions walk the scans themselves from `first_sos` (the length field of the first SOS
  // segment; DHT, DRI and further SOS follow between scans).  restart_interval and dc / ac are the state there.
  bool progressive = false;
  size_t first_sos = 0;
  // SOF0/1 whose first scan is not all components in frame order: walked from `first_sos` in the same way, every
  // scan a full-block one
  bool multiscan = false;
  // compact payload (jpeg_decode_compact): its bytes and the byte offsets of its three arrays; -1 = dense int16
  int64_t compact_bytes = -1;
  int64_t cmask_off = 0, cvoff_off = 0, cval_off = 0;
  JpegHuffSpec dc[4], ac[4];
};

enum class JpegStatus : int { Ok = 0, Unsupported = 1, Corrupt = 2 };

// A progressive file with more scans is handed back (each scan is a pass over the image: the decode-bomb guard;
// PIL writes 10 scans for colour and 6 for grey, optimiser scripts stay below 16).
constexpr int kJpegMaxScans = 32;

// ARENA_JPEG_PROGRESSIVE (default 0), read once: the process default of jpeg_parse's `progressive`.  The setter
// replaces it (for a process that decides after start-up) and returns the previous value.
bool jpeg_progressive_enabled();
bool jpeg_set_progressive_enabled(bool on);

// Parse the markers up to the first scan.  `max_pixels` > 0 rejects larger frames as Corrupt with an
// "image too large" message (the decode-bomb guard of processing/transforms.py).  `progressive`: 1 accepts SOF2
// under the frame checks of SOF0/1, 0 reports it as Unsupported, -1 follows jpeg_progressive_enabled().
//
// Orientation, as cv2.imdecode honours it (processing/exif.py is the same rule in Python, for the PIL paths): the
// first APP1 segment before SOS whose payload starts with "Exif\0\0" decides.  Its TIFF header ("II" or "MM", 42,
// IFD0 offset) leads to IFD0; the first entry with tag 0x0112 counts when it is one SHORT with a value of 1..8.
// Everything else is orientation 1: no such segment, another type or count, a value of 0 or 9, an IFD or entry
// table that leaves the segment, an orientation that only XMP states.  Broken EXIF never changes the status.
JpegStatus jpeg_parse(const uint8_t* data, size_t n, JpegInfo& info, std::string& err, int64_t max_pixels = 0,
                      int progressive = -1);

// Entropy-decode the scan: info.coef_count int16 quantized coefficients, natural order, one block after the
// other (component c's block (by, bx) at comp[c].coef_off + (by * bw + bx) * 64).  A scan cut short by a
// marker is padded with zero bits (libjpeg's warning, which PIL ignores); a file that simply ends inside the
// scan is Corrupt ("image file is truncated", as PIL raises), like structurally broken streams.  A sound scan with a
// block beyond the coefficient range (above) is Unsupported, in every kind of file: single-scan files say so after the
// scan (a damaged one stays Corrupt), sequential multi-scan files at the block, progressive files after the last scan.
//
// A progressive file (info.progressive) is decoded scan by scan into the same dense layout: DC scans interleaved
// or not, single-component AC scans, first and refinement passes, EOB runs, restart intervals, and tables or a
// restart interval redefined between scans.  A single-component scan of a 3-component frame covers the
// component's real ceil(cw / 8) x ceil(ch / 8) blocks; the MCU padding of the grid keeps zero AC and the DC of the
// interleaved DC scans.  The result is Ok only when it is what libjpeg computes without a warning; Unsupported
// (hand the upload to PIL) when a scan header breaks G.1.1.1.1, the progression of some coefficient is
// inconsistent (refinement before the first scan, a first scan twice, Ah not the previous Al, AC before DC) or at
// EOI incomplete (libjpeg would smooth), there are more than kJpegMaxScans scans, a DQT or anything but DHT, DRI,
// APPn and COM lies between scans, a value leaves int16, or the entropy-coded data is damaged where libjpeg warns:
// a code that matches nothing, a refinement symbol of another magnitude than 1, a segment that a marker cuts short
// or that leaves bytes over, a restart marker that is missing or not the expected RSTn.  (Baseline scans keep
// their zero-bit padding of a segment cut short.)
//
// A sequential file in several scans (info.multiscan) goes through the same walker with full-block scans (Ss 0,
// Se 63, Ah = Al = 0; anything else is handed back) and the same strictness about damaged data.  libjpeg does not
// smooth such a file; it outputs whatever it has, so the result is Ok only when every component was coded by exactly
// one scan: a component coded twice or never is Unsupported.
JpegStatus jpeg_decode_coefs(const uint8_t* data, size_t n, const JpegInfo& info, int16_t* coef, std::string& err);

// The same scan into the compact payload the split decoder ships (3-4x fewer bytes than the dense blocks at q90:
// most AC coefficients are zero).  Per 8x8 block, in the dense layout's block order (component 0's blocks row by
// row, then 1, 2): a uint64 mask (bit k: the coefficient at zigzag index k is coded), then per block the uint32
// index of its first value, then the int16 values of every block in zigzag order (16-byte aligned array).  `out`
// holds jpeg_compact_capacity(info) bytes; on success info.compact_bytes / cmask_off / cvoff_off / cval_off
// describe what was written.  Status and error messages as jpeg_decode_coefs.  A file whose scans are walked
// (progressive or multi-scan sequential) is decoded into dense blocks in a thread-local scratch (released after use when above 16 MB) and packed after its last scan.
JpegStatus jpeg_decode_compact(const uint8_t* data, size_t n, JpegInfo& info, uint8_t* out, std::string& err);
int64_t jpeg_total_blocks(const JpegInfo& info);
int64_t jpeg_compact_capacity(const JpegInfo& info);
// bytes of the decoded payload (compact, or dense int16)
int64_t jpeg_payload_bytes(const JpegInfo& info);
// ARENA_JPEG_COMPACT (default 1): the serving paths decode into the compact payload; 0 keeps dense blocks
bool jpeg_compact_enabled();
// compact payload -> dense int16 blocks (host reference paths)
void jpeg_compact_to_dense(const JpegInfo& info, const uint8_t* payload, int16_t* coef);
// the payload as dense blocks: itself when dense, else expanded into `scratch`
const int16_t* jpeg_dense_coefs(const JpegInfo& info, const uint8_t* payload, std::vector<int16_t>& scratch);

// Host reconstruction with the device kernels' exact arithmetic (kernels/jpeg_math.h): packed RGB of
// out_height x out_width pixels, each source pixel placed by info.orientation (table in kernels/jpeg_idct.hip).
void jpeg_coefs_to_rgb(const JpegInfo& info, const int16_t* coef, uint8_t* rgb);

// The device descriptor of a parsed image, with byte offsets relative to `coef_base` / `plane_base` / `rgb_off`.
JpegDesc jpeg_device_desc(const JpegInfo& info, int64_t coef_base, int64_t plane_base, int64_t rgb_off);

}  // namespace arena
