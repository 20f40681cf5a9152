// Device entropy coder of the JPEG crop encoder: the Huffman-coded, byte-stuffed scan of every crop, from the
// coefficient blocks jpeg_fdct_kernel leaves (csrc/kernels/jpeg_fdct.hip), byte for byte what the host writer
// jpeg_write (csrc/runtime/jpeg_encode.cpp) makes of them.  The arithmetic is kernels/jpeg_huff_math.h, which the
// host runs through the same phases (jpeg_entropy_phased_host).
//
// An encoder has no serial dependency a decoder has: a slot's code depends on its 64 coefficients and on the DC of
// one earlier slot, which is a coefficient in memory; where the code goes is a prefix sum of code lengths; byte
// stuffing is a second prefix sum.  Five launches on one stream, none of which waits for another workgroup:
//
//   jpeg_huff_size_kernel   grid (slot groups, crops).  32 slots per 256-lane workgroup, eight lanes per slot.  A lane
//                           loads 16 bytes of its block (the layout the FDCT kernel writes), the block is staged in
//                           LDS in zigzag order, a lane then owns zigzag coefficients 8l..8l+7: the non-zero mask is
//                           the OR of eight partial masks (three xor-shuffles), the slot's bits the sum of eight
//                           partial sums.  Writes one uint32 per slot.
//   jpeg_huff_scan_kernel   grid (crops).  One workgroup turns a crop's sizes into exclusive bit offsets in place and
//                           writes the total into the result record.
//   jpeg_huff_emit_kernel   the size kernel's grid and staging.  Lanes OR their symbols into an LDS image of the
//                           workgroup's bit range (LDS atomics), which then goes to the zeroed bit buffer with plain
//                           word stores; the first and the last word, which a neighbour workgroup may share, with one
//                           global atomic OR each.  The workgroup that holds the crop's last slot adds the 1-bits
//                           that pad the last byte.
//   jpeg_huff_count_kernel  grid (segments, crops).  0xFF bytes per segment of kStuffSegment unstuffed bytes.
//   jpeg_huff_stuff_kernel  the same grid.  Every workgroup sums its crop's segment counts (a few hundred at most):
//                           the stuffed length, hence ok / overflow, is known before anything is written.  The first
//                           segment's workgroup writes the result record.  If the scan fits the reserve, every lane
//                           places its 16 bytes (and the 0x00 after each 0xFF) at their final positions: one writer
//                           per byte.  On overflow nothing is written and the host codes the crop itself.
//
// Bounds: the symbol functions clamp magnitudes to the domain (|coefficient| <= 1023), so a slot never exceeds
// jpegh::kMaxBlockBits whatever the input holds; the bit buffer has kBitBufBytesPerSlot (256) bytes per slot, the LDS
// image room for 32 such slots.  Writes to the scan buffer stay below the stuffed length, which is at most the
// reserve.
#include <hip/hip_runtime.h>

#include "jpeg_enc_desc.h"
#include "jpeg_huff_math.h"
#include "launch.h"

namespace arena {

namespace {

constexpr int kSlotsPerGroup = 32;
// LDS image of one workgroup's bits: 32 slots, up to 31 bits of misalignment in front, 7 pad bits behind
constexpr int kGroupWords = (kSlotsPerGroup * jpegh::kMaxBlockBits + 31 + 7 + 31) / 32 + 1;
constexpr int kTableWords = 4 * jpegh::kCodeTableEntries;

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
  return ((uint64_t)hi << 32) | lo;
}

// Inclusive prefix sum of v over the 256 lanes of the workgroup; `total` is the workgroup's sum.  scratch: 4 words.
__device__ __forceinline__ uint32_t group_scan(uint32_t v, uint32_t* scratch, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, d);
    if (lane >= d) v += u;
  }
  __syncthreads();  // scratch may still be read from the previous call
  if (lane == 63) scratch[wave] = v;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t t = scratch[k];
    if (k < wave) before += t;
    total += t;
  }
  return v + before;
}

// What the size and the emit kernel share: one slot per eight lanes.
struct Slot {
  uint64_t code[8];  // lane l: the symbols of zigzag coefficients 8l .. 8l + 7 (len 0: nothing)
  int len[8];
  uint64_t head;  // lane 0: the DC symbol; lane 7: the end-of-block symbol, emitted after code[]
  int head_len;
  uint32_t before;  // bits of the slot's lower lanes
  uint32_t bits;    // bits of the whole slot
};

// zz: the workgroup's [32][64] staging area, tb: the code tables in LDS.  Contains barriers: all 256 lanes call it.
__device__ __forceinline__ Slot code_slot(const JpegEntDesc& d, const uint8_t* __restrict__ coef, int blk, bool live,
                                          bool natural, int16_t (*zz)[64], const uint32_t* tb) {
  const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
  const uint8_t* base = coef + d.coef_off;
  if (live) {
    const uint4 q = *reinterpret_cast<const uint4*>(base + (int64_t)blk * 128 + l * 16);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int idx = l * 8 + j;
      zz[g][natural ? jpegh::kZigzagOf[idx] : idx] = (int16_t)(uint16_t)(w[j >> 1] >> ((j & 1) * 16));
    }
  }
  __syncthreads();
  const int mcu = blk / kJpegEncBlocksPerMcu, s = blk - mcu * kJpegEncBlocksPerMcu;
  const bool real = live && jpegh::slot_real(d.w, d.h, d.mcux, mcu, s);
  int v[8];
  {
    const uint4 q = *reinterpret_cast<const uint4*>(&zz[g][l * 8]);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = real ? (int)(int16_t)(uint16_t)(w[j >> 1] >> ((j & 1) * 16)) : 0;
  }
  uint64_t nz = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) nz |= (uint64_t)(v[j] != 0) << (l * 8 + j);
  nz |= shfl_xor64(nz, 1);
  nz |= shfl_xor64(nz, 2);
  nz |= shfl_xor64(nz, 4);
  const uint32_t* dct = jpegh::slot_tables(tb, s);
  const uint32_t* act = dct + jpegh::kCodeTableEntries;
  Slot o;
  uint32_t mine = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = l * 8 + j;
    o.code[j] = 0;
    o.len[j] = 0;
    if (k > 0 && v[j] != 0) jpegh::ac_symbol(nz, k, v[j], act, o.code[j], o.len[j]);
    mine += (uint32_t)o.len[j];
  }
  o.head = 0;
  o.head_len = 0;
  if (live && l == 0) {
    const auto dc_at = [&](int slot) { return (int)*reinterpret_cast<const int16_t*>(base + (int64_t)slot * 128); };
    const int diff = jpegh::effective_dc(d.w, d.h, d.mcux, mcu, s, dc_at) - jpegh::predictor(d.w, d.h, d.mcux, mcu, s, dc_at);
    jpegh::dc_symbol(diff, dct, o.head, o.head_len);
  }
  if (live && l == 7) jpegh::eob_symbol(nz, act, o.head, o.head_len);
  mine += (uint32_t)o.head_len;
  uint32_t incl = mine;
#pragma unroll
  for (int dlt = 1; dlt < 8; dlt <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)incl, dlt, 8);
    if (l >= dlt) incl += u;
  }
  o.before = incl - mine;
  o.bits = (uint32_t)__shfl((int)incl, 7, 8);
  return o;
}

__device__ __forceinline__ void load_tables(const uint32_t* __restrict__ tables, uint32_t* tb) {
  for (int i = threadIdx.x; i < kTableWords; i += 256) tb[i] = tables[i];
}

__global__ __launch_bounds__(256) void jpeg_huff_size_kernel(const JpegEntDesc* __restrict__ descs,
                                                             const uint8_t* __restrict__ coef,
                                                             const uint32_t* __restrict__ tables,
                                                             uint32_t* __restrict__ slot_bits, int natural) {
  __shared__ __attribute__((aligned(16))) int16_t zz[kSlotsPerGroup][64];
  __shared__ uint32_t tb[kTableWords];
  const JpegEntDesc d = descs[blockIdx.y];
  if ((int)blockIdx.x * kSlotsPerGroup >= d.total_blocks) return;  // the whole workgroup
  load_tables(tables, tb);
  const int blk = (int)blockIdx.x * kSlotsPerGroup + (threadIdx.x >> 3);
  const bool live = blk < d.total_blocks;
  const Slot o = code_slot(d, coef, blk, live, natural != 0, zz, tb);
  if (live && (threadIdx.x & 7) == 7) slot_bits[d.slot_base + blk] = o.bits;
}

__global__ __launch_bounds__(256) void jpeg_huff_scan_kernel(const JpegEntDesc* __restrict__ descs,
                                                             uint32_t* __restrict__ slot_bits,
                                                             JpegEntResult* __restrict__ res) {
  __shared__ uint32_t scratch[4];
  const JpegEntDesc d = descs[blockIdx.x];
  uint32_t* p = slot_bits + d.slot_base;
  uint32_t carry = 0;
  for (int first = 0; first < d.total_blocks; first += 256) {
    const int i = first + (int)threadIdx.x;
    const uint32_t v = i < d.total_blocks ? p[i] : 0u;
    uint32_t total;
    const uint32_t incl = group_scan(v, scratch, total);
    if (i < d.total_blocks) p[i] = carry + incl - v;
    carry += total;
  }
  if (threadIdx.x == 0) {
    res[blockIdx.x].total_bits = carry;
    res[blockIdx.x].raw_bytes = (carry + 7) / 8;
  }
}

__global__ __launch_bounds__(256) void jpeg_huff_emit_kernel(const JpegEntDesc* __restrict__ descs,
                                                             const uint8_t* __restrict__ coef,
                                                             const uint32_t* __restrict__ tables,
                                                             const uint32_t* __restrict__ slot_bits,
                                                             const JpegEntResult* __restrict__ res,
                                                             uint8_t* __restrict__ bitbuf, int natural) {
  __shared__ __attribute__((aligned(16))) int16_t zz[kSlotsPerGroup][64];
  __shared__ uint32_t tb[kTableWords];
  __shared__ uint32_t img[kGroupWords];
  __shared__ uint32_t s_end;
  const JpegEntDesc d = descs[blockIdx.y];
  const int first = (int)blockIdx.x * kSlotsPerGroup;
  if (first >= d.total_blocks) return;  // the whole workgroup
  load_tables(tables, tb);
  for (int i = threadIdx.x; i < kGroupWords; i += 256) img[i] = 0;
  const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
  const int blk = first + g;
  const bool live = blk < d.total_blocks;
  const Slot o = code_slot(d, coef, blk, live, natural != 0, zz, tb);  // its barrier also covers img and tb
  const uint32_t base_word = slot_bits[d.slot_base + first] >> 5;
  const bool last = blk == d.total_blocks - 1;
  if (live) {
    const uint32_t at = slot_bits[d.slot_base + blk] - base_word * 32;
    const auto or_word = [&](uint32_t i, uint32_t v) {
      if (i < (uint32_t)kGroupWords) atomicOr(&img[i], v);
    };
    uint32_t pos = at + o.before;
    if (l == 0) {
      jpegh::put_bits(pos, o.head, o.head_len, or_word);
      pos += (uint32_t)o.head_len;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      jpegh::put_bits(pos, o.code[j], o.len[j], or_word);
      pos += (uint32_t)o.len[j];
    }
    if (l == 7) {
      jpegh::put_bits(pos, o.head, o.head_len, or_word);
      pos += (uint32_t)o.head_len;  // = at + o.bits
      if (last) {                   // the crop's last slot: pad to a whole byte with 1-bits
        uint64_t code;
        int len;
        jpegh::pad_symbol(res[blockIdx.y].total_bits, code, len);
        jpegh::put_bits(pos, code, len, or_word);
        pos += (uint32_t)len;
      }
      if (last || g == kSlotsPerGroup - 1) s_end = pos;
    }
  }
  __syncthreads();
  const uint32_t nwords = min((s_end + 31) >> 5, (uint32_t)kGroupWords);
  uint32_t* dst = reinterpret_cast<uint32_t*>(bitbuf + (int64_t)d.slot_base * jpegh::kBitBufBytesPerSlot) + base_word;
  for (uint32_t i = threadIdx.x; i < nwords; i += 256) {
    const uint32_t v = jpegh::store_be32(img[i]);
    if (i == 0 || i == nwords - 1) {
      if (v) atomicOr(&dst[i], v);  // a neighbour workgroup's bits may share this word; the buffer was zeroed
    } else {
      dst[i] = v;
    }
  }
}

// 16 unstuffed bytes of a lane and how many of them, among the first `n`, are 0xFF
__device__ __forceinline__ uint32_t count_ff(const uint4& q, int n, uint8_t b[16]) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    b[j] = (uint8_t)(w[j >> 2] >> ((j & 3) * 8));
    c += (j < n && b[j] == 0xFF) ? 1u : 0u;
  }
  return c;
}

__global__ __launch_bounds__(256) void jpeg_huff_count_kernel(const JpegEntDesc* __restrict__ descs,
                                                              const JpegEntResult* __restrict__ res,
                                                              const uint8_t* __restrict__ bitbuf,
                                                              uint32_t* __restrict__ seg_ff) {
  __shared__ uint32_t scratch[4];
  const JpegEntDesc d = descs[blockIdx.y];
  const uint32_t nbytes = res[blockIdx.y].raw_bytes;
  const uint32_t start = blockIdx.x * (uint32_t)jpegh::kStuffSegment;
  if (start >= nbytes) return;  // the whole workgroup
  const uint32_t at = start + threadIdx.x * 16;
  uint32_t c = 0;
  if (at < nbytes) {
    const uint8_t* src = bitbuf + (int64_t)d.slot_base * jpegh::kBitBufBytesPerSlot;
    uint8_t b[16];
    c = count_ff(*reinterpret_cast<const uint4*>(src + at), (int)min(16u, nbytes - at), b);
  }
  uint32_t total;
  (void)group_scan(c, scratch, total);
  if (threadIdx.x == 0) seg_ff[d.seg_base + (int)blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void jpeg_huff_stuff_kernel(const JpegEntDesc* __restrict__ descs,
                                                              JpegEntResult* __restrict__ res,
                                                              const uint8_t* __restrict__ bitbuf,
                                                              const uint32_t* __restrict__ seg_ff,
                                                              uint8_t* __restrict__ out) {
  __shared__ uint32_t scratch[4];
  const JpegEntDesc d = descs[blockIdx.y];
  const uint32_t nbytes = res[blockIdx.y].raw_bytes;
  const uint32_t seg = blockIdx.x, start = seg * (uint32_t)jpegh::kStuffSegment;
  if (start >= nbytes) return;  // the whole workgroup
  // 0xFF bytes of the whole crop and of the segments before this one
  const uint32_t nseg = (nbytes + jpegh::kStuffSegment - 1) / jpegh::kStuffSegment;
  uint32_t all = 0, before = 0;
  for (uint32_t i = threadIdx.x; i < nseg; i += 256) {
    const uint32_t c = seg_ff[d.seg_base + (int)i];
    all += c;
    before += i < seg ? c : 0u;
  }
  uint32_t all_total, before_total;
  (void)group_scan(all, scratch, all_total);
  (void)group_scan(before, scratch, before_total);
  const uint32_t stuffed = nbytes + all_total;
  const bool fits = stuffed <= (uint32_t)d.reserve;
  if (seg == 0 && threadIdx.x == 0) {
    res[blockIdx.y].scan_bytes = stuffed;
    res[blockIdx.y].status = fits ? jpegh::kEntropyOk : jpegh::kEntropyOverflow;
  }
  if (!fits) return;  // the whole workgroup: nothing of this crop is written, the host codes it
  const uint32_t at = start + threadIdx.x * 16;
  uint8_t b[16];
  uint32_t c = 0;
  int n = 0;
  if (at < nbytes) {
    const uint8_t* src = bitbuf + (int64_t)d.slot_base * jpegh::kBitBufBytesPerSlot;
    n = (int)min(16u, nbytes - at);
    c = count_ff(*reinterpret_cast<const uint4*>(src + at), n, b);
  }
  uint32_t total;
  uint32_t ff = before_total + group_scan(c, scratch, total) - c;  // 0xFF bytes before this lane's first byte
  uint8_t* dst = out + d.out_off;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < n) {
      const uint32_t p = jpegh::stuffed_at(at + (uint32_t)j, ff);
      if (p < stuffed) dst[p] = b[j];
      if (b[j] == 0xFF) {
        if (p + 1 < stuffed) dst[p + 1] = 0;
        ++ff;
      }
    }
  }
}

}  // namespace

void jpeg_entropy(const JpegEntDesc* d_descs, const JpegEntBuffers& b, int n_crops, int max_blocks, bool natural,
                  hipStream_t s) {
  if (n_crops <= 0 || max_blocks <= 0) return;
  const dim3 slots((unsigned)((max_blocks + kSlotsPerGroup - 1) / kSlotsPerGroup), (unsigned)n_crops);
  const dim3 segs((unsigned)jpegh::stuff_segments(max_blocks), (unsigned)n_crops);
  hipLaunchKernelGGL(jpeg_huff_size_kernel, slots, dim3(256), 0, s, d_descs, b.coef, b.tables, b.slot_bits, (int)natural);
  hipLaunchKernelGGL(jpeg_huff_scan_kernel, dim3((unsigned)n_crops), dim3(256), 0, s, d_descs, b.slot_bits, b.res);
  hipLaunchKernelGGL(jpeg_huff_emit_kernel, slots, dim3(256), 0, s, d_descs, b.coef, b.tables,
                     (const uint32_t*)b.slot_bits, (const JpegEntResult*)b.res, b.bitbuf, (int)natural);
  hipLaunchKernelGGL(jpeg_huff_count_kernel, segs, dim3(256), 0, s, d_descs, (const JpegEntResult*)b.res,
                     (const uint8_t*)b.bitbuf, b.seg_ff);
  hipLaunchKernelGGL(jpeg_huff_stuff_kernel, segs, dim3(256), 0, s, d_descs, b.res, (const uint8_t*)b.bitbuf,
                     (const uint32_t*)b.seg_ff, b.out);
}

}  // namespace arena
