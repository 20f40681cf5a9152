// Detect-head tile gate: which program ops it pairs, and its threshold.  Plain C++ (no HIP), shared by the
// executor, the bindings and the tests.
//
// decode_kernel (kernels/detect.hip) reduces an anchor's 80 class logits to its best sigmoid, returns when that is
// below conf_thr, and only then reads the anchor's 64 box (DFL) logits.  In a program that ends in DECODE the box
// logits of an anchor that fails the class test are therefore read by nothing, and the fp32 conv that produces them
// (3x3 64 -> 64 with the 1x1 -> 64 in its epilogue, halo_x3g.hip) can skip every tile without a passing class
// logit (ConvParams.gate).  The executor runs the class conv of the level first and hands its output to the box
// conv as the gate.  Box logits of skipped tiles in det*.out are stale by design.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace arena {

// The channel split decode_kernel hard-codes: per anchor 64 box logits (4 sides x 16 DFL bins), then 80 classes.
constexpr int kHeadBoxChannels = 64;
constexpr int kHeadClsChannels = 80;

// gate_min = logit(conf_thr) - kHeadGateMargin, for kHeadGateThrMin <= conf_thr <= kHeadGateThrMax (as floats).
//
// Decode keeps an anchor when max_c fl(1 / (1 + expf(-v_c))) >= conf_thr.  The gate must keep every tile that holds
// such an anchor, without relying on the device expf being monotonic, so it tests v >= gate_min with a margin below
// the exact logit(conf_thr) instead of the predicate itself.  With s(v) the true sigmoid, s'(v) = s (1 - s).  For
// v in [logit(thr) - 1/64, logit(thr)] and thr in [1e-3, 0.999], s(v) lies in [thr e^(-1/64) , thr] when thr is
// small and 1 - s(v) in [1 - thr, (1 - thr) e^(1/64)] when it is large, so s (1 - s) >= 0.98 * 1e-3 * 0.999 there
// and s(logit(thr) - 1/64) <= thr - 1.5e-5.  s is increasing, so every v < gate_min has a true sigmoid at least
// 1.5e-5 below thr, while the computed one (a correctly rounded expf, one add, one divide: a few ulp of a value
// <= 1) is within about 1e-7 of it: it cannot reach thr.  Rounding gate_min to float moves it by < 1e-6 at
// |logit| <= 6.91, far inside the margin; it is rounded downwards all the same.  NaN logits fail both tests.
constexpr double kHeadGateMargin = 1.0 / 64.0;
constexpr float kHeadGateThrMin = 1e-3f;
constexpr float kHeadGateThrMax = 0.999f;

// false: the gate is off for this threshold
inline bool head_gate_min(float conf_thr, float* gate_min) {
  if (!(conf_thr >= kHeadGateThrMin && conf_thr <= kHeadGateThrMax)) return false;
  const double t = (double)conf_thr;
  const double g = std::log(t / (1.0 - t)) - kHeadGateMargin;
  float f = (float)g;
  if ((double)f > g) f = std::nextafterf(f, -INFINITY);
  *gate_min = f;
  return true;
}

// Op record fields read here (engine/planner.py; executor.cpp checks the op codes against its enum)
constexpr int64_t kHgOpConv = 1, kHgOpDecode = 6;
constexpr int kHgDtypeField = 47;

struct HeadGatePair {
  int box;         // op index of the gated conv: fused 1x1 output = channels [0, 64) of the level
  int cls;         // box + 1: the conv that writes the level's class logits, channels [64, 144)
  int level;       // level of the DECODE record
  float conf_thr;  // of the DECODE record
};

// The pairs of a program of n records of `fields` int64 each.  For every level (buf, coff, cs, hw) of the program's
// DECODE record: an fp32 CONV i whose fused pointwise output is 64 channels at (buf, coff) with pixel stride cs on
// an hw x hw map, directly followed by an fp32 CONV over the same map whose output (pointwise or plain) is the 80
// channels at (buf, coff + 64), the two reading disjoint channel ranges of their input and neither reading buf.
// Programs without DECODE (raw detector output, classifier only), the unfused head, levels whose head is not
// fused, and bf16 programs have none.
inline std::vector<HeadGatePair> head_gate_pairs(const int64_t* ops, int n, int fields) {
  std::vector<HeadGatePair> out;
  if (ops == nullptr || fields <= kHgDtypeField) return out;
  auto rec = [&](int i) { return ops + (size_t)i * fields; };
  for (int d = 0; d < n; ++d) {
    const int64_t* dr = rec(d);
    if (dr[0] != kHgOpDecode || dr[kHgDtypeField] != 1) continue;
    uint32_t bits = (uint32_t)dr[18];
    float thr;
    std::memcpy(&thr, &bits, 4);
    for (int l = 0; l < 3; ++l) {
      const int64_t buf = dr[1 + 4 * l], coff = dr[2 + 4 * l], cs = dr[3 + 4 * l], hw = dr[4 + 4 * l];
      if (buf < 0) continue;
      for (int i = 0; i + 1 < d; ++i) {
        const int64_t* a = rec(i);
        const int64_t* c = rec(i + 1);
        if (a[0] != kHgOpConv || a[kHgDtypeField] != 1 || c[0] != kHgOpConv || c[kHgDtypeField] != 1) continue;
        // box conv: fused pointwise output (r[34] channels at (r[36], r[37]), stride r[38])
        if (!(a[34] == kHeadBoxChannels && a[36] == buf && a[37] == coff && a[38] == cs && a[13] == hw && a[14] == hw))
          continue;
        // class conv: pointwise output, or plain output (r[15] channels at (r[10], r[11]), stride r[12])
        const bool c_pw = c[34] > 0;
        const int64_t cb = c_pw ? c[36] : c[10], cc = c_pw ? c[37] : c[11], cst = c_pw ? c[38] : c[12];
        const int64_t cn = c_pw ? c[34] : c[15];
        if (!(cn == kHeadClsChannels && cb == buf && cc == coff + kHeadBoxChannels && cst == cs && c[13] == hw &&
              c[14] == hw && c[30] == a[30]))
          continue;
        // independent: disjoint input channel ranges ([r[2], r[2] + r[6]) of buffer r[1]), neither reads the output
        // buffer, no residual input
        const bool disjoint = a[1] != c[1] || a[2] + a[6] <= c[2] || c[2] + c[6] <= a[2];
        if (!disjoint || a[1] == buf || c[1] == buf || a[22] >= 0 || c[22] >= 0) continue;
        out.push_back(HeadGatePair{i, i + 1, l, thr});
        break;
      }
    }
  }
  return out;
}

// The first head conv F of a pair, or -1: the op directly before the box conv, an fp32 3x3 stride-1 CONV with
// kHeadBoxChannels + kHeadClsChannels output channels over the pair's map, without pointwise epilogue, residual or
// second output, whose output range is exactly the box conv's input channels followed by the class conv's, and
// which nothing but the pair reads (every op's input buffers: r[1] and the residual r[22] of a CONV, the three head
// levels of DECODE / raw output, r[1] of every other op).  The box half of such a conv is read only by the box conv
// (head_marks.h), so the executor may run F as two channel windows around the class conv, all three inside the
// program slots F .. cls: the lifetimes the arena layout was made for still hold.
constexpr int64_t kHgOpYoloRaw = 13;
inline int head_gate_first_conv(const int64_t* ops, int n, int fields, const HeadGatePair& gp) {
  if (ops == nullptr || fields <= kHgDtypeField || gp.box < 1 || gp.cls != gp.box + 1 || gp.cls >= n) return -1;
  auto rec = [&](int i) { return ops + (size_t)i * fields; };
  const int fi = gp.box - 1;
  const int64_t *f = rec(fi), *a = rec(gp.box), *c = rec(gp.cls);
  constexpr int kN = kHeadBoxChannels + kHeadClsChannels;
  if (!(f[0] == kHgOpConv && f[kHgDtypeField] == 1 && f[17] == 3 && f[18] == 3 && f[19] == 1 && f[15] == kN &&
        f[34] == 0 && f[22] < 0 && f[25] < 0 && f[10] >= 0))
    return -1;
  if (!(f[13] == a[4] && f[14] == a[5] && f[13] == a[13] && f[14] == a[14] && f[30] == a[30])) return -1;
  if (!(a[1] == f[10] && a[2] == f[11] && a[6] == kHeadBoxChannels && a[3] == f[12])) return -1;
  if (!(c[1] == f[10] && c[2] == f[11] + kHeadBoxChannels && c[6] == kHeadClsChannels && c[3] == f[12])) return -1;
  const int64_t buf = f[10];
  for (int i = 0; i < n; ++i) {
    if (i == fi || i == gp.box || i == gp.cls) continue;
    const int64_t* r = rec(i);
    bool reads = r[1] == buf;
    if (r[0] == kHgOpConv) reads |= r[22] == buf;
    if (r[0] == kHgOpDecode || r[0] == kHgOpYoloRaw) reads |= r[5] == buf || r[9] == buf;
    if (reads) return -1;
  }
  return fi;
}

}  // namespace arena
