// enc_aq.h — adaptive quantisation of the device encoder (vts_transcode_ext9;
// transcode.hip: enc_aq and every stage that reads a macroblock's QP;
// DESIGN.md §11 "Adaptive quantisation"), written once as integer arithmetic
// for the kernels and for the CPU harness (tests/native/enc_aq_host.cpp).
//
// The law (the model is x264's aq-mode 1, variance-adaptive with a fixed
// centre).  Per macroblock, over the 256 luma and 2 x 64 chroma samples of the
// encoder's input picture, with S1 the sum and S2 the sum of squares of a
// plane's samples:
//   E   = (S2y - (S1y^2 >> 8)) + (S2u - (S1u^2 >> 6)) + (S2v - (S1v^2 >> 6))
//   L   = log2 of max(E, 1) in Q8: 256 floor(log2 E) plus the mantissa
//         interpolated linearly, ((E - 2^k) << 8) >> k
//   off = clamp(round_half_away(strength_q8 (L - 3693) / 65536), -aq_max, aq_max)
// 3693 = 14.427 x 256 is x264's centre for 8-bit 4:2:0.  A constant macroblock
// (E = 0, L = 0) gives -aq_max at strength_q8 = 256; strength_q8 = 1 gives 0
// everywhere, |L - 3693| being far below 65536 / 2.
// The macroblock is coded at qp_mb = clamp(QP_picture + off, lo, hi).
//
// The running QP (7.4.5): QP_Y,PRED starts at SliceQPY at each slice (a
// macroblock row).  A macroblock sends mb_qp_delta = qp_mb - QP_Y,PRED only if
// it is Intra16x16 or has a non-zero coded_block_pattern, and QP_Y,PRED
// becomes its qp_mb; P_Skip, I_PCM and pattern-0 macroblocks send nothing and
// leave it.  Their QP_Y (what the in-loop filter reads) is the running one;
// I_PCM is qP = 0 for the filter.  With |off| <= 10 two macroblocks of a
// picture differ by at most 20, inside mb_qp_delta's -26 .. 25.
// Nothing here depends on the device, and no HIP header is included.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VTS_AQ_HD __host__ __device__
#else
#define VTS_AQ_HD
#endif

namespace vts {
namespace full {
namespace eaq {

constexpr int kCentreQ8 = 3693;       // 14.427 x 256
constexpr int kMaxDefault = 8;        // aq_max = 0
constexpr int kMaxLimit = 10;         // |mb_qp_delta| <= 20
constexpr int kStrengthMaxQ8 = 768;   // 3.0

// E from the six sums.  S1y <= 65280: its square is below 2^32; E < 2^23.
VTS_AQ_HD inline uint32_t energy(uint32_t s1y, uint32_t s2y, uint32_t s1u, uint32_t s2u, uint32_t s1v, uint32_t s2v) {
  return (s2y - ((s1y * s1y) >> 8)) + (s2u - ((s1u * s1u) >> 6)) + (s2v - ((s1v * s1v) >> 6));
}

// log2(max(E, 1)) in Q8 (E < 2^24, so the shifted mantissa stays in 32 bits)
VTS_AQ_HD inline int log2_q8(uint32_t e) {
  if (e < 2) return 0;
  int k = 0;
  for (uint32_t v = e; v > 1; v >>= 1) ++k;
  return 256 * k + static_cast<int>(((e - (1u << k)) << 8) >> k);
}

VTS_AQ_HD inline int offset_of_energy(uint32_t e, int strength_q8, int aq_max) {
  const int x = strength_q8 * (log2_q8(e) - kCentreQ8);  // |x| < 2^23
  const int r = x < 0 ? -((-x + 32768) >> 16) : (x + 32768) >> 16;
  return r < -aq_max ? -aq_max : (r > aq_max ? aq_max : r);
}

// the QP a macroblock is coded at
VTS_AQ_HD inline int qp_mb(int qp_picture, int off, int lo, int hi) {
  const int q = qp_picture + off;
  return q < lo ? lo : (q > hi ? hi : q);
}

// Whether a macroblock sends mb_qp_delta: Intra16x16 always, I_PCM never,
// everything else (inter, I_NxN; P_Skip has pattern 0) with a pattern
VTS_AQ_HD inline bool sends_delta(bool pcm, bool intra16, int cbp) { return !pcm && (intra16 || cbp != 0); }

// A slice's running QP and what the CABAC ctxIdxInc of mb_qp_delta's first
// bin needs: whether the previous macroblock of the slice sent a non-zero delta
struct RunQp {
  int pred;      // QP_Y,PRED
  bool prev_nz;  // ctxIdxInc of the next mb_qp_delta's bin 0
  VTS_AQ_HD void start(int slice_qp) {
    pred = slice_qp;
    prev_nz = false;
  }
  // The macroblock after the ones so far: its mb_qp_delta (0 when it sends
  // none), the state as the next macroblock finds it.  inc (may be NULL): the
  // ctxIdxInc this macroblock's own first bin is coded with.
  VTS_AQ_HD int step(bool sends, int qp, int *inc = nullptr) {
    if (inc) *inc = prev_nz ? 1 : 0;
    if (!sends) {
      prev_nz = false;
      return 0;
    }
    const int d = qp - pred;
    pred = qp;
    prev_nz = d != 0;
    return d;
  }
  // QP_Y of the macroblock just stepped over, as the in-loop filter reads it
  VTS_AQ_HD int filter_qp(bool pcm) const { return pcm ? 0 : pred; }
};

// bits of se(v)
VTS_AQ_HD inline int se_bits(int v) {
  uint32_t code = static_cast<uint32_t>(v > 0 ? 2 * v - 1 : -2 * v) + 1;
  int n = 0;
  while (code > 1) {
    code >>= 1;
    ++n;
  }
  return 2 * n + 1;
}

}  // namespace eaq
}  // namespace full
}  // namespace vts
