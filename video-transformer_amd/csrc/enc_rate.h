// enc_rate.h — the two rate-aware decisions of the device encoder's motion
// search (transcode.hip: enc_search), written once for the
// kernel and for the CPU harness (tests/native/enc_rate_host.cpp).
//
//   mvcost:     candidates are ordered by (16 SAD + lambda16 bits(v - p), index)
//               instead of (SAD, index); v and p in quarter samples, p the
//               guess of the writer's predictor that exists while a level's
//               macroblocks search in parallel (pred_of_cmd).
//   early_skip: before the search, the residual of the prediction at vector
//               (0, 0) goes through the transform and the quantiser; when no
//               level survives the macroblock is P_Skip (all_zero_*: the
//               quantiser's own answer, enc_residual.h).
//
// Nothing here depends on the device: the kernel and the harness call the
// same functions.
#pragma once
#include <cstdint>

#include "enc_deblock.h"
#include "enc_residual.h"

namespace vts {
namespace full {
namespace erate {

// length of se(v) for the value k (9.1, 9.1.1): codeNum = 2|k| - (k > 0),
// 2 floor(log2(codeNum + 1)) + 1 bits
VTS_HD VTS_INLINE int selen(int k) {
  const uint32_t code = k > 0 ? 2u * static_cast<uint32_t>(k) - 1u : 2u * static_cast<uint32_t>(-k);
  return 2 * (31 - __builtin_clz(code + 1u)) + 1;
}
// bits of mvd_l0 (dx, dy), quarter samples
VTS_HD VTS_INLINE int mv_bits(int dx, int dy) { return selen(dx) + selen(dy); }

// 16 times the SAD-domain Lagrangian of a residual QP:
// int(16 sqrt(0.85 2^((qp - 12) / 3)) + 0.5)
VTS_HD VTS_INLINE int lambda16_of_qp(int qp) {
  static constexpr int16_t kLambda16[52] = {4,   4,   5,   5,   6,   7,   7,   8,   9,   10,  12,  13,   15,
                                            17,  19,  21,  23,  26,  30,  33,  37,  42,  47,  53,  59,   66,
                                            74,  83,  94,  105, 118, 132, 149, 167, 187, 210, 236, 265,  297,
                                            334, 375, 421, 472, 530, 595, 668, 749, 841, 944, 1060, 1189, 1335};
  return kLambda16[qp];
}
// the lambda16 a search runs with: the caller's when > 0, else the table's
VTS_HD VTS_INLINE int lambda16(int qp, int mv_lambda16) { return mv_lambda16 > 0 ? mv_lambda16 : lambda16_of_qp(qp); }

// The cost of candidate vector (vx, vy) with luma SAD sad against the
// predictor (px, py); lam16 = 0 orders as the SAD alone.  At most 16 * 65280
// + 4096 * 2 * 31: 21 bits.
VTS_HD VTS_INLINE uint32_t cost16(uint32_t sad, int lam16, int vx, int vy, int px, int py) {
  return 16u * sad + static_cast<uint32_t>(lam16) * static_cast<uint32_t>(mv_bits(vx - px, vy - py));
}
// The key candidates are compared by: (cost, index), index < 65536 (0 = the
// centre, then raster order); the SAD (< 65536) rides below the index, where
// it cannot change the order, so that the winner's is known after the
// reduction.
VTS_HD VTS_INLINE uint64_t key_of(uint32_t cost, uint32_t index, uint32_t sad) {
  return (static_cast<uint64_t>(cost) << 32) | (index << 16) | sad;
}
VTS_HD VTS_INLINE uint32_t key_index(uint64_t key) { return static_cast<uint32_t>(key >> 16) & 0xffffu; }
VTS_HD VTS_INLINE uint32_t key_sad(uint64_t key) { return static_cast<uint32_t>(key) & 0xffffu; }

struct Mv {
  int x, y;
};
// The predictor guess p of macroblock (mx, .) of the P picture at GOP position
// j >= 1: (0, 0) in column 0 (the writer's own predictor there: 8.4.1.3 with A
// the only neighbour and one slice per row) and at j = 1 (the previous picture
// is the IDR); else from left_prev, the final command word of (mx - 1, my) in
// the picture at GOP position j - 1: its vector, (0, 0) when that macroblock
// was I_PCM or Intra16x16 (a P_Skip word is 0).
VTS_HD VTS_INLINE Mv pred_of_cmd(uint32_t left_prev, int mx, int j) {
  Mv p{0, 0};
  if (mx == 0 || j <= 1 || left_prev == edb::kPcmCmd || edb::is_intra_cmd(left_prev)) return p;
  p.x = static_cast<int16_t>(left_prev & 0xffffu);
  p.y = static_cast<int16_t>(left_prev >> 16);
  return p;
}

// ---- the early P_Skip probe: does any level of a residual survive the
// quantiser?  Not restated here: enc_residual.h's code_block / code_chroma_dc
// asked whether a level is left.
using eres::all_zero_block;
using eres::all_zero_chroma_dc;

}  // namespace erate
}  // namespace full
}  // namespace vts
