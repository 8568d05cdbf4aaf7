// enc_part.h — the rules of the device encoder's inter partitions
// (vts_transcode_ext6.partitions; transcode.hip: enc_search<.., PT = true>,
// enc_write; DESIGN.md §11 "Partitions"), written once for the kernels and
// for the CPU harness (tests/native/enc_part_host.cpp).
//
// A macroblock's motion is four quadrant vectors (8x8, raster order: 0
// top-left, 1 top-right, 2 bottom-left, 3 bottom-right).  It is searched as
// nine blocks, each a union of quadrants: the whole macroblock, two 16x8, two
// 8x16, four 8x8; it is coded in one of four shapes:
//   0  P_L0_16x16     one vector          (block 0)
//   1  P_L0_L0_16x8   top, bottom         (blocks 1, 2)
//   2  P_L0_L0_8x16   left, right         (blocks 3, 4)
//   3  P_8x8          four P_L0_8x8       (blocks 5 .. 8)
// There are no sub-8x8 shapes, one reference picture and no P_8x8ref0.
//
//   decide_shape    the shape at the integer stage, from the nine blocks'
//                   winning costs under enc_rate.h's key;
//   canonical_shape the shape a macroblock is coded in, the coarsest its four
//                   final vectors allow;
//   pred_block      the 8.4.1.3 predictor of every block under one slice per
//                   macroblock row, from the macroblock's own quadrants and
//                   the left macroblock's quadrants 1 and 3.
//
// Nothing here depends on the device.
#pragma once
#include <cstdint>

#include "enc_rate.h"

namespace vts {
namespace full {
namespace epart {

using erate::Mv;

enum : int { k16x16 = 0, k16x8 = 1, k8x16 = 2, k8x8 = 3 };
constexpr int kBlocks = 9;

// the quadrants of block b as a mask (bit q = quadrant q)
VTS_HD VTS_INLINE int block_quads(int b) {
  return b == 0 ? 15 : (b == 1 ? 3 : (b == 2 ? 12 : (b == 3 ? 5 : (b == 4 ? 10 : 1 << (b - 5)))));
}
// a shape's first block and its number of blocks (the blocks follow in syntax order)
VTS_HD VTS_INLINE int shape_first(int s) { return s == 0 ? 0 : (s == 1 ? 1 : (s == 2 ? 3 : 5)); }
VTS_HD VTS_INLINE int shape_blocks(int s) { return s == 0 ? 1 : (s == 3 ? 4 : 2); }
// What a shape costs before any vector: ue(v) of mb_type in a P slice (0, 1,
// 2, 3: 1, 3, 3, 5 bits) and, for P_8x8, four sub_mb_type 0 of 1 bit
VTS_HD VTS_INLINE int shape_bits(int s) { return s == 0 ? 1 : (s == 3 ? 9 : 3); }
// a block's first sample and size inside the macroblock
struct Rect {
  int x, y, w, h;
};
VTS_HD VTS_INLINE Rect block_rect(int b) {
  const int m = block_quads(b);
  return Rect{(m & 5) ? 0 : 8, (m & 3) ? 0 : 8, ((m & 5) && (m & 10)) ? 16 : 8, ((m & 3) && (m & 12)) ? 16 : 8};
}
// the quadrant of the sample (x, y) of the macroblock
VTS_HD VTS_INLINE int quad_at(int x, int y) { return (y >= 8 ? 2 : 0) + (x >= 8 ? 1 : 0); }
// a block's SAD from a candidate's four quadrant SADs
VTS_HD VTS_INLINE uint32_t block_sad(const uint32_t *q, int b) {
  const int m = block_quads(b);
  return ((m & 1) ? q[0] : 0u) + ((m & 2) ? q[1] : 0u) + ((m & 4) ? q[2] : 0u) + ((m & 8) ? q[3] : 0u);
}

// The shape at the integer stage: cost[b] is block b's least (16 SAD +
// lambda16 bits(v - p)) over the window's candidates (the cost of the winner
// under enc_rate.h's key); a shape costs the sum over its blocks plus
// lambda16 shape_bits; the least wins, ties go to the shape with fewer vectors.
VTS_HD VTS_INLINE uint32_t shape_cost(const uint32_t *cost, int lam16, int s) {
  uint32_t c = static_cast<uint32_t>(lam16) * static_cast<uint32_t>(shape_bits(s));
  for (int i = 0; i < shape_blocks(s); ++i) c += cost[shape_first(s) + i];
  return c;
}
VTS_HD VTS_INLINE int decide_shape(const uint32_t *cost, int lam16) {
  int best = 0;
  uint32_t bc = shape_cost(cost, lam16, 0);
  for (int s = 1; s < 4; ++s) {
    const uint32_t c = shape_cost(cost, lam16, s);
    if (c < bc) {
      bc = c;
      best = s;
    }
  }
  return best;
}

// The shape a macroblock is coded in: the coarsest its four quadrant vectors
// (words mvx | mvy << 16) allow
VTS_HD VTS_INLINE int canonical_shape(const uint32_t *v) {
  if (v[0] == v[1] && v[2] == v[3]) return v[0] == v[2] ? k16x16 : k16x8;
  return (v[0] == v[2] && v[1] == v[3]) ? k8x16 : k8x8;
}

// ---- words.  A vector's word is mvx | mvy << 16 (a 16x16 macroblock's
// command word); a partitioned macroblock's command word is 0x8000 | shape <<
// 16: the low half is a vector component no search can produce, the high half
// (1 .. 3) is neither I_PCM's nor an intra word's 0x8000.  Its vectors are in
// the level's mv4 array, four words a macroblock; there an intra or I_PCM
// macroblock holds kNoMv four times.
constexpr uint32_t kNoMv = 0x80008000u;
VTS_HD VTS_INLINE uint32_t part_cmd(int shape) { return 0x8000u | (static_cast<uint32_t>(shape) << 16); }
VTS_HD VTS_INLINE bool is_part_cmd(uint32_t c) { return (c & 0xfffcffffu) == 0x8000u && (c >> 16) != 0; }
VTS_HD VTS_INLINE int part_shape(uint32_t c) { return static_cast<int>(c >> 16); }
VTS_HD VTS_INLINE uint32_t mv_word(int mvx, int mvy) {
  return static_cast<uint32_t>(static_cast<uint16_t>(mvx)) | (static_cast<uint32_t>(static_cast<uint16_t>(mvy)) << 16);
}
VTS_HD VTS_INLINE Mv mv_of_word(uint32_t w) { return Mv{static_cast<int16_t>(w & 0xffffu), static_cast<int16_t>(w >> 16)}; }

// enc_rate.h's predictor guess with partitions: as pred_of_cmd, and a
// partitioned left macroblock gives its quadrant 1 (left_q1, from mv4), which
// is what the writer's predictor of a 16x16 macroblock reads there
VTS_HD VTS_INLINE Mv pred_guess(uint32_t left_prev, uint32_t left_q1, int mx, int j) {
  if (mx > 0 && j > 1 && is_part_cmd(left_prev)) return mv_of_word(left_q1);
  return erate::pred_of_cmd(left_prev, mx, j);
}

// ---- motion vector prediction (8.4.1.3).  A slice is one macroblock row:
// neighbours B, C and D of the upper blocks lie in another slice, and those of
// the lower blocks inside the macroblock; the macroblock to the right is not
// yet decoded, so its C is replaced by D.  Every block has refIdx 0.
struct Left {
  bool ok;    // the left macroblock is in the slice and has vectors (inter, P_Skip included)
  Mv q1, q3;  // its quadrants 1 and 3
};
VTS_HD VTS_INLINE int median3(int a, int b, int c) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return c < lo ? lo : (c > hi ? hi : c);
}
// The predictor of partition `part` (syntax order) of a macroblock of `shape`;
// q: the macroblock's quadrant vectors, of which only those of earlier
// partitions are read.
//   16x16      A (left quadrant 1) when it has a vector: B and C are absent,
//              so they take A's values; else (0, 0).
//   16x8 top   as 16x16 (B is absent: no directional match).
//   16x8 bottom  A (left quadrant 3) when it has a vector (the directional
//              rule); else B, the top partition, the only one with refIdx 0
//              (C is the macroblock to the right, D the left one).
//   8x16 left  A (left quadrant 1) by the directional rule, else (0, 0).
//   8x16 right C and D are absent, B is absent: A, the left partition.
//   8x8 0      as 16x16.   8x8 1: A, quadrant 0 (B, C, D absent).
//   8x8 2      median(A = left quadrant 3 or (0, 0), B = quadrant 0, C = quadrant 1).
//   8x8 3      median(A = quadrant 2, B = quadrant 1, D = quadrant 0 for C).
VTS_HD VTS_INLINE Mv pred_block(int shape, int part, const Mv *q, const Left &l) {
  const Mv zero{0, 0};
  const Mv a1 = l.ok ? l.q1 : zero;
  if (part == 0) return a1;
  if (shape == k16x8) return l.ok ? l.q3 : q[0];
  if (shape == k8x16 || part == 1) return q[0];
  if (part == 2) {
    const Mv a3 = l.ok ? l.q3 : zero;
    return Mv{median3(a3.x, q[0].x, q[1].x), median3(a3.y, q[0].y, q[1].y)};
  }
  return Mv{median3(q[2].x, q[1].x, q[0].x), median3(q[2].y, q[1].y, q[0].y)};
}
// the quadrant that carries partition `part` of `shape` (its first one)
VTS_HD VTS_INLINE int part_quad(int shape, int part) { return shape == k16x8 ? 2 * part : part; }

// Whether a macroblock with these quadrant vectors counts as sub-sample: 0
// integer, 1 a fractional component but no odd one (half), 2 an odd one (quarter)
VTS_HD VTS_INLINE int frac_class(const uint32_t *v) {
  uint32_t f = 0;
  for (int i = 0; i < 4; ++i) f |= (v[i] | (v[i] >> 16)) & 3u;
  return (f & 1u) ? 2 : (f ? 1 : 0);
}

}  // namespace epart
}  // namespace full
}  // namespace vts
