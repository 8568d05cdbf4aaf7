// enc_deblock.h — the decisions of the device encoder's in-loop deblocking
// filter (transcode.hip: enc_deblock), written once for the
// kernel and for the CPU harness (tests/native/enc_deblock_host.cpp).
//
// The encoder writes one slice per macroblock row with
// disable_deblocking_filter_idc = 2, so a macroblock's left edge, its three
// inner vertical and its three inner horizontal luma edges are filtered and
// its top edge never is (8.7).  Everything is decided from what a level
// already holds about a macroblock: its command word, coded_block_pattern and
// levels.  The tables and the sample filter are the decoder's
// (h264_tables.h, full::filter_line); nothing is restated here.
#pragma once
#include <cstdint>

#include "recon_full.h"

namespace vts {
namespace full {
namespace edb {

// Command words of the encoder's levels (enc_search / enc_intra write them,
// enc_write and enc_deblock read them): an inter macroblock's is its
// quarter-sample vector, mvx | mvy << 16.
constexpr uint32_t kPcmCmd = 0x80008000u;    // (mvx, mvy) = (-32768, -32768): never a motion
constexpr uint32_t kIntraCmd = 0x80000000u;  // Intra16x16: high half 0x8000, bit 15 clear (modes, cbp below)
VTS_HD VTS_INLINE bool is_intra_cmd(uint32_t c) { return (c & 0xffff8000u) == kIntraCmd; }

enum : int { kInter = 0, kI16 = 1, kPcm = 2 };

// What the filter needs of one macroblock.
struct Mb {
  int kind;      // kInter (P_L0_16x16 or P_Skip, one reference picture), kI16, kPcm
  int mvx, mvy;  // quarter samples (inter; P_Skip is (0, 0) here: the row above is another slice)
  uint32_t nz;   // inter: bit b set = the raster 4x4 luma block b has a non-zero level
  bool part;     // inter with partitions (enc_part.h): the vector is per 8x8 quadrant, in q0 .. q3
  uint32_t q0, q1, q2, q3;  // part: the quadrants' vectors as words mvx | mvy << 16, raster order (scalars: no
                            // member is ever indexed, so the struct stays in registers)
};

// luma4x4BlkIdx -> raster 4x4 index (6.4.3)
VTS_HD VTS_INLINE int raster_of_blk(int k) { return ((k >> 3) * 2 + ((k >> 1) & 1)) * 4 + ((k >> 2) & 1) * 2 + (k & 1); }

// The non-zero mask of an inter macroblock from its levels as enc_search
// stores them (16 per block, by luma4x4BlkIdx): a block counts only when its
// 8x8's coded_block_pattern bit is set (enc_write codes no other)
VTS_HD VTS_INLINE bool blk_nz(const int16_t *lv, int cbp, int k) {  // lv: the 16 levels of block k (luma4x4BlkIdx)
  if (!((cbp >> (k >> 2)) & 1)) return false;
  bool any = false;
  for (int q = 0; q < 16; ++q) any |= lv[q] != 0;
  return any;
}
VTS_HD VTS_INLINE uint32_t nz_raster(uint32_t by_blk) {  // bit k by luma4x4BlkIdx -> bit by raster index
  uint32_t nz = 0;
  for (int k = 0; k < 16; ++k) nz |= ((by_blk >> k) & 1u) << raster_of_blk(k);
  return nz;
}
VTS_HD inline uint32_t nz_of_levels(const int16_t *cp, int cbp) {
  uint32_t by_blk = 0;
  for (int k = 0; k < 16; ++k) by_blk |= static_cast<uint32_t>(blk_nz(cp + 16 * k, cbp, k)) << k;
  return nz_raster(by_blk);
}

VTS_HD VTS_INLINE Mb mb_of_cmd(uint32_t cmd, uint32_t nz) {
  Mb m;
  m.kind = cmd == kPcmCmd ? kPcm : (is_intra_cmd(cmd) ? kI16 : kInter);
  m.mvx = m.kind == kInter ? static_cast<int16_t>(cmd & 0xffffu) : 0;
  m.mvy = m.kind == kInter ? static_cast<int16_t>(cmd >> 16) : 0;
  m.nz = m.kind == kInter ? nz : 0;
  m.part = false;
  m.q0 = m.q1 = m.q2 = m.q3 = 0;
  return m;
}
// The same with partitions on: mv4 the macroblock's four quadrant vectors
// (enc_part.h: the level's mv4 array), which every inter macroblock has; a
// partitioned macroblock's command word (low half 0x8000, high half 1..3) is
// inter and carries no vector itself
VTS_HD VTS_INLINE Mb mb_of_cmd4(uint32_t cmd, uint32_t nz, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
  Mb m = mb_of_cmd(cmd, nz);
  const bool inter = m.kind == kInter;
  m.part = inter;
  m.q0 = inter ? v0 : 0;
  m.q1 = inter ? v1 : 0;
  m.q2 = inter ? v2 : 0;
  m.q3 = inter ? v3 : 0;
  return m;
}
VTS_HD VTS_INLINE Mb mb_of_cmd4(uint32_t cmd, uint32_t nz, const uint32_t *mv4) {
  return mb_of_cmd4(cmd, nz, mv4[0], mv4[1], mv4[2], mv4[3]);
}
// the quadrant of raster 4x4 block b
VTS_HD VTS_INLINE int quad_of_raster(int b) { return ((b >> 3) << 1) | ((b >> 1) & 1); }

// quadrant i's vector, by selects: the index is a lane's own
VTS_HD VTS_INLINE uint32_t quad_word(const Mb &m, int i) { return i == 0 ? m.q0 : (i == 1 ? m.q1 : (i == 2 ? m.q2 : m.q3)); }
// The motion part of bS (8.7.2.1, one reference picture): the two 4x4 blocks'
// vectors differ by >= 4 quarter samples in a component.  Without partitions a
// macroblock has one vector; with them each block has its quadrant's, so the
// inner edges at x = 8 and y = 8 can be 1 and the left edge is 1 per half.
VTS_HD VTS_INLINE bool blocks_far(const Mb &p, int bp, const Mb &q, int bq) {
  if (!p.part && !q.part) return mv_far(p.mvx, p.mvy, q.mvx, q.mvy);
  const uint32_t a = quad_word(p, quad_of_raster(bp)), b = quad_word(q, quad_of_raster(bq));
  return mv_far(static_cast<int16_t>(a & 0xffffu), static_cast<int16_t>(a >> 16), static_cast<int16_t>(b & 0xffffu),
                static_cast<int16_t>(b >> 16));
}

// bS of a line between raster 4x4 blocks bp of p and bq of q (8.7.2.1).
// kPart = false: no macroblock has quadrant vectors (the encoder without
// partitions: the code is what it was)
template <bool kPart = true>
VTS_HD VTS_INLINE int bs(const Mb &p, int bp, const Mb &q, int bq, bool mb_edge) {
  if (p.kind != kInter || q.kind != kInter) return mb_edge ? 4 : 3;
  if (((p.nz >> bp) | (q.nz >> bq)) & 1u) return 2;
  if constexpr (kPart) return blocks_far(p, bp, q, bq) ? 1 : 0;
  else return mv_far(p.mvx, p.mvy, q.mvx, q.mvy) ? 1 : 0;
}

// bS of line k (0..15, luma samples along the edge) of edge e (0: the left
// macroblock edge, p = the macroblock to the left; 1..3: inner, p = q) in
// direction dir (0: vertical edges, 1: horizontal edges)
template <bool kPart = true>
VTS_HD VTS_INLINE int line_bs(const Mb &p, const Mb &q, int dir, int e, int k) {
  const int bq = dir ? e * 4 + (k >> 2) : (k >> 2) * 4 + e;
  const int bp = dir ? ((e + 3) & 3) * 4 + (k >> 2) : (k >> 2) * 4 + ((e + 3) & 3);
  return bs<kPart>(p, bp, q, bq, e == 0);
}

// qPp / qPq of 8.7.2.2: 0 for I_PCM, else the slice's QP (mb_qp_delta is 0)
VTS_HD VTS_INLINE int qp_of(const Mb &m, int slice_qp) { return m.kind == kPcm ? 0 : slice_qp; }

struct Idx {
  int iA, alpha, beta;
};
// indexA / indexB and alpha' / beta' of an edge between macroblocks of qPp and
// qPq; off_a / off_b = FilterOffsetA / B = 2 slice_alpha_c0_offset_div2 / 2
// slice_beta_offset_div2; chroma: QPc of each side with the PPS's
// chroma_qp_index_offset cqp_off
VTS_HD VTS_INLINE Idx indices(int qpp, int qpq, int off_a, int off_b, bool chroma, int cqp_off) {
  const int qpav = chroma ? (qpc_of(qpp, cqp_off) + qpc_of(qpq, cqp_off) + 1) >> 1 : (qpp + qpq + 1) >> 1;
  Idx x;
  x.iA = clip3(0, 51, qpav + off_a);
  x.alpha = kAl[x.iA];
  x.beta = kBe[clip3(0, 51, qpav + off_b)];
  return x;
}

// One line across an edge, s[k step], k = -4..3; true when the line's
// filterSamplesFlag was set (the samples went through the filter)
VTS_HD VTS_INLINE bool filter(uint8_t *s, int64_t step, int bS, bool chroma, const Idx &x) {
  if (!x.alpha || !x.beta || bS <= 0) return false;
  const int p0 = s[-step], p1 = s[-2 * step], q0 = s[0], q1 = s[step];
  const bool on = iabs(p0 - q0) < x.alpha && iabs(p1 - p0) < x.beta && iabs(q1 - q0) < x.beta;
  filter_line(s, step, bS, chroma, x.iA, x.alpha, x.beta);
  return on;
}

}  // namespace edb
}  // namespace full
}  // namespace vts
