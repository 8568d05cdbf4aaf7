// enc_intra4.h — the Intra_4x4 decisions of the device encoder (transcode.hip:
// enc_intra<true>, the I_NxN syntax of enc_write / enc_write_cabac; DESIGN.md
// §11 "Intra4x4"), written once for the kernels and for the CPU harness
// (tests/native/enc_intra4_host.cpp).
//
// A slice is one macroblock row, so the row above a macroblock is never
// available: a 4x4 block has samples above it only inside its own macroblock,
// and samples to its left inside the macroblock or from the left macroblock
// (mx > 0; constrained_intra_pred_flag is 0, so any kind of macroblock will
// do).  Everything below follows from the block's index and that one fact:
//
//   avail_of      6.4.x: which neighbouring samples a block has;
//   allowed_modes the Intra4x4PredModes those samples permit;
//   pred_row      8.3.1.2.1 .. 8.3.1.2.9: one row of a block's prediction;
//   pred_mode_of  8.3.1.1: predIntra4x4PredMode from the blocks A and B;
//   mode_key      what the modes of a block are ordered by;
//   mode_code     prev_intra4x4_pred_mode_flag / rem_intra4x4_pred_mode.
//
// The per-macroblock word the levels carry (vts_transcode_ext5.i4_out): nibble
// k is the Intra4x4PredMode of luma4x4BlkIdx k; a macroblock that is not
// I_NxN has ~0.
#pragma once
#include <cstdint>

#include "enc_deblock.h"
#include "enc_rate.h"

namespace vts {
namespace full {
namespace ei4 {

// Command word of an I_NxN macroblock: kIntraCmd with bit 14, bits 0..1 zero,
// 2..3 intra_chroma_pred_mode, 4..9 coded_block_pattern.  edb::is_intra_cmd
// holds for it.
constexpr uint32_t kI4Cmd = edb::kIntraCmd | 0x4000u;
VTS_HD VTS_INLINE bool is_i4_cmd(uint32_t c) { return (c & 0xffffc000u) == kI4Cmd; }
constexpr uint64_t kNoModes = ~0ull;

// raster 4x4 index (row * 4 + column) -> luma4x4BlkIdx (6.4.3 inverted)
VTS_HD VTS_INLINE int blk_of_raster(int r) {
  const int bx = r & 3, by = r >> 2;
  return ((by >> 1) * 2 + (bx >> 1)) * 4 + (by & 1) * 2 + (bx & 1);
}
VTS_HD VTS_INLINE int mode_at(uint64_t word, int k) { return static_cast<int>((word >> (4 * k)) & 15u); }

// The neighbouring samples of luma4x4BlkIdx k; mb_left: the macroblock has a
// left neighbour in its slice (mx > 0).  tr false: p[4..7, -1] repeat p[3, -1].
struct Avail {
  bool left, top, tl, tr;
};
VTS_HD VTS_INLINE Avail avail_of(int k, bool mb_left) {
  const int r = edb::raster_of_blk(k), bx = r & 3, by = r >> 2;
  Avail a;
  a.left = bx > 0 || mb_left;
  a.top = by > 0;
  a.tl = a.left && a.top;
  // the block above and to the right lies in this macroblock and precedes k: blocks 2, 6, 8, 9, 10, 12, 14
  a.tr = ((0x5744u >> k) & 1u) != 0;
  return a;
}
// bit m set: Intra4x4PredMode m may be used.  0 Vertical, 3 Diagonal_Down_Left
// and 7 Vertical_Left need the samples above; 1 Horizontal and 8 Horizontal_Up
// those to the left; 4, 5, 6 both and the corner; 2 DC nothing.
VTS_HD VTS_INLINE uint32_t allowed_modes(const Avail &a) {
  uint32_t m = 1u << 2;
  if (a.top) m |= (1u << 0) | (1u << 3) | (1u << 7);
  if (a.left) m |= (1u << 1) | (1u << 8);
  if (a.top && a.left && a.tl) m |= (1u << 4) | (1u << 5) | (1u << 6);
  return m;
}

// Row y of the prediction of mode `mode`, four samples packed low byte first.
// T[0] = L[0] = p[-1, -1], T[1 + x] = p[x, -1] for x = 0..7 (the caller has
// replicated p[3, -1] where the top-right samples are unavailable), L[1 + y] =
// p[-1, y].  The statements are the decoder's (recon_full.h, MbRecon::intra4x4).
VTS_HD VTS_INLINE uint32_t pred_row(int mode, int y, const int *T, const int *L, const Avail &a) {
#define PT(x) T[1 + (x)]
#define PL(y) L[1 + (y)]
  uint32_t out = 0;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    int v;
    switch (mode) {
      case 0: v = PT(x); break;
      case 1: v = PL(y); break;
      case 2:
        if (a.top && a.left) v = (PT(0) + PT(1) + PT(2) + PT(3) + PL(0) + PL(1) + PL(2) + PL(3) + 4) >> 3;
        else if (a.left) v = (PL(0) + PL(1) + PL(2) + PL(3) + 2) >> 2;
        else if (a.top) v = (PT(0) + PT(1) + PT(2) + PT(3) + 2) >> 2;
        else v = 128;
        break;
      case 3:
        v = (x == 3 && y == 3) ? (PT(6) + 3 * PT(7) + 2) >> 2 : (PT(x + y) + 2 * PT(x + y + 1) + PT(x + y + 2) + 2) >> 2;
        break;
      case 4:
        if (x > y) v = (PT(x - y - 2) + 2 * PT(x - y - 1) + PT(x - y) + 2) >> 2;
        else if (x < y) v = (PL(y - x - 2) + 2 * PL(y - x - 1) + PL(y - x) + 2) >> 2;
        else v = (PT(0) + 2 * PT(-1) + PL(0) + 2) >> 2;
        break;
      case 5: {
        const int z = 2 * x - y;
        if (z >= 0 && !(z & 1)) v = (PT(x - (y >> 1) - 1) + PT(x - (y >> 1)) + 1) >> 1;
        else if (z >= 0) v = (PT(x - (y >> 1) - 2) + 2 * PT(x - (y >> 1) - 1) + PT(x - (y >> 1)) + 2) >> 2;
        else if (z == -1) v = (PL(0) + 2 * PL(-1) + PT(0) + 2) >> 2;
        else v = (PL(y - 1) + 2 * PL(y - 2) + PL(y - 3) + 2) >> 2;
        break;
      }
      case 6: {
        const int z = 2 * y - x;
        if (z >= 0 && !(z & 1)) v = (PL(y - (x >> 1) - 1) + PL(y - (x >> 1)) + 1) >> 1;
        else if (z >= 0) v = (PL(y - (x >> 1) - 2) + 2 * PL(y - (x >> 1) - 1) + PL(y - (x >> 1)) + 2) >> 2;
        else if (z == -1) v = (PL(0) + 2 * PL(-1) + PT(0) + 2) >> 2;
        else v = (PT(x - 1) + 2 * PT(x - 2) + PT(x - 3) + 2) >> 2;
        break;
      }
      case 7:
        v = (y & 1) ? (PT(x + (y >> 1)) + 2 * PT(x + (y >> 1) + 1) + PT(x + (y >> 1) + 2) + 2) >> 2
                    : (PT(x + (y >> 1)) + PT(x + (y >> 1) + 1) + 1) >> 1;
        break;
      default: {
        const int z = x + 2 * y;
        if (z == 0 || z == 2 || z == 4) v = (PL(y + (x >> 1)) + PL(y + (x >> 1) + 1) + 1) >> 1;
        else if (z == 1 || z == 3) v = (PL(y + (x >> 1)) + 2 * PL(y + (x >> 1) + 1) + PL(y + (x >> 1) + 2) + 2) >> 2;
        else if (z == 5) v = (PL(2) + 3 * PL(3) + 2) >> 2;
        else v = PL(3);
        break;
      }
    }
    out |= static_cast<uint32_t>(v) << (8 * x);
  }
#undef PT
#undef PL
  return out;
}

// The neighbour samples of block k out of the macroblock's tile: 16 rows of
// `pitch` bytes, bytes 0..3 of a row the left macroblock's last four columns
// (byte 3 is p[-1, y] of column 0; any value when mb_left is false), bytes
// 4..19 the macroblock's own reconstruction so far.  Unavailable samples are 0
// (no allowed mode reads them), the top-right ones repeat p[3, -1].
constexpr int kTilePitch = 20;
// sample i of the block's 13: i = 0..8 is T[i], 9..12 is L[i - 8] (the kernel fills them one per lane)
VTS_HD VTS_INLINE int edge_sample(const uint8_t *tile, int k, const Avail &a, int i) {
  const int r = edb::raster_of_blk(k), bx = r & 3, by = r >> 2;
  const uint8_t *p = tile + by * 4 * kTilePitch + 4 + bx * 4;  // the block's sample (0, 0)
  if (i == 0) return a.tl ? p[-kTilePitch - 1] : 0;
  if (i < 9) return a.top ? p[-kTilePitch + ((i - 1 < 4 || a.tr) ? i - 1 : 3)] : 0;
  return a.left ? p[(i - 9) * kTilePitch - 1] : 0;
}
VTS_HD VTS_INLINE void neighbours(const uint8_t *tile, int k, const Avail &a, int *T, int *L) {
#pragma unroll
  for (int i = 0; i < 9; ++i) T[i] = edge_sample(tile, k, a, i);
  L[0] = T[0];
#pragma unroll
  for (int i = 9; i < 13; ++i) L[i - 8] = edge_sample(tile, k, a, i);
}

// predIntra4x4PredMode of block k (8.3.1.1).  cur: the modes of this
// macroblock's earlier blocks; mb_left: the left macroblock exists; left: its
// word (kNoModes unless it is I_NxN: any other kind counts as DC, 2).  B, the
// macroblock above, is another slice: every top-row block is predicted 2
// (dcPredModePredictedFlag), and so is column 0 without a left macroblock.
VTS_HD VTS_INLINE int pred_mode_of(int k, uint64_t cur, bool mb_left, uint64_t left) {
  const int r = edb::raster_of_blk(k), bx = r & 3, by = r >> 2;
  if (by == 0 || (bx == 0 && !mb_left)) return 2;
  const int ma = bx ? mode_at(cur, blk_of_raster(r - 1)) : (left == kNoModes ? 2 : mode_at(left, blk_of_raster(by * 4 + 3)));
  const int mb = mode_at(cur, blk_of_raster(r - 4));
  return ma < mb ? ma : mb;
}

// bits of a block's mode in the slice data: prev_intra4x4_pred_mode_flag, and
// rem_intra4x4_pred_mode when the mode is not the predicted one (CAVLC)
VTS_HD VTS_INLINE int mode_bits(int mode, int pred) { return mode == pred ? 1 : 4; }
// rem_intra4x4_pred_mode of a mode that is not the predicted one
VTS_HD VTS_INLINE int rem_mode(int mode, int pred) { return mode < pred ? mode : mode - 1; }

// What a block's modes are ordered by: (16 SAD + lambda16_of_qp(qp) bits,
// mode); the least key wins, so ties go to the lower mode number.  SAD <= 16
// x 255 and lambda16 <= 1335: the cost stays within 17 bits.
VTS_HD VTS_INLINE uint64_t mode_key(uint32_t sad, int qp, int mode, int pred) {
  const uint32_t cost = 16u * sad + static_cast<uint32_t>(erate::lambda16_of_qp(qp)) * static_cast<uint32_t>(mode_bits(mode, pred));
  return (static_cast<uint64_t>(cost) << 32) | static_cast<uint32_t>(mode);
}
VTS_HD VTS_INLINE int key_mode(uint64_t key) { return static_cast<int>(key & 15u); }

// SAD of two rows of four packed samples (the kernel uses v_sad_u8)
VTS_HD VTS_INLINE uint32_t sad_row4(uint32_t a, uint32_t b) {
  uint32_t s = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int d = static_cast<int>((a >> (8 * c)) & 255u) - static_cast<int>((b >> (8 * c)) & 255u);
    s += static_cast<uint32_t>(d < 0 ? -d : d);
  }
  return s;
}

}  // namespace ei4
}  // namespace full
}  // namespace vts
