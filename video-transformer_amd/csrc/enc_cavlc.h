// enc_cavlc.h — CAVLC slice data (7.3.4, 7.3.5, 9.2) of the device encoder's
// slices (transcode.hip: enc_write), written once for the
// kernels and for the CPU harnesses (tests/native/enc_cabac_host.cpp,
// enc_intra4_host.cpp, enc_part_host.cpp).  oracle/transcode_oracle.c restates it independently.
//
//   residual_block  residual_block_cavlc of one block into a Sink (enc_rbsp.h:
//                   the kernel's WordSink, the harness's ByteSink, BitCount),
//                   or counted with no sink at all (count_block: what
//                   enc_search and enc_intra call on every lane);
//   nc_luma / nc_chroma  nC of 9.2.1 from the blocks' total_coeff;
//   Row             what a slice carries from macroblock to macroblock;
//   mb_*            macroblock_layer() of each kind from what a level holds
//                   about it (command word, coded_block_pattern, levels, mode
//                   word), from mb_skip_run on, leaving the Row as the
//                   macroblock to the right finds it.  dqp is the mb_qp_delta
//                   a macroblock sends when its syntax has one (enc_aq.h's
//                   running-QP rule is the caller's; 0 without adaptive
//                   quantisation).
//
// A slice is one macroblock row: neighbour B (above) is never available
// across macroblocks, and A (left) is the previous macroblock of the slice.
#pragma once
#include <cstdint>
#include <type_traits>

#include "enc_deblock.h"
#include "enc_intra4.h"
#include "enc_part.h"
#include "enc_rbsp.h"
#include "h264_tables.h"

namespace vts {
namespace full {
namespace ecav {

using erbsp::ue_bits;

// Under hipcc the tables are device constants and the functions device
// functions only: a use from host code, were it only a __host__ __device__
// function that nothing calls, makes the compiler export a static device
// variable, and every access to it then loads its address from the GOT.
#if defined(__HIPCC__)
#define VTS_EVTAB __device__ __constant__ static const
#define VTS_EV __device__
#else
#define VTS_EVTAB static const
#define VTS_EV
#endif
VTS_EVTAB uint8_t kCtLen[4][17][4] = VTS_CT_LEN_DATA;
VTS_EVTAB uint8_t kCtCode[4][17][4] = VTS_CT_CODE_DATA;
VTS_EVTAB uint8_t kTzLen[15][16] = VTS_TZ_LEN_DATA;
VTS_EVTAB uint8_t kTzCode[15][16] = VTS_TZ_CODE_DATA;
VTS_EVTAB uint8_t kTzcLen[3][4] = VTS_TZC_LEN_DATA;
VTS_EVTAB uint8_t kTzcCode[3][4] = VTS_TZC_CODE_DATA;
VTS_EVTAB uint8_t kRbLen[7][15] = VTS_RB_LEN_DATA;
VTS_EVTAB uint8_t kRbCode[7][15] = VTS_RB_CODE_DATA;
VTS_EVTAB uint8_t kCbpInterTab[48] = VTS_CBPP_DATA;  // Table 9-4, Inter column
VTS_EVTAB uint8_t kCbpIntraTab[48] = VTS_CBPI_DATA;  // Table 9-4, Intra_4x4 column
#undef VTS_EVTAB

// me(v) of coded_block_pattern (Table 9-4)
VTS_EV VTS_INLINE uint32_t cbp_inter_code(int cbp) {
  uint32_t code = 0;
  while (kCbpInterTab[code] != cbp) ++code;
  return code;
}
VTS_EV VTS_INLINE uint32_t cbp_intra_code(int cbp) {
  uint32_t code = 0;
  while (kCbpIntraTab[code] != cbp) ++code;
  return code;
}

// ------------------------------------------------------- the block coder
struct NoSink {};  // residual_block counts only
struct Block {
  int bits, tc;  // the block's bits and its total_coeff
};

// residual_block_cavlc (7.3.5.3.2, 9.2) of levels lv[0, maxNum) in scan order
// with nC (-1: chroma DC); nC < -1: an upper bound on the bits (coeff_token
// taken as the longest code over the nC classes and the 6-bit FLC; nothing
// can be written).  Sink = NoSink: o is not touched.  The loops run over all
// 16 positions so that a register array is indexed by constants.
template <class Sink, class Lv>
VTS_EV Block residual_block(Sink *o, const Lv *lv, int maxNum, int nC) {
  constexpr bool kWrite = !std::is_same<Sink, NoSink>::value;
  int tc = 0, t1 = 0, top = -1;
  bool open = true;
#pragma unroll
  for (int i = 15; i >= 0; --i) {
    const int v = i < maxNum ? lv[i] : 0;
    if (!v) continue;
    if (top < 0) top = i;
    ++tc;
    if (open && t1 < 3 && (v == 1 || v == -1)) ++t1;
    else open = false;
  }
  int bits;
  if (nC < -1) {  // the bound
    const int a = kCtLen[0][tc][t1], b = kCtLen[1][tc][t1], c = kCtLen[2][tc][t1];
    const int ab = a > b ? a : b, abc = ab > c ? ab : c;
    bits = abc > 6 ? abc : 6;
  } else if (nC >= 8) {
    bits = 6;
    if constexpr (kWrite) o->bits(6, tc == 0 ? 3u : static_cast<uint32_t>(((tc - 1) << 2) | t1));
  } else {
    const int col = nC == -1 ? 3 : (nC < 2 ? 0 : (nC < 4 ? 1 : 2));
    bits = kCtLen[col][tc][t1];
    if constexpr (kWrite) o->bits(bits, kCtCode[col][tc][t1]);
  }
  if (tc == 0) return Block{bits, 0};
  int k = 0, sl = (tc > 10 && t1 < 3) ? 1 : 0;
#pragma unroll
  for (int i = 15; i >= 0; --i) {  // trailing ones' signs, then levels (9.2.2.1 inverted)
    const int v = i < maxNum ? lv[i] : 0;
    if (!v) continue;
    if (k < t1) {
      ++bits;
      if constexpr (kWrite) o->bits(1, v < 0 ? 1u : 0u);
    } else {
      int code = v > 0 ? 2 * v - 2 : -2 * v - 1;
      if (k == t1 && t1 < 3) code -= 2;
      int prefix, suffix = 0, ssize = 0;
      if (sl == 0) {
        if (code < 14) prefix = code;
        else if (code < 30) { prefix = 14; suffix = code - 14; ssize = 4; }
        else { prefix = 15; suffix = code - 30; ssize = 12; }
      } else if (code < (15 << sl)) {
        prefix = code >> sl;
        suffix = code & ((1 << sl) - 1);
        ssize = sl;
      } else {
        prefix = 15;
        suffix = code - (15 << sl);
        ssize = 12;
      }
      bits += prefix + 1 + ssize;
      if constexpr (kWrite) {
        o->bits(prefix + 1, 1u);
        if (ssize) o->bits(ssize, static_cast<uint32_t>(suffix));
      }
      if (sl == 0) sl = 1;
      if ((v < 0 ? -v : v) > (3 << (sl - 1)) && sl < 6) ++sl;
    }
    ++k;
  }
  int zl = top + 1 - tc;  // total_zeros
  if (tc < maxNum) {
    const int len = maxNum == 4 ? kTzcLen[tc - 1][zl] : kTzLen[tc - 1][zl];
    bits += len;
    if constexpr (kWrite) o->bits(len, maxNum == 4 ? kTzcCode[tc - 1][zl] : kTzCode[tc - 1][zl]);
  }
  int prev = -1;
#pragma unroll
  for (int i = 15; i >= 0; --i) {  // run_before of every coefficient but the lowest
    const int v = i < maxNum ? lv[i] : 0;
    if (!v) continue;
    if (prev >= 0 && zl > 0) {
      const int run = prev - i - 1, row = (zl < 7 ? zl : 7) - 1;
      bits += kRbLen[row][run];
      if constexpr (kWrite) o->bits(kRbLen[row][run], kRbCode[row][run]);
      zl -= run;
    }
    prev = i;
  }
  return Block{bits, tc};
}
// the block's bits, nothing written
template <class Lv>
VTS_EV VTS_INLINE int count_block(const Lv *lv, int maxNum, int nC) {
  return residual_block(static_cast<NoSink *>(nullptr), lv, maxNum, nC).bits;
}

// ------------------------------------------------------- nC (9.2.1)
// from the left (na) and upper (nb) blocks' total_coeff, -1 = unavailable
VTS_EV VTS_INLINE int nc_of(int na, int nb) {
  return (na >= 0 && nb >= 0) ? (na + nb + 1) >> 1 : (na >= 0 ? na : (nb >= 0 ? nb : 0));
}
// luma block at raster index r: cur the macroblock's sixteen total_coeff
// (raster), left the left macroblock's right column
VTS_EV VTS_INLINE int nc_luma(int r, const int *cur, const int *left) {
  const int bx = r & 3, by = r >> 2;
  return nc_of(bx ? cur[r - 1] : left[by], by ? cur[r - 4] : -1);
}
// chroma AC block k of plane pl: cur [plane][block], left [plane][row]
VTS_EV VTS_INLINE int nc_chroma(int pl, int k, const int (*cur)[4], const int (*left)[2]) {
  const int bx = k & 1, by = k >> 1;
  return nc_of(bx ? cur[pl][by * 2] : left[pl][by], by ? cur[pl][bx] : -1);
}

// ------------------------------------------------------- the slice's state
struct Row {
  int lnz[4], lnzc[2][2];   // total_coeff of the left macroblock's right column, -1 none
  int cnz[16], cnzc[2][4];  // the current macroblock's: luma raster, chroma [plane][block]
  uint64_t left_modes;      // the left macroblock's Intra4x4PredModes when it is I_NxN, else ~0
  bool has_left;
  bool a_ok;                // the left macroblock has a motion vector (8.4.1.3: A the only neighbour)
  int amx, amy;             // ... of its quadrant 1, beside this macroblock's upper half
  int a3x, a3y;             // ... of its quadrant 3 (partitions, enc_part.h; else the same vector)
  uint32_t skip;            // the pending mb_skip_run
  VTS_EV void start() {     // of a slice
    all(-1);
    left_modes = ei4::kNoModes;
    has_left = a_ok = false;
    amx = amy = a3x = a3y = 0;
    skip = 0;
  }
  VTS_EV void all(int v) {  // 16 after I_PCM, 0 after P_Skip
    for (int i = 0; i < 4; ++i) lnz[i] = v;
    lnzc[0][0] = lnzc[0][1] = lnzc[1][0] = lnzc[1][1] = v;
  }
  VTS_EV void clear() {
    for (int i = 0; i < 16; ++i) cnz[i] = 0;
    for (int i = 0; i < 4; ++i) cnzc[0][i] = cnzc[1][i] = 0;
  }
  VTS_EV void shift() {     // the macroblock becomes the left one
    for (int i = 0; i < 4; ++i) lnz[i] = cnz[i * 4 + 3];
    for (int pl = 0; pl < 2; ++pl) {
      lnzc[pl][0] = cnzc[pl][1];
      lnzc[pl][1] = cnzc[pl][3];
    }
  }
  // the neighbour facts other than total_coeff that a macroblock leaves
  VTS_EV void left_is(uint64_t modes, bool mv, int mvx, int mvy) {
    left_modes = modes;
    has_left = true;
    a_ok = mv;
    amx = a3x = mvx;
    amy = a3y = mvy;
  }
  VTS_EV epart::Left left_mv() const { return epart::Left{a_ok, {amx, amy}, {a3x, a3y}}; }
};

// ------------------------------------------------------- residual() (7.3.5.3)
// cp: a macroblock's levels in transcode.hip's layout: luma at 0, Cb / Cr DC
// at 256, AC at 264 (8 blocks of 15)
template <class Sink>
VTS_EV void chroma_residual(Sink &o, const int16_t *cp, int cc, Row &z) {
  int lv[16];
  if (cc)
    for (int pl = 0; pl < 2; ++pl) {
      for (int q = 0; q < 4; ++q) lv[q] = cp[256 + 4 * pl + q];
      residual_block(&o, lv, 4, -1);
    }
  if (cc == 2)
    for (int pl = 0; pl < 2; ++pl)
      for (int k = 0; k < 4; ++k) {
        for (int q = 0; q < 15; ++q) lv[q] = cp[264 + 60 * pl + 15 * k + q];
        z.cnzc[pl][k] = residual_block(&o, lv, 15, nc_chroma(pl, k, z.cnzc, z.lnzc)).tc;
      }
}
// sixteen blocks of 16 by luma4x4BlkIdx under the 8x8 pattern (inter, I_NxN)
template <class Sink>
VTS_EV void luma_residual(Sink &o, const int16_t *cp, int cbp, Row &z) {
  int lv[16];
  for (int k = 0; k < 16; ++k) {
    if (!((cbp >> (k >> 2)) & 1)) continue;
    const int r = edb::raster_of_blk(k);
    for (int q = 0; q < 16; ++q) lv[q] = cp[16 * k + q];
    z.cnz[r] = residual_block(&o, lv, 16, nc_luma(r, z.cnz, z.lnz)).tc;
  }
}
// Intra16x16DCLevel at 0 (nC of block 0), then the sixteen Intra16x16ACLevel
// blocks of 15 at 16 when the luma pattern is 15
template <class Sink>
VTS_EV void luma16_residual(Sink &o, const int16_t *cp, int cbp, Row &z) {
  int lv[16];
  for (int q = 0; q < 16; ++q) lv[q] = cp[q];
  residual_block(&o, lv, 16, nc_luma(0, z.cnz, z.lnz));
  if (cbp & 15)
    for (int k = 0; k < 16; ++k) {
      const int r = edb::raster_of_blk(k);
      for (int q = 0; q < 15; ++q) lv[q] = cp[16 + 15 * k + q];
      z.cnz[r] = residual_block(&o, lv, 15, nc_luma(r, z.cnz, z.lnz)).tc;
    }
}

// ------------------------------------------------------- macroblocks
// mb_skip_run ahead of a macroblock that is not skipped (P slices)
template <class Sink>
VTS_EV VTS_INLINE void skip_run(Sink &o, bool islice, Row &z) {
  if (!islice) {
    o.ue(z.skip);
    z.skip = 0;
  }
}
// P_Skip: counted, written with the next macroblock or by slice_end.  Its
// motion is 0: neighbour B lies in another slice.
VTS_EV VTS_INLINE void mb_skip(Row &z) {
  ++z.skip;
  z.all(0);
  z.left_is(ei4::kNoModes, true, 0, 0);
}
// P_L0_16x16 from its command word (the vector, mvx | mvy << 16),
// coded_block_pattern and levels
template <class Sink>
VTS_EV void mb_inter(Sink &o, Row &z, uint32_t cmd, int cbp, const int16_t *cp, int dqp = 0) {
  const int mvx = static_cast<int16_t>(cmd & 0xffffu), mvy = static_cast<int16_t>(cmd >> 16);
  skip_run(o, false, z);
  o.ue(0);  // mb_type
  o.se(mvx - (z.a_ok ? z.amx : 0));
  o.se(mvy - (z.a_ok ? z.amy : 0));
  o.ue(cbp_inter_code(cbp));
  z.clear();
  if (cbp) {
    o.se(dqp);  // mb_qp_delta
    luma_residual(o, cp, cbp, z);
    chroma_residual(o, cp, cbp >> 4, z);
  }
  z.shift();
  z.left_is(ei4::kNoModes, true, mvx, mvy);
}
// A partitioned macroblock (enc_part.h) from its command word (0x8000 | shape
// << 16, shape 1 P_L0_L0_16x8, 2 P_L0_L0_8x16, 3 P_8x8 of four P_L0_8x8), its
// four quadrant vectors mv4 (words), coded_block_pattern and levels: mb_type,
// the sub_mb_types, the mvds in syntax order against epart::pred_block (one
// reference picture: no ref_idx_l0), then as mb_inter
template <class Sink>
VTS_EV void mb_p_part(Sink &o, Row &z, uint32_t cmd, const uint32_t *mv4, int cbp, const int16_t *cp, int dqp = 0) {
  const int shape = epart::part_shape(cmd);
  epart::Mv q[4];
  for (int i = 0; i < 4; ++i) q[i] = epart::mv_of_word(mv4[i]);
  skip_run(o, false, z);
  o.ue(static_cast<uint32_t>(shape));  // mb_type
  if (shape == epart::k8x8)
    for (int i = 0; i < 4; ++i) o.ue(0);  // sub_mb_type P_L0_8x8
  const epart::Left l = z.left_mv();
  for (int part = 0; part < epart::shape_blocks(shape); ++part) {
    const epart::Mv p = epart::pred_block(shape, part, q, l), v = q[epart::part_quad(shape, part)];
    o.se(v.x - p.x);
    o.se(v.y - p.y);
  }
  o.ue(cbp_inter_code(cbp));
  z.clear();
  if (cbp) {
    o.se(dqp);  // mb_qp_delta
    luma_residual(o, cp, cbp, z);
    chroma_residual(o, cp, cbp >> 4, z);
  }
  z.shift();
  z.left_is(ei4::kNoModes, true, q[1].x, q[1].y);
  z.a3x = q[3].x;
  z.a3y = q[3].y;
}
// macroblock_layer() of Intra16x16 from mb_type on (Table 7-11; 5 more in a P
// slice), from its command word (bits 0..1 Intra16x16PredMode, 2..3
// intra_chroma_pred_mode, 4..9 coded_block_pattern) and levels
template <class Sink>
VTS_EV void intra16_layer(Sink &o, bool islice, Row &z, uint32_t cmd, const int16_t *cp, int dqp = 0) {
  const int cbp = static_cast<int>(cmd >> 4) & 63;
  const uint32_t mbt = 1 + (cmd & 3u) + 4 * static_cast<uint32_t>(cbp >> 4) + ((cbp & 15) ? 12 : 0);
  o.ue(islice ? mbt : 5 + mbt);
  o.ue((cmd >> 2) & 3u);  // intra_chroma_pred_mode
  o.se(dqp);              // mb_qp_delta
  z.clear();
  luma16_residual(o, cp, cbp, z);
  chroma_residual(o, cp, cbp >> 4, z);
  z.shift();
  z.left_is(ei4::kNoModes, false, 0, 0);
}
// macroblock_layer() of I_NxN from mb_type on (0; 5 in a P slice), from its
// command word (bits 2..3 intra_chroma_pred_mode, 4..9 coded_block_pattern),
// its Intra4x4PredModes and levels (the inter layout).  There is no
// transform_size_8x8_flag: the PPS has no 8x8 transform.
template <class Sink>
VTS_EV void intra4_layer(Sink &o, bool islice, Row &z, uint32_t cmd, uint64_t modes, const int16_t *cp, int dqp = 0) {
  const int cbp = static_cast<int>(cmd >> 4) & 63;
  o.ue(islice ? 0 : 5);
  for (int k = 0; k < 16; ++k) {
    const int m = ei4::mode_at(modes, k), pm = ei4::pred_mode_of(k, modes, z.has_left, z.left_modes);
    if (m == pm) o.bits(1, 1);  // prev_intra4x4_pred_mode_flag
    else o.bits(4, static_cast<uint32_t>(ei4::rem_mode(m, pm)));  // the flag 0, rem_intra4x4_pred_mode
  }
  o.ue((cmd >> 2) & 3u);  // intra_chroma_pred_mode
  o.ue(cbp_intra_code(cbp));
  z.clear();
  if (cbp) {
    o.se(dqp);  // mb_qp_delta
    luma_residual(o, cp, cbp, z);
    chroma_residual(o, cp, cbp >> 4, z);
  }
  z.shift();
  z.left_is(modes, false, 0, 0);
}
template <class Sink>
VTS_EV void mb_intra16(Sink &o, bool islice, Row &z, uint32_t cmd, const int16_t *cp, int dqp = 0) {
  skip_run(o, islice, z);
  intra16_layer(o, islice, z, cmd, cp, dqp);
}
template <class Sink>
VTS_EV void mb_intra4(Sink &o, bool islice, Row &z, uint32_t cmd, uint64_t modes, const int16_t *cp, int dqp = 0) {
  skip_run(o, islice, z);
  intra4_layer(o, islice, z, cmd, modes, cp, dqp);
}
// I_PCM up to the samples: mb_skip_run and mb_type.  The caller writes
// pcm_alignment_zero_bits and the 384 samples, or leaves their gap.
template <class Sink>
VTS_EV void mb_pcm_head(Sink &o, bool islice, Row &z) {
  skip_run(o, islice, z);
  o.ue(islice ? 25 : 30);
  z.all(16);
  z.left_is(ei4::kNoModes, false, 0, 0);
}
// the last mb_skip_run and rbsp_slice_trailing_bits
template <class Sink>
VTS_EV void slice_end(Sink &o, Row &z) {
  if (z.skip) o.ue(z.skip);
  o.bits(1, 1);  // rbsp_stop_one_bit
  o.align();
}

#undef VTS_EV

}  // namespace ecav
}  // namespace full
}  // namespace vts
