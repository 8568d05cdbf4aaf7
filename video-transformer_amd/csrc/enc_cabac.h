// enc_cabac.h — CABAC entropy coding (9.3) of the device encoder's slices
// (transcode.hip: enc_write_cabac), written once for the
// kernel and for the CPU harness (tests/native/enc_cabac_host.cpp).
//
//   Encoder<Sink>  the arithmetic encoder of 9.3.4 (Figures 9-7 .. 9-12):
//                  InitEncoder, EncodeDecision, EncodeBypass, EncodeTerminate,
//                  EncodeFlush, PutBit with outstanding bits; its bits go into
//                  a Sink (enc_rbsp.h: ByteSink in the harness, WordSink in the
//                  kernel: RBSP bits -> EBSP bytes with emulation prevention).
//   init_contexts  9.3.1.1 from h264_cabac_tables.h: the I column or
//                  cabac_init_idc 0, the only column the device decoder reads.
//   one function per syntax element of 7.3.4 / 7.3.5 that the encoder has:
//                  values and neighbour facts -> (ctxIdx, bin) decisions;
//   mb_*           a macroblock of each kind from what a level holds about it
//                  (command word, coded_block_pattern, levels), and the
//                  neighbour facts it leaves for the next one.
//
// A slice is one macroblock row: neighbour B (above) is never available
// across macroblocks and A (left) is available from mx = 1 on.  Every
// ctxIdxInc below is therefore a function of the left macroblock's facts
// (Left) and of the macroblock's own earlier blocks; parse_cabac.h derives
// the same increments on the decoding side.
//
//   BinRing        the same interface recording the bins, drain() coding them
//                  in one loop: what the kernel uses.
//
// Every loop is bounded by the data: renormalisation takes at most 7 steps
// (range >= 6 after a decision, 2 after a terminate), the outstanding-bit run
// is written in chunks of 32 and is bounded by the bits of the slice so far,
// the Exp-Golomb suffixes by the 16-bit levels and vectors.
#pragma once
#include <cstdint>

#include "enc_deblock.h"
#include "enc_intra4.h"
#include "enc_part.h"
#include "enc_rbsp.h"
#include "h264_cabac_tables.h"

namespace vts {
namespace full {
namespace ecab {

constexpr int kNumCtx = 277;  // ctxIdx 0 .. 276: the frame-coded 4x4 syntax and end_of_slice_flag

// Staging bytes that hold any one macroblock written here:
//   context-coded bins: at most 6 bits each (rangeTabLPS >= 6: a decision
//     leaves range >= 6, six doublings reach 256), terminate bins at most 7;
//   bypass bins: 1 bit each;
//   header: mb_skip_flag 1, mb_type 7, intra_chroma_pred_mode 3,
//     coded_block_pattern 6, mb_qp_delta 1, mvd prefixes 2 x 9,
//     end_of_slice_flag 1: 37 bins, 259 bits taken at 7; the two mvd suffixes
//     and signs (|mvd| < 2^16: UEG3 of 13 + 1 + 16 bits) 64 bits;
//   residual: 27 coded_block_flags, 162 bits; 384 levels (16 + 240 + 8 + 120
//     intra, 256 + 8 + 120 inter) of significant, last, 14 prefix bins and a
//     UEG0 suffix with sign of at most 13 + 1 + 13 + 1 bits (|level| < 2^13:
//     the quantiser at qp >= 1 over 8-bit residuals), 384 (16 x 6 + 28) =
//     47616 bits;
//   together 48101 bits = 6013 bytes, and at most one emulation prevention
//   byte per two of them: 9020, rounded to 9024.  An I_PCM macroblock (its
//   mb_type, the flush, 7 alignment bits, 384 samples, end_of_slice_flag)
//   stays under 400 as before.  The slice header and the final flush fit the
//   slot's 64 spare bytes.
//   An I_NxN macroblock (mb_intra4) has no mvd but 16 x 4 mode bins: its header
//   is mb_skip_flag 1, mb_type 2, the modes 64, intra_chroma_pred_mode 3,
//   coded_block_pattern 6, mb_qp_delta 1, end_of_slice_flag 1: 78 bins, 546 bits
//   taken at 7, which is 223 more than the 323 counted above, with 26 flags for
//   27 and the same 384 levels: 48318 bits, 9060 bytes by the arithmetic above.
//   That arithmetic allows |level| < 2^13; the quantiser clamps at 2047
//   (eres::quant1), so a level's UEG0 suffix and sign take at most 10 + 1 + 10
//   + 1 bits and a level 16 x 6 + 22 = 118, not 124: 384 x 118 + 546 + 156 =
//   46014 bits = 5752 bytes, 8628 with emulation prevention.  9024 bounds it.
//   A partitioned macroblock (mb_p_part) is an inter one with up to 4
//   sub_mb_type bins and 6 more mvd (prefix 9 bins at 7 bits, suffix and sign
//   32 bits): 28 + 6 x 95 = 598 bits over the inter macroblock's 45791 of the
//   arithmetic just given, 46389 bits = 5799 bytes, 8699 with emulation
//   prevention.  9024 bounds it.
//   With adaptive quantisation (enc_aq.h) mb_qp_delta is up to 41 bins (|v| <=
//   20) where 1 is counted above: 40 x 7 = 280 bits more, 46669 bits = 5834
//   bytes, 8751 with emulation prevention.  9024 bounds it.
constexpr int kMbBytes = 9024;

#if defined(__HIPCC__)
#define VTS_ECTAB __device__ __constant__ static const
#else
#define VTS_ECTAB static const
#endif
VTS_ECTAB int8_t kInitI[VTS_CABAC_NCTX][2] = VTS_CABAC_INIT_I_DATA;
VTS_ECTAB int8_t kInitP0[VTS_CABAC_NCTX][2] = VTS_CABAC_INIT_P0_DATA;
VTS_ECTAB uint8_t kRangeLps[64][4] = VTS_CABAC_RANGE_LPS_DATA;
VTS_ECTAB uint8_t kTransLps[64] = VTS_CABAC_TRANS_LPS_DATA;
#undef VTS_ECTAB

// 9.3.1.1: the context variable of ctxIdx for SliceQPY = qp as pStateIdx << 1 | valMPS
VTS_HD VTS_INLINE uint8_t init_context(int ctx, bool islice, int qp) {
  const int m = islice ? kInitI[ctx][0] : kInitP0[ctx][0], n = islice ? kInitI[ctx][1] : kInitP0[ctx][1];
  const int q = qp < 0 ? 0 : (qp > 51 ? 51 : qp);
  int pre = ((m * q) >> 4) + n;
  pre = pre < 1 ? 1 : (pre > 126 ? 126 : pre);
  return static_cast<uint8_t>(pre <= 63 ? (63 - pre) << 1 : ((pre - 64) << 1) | 1);
}
VTS_HD inline void init_contexts(uint8_t *st, bool islice, int qp) {
  for (int i = 0; i < kNumCtx; ++i) st[i] = init_context(i, islice, qp);
}

using erbsp::ByteSink;  // the harness's sink; the kernel's is erbsp::WordSink (enc_rbsp.h)

// The slice header with entropy_coding_mode_flag = 1 and SliceQPY = qp
template <class Sink>
VTS_HD VTS_INLINE void slice_header(Sink &o, bool idr, int first_mb, int frame_num, int idr_pic_id, int qp, bool dbk,
                                    int dbk_alpha, int dbk_beta) {
  erbsp::slice_header(o, true, idr, first_mb, frame_num, idr_pic_id, qp - 26, dbk, dbk_alpha, dbk_beta);
}

// 9.3.4: st holds kNumCtx context variables (LDS in the kernel).
template <class Sink>
struct Encoder {
  Sink *o;
  uint8_t *st;
  uint32_t low, range;
  int outstanding;
  bool first;

  VTS_HD void start() {  // InitEncoder (9.3.4.1), also after pcm samples (9.3.1.2)
    low = 0;
    range = 510;
    first = true;
    outstanding = 0;
  }
  VTS_HD void put_bit(uint32_t b) {  // PutBit (Figure 9-10)
    if (first) first = false;
    else o->bits(1, b);
    while (outstanding > 0) {
      const int k = outstanding < 32 ? outstanding : 32;
      o->bits(k, b ? 0u : (k == 32 ? 0xffffffffu : (1u << k) - 1u));
      outstanding -= k;
    }
  }
  VTS_HD void renorm() {  // RenormE (Figure 9-9)
    while (range < 256) {
      if (low < 256) {
        put_bit(0);
      } else if (low >= 512) {
        low -= 512;
        put_bit(1);
      } else {
        low -= 256;
        ++outstanding;
      }
      range <<= 1;
      low <<= 1;
    }
  }
  VTS_HD void decision(int ctx, int bin) {  // EncodeDecision (Figure 9-7)
    const int s = st[ctx], ps = s >> 1, mps = s & 1;
    const uint32_t lps = kRangeLps[ps][(range >> 6) & 3];
    range -= lps;
    if (bin != mps) {
      low += range;
      range = lps;
      st[ctx] = static_cast<uint8_t>((kTransLps[ps] << 1) | (ps == 0 ? 1 - mps : mps));
    } else {
      st[ctx] = static_cast<uint8_t>(((ps < 62 ? ps + 1 : 62) << 1) | mps);
    }
    renorm();
  }
  VTS_HD void bypass(int bin) {  // EncodeBypass (Figure 9-11)
    low <<= 1;
    if (bin) low += range;
    if (low >= 1024) {
      put_bit(1);
      low -= 1024;
    } else if (low < 512) {
      put_bit(0);
    } else {
      low -= 512;
      ++outstanding;
    }
  }
  // EncodeTerminate (Figure 9-12); bin 1 goes on into EncodeFlush (9.3.4.5),
  // whose last written bit is 1: rbsp_stop_one_bit at the end of a slice, and
  // before pcm_alignment_zero_bits a non-zero bit in the byte before the samples
  VTS_HD void terminate(int bin) {
    range -= 2;
    if (bin) {
      low += range;
      range = 2;
      renorm();
      put_bit((low >> 9) & 1u);
      o->bits(2, ((low >> 7) & 3u) | 1u);
    } else {
      renorm();
    }
  }
  VTS_HD void block_begin() {}  // BinRing's drain point; nothing to do when the bins are coded as they come
  VTS_HD void sync() {}
};

// The bins of a macroblock's syntax, recorded first and coded after: the
// syntax functions below reach the three bin coders from some sixty places,
// and coding each bin where it arises puts sixty copies of the coder into
// the kernel (127 000 instructions) with its state in memory between them.
// BinRing has the Encoder's interface towards those functions, stores one
// 16-bit entry per bin (bits 0..8 ctxIdx, 9 the bin, 10 bypass, 11 terminate)
// and drain() codes a run of entries in the one loop that holds the coder and
// the sink in registers.  The ring is drained where less than a block's worst
// case is free:
//   a residual block: coded_block_flag 1, significant and last 15 + 15, and
//     for each of 16 levels 14 prefix bins, a UEG0 suffix of at most 15 + 1 +
//     15 bins (|level| <= 2^15) and the sign: 31 + 16 x 46 = 767;
//   a macroblock's header: well under that (mvd of 9 + 30 + 1 bins each, two, or
//     with partitions eight and four sub_mb_type bins: 340 with the rest).
constexpr int kRingBins = 2048, kBlockBins = 768;
constexpr uint32_t kBinBypass = 1u << 10, kBinTerminate = 1u << 11;

template <class Sink>
#if defined(__HIPCC__)
__attribute__((noinline))
#endif
VTS_HD void drain(Encoder<Sink> *enc, const uint16_t *ring, int n) {
  Encoder<Sink> e = *enc;  // local copies: the loop's state stays in registers
  Sink o = *enc->o;
  e.o = &o;
  for (int i = 0; i < n; ++i) {
    const uint32_t v = ring[i];
    const int bin = static_cast<int>((v >> 9) & 1u);
    if (v & kBinBypass) e.bypass(bin);
    else if (v & kBinTerminate) e.terminate(bin);
    else e.decision(static_cast<int>(v & 511u), bin);
  }
  *enc->o = o;
  e.o = enc->o;
  *enc = e;
}

template <class Sink>
struct BinRing {
  Encoder<Sink> *enc;
  uint16_t *ring;  // kRingBins entries (LDS in the kernel)
  int n;
  VTS_HD VTS_INLINE void decision(int ctx, int bin) { ring[n++] = static_cast<uint16_t>(ctx | (bin << 9)); }
  VTS_HD VTS_INLINE void bypass(int bin) { ring[n++] = static_cast<uint16_t>(kBinBypass | (bin << 9)); }
  VTS_HD VTS_INLINE void terminate(int bin) { ring[n++] = static_cast<uint16_t>(kBinTerminate | (bin << 9)); }
  VTS_HD VTS_INLINE void sync() {  // everything recorded so far is coded
    if (n) drain(enc, ring, n);
    n = 0;
  }
  VTS_HD VTS_INLINE void block_begin() {  // room for a block's or a header's worst case, and end_of_slice_flag
    if (n > kRingBins - kBlockBins - 8) sync();
  }
  VTS_HD VTS_INLINE void start() {  // InitEncoder behind pcm samples: the caller has sync()ed before them
    enc->start();
  }
};

// the UEGk suffix, bypass bins (9.3.2.3)
template <class E>
VTS_HD inline void exp_golomb(E &e, uint32_t v, int k) {
  while (v >= (1u << k)) {
    e.bypass(1);
    v -= 1u << k;
    ++k;
  }
  e.bypass(0);
  while (k--) e.bypass(static_cast<int>((v >> k) & 1u));
}

// ------------------------------------------------------- neighbour facts
enum : int { kNone = 0, kPcm = 1, kSkip = 2, kI16 = 3, kInter = 4, kI4 = 5 };
// coded_block_flag bits of a macroblock: bit 0 Intra16x16DCLevel, 1 + raster
// luma 4x4 block, 17 + plane chroma DC, 19 + 4 plane + raster chroma AC.  A
// block whose flag is not sent has 0, which is what 9.3.3.1.1.9 assigns to an
// available neighbour without the block; I_PCM has every bit.
constexpr uint32_t kCbfAll = 0x07ffffffu;
struct Left {        // the macroblock to the left in the slice (mx = 0: kNone)
  int kind;
  int cbp;           // coded_block_pattern (Intra16x16: the one mb_type says; P_Skip 0)
  int cmode;         // intra_chroma_pred_mode (Intra16x16, I_NxN)
  int amvd[2];       // |mvd_l0| (inter that is not skipped; else 0)
  uint32_t cbf;
  uint64_t i4 = ei4::kNoModes;  // I_NxN: its Intra4x4PredModes (enc_intra4.h), else ~0
  int bmvd[2] = {0, 0};         // |mvd_l0| of its quadrant 3 (amvd: of its quadrant 1; partitions, else unread)
  bool dq = false;              // it sent a non-zero mb_qp_delta (adaptive quantisation; every `l = Left{..}` clears it)
};
VTS_HD VTS_INLINE Left left_none() { return Left{kNone, 0, 0, {0, 0}, 0, ei4::kNoModes}; }

// ------------------------------------------------------- syntax elements
// mb_skip_flag (P): ctxIdx 11 + condTermFlagA; a skipped or absent A counts 0
template <class E>
VTS_HD VTS_INLINE void mb_skip_flag(E &e, const Left &l, int skip) {
  e.decision(11 + (l.kind != kNone && l.kind != kSkip ? 1 : 0), skip);
}
// mb_type of an intra macroblock (Table 9-36): in an I slice ctxIdx 3.., bin 0
// by A (1 when available and not I_NxN); in a P slice the prefix 1 at
// ctxIdx 14 and the suffix at 17...  t = 25: I_PCM (the terminate bin 1 and
// the flush; the caller aligns, leaves the samples and calls start()), else
// Intra16x16 with prediction mode pm, chroma cc = cbp / 16, luma15 = cbp & 15 != 0
template <class E>
VTS_HD inline void mb_type_intra(E &e, bool islice, const Left &l, bool pcm, int pm, int cc, bool luma15) {
  int b;  // ctxIdx of bin 2 (luma); chroma and the mode bits follow by Table 9-39
  if (islice) {
    e.decision(3 + (l.kind != kNone && l.kind != kI4 ? 1 : 0), 1);
    b = 3 + 3;
  } else {
    e.decision(14, 1);
    e.decision(17, 1);
    b = 17 + 1;
  }
  e.terminate(pcm ? 1 : 0);
  if (pcm) return;
  e.decision(b, luma15 ? 1 : 0);
  e.decision(b + 1, cc ? 1 : 0);
  if (islice) {
    if (cc) e.decision(b + 2, cc == 2 ? 1 : 0);
    e.decision(b + 3, pm >> 1);
    e.decision(b + 4, pm & 1);
  } else {
    if (cc) e.decision(b + 1, cc == 2 ? 1 : 0);
    e.decision(b + 2, pm >> 1);
    e.decision(b + 2, pm & 1);
  }
}
// mb_type I_NxN: in an I slice the one bin 0 at ctxIdx 3 + condTermFlagA; in a
// P slice the prefix 1 at ctxIdx 14, then 0 at 17
template <class E>
VTS_HD VTS_INLINE void mb_type_i4(E &e, bool islice, const Left &l) {
  if (islice) {
    e.decision(3 + (l.kind != kNone && l.kind != kI4 ? 1 : 0), 0);
  } else {
    e.decision(14, 1);
    e.decision(17, 0);
  }
}
// prev_intra4x4_pred_mode_flag at ctxIdx 68, then rem_intra4x4_pred_mode as
// three bins at 69, least significant first
template <class E>
VTS_HD VTS_INLINE void intra4_pred_mode(E &e, int mode, int pred) {
  e.decision(68, mode == pred);
  if (mode == pred) return;
  const int rem = ei4::rem_mode(mode, pred);
  e.decision(69, rem & 1);
  e.decision(69, (rem >> 1) & 1);
  e.decision(69, (rem >> 2) & 1);
}
// mb_type P_L0_16x16: bins 0 0 0 at ctxIdx 14, 15, 16
template <class E>
VTS_HD VTS_INLINE void mb_type_p16x16(E &e) {
  e.decision(14, 0);
  e.decision(15, 0);
  e.decision(16, 0);
}
// intra_chroma_pred_mode: TU cMax 3, ctxIdx 64 + condTermFlagA, then 67
template <class E>
VTS_HD VTS_INLINE void intra_chroma_pred_mode(E &e, const Left &l, int mode) {
  e.decision(64 + ((l.kind == kI16 || l.kind == kI4) && l.cmode != 0 ? 1 : 0), mode > 0);
  if (mode > 0) {
    e.decision(67, mode > 1);
    if (mode > 1) e.decision(67, mode > 2);
  }
}
// mvd_l0 component (base 40 x / 47 y): UEG3, signedValFlag 1, uCoff 9; bin 0
// by the sum of the neighbours' |mvd|, which is A's alone
template <class E>
VTS_HD inline void mvd(E &e, int base, int sum, int v) {
  const int a = v < 0 ? -v : v;
  e.decision(base + (sum < 3 ? 0 : (sum > 32 ? 2 : 1)), a > 0);
  if (!a) return;
  const int pre = a < 9 ? a : 9;
  for (int i = 1; i < pre; ++i) e.decision(base + (i + 2 < 6 ? i + 2 : 6), 1);
  if (a < 9) e.decision(base + (a + 2 < 6 ? a + 2 : 6), 0);
  else exp_golomb(e, static_cast<uint32_t>(a - 9), 3);
  e.bypass(v < 0);
}
// coded_block_pattern: four luma bins at 73 + condTermFlagA + 2 condTermFlagB
// (0 for a neighbouring 8x8 with its bit set, for I_PCM and for an absent
// macroblock; 1 otherwise, P_Skip included), chroma at 77 .. 84
template <class E>
VTS_HD inline void coded_block_pattern(E &e, const Left &l, int cbp) {
  const bool la = l.kind != kNone && l.kind != kPcm;
  for (int b8 = 0; b8 < 4; ++b8) {
    int ca, cb;
    if (b8 & 1) ca = !((cbp >> (b8 - 1)) & 1);
    else ca = la && !((l.cbp >> (b8 + 1)) & 1);
    cb = b8 >= 2 ? !((cbp >> (b8 - 2)) & 1) : 0;
    e.decision(73 + ca + 2 * cb, (cbp >> b8) & 1);
  }
  const int cc = cbp >> 4, lc = l.kind == kPcm ? 2 : ((l.kind == kI16 || l.kind == kI4 || l.kind == kInter) ? l.cbp >> 4 : 0);
  e.decision(77 + (lc != 0 ? 1 : 0), cc != 0);
  if (cc) e.decision(81 + (lc == 2 ? 1 : 0), cc == 2);
}
// mb_qp_delta = 0: the one bin 0; the previous macroblock's delta is 0 too
template <class E>
VTS_HD VTS_INLINE void mb_qp_delta0(E &e) {
  e.decision(60, 0);
}
// mb_qp_delta of any value (adaptive quantisation, enc_aq.h): the unary code of
// the mapped value (9.3.2.7: 2 v - 1 for v > 0, else -2 v), bin 0 at ctxIdx 60 +
// inc (inc: the previous macroblock of the slice sent a non-zero delta,
// 9.3.3.1.1.5), bin 1 at 62, every later bin at 63.  |v| <= 20: at most 41 bins.
template <class E>
VTS_HD inline void mb_qp_delta(E &e, int inc, int v) {
  const int m = v > 0 ? 2 * v - 1 : -2 * v;
  e.decision(60 + inc, m > 0);
  if (!m) return;
  e.decision(62, m > 1);
  for (int i = 2; i <= m; ++i) e.decision(63, i < m);
}
// residual_block_cabac (7.3.5.3.3) of lv[0 .. n) in scan order, ctxBlockCat
// cat: 0 Intra16x16DCLevel, 1 Intra16x16ACLevel, 2 LumaLevel4x4, 3 chroma DC,
// 4 chroma AC.  inc: transBlockA + 2 transBlockB of coded_block_flag.
// Returns coded_block_flag.
template <class E>
VTS_HD inline int residual_block(E &e, int cat, int inc, const int16_t *lv, int n) {
  const int cbf_off = 85 + 4 * cat;
  const int sig_off = cat == 0 ? 0 : (cat == 1 ? 15 : (cat == 2 ? 29 : (cat == 3 ? 44 : 47)));
  const int abs_off = 227 + (cat == 0 ? 0 : (cat == 1 ? 10 : (cat == 2 ? 20 : (cat == 3 ? 30 : 39))));
  int last = -1;
  for (int i = 0; i < n; ++i)
    if (lv[i]) last = i;
  e.block_begin();
  e.decision(cbf_off + inc, last >= 0);
  if (last < 0) return 0;
  for (int i = 0; i < n - 1; ++i) {  // the last of n is inferred
    const int ci = cat == 3 ? (i < 2 ? i : 2) : i;
    e.decision(105 + sig_off + ci, lv[i] != 0);
    if (lv[i]) {
      e.decision(166 + sig_off + ci, i == last);
      if (i == last) break;
    }
  }
  int eq1 = 0, gt1 = 0;
  for (int i = last; i >= 0; --i) {  // coeff_abs_level_minus1 (UEG0, uCoff 14) and the sign, highest first
    const int v = lv[i];
    if (!v) continue;
    const int a = (v < 0 ? -v : v) - 1;
    e.decision(abs_off + (gt1 ? 0 : (1 + eq1 < 4 ? 1 + eq1 : 4)), a > 0);
    if (a > 0) {
      const int lim = 4 - (cat == 3 ? 1 : 0);
      const int c2 = abs_off + 5 + (gt1 < lim ? gt1 : lim);
      const int pre = a < 14 ? a : 14;
      for (int j = 1; j < pre; ++j) e.decision(c2, 1);
      if (a < 14) e.decision(c2, 0);
      else exp_golomb(e, static_cast<uint32_t>(a - 14), 0);
      ++gt1;
    } else {
      ++eq1;
    }
    e.bypass(v < 0);
  }
  return 1;
}

// ------------------------------------------------------- macroblocks
// mb_qp_delta = dqp of a macroblock whose left neighbour in the slice is l;
// the mb_* functions below note a non-zero one in the Left they leave
template <class E>
VTS_HD VTS_INLINE void send_qp_delta(E &e, const Left &l, int dqp) {
  if (dqp == 0 && !l.dq) mb_qp_delta0(e);
  else mb_qp_delta(e, l.dq ? 1 : 0, dqp);
}
// condTermFlagN of coded_block_flag for a block outside the macroblock
// (9.3.3.1.1.9): A by the left macroblock's bit, an absent macroblock by the
// current one being intra
VTS_HD VTS_INLINE int cbf_left(const Left &l, int bit, bool intra) {
  return l.kind == kNone ? (intra ? 1 : 0) : static_cast<int>((l.cbf >> bit) & 1u);
}
// luma block k (luma4x4BlkIdx) of a macroblock whose flags so far are cbf
VTS_HD VTS_INLINE int cbf_inc_luma(const Left &l, uint32_t cbf, int k, bool intra) {
  const int r = edb::raster_of_blk(k), bx = r & 3, by = r >> 2;
  const int ca = bx ? static_cast<int>((cbf >> (1 + r - 1)) & 1u) : cbf_left(l, 1 + by * 4 + 3, intra);
  const int cb = by ? static_cast<int>((cbf >> (1 + r - 4)) & 1u) : (intra ? 1 : 0);
  return ca + 2 * cb;
}
// chroma of residual() (7.3.5.3): DC when cc != 0, AC when cc == 2; cp the
// macroblock's levels (transcode.hip's layout: Cb / Cr DC at 256, AC at 264)
template <class E>
VTS_HD inline uint32_t chroma_residual(E &e, const Left &l, const int16_t *cp, int cc, bool intra, uint32_t cbf) {
  if (cc)
    for (int pl = 0; pl < 2; ++pl) {
      const int inc = cbf_left(l, 17 + pl, intra) + 2 * (intra ? 1 : 0);
      cbf |= static_cast<uint32_t>(residual_block(e, 3, inc, cp + 256 + 4 * pl, 4)) << (17 + pl);
    }
  if (cc == 2)
    for (int pl = 0; pl < 2; ++pl)
      for (int k = 0; k < 4; ++k) {
        const int bx = k & 1, by = k >> 1, bit = 19 + 4 * pl + k;
        const int ca = bx ? static_cast<int>((cbf >> (bit - 1)) & 1u) : cbf_left(l, 19 + 4 * pl + by * 2 + 1, intra);
        const int cb = by ? static_cast<int>((cbf >> (bit - 2)) & 1u) : (intra ? 1 : 0);
        cbf |= static_cast<uint32_t>(residual_block(e, 4, ca + 2 * cb, cp + 264 + 60 * pl + 15 * k, 15)) << bit;
      }
  return cbf;
}

// P_Skip: mb_skip_flag 1, end_of_slice_flag
template <class E>
VTS_HD inline void mb_skip(E &e, Left &l, bool last) {
  e.block_begin();
  mb_skip_flag(e, l, 1);
  e.terminate(last);
  l = Left{kSkip, 0, 0, {0, 0}, 0};
}
// Intra16x16 from its command word (bits 0..1 Intra16x16PredMode, 2..3
// intra_chroma_pred_mode, 4..9 coded_block_pattern) and levels (DC at 0, the
// 16 AC blocks of 15 at 16, chroma)
template <class E>
VTS_HD inline void mb_intra16(E &e, bool islice, Left &l, uint32_t cmd, const int16_t *cp, bool last, int dqp = 0) {
  const int cbp = static_cast<int>(cmd >> 4) & 63, cmode = static_cast<int>(cmd >> 2) & 3;
  e.block_begin();
  if (!islice) mb_skip_flag(e, l, 0);
  mb_type_intra(e, islice, l, false, static_cast<int>(cmd & 3u), cbp >> 4, (cbp & 15) != 0);
  intra_chroma_pred_mode(e, l, cmode);
  send_qp_delta(e, l, dqp);
  uint32_t cbf = static_cast<uint32_t>(residual_block(e, 0, cbf_left(l, 0, true) + 2, cp, 16));
  if (cbp & 15)
    for (int k = 0; k < 16; ++k)
      cbf |= static_cast<uint32_t>(residual_block(e, 1, cbf_inc_luma(l, cbf, k, true), cp + 16 + 15 * k, 15))
             << (1 + edb::raster_of_blk(k));
  cbf = chroma_residual(e, l, cp, cbp >> 4, true, cbf);
  e.terminate(last);
  l = Left{kI16, cbp, cmode, {0, 0}, cbf};
  l.dq = dqp != 0;
}
// I_NxN (Intra_4x4) from its command word (bits 2..3 intra_chroma_pred_mode,
// 4..9 coded_block_pattern), its Intra4x4PredModes and levels (the inter
// layout: 16 per luma block by luma4x4BlkIdx, chroma).  There is no
// transform_size_8x8_flag: the PPS has no 8x8 transform.  A luma block's
// coded_block_flag takes condTermFlag 1 for a neighbour outside the slice
// (intra: cbf_inc_luma), mb_qp_delta is sent only with a pattern.
template <class E>
VTS_HD inline void mb_intra4(E &e, bool islice, Left &l, uint32_t cmd, uint64_t modes, const int16_t *cp, bool last,
                             int dqp = 0) {
  const int cbp = static_cast<int>(cmd >> 4) & 63, cmode = static_cast<int>(cmd >> 2) & 3;
  e.block_begin();
  if (!islice) mb_skip_flag(e, l, 0);
  mb_type_i4(e, islice, l);
  for (int k = 0; k < 16; ++k)
    intra4_pred_mode(e, ei4::mode_at(modes, k), ei4::pred_mode_of(k, modes, l.kind != kNone, l.kind == kI4 ? l.i4 : ei4::kNoModes));
  intra_chroma_pred_mode(e, l, cmode);
  coded_block_pattern(e, l, cbp);
  uint32_t cbf = 0;
  if (cbp) {
    send_qp_delta(e, l, dqp);
    for (int k = 0; k < 16; ++k)
      if ((cbp >> (k >> 2)) & 1)
        cbf |= static_cast<uint32_t>(residual_block(e, 2, cbf_inc_luma(l, cbf, k, true), cp + 16 * k, 16))
               << (1 + edb::raster_of_blk(k));
    cbf = chroma_residual(e, l, cp, cbp >> 4, true, cbf);
  }
  e.terminate(last);
  l = Left{kI4, cbp, cmode, {0, 0}, cbf, modes};
  l.dq = cbp && dqp != 0;
}
// P_L0_16x16 with the vector difference (dx, dy), coded_block_pattern cbp and
// levels (16 per luma block by luma4x4BlkIdx, chroma)
template <class E>
VTS_HD inline void mb_inter(E &e, Left &l, int dx, int dy, int cbp, const int16_t *cp, bool last, int dqp = 0) {
  e.block_begin();
  mb_skip_flag(e, l, 0);
  mb_type_p16x16(e);
  mvd(e, 40, l.amvd[0], dx);
  mvd(e, 47, l.amvd[1], dy);
  coded_block_pattern(e, l, cbp);
  uint32_t cbf = 0;
  if (cbp) {
    send_qp_delta(e, l, dqp);
    for (int k = 0; k < 16; ++k)
      if ((cbp >> (k >> 2)) & 1)
        cbf |= static_cast<uint32_t>(residual_block(e, 2, cbf_inc_luma(l, cbf, k, false), cp + 16 * k, 16))
               << (1 + edb::raster_of_blk(k));
    cbf = chroma_residual(e, l, cp, cbp >> 4, false, cbf);
  }
  e.terminate(last);
  const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  l = Left{kInter, cbp, 0, {ax < 33 ? ax : 33, ay < 33 ? ay : 33}, cbf};
  l.bmvd[0] = l.amvd[0];
  l.bmvd[1] = l.amvd[1];
  l.dq = cbp && dqp != 0;
}
// mb_type of the partitioned P macroblocks (Table 9-37): P_L0_L0_16x8 (1) bins
// 0 1 1 at ctxIdx 14, 15, 17; P_L0_L0_8x16 (2) 0 1 0; P_8x8 (3) 0 0 1 at 14,
// 15, 16
template <class E>
VTS_HD VTS_INLINE void mb_type_p_part(E &e, int shape) {
  e.decision(14, 0);
  if (shape == epart::k8x8) {
    e.decision(15, 0);
    e.decision(16, 1);
  } else {
    e.decision(15, 1);
    e.decision(17, shape == epart::k16x8);
  }
}
// A partitioned macroblock (enc_part.h) of `shape` with the quadrant vectors
// mv4 (words); lmv: the left macroblock's vectors for epart::pred_block.
// mb_type, for P_8x8 four sub_mb_type P_L0_8x8 (the one bin 1 at ctxIdx 21),
// the mvds in syntax order, then as mb_inter.  ctxIdxInc of an mvd's first bin
// is by |mvd| of A plus |mvd| of B (9.3.3.1.1.7): B lies in another slice (0)
// for the upper blocks and inside the macroblock for the lower ones, A is the
// left macroblock's right column (its quadrant 1 or 3) or the block to the
// left inside the macroblock.
template <class E>
VTS_HD inline void mb_p_part(E &e, Left &l, int shape, const uint32_t *mv4, const epart::Left &lmv, int cbp,
                             const int16_t *cp, bool last, int dqp = 0) {
  epart::Mv q[4];
  for (int i = 0; i < 4; ++i) q[i] = epart::mv_of_word(mv4[i]);
  e.block_begin();
  mb_skip_flag(e, l, 0);
  mb_type_p_part(e, shape);
  if (shape == epart::k8x8)
    for (int i = 0; i < 4; ++i) e.decision(21, 1);
  int cur[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};  // |mvd| by quadrant
  for (int part = 0; part < epart::shape_blocks(shape); ++part) {
    const int fq = epart::part_quad(shape, part), mask = epart::block_quads(epart::shape_first(shape) + part);
    const epart::Mv p = epart::pred_block(shape, part, q, lmv);
    const int d[2] = {q[fq].x - p.x, q[fq].y - p.y};
    for (int c = 0; c < 2; ++c) {
      const int a = (fq & 1) ? cur[fq - 1][c] : (fq == 0 ? l.amvd[c] : l.bmvd[c]);
      const int b = fq >= 2 ? cur[fq - 2][c] : 0;
      mvd(e, c ? 47 : 40, a + b, d[c]);
    }
    for (int i = 0; i < 4; ++i)
      if ((mask >> i) & 1)
        for (int c = 0; c < 2; ++c) {
          const int a = d[c] < 0 ? -d[c] : d[c];
          cur[i][c] = a < 33 ? a : 33;
        }
  }
  coded_block_pattern(e, l, cbp);
  uint32_t cbf = 0;
  if (cbp) {
    send_qp_delta(e, l, dqp);
    for (int k = 0; k < 16; ++k)
      if ((cbp >> (k >> 2)) & 1)
        cbf |= static_cast<uint32_t>(residual_block(e, 2, cbf_inc_luma(l, cbf, k, false), cp + 16 * k, 16))
               << (1 + edb::raster_of_blk(k));
    cbf = chroma_residual(e, l, cp, cbp >> 4, false, cbf);
  }
  e.terminate(last);
  l = Left{kInter, cbp, 0, {cur[1][0], cur[1][1]}, cbf};
  l.bmvd[0] = cur[3][0];
  l.bmvd[1] = cur[3][1];
  l.dq = cbp && dqp != 0;
}
// I_PCM up to the samples: mb_type through the terminate bin and the flush.
// The caller writes pcm_alignment_zero_bits and the 384 samples (or leaves
// their gap), then calls mb_pcm_end.
template <class E>
VTS_HD inline void mb_pcm_begin(E &e, bool islice, const Left &l) {
  e.block_begin();
  if (!islice) mb_skip_flag(e, l, 0);
  mb_type_intra(e, islice, l, true, 0, 0, false);
  e.sync();  // the sink is the caller's until mb_pcm_end
}
// the arithmetic encoder restarts behind the samples (9.3.1.2), the contexts
// stay; end_of_slice_flag
template <class E>
VTS_HD inline void mb_pcm_end(E &e, Left &l, bool last) {
  e.start();
  e.terminate(last);
  l = Left{kPcm, 0x2f, 0, {0, 0}, kCbfAll};
}

}  // namespace ecab
}  // namespace full
}  // namespace vts
