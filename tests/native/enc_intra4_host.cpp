// CPU harness of the device encoder's Intra_4x4 path (enc_intra4.h, the header
// enc_intra<true> and both slice writers call; enc_cabac.h's mb_intra4):
//   ei4h_block:     availability, allowed modes and the nine predictions of one
//                   block over a given tile;
//   ei4h_pred_mode: predIntra4x4PredMode; ei4h_key: the mode key;
//   ei4h_encode:    pictures of seeded macroblock kinds (I_PCM, Intra16x16,
//                   I_NxN, P_Skip, coded inter at vector (0, 0), or the
//                   encoder's own choice between the intra kinds) coded
//                   serially with the headers' arithmetic: command words,
//                   patterns, levels, mode words, the two candidates' bits and
//                   the reconstruction;
//   ei4h_write:     those pictures as slices, one per macroblock row: CAVLC by
//                   the writer below, which restates enc_write's syntax, or
//                   CABAC through enc_cabac.h, directly or through BinRing.
// TEST INFRASTRUCTURE (tests/test_enc_intra4_host.py; enc_intra4_main.cpp runs
// the same functions under the sanitizers).
#include <cstdint>
#include <cstring>
#include <vector>

#include "enc_cabac.h"
#include "enc_intra4.h"
#include "enc_residual.h"
#include "h264.h"
#include "h264_tables.h"

using namespace vts;
namespace ecab = vts::full::ecab;
namespace edb = vts::full::edb;
namespace ei4 = vts::full::ei4;
namespace eres = vts::full::eres;

namespace {
constexpr int kCoefPerMb = 384;  // transcode.hip's level layout
constexpr int kPcmBits = 3072;
const uint8_t kCtLen[4][17][4] = VTS_CT_LEN_DATA;
const uint8_t kCtCode[4][17][4] = VTS_CT_CODE_DATA;
const uint8_t kTzLen[15][16] = VTS_TZ_LEN_DATA;
const uint8_t kTzCode[15][16] = VTS_TZ_CODE_DATA;
const uint8_t kTzcLen[3][4] = VTS_TZC_LEN_DATA;
const uint8_t kTzcCode[3][4] = VTS_TZC_CODE_DATA;
const uint8_t kRbLen[7][15] = VTS_RB_LEN_DATA;
const uint8_t kRbCode[7][15] = VTS_RB_CODE_DATA;
const uint8_t kCbpInterTab[48] = VTS_CBPP_DATA;
const uint8_t kCbpIntraTab[48] = VTS_CBPI_DATA;
const uint8_t kQpc[52] = VTS_QPC_DATA;
const uint8_t kZz[16] = VTS_ZZ_DATA;

using Sink = ecab::ByteSink;
// RBSP bits counted, nothing stored
struct BitCount {
  int64_t n = 0;
  void bits(int k, uint32_t) { n += k; }
  void ue(uint32_t v) { n += 2 * (31 - __builtin_clz(v + 1)) + 1; }
  void se(int v) { ue(v > 0 ? static_cast<uint32_t>(2 * v - 1) : static_cast<uint32_t>(-2 * v)); }
};

// residual_block_cavlc (7.3.5.3.2, 9.2) of lv[0 .. maxNum) in scan order; returns total_coeff
template <class S>
int cavlc_block(S &o, const int16_t *lv, int maxNum, int nC) {
  int tc = 0, t1 = 0, top = -1;
  bool open = true;
  for (int i = maxNum - 1; i >= 0; --i) {
    const int v = lv[i];
    if (!v) continue;
    if (top < 0) top = i;
    ++tc;
    if (open && t1 < 3 && (v == 1 || v == -1)) ++t1;
    else open = false;
  }
  if (nC >= 8) {
    o.bits(6, tc == 0 ? 3u : static_cast<uint32_t>(((tc - 1) << 2) | t1));
  } else {
    const int col = nC == -1 ? 3 : (nC < 2 ? 0 : (nC < 4 ? 1 : 2));
    o.bits(kCtLen[col][tc][t1], kCtCode[col][tc][t1]);
  }
  if (!tc) return 0;
  int k = 0, sl = (tc > 10 && t1 < 3) ? 1 : 0;
  for (int i = maxNum - 1; i >= 0; --i) {
    const int v = lv[i];
    if (!v) continue;
    if (k < t1) {
      o.bits(1, v < 0 ? 1u : 0u);
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
      o.bits(prefix + 1, 1u);
      if (ssize) o.bits(ssize, static_cast<uint32_t>(suffix));
      if (sl == 0) sl = 1;
      if ((v < 0 ? -v : v) > (3 << (sl - 1)) && sl < 6) ++sl;
    }
    ++k;
  }
  int zl = top + 1 - tc;
  if (tc < maxNum) o.bits(maxNum == 4 ? kTzcLen[tc - 1][zl] : kTzLen[tc - 1][zl],
                          maxNum == 4 ? kTzcCode[tc - 1][zl] : kTzCode[tc - 1][zl]);
  int prev = -1;
  for (int i = maxNum - 1; i >= 0; --i) {
    if (!lv[i]) continue;
    if (prev >= 0 && zl > 0) {
      const int run = prev - i - 1, row = (zl < 7 ? zl : 7) - 1;
      o.bits(kRbLen[row][run], kRbCode[row][run]);
      zl -= run;
    }
    prev = i;
  }
  return tc;
}
int nc_of(int na, int nb) { return (na >= 0 && nb >= 0) ? (na + nb + 1) >> 1 : (na >= 0 ? na : (nb >= 0 ? nb : 0)); }

// What a slice's CAVLC writer carries from macroblock to macroblock: total_coeff of the left macroblock's
// right column (-1: none), and the left macroblock's mode word when it is I_NxN
struct Row {
  int l[4], lc[2][2], c[16], cc[2][4];
  uint64_t left_modes;
  bool has_left;
  void start() {
    for (int i = 0; i < 4; ++i) l[i] = -1;
    lc[0][0] = lc[0][1] = lc[1][0] = lc[1][1] = -1;
    left_modes = ei4::kNoModes;
    has_left = false;
  }
  void all(int v) {
    for (int i = 0; i < 4; ++i) l[i] = v;
    lc[0][0] = lc[0][1] = lc[1][0] = lc[1][1] = v;
  }
  void clear() {
    std::memset(c, 0, sizeof c);
    std::memset(cc, 0, sizeof cc);
  }
  void shift() {
    for (int i = 0; i < 4; ++i) l[i] = c[i * 4 + 3];
    for (int pl = 0; pl < 2; ++pl) {
      lc[pl][0] = cc[pl][1];
      lc[pl][1] = cc[pl][3];
    }
  }
};
template <class S>
void cavlc_chroma(S &o, const int16_t *cp, int cc, Row &z) {
  if (cc)
    for (int pl = 0; pl < 2; ++pl) cavlc_block(o, cp + 256 + 4 * pl, 4, -1);
  if (cc == 2)
    for (int pl = 0; pl < 2; ++pl)
      for (int k = 0; k < 4; ++k) {
        const int bx = k & 1, by = k >> 1;
        const int na = bx ? z.cc[pl][by * 2] : z.lc[pl][by], nb = by ? z.cc[pl][bx] : -1;
        z.cc[pl][k] = cavlc_block(o, cp + 264 + 60 * pl + 15 * k, 15, nc_of(na, nb));
      }
}
template <class S>
void cavlc_luma(S &o, const int16_t *lv, int n, int k, Row &z) {
  const int r = edb::raster_of_blk(k), bx = r & 3, by = r >> 2;
  const int na = bx ? z.c[r - 1] : z.l[by], nb = by ? z.c[r - 4] : -1;
  z.c[r] = cavlc_block(o, lv, n, nc_of(na, nb));
}

// macroblock_layer() (7.3.5) of an intra macroblock that is not I_PCM, from mb_type on, as enc_write writes
// it; z is left as the macroblock to the right finds it
template <class S>
void cavlc_intra_mb(S &o, bool idr, uint32_t c, uint64_t modes, const int16_t *cp, Row &z) {
  const int cbp = static_cast<int>(c >> 4) & 63;
  z.clear();
  if (ei4::is_i4_cmd(c)) {  // I_NxN
    o.ue(idr ? 0 : 5);
    for (int k = 0; k < 16; ++k) {
      const int m = ei4::mode_at(modes, k), pm = ei4::pred_mode_of(k, modes, z.has_left, z.left_modes);
      if (m == pm) o.bits(1, 1);
      else o.bits(4, static_cast<uint32_t>(ei4::rem_mode(m, pm)));
    }
    o.ue((c >> 2) & 3u);
    uint32_t code = 0;
    while (kCbpIntraTab[code] != cbp) ++code;
    o.ue(code);
    if (cbp) {
      o.se(0);
      for (int k = 0; k < 16; ++k)
        if ((cbp >> (k >> 2)) & 1) cavlc_luma(o, cp + 16 * k, 16, k, z);
      cavlc_chroma(o, cp, cbp >> 4, z);
    }
    z.left_modes = modes;
  } else {  // Intra16x16
    const uint32_t mbt = 1 + (c & 3u) + 4 * static_cast<uint32_t>(cbp >> 4) + ((cbp & 15) ? 12 : 0);
    o.ue(idr ? mbt : 5 + mbt);
    o.ue((c >> 2) & 3u);
    o.se(0);
    cavlc_block(o, cp, 16, nc_of(z.l[0], -1));
    if (cbp & 15)
      for (int k = 0; k < 16; ++k) cavlc_luma(o, cp + 16 + 15 * k, 15, k, z);
    cavlc_chroma(o, cp, cbp >> 4, z);
    z.left_modes = ei4::kNoModes;
  }
  z.shift();
  z.has_left = true;
}

// one slice (macroblock row) as CAVLC: what enc_write writes
void cavlc_row(Sink &o, bool idr, int row, int mbw, int frame_num, int qp, const uint32_t *cmd, const uint8_t *cbp_row,
               const int16_t *coef, const uint64_t *modes, const uint8_t *pcm) {
  o.put(idr ? 0x65 : 0x41);
  o.ue(static_cast<uint32_t>(row * mbw));
  o.ue(idr ? 7 : 5);
  o.ue(0);
  o.bits(16, static_cast<uint32_t>(frame_num));
  if (idr) {
    o.ue(0);
    o.bits(2, 0);
  } else {
    o.bits(3, 0);
  }
  o.se(qp - 26);
  o.ue(1);
  Row z;
  z.start();
  uint32_t skip = 0;
  for (int mx = 0; mx < mbw; ++mx) {
    const uint32_t c = cmd[mx];
    const int16_t *cp = coef + static_cast<int64_t>(mx) * kCoefPerMb;
    if (c == edb::kPcmCmd || edb::is_intra_cmd(c)) {
      if (!idr) {
        o.ue(skip);
        skip = 0;
      }
      if (c == edb::kPcmCmd) {
        o.ue(idr ? 25 : 30);
        o.align();
        for (int i = 0; i < 384; ++i) o.byte(pcm[384 * mx + i]);
        z.all(16);
        z.left_modes = ei4::kNoModes;
        z.has_left = true;
      } else {
        cavlc_intra_mb(o, idr, c, modes[mx], cp, z);
      }
      continue;
    }
    const int cbp = cbp_row[mx];  // the harness codes vector (0, 0) only: mvd is 0 whatever the predictor
    if (cbp == 0) {
      ++skip;
      z.all(0);
    } else {
      o.ue(skip);
      skip = 0;
      o.ue(0);
      o.se(0);
      o.se(0);
      int code = 0;
      while (kCbpInterTab[code] != cbp) ++code;
      o.ue(static_cast<uint32_t>(code));
      z.clear();
      o.se(0);
      for (int k = 0; k < 16; ++k)
        if ((cbp >> (k >> 2)) & 1) cavlc_luma(o, cp + 16 * k, 16, k, z);
      cavlc_chroma(o, cp, cbp >> 4, z);
      z.shift();
    }
    z.left_modes = ei4::kNoModes;
    z.has_left = true;
  }
  if (skip) o.ue(skip);
  o.bits(1, 1);
  o.align();
}

// the same slice through enc_cabac.h, in the order enc_write_cabac walks it
template <class E>
void cabac_mbs(E &e, Sink &o, bool idr, int mbw, const uint32_t *cmd, const uint8_t *cbp_row, const int16_t *coef,
               const uint64_t *modes, const uint8_t *pcm) {
  ecab::Left l = ecab::left_none();
  for (int mx = 0; mx < mbw; ++mx) {
    const uint32_t c = cmd[mx];
    const int16_t *cp = coef + static_cast<int64_t>(mx) * kCoefPerMb;
    const bool last = mx == mbw - 1;
    if (c == edb::kPcmCmd) {
      ecab::mb_pcm_begin(e, idr, l);
      o.align();
      for (int i = 0; i < 384; ++i) o.byte(pcm[384 * mx + i]);
      ecab::mb_pcm_end(e, l, last);
    } else if (ei4::is_i4_cmd(c)) {
      ecab::mb_intra4(e, idr, l, c, modes[mx], cp, last);
    } else if (edb::is_intra_cmd(c)) {
      ecab::mb_intra16(e, idr, l, c, cp, last);
    } else if (cbp_row[mx] == 0) {
      ecab::mb_skip(e, l, last);
    } else {
      ecab::mb_inter(e, l, 0, 0, cbp_row[mx], cp, last);
    }
  }
  e.sync();
}
void cabac_row(Sink &o, bool ring, bool idr, int row, int mbw, int frame_num, int qp, const uint32_t *cmd,
               const uint8_t *cbp_row, const int16_t *coef, const uint64_t *modes, const uint8_t *pcm) {
  ecab::slice_header(o, idr, row * mbw, frame_num, 0, qp, false, 0, 0);
  uint8_t st[ecab::kNumCtx];
  ecab::init_contexts(st, idr, qp);
  ecab::Encoder<Sink> e{&o, st, 0, 0, 0, false};
  e.start();
  if (ring) {
    std::vector<uint16_t> bins(ecab::kRingBins);
    ecab::BinRing<Sink> r{&e, bins.data(), 0};
    cabac_mbs(r, o, idr, mbw, cmd, cbp_row, coef, modes, pcm);
  } else {
    cabac_mbs(e, o, idr, mbw, cmd, cbp_row, coef, modes, pcm);
  }
  o.align();
}

// ------------------------------------------------------------ the encoder
// A macroblock's samples out of / into an NV12 picture [H * 3 / 2][W]
struct MbPix {
  uint8_t y[16][16], c[2][8][8];
};
void load_mb(const uint8_t *pic, int W, int H, int mx, int my, MbPix &p) {
  for (int r = 0; r < 16; ++r) std::memcpy(p.y[r], pic + static_cast<int64_t>(my * 16 + r) * W + mx * 16, 16);
  for (int r = 0; r < 8; ++r)
    for (int x = 0; x < 8; ++x)
      for (int pl = 0; pl < 2; ++pl) p.c[pl][r][x] = pic[static_cast<int64_t>(H + my * 8 + r) * W + 2 * (mx * 8 + x) + pl];
}
void store_mb(uint8_t *pic, int W, int H, int mx, int my, const MbPix &p) {
  for (int r = 0; r < 16; ++r) std::memcpy(pic + static_cast<int64_t>(my * 16 + r) * W + mx * 16, p.y[r], 16);
  for (int r = 0; r < 8; ++r)
    for (int x = 0; x < 8; ++x)
      for (int pl = 0; pl < 2; ++pl) pic[static_cast<int64_t>(H + my * 8 + r) * W + 2 * (mx * 8 + x) + pl] = p.c[pl][r][x];
}

// chroma of a macroblock against prediction pc: levels into cp (DC at 256, AC at 264), the reconstruction
// into rec; returns coded_block_pattern / 16
int code_chroma(const MbPix &src, const uint8_t (*pc)[8][8], int qpc, int16_t *cp, MbPix &rec) {
  int z[2][4][16], dcl[2][4];
  bool acnz = false, dcnz = false;
  for (int pl = 0; pl < 2; ++pl) {
    int dcw[4];
    for (int k = 0; k < 4; ++k) {
      int x[16], lv[16];
      for (int i = 0; i < 16; ++i) x[i] = src.c[pl][(k >> 1) * 4 + (i >> 2)][(k & 1) * 4 + (i & 3)] - pc[pl][(k >> 1) * 4 + (i >> 2)][(k & 1) * 4 + (i & 3)];
      acnz |= eres::code_block<true>(x, qpc, z[pl][k], lv, &dcw[k]);
      for (int q = 0; q < 15; ++q) cp[264 + 60 * pl + 15 * k + q] = static_cast<int16_t>(lv[q]);
    }
    dcnz |= eres::code_chroma_dc(dcw, qpc, dcl[pl]);
    for (int q = 0; q < 4; ++q) cp[256 + 4 * pl + q] = static_cast<int16_t>(dcl[pl][q]);
  }
  const int cc = acnz ? 2 : (dcnz ? 1 : 0);
  for (int pl = 0; pl < 2; ++pl)
    for (int k = 0; k < 4; ++k) {
      int res[16];
      eres::chroma_residual(dcl[pl], k, z[pl][k], cc == 2, qpc, res);
      for (int i = 0; i < 16; ++i) {
        const int r = (k >> 1) * 4 + (i >> 2), x = (k & 1) * 4 + (i & 3);
        rec.c[pl][r][x] = static_cast<uint8_t>(full::clip1(pc[pl][r][x] + res[i]));
      }
    }
  return cc;
}

uint32_t pack4(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | (static_cast<uint32_t>(p[3]) << 24); }

struct Enc {
  int mbw, mbh, W, H, qp;
  uint32_t *cmd;
  uint8_t *cbp;
  int16_t *coef;
  uint64_t *modes;
  int32_t *bits;  // per macroblock: the Intra16x16 and the I_NxN candidates' bits (0: not computed)
};

// one intra macroblock: Intra16x16 (want 1), I_NxN (2) or the encoder's rule (5); z: the slice's writer state
// before the macroblock, advanced as the writer will
void intra_mb(const Enc &E, bool idr, int want, int mx, int64_t mbi, const MbPix &src, const uint8_t *left_y,
              const uint8_t (*left_c)[8], Row &z, MbPix &rec) {
  const int qp = E.qp, qpc = kQpc[qp];
  int16_t *cp = E.coef + mbi * kCoefPerMb;
  // ---- chroma and the Intra16x16 luma mode by SAD, as enc_intra decides them
  int lmode = 2, cmode = 0, dcy = 128;
  uint8_t pc[2][8][8];
  int dcc[2][2] = {{128, 128}, {128, 128}};
  if (mx > 0) {
    int s = 0;
    for (int i = 0; i < 16; ++i) s += left_y[i];
    dcy = (s + 8) >> 4;
    for (int pl = 0; pl < 2; ++pl)
      for (int h = 0; h < 2; ++h) dcc[pl][h] = (left_c[pl][4 * h] + left_c[pl][4 * h + 1] + left_c[pl][4 * h + 2] + left_c[pl][4 * h + 3] + 2) >> 2;
    int sh = 0, sd = 0, cd = 0, chh = 0;
    for (int r = 0; r < 16; ++r)
      for (int x = 0; x < 16; ++x) {
        sh += std::abs(src.y[r][x] - left_y[r]);
        sd += std::abs(src.y[r][x] - dcy);
      }
    for (int pl = 0; pl < 2; ++pl)
      for (int r = 0; r < 8; ++r)
        for (int x = 0; x < 8; ++x) {
          cd += std::abs(src.c[pl][r][x] - dcc[pl][r >> 2]);
          chh += std::abs(src.c[pl][r][x] - left_c[pl][r]);
        }
    lmode = sh <= sd ? 1 : 2;
    cmode = cd <= chh ? 0 : 1;
  }
  for (int pl = 0; pl < 2; ++pl)
    for (int r = 0; r < 8; ++r)
      for (int x = 0; x < 8; ++x) pc[pl][r][x] = static_cast<uint8_t>(cmode == 1 ? left_c[pl][r] : dcc[pl][r >> 2]);
  int16_t c16[kCoefPerMb] = {0}, c4[kCoefPerMb] = {0};
  MbPix r16 = {}, r4 = {};
  const int cc = code_chroma(src, pc, qpc, c16, r16);
  std::memcpy(c4 + 256, c16 + 256, 128 * sizeof(int16_t));
  std::memcpy(r4.c, r16.c, sizeof r4.c);
  // ---- the Intra16x16 candidate
  int cbp16;
  {
    int zb[16][16], dcw[16], lev[16], sc[16];
    bool ac = false;
    for (int k = 0; k < 16; ++k) {
      const int r = edb::raster_of_blk(k), bx = r & 3, by = r >> 2;
      int x[16], lv[16];
      for (int i = 0; i < 16; ++i) x[i] = src.y[by * 4 + (i >> 2)][bx * 4 + (i & 3)] - (lmode == 1 ? left_y[by * 4 + (i >> 2)] : dcy);
      ac |= eres::code_block<true>(x, qp, zb[k], lv, &dcw[r]);
      for (int q = 0; q < 15; ++q) c16[16 + 15 * k + q] = static_cast<int16_t>(lv[q]);
    }
    eres::code_i16_dc(dcw, qp, lev);
    full::i16_dc_inverse(lev, qp, full::level_scale(qp % 6, 0, 0), sc);
    for (int q = 0; q < 16; ++q) c16[q] = static_cast<int16_t>(lev[kZz[q]]);
    for (int k = 0; k < 16; ++k) {
      const int r = edb::raster_of_blk(k), bx = r & 3, by = r >> 2;
      int res[16];
      eres::residual_dc_done(sc[r], zb[k], ac, qp, res);
      for (int i = 0; i < 16; ++i)
        r16.y[by * 4 + (i >> 2)][bx * 4 + (i & 3)] =
            static_cast<uint8_t>(full::clip1((lmode == 1 ? left_y[by * 4 + (i >> 2)] : dcy) + res[i]));
    }
    cbp16 = (ac ? 15 : 0) | (cc << 4);
  }
  const uint32_t cmd16 = edb::kIntraCmd | static_cast<uint32_t>(lmode | (cmode << 2) | (cbp16 << 4));
  // ---- the I_NxN candidate, block by block over the tile
  uint64_t word = 0;
  int cbp4 = cc << 4;
  {
    uint8_t tile[16 * ei4::kTilePitch] = {0};
    for (int r = 0; r < 16; ++r) tile[r * ei4::kTilePitch + 3] = mx > 0 ? left_y[r] : 0;
    for (int k = 0; k < 16; ++k) {
      const int r = edb::raster_of_blk(k), bx = r & 3, by = r >> 2;
      const ei4::Avail av = ei4::avail_of(k, mx > 0);
      const uint32_t allowed = ei4::allowed_modes(av);
      const int pm = ei4::pred_mode_of(k, word, mx > 0, z.left_modes);
      int T[9], L[5];
      ei4::neighbours(tile, k, av, T, L);
      uint64_t best = ~0ull;
      for (int m = 0; m < 9; ++m) {
        if (!((allowed >> m) & 1u)) continue;
        uint32_t sad = 0;
        for (int y = 0; y < 4; ++y) sad += ei4::sad_row4(ei4::pred_row(m, y, T, L, av), pack4(&src.y[by * 4 + y][bx * 4]));
        const uint64_t key = ei4::mode_key(sad, qp, m, pm);
        best = key < best ? key : best;
      }
      const int m = ei4::key_mode(best);
      word |= static_cast<uint64_t>(m) << (4 * k);
      int x[16], zq[16], lv[16], res[16];
      uint32_t pr[4];
      for (int y = 0; y < 4; ++y) {
        pr[y] = ei4::pred_row(m, y, T, L, av);
        eres::diff_row4(pack4(&src.y[by * 4 + y][bx * 4]), pr[y], x + 4 * y);
      }
      if (eres::code_block<false>(x, qp, zq, lv, nullptr)) cbp4 |= 1 << (k >> 2);
      full::scale_idct4(zq, qp, false, res);
      for (int y = 0; y < 4; ++y) {
        const uint32_t o = eres::recon_row4(pr[y], res + 4 * y);
        for (int c = 0; c < 4; ++c) tile[(by * 4 + y) * ei4::kTilePitch + 4 + bx * 4 + c] = static_cast<uint8_t>(o >> (8 * c));
      }
      for (int q = 0; q < 16; ++q) c4[16 * k + q] = static_cast<int16_t>(lv[q]);
    }
    for (int r = 0; r < 16; ++r) std::memcpy(r4.y[r], tile + r * ei4::kTilePitch + 4, 16);
  }
  const uint32_t cmd4 = ei4::kI4Cmd | static_cast<uint32_t>((cmode << 2) | (cbp4 << 4));
  // ---- the bits of both with the writer's own contexts, and the choice
  Row z16 = z, z4 = z;
  BitCount b16, b4;
  cavlc_intra_mb(b16, idr, cmd16, ei4::kNoModes, c16, z16);
  cavlc_intra_mb(b4, idr, cmd4, word, c4, z4);
  E.bits[2 * mbi] = static_cast<int32_t>(b16.n);
  E.bits[2 * mbi + 1] = static_cast<int32_t>(b4.n);
  const bool use4 = want == 2 || (want == 5 && b4.n < b16.n);
  const int64_t nb = use4 ? b4.n : b16.n;
  if (want == 5 && nb > kPcmBits) {  // stays I_PCM
    E.cmd[mbi] = edb::kPcmCmd;
    E.cbp[mbi] = 0;
    E.modes[mbi] = ei4::kNoModes;
    rec = src;
    z.all(16);
    z.left_modes = ei4::kNoModes;
    z.has_left = true;
    return;
  }
  E.cmd[mbi] = use4 ? cmd4 : cmd16;
  E.cbp[mbi] = static_cast<uint8_t>(use4 ? cbp4 : cbp16);
  E.modes[mbi] = use4 ? word : ei4::kNoModes;
  std::memcpy(cp, use4 ? c4 : c16, sizeof c16);
  rec = use4 ? r4 : r16;
  z = use4 ? z4 : z16;
}

// an inter macroblock at vector (0, 0): P_Skip (want 3: the prediction is the reconstruction) or coded
void inter_mb(const Enc &E, int want, int64_t mbi, const MbPix &src, const MbPix &ref, Row &z, MbPix &rec) {
  const int qp = E.qp, qpc = kQpc[qp];
  int16_t *cp = E.coef + mbi * kCoefPerMb;
  E.cmd[mbi] = 0;
  E.modes[mbi] = ei4::kNoModes;
  z.left_modes = ei4::kNoModes;
  z.has_left = true;
  int cbp = 0;
  if (want != 3) {
    for (int k = 0; k < 16; ++k) {
      const int r = edb::raster_of_blk(k), bx = r & 3, by = r >> 2;
      int x[16], zq[16], lv[16], res[16];
      for (int i = 0; i < 16; ++i) x[i] = src.y[by * 4 + (i >> 2)][bx * 4 + (i & 3)] - ref.y[by * 4 + (i >> 2)][bx * 4 + (i & 3)];
      if (eres::code_block<false>(x, qp, zq, lv, nullptr)) cbp |= 1 << (k >> 2);
      full::scale_idct4(zq, qp, false, res);
      for (int i = 0; i < 16; ++i)
        rec.y[by * 4 + (i >> 2)][bx * 4 + (i & 3)] = static_cast<uint8_t>(full::clip1(ref.y[by * 4 + (i >> 2)][bx * 4 + (i & 3)] + res[i]));
      for (int q = 0; q < 16; ++q) cp[16 * k + q] = static_cast<int16_t>(lv[q]);
    }
    cbp |= code_chroma(src, ref.c, qpc, cp, rec) << 4;
  }
  E.cbp[mbi] = static_cast<uint8_t>(cbp);
  if (cbp == 0) {  // P_Skip
    rec = ref;
    z.all(0);
    return;
  }
  // the writer's total_coeff bookkeeping, for the intra macroblocks to the right
  BitCount b;
  z.clear();
  for (int k = 0; k < 16; ++k)
    if ((cbp >> (k >> 2)) & 1) cavlc_luma(b, cp + 16 * k, 16, k, z);
  cavlc_chroma(b, cp, cbp >> 4, z);
  z.shift();
}
}  // namespace

// Block k over `tile` (16 rows of 20 bytes, enc_intra4.h): avail[4] = left, top, top-left, top-right;
// pred[m][16] the prediction of every mode m (raster); returns the allowed-mode mask
extern "C" uint32_t ei4h_block(int k, int mb_left, const uint8_t *tile, uint8_t *avail, uint8_t *pred) {
  const ei4::Avail av = ei4::avail_of(k, mb_left != 0);
  avail[0] = av.left;
  avail[1] = av.top;
  avail[2] = av.tl;
  avail[3] = av.tr;
  int T[9], L[5];
  ei4::neighbours(tile, k, av, T, L);
  for (int m = 0; m < 9; ++m)
    for (int y = 0; y < 4; ++y) {
      const uint32_t row = ei4::pred_row(m, y, T, L, av);
      for (int x = 0; x < 4; ++x) pred[m * 16 + y * 4 + x] = static_cast<uint8_t>(row >> (8 * x));
    }
  return ei4::allowed_modes(av);
}
extern "C" int ei4h_pred_mode(int k, uint64_t cur, int mb_left, uint64_t left) {
  return ei4::pred_mode_of(k, cur, mb_left != 0, left);
}
extern "C" uint64_t ei4h_key(uint32_t sad, int qp, int mode, int pred) { return ei4::mode_key(sad, qp, mode, pred); }
extern "C" int ei4h_lambda16(int qp) { return full::erate::lambda16_of_qp(qp); }

// npic pictures (picture 0 IDR, the others P from the previous reconstruction) of mbh x mbw macroblocks at
// QP qp.  src / rec: NV12 [pic][16 mbh * 3 / 2][16 mbw]; kind [pic][my][mx]: 0 I_PCM, 1 Intra16x16, 2 I_NxN,
// 3 P_Skip, 4 inter at vector (0, 0), 5 the encoder's choice between the three intra kinds.  Fills cmd, cbp,
// coef [..][384], modes and bits [..][2].
extern "C" void ei4h_encode(int mbw, int mbh, int npic, int qp, const uint8_t *src, const uint8_t *kind, uint32_t *cmd,
                            uint8_t *cbp, int16_t *coef, uint64_t *modes, int32_t *bits, uint8_t *rec) {
  const int W = 16 * mbw, H = 16 * mbh;
  const int64_t fsz = static_cast<int64_t>(W) * H * 3 / 2;
  const Enc E{mbw, mbh, W, H, qp, cmd, cbp, coef, modes, bits};
  for (int p = 0; p < npic; ++p)
    for (int my = 0; my < mbh; ++my) {
      Row z;
      z.start();
      for (int mx = 0; mx < mbw; ++mx) {
        const int64_t mbi = (static_cast<int64_t>(p) * mbh + my) * mbw + mx;
        MbPix s, r = {}, left = {}, ref = {};
        load_mb(src + p * fsz, W, H, mx, my, s);
        if (mx > 0) load_mb(rec + p * fsz, W, H, mx - 1, my, left);
        if (p > 0) load_mb(rec + (p - 1) * fsz, W, H, mx, my, ref);
        bits[2 * mbi] = bits[2 * mbi + 1] = 0;
        const int want = kind[mbi];
        if (want == 0) {
          cmd[mbi] = edb::kPcmCmd;
          cbp[mbi] = 0;
          modes[mbi] = ei4::kNoModes;
          r = s;
          z.all(16);
          z.left_modes = ei4::kNoModes;
          z.has_left = true;
        } else if (want == 3 || want == 4) {
          inter_mb(E, want, mbi, s, ref, z, r);
        } else {
          uint8_t ly[16], lc[2][8];
          for (int i = 0; i < 16; ++i) ly[i] = left.y[i][15];
          for (int pl = 0; pl < 2; ++pl)
            for (int i = 0; i < 8; ++i) lc[pl][i] = left.c[pl][i][7];
          intra_mb(E, p == 0, want, mx, mbi, s, ly, lc, z, r);
        }
        store_mb(rec + p * fsz, W, H, mx, my, r);
      }
    }
}

// Those pictures as AVCC samples (4-byte lengths, one NAL unit per row) into out, their sizes into sizes.
// cabac: 0 CAVLC, 1 the bins coded as they come, 2 through the kernel's BinRing.  Returns the bytes, -1 on
// overflow.  I_PCM samples come from src.
extern "C" int64_t ei4h_write(int mbw, int mbh, int npic, int qp, int cabac, const uint8_t *src, const uint32_t *cmd,
                              const uint8_t *cbp, const int16_t *coef, const uint64_t *modes, uint8_t *out, int64_t cap,
                              int64_t *sizes) {
  const int W = 16 * mbw, H = 16 * mbh;
  const int64_t fsz = static_cast<int64_t>(W) * H * 3 / 2;
  int64_t at = 0;
  const int64_t slot = 64 + static_cast<int64_t>(mbw) * ecab::kMbBytes;
  std::vector<uint8_t> buf(static_cast<size_t>(slot)), pcm(static_cast<size_t>(mbw) * 384);
  for (int p = 0; p < npic; ++p) {
    const int64_t at0 = at;
    for (int row = 0; row < mbh; ++row) {
      const int64_t r = (static_cast<int64_t>(p) * mbh + row) * mbw;
      for (int mx = 0; mx < mbw; ++mx) {  // pcm_sample_luma 16 x 16, then Cb 8 x 8, Cr 8 x 8
        MbPix s;
        load_mb(src + p * fsz, W, H, mx, row, s);
        std::memcpy(&pcm[384 * mx], s.y, 256);
        std::memcpy(&pcm[384 * mx + 256], s.c, 128);
      }
      Sink o{buf.data(), slot, 0, 0, 0, 0, false};
      if (cabac) cabac_row(o, cabac == 2, p == 0, row, mbw, p, qp, cmd + r, cbp + r, coef + r * kCoefPerMb, modes + r, pcm.data());
      else cavlc_row(o, p == 0, row, mbw, p, qp, cmd + r, cbp + r, coef + r * kCoefPerMb, modes + r, pcm.data());
      if (o.over || at + 4 + o.n > cap) return -1;
      out[at] = static_cast<uint8_t>(o.n >> 24);
      out[at + 1] = static_cast<uint8_t>(o.n >> 16);
      out[at + 2] = static_cast<uint8_t>(o.n >> 8);
      out[at + 3] = static_cast<uint8_t>(o.n);
      std::memcpy(out + at + 4, buf.data(), static_cast<size_t>(o.n));
      at += 4 + o.n;
    }
    sizes[p] = at - at0;
  }
  return at;
}

#ifndef EI4H_NO_SPS_PPS  // enc_intra4_main.cpp links no stream writer
// SPS / PPS NAL units (each at most 64 bytes) of an mbw x mbh picture; sizes in n[0], n[1]
extern "C" void ei4h_sps_pps(int mbw, int mbh, int cabac, uint8_t *sps, uint8_t *pps, int32_t *n) {
  std::vector<uint8_t> s, p;
  make_sps_pps(mbw, mbh, 0, 0, 30, &s, &p, 0, cabac != 0);
  std::memcpy(sps, s.data(), s.size());
  std::memcpy(pps, p.data(), p.size());
  n[0] = static_cast<int32_t>(s.size());
  n[1] = static_cast<int32_t>(p.size());
}
#endif
