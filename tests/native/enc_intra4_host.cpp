// CPU harness of the device encoder's Intra_4x4 path (enc_intra4.h, the header
// enc_intra<true> and both slice writers call; enc_cabac.h's mb_intra4):
//   ei4h_block:     availability, allowed modes and the nine predictions of one
//                   block over a given tile;
//   ei4h_pred_mode: predIntra4x4PredMode; ei4h_key: the mode key;
//   ei4h_encode:    pictures of seeded macroblock kinds (I_PCM, Intra16x16,
//                   I_NxN, P_Skip, coded inter at vector (0, 0), or the
//                   encoder's own choice between the intra kinds) coded
//                   serially with the headers' arithmetic: command words,
//                   patterns, levels, mode words, the two candidates' bits (on
//                   enc_cavlc.h's counting sink) and the reconstruction;
//   ei4h_write:     those pictures as slices, one per macroblock row: CAVLC
//                   through enc_cavlc.h, the code enc_write calls, or CABAC
//                   through enc_cabac.h, directly or through BinRing
//                   (enc_rows.h walks both);
//   ei4h_count:     a slice's macroblocks on enc_cavlc.h's counting sink
//                   against the bits the byte sink receives.
// TEST INFRASTRUCTURE (tests/test_enc_intra4_host.py; enc_intra4_main.cpp runs
// the same functions under the sanitizers).
#include <cstdint>
#include <cstring>
#include <vector>

#include "enc_intra4.h"
#include "enc_residual.h"
#include "enc_rows.h"
#include "h264.h"
#include "h264_tables.h"

using namespace vts;
namespace eres = vts::full::eres;

namespace {
constexpr int kPcmBits = 3072;
const uint8_t kQpc[52] = VTS_QPC_DATA;
const uint8_t kZz[16] = VTS_ZZ_DATA;
using Row = ecav::Row;
using BitCount = erbsp::BitCount;

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
  ecav::intra16_layer(b16, idr, z16, cmd16, c16);
  ecav::intra4_layer(b4, idr, z4, cmd4, word, c4);
  E.bits[2 * mbi] = static_cast<int32_t>(b16.n);
  E.bits[2 * mbi + 1] = static_cast<int32_t>(b4.n);
  const bool use4 = want == 2 || (want == 5 && b4.n < b16.n);
  const int64_t nb = use4 ? b4.n : b16.n;
  if (want == 5 && nb > kPcmBits) {  // stays I_PCM
    E.cmd[mbi] = edb::kPcmCmd;
    E.cbp[mbi] = 0;
    E.modes[mbi] = ei4::kNoModes;
    rec = src;
    BitCount b;  // the writer's bookkeeping only
    ecav::mb_pcm_head(b, idr, z);
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
  BitCount b;  // the writer's bookkeeping, for the intra macroblocks to the right
  if (cbp == 0) {  // P_Skip
    rec = ref;
    ecav::mb_skip(z);
  } else {
    ecav::mb_inter(b, z, 0, cbp, cp);
  }
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
          BitCount b;
          ecav::mb_pcm_head(b, p == 0, z);
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
  std::vector<uint8_t> pcm(static_cast<size_t>(mbw) * 384);
  auto row_data = [&](int p, int row) {
    const int64_t r = (static_cast<int64_t>(p) * mbh + row) * mbw;
    for (int mx = 0; mx < mbw; ++mx) {  // pcm_sample_luma 16 x 16, then Cb 8 x 8, Cr 8 x 8
      MbPix s;
      load_mb(src + p * fsz, W, H, mx, row, s);
      std::memcpy(&pcm[384 * mx], s.y, 256);
      std::memcpy(&pcm[384 * mx + 256], s.c, 128);
    }
    return RowData{cmd + r, cbp + r, coef + r * kCoefPerMb, modes + r, pcm.data()};
  };
  return write_pictures(mbw, mbh, npic, qp, false, cabac, row_data, out, cap, sizes);
}

// Counting against writing, macroblock by macroblock of one CAVLC slice: counted[mx] the bits enc_cavlc.h's
// mb_* function adds on the counting sink, written[mx] the RBSP bits the byte sink received from the same
// call (the bytes it stored less the emulation prevention bytes among them, and the bits it still holds).
// A P_Skip macroblock gives 0 and 0: its run goes with the next coded macroblock.  I_PCM: the head only (the
// samples follow in the byte sink, outside the count).  Returns 0 when the two row states ended equal and
// nothing overflowed.
extern "C" int ei4h_count(int idr, int mbw, const uint32_t *cmd, const uint8_t *cbp, const int16_t *coef,
                          const uint64_t *modes, const uint8_t *pcm, int64_t *counted, int64_t *written) {
  const RowData d{cmd, cbp, coef, modes, pcm};
  std::vector<uint8_t> buf(static_cast<size_t>(64 + static_cast<int64_t>(mbw) * ecab::kMbBytes));
  Sink o{buf.data(), static_cast<int64_t>(buf.size())};
  auto rbsp_bits = [&]() {
    int64_t ep = 0;
    for (int64_t i = 0, zeros = 0; i < o.n; ++i) {
      if (zeros >= 2 && buf[i] == 3) {
        ++ep;
        zeros = 0;
        continue;
      }
      zeros = buf[i] ? 0 : zeros + 1;
    }
    return 8 * (o.n - ep) + o.nacc;
  };
  Row zw, zc;
  zw.start();
  zc.start();
  int bad = 0;
  for (int mx = 0; mx < mbw; ++mx) {
    BitCount b;
    const int64_t before = rbsp_bits();
    cavlc_mb(b, idr != 0, zc, d, mx);
    cavlc_mb(o, idr != 0, zw, d, mx);
    counted[mx] = b.n;
    written[mx] = rbsp_bits() - before;
    if (cmd[mx] == edb::kPcmCmd) pcm_samples(o, pcm + 384 * mx);
    bad |= std::memcmp(zw.lnz, zc.lnz, sizeof zw.lnz) || std::memcmp(zw.lnzc, zc.lnzc, sizeof zw.lnzc) ||
           zw.skip != zc.skip || zw.left_modes != zc.left_modes || zw.a_ok != zc.a_ok || zw.amx != zc.amx || zw.amy != zc.amy;
  }
  return bad || o.over;
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
