// CPU harness of the device encoder's CABAC writer (enc_cabac.h, the header
// the enc_write_cabac kernel calls):
//   ech_engine:    a sequence of decisions, bypass and terminate bins, raw
//                  bytes and restarts through ecab::Encoder into a ByteSink;
//   ech_contexts:  the 277 context variables of 9.3.1.1;
//   ech_sps_pps:   make_sps_pps (synth.cpp) with and without CABAC;
//   ech_pictures:  macroblock rows (command words, coded_block_pattern,
//                  levels, I_PCM samples: what a level of transcode.hip holds)
//                  written as slices, one per row, either through the
//                  header's mb_* functions or as CAVLC by the writer below,
//                  which restates enc_write's syntax for the comparison.
// TEST INFRASTRUCTURE (tests/test_enc_cabac_host.py; enc_cabac_main.cpp runs
// the same functions under the sanitizers).
#include <cstdint>
#include <cstring>
#include <vector>

#include "enc_cabac.h"
#include "h264.h"
#include "h264_tables.h"

using namespace vts;
namespace ecab = vts::full::ecab;
namespace edb = vts::full::edb;

namespace {
constexpr int kCoefPerMb = 384;  // transcode.hip's level layout
const uint8_t kCtLen[4][17][4] = VTS_CT_LEN_DATA;
const uint8_t kCtCode[4][17][4] = VTS_CT_CODE_DATA;
const uint8_t kTzLen[15][16] = VTS_TZ_LEN_DATA;
const uint8_t kTzCode[15][16] = VTS_TZ_CODE_DATA;
const uint8_t kTzcLen[3][4] = VTS_TZC_LEN_DATA;
const uint8_t kTzcCode[3][4] = VTS_TZC_CODE_DATA;
const uint8_t kRbLen[7][15] = VTS_RB_LEN_DATA;
const uint8_t kRbCode[7][15] = VTS_RB_CODE_DATA;
const uint8_t kCbpInterTab[48] = VTS_CBPP_DATA;

using Sink = ecab::ByteSink;

// residual_block_cavlc (7.3.5.3.2, 9.2) of lv[0 .. maxNum) in scan order; returns total_coeff
int cavlc_block(Sink &o, const int16_t *lv, int maxNum, int nC) {
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

// total_coeff of the left macroblock's right column (-1: none) and of the current macroblock
struct Nz {
  int l[4], lc[2][2], c[16], cc[2][4];
  void none() {
    for (int i = 0; i < 4; ++i) l[i] = -1;
    lc[0][0] = lc[0][1] = lc[1][0] = lc[1][1] = -1;
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
void cavlc_chroma(Sink &o, const int16_t *cp, int cc, Nz &z) {
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
void cavlc_luma(Sink &o, const int16_t *lv, int n, int k, Nz &z) {
  const int r = edb::raster_of_blk(k), bx = r & 3, by = r >> 2;
  const int na = bx ? z.c[r - 1] : z.l[by], nb = by ? z.c[r - 4] : -1;
  z.c[r] = cavlc_block(o, lv, n, nc_of(na, nb));
}

// one slice (macroblock row) of the encoder's syntax as CAVLC: what enc_write writes
void cavlc_row(Sink &o, bool idr, int row, int mbw, int frame_num, int qp, bool dbk, const uint32_t *cmd,
               const uint8_t *cbp_row, const int16_t *coef, const uint8_t *pcm) {
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
  if (dbk) {
    o.ue(2);
    o.se(0);
    o.se(0);
  } else {
    o.ue(1);
  }
  Nz z;
  z.none();
  uint32_t skip = 0;
  bool a_ok = false;
  int amx = 0, amy = 0;
  for (int mx = 0; mx < mbw; ++mx) {
    const uint32_t c = cmd[mx];
    const int16_t *cp = coef + static_cast<int64_t>(mx) * kCoefPerMb;
    if (c == edb::kPcmCmd || edb::is_intra_cmd(c)) {
      if (!idr) {
        o.ue(skip);
        skip = 0;
      }
      a_ok = false;
      if (c == edb::kPcmCmd) {
        o.ue(idr ? 25 : 30);
        o.align();
        for (int i = 0; i < 384; ++i) o.byte(pcm[384 * mx + i]);
        z.all(16);
        continue;
      }
      const int cbp = static_cast<int>(c >> 4) & 63;
      const uint32_t mbt = 1 + (c & 3u) + 4 * static_cast<uint32_t>(cbp >> 4) + ((cbp & 15) ? 12 : 0);
      o.ue(idr ? mbt : 5 + mbt);
      o.ue((c >> 2) & 3u);
      o.se(0);
      z.clear();
      cavlc_block(o, cp, 16, nc_of(z.l[0], -1));
      if (cbp & 15)
        for (int k = 0; k < 16; ++k) cavlc_luma(o, cp + 16 + 15 * k, 15, k, z);
      cavlc_chroma(o, cp, cbp >> 4, z);
      z.shift();
      continue;
    }
    const int mvx = static_cast<int16_t>(c & 0xffffu), mvy = static_cast<int16_t>(c >> 16), cbp = cbp_row[mx];
    if (mvx == 0 && mvy == 0 && cbp == 0) {
      ++skip;
      z.all(0);
    } else {
      o.ue(skip);
      skip = 0;
      o.ue(0);
      o.se(mvx - (a_ok ? amx : 0));
      o.se(mvy - (a_ok ? amy : 0));
      int code = 0;
      while (kCbpInterTab[code] != cbp) ++code;
      o.ue(static_cast<uint32_t>(code));
      z.clear();
      if (cbp) {
        o.se(0);
        for (int k = 0; k < 16; ++k)
          if ((cbp >> (k >> 2)) & 1) cavlc_luma(o, cp + 16 * k, 16, k, z);
        cavlc_chroma(o, cp, cbp >> 4, z);
      }
      z.shift();
    }
    a_ok = true;
    amx = mvx;
    amy = mvy;
  }
  if (skip) o.ue(skip);
  o.bits(1, 1);
  o.align();
}

// the same slice through enc_cabac.h, in the order enc_write_cabac walks it; E: the Encoder itself, or
// the kernel's BinRing in front of it
template <class E>
void cabac_mbs(E &e, Sink &o, bool idr, int mbw, const uint32_t *cmd, const uint8_t *cbp_row, const int16_t *coef,
               const uint8_t *pcm) {
  ecab::Left l = ecab::left_none();
  bool a_ok = false;
  int amx = 0, amy = 0;
  for (int mx = 0; mx < mbw; ++mx) {
    const uint32_t c = cmd[mx];
    const int16_t *cp = coef + static_cast<int64_t>(mx) * kCoefPerMb;
    const bool last = mx == mbw - 1;
    if (c == edb::kPcmCmd) {
      ecab::mb_pcm_begin(e, idr, l);
      o.align();
      for (int i = 0; i < 384; ++i) o.byte(pcm[384 * mx + i]);
      ecab::mb_pcm_end(e, l, last);
      a_ok = false;
    } else if (edb::is_intra_cmd(c)) {
      ecab::mb_intra16(e, idr, l, c, cp, last);
      a_ok = false;
    } else {
      const int mvx = static_cast<int16_t>(c & 0xffffu), mvy = static_cast<int16_t>(c >> 16), cbp = cbp_row[mx];
      if (mvx == 0 && mvy == 0 && cbp == 0) ecab::mb_skip(e, l, last);
      else ecab::mb_inter(e, l, mvx - (a_ok ? amx : 0), mvy - (a_ok ? amy : 0), cbp, cp, last);
      a_ok = true;
      amx = mvx;
      amy = mvy;
    }
  }
  e.sync();
}
void cabac_row(Sink &o, bool ring, bool idr, int row, int mbw, int frame_num, int qp, bool dbk, const uint32_t *cmd,
               const uint8_t *cbp_row, const int16_t *coef, const uint8_t *pcm) {
  ecab::slice_header(o, idr, row * mbw, frame_num, 0, qp, dbk, 0, 0);
  uint8_t st[ecab::kNumCtx];
  ecab::init_contexts(st, idr, qp);
  ecab::Encoder<Sink> e{&o, st, 0, 0, 0, false};
  e.start();
  if (ring) {
    std::vector<uint16_t> bins(ecab::kRingBins);
    ecab::BinRing<Sink> r{&e, bins.data(), 0};
    cabac_mbs(r, o, idr, mbw, cmd, cbp_row, coef, pcm);
  } else {
    cabac_mbs(e, o, idr, mbw, cmd, cbp_row, coef, pcm);
  }
  o.align();  // the flush ended in rbsp_stop_one_bit
}
}  // namespace

// ops: n triples (kind, a, b): 0 decision(ctx a, bin b), 1 bypass(b), 2 terminate(b), 3 raw byte a,
// 4 alignment zero bits, 5 restart (InitEncoder; the contexts stay).  Returns the bytes, -1 on overflow.
extern "C" int64_t ech_engine(const int32_t *ops, int64_t n, int islice, int qp, uint8_t *out, int64_t cap) {
  Sink o{out, cap, 0, 0, 0, 0, false};
  uint8_t st[ecab::kNumCtx];
  ecab::init_contexts(st, islice != 0, qp);
  ecab::Encoder<Sink> e{&o, st, 0, 0, 0, false};
  e.start();
  for (int64_t i = 0; i < n; ++i) {
    const int k = ops[3 * i], a = ops[3 * i + 1], b = ops[3 * i + 2];
    if (k == 0) e.decision(a, b);
    else if (k == 1) e.bypass(b);
    else if (k == 2) e.terminate(b);
    else if (k == 3) o.byte(static_cast<uint32_t>(a));
    else if (k == 4) o.align();
    else e.start();
  }
  o.align();
  return o.over ? -1 : o.n;
}

extern "C" void ech_contexts(int islice, int qp, uint8_t *st) { ecab::init_contexts(st, islice != 0, qp); }

#ifndef ECH_NO_SPS_PPS  // enc_cabac_main.cpp links no stream writer
// SPS / PPS NAL units (each at most 64 bytes) of an mbw x mbh picture; sizes in n[0], n[1]
extern "C" void ech_sps_pps(int mbw, int mbh, int cabac, uint8_t *sps, uint8_t *pps, int32_t *n) {
  std::vector<uint8_t> s, p;
  make_sps_pps(mbw, mbh, 0, 0, 30, &s, &p, 0, cabac != 0);
  std::memcpy(sps, s.data(), s.size());
  std::memcpy(pps, p.data(), p.size());
  n[0] = static_cast<int32_t>(s.size());
  n[1] = static_cast<int32_t>(p.size());
}
#endif

// npic pictures of mbh rows of mbw macroblocks (picture 0 IDR, the others P; frame_num = the index): one
// AVCC sample each (4-byte lengths, one NAL unit per row) into out, their sizes into sizes.  cabac: 0 CAVLC,
// 1 the bins coded as they come, 2 through the kernel's BinRing.  cmd / cbp:
// [pic][row][mx], coef: ... [384], pcm: ... [384] samples >= 1.  Returns the bytes, -1 on overflow.
extern "C" int64_t ech_pictures(int mbw, int mbh, int npic, int qp, int dbk, int cabac, const uint32_t *cmd,
                                const uint8_t *cbp, const int16_t *coef, const uint8_t *pcm, uint8_t *out,
                                int64_t cap, int64_t *sizes) {
  int64_t at = 0;
  const int64_t slot = 64 + static_cast<int64_t>(mbw) * ecab::kMbBytes;
  std::vector<uint8_t> buf(static_cast<size_t>(slot));
  for (int p = 0; p < npic; ++p) {
    const int64_t at0 = at;
    for (int row = 0; row < mbh; ++row) {
      const int64_t r = (static_cast<int64_t>(p) * mbh + row) * mbw;
      Sink o{buf.data(), slot, 0, 0, 0, 0, false};
      if (cabac) cabac_row(o, cabac == 2, p == 0, row, mbw, p, qp, dbk != 0, cmd + r, cbp + r, coef + r * kCoefPerMb, pcm + r * 384);
      else cavlc_row(o, p == 0, row, mbw, p, qp, dbk != 0, cmd + r, cbp + r, coef + r * kCoefPerMb, pcm + r * 384);
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
