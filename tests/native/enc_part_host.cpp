// CPU harness of the device encoder's inter partitions (enc_part.h, the header
// enc_search<.., PT = true>, both slice writers and enc_deblock call;
// enc_cavlc.h's and enc_cabac.h's mb_p_part; enc_deblock.h's motion bS):
//   eph_pred:      epart::pred_block, the 8.4.1.3 predictor of a partition;
//   eph_pick:      seeded per-candidate quadrant SADs through the nine blocks'
//                  keys (enc_rate.h) and epart::decide_shape;
//   eph_canonical, eph_shape_bits, eph_block_quads, eph_guess: the small rules;
//   eph_bs:        edb::line_bs between two macroblocks with quadrant vectors;
//   eph_encode:    pictures of seeded macroblock kinds and quadrant vectors
//                  coded serially with the headers' arithmetic: the prediction
//                  of every quadrant at its own quarter-sample vector (8.4.2.2
//                  restated below, edge-clamped), the residual, the canonical
//                  shape, command words, mv4, levels, the reconstruction and,
//                  when asked, the in-loop filter walked as enc_deblock walks it;
//   eph_write:     those pictures as slices, one per macroblock row, CAVLC or
//                  CABAC (directly or through BinRing), in the kernels' dispatch;
//   eph_count:     a slice's macroblocks on the counting sink against the bits
//                  the byte sink receives.
// The intra kinds and the stream plumbing are enc_intra4_host.cpp's, included
// whole: its functions are internal to its translation unit.
// TEST INFRASTRUCTURE (tests/test_enc_part_host.py; enc_part_main.cpp runs the
// same functions under the sanitizers).
#include "enc_intra4_host.cpp"
#include "enc_part.h"

namespace epart = vts::full::epart;

namespace {
struct PRow {
  RowData d;
  const uint32_t *mv4;  // [mx][4]
};

// ---- 8.4.2.2 per sample, taps clamped to the picture
struct RefPic {
  const uint8_t *p;
  int W, H;
  int y(int x, int yy) const { return p[static_cast<int64_t>(full::clip3(0, H - 1, yy)) * W + full::clip3(0, W - 1, x)]; }
  int c(int pl, int x, int yy) const {
    return p[static_cast<int64_t>(H + full::clip3(0, H / 2 - 1, yy)) * W + 2 * full::clip3(0, W / 2 - 1, x) + pl];
  }
};
int luma_sample(const RefPic &R, int x, int y, int mvx, int mvy) {
  const int xi = x + (mvx >> 2), yi = y + (mvy >> 2), xf = mvx & 3, yf = mvy & 3;
  auto P = [&](int dx, int dy) { return R.y(xi + dx, yi + dy); };
  auto hrow = [&](int dy) { return full::tap6(P(-2, dy), P(-1, dy), P(0, dy), P(1, dy), P(2, dy), P(3, dy)); };
  auto vcol = [&](int dx) { return full::tap6(P(dx, -2), P(dx, -1), P(dx, 0), P(dx, 1), P(dx, 2), P(dx, 3)); };
  const int G = P(0, 0);
  if (!xf && !yf) return G;
  const int b = full::clip1((hrow(0) + 16) >> 5), h = full::clip1((vcol(0) + 16) >> 5);
  const int s = full::clip1((hrow(1) + 16) >> 5), m = full::clip1((vcol(1) + 16) >> 5);
  const int j = full::clip1((full::tap6(hrow(-2), hrow(-1), hrow(0), hrow(1), hrow(2), hrow(3)) + 512) >> 10);
  switch (yf * 4 + xf) {
    case 1: return (G + b + 1) >> 1;
    case 2: return b;
    case 3: return (P(1, 0) + b + 1) >> 1;
    case 4: return (G + h + 1) >> 1;
    case 5: return (b + h + 1) >> 1;
    case 6: return (b + j + 1) >> 1;
    case 7: return (b + m + 1) >> 1;
    case 8: return h;
    case 9: return (h + j + 1) >> 1;
    case 10: return j;
    case 11: return (j + m + 1) >> 1;
    case 12: return (P(0, 1) + h + 1) >> 1;
    case 13: return (h + s + 1) >> 1;
    case 14: return (j + s + 1) >> 1;
    default: return (m + s + 1) >> 1;
  }
}
int chroma_sample(const RefPic &R, int pl, int x, int y, int mvx, int mvy) {
  const int xi = x + (mvx >> 3), yi = y + (mvy >> 3), fx = mvx & 7, fy = mvy & 7;
  return ((8 - fx) * (8 - fy) * R.c(pl, xi, yi) + fx * (8 - fy) * R.c(pl, xi + 1, yi) + (8 - fx) * fy * R.c(pl, xi, yi + 1) +
          fx * fy * R.c(pl, xi + 1, yi + 1) + 32) >> 6;
}
// the composite prediction of macroblock (mx, my) with the quadrant vectors v
void predict_mb(const RefPic &R, int mx, int my, const epart::Mv *v, MbPix &p) {
  for (int y = 0; y < 16; ++y)
    for (int x = 0; x < 16; ++x) {
      const epart::Mv &q = v[epart::quad_at(x, y)];
      p.y[y][x] = static_cast<uint8_t>(luma_sample(R, mx * 16 + x, my * 16 + y, q.x, q.y));
    }
  for (int pl = 0; pl < 2; ++pl)
    for (int y = 0; y < 8; ++y)
      for (int x = 0; x < 8; ++x) {
        const epart::Mv &q = v[epart::quad_at(2 * x, 2 * y)];
        p.c[pl][y][x] = static_cast<uint8_t>(chroma_sample(R, pl, mx * 8 + x, my * 8 + y, q.x, q.y));
      }
}

// an inter macroblock with the quadrant vectors v against the prediction pred, as enc_search's residual
// epilogue codes it; skip: no residual (the reconstruction is the prediction)
void part_mb(const Enc &E, uint32_t *mv4, bool skip, int64_t mbi, const MbPix &src, const MbPix &pred, const epart::Mv *v,
             Row &z, MbPix &rec) {
  const int qp = E.qp, qpc = kQpc[qp];
  int16_t *cp = E.coef + mbi * kCoefPerMb;
  E.modes[mbi] = ei4::kNoModes;
  uint32_t *w = mv4 + 4 * mbi;
  for (int i = 0; i < 4; ++i) w[i] = epart::mv_word(v[i].x, v[i].y);
  const int shape = epart::canonical_shape(w);
  E.cmd[mbi] = shape ? epart::part_cmd(shape) : w[0];
  int cbp = 0;
  rec = pred;
  if (!skip) {
    for (int k = 0; k < 16; ++k) {
      const int r = edb::raster_of_blk(k), bx = r & 3, by = r >> 2;
      int x[16], zq[16], lv[16], res[16];
      for (int i = 0; i < 16; ++i) x[i] = src.y[by * 4 + (i >> 2)][bx * 4 + (i & 3)] - pred.y[by * 4 + (i >> 2)][bx * 4 + (i & 3)];
      if (eres::code_block<false>(x, qp, zq, lv, nullptr)) cbp |= 1 << (k >> 2);
      full::scale_idct4(zq, qp, false, res);
      for (int i = 0; i < 16; ++i)
        rec.y[by * 4 + (i >> 2)][bx * 4 + (i & 3)] = static_cast<uint8_t>(full::clip1(pred.y[by * 4 + (i >> 2)][bx * 4 + (i & 3)] + res[i]));
      for (int q = 0; q < 16; ++q) cp[16 * k + q] = static_cast<int16_t>(lv[q]);
    }
    cbp |= code_chroma(src, pred.c, qpc, cp, rec) << 4;
  }
  E.cbp[mbi] = static_cast<uint8_t>(cbp);
  BitCount b;  // the writer's bookkeeping, for the macroblocks to the right
  if (shape) ecav::mb_p_part(b, z, E.cmd[mbi], w, cbp, cp);
  else if (w[0] == 0 && cbp == 0) ecav::mb_skip(z);
  else ecav::mb_inter(b, z, w[0], cbp, cp);
}

// the in-loop filter over one picture, walked as enc_deblock<true> walks it
void deblock_pic(int mbw, int mbh, int qp, const uint32_t *cmd, const uint8_t *cbp, const int16_t *coef, const uint32_t *mv4,
                 uint8_t *pic) {
  const int pitch = 16 * mbw;
  uint8_t *Y = pic, *UV = pic + static_cast<int64_t>(pitch) * 16 * mbh;
  for (int my = 0; my < mbh; ++my) {
    edb::Mb left = edb::mb_of_cmd(edb::kPcmCmd, 0);
    for (int mx = 0; mx < mbw; ++mx) {
      const int a = my * mbw + mx;
      const edb::Mb cur = edb::mb_of_cmd4(cmd[a], edb::nz_of_levels(coef + static_cast<int64_t>(a) * kCoefPerMb, cbp[a]), mv4 + 4 * a);
      for (int dir = 0; dir < 2; ++dir)
        for (int e = 0; e < 4; ++e) {
          if (e == 0 && (dir == 1 || mx == 0)) continue;
          const edb::Mb &p = e == 0 ? left : cur;
          const int qpp = edb::qp_of(p, qp), qpq = edb::qp_of(cur, qp);
          const edb::Idx xl = edb::indices(qpp, qpq, 0, 0, false, 0);
          for (int k = 0; k < 16; ++k) {
            uint8_t *s = dir ? Y + static_cast<int64_t>(my * 16 + 4 * e) * pitch + mx * 16 + k
                             : Y + static_cast<int64_t>(my * 16 + k) * pitch + mx * 16 + 4 * e;
            edb::filter(s, dir ? pitch : 1, edb::line_bs(p, cur, dir, e, k), false, xl);
          }
          if (e & 1) continue;
          const edb::Idx xc = edb::indices(qpp, qpq, 0, 0, true, 0);
          for (int pl = 0; pl < 2; ++pl)
            for (int k = 0; k < 8; ++k) {
              uint8_t *s = dir ? UV + static_cast<int64_t>(my * 8 + 2 * e) * pitch + 2 * (mx * 8 + k) + pl
                               : UV + static_cast<int64_t>(my * 8 + k) * pitch + 2 * (mx * 8 + 2 * e) + pl;
              edb::filter(s, dir ? pitch : 2, edb::line_bs(p, cur, dir, e, 2 * k), true, xc);
            }
        }
      left = cur;
    }
  }
}

// macroblock mx of the row through enc_cavlc.h: enc_write's dispatch with partitions
template <class S>
void cavlc_mb_p(S &o, bool idr, ecav::Row &z, const PRow &r, int mx) {
  const uint32_t c = r.d.cmd[mx];
  if (epart::is_part_cmd(c)) ecav::mb_p_part(o, z, c, r.mv4 + 4 * mx, r.d.cbp[mx], r.d.coef + static_cast<int64_t>(mx) * kCoefPerMb);
  else cavlc_mb(o, idr, z, r.d, mx);
}
void cavlc_row_p(Sink &o, bool idr, int row, int mbw, int frame_num, int qp, bool dbk, const PRow &r) {
  erbsp::slice_header(o, false, idr, row * mbw, frame_num, 0, qp - 26, dbk, 0, 0);
  ecav::Row z;
  z.start();
  for (int mx = 0; mx < mbw; ++mx) {
    cavlc_mb_p(o, idr, z, r, mx);
    if (r.d.cmd[mx] == edb::kPcmCmd) pcm_samples(o, r.d.pcm + 384 * mx);
  }
  ecav::slice_end(o, z);
}
// the same slice as CABAC: enc_write_cabac's dispatch with partitions
template <class E>
void cabac_mbs_p(E &e, Sink &o, bool idr, int mbw, const PRow &r) {
  const RowData &d = r.d;
  ecab::Left l = ecab::left_none();
  bool a_ok = false;
  int amx = 0, amy = 0, a3x = 0, a3y = 0;
  for (int mx = 0; mx < mbw; ++mx) {
    const uint32_t c = d.cmd[mx];
    const int16_t *cp = d.coef + static_cast<int64_t>(mx) * kCoefPerMb;
    const bool last = mx == mbw - 1;
    if (c == edb::kPcmCmd) {
      ecab::mb_pcm_begin(e, idr, l);
      pcm_samples(o, d.pcm + 384 * mx);
      ecab::mb_pcm_end(e, l, last);
      a_ok = false;
    } else if (ei4::is_i4_cmd(c)) {
      ecab::mb_intra4(e, idr, l, c, d.modes[mx], cp, last);
      a_ok = false;
    } else if (edb::is_intra_cmd(c)) {
      ecab::mb_intra16(e, idr, l, c, cp, last);
      a_ok = false;
    } else if (epart::is_part_cmd(c)) {
      const uint32_t *v = r.mv4 + 4 * mx;
      ecab::mb_p_part(e, l, epart::part_shape(c), v, epart::Left{a_ok, {amx, amy}, {a3x, a3y}}, d.cbp[mx], cp, last);
      a_ok = true;
      amx = epart::mv_of_word(v[1]).x;
      amy = epart::mv_of_word(v[1]).y;
      a3x = epart::mv_of_word(v[3]).x;
      a3y = epart::mv_of_word(v[3]).y;
    } else {
      const int mvx = static_cast<int16_t>(c & 0xffffu), mvy = static_cast<int16_t>(c >> 16), cbp = d.cbp[mx];
      if (mvx == 0 && mvy == 0 && cbp == 0) ecab::mb_skip(e, l, last);
      else ecab::mb_inter(e, l, mvx - (a_ok ? amx : 0), mvy - (a_ok ? amy : 0), cbp, cp, last);
      a_ok = true;
      amx = a3x = mvx;
      amy = a3y = mvy;
    }
  }
  e.sync();
}
void cabac_row_p(Sink &o, bool ring, bool idr, int row, int mbw, int frame_num, int qp, bool dbk, const PRow &r) {
  ecab::slice_header(o, idr, row * mbw, frame_num, 0, qp, dbk, 0, 0);
  uint8_t st[ecab::kNumCtx];
  ecab::init_contexts(st, idr, qp);
  ecab::Encoder<Sink> e{&o, st, 0, 0, 0, false};
  e.start();
  if (ring) {
    std::vector<uint16_t> bins(ecab::kRingBins);
    ecab::BinRing<Sink> br{&e, bins.data(), 0};
    cabac_mbs_p(br, o, idr, mbw, r);
  } else {
    cabac_mbs_p(e, o, idr, mbw, r);
  }
  o.align();  // the flush ended in rbsp_stop_one_bit
}
}  // namespace

extern "C" void eph_pred(int shape, int part, const int32_t *q8, int left_ok, const int32_t *l4, int32_t *out) {
  epart::Mv q[4];
  for (int i = 0; i < 4; ++i) q[i] = epart::Mv{q8[2 * i], q8[2 * i + 1]};
  const epart::Mv p = epart::pred_block(shape, part, q, epart::Left{left_ok != 0, {l4[0], l4[1]}, {l4[2], l4[3]}});
  out[0] = p.x;
  out[1] = p.y;
}
extern "C" int eph_canonical(const uint32_t *v) { return epart::canonical_shape(v); }
extern "C" int eph_shape_bits(int s) { return epart::shape_bits(s); }
extern "C" int eph_block_quads(int b) { return epart::block_quads(b); }
extern "C" int eph_frac_class(const uint32_t *v) { return epart::frac_class(v); }
extern "C" uint32_t eph_part_cmd(int shape) { return epart::part_cmd(shape); }
extern "C" int eph_is_part_cmd(uint32_t c) { return epart::is_part_cmd(c); }
extern "C" void eph_guess(uint32_t left_prev, uint32_t left_q1, int mx, int j, int32_t *out) {
  const epart::Mv p = epart::pred_guess(left_prev, left_q1, mx, j);
  out[0] = p.x;
  out[1] = p.y;
}
// ncand candidates (index = position; vec [ncand][2] quarter samples, quads [ncand][4] the quadrant SADs)
// against the predictor guess (px, py): every block's winning cost, index and SAD, and the shape
extern "C" int eph_pick(int ncand, const uint32_t *quads, const int32_t *vec, int lam16, int px, int py, uint32_t *cost9,
                        int32_t *idx9, uint32_t *sad9) {
  uint64_t best[epart::kBlocks];
  for (int b = 0; b < epart::kBlocks; ++b) best[b] = ~0ull;
  for (int c = 0; c < ncand; ++c)
    for (int b = 0; b < epart::kBlocks; ++b) {
      const uint32_t sad = epart::block_sad(quads + 4 * c, b);
      const uint64_t k = full::erate::key_of(full::erate::cost16(sad, lam16, vec[2 * c], vec[2 * c + 1], px, py),
                                              static_cast<uint32_t>(c), sad);
      if (k < best[b]) best[b] = k;
    }
  for (int b = 0; b < epart::kBlocks; ++b) {
    cost9[b] = static_cast<uint32_t>(best[b] >> 32);
    idx9[b] = static_cast<int32_t>(full::erate::key_index(best[b]));
    sad9[b] = full::erate::key_sad(best[b]);
  }
  return epart::decide_shape(cost9, lam16);
}
// bS of line k of edge e in direction dir between p (the left macroblock for e = 0, else q itself) and q
extern "C" int eph_bs(uint32_t cmd_p, uint32_t nz_p, const uint32_t *mv4_p, uint32_t cmd_q, uint32_t nz_q,
                      const uint32_t *mv4_q, int dir, int e, int k) {
  const edb::Mb p = edb::mb_of_cmd4(cmd_p, nz_p, mv4_p), q = edb::mb_of_cmd4(cmd_q, nz_q, mv4_q);
  return edb::line_bs(e == 0 ? p : q, q, dir, e, k);
}

// npic pictures (picture 0 IDR, the others P from the previous reconstruction) of mbh x mbw macroblocks at
// QP qp.  src / rec: NV12 [pic][16 mbh * 3 / 2][16 mbw]; kind [pic][my][mx]: 0 I_PCM, 1 Intra16x16, 2 I_NxN,
// 3 inter without residual, 4 inter with it; vec [pic][my][mx][4][2] the quadrant vectors of the inter kinds.
// dbk: every picture is filtered before the next predicts from it.  Fills cmd, cbp, coef [..][384], modes, mv4.
extern "C" void eph_encode(int mbw, int mbh, int npic, int qp, int dbk, const uint8_t *src, const uint8_t *kind,
                           const int32_t *vec, uint32_t *cmd, uint8_t *cbp, int16_t *coef, uint64_t *modes, uint32_t *mv4,
                           uint8_t *rec) {
  const int W = 16 * mbw, H = 16 * mbh;
  const int64_t fsz = static_cast<int64_t>(W) * H * 3 / 2;
  std::vector<int32_t> bits(static_cast<size_t>(2) * npic * mbw * mbh);
  const Enc E{mbw, mbh, W, H, qp, cmd, cbp, coef, modes, bits.data()};
  for (int p = 0; p < npic; ++p) {
    for (int my = 0; my < mbh; ++my) {
      Row z;
      z.start();
      for (int mx = 0; mx < mbw; ++mx) {
        const int64_t mbi = (static_cast<int64_t>(p) * mbh + my) * mbw + mx;
        MbPix s, r = {}, left = {};
        load_mb(src + p * fsz, W, H, mx, my, s);
        if (mx > 0) load_mb(rec + p * fsz, W, H, mx - 1, my, left);
        const int want = kind[mbi];
        for (int i = 0; i < 4; ++i) mv4[4 * mbi + i] = epart::kNoMv;
        if (want == 0) {
          cmd[mbi] = edb::kPcmCmd;
          cbp[mbi] = 0;
          modes[mbi] = ei4::kNoModes;
          r = s;
          BitCount b;
          ecav::mb_pcm_head(b, p == 0, z);
        } else if (want >= 3) {
          epart::Mv v[4];
          for (int i = 0; i < 4; ++i) v[i] = epart::Mv{vec[8 * mbi + 2 * i], vec[8 * mbi + 2 * i + 1]};
          MbPix pred;
          predict_mb(RefPic{rec + (p - 1) * fsz, W, H}, mx, my, v, pred);
          part_mb(E, mv4, want == 3, mbi, s, pred, v, z, r);
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
    if (dbk) {
      const int64_t m0 = static_cast<int64_t>(p) * mbw * mbh;
      deblock_pic(mbw, mbh, qp, cmd + m0, cbp + m0, coef + m0 * kCoefPerMb, mv4 + 4 * m0, rec + p * fsz);
    }
  }
}

// Those pictures as AVCC samples (4-byte lengths, one NAL unit per row) into out, their sizes into sizes.
// cabac: 0 CAVLC, 1 the bins coded as they come, 2 through the kernel's BinRing.  Returns the bytes, -1 on
// overflow.  I_PCM samples come from src.
extern "C" int64_t eph_write(int mbw, int mbh, int npic, int qp, int dbk, int cabac, const uint8_t *src, const uint32_t *cmd,
                             const uint8_t *cbp, const int16_t *coef, const uint64_t *modes, const uint32_t *mv4,
                             uint8_t *out, int64_t cap, int64_t *sizes) {
  const int W = 16 * mbw, H = 16 * mbh;
  const int64_t fsz = static_cast<int64_t>(W) * H * 3 / 2;
  std::vector<uint8_t> pcm(static_cast<size_t>(mbw) * 384);
  const int64_t slot = 64 + static_cast<int64_t>(mbw) * ecab::kMbBytes;
  std::vector<uint8_t> buf(static_cast<size_t>(slot));
  int64_t at = 0;
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
      const PRow pr{RowData{cmd + r, cbp + r, coef + r * kCoefPerMb, modes + r, pcm.data()}, mv4 + 4 * r};
      Sink o{buf.data(), slot};
      if (cabac) cabac_row_p(o, cabac == 2, p == 0, row, mbw, p, qp, dbk != 0, pr);
      else cavlc_row_p(o, p == 0, row, mbw, p, qp, dbk != 0, pr);
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

// Counting against writing, macroblock by macroblock of one CAVLC slice, as ei4h_count with partitions
extern "C" int eph_count(int idr, int mbw, const uint32_t *cmd, const uint8_t *cbp, const int16_t *coef, const uint64_t *modes,
                         const uint32_t *mv4, const uint8_t *pcm, int64_t *counted, int64_t *written) {
  const PRow r{RowData{cmd, cbp, coef, modes, pcm}, mv4};
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
    cavlc_mb_p(b, idr != 0, zc, r, mx);
    cavlc_mb_p(o, idr != 0, zw, r, mx);
    counted[mx] = b.n;
    written[mx] = rbsp_bits() - before;
    if (cmd[mx] == edb::kPcmCmd) pcm_samples(o, pcm + 384 * mx);
    bad |= std::memcmp(zw.lnz, zc.lnz, sizeof zw.lnz) || std::memcmp(zw.lnzc, zc.lnzc, sizeof zw.lnzc) || zw.skip != zc.skip ||
           zw.a_ok != zc.a_ok || zw.amx != zc.amx || zw.amy != zc.amy || zw.a3x != zc.a3x || zw.a3y != zc.a3y;
  }
  return bad || o.over;
}
