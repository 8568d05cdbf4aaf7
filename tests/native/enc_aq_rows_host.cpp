// CPU harness of pictures whose QP changes from macroblock to macroblock
// (vts_transcode_ext9, enc_aq.h: mb_qp_delta against the slice's running QP):
//   eaqr_encode: eph_encode (enc_part_host.cpp) with a QP per macroblock: the
//                quantiser and the reconstruction of a macroblock run at its own
//                QP, and the in-loop filter looks up an edge's indices from the
//                QP_Y of its two sides, the running QP where a macroblock sent no
//                delta (0 for I_PCM), walked as enc_deblock walks it;
//   eaqr_write:  eph_write with those QPs: the shared row writers with the
//                mb_qp_delta that eaq::RunQp gives, in the kernels' dispatch.
// The macroblock kinds, the prediction and the stream plumbing are
// enc_part_host.cpp's, included whole: its functions are internal to its
// translation unit.  TEST INFRASTRUCTURE (tests/test_enc_aq_host.py).
#include "enc_part_host.cpp"

#include "enc_aq.h"

namespace eaq = vts::full::eaq;

namespace {
bool sends(uint32_t c, int cbp) {
  return eaq::sends_delta(c == edb::kPcmCmd, edb::is_intra_cmd(c) && !ei4::is_i4_cmd(c), cbp);
}

// deblock_pic with a QP per macroblock (qp [mbh][mbw]; slice_qp: SliceQPY of every slice)
void deblock_pic_aq(int mbw, int mbh, int slice_qp, const uint8_t *qp, const uint32_t *cmd, const uint8_t *cbp,
                    const int16_t *coef, const uint32_t *mv4, uint8_t *pic) {
  const int pitch = 16 * mbw;
  uint8_t *Y = pic, *UV = pic + static_cast<int64_t>(pitch) * 16 * mbh;
  for (int my = 0; my < mbh; ++my) {
    edb::Mb left = edb::mb_of_cmd(edb::kPcmCmd, 0);
    eaq::RunQp rq;
    rq.start(slice_qp);
    int qy_left = 0;
    for (int mx = 0; mx < mbw; ++mx) {
      const int a = my * mbw + mx;
      const edb::Mb cur = edb::mb_of_cmd4(cmd[a], edb::nz_of_levels(coef + static_cast<int64_t>(a) * kCoefPerMb, cbp[a]), mv4 + 4 * a);
      rq.step(sends(cmd[a], cbp[a]), qp[a]);
      const int qy_cur = rq.filter_qp(cmd[a] == edb::kPcmCmd);
      for (int dir = 0; dir < 2; ++dir)
        for (int e = 0; e < 4; ++e) {
          if (e == 0 && (dir == 1 || mx == 0)) continue;
          const edb::Mb &p = e == 0 ? left : cur;
          const int qpp = e == 0 ? qy_left : qy_cur, qpq = qy_cur;
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
      qy_left = qy_cur;
    }
  }
}

// one slice as CAVLC: enc_write<.., kAq = true>'s dispatch
void cavlc_row_aq(Sink &o, bool idr, int row, int mbw, int frame_num, int slice_qp, const uint8_t *qp, bool dbk, const PRow &r) {
  erbsp::slice_header(o, false, idr, row * mbw, frame_num, 0, slice_qp - 26, dbk, 0, 0);
  ecav::Row z;
  z.start();
  eaq::RunQp rq;
  rq.start(slice_qp);
  for (int mx = 0; mx < mbw; ++mx) {
    const uint32_t c = r.d.cmd[mx];
    const int16_t *cp = r.d.coef + static_cast<int64_t>(mx) * kCoefPerMb;
    const int dqp = rq.step(sends(c, r.d.cbp[mx]), qp[mx]);
    if (c == edb::kPcmCmd) {
      ecav::mb_pcm_head(o, idr, z);
      pcm_samples(o, r.d.pcm + 384 * mx);
    } else if (ei4::is_i4_cmd(c)) {
      ecav::mb_intra4(o, idr, z, c, r.d.modes[mx], cp, dqp);
    } else if (edb::is_intra_cmd(c)) {
      ecav::mb_intra16(o, idr, z, c, cp, dqp);
    } else if (c == 0 && r.d.cbp[mx] == 0) {
      ecav::mb_skip(z);
    } else if (epart::is_part_cmd(c)) {
      ecav::mb_p_part(o, z, c, r.mv4 + 4 * mx, r.d.cbp[mx], cp, dqp);
    } else {
      ecav::mb_inter(o, z, c, r.d.cbp[mx], cp, dqp);
    }
  }
  ecav::slice_end(o, z);
}

// the same slice as CABAC: enc_write_cabac<.., kAq = true>'s dispatch
template <class E>
void cabac_mbs_aq(E &e, Sink &o, bool idr, int mbw, int slice_qp, const uint8_t *qp, const PRow &r) {
  const RowData &d = r.d;
  ecab::Left l = ecab::left_none();
  bool a_ok = false;
  int amx = 0, amy = 0, a3x = 0, a3y = 0;
  eaq::RunQp rq;
  rq.start(slice_qp);
  for (int mx = 0; mx < mbw; ++mx) {
    const uint32_t c = d.cmd[mx];
    const int16_t *cp = d.coef + static_cast<int64_t>(mx) * kCoefPerMb;
    const bool last = mx == mbw - 1;
    const int dqp = rq.step(sends(c, d.cbp[mx]), qp[mx]);
    if (c == edb::kPcmCmd) {
      ecab::mb_pcm_begin(e, idr, l);
      pcm_samples(o, d.pcm + 384 * mx);
      ecab::mb_pcm_end(e, l, last);
      a_ok = false;
    } else if (ei4::is_i4_cmd(c)) {
      ecab::mb_intra4(e, idr, l, c, d.modes[mx], cp, last, dqp);
      a_ok = false;
    } else if (edb::is_intra_cmd(c)) {
      ecab::mb_intra16(e, idr, l, c, cp, last, dqp);
      a_ok = false;
    } else if (epart::is_part_cmd(c)) {
      const uint32_t *v = r.mv4 + 4 * mx;
      ecab::mb_p_part(e, l, epart::part_shape(c), v, epart::Left{a_ok, {amx, amy}, {a3x, a3y}}, d.cbp[mx], cp, last, dqp);
      a_ok = true;
      amx = epart::mv_of_word(v[1]).x;
      amy = epart::mv_of_word(v[1]).y;
      a3x = epart::mv_of_word(v[3]).x;
      a3y = epart::mv_of_word(v[3]).y;
    } else {
      const int mvx = static_cast<int16_t>(c & 0xffffu), mvy = static_cast<int16_t>(c >> 16), cbp = d.cbp[mx];
      if (mvx == 0 && mvy == 0 && cbp == 0) ecab::mb_skip(e, l, last);
      else ecab::mb_inter(e, l, mvx - (a_ok ? amx : 0), mvy - (a_ok ? amy : 0), cbp, cp, last, dqp);
      a_ok = true;
      amx = a3x = mvx;
      amy = a3y = mvy;
    }
  }
  e.sync();
}
void cabac_row_aq(Sink &o, bool ring, bool idr, int row, int mbw, int frame_num, int slice_qp, const uint8_t *qp, bool dbk,
                  const PRow &r) {
  ecab::slice_header(o, idr, row * mbw, frame_num, 0, slice_qp, dbk, 0, 0);
  uint8_t st[ecab::kNumCtx];
  ecab::init_contexts(st, idr, slice_qp);
  ecab::Encoder<Sink> e{&o, st, 0, 0, 0, false};
  e.start();
  if (ring) {
    std::vector<uint16_t> bins(ecab::kRingBins);
    ecab::BinRing<Sink> br{&e, bins.data(), 0};
    cabac_mbs_aq(br, o, idr, mbw, slice_qp, qp, r);
  } else {
    cabac_mbs_aq(e, o, idr, mbw, slice_qp, qp, r);
  }
  o.align();  // the flush ended in rbsp_stop_one_bit
}
}  // namespace

// As eph_encode; slice_qp [npic], qp [pic][my][mx] the macroblocks' own QPs.
extern "C" void eaqr_encode(int mbw, int mbh, int npic, const int32_t *slice_qp, const uint8_t *qp, int dbk, const uint8_t *src,
                            const uint8_t *kind, const int32_t *vec, uint32_t *cmd, uint8_t *cbp, int16_t *coef, uint64_t *modes,
                            uint32_t *mv4, uint8_t *rec) {
  const int W = 16 * mbw, H = 16 * mbh;
  const int64_t fsz = static_cast<int64_t>(W) * H * 3 / 2;
  std::vector<int32_t> bits(static_cast<size_t>(2) * npic * mbw * mbh);
  for (int p = 0; p < npic; ++p) {
    for (int my = 0; my < mbh; ++my) {
      Row z;
      z.start();
      for (int mx = 0; mx < mbw; ++mx) {
        const int64_t mbi = (static_cast<int64_t>(p) * mbh + my) * mbw + mx;
        const Enc E{mbw, mbh, W, H, qp[mbi], cmd, cbp, coef, modes, bits.data()};
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
      deblock_pic_aq(mbw, mbh, slice_qp[p], qp + m0, cmd + m0, cbp + m0, coef + m0 * kCoefPerMb, mv4 + 4 * m0, rec + p * fsz);
    }
  }
}

// As eph_write; slice_qp [npic], qp [pic][my][mx].
extern "C" int64_t eaqr_write(int mbw, int mbh, int npic, const int32_t *slice_qp, const uint8_t *qp, int dbk, int cabac,
                              const uint8_t *src, const uint32_t *cmd, const uint8_t *cbp, const int16_t *coef,
                              const uint64_t *modes, const uint32_t *mv4, uint8_t *out, int64_t cap, int64_t *sizes) {
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
      if (cabac) cabac_row_aq(o, cabac == 2, p == 0, row, mbw, p, slice_qp[p], qp + r, dbk != 0, pr);
      else cavlc_row_aq(o, p == 0, row, mbw, p, slice_qp[p], qp + r, dbk != 0, pr);
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
