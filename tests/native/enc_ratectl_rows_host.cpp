// CPU harness of pictures whose QP changes from picture to picture
// (vts_transcode_ext7: slice_qp_delta = the picture's QP - 26 in every slice
// header, the CABAC contexts initialised at that SliceQPY, mb_qp_delta 0):
//   erq_encode: eph_encode (enc_part_host.cpp) with a QP per picture: the
//               quantiser, the reconstruction and the in-loop filter of picture
//               p run at qp[p], and picture p + 1 predicts from that;
//   erq_write:  eph_write with a QP per picture, through the same row writers.
// The macroblock kinds, the prediction and the writers' dispatch are
// enc_part_host.cpp's, included whole: its functions are internal to its
// translation unit.  TEST INFRASTRUCTURE (tests/test_enc_ratectl_host.py).
#include "enc_part_host.cpp"

// As eph_encode; qp [npic].
extern "C" void erq_encode(int mbw, int mbh, int npic, const int32_t *qp, int dbk, const uint8_t *src, const uint8_t *kind,
                           const int32_t *vec, uint32_t *cmd, uint8_t *cbp, int16_t *coef, uint64_t *modes, uint32_t *mv4,
                           uint8_t *rec) {
  const int W = 16 * mbw, H = 16 * mbh;
  const int64_t fsz = static_cast<int64_t>(W) * H * 3 / 2;
  std::vector<int32_t> bits(static_cast<size_t>(2) * npic * mbw * mbh);
  for (int p = 0; p < npic; ++p) {
    const Enc E{mbw, mbh, W, H, qp[p], cmd, cbp, coef, modes, bits.data()};
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
      deblock_pic(mbw, mbh, qp[p], cmd + m0, cbp + m0, coef + m0 * kCoefPerMb, mv4 + 4 * m0, rec + p * fsz);
    }
  }
}

// As eph_write; qp [npic].
extern "C" int64_t erq_write(int mbw, int mbh, int npic, const int32_t *qp, int dbk, int cabac, const uint8_t *src,
                             const uint32_t *cmd, const uint8_t *cbp, const int16_t *coef, const uint64_t *modes,
                             const uint32_t *mv4, uint8_t *out, int64_t cap, int64_t *sizes) {
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
      if (cabac) cabac_row_p(o, cabac == 2, p == 0, row, mbw, p, qp[p], dbk != 0, pr);
      else cavlc_row_p(o, p == 0, row, mbw, p, qp[p], dbk != 0, pr);
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
