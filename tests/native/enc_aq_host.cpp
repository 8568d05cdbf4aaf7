// CPU harness of the device encoder's adaptive quantisation (enc_aq.h, the
// header the kernel enc_aq and every stage that reads a macroblock's QP call):
//   eaqh_energy, eaqh_log2_q8, eaqh_offset, eaqh_qp_mb, eaqh_se_bits: the law's functions;
//   eaqh_picture:  the offsets of every macroblock of one coded NV12 picture,
//                  the sums taken sample by sample;
//   eaqh_row:      the running-QP rule over one slice of hand-made macroblocks:
//                  mb_qp_delta, the CABAC ctxIdxInc of its first bin and the
//                  QP_Y the in-loop filter reads, macroblock by macroblock.
// TEST INFRASTRUCTURE (tests/test_enc_aq_host.py, and the GPU test that
// compares the device's macroblock QPs with eaqh_picture on the encoder's
// input; enc_aq_main.cpp runs the same functions under the sanitizers).
#include <cstdint>

#include "enc_aq.h"

namespace eaq = vts::full::eaq;

extern "C" uint32_t eaqh_energy(uint32_t s1y, uint32_t s2y, uint32_t s1u, uint32_t s2u, uint32_t s1v, uint32_t s2v) {
  return eaq::energy(s1y, s2y, s1u, s2u, s1v, s2v);
}
extern "C" int eaqh_log2_q8(uint32_t e) { return eaq::log2_q8(e); }
extern "C" int eaqh_offset(uint32_t e, int strength_q8, int aq_max) { return eaq::offset_of_energy(e, strength_q8, aq_max); }
extern "C" int eaqh_qp_mb(int qp, int off, int lo, int hi) { return eaq::qp_mb(qp, off, lo, hi); }
extern "C" int eaqh_se_bits(int v) { return eaq::se_bits(v); }

// pic: NV12, cw x ch luma rows then ch / 2 rows of Cb|Cr pairs; off [ch / 16][cw / 16]
extern "C" void eaqh_picture(const uint8_t *pic, int cw, int ch, int strength_q8, int aq_max, int8_t *off) {
  const int mbw = cw / 16, mbh = ch / 16;
  const uint8_t *uv = pic + static_cast<int64_t>(cw) * ch;
  for (int my = 0; my < mbh; ++my)
    for (int mx = 0; mx < mbw; ++mx) {
      uint32_t s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
      for (int y = 0; y < 16; ++y)
        for (int x = 0; x < 16; ++x) {
          const uint32_t v = pic[static_cast<int64_t>(my * 16 + y) * cw + mx * 16 + x];
          s1[0] += v;
          s2[0] += v * v;
        }
      for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 8; ++x)
          for (int pl = 0; pl < 2; ++pl) {
            const uint32_t v = uv[static_cast<int64_t>(my * 8 + y) * cw + 2 * (mx * 8 + x) + pl];
            s1[1 + pl] += v;
            s2[1 + pl] += v * v;
          }
      off[my * mbw + mx] =
          static_cast<int8_t>(eaq::offset_of_energy(eaq::energy(s1[0], s2[0], s1[1], s2[1], s1[2], s2[2]), strength_q8, aq_max));
    }
}

// One slice of n macroblocks.  kind [n]: 0 I_PCM, 1 Intra16x16, 2 anything else (inter, I_NxN, P_Skip with
// pattern 0); cbp [n]; qp [n] the macroblocks' own QPs.  delta [n]: mb_qp_delta (0 where none is sent);
// sent [n]; inc [n]: ctxIdxInc of the first bin where one is sent; qpy [n]: QP_Y for the in-loop filter.
extern "C" void eaqh_row(int n, int slice_qp, const uint8_t *kind, const uint8_t *cbp, const uint8_t *qp, int32_t *delta,
                         uint8_t *sent, uint8_t *inc, int32_t *qpy) {
  eaq::RunQp rq;
  rq.start(slice_qp);
  for (int i = 0; i < n; ++i) {
    const bool pcm = kind[i] == 0, s = eaq::sends_delta(pcm, kind[i] == 1, cbp[i]);
    int ci = 0;
    delta[i] = rq.step(s, qp[i], &ci);
    sent[i] = s;
    inc[i] = static_cast<uint8_t>(ci);
    qpy[i] = rq.filter_qp(pcm);
  }
}
