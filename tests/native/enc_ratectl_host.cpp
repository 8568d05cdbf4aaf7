// CPU harness of the device encoder's rate control law (enc_ratectl.h, the
// header the kernel enc_rc calls):
//   erch_next_qp, erch_first_qp, erch_frame_budget: the law's functions;
//   erch_replay:   the law over one GOP whose pictures' measures are given, as
//                  enc_rc walks it behind every level: the QP of every picture.
// TEST INFRASTRUCTURE (tests/test_enc_ratectl_host.py, and the GPU test that
// compares the device's QPs with erch_replay on the call's own measures;
// enc_ratectl_main.cpp runs the same functions under the sanitizers).
#include <cstdint>

#include "enc_ratectl.h"

namespace erc = vts::full::erc;

extern "C" int erch_next_qp(int64_t B, int64_t L, int64_t j, int64_t spent, int64_t bits_j, int qp_j, int qp_min, int qp_max) {
  return erc::next_qp(B, L, j, spent, bits_j, qp_j, qp_min, qp_max);
}
extern "C" int erch_first_qp(int qp, int qp_min, int qp_max) { return erc::first_qp(qp, qp_min, qp_max); }
extern "C" int64_t erch_frame_budget(int bitrate_kbps, int64_t delta, int64_t timescale) {
  return erc::frame_budget(bitrate_kbps, delta, timescale);
}
extern "C" int64_t erch_step_q10(int k) { return erc::step_q10(k); }

// bits [L]: the measure of the GOP's pictures; qps [L]: the QP each is coded at.  The QP of picture j + 1
// depends on the measures of pictures 0 .. j alone, as on the device.
extern "C" void erch_replay(int64_t B, int64_t L, int qp, int qp_min, int qp_max, const uint32_t *bits, uint8_t *qps) {
  int64_t spent = 0;
  qps[0] = static_cast<uint8_t>(erc::first_qp(qp, qp_min, qp_max));
  for (int64_t j = 0; j + 1 < L; ++j) {
    spent += bits[j];
    qps[j + 1] = static_cast<uint8_t>(erc::next_qp(B, L, j, spent, bits[j], qps[j], qp_min, qp_max));
  }
}
