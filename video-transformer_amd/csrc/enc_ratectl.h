// enc_ratectl.h — the device encoder's rate control law (transcode.hip:
// enc_rc; DESIGN.md §11 "Rate control"), written once as integer arithmetic
// for the kernel and for the CPU harness (tests/native/enc_ratectl_host.cpp).
//
// One controller per GOP; GOPs share nothing, each has the budget B * L of
// its own L pictures at B bits a picture.  After picture j of a GOP was coded
// at QP qp_j and measured bits_j (the rate measure of vts_transcode_ext7:
// an upper bound of the macroblocks' bits), next_qp gives the QP of picture
// j + 1:
//   picture 0   clamp(qp)                                       (first_qp)
//   picture 1   clamp(qp_0 + 3): x264's default ipratio 1.4, 6 log2(1.4) = 2.9
//   picture j + 1, j >= 1: want = (B L - spent_j) / (L - j - 1), what is left
//               of the budget spread evenly over the pictures left;
//               bits_j == 0: qp_j (a picture that cost nothing says nothing
//               about the quantiser); want <= 0: qp_j + 4; else the step that
//               the ratio bits_j : want asks for, Qstep doubling every 6:
//               up by the largest k in 0..4 with bits_j 1024 >= want T[k],
//               down by the largest k with want 1024 >= bits_j T[k],
//               T[k] = 2^(k / 6) in Q10; clamped to [qp_min, qp_max].
// Nothing here depends on the device, and no HIP header is included.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VTS_RC_HD __host__ __device__
#else
#define VTS_RC_HD
#endif

namespace vts {
namespace full {
namespace erc {

constexpr int kMaxStep = 4;      // x264's default qpstep
constexpr int kIpStep = 3;       // picture 1 against the IDR picture
constexpr int kQpMinDefault = 10, kQpMaxDefault = 51;
constexpr int kMaxKbps = 1000000;

VTS_RC_HD inline int clamp_qp(int qp, int qp_min, int qp_max) { return qp < qp_min ? qp_min : (qp > qp_max ? qp_max : qp); }

// B: the bits of one picture at bitrate_kbps, a picture lasting `delta` ticks
// of `timescale` a second (floor; at most 10^9 delta / timescale)
VTS_RC_HD inline int64_t frame_budget(int bitrate_kbps, int64_t delta, int64_t timescale) {
  return static_cast<int64_t>(bitrate_kbps) * 1000 * delta / timescale;
}

VTS_RC_HD inline int first_qp(int qp, int qp_min, int qp_max) { return clamp_qp(qp, qp_min, qp_max); }

// 2^(k / 6) in Q10
VTS_RC_HD inline int64_t step_q10(int k) { return k == 0 ? 1024 : (k == 1 ? 1149 : (k == 2 ? 1290 : (k == 3 ? 1448 : 1625))); }

// The QP of picture j + 1 of a GOP of L pictures (j + 1 < L).  spent: the
// measure of pictures 0 .. j summed; bits_j: picture j's (< 2^32); qp_j: the
// QP picture j was coded at.  All products are int64: bits_j 1625 < 2^43, and
// want is capped at 2^50, far above any bits_j 1625 / 1024, so the cap changes
// no answer and want 1625 < 2^61.
VTS_RC_HD inline int next_qp(int64_t B, int64_t L, int64_t j, int64_t spent, int64_t bits_j, int qp_j, int qp_min,
                             int qp_max) {
  if (j == 0) return clamp_qp(qp_j + kIpStep, qp_min, qp_max);
  if (bits_j == 0) return clamp_qp(qp_j, qp_min, qp_max);
  const int64_t left = L - j - 1;
  int64_t want = (B * L - spent) / (left > 0 ? left : 1);
  if (want <= 0) return clamp_qp(qp_j + kMaxStep, qp_min, qp_max);
  const int64_t cap = int64_t(1) << 50;
  want = want > cap ? cap : want;
  int step = 0;
  if (bits_j >= want) {
    for (int k = 1; k <= kMaxStep; ++k)
      if (bits_j * 1024 >= want * step_q10(k)) step = k;
  } else {
    for (int k = 1; k <= kMaxStep; ++k)
      if (want * 1024 >= bits_j * step_q10(k)) step = -k;
  }
  return clamp_qp(qp_j + step, qp_min, qp_max);
}

}  // namespace erc
}  // namespace full
}  // namespace vts
