// CPU harness of the motion search's rate-aware decisions (enc_rate.h, the
// header the enc_search kernel calls): plain C entry points over the header's
// functions, so that pytest can compare their values with Python's.
// TEST INFRASTRUCTURE (tests/test_enc_rate_host.py).
#include <cstdint>

#include "enc_rate.h"

namespace er = vts::full::erate;

extern "C" int erh_selen(int k) { return er::selen(k); }
extern "C" int erh_mv_bits(int dx, int dy) { return er::mv_bits(dx, dy); }
extern "C" int erh_lambda16(int qp, int mv_lambda16) { return er::lambda16(qp, mv_lambda16); }

// the key of a candidate: vector (vx, vy), predictor (px, py), quarter samples
extern "C" uint64_t erh_key(uint32_t sad, int lam16, int vx, int vy, int px, int py, uint32_t index) {
  return er::key_of(er::cost16(sad, lam16, vx, vy, px, py), index, sad);
}
extern "C" uint64_t erh_key_of(uint32_t cost, uint32_t index, uint32_t sad) { return er::key_of(cost, index, sad); }
extern "C" uint32_t erh_key_index(uint64_t key) { return er::key_index(key); }
extern "C" uint32_t erh_key_sad(uint64_t key) { return er::key_sad(key); }

extern "C" void erh_pred(uint32_t left_prev, int mx, int j, int *out) {
  const er::Mv p = er::pred_of_cmd(left_prev, mx, j);
  out[0] = p.x;
  out[1] = p.y;
}

// The probe on one macroblock whose 16 luma and 8 chroma 4x4 residual blocks
// all equal x (raster): bit 0 a luma level, bit 1 a chroma AC level, bit 2 a
// chroma DC level is non-zero at residual QP qp (chroma at QPc of offset 0).
extern "C" int erh_probe(const int *x, int qp) {
  const int qpc = vts::full::qpc_of(qp, 0);
  int dc[4], r = 0;
  if (!er::all_zero_block(x, qp, nullptr)) r |= 1;
  if (!er::all_zero_block(x, qpc, &dc[0])) r |= 2;
  dc[1] = dc[2] = dc[3] = dc[0];
  if (!er::all_zero_chroma_dc(dc, qpc)) r |= 4;
  return r;
}
