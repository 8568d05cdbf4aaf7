// CPU harness of the device encoder's residual arithmetic (enc_residual.h,
// the header enc_search and enc_intra call): plain C entry points over the
// header's functions, each over n blocks, so that pytest can compare their
// values with numpy's.
// TEST INFRASTRUCTURE (tests/test_enc_residual_host.py).
#include <cstdint>

#include "enc_residual.h"

namespace eres = vts::full::eres;

namespace {
uint32_t pack4(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | (static_cast<uint32_t>(p[3]) << 24); }
void unpack4(uint32_t v, uint8_t *p) {
  for (int c = 0; c < 4; ++c) p[c] = static_cast<uint8_t>(v >> (8 * c));
}
}  // namespace

extern "C" void ersh_fwd4(int n, const int *x, int *w) {
  for (int b = 0; b < n; ++b) eres::fwd4(x + 16 * b, w + 16 * b);
}
// z raster, lv zig-zag (with dc_out: 15 AC levels, lv[15] = 0, and dc[b] the DC coefficient)
extern "C" void ersh_code_blocks(int n, const int *x, int qp, int dc_out, int *z, int *lv, int *dc, int *nz) {
  for (int b = 0; b < n; ++b)
    nz[b] = dc_out ? eres::code_block<true>(x + 16 * b, qp, z + 16 * b, lv + 16 * b, dc + b)
                   : eres::code_block<false>(x + 16 * b, qp, z + 16 * b, lv + 16 * b, nullptr);
}
extern "C" void ersh_chroma_dc(int n, const int *c, int qpc, int *lv, int *nz) {
  for (int b = 0; b < n; ++b) nz[b] = eres::code_chroma_dc(c + 4 * b, qpc, lv + 4 * b);
}
extern "C" void ersh_i16_dc(int n, const int *d, int qp, int *lv) {
  for (int b = 0; b < n; ++b) eres::code_i16_dc(d + 16 * b, qp, lv + 16 * b);
}
// the probe's predicates
extern "C" void ersh_all_zero(int n, const int *x, int qp, int dc_out, int *zero, int *dc) {
  for (int b = 0; b < n; ++b) zero[b] = eres::all_zero_block(x + 16 * b, qp, dc_out ? dc + b : nullptr);
}
extern "C" void ersh_all_zero_chroma_dc(int n, const int *c, int qpc, int *zero) {
  for (int b = 0; b < n; ++b) zero[b] = eres::all_zero_chroma_dc(c + 4 * b, qpc);
}
// source minus prediction through the packed rows
extern "C" void ersh_diff(int n, const uint8_t *src, const uint8_t *pred, int *x) {
  for (int b = 0; b < n; ++b)
    for (int r = 0; r < 4; ++r) eres::diff_row4(pack4(src + 16 * b + 4 * r), pack4(pred + 16 * b + 4 * r), x + 16 * b + 4 * r);
}
// an inter luma block: the levels z through the decoder's inverse path onto pred
extern "C" void ersh_recon_inter(int n, const int *z, int qp, const uint8_t *pred, uint8_t *out) {
  for (int b = 0; b < n; ++b) {
    int res[16];
    vts::full::scale_idct4(z + 16 * b, qp, false, res);
    for (int r = 0; r < 4; ++r) unpack4(eres::recon_row4(pack4(pred + 16 * b + 4 * r), res + 4 * r), out + 16 * b + 4 * r);
  }
}
// n chroma planes of 4 blocks: DC levels dcl[4], AC levels z (used when ac)
extern "C" void ersh_recon_chroma(int n, const int *dcl, const int *z, int ac, int qpc, const uint8_t *pred, uint8_t *out) {
  for (int p = 0; p < n; ++p)
    for (int k = 0; k < 4; ++k) {
      const int b = 4 * p + k;
      int res[16];
      eres::chroma_residual(dcl + 4 * p, k, z + 16 * b, ac != 0, qpc, res);
      for (int r = 0; r < 4; ++r) unpack4(eres::recon_row4(pack4(pred + 16 * b + 4 * r), res + 4 * r), out + 16 * b + 4 * r);
    }
}
// n Intra16x16 macroblocks of 16 blocks (by block row, column): DC levels
// dclev[16], AC levels z (used when ac), one prediction value per block row
// (splat over the packed row, as enc_intra does)
extern "C" void ersh_recon_i16(int n, const int *dclev, const int *z, int ac, int qp, const uint8_t *pred, uint8_t *out) {
  for (int m = 0; m < n; ++m) {
    int dcy[16];
    vts::full::i16_dc_inverse(dclev + 16 * m, qp, vts::full::level_scale(qp % 6, 0, 0), dcy);
    for (int k = 0; k < 16; ++k) {
      const int b = 16 * m + k;
      int res[16];
      eres::residual_dc_done(dcy[k], z + 16 * b, ac != 0, qp, res);
      for (int r = 0; r < 4; ++r) unpack4(eres::recon_row4(pred[4 * b + r] * 0x01010101u, res + 4 * r), out + 16 * b + 4 * r);
    }
  }
}
