// enc_residual.h — the residual arithmetic of the device encoder (transcode.hip:
// enc_search's probe and residual epilogue, enc_intra), written
// once for the kernels and for the CPU harnesses
// (tests/native/enc_residual_host.cpp, enc_rate_host.cpp).
//
//   forward:  W = Cf X Cf^T of a 4x4 residual block X (fwd4), levels
//             sign(W) min(2047, (|W| MF + f) >> qbits) with qbits = 15 + qp / 6
//             and f = 2^qbits / 6 (quant1); the DC terms that travel apart
//             (chroma 2x2, Intra16x16 luma 4x4) through their Hadamard and the
//             quantiser at (qbits + 1, 2f).
//   inverse:  the decoder's own scaling and transforms (recon_full.h:
//             level_scale, scale_idct4, i16_dc_inverse), so that the encoder's
//             reconstruction is the decoder's by construction.
//
// Blocks are raster (row i, column j) unless said otherwise.  Nothing here
// depends on the device; oracle/transcode_oracle.c restates it independently.
#pragma once
#include <cstdint>

#include "recon_full.h"

namespace vts {
namespace full {
namespace eres {

// flat-matrix MF of position (i, j), by class: both even, both odd, mixed
VTS_HD VTS_INLINE int pos_class(int i, int j) { return (!(i & 1) && !(j & 1)) ? 0 : ((i & 1) && (j & 1) ? 1 : 2); }
VTS_HD VTS_INLINE int mf_of(int qp, int i, int j) {
  constexpr int kMf[6][3] = {{13107, 5243, 8066}, {11916, 4660, 7490}, {10082, 4194, 6554},
                             {9362, 3647, 5825},  {8192, 3355, 5243},  {7282, 2893, 4559}};
  return kMf[qp % 6][pos_class(i, j)];
}
// One axis of the forward core transform Cf and of the 4x4 Hadamard: four
// terms in, four out at stride s
VTS_HD VTS_INLINE void cf4(int a, int b, int c, int d, int *o, int s) {
  o[0] = a + b + c + d;
  o[s] = 2 * a + b - c - 2 * d;
  o[2 * s] = a - b - c + d;
  o[3 * s] = a - 2 * b + 2 * c - d;
}
VTS_HD VTS_INLINE void had4(int a, int b, int c, int d, int *o, int s) {
  o[0] = a + b + c + d;
  o[s] = a + b - c - d;
  o[2 * s] = a - b - c + d;
  o[3 * s] = a - b + c - d;
}
VTS_HD VTS_INLINE void fwd4(const int *x, int *w) {  // W = Cf X Cf^T
  int t[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) cf4(x[i * 4], x[i * 4 + 1], x[i * 4 + 2], x[i * 4 + 3], t + i * 4, 1);
#pragma unroll
  for (int j = 0; j < 4; ++j) cf4(t[j], t[4 + j], t[8 + j], t[12 + j], w + j, 4);
}
VTS_HD VTS_INLINE int quant1(int w, int mf, int qbits, int64_t f) {
  const int64_t v = (static_cast<int64_t>(w < 0 ? -w : w) * mf + f) >> qbits;
  const int z = static_cast<int>(v < 2047 ? v : 2047);
  return w < 0 ? -z : z;
}
// the rounding offset f of a QP's quantiser
VTS_HD VTS_INLINE int64_t round_of(int qp) { return (int64_t(1) << (15 + qp / 6)) / 6; }

// A 4x4 residual block x at QP qp: z receives the levels, lv the same in
// zig-zag order; true when a level is non-zero.  With kDcOut the DC term is
// held out (chroma; Intra16x16 luma): *dc receives the coefficient, z[0] is 0
// and lv holds the 15 AC levels from index 0.
template <bool kDcOut>
VTS_HD VTS_INLINE bool code_block(const int *x, int qp, int *z, int *lv, int *dc) {
  int w[16];
  fwd4(x, w);
  constexpr int first = kDcOut ? 1 : 0;
  const int qbits = 15 + qp / 6;
  const int64_t f = round_of(qp);
  constexpr uint8_t kScan[16] = VTS_ZZ_DATA;  // 8.5.6 zig-zag, here so that the unrolled indices are constants
  bool nz = false;
  z[0] = 0;
  lv[15] = 0;
  if (kDcOut) *dc = w[0];
#pragma unroll
  for (int q = first; q < 16; ++q) {
    z[q] = quant1(w[q], mf_of(qp, q >> 2, q & 3), qbits, f);
    nz |= z[q] != 0;
  }
#pragma unroll
  for (int q = first; q < 16; ++q) lv[q - first] = z[kScan[q]];
  return nz;
}

// Term k of the 2x2 Hadamard of c (its own inverse up to scale): the forward
// transform of a chroma plane's four DC coefficients, and 8.5.11.1's f of
// their levels
VTS_HD VTS_INLINE int had2_at(const int *c, int k) {
  return k == 0 ? c[0] + c[1] + c[2] + c[3]
                : (k == 1 ? c[0] - c[1] + c[2] - c[3] : (k == 2 ? c[0] + c[1] - c[2] - c[3] : c[0] - c[1] - c[2] + c[3]));
}
// The four DC coefficients c of a chroma plane to their levels, quantised at
// (qbits + 1, 2f); true when one is non-zero
VTS_HD VTS_INLINE bool code_chroma_dc(const int *c, int qpc, int *lv) {
  bool nz = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    lv[k] = quant1(had2_at(c, k), mf_of(qpc, 0, 0), 15 + qpc / 6 + 1, 2 * round_of(qpc));
    nz |= lv[k] != 0;
  }
  return nz;
}
// The 16 DC coefficients of an Intra16x16 macroblock's luma blocks (by block
// row, column) to their levels: (H D H) / 2, quantised at (qbits + 1, 2f)
VTS_HD VTS_INLINE void code_i16_dc(const int *d, int qp, int *lv) {
  int t[16], h[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) had4(d[i * 4], d[i * 4 + 1], d[i * 4 + 2], d[i * 4 + 3], t + i * 4, 1);
#pragma unroll
  for (int j = 0; j < 4; ++j) had4(t[j], t[4 + j], t[8 + j], t[12 + j], h + j, 4);
#pragma unroll
  for (int k = 0; k < 16; ++k) lv[k] = quant1((h[k] + 1) >> 1, mf_of(qp, 0, 0), 15 + qp / 6 + 1, 2 * round_of(qp));
}

// ---- the early P_Skip probe's predicates: a level is zero iff the
// quantiser above says so
// A 4x4 residual block x at QP qp: true when every level is zero.  Luma
// (dc == nullptr): all 16; chroma: the 15 AC levels, and *dc receives the DC
// coefficient for all_zero_chroma_dc.
VTS_HD VTS_INLINE bool all_zero_block(const int *x, int qp, int *dc) {
  int z[16], lv[16];
  return !(dc ? code_block<true>(x, qp, z, lv, dc) : code_block<false>(x, qp, z, lv, nullptr));
}
VTS_HD VTS_INLINE bool all_zero_chroma_dc(const int *c, int qpc) {
  int lv[4];
  return !code_chroma_dc(c, qpc, lv);
}

// ---- reconstruction
// The residual of a block whose DC arrives already scaled (8.5.12 with
// dc_done): its AC levels z when ac, else none
VTS_HD VTS_INLINE void residual_dc_done(int dc_scaled, const int *z, bool ac, int qp, int *res) {
  int c[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) c[q] = ac ? z[q] : 0;
  c[0] = dc_scaled;
  scale_idct4(c, qp, true, res);
}
// The residual of chroma block k of a plane from the plane's DC levels dcl
// (8.5.11.1, 8.5.11.2) and the block's AC levels z (when ac)
VTS_HD VTS_INLINE void chroma_residual(const int *dcl, int k, const int *z, bool ac, int qpc, int *res) {
  residual_dc_done(((had2_at(dcl, k) * level_scale(qpc % 6, 0, 0)) << (qpc / 6)) >> 5, z, ac, qpc, res);
}

// ---- one row of a block in the packed-byte rows the kernels keep in LDS:
// source s minus prediction p, and Clip1(prediction + residual)
VTS_HD VTS_INLINE int byte_of(uint32_t v, int c) { return static_cast<int>((v >> (8 * c)) & 255u); }
VTS_HD VTS_INLINE void diff_row4(uint32_t s, uint32_t p, int *x) {
#pragma unroll
  for (int c = 0; c < 4; ++c) x[c] = byte_of(s, c) - byte_of(p, c);
}
VTS_HD VTS_INLINE uint32_t recon_row4(uint32_t p, const int *res) {
  uint32_t o = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) o |= static_cast<uint32_t>(clip1(byte_of(p, c) + res[c])) << (8 * c);
  return o;
}

}  // namespace eres
}  // namespace full
}  // namespace vts
