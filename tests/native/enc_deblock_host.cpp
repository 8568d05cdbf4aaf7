// CPU harness of the encoder's in-loop deblocking decisions (enc_deblock.h,
// the header the enc_deblock kernel calls): one picture is filtered twice,
//   edh_walk: a scalar walk over the header's functions in the kernel's order
//             (per macroblock row, mx ascending; the vertical edges 0..3, then
//             the horizontal edges 1..3; luma lines, then the chroma lines of
//             edges 0 and 2),
//   edh_ref:  the general decoder's full::deblock_mb (recon_full.h) over
//             MbRecs that say the same thing, disable_deblocking_filter_idc 2
//             and one slice per macroblock row.
// TEST INFRASTRUCTURE (tests/test_enc_deblock_host.py compares the two).
#include <cstdint>
#include <cstring>
#include <vector>

#include "enc_deblock.h"
#include "recon_full.h"

using namespace vts;
namespace edb = vts::full::edb;

namespace {
constexpr int kCoefPerMb = 384;  // transcode.hip's level layout: luma 16 x 16 by luma4x4BlkIdx first
}

// pic: NV12, luma rows of 16 mbw bytes, then 8 mbh rows of Cb|Cr pairs.
// Returns the macroblocks with at least one filtered line.
extern "C" int64_t edh_walk(int mbw, int mbh, int qp, int alpha_div2, int beta_div2, const uint32_t *cmd,
                            const uint8_t *cbp, const int16_t *coef, uint8_t *pic) {
  const int pitch = 16 * mbw;
  uint8_t *Y = pic, *UV = pic + static_cast<int64_t>(pitch) * 16 * mbh;
  int64_t count = 0;
  for (int my = 0; my < mbh; ++my) {
    edb::Mb left = edb::mb_of_cmd(edb::kPcmCmd, 0);
    for (int mx = 0; mx < mbw; ++mx) {
      const int a = my * mbw + mx;
      const edb::Mb cur = edb::mb_of_cmd(cmd[a], edb::nz_of_levels(coef + static_cast<int64_t>(a) * kCoefPerMb, cbp[a]));
      bool filtered = false;
      for (int dir = 0; dir < 2; ++dir)
        for (int e = 0; e < 4; ++e) {
          if (e == 0 && (dir == 1 || mx == 0)) continue;
          const edb::Mb &p = e == 0 ? left : cur;
          const int qpp = edb::qp_of(p, qp), qpq = edb::qp_of(cur, qp);
          const edb::Idx xl = edb::indices(qpp, qpq, 2 * alpha_div2, 2 * beta_div2, false, 0);
          for (int k = 0; k < 16; ++k) {
            uint8_t *s = dir ? Y + static_cast<int64_t>(my * 16 + 4 * e) * pitch + mx * 16 + k
                             : Y + static_cast<int64_t>(my * 16 + k) * pitch + mx * 16 + 4 * e;
            filtered |= edb::filter(s, dir ? pitch : 1, edb::line_bs(p, cur, dir, e, k), false, xl);
          }
          if (e & 1) continue;
          const edb::Idx xc = edb::indices(qpp, qpq, 2 * alpha_div2, 2 * beta_div2, true, 0);
          for (int pl = 0; pl < 2; ++pl)
            for (int k = 0; k < 8; ++k) {
              uint8_t *s = dir ? UV + static_cast<int64_t>(my * 8 + 2 * e) * pitch + 2 * (mx * 8 + k) + pl
                               : UV + static_cast<int64_t>(my * 8 + k) * pitch + 2 * (mx * 8 + 2 * e) + pl;
              filtered |= edb::filter(s, dir ? pitch : 2, edb::line_bs(p, cur, dir, e, 2 * k), true, xc);
            }
        }
      count += filtered;
      left = cur;
    }
  }
  return count;
}

extern "C" void edh_ref(int mbw, int mbh, int qp, int alpha_div2, int beta_div2, const uint32_t *cmd,
                        const uint8_t *cbp, const int16_t *coef, uint8_t *pic) {
  static const int bx[16] = {0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3};
  static const int by[16] = {0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3};
  const int nmb = mbw * mbh;
  std::vector<MbRec> recs(static_cast<size_t>(nmb));
  std::vector<FullSlice> slices(static_cast<size_t>(mbh));
  for (int my = 0; my < mbh; ++my) {
    FullSlice &s = slices[my];
    std::memset(&s, 0, sizeof s);
    s.first_mb = my * mbw;
    s.qp = qp;
    s.is_p = 1;
    s.num_ref = 1;
    s.dbk_idc = 2;
    s.dbk_a = 2 * alpha_div2;
    s.dbk_b = 2 * beta_div2;
    s.ext = -1;
  }
  for (int a = 0; a < nmb; ++a) {
    MbRec &m = recs[a];
    std::memset(&m, 0, sizeof m);
    m.slice = static_cast<uint32_t>(a / mbw);
    m.qp = static_cast<uint8_t>(qp);
    const uint32_t c = cmd[a];
    if (c == 0x80008000u) {
      m.type = kMbPcm;
      m.qp = 0;
      std::memset(m.nz, 16, sizeof m.nz);
      std::memset(m.ref, -1, sizeof m.ref);
    } else if ((c >> 15) == 0x10000u) {  // high half 0x8000, bit 15 clear
      m.type = kMbI16;
      m.cbp = static_cast<uint8_t>((c >> 4) & 63);
      std::memset(m.ref, -1, sizeof m.ref);
    } else {
      const int mvx = static_cast<int16_t>(c & 0xffffu), mvy = static_cast<int16_t>(c >> 16);
      m.type = (mvx == 0 && mvy == 0 && cbp[a] == 0) ? kMbSkip : kMbInter;
      m.cbp = cbp[a];
      for (int k = 0; k < 16; ++k) {
        m.mv[k][0] = static_cast<int16_t>(mvx);
        m.mv[k][1] = static_cast<int16_t>(mvy);
        int n = 0;
        if ((cbp[a] >> (k >> 2)) & 1)
          for (int q = 0; q < 16; ++q) n += coef[static_cast<int64_t>(a) * kCoefPerMb + 16 * k + q] != 0;
        m.nz[by[k] * 4 + bx[k]] = static_cast<uint8_t>(n);
      }
    }
  }
  full::ReconCtx ctx{};
  ctx.recs = recs.data();
  ctx.slices = slices.data();
  ctx.surf = pic;
  ctx.frame_stride = static_cast<int64_t>(16 * mbw) * 16 * mbh * 3 / 2;
  ctx.pitch = 16 * mbw;
  ctx.uv_off = static_cast<int64_t>(16 * mbw) * 16 * mbh;
  ctx.mbw = mbw;
  ctx.mbh = mbh;
  for (int a = 0; a < nmb; ++a) full::deblock_mb(ctx, 0, a);
}
