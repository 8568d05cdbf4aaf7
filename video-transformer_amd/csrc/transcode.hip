// transcode.hip — the kernels of vts_transcode, the 360p upload transcode on
// the device (replaces the pixel work of the reference's
// ContentAnalyzer._compress_video_for_upload, content_analyzer.py:167-236,
// `ffmpeg -vf scale=-2:360 -c:v libx264 -crf 28`), and one launch function per
// stage (transcode.h).  The host driver that queues them is
// transcode_driver.cpp, the downscale that feeds them downscale.hip.
// DESIGN.md §11.
//
// Pipeline, all device work after the one decode:
//   1. the session's decode + score run (run_all), with `small_window`
//      downscaling every window's frames (area filter, NV12 -> NV12 at
//      (w, 360), coded 16-aligned) into a whole-video store while they sit
//      in the decode ring;
//   2. GOP plan on the host (enc_plan.h): IDR at frame 0 and every `keyint`
//      frames (and, opt-in, at every scene cut from the scores);
//   3. per GOP position j ("level", every GOP at once, as the decoder's
//      reconstruct levels): `enc_search` — one wave per macroblock, full
//      integer motion search in LDS against the previous reconstruction
//      (opt-in, vts_transcode_ext.subpel: refined to half / quarter samples),
//      decision inter / I_PCM, reconstruction written (the next level's
//      reference); with intra = 1, `enc_intra` — one wave per macroblock
//      row recodes the level's I_PCM macroblocks (level 0: the whole IDR
//      picture) as Intra16x16 where cheaper, and `enc_hash` hashes the
//      level's reconstruction; then per chunk of 16 levels on a second stream:
//      `enc_write` — one lane per slice (macroblock row) writes the CAVLC
//      slice NAL with emulation prevention into a fixed-capacity staging slot,
//      leaving I_PCM payloads as gaps (opt-in, vts_transcode_ext4.cabac:
//      `enc_write_cabac` — one wave per slice writes it as CABAC through
//      enc_cabac.h instead); `enc_scan` — device offsets;
//      `enc_gather` + `enc_pcm` — packed output, one D2H copy per chunk;
//      opt-in (vts_transcode_ext7): every stage reads a picture's QP from a
//      per-frame array, and with a bitrate `enc_rc` — one thread per GOP
//      between two levels sets the next picture's QP (enc_ratectl.h);
//      opt-in (vts_transcode_ext9): `enc_aq` — ahead of level 0, four
//      macroblocks a wave — gives every macroblock a QP offset from its
//      source samples (enc_aq.h), every stage codes it at its own QP and the
//      writers send mb_qp_delta;
//   4. host: MP4 mux (Mp4Writer) in display order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "enc_aq.h"
#include "enc_cabac.h"
#include "enc_cavlc.h"
#include "enc_deblock.h"
#include "enc_part.h"
#include "enc_rate.h"
#include "enc_ratectl.h"
#include "recon_full.h"
#include "transcode.h"

namespace vts {
namespace {

using full::edb::kPcmCmd;  // (mvx, mvy) = (-32768, -32768): never a motion (enc_deblock.h)
constexpr int kWinPitch = 16 + 2 * kMaxRange + 4;  // LDS window row pitch (bytes)
// Sub-sample refinement (vts_transcode_ext.subpel): the window grows by the
// 6-tap filter's reach around every integer candidate, 2 + 1 samples before
// (the fraction may step below the integer winner) and 3 after; the low
// column margin is 4 so that the integer pass keeps its dword alignment.
constexpr int kSpLoX = 4, kSpLoY = 3, kSpHi = 3;
constexpr int kWinPitchSp = 16 + 2 * kMaxRange + 12;  // >= 4 ceil((16 + 2 R + kSpLoX + kSpHi) / 4), + a dword
constexpr int kSpPitch = 20;                          // half-sample plane row pitch: 18 samples, 5 dwords

// ------------------------------------------------------ residual coding
// Quantised residual of P_L0_16x16 macroblocks: the forward
// core transform W = Cf X Cf^T, levels sign(W) min(2047, (|W| MF + f) >>
// qbits) with qbits = 15 + qp / 6 and f = 2^qbits / 6 (chroma DC through the
// 2x2 Hadamard at qbits + 1 and 2f), the decoder's own scaling + inverse
// transform (full::scale_idct4) for the reconstruction, and CAVLC
// residual_block (9.2, enc_cavlc.h) for the bits.  Restated in
// oracle/transcode_oracle.c.
constexpr int kPcmBits = 3072;   // I_PCM payload: a residual bounded above it is not worth coding
__device__ __constant__ static const uint8_t kZz4[16] = VTS_ZZ_DATA;
__device__ __constant__ static const uint8_t kQpcTab[52] = VTS_QPC_DATA;
__device__ __constant__ static const uint8_t kBlkXd[16] = {0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3};
__device__ __constant__ static const uint8_t kBlkYd[16] = {0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3};
namespace er = full::erate;
namespace eres = full::eres;  // the transform, the quantiser and the reconstruction (enc_residual.h)
namespace ei4 = full::ei4;    // the Intra_4x4 decisions (enc_intra4.h)
namespace ecav = full::ecav;  // the CAVLC slice writer and its bit counts (enc_cavlc.h)
namespace ep = full::epart;   // the inter partitions (enc_part.h)
namespace eaq = full::eaq;    // adaptive quantisation: the law and the running-QP rule (enc_aq.h)

// ------------------------------------------------------ motion search
__device__ __forceinline__ uint32_t u32_at(const uint8_t *lds_row, int off) {  // 4 bytes at any offset
  const uint32_t *p = reinterpret_cast<const uint32_t *>(lds_row + (off & ~3));
  return __builtin_amdgcn_alignbyte(p[1], p[0], off & 3);  // byte shift
}

// enc_search, one wave per macroblock, in stages (each a function below, in
// the kernel's order): the early P_Skip probe; the window load — the
// reference window (16 + 2R)^2 and the source block go to LDS; the integer
// search — each lane takes candidates, the least key is a 64-bit min over
// the wave; the sub-sample refinement; the chroma prediction; and one of two
// epilogues, without or with residual coding.

// Window margins and row pitch by SP
template <int SP>
struct WinGeo {
  static constexpr int LX = SP ? kSpLoX : 0, LY = SP ? kSpLoY : 0, HI = SP ? kSpHi : 0;
  static constexpr int WP = SP ? kWinPitchSp : kWinPitch;
  static constexpr int kBytes = (16 + 2 * kMaxRange + LY + HI) * WP;
};

// The key every pass orders its candidates by: make(sad, index, vx, vy) of
// the candidate vector (vx, vy) in quarter samples, and the winner's index
// and SAD back out of the reduced key.  RC: (16 SAD + lambda16 bits(v - p),
// index) with the SAD riding below (enc_rate.h); else (SAD, index).
template <bool RC>
struct SearchKey {
  int lam16 = 0;   // RC: 0 orders the candidates as the SAD alone
  er::Mv p{0, 0};  // RC: the predictor guess, quarter samples
  __device__ __forceinline__ uint64_t make(uint32_t sad, uint32_t index, int vx, int vy) const {
    if constexpr (RC) return er::key_of(er::cost16(sad, lam16, vx, vy, p.x, p.y), index, sad);
    else return (static_cast<uint64_t>(sad) << 32) | index;
  }
  __device__ __forceinline__ static uint32_t index(uint64_t key) { return RC ? er::key_index(key) : static_cast<uint32_t>(key); }
  __device__ __forceinline__ static uint32_t sad(uint64_t key) { return RC ? er::key_sad(key) : static_cast<uint32_t>(key >> 32); }
};

// Integer candidates: index 0 is the centre, the others follow in raster
// order of the (2R + 1)^2 square (position r)
__device__ __forceinline__ int cand_of_raster(int r, int center) { return r == center ? 0 : (r < center ? r + 1 : r); }
__device__ __forceinline__ int raster_of_cand(int c, int center) { return c == 0 ? center : (c - 1 < center ? c - 1 : c); }

// Where a lane's samples of macroblock (mx, my) lie in a picture: 4 luma
// samples of row lane / 4, and one Cb|Cr pair of chroma row lane / 8
__device__ __forceinline__ int64_t luma_off(const SearchArgs &a, int lane, int mx, int my) {
  return static_cast<int64_t>(my * 16 + (lane >> 2)) * a.cw + mx * 16 + 4 * (lane & 3);
}
__device__ __forceinline__ int64_t chroma_off(const SearchArgs &a, int lane, int mx, int my) {
  return static_cast<int64_t>(a.cw) * a.ch + static_cast<int64_t>(my * 8 + (lane >> 3)) * a.cw + 2 * (mx * 8 + (lane & 7));
}

// The 4x4 residual blocks of a macroblock in the layout every residual stage
// uses: lanes 0..15 the luma blocks (luma4x4BlkIdx), lanes 16..23 the chroma
// blocks (plane pl, block k).  They take the prediction from y(row, bx), the 4
// packed luma samples of row `row` in 4x4 column bx, and c(pl, i), sample i
// (raster 8x8) of chroma plane pl.
// Inter: the prediction (and the chroma source) in LDS, in the lanes' own
// layout (luma_off / chroma_off)
struct MbPred {
  uint32_t py[64];
  uint16_t pc[64], srcc[64];
  __device__ __forceinline__ uint32_t y(int row, int bx) const { return py[row * 4 + bx]; }
  __device__ __forceinline__ int c(int pl, int i) const { return eres::byte_of(pc[i], pl); }
};
// Intra16x16: both modes are constant along a row
struct IntraPred {
  const int *py, (*pc)[8];  // per row: luma [16], chroma [plane][8]
  __device__ __forceinline__ uint32_t y(int row, int) const { return static_cast<uint32_t>(py[row]) * 0x01010101u; }
  __device__ __forceinline__ int c(int pl, int i) const { return pc[pl][i >> 3]; }
};
struct ChromaLane {
  int pl, k, bx, by;  // (bx, by): the block's first sample in the 8x8 plane
};
__device__ __forceinline__ ChromaLane chroma_lane(int lane) {
  const int k = (lane - 16) & 3;
  return {(lane - 16) >> 2, k, (k & 1) * 4, (k >> 1) * 4};
}
// lane < 16: the luma block's residual, and its reconstruction into recy
template <class Pred>
__device__ __forceinline__ void luma_block_diff(int lane, const uint32_t *srcy, const Pred &pred, int *x) {
  const int bx = kBlkXd[lane], by = kBlkYd[lane];
#pragma unroll
  for (int r = 0; r < 4; ++r) eres::diff_row4(srcy[(by * 4 + r) * 4 + bx], pred.y(by * 4 + r, bx), x + 4 * r);
}
template <class Pred>
__device__ __forceinline__ void luma_block_recon(int lane, const Pred &pred, const int *res, uint32_t *recy) {
  const int bx = kBlkXd[lane], by = kBlkYd[lane];
#pragma unroll
  for (int r = 0; r < 4; ++r) recy[(by * 4 + r) * 4 + bx] = eres::recon_row4(pred.y(by * 4 + r, bx), res + 4 * r);
}
// lane 16..23: the chroma block's residual; its AC levels (true: one is
// non-zero) with the DC coefficient to dcw[pl][k]; its reconstruction into
// recc[pl] from the plane's DC levels dcl[pl] and (ac) those AC levels
template <class Pred>
__device__ __forceinline__ ChromaLane chroma_block_diff(int lane, const uint16_t *srcc, const Pred &pred, int *x) {
  const ChromaLane cl = chroma_lane(lane);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = (cl.by + r) * 8 + cl.bx + c;
      x[r * 4 + c] = eres::byte_of(srcc[i], cl.pl) - pred.c(cl.pl, i);
    }
  return cl;
}
template <class Pred>
__device__ __forceinline__ bool chroma_block_code(int lane, const uint16_t *srcc, const Pred &pred, int qpc, int *z, int *lv,
                                                  int (*dcw)[4]) {
  int x[16];
  const ChromaLane cl = chroma_block_diff(lane, srcc, pred, x);
  return eres::code_block<true>(x, qpc, z, lv, &dcw[cl.pl][cl.k]);
}
template <class Pred>
__device__ __forceinline__ void chroma_block_recon(int lane, const Pred &pred, const int (*dcl)[4], const int *z, bool ac,
                                                   int qpc, uint8_t (*recc)[64]) {
  const ChromaLane cl = chroma_lane(lane);
  int res[16];
  eres::chroma_residual(dcl[cl.pl], cl.k, z, ac, qpc, res);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = (cl.by + r) * 8 + cl.bx + c;
      recc[cl.pl][i] = static_cast<uint8_t>(full::clip1(pred.c(cl.pl, i) + res[r * 4 + c]));
    }
}
// chroma coded_block_pattern class: 2 with an AC level (ballot bits 16..23), 1 with a DC level only
__device__ __forceinline__ int chroma_cbp(uint64_t nzm, const int (*dcl)[4]) {
  bool dcnz = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) dcnz |= dcl[k >> 2][k & 3] != 0;
  return ((nzm >> 16) & 0xffu) ? 2 : (dcnz ? 1 : 0);
}
// the chroma levels the slice writer codes: lanes 16..23 the AC blocks, 24 / 25 the planes' DC
__device__ __forceinline__ void store_chroma_levels(int16_t *cp, int lane, const int *lv, const int (*dcl)[4]) {
  if (lane >= 16 && lane < 24) {
#pragma unroll
    for (int q = 0; q < 15; ++q) cp[264 + 15 * (lane - 16) + q] = static_cast<int16_t>(lv[q]);
  } else if (lane >= 24 && lane < 26) {
#pragma unroll
    for (int q = 0; q < 4; ++q) cp[256 + 4 * (lane - 24) + q] = static_cast<int16_t>(dcl[lane - 24][q]);
  }
}

// ---- stage: early P_Skip.  The co-located prediction (vector (0, 0);
// chroma 8.4.2.2.2 at (0, 0) is the co-located sample) goes through the
// residual path's transform and quantiser; with no level left the macroblock
// is decided before the window is loaded: true, and everything is written
__device__ __forceinline__ bool probe_skip(const SearchArgs &a, int lane, int64_t mbi, int mx, int my, const uint8_t *src,
                                           const uint8_t *ref, uint8_t *dst, const uint32_t *srcy, MbPred &P) {
  __shared__ int edc[2][4];
  const int64_t lo = luma_off(a, lane, mx, my), co = chroma_off(a, lane, mx, my);
  const uint32_t py = *reinterpret_cast<const uint32_t *>(ref + lo);
  const uint16_t pc = *reinterpret_cast<const uint16_t *>(ref + co);
  P.py[lane] = py;
  P.pc[lane] = pc;
  P.srcc[lane] = *reinterpret_cast<const uint16_t *>(src + co);
  __syncthreads();
  const int qpc = kQpcTab[a.qp];
  bool nz = false;
  if (lane < 16) {
    int x[16];
    luma_block_diff(lane, srcy, P, x);
    nz = !eres::all_zero_block(x, a.qp, nullptr);
  } else if (lane < 24) {
    int x[16], dc;  // a local: its address is known not to be null
    const ChromaLane cl = chroma_block_diff(lane, P.srcc, P, x);
    nz = !eres::all_zero_block(x, qpc, &dc);
    edc[cl.pl][cl.k] = dc;
  }
  __syncthreads();
  if (lane == 16 || lane == 17) nz |= !eres::all_zero_chroma_dc(edc[lane - 16], qpc);
  if (__ballot(nz) != 0) return false;
  // wave-uniform: P_Skip, the reconstruction is the prediction
  *reinterpret_cast<uint32_t *>(dst + lo) = py;
  *reinterpret_cast<uint16_t *>(dst + co) = pc;
  if (lane == 0) {
    a.cmd[mbi] = 0;
    a.cbp[mbi] = 0;
    atomicAdd(a.es_stat, 1ull);
  }
  return true;
}

// ---- stage: the window load.  Rows of W4 dwords (one division per lane,
// then carry stepping); a dword wholly inside the picture row and aligned
// (R % 4 == 0) is one load, else 4 edge-clamped byte loads
template <int SP>
__device__ __forceinline__ void load_window(const SearchArgs &a, int lane, const uint8_t *ref, int mx, int my, uint8_t *win) {
  using G = WinGeo<SP>;
  const int R = a.range, wsz = 16 + 2 * R + G::LX + G::HI, wrows = 16 + 2 * R + G::LY + G::HI;
  const int x0 = mx * 16 - R - G::LX, y0 = my * 16 - R - G::LY;
  const int W4 = (wsz + 3) >> 2, total = wrows * W4;
  int r = lane / W4, cd = lane - r * W4;
  const int dr = 64 / W4, dc = 64 - dr * W4;
  for (int k = lane; k < total; k += 64) {
    const uint8_t *rowp = ref + static_cast<int64_t>(min(max(y0 + r, 0), a.ch - 1)) * a.cw;
    const int sx = x0 + 4 * cd;
    uint32_t v;
    if (sx >= 0 && sx + 3 < a.cw && !(sx & 3)) {
      v = *reinterpret_cast<const uint32_t *>(rowp + sx);
    } else {
      v = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) v |= static_cast<uint32_t>(rowp[min(max(sx + q, 0), a.cw - 1)]) << (8 * q);
    }
    *reinterpret_cast<uint32_t *>(win + r * G::WP + 4 * cd) = v;
    r += dr;
    cd += dc;
    if (cd >= W4) {
      cd -= W4;
      ++r;
    }
  }
}

// ---- stage: the integer search.  The window holds edge-clamped samples:
// every candidate is valid.  The winner's offset and luma SAD.
struct IntegerMv {
  int dx, dy;
  uint32_t sad;
};
template <int RT, int SP, bool RC>
__device__ __forceinline__ IntegerMv integer_search(int lane, int R, const uint8_t *win, const uint32_t *srcy,
                                                    const SearchKey<RC> &key) {
  using G = WinGeo<SP>;
  constexpr int LX = G::LX, LY = G::LY, WP = G::WP;
  const int side = 2 * R + 1, ncand = side * side, center = R * side + R;
  uint64_t best = ~0ull;
  if constexpr (RT > 0) {
    // Register blocking: lane (gx, gy) owns the NB candidates dx = gx - R,
    // dy in [gy NB, gy NB + NB) - R.  Each of their 16 + NB - 1 window rows is
    // read from LDS once (5 dwords, 4 byte-aligns) and SAD'd against every
    // source row it meets (a broadcast LDS read per use): ~4.6x fewer LDS
    // reads and ~2x fewer VALU instructions than one candidate per pass.
    constexpr int SIDE = 2 * RT + 1, NG = 64 / SIDE, NB = (SIDE + NG - 1) / NG;
    const int gx = lane % SIDE, gy = lane / SIDE, dy0 = gy * NB;
    if (gy < NG && dy0 < SIDE) {
      uint32_t acc[NB];
#pragma unroll
      for (int g = 0; g < NB; ++g) acc[g] = 0;
      const int sh = gx & 3;
      const uint32_t *wb = reinterpret_cast<const uint32_t *>(win + (dy0 + LY) * WP + LX + (gx & ~3));
#pragma unroll 2
      for (int w = 0; w < 16 + NB - 1; ++w) {
        const uint32_t *wr = wb + w * (WP / 4);
        const uint32_t w0 = wr[0], w1 = wr[1], w2 = wr[2], w3 = wr[3], w4 = wr[4];
        const uint32_t r0 = __builtin_amdgcn_alignbyte(w1, w0, sh), r1 = __builtin_amdgcn_alignbyte(w2, w1, sh);
        const uint32_t r2 = __builtin_amdgcn_alignbyte(w3, w2, sh), r3 = __builtin_amdgcn_alignbyte(w4, w3, sh);
#pragma unroll
        for (int g = 0; g < NB; ++g) {
          const int yy = w - g;
          if (yy >= 0 && yy < 16) {
            const uint4 q = reinterpret_cast<const uint4 *>(srcy)[yy];  // broadcast read
            acc[g] = __builtin_amdgcn_sad_u8(r0, q.x, acc[g]);
            acc[g] = __builtin_amdgcn_sad_u8(r1, q.y, acc[g]);
            acc[g] = __builtin_amdgcn_sad_u8(r2, q.z, acc[g]);
            acc[g] = __builtin_amdgcn_sad_u8(r3, q.w, acc[g]);
          }
        }
      }
#pragma unroll
      for (int g = 0; g < NB; ++g) {
        const int dyi = dy0 + g;
        if (dyi < SIDE) {
          const uint64_t k = key.make(acc[g], cand_of_raster(dyi * SIDE + gx, center), 4 * (gx - RT), 4 * (dyi - RT));
          best = k < best ? k : best;
        }
      }
    }
  } else {
    for (int c = lane; c < ncand; c += 64) {
      const int r = raster_of_cand(c, center);
      const int dy = r / side - R, dx = r % side - R;
      uint32_t s = 0;
      const int ox = dx + R, sh = ox & 3;
      // per row: the 5 dwords covering the 16 candidate bytes, 4 byte-aligns,
      // the source row as one 16-byte broadcast read, 4 v_sad_u8
      const uint32_t *wr = reinterpret_cast<const uint32_t *>(win + (dy + R + LY) * WP + LX + (ox & ~3));
      const uint4 *sr = reinterpret_cast<const uint4 *>(srcy);
#pragma unroll 4
      for (int yy = 0; yy < 16; ++yy) {
        const uint32_t *w = wr + yy * (WP / 4);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
        const uint4 sv = sr[yy];
        s = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w1, w0, sh), sv.x, s);
        s = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w2, w1, sh), sv.y, s);
        s = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w3, w2, sh), sv.z, s);
        s = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w4, w3, sh), sv.w, s);
      }
      const uint64_t k = key.make(s, c, 4 * dx, 4 * dy);
      best = k < best ? k : best;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor(best, off);
    best = o < best ? o : best;
  }
  const int r = raster_of_cand(static_cast<int>(key.index(best)), center);
  return {r % side - R, r / side - R, key.sad(best)};
}

// ---- stage: the integer search with partitions (PT).  The same candidates
// and LDS reads, but a candidate's SAD is kept as four quadrant sums (left /
// right: the row's dwords 0, 1 against 2, 3; top / bottom: the source row),
// from which each of enc_part.h's nine blocks takes its own; nine 64-bit
// minima over the wave instead of one.  The rate term is the candidate's own,
// the same for every block: they share the macroblock's predictor guess.
struct PartMv {
  uint64_t key[ep::kBlocks];  // the winning key of every block
};
__device__ __forceinline__ void part_take(uint64_t *best, const uint32_t *q, uint32_t index, uint32_t rate) {
#pragma unroll
  for (int b = 0; b < ep::kBlocks; ++b) {
    const uint32_t sad = ep::block_sad(q, b);
    const uint64_t k = er::key_of(16u * sad + rate, index, sad);
    best[b] = k < best[b] ? k : best[b];
  }
}
template <int RT, int SP>
__device__ __forceinline__ PartMv integer_search_part(int lane, int R, const uint8_t *win, const uint32_t *srcy,
                                                      const SearchKey<true> &key) {
  using G = WinGeo<SP>;
  constexpr int LX = G::LX, LY = G::LY, WP = G::WP;
  const int side = 2 * R + 1, ncand = side * side, center = R * side + R;
  PartMv m;
#pragma unroll
  for (int b = 0; b < ep::kBlocks; ++b) m.key[b] = ~0ull;
  const uint4 *sr = reinterpret_cast<const uint4 *>(srcy);
  if constexpr (RT > 0) {
    // integer_search's register blocking, in passes of at most PB candidate
    // rows a lane so that the 4 PB accumulators stay in registers; each half
    // of the source rows walks its own 8 + PB - 1 window rows
    constexpr int SIDE = 2 * RT + 1, NG = 64 / SIDE, NB = (SIDE + NG - 1) / NG, PB = NB < 6 ? NB : 6;
    const int gx = lane % SIDE, gy = lane / SIDE, dy0 = gy * NB;
    if (gy < NG && dy0 < SIDE) {
      const int sh = gx & 3;
      for (int p0 = 0; p0 < NB; p0 += PB) {
        const int nv = min(PB, min(NB - p0, SIDE - dy0 - p0));  // the pass's candidate rows
        if (nv <= 0) break;
        uint32_t acc[PB][4];
#pragma unroll
        for (int g = 0; g < PB; ++g) acc[g][0] = acc[g][1] = acc[g][2] = acc[g][3] = 0;
        const uint32_t *wb = reinterpret_cast<const uint32_t *>(win + (dy0 + p0 + LY) * WP + LX + (gx & ~3));
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll 2
          for (int w = 0; w < 8 + nv - 1; ++w) {
            const uint32_t *wr = wb + (w + 8 * h) * (WP / 4);
            const uint32_t w0 = wr[0], w1 = wr[1], w2 = wr[2], w3 = wr[3], w4 = wr[4];
            const uint32_t r0 = __builtin_amdgcn_alignbyte(w1, w0, sh), r1 = __builtin_amdgcn_alignbyte(w2, w1, sh);
            const uint32_t r2 = __builtin_amdgcn_alignbyte(w3, w2, sh), r3 = __builtin_amdgcn_alignbyte(w4, w3, sh);
#pragma unroll
            for (int g = 0; g < PB; ++g) {
              const int yy = w - g;
              if (yy >= 0 && yy < 8) {
                const uint4 q = sr[yy + 8 * h];  // broadcast read
                acc[g][2 * h] = __builtin_amdgcn_sad_u8(r0, q.x, acc[g][2 * h]);
                acc[g][2 * h] = __builtin_amdgcn_sad_u8(r1, q.y, acc[g][2 * h]);
                acc[g][2 * h + 1] = __builtin_amdgcn_sad_u8(r2, q.z, acc[g][2 * h + 1]);
                acc[g][2 * h + 1] = __builtin_amdgcn_sad_u8(r3, q.w, acc[g][2 * h + 1]);
              }
            }
          }
        }
#pragma unroll
        for (int g = 0; g < PB; ++g) {
          const int dyi = dy0 + p0 + g;
          if (g < nv) {
            const int vx = 4 * (gx - RT), vy = 4 * (dyi - RT);
            part_take(m.key, acc[g], cand_of_raster(dyi * SIDE + gx, center),
                      static_cast<uint32_t>(key.lam16) * static_cast<uint32_t>(er::mv_bits(vx - key.p.x, vy - key.p.y)));
          }
        }
      }
    }
  } else {
    for (int c = lane; c < ncand; c += 64) {
      const int r = raster_of_cand(c, center);
      const int dy = r / side - R, dx = r % side - R;
      uint32_t q4[4] = {0, 0, 0, 0};
      const int ox = dx + R, sh = ox & 3;
      const uint32_t *wr = reinterpret_cast<const uint32_t *>(win + (dy + R + LY) * WP + LX + (ox & ~3));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll 4
        for (int yy = 0; yy < 8; ++yy) {
          const uint32_t *w = wr + (yy + 8 * h) * (WP / 4);
          const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
          const uint4 sv = sr[yy + 8 * h];
          q4[2 * h] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w1, w0, sh), sv.x, q4[2 * h]);
          q4[2 * h] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w2, w1, sh), sv.y, q4[2 * h]);
          q4[2 * h + 1] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w3, w2, sh), sv.z, q4[2 * h + 1]);
          q4[2 * h + 1] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w4, w3, sh), sv.w, q4[2 * h + 1]);
        }
      }
      part_take(m.key, q4, static_cast<uint32_t>(c),
                static_cast<uint32_t>(key.lam16) * static_cast<uint32_t>(er::mv_bits(4 * dx - key.p.x, 4 * dy - key.p.y)));
    }
  }
#pragma unroll
  for (int b = 0; b < ep::kBlocks; ++b)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t o = __shfl_xor(m.key[b], off);
      m.key[b] = o < m.key[b] ? o : m.key[b];
    }
  return m;
}

// The prediction of quarter-sample offset (qx, qy) from an integer position
// (8.4.2.2.1, Table 8-12) in terms of the half-sample grid around it, where
// (X, Y) even/even is an integer sample G, odd/even b, even/odd h, odd/odd j:
// a position on the grid is that sample; any other is (p + q + 1) >> 1 of
// two grid neighbours, (XA, YA) and (XB, YB) — the horizontal or vertical
// pair when one component is even, else the two of the cell's four corners
// that are b / h samples.
__device__ __forceinline__ void sp_pair(int qx, int qy, int &XA, int &YA, int &XB, int &YB) {
  const int X0 = qx >> 1, Y0 = qy >> 1, ax = qx & 1, ay = qy & 1;
  if (ax && ay) {
    const int odd = (X0 + Y0) & 1;  // the corner (X0, Y0) is b or h
    XA = X0 + 1 - odd;
    YA = Y0;
    XB = X0 + odd;
    YB = Y0 + 1;
  } else {
    XA = X0;
    YA = Y0;
    XB = X0 + ax;
    YB = Y0 + ay;
  }
}
// rounding byte average of two dwords, no unpacking
__device__ __forceinline__ uint32_t avg_u8x4(uint32_t p, uint32_t q) { return (p | q) - (((p ^ q) >> 1) & 0x7f7f7f7fu); }

// What refine_and_predict works on: the whole macroblock, or with partitions
// one block of it (enc_part.h).  A type, not an argument: with WholeMb the
// function compiles to the code it was.
struct WholeMb {
  static constexpr bool kPart = false;
};
struct PartBlk {
  static constexpr bool kPart = true;
  ep::Rect r;
};
// ---- stage: the luma prediction at the winning vector, after (SP > 0) the
// sub-sample refinement around the integer winner w: (cqx, cqy) receives the
// refined vector in quarter samples from w; returned, the lane's 4 samples.
// PartBlk: the same for the block blk.r, called block after block
// (wave-uniform): w is the block's integer winner and its SAD, the planes are
// built around that winner as for a macroblock displaced by it, in the same
// LDS, and a candidate's SAD is taken over the block's samples alone; the
// returned samples are those of the macroblock at the block's vector.
template <int SP, bool RC, class Blk = WholeMb>
__device__ __forceinline__ uint32_t refine_and_predict(int lane, int R, const uint8_t *win, const uint32_t *srcy,
                                                       const IntegerMv &w, const SearchKey<RC> &key, int &cqx, int &cqy,
                                                       [[maybe_unused]] Blk blk = Blk{}) {
  constexpr bool PT = Blk::kPart;
  using G = WinGeo<SP>;
  constexpr int WP = G::WP;
  const int ly = lane >> 2, lx = 4 * (lane & 3);
  cqx = cqy = 0;
  if constexpr (SP == 0) {
    return u32_at(win + (w.dy + R + ly) * WP, w.dx + R + lx);
  } else {
    if constexpr (PT) __syncthreads();  // the lanes are done with the block before's planes
    // With (x, y) relative to the integer winner's block, whose sample (0, 0)
    // is win[oy][ox]: the half-sample planes b(x + 1/2, y), h(x, y + 1/2),
    // j(x + 1/2, y + 1/2) for every position a candidate of either step reads,
    // x, y in -1 .. 16 (the planes' index is x + 1, y + 1).  j is filtered from
    // the unclipped horizontal intermediates of rows -3 .. 18, which also give b.
    __shared__ int16_t hmid[22 * 18];
    __shared__ __attribute__((aligned(16))) uint8_t pb[18 * kSpPitch], ph[17 * kSpPitch], pj[17 * kSpPitch];
    const int ox = G::LX + R + w.dx, oy = G::LY + R + w.dy;
    for (int i = lane; i < 22 * 17; i += 64) {  // x = xx - 1 in -1 .. 15, row yy - 3
      const int yy = i / 17, xx = i - yy * 17;
      const uint8_t *p = win + (oy - 3 + yy) * WP + ox + xx - 3;
      const int t = full::tap6(p[0], p[1], p[2], p[3], p[4], p[5]);
      hmid[yy * 18 + xx] = static_cast<int16_t>(t);
      if (yy >= 2 && yy < 20) pb[(yy - 2) * kSpPitch + xx] = static_cast<uint8_t>(full::clip1((t + 16) >> 5));
    }
    for (int i = lane; i < 17 * 18; i += 64) {  // x = xx - 1 in -1 .. 16, y = yy - 1 in -1 .. 15
      const int yy = i / 18, xx = i - yy * 18;
      const uint8_t *p = win + (oy + yy - 3) * WP + ox + xx - 1;
      const int t = full::tap6(p[0], p[WP], p[2 * WP], p[3 * WP], p[4 * WP], p[5 * WP]);
      ph[yy * kSpPitch + xx] = static_cast<uint8_t>(full::clip1((t + 16) >> 5));
    }
    __syncthreads();
    for (int i = lane; i < 17 * 17; i += 64) {  // x = xx - 1, y = yy - 1 in -1 .. 15: rows yy .. yy + 5 of hmid
      const int yy = i / 17, xx = i - yy * 17;
      const int16_t *p = hmid + yy * 18 + xx;
      const int t = full::tap6(p[0], p[18], p[36], p[54], p[72], p[90]);
      pj[yy * kSpPitch + xx] = static_cast<uint8_t>(full::clip1((t + 512) >> 10));
    }
    __syncthreads();
    // One of the two grid samples a prediction averages: the 4-aligned LDS
    // row, byte offset and pitch at which its block row 0 starts
    struct Operand {
      const uint8_t *row;
      int off, pitch;
    };
    auto operand = [&](int X, int Y) -> Operand {  // X, Y in -2 .. 2
      const int cx = X >> 1, cy = Y >> 1;
      if (!((X | Y) & 1)) return {win + (oy + cy) * WP, ox + cx, WP};
      return {((X & 1) ? ((Y & 1) ? pj : pb) : ph) + (cy + 1) * kSpPitch, cx + 1, kSpPitch};
    };
    auto operands = [&](int qx, int qy, Operand &A, Operand &B) {
      int XA, YA, XB, YB;
      sp_pair(qx, qy, XA, YA, XB, YB);
      A = operand(XA, YA);
      B = operand(XB, YB);
    };
    // Per step the 8 candidates around the centre go to 8 lanes each (2 rows
    // a lane); the centre's SAD is known.  Index: centre 0, the others 1 .. 8
    // in raster order.
    uint32_t csad = w.sad;
    Operand A, B;
#pragma unroll
    for (int step = 2; step >= (SP == 2 ? 1 : 2); step >>= 1) {
      const int k = (lane >> 3) + 1, pos = k - 1 < 4 ? k - 1 : k;
      const int qx = cqx + step * (pos % 3 - 1), qy = cqy + step * (pos / 3 - 1);
      operands(qx, qy, A, B);
      uint32_t s = 0;
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const int row = 2 * (lane & 7) + rr;
        const uint32_t *wa = reinterpret_cast<const uint32_t *>(A.row + row * A.pitch + (A.off & ~3));
        const uint32_t *wb = reinterpret_cast<const uint32_t *>(B.row + row * B.pitch + (B.off & ~3));
        const uint4 sv = reinterpret_cast<const uint4 *>(srcy)[row];
        const uint32_t a0 = wa[0], a1 = wa[1], a2 = wa[2], a3 = wa[3], a4 = wa[4];
        const uint32_t b0 = wb[0], b1 = wb[1], b2 = wb[2], b3 = wb[3], b4 = wb[4];
        const int sa = A.off & 3, sb = B.off & 3;
        if constexpr (PT) {  // the block's rows and halves of a row only (wave-uniform block, per-lane row)
          uint32_t sl = 0, sr = 0;
          sl = __builtin_amdgcn_sad_u8(avg_u8x4(__builtin_amdgcn_alignbyte(a1, a0, sa), __builtin_amdgcn_alignbyte(b1, b0, sb)), sv.x, sl);
          sl = __builtin_amdgcn_sad_u8(avg_u8x4(__builtin_amdgcn_alignbyte(a2, a1, sa), __builtin_amdgcn_alignbyte(b2, b1, sb)), sv.y, sl);
          sr = __builtin_amdgcn_sad_u8(avg_u8x4(__builtin_amdgcn_alignbyte(a3, a2, sa), __builtin_amdgcn_alignbyte(b3, b2, sb)), sv.z, sr);
          sr = __builtin_amdgcn_sad_u8(avg_u8x4(__builtin_amdgcn_alignbyte(a4, a3, sa), __builtin_amdgcn_alignbyte(b4, b3, sb)), sv.w, sr);
          if (row >= blk.r.y && row < blk.r.y + blk.r.h) s += (blk.r.x == 0 ? sl : 0u) + (blk.r.x + blk.r.w == 16 ? sr : 0u);
          continue;
        }
        s = __builtin_amdgcn_sad_u8(avg_u8x4(__builtin_amdgcn_alignbyte(a1, a0, sa), __builtin_amdgcn_alignbyte(b1, b0, sb)), sv.x, s);
        s = __builtin_amdgcn_sad_u8(avg_u8x4(__builtin_amdgcn_alignbyte(a2, a1, sa), __builtin_amdgcn_alignbyte(b2, b1, sb)), sv.y, s);
        s = __builtin_amdgcn_sad_u8(avg_u8x4(__builtin_amdgcn_alignbyte(a3, a2, sa), __builtin_amdgcn_alignbyte(b3, b2, sb)), sv.z, s);
        s = __builtin_amdgcn_sad_u8(avg_u8x4(__builtin_amdgcn_alignbyte(a4, a3, sa), __builtin_amdgcn_alignbyte(b4, b3, sb)), sv.w, s);
      }
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      s += __shfl_xor(s, 4);
      // the centre's key is its own at this vector, not the integer pass's
      uint64_t best = key.make(s, k, 4 * w.dx + qx, 4 * w.dy + qy);
      const uint64_t ckey = key.make(csad, 0, 4 * w.dx + cqx, 4 * w.dy + cqy);
      best = ckey < best ? ckey : best;
#pragma unroll
      for (int off = 32; off >= 8; off >>= 1) {
        const uint64_t o = __shfl_xor(best, off);
        best = o < best ? o : best;
      }
      const int kw = static_cast<int>(key.index(best));
      if (kw) {  // wave-uniform
        const int pw = kw - 1 < 4 ? kw - 1 : kw;
        cqx += step * (pw % 3 - 1);
        cqy += step * (pw / 3 - 1);
        csad = key.sad(best);
      }
    }
    operands(cqx, cqy, A, B);
    return avg_u8x4(u32_at(A.row + ly * A.pitch, A.off + lx), u32_at(B.row + ly * B.pitch, B.off + lx));
  }
}

// ---- stage: the chroma prediction (8.4.2.2.2) of the lane's Cb|Cr pair at
// the quarter-sample luma vector (mvx, mvy); taps clamped to the picture as
// the decoder clamps them
struct ChromaPx {
  int u, v;
};
__device__ __forceinline__ ChromaPx chroma_pred(const SearchArgs &a, int lane, const uint8_t *ref, int mx, int my, int mvx,
                                                int mvy) {
  const int ci = lane & 7, cj = lane >> 3, fx = mvx & 7, fy = mvy & 7;
  const int ccw = a.cw / 2, cch = a.ch / 2;
  const uint8_t *ruv = ref + static_cast<int64_t>(a.cw) * a.ch;
  const int xi = mx * 8 + ci + (mvx >> 3), yi = my * 8 + cj + (mvy >> 3);
  const int xa = min(max(xi, 0), ccw - 1), xb = min(max(xi + 1, 0), ccw - 1);
  const int ya = min(max(yi, 0), cch - 1), yb = min(max(yi + 1, 0), cch - 1);
  const uint16_t A = *reinterpret_cast<const uint16_t *>(ruv + static_cast<int64_t>(ya) * a.cw + 2 * xa);
  const uint16_t B = *reinterpret_cast<const uint16_t *>(ruv + static_cast<int64_t>(ya) * a.cw + 2 * xb);
  const uint16_t Cc = *reinterpret_cast<const uint16_t *>(ruv + static_cast<int64_t>(yb) * a.cw + 2 * xa);
  const uint16_t D = *reinterpret_cast<const uint16_t *>(ruv + static_cast<int64_t>(yb) * a.cw + 2 * xb);
  const int wa = (8 - fx) * (8 - fy), wb = fx * (8 - fy), wc = (8 - fx) * fy, wd = fx * fy;
  return {(wa * (A & 255) + wb * (B & 255) + wc * (Cc & 255) + wd * (D & 255) + 32) >> 6,
          (wa * (A >> 8) + wb * (B >> 8) + wc * (Cc >> 8) + wd * (D >> 8) + 32) >> 6};
}

// What both epilogues decide between and where it goes: the lane's samples
// of the prediction and of the source, and the macroblock's vector
struct MbOut {
  uint8_t *dst;
  int64_t lo, co, mbi;  // luma_off, chroma_off, the macroblock's index in cmd / cbp / coef
  uint32_t py, sy4;
  uint16_t pc, suv;
  uint32_t mvw;  // the vector's word, mvx | mvy << 16
  int frac;      // mvx | mvy
  int frame;     // RC: the picture's frame number
  int mvbits;    // RC: the bits of the vectors the macroblock codes, against the predictor guess
};
// the macroblock's words: inter with its vector, else I_PCM
template <int SP>
__device__ __forceinline__ void write_words(const SearchArgs &a, const MbOut &o, bool inter, int cbp) {
  a.cmd[o.mbi] = inter ? o.mvw : kPcmCmd;
  if (a.cbp) a.cbp[o.mbi] = static_cast<uint8_t>(inter ? cbp : 0);
  if constexpr (SP > 0)
    if (inter && (o.frac & 3)) atomicAdd(&a.sp_stats[o.frac & 1], 1ull);
}

// ---- epilogue without residual coding: inter within max_sad, else I_PCM
template <int SP>
__device__ __forceinline__ void finish_plain(const SearchArgs &a, int lane, const MbOut &o, uint32_t cost) {
  const bool inter = a.max_sad >= 0 && cost <= static_cast<uint32_t>(a.max_sad);
  *reinterpret_cast<uint32_t *>(o.dst + o.lo) = inter ? o.py : o.sy4;
  *reinterpret_cast<uint16_t *>(o.dst + o.co) = inter ? o.pc : o.suv;
  if (lane == 0) write_words<SP>(a, o, inter, 0);
}

// ---- epilogue with residual coding: the blocks by lane as MbPred lays them
// out, then lanes 16 / 17 the chroma DC levels and 24 / 25 their bits; inter
// when the residual's CAVLC bound is within an I_PCM payload, else I_PCM;
// returned: inter
// RC: the macroblock's share of the picture's rate measure (a.est_f; NULL:
// none) is added: P_Skip 0, inter the bound plus its vectors' bits, I_PCM
// a.pcm_bits; false: the code is the epilogue's without it
template <int SP, bool RC = false>
__device__ __forceinline__ bool finish_residual(const SearchArgs &a, int lane, const MbOut &o, const uint32_t *srcy, MbPred &P) {
  __shared__ uint32_t recy[64];
  __shared__ uint8_t recc[2][64];
  __shared__ int dcw[2][4], dcl[2][4];
  P.py[lane] = o.py;
  P.pc[lane] = o.pc;
  P.srcc[lane] = o.suv;
  __syncthreads();
  const int qp = a.qp, qpc = kQpcTab[qp];
  int lv[16], z[16], nzb = 0, bits = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) lv[i] = z[i] = 0;
  if (lane < 16) {
    int x[16], res[16];
    luma_block_diff(lane, srcy, P, x);
    nzb = eres::code_block<false>(x, qp, z, lv, nullptr);
    full::scale_idct4(z, qp, false, res);
    luma_block_recon(lane, P, res, recy);
    bits = ecav::count_block(lv, 16, -2);
  } else if (lane < 24) {
    nzb = chroma_block_code(lane, P.srcc, P, qpc, z, lv, dcw);
  }
  __syncthreads();
  if (lane == 16 || lane == 17) eres::code_chroma_dc(dcw[lane - 16], qpc, dcl[lane - 16]);
  __syncthreads();
  const uint64_t nzm = __ballot(nzb);
  int cbp = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if ((nzm >> (4 * q)) & 15u) cbp |= 1 << q;
  const int cc = chroma_cbp(nzm, dcl);
  cbp |= cc << 4;
  int contrib = 0;  // this lane's share of the residual's CAVLC bound
  if (lane < 16) {
    contrib = ((cbp >> (lane >> 2)) & 1) ? bits : 0;
  } else if (lane < 24) {
    contrib = cc == 2 ? ecav::count_block(lv, 15, -2) : 0;
  } else if (lane < 26 && cc) {
    const int d4[4] = {dcl[lane - 24][0], dcl[lane - 24][1], dcl[lane - 24][2], dcl[lane - 24][3]};
    contrib = ecav::count_block(d4, 4, -1);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) contrib += __shfl_xor(contrib, off);
  const bool inter = contrib <= kPcmBits;
  if (lane >= 16 && lane < 24) chroma_block_recon(lane, P, dcl, z, cc == 2, qpc, recc);  // 8.5.11 DC, then 8.5.12
  __syncthreads();
  *reinterpret_cast<uint32_t *>(o.dst + o.lo) = inter ? recy[lane] : o.sy4;
  *reinterpret_cast<uint16_t *>(o.dst + o.co) = inter ? static_cast<uint16_t>(recc[0][lane] | (recc[1][lane] << 8)) : o.suv;
  if (inter && cbp) {  // the levels the slice writer codes
    int16_t *cp = a.coef + o.mbi * kCoefPerMb;
    if (lane < 16) {
#pragma unroll
      for (int q = 0; q < 16; ++q) cp[16 * lane + q] = static_cast<int16_t>(lv[q]);
    }
    store_chroma_levels(cp, lane, lv, dcl);
  }
  if (lane == 0) write_words<SP>(a, o, inter, cbp);
  if constexpr (RC) {
    if (a.est_f && lane == 0) {
      const int est = !inter ? a.pcm_bits : (cbp == 0 && o.mvw == 0 ? 0 : contrib + o.mvbits);
      if (est) atomicAdd(a.est_f + o.frame, static_cast<uint32_t>(est));
    }
  }
  return inter;
}

// RT: compile-time search range (register-blocked path), 0 = any range.
// SP: sub-sample refinement around the integer winner, 0 none (the code is
// the integer-only kernel's), 1 half samples, 2 half then quarter samples.
// RC: the rate-aware decisions of enc_rate.h, each switched by a bit of
// a.rate (wave-uniform), and with them the per-picture QP and the rate measure
// of vts_transcode_ext7 (a.qp_f, a.est_f; NULL: off, a runtime test each) and
// the macroblock's QP offset of vts_transcode_ext9 (a.aq_off, the same way);
// false: the code is the kernel's without them.  Every
// instance asks for 5 waves/SIMD: they fit (88 .. 90 VGPRs, no scratch), but
// left to itself the register allocator settles at 98 .. 102 and 4 waves.
// PT (with RC only): the inter partitions of enc_part.h.  The integer stage
// keeps every candidate's quadrant SADs and decides the shape from the nine
// blocks' winners; each block of that shape is refined on its own; every lane
// predicts its luma samples and its Cb|Cr pair with the vector of the quadrant
// they lie in, so the residual path sees one composite prediction; the four
// quadrant vectors go to a.mv4 and the macroblock is coded in their canonical
// shape.  These instances allow 4 waves/SIMD instead of asking for 5: those
// without refinement at R = 4, 8, 16 take 98 VGPRs and run 4, the other nine
// 88 .. 95 and 5; none uses scratch (profiles/part_resources.txt).
// false: the code is the kernel's without it.
template <int RT, int SP, bool RC, bool PT = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(PT ? 4 : 5))) enc_search(SearchArgs a) {
  static_assert(RC || !PT, "partitions need the vector cost");
  __shared__ __attribute__((aligned(16))) uint8_t win[WinGeo<SP>::kBytes];
  __shared__ __attribute__((aligned(16))) uint32_t srcy[64];
  __shared__ MbPred P;
  const int lane = threadIdx.x;
  const int64_t e = blockIdx.x / a.nmb;
  const int mb = static_cast<int>(blockIdx.x % a.nmb);
  const int mx = mb % a.mbw, my = mb / a.mbw;
  const int4 en = a.ent[e];
  const uint8_t *src = a.small + static_cast<int64_t>(en.x) * a.stride;
  const uint8_t *ref = en.y < 0 ? a.small + static_cast<int64_t>(en.x - 1) * a.stride
                                : a.recon + static_cast<int64_t>(en.y) * a.stride;
  MbOut o;
  o.dst = a.recon + static_cast<int64_t>(en.z) * a.stride;
  o.mbi = e * a.nmb + mb;
  srcy[lane] = *reinterpret_cast<const uint32_t *>(src + luma_off(a, lane, mx, my));
  SearchKey<RC> key;
  if constexpr (RC) {
    o.frame = en.x;
    o.mvbits = 0;
    if (a.qp_f) {  // wave-uniform: the picture's own QP, and the lambda that follows it
      a.qp = a.qp_f[en.x];
      a.lambda16 = er::lambda16(a.qp, a.mv_lambda16);
    }
    if (a.aq_off) {  // wave-uniform: the macroblock's own QP (enc_aq.h), and the lambda that follows it
      a.qp = eaq::qp_mb(a.qp, a.aq_off[static_cast<int64_t>(en.x) * a.nmb + mb], a.aq_lo, a.aq_hi);
      a.lambda16 = er::lambda16(a.qp, a.mv_lambda16);
    }
    const bool coded = a.qp >= 1 && a.max_sad >= 0;
    if (coded && (a.rate & 2) && probe_skip(a, lane, o.mbi, mx, my, src, ref, o.dst, srcy, P)) {
      if constexpr (PT)
        if (lane < 4) a.mv4[o.mbi * 4 + lane] = 0;
      return;
    }
    if (coded && (a.rate & 1)) {
      key.lam16 = a.lambda16;
      if constexpr (PT) {
        const int64_t lp = mx > 0 && a.gop_pos > 1 ? static_cast<int64_t>(en.w) * a.nmb + mb - 1 : -1;
        key.p = ep::pred_guess(lp >= 0 ? a.cmd_prev[lp] : 0u, lp >= 0 ? a.mv4_prev[lp * 4 + 1] : 0u, mx, a.gop_pos);
      } else {
        key.p = er::pred_of_cmd(mx > 0 && a.gop_pos > 1 ? a.cmd_prev[static_cast<int64_t>(en.w) * a.nmb + mb - 1] : 0u, mx,
                                a.gop_pos);
      }
    }
  }
  load_window<SP>(a, lane, ref, mx, my, win);
  __syncthreads();
  if constexpr (PT) {
    const int R = a.range, side = 2 * R + 1, center = R * side + R;
    const PartMv pm = integer_search_part<RT, SP>(lane, R, win, srcy, key);
    uint32_t cost9[ep::kBlocks];
#pragma unroll
    for (int b = 0; b < ep::kBlocks; ++b) cost9[b] = static_cast<uint32_t>(pm.key[b] >> 32);
    const int shape = ep::decide_shape(cost9, key.lam16);  // wave-uniform: it comes out of wave reductions
    const int lq = ep::quad_at(4 * (lane & 3), lane >> 2);  // the quadrant of the lane's luma samples
    uint32_t qv[4] = {0, 0, 0, 0};
    o.py = 0;
    for (int i = 0; i < ep::shape_blocks(shape); ++i) {  // wave-uniform
      const int b = ep::shape_first(shape) + i;
      uint64_t k = pm.key[0];
#pragma unroll
      for (int bb = 1; bb < ep::kBlocks; ++bb) k = bb == b ? pm.key[bb] : k;
      const int r = raster_of_cand(static_cast<int>(key.index(k)), center);
      const IntegerMv w{r % side - R, r / side - R, key.sad(k)};
      int cqx, cqy;
      const uint32_t py = refine_and_predict<SP, true, PartBlk>(lane, R, win, srcy, w, key, cqx, cqy, PartBlk{ep::block_rect(b)});
      const uint32_t word = ep::mv_word(4 * w.dx + cqx, 4 * w.dy + cqy);
      const int m = ep::block_quads(b);
#pragma unroll
      for (int q = 0; q < 4; ++q) qv[q] = ((m >> q) & 1) ? word : qv[q];
      o.py = ((m >> lq) & 1) ? py : o.py;
    }
    const int cshape = ep::canonical_shape(qv);
    o.mvw = cshape ? ep::part_cmd(cshape) : qv[0];
    const int fc = ep::frac_class(qv);
    o.frac = fc == 2 ? 1 : (fc == 1 ? 2 : 0);  // write_words: counted once, quarter before half
    o.sy4 = srcy[lane];
    const int cq = ep::quad_at(2 * (lane & 7), 2 * (lane >> 3));  // the quadrant of the lane's Cb|Cr pair
    const ep::Mv cv = ep::mv_of_word(cq == 0 ? qv[0] : (cq == 1 ? qv[1] : (cq == 2 ? qv[2] : qv[3])));
    const ChromaPx pc = chroma_pred(a, lane, ref, mx, my, cv.x, cv.y);
    o.pc = static_cast<uint16_t>(pc.u | (pc.v << 8));
    o.co = chroma_off(a, lane, mx, my);
    o.suv = *reinterpret_cast<const uint16_t *>(src + o.co);
    o.lo = luma_off(a, lane, mx, my);
    if (a.est_f) {  // wave-uniform: the measure is on; the vectors the canonical shape codes
      for (int i = 0; i < ep::shape_blocks(cshape); ++i) {
        const int q = ep::part_quad(cshape, i);
        const ep::Mv v = ep::mv_of_word(q == 0 ? qv[0] : (q == 1 ? qv[1] : (q == 2 ? qv[2] : qv[3])));
        o.mvbits += er::mv_bits(v.x - key.p.x, v.y - key.p.y);
      }
    }
    const bool inter = finish_residual<SP, true>(a, lane, o, srcy, P);
    if (lane < 4) a.mv4[o.mbi * 4 + lane] = !inter ? ep::kNoMv : (lane == 0 ? qv[0] : (lane == 1 ? qv[1] : (lane == 2 ? qv[2] : qv[3])));
    return;
  }
  const IntegerMv w = integer_search<RT, SP, RC>(lane, a.range, win, srcy, key);
  int cqx, cqy;
  o.py = refine_and_predict<SP, RC>(lane, a.range, win, srcy, w, key, cqx, cqy);
  const int mvx = 4 * w.dx + cqx, mvy = 4 * w.dy + cqy;
  o.mvw = static_cast<uint32_t>(static_cast<uint16_t>(mvx)) | (static_cast<uint32_t>(static_cast<uint16_t>(mvy)) << 16);
  o.frac = mvx | mvy;
  if constexpr (RC)
    if (a.est_f) o.mvbits = er::mv_bits(mvx - key.p.x, mvy - key.p.y);  // wave-uniform: the measure is on
  // the macroblock's cost at that vector: luma and chroma SAD
  o.sy4 = srcy[lane];
  uint32_t cost = __builtin_amdgcn_sad_u8(o.py, o.sy4, 0);
  const ChromaPx pc = chroma_pred(a, lane, ref, mx, my, mvx, mvy);
  o.pc = static_cast<uint16_t>(pc.u | (pc.v << 8));
  o.co = chroma_off(a, lane, mx, my);
  o.suv = *reinterpret_cast<const uint16_t *>(src + o.co);
  cost += static_cast<uint32_t>(abs(pc.u - (o.suv & 255)) + abs(pc.v - (o.suv >> 8)));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cost += __shfl_xor(cost, off);
  o.lo = luma_off(a, lane, mx, my);
  if (a.qp < 1 || a.max_sad < 0) finish_plain<SP>(a, lane, o, cost);
  else finish_residual<SP, RC>(a, lane, o, srcy, P);
}

// ------------------------------------------------------ slice writer
// RBSP bits -> EBSP bytes into a staging slot, four bytes per (aligned) dword
// store: slot payload (slot + 4), 4-byte aligned
using NalOut = full::erbsp::WordSink;

// ------------------------------------------------------ intra coding
// Intra16x16 in place of I_PCM (vts_transcode_params.intra).
// A slice is one macroblock row, so the row above is never available: luma
// predicts Horizontal (1) or DC (2) from the left macroblock's reconstructed
// right column, chroma DC (0) or Horizontal (1), and DC = 128 at mx = 0
// (8.3.3, 8.3.4).  Each row is a serial chain, so enc_intra is one wave per
// (level entry, macroblock row) walking mx = 0 .. mbw - 1; all ordering is
// program order inside that wave plus stream order between launches.
//
// Command word of an Intra16x16 macroblock: the high half 0x8000 (mvy =
// -32768: never a motion) with bit 15 clear; bits 0..1 Intra16x16PredMode,
// 2..3 intra_chroma_pred_mode, 4..9 coded_block_pattern (luma 0 or 15).
using full::edb::kIntraCmd;
using full::edb::is_intra_cmd;
// kI4 (vts_transcode_ext5.intra4x4, DESIGN.md §11 "Intra4x4"): every
// candidate macroblock is also tried as I_NxN with sixteen Intra_4x4 blocks,
// and that is what it becomes when its CAVLC bits are strictly fewer than the
// Intra16x16 candidate's; chroma is the same for both.  The sixteen blocks are
// a serial chain (a block predicts from the reconstruction of the ones before
// it, kept in an LDS tile), each of them spread over the wave: lanes 0..12
// fetch the block's 13 neighbouring samples, lanes 0..35 take (mode, row) =
// (lane / 4, lane % 4), predict that row (enc_intra4.h), v_sad_u8 it against
// the source and the quad sums the mode's SAD; the least (cost, mode) key is a
// 64-bit minimum over the wave; lane 0 transforms, quantises and reconstructs
// the block into the tile.  The levels wait in LDS for the bit count, which
// lanes 0..15 then take a block each as the Intra16x16 candidate's.
// false: the code is the kernel's without it.
// kAq (vts_transcode_ext9, enc_aq.h): a macroblock's QP is its own, from
// a.aq_off; false: the code is the kernel's without it (a runtime test of the
// pointer costs enc_intra<true> scratch).
template <bool kI4, bool kAq>
__global__ void __launch_bounds__(64) enc_intra(IntraArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t srcy[64], recy[64];
  __shared__ uint16_t srcc[64];
  __shared__ uint8_t recc[2][64];
  __shared__ int left_y[16], left_c[2][8];  // the left macroblock's right column (reconstruction)
  __shared__ int pred_y[16], pred_c[2][8];  // the chosen prediction of each row (both modes are constant along a row)
  __shared__ int lnz[4], lnzc[2][2];        // total_coeff of the left macroblock's right column, -1 none
  __shared__ int tcy[16], tcc[2][4];        // this macroblock's total_coeff, luma in raster order
  __shared__ int ydw[16], ydl[16], yds[16]; // luma DC: transform terms, levels, scaled (8.5.10), raster
  __shared__ int dcw[2][4], dcl[2][4];
  const int lane = threadIdx.x;
  const int e = blockIdx.x / a.mbh, my = blockIdx.x % a.mbh;
  const int4 en = a.ent[e];
  const uint8_t *src = a.small + static_cast<int64_t>(en.x) * a.stride;
  uint8_t *dst = a.recon + static_cast<int64_t>(en.z) * a.stride;
  const int64_t mb0 = (static_cast<int64_t>(e) * a.mbh + my) * a.mbw;
  const int qp_pic = a.qp_f ? a.qp_f[en.x] : a.qp, qpc_pic = kQpcTab[qp_pic];  // wave-uniform: the picture's own QP when given
  // kAq: every macroblock has its own QP, and the bits of its mb_qp_delta
  // follow the slice's running QP (enc_aq.h), which the walk keeps over the
  // macroblocks it does not code too
  const int8_t *aqr = kAq ? a.aq_off + (static_cast<int64_t>(en.x) * a.mbh + my) * a.mbw : nullptr;
  eaq::RunQp rq;
  rq.start(qp_pic);
  const int ly = lane >> 2, lx = 4 * (lane & 3), ci = lane & 7, cj = lane >> 3;
  uint32_t row_bits = 0;  // the rate measure of the macroblocks this wave decides (a.est_f)
  if (lane < 4) lnz[lane] = -1;
  if (lane < 4) lnzc[lane >> 1][lane & 1] = -1;
  bool left_mine = false;  // the left macroblock was coded by this wave: its column is in left_y / left_c
  [[maybe_unused]] uint64_t left_modes = ei4::kNoModes;  // kI4: the left macroblock's Intra4x4PredModes when it is I_NxN
  for (int mx = 0; mx < a.mbw; ++mx) {
    const int qp = kAq ? eaq::qp_mb(qp_pic, aqr[mx], a.aq_lo, a.aq_hi) : qp_pic, qpc = kAq ? kQpcTab[qp] : qpc_pic;  // wave-uniform
    if (!a.all && a.cmd[mb0 + mx] != kPcmCmd) {  // wave-uniform
      if constexpr (kAq) rq.step(a.cbp[mb0 + mx] != 0, qp);  // enc_search's: inter, its delta sent with a pattern
      left_mine = false;
      if constexpr (kI4) left_modes = ei4::kNoModes;
      continue;
    }
    const int64_t lo = static_cast<int64_t>(my * 16 + ly) * a.cw + mx * 16 + lx;
    const int64_t co = static_cast<int64_t>(a.cw) * a.ch + static_cast<int64_t>(my * 8 + cj) * a.cw + 2 * (mx * 8 + ci);
    const uint32_t sy4 = *reinterpret_cast<const uint32_t *>(src + lo);
    const uint16_t suv = *reinterpret_cast<const uint16_t *>(src + co);
    srcy[lane] = sy4;
    srcc[lane] = suv;
    if (mx > 0 && !left_mine) {
      // the left macroblock is enc_search's (an earlier launch): its column
      // from dst, its total_coeff from its levels as enc_write will count them
      if (lane < 16) {
        left_y[lane] = dst[static_cast<int64_t>(my * 16 + lane) * a.cw + mx * 16 - 1];
      } else if (lane < 24) {
        const uint16_t p = *reinterpret_cast<const uint16_t *>(
            dst + static_cast<int64_t>(a.cw) * a.ch + static_cast<int64_t>(my * 8 + lane - 16) * a.cw + 2 * (mx * 8 - 1));
        left_c[0][lane - 16] = p & 255;
        left_c[1][lane - 16] = p >> 8;
      } else if (lane >= 32 && lane < 40) {
        const int lcbp = a.cbp[mb0 + mx - 1];
        const int16_t *lp = a.coef + (mb0 + mx - 1) * kCoefPerMb;
        const int i = lane - 32;
        int n = 0;
        if (i < 4) {
          const int blk = 5 + 2 * (i & 1) + 8 * (i >> 1);  // luma4x4BlkIdx 5, 7, 13, 15
          if ((lcbp >> (blk >> 2)) & 1)
            for (int q = 0; q < 16; ++q) n += lp[16 * blk + q] != 0;
          lnz[i] = n;
        } else {
          const int pl = (i - 4) >> 1, k = 1 + 2 * (i & 1);
          if ((lcbp >> 4) == 2)
            for (int q = 0; q < 15; ++q) n += lp[264 + 60 * pl + 15 * k + q] != 0;
          lnzc[pl][i & 1] = n;
        }
      }
    }
    __syncthreads();
    // ---- prediction modes by SAD (ties: the lower mode number)
    int lmode = 2, cmode = 0, dcy = 128, dcu = 128, dcv = 128;
    if (mx > 0) {
      int s = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) s += left_y[i];
      dcy = (s + 8) >> 4;
      int su = 0, sv = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        su += left_c[0][(cj & 4) + i];
        sv += left_c[1][(cj & 4) + i];
      }
      dcu = (su + 2) >> 2;  // 8.3.4: no row above, so every chroma 4x4 block takes its own rows' left samples
      dcv = (sv + 2) >> 2;
      const int u = suv & 255, v = suv >> 8;
      // four sums, each < 2^16, reduced as two packed words
      uint32_t sl = __builtin_amdgcn_sad_u8(static_cast<uint32_t>(left_y[ly]) * 0x01010101u, sy4, 0) |
                    (__builtin_amdgcn_sad_u8(static_cast<uint32_t>(dcy) * 0x01010101u, sy4, 0) << 16);
      uint32_t sc = static_cast<uint32_t>(abs(dcu - u) + abs(dcv - v)) |
                    (static_cast<uint32_t>(abs(left_c[0][cj] - u) + abs(left_c[1][cj] - v)) << 16);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        sl += __shfl_xor(sl, off);
        sc += __shfl_xor(sc, off);
      }
      lmode = (sl & 0xffffu) <= (sl >> 16) ? 1 : 2;
      cmode = (sc & 0xffffu) <= (sc >> 16) ? 0 : 1;
    }
    if (lane < 16) pred_y[lane] = lmode == 1 ? left_y[lane] : dcy;
    if (cmode == 1) {
      if (lane < 16) pred_c[lane >> 3][lane & 7] = left_c[lane >> 3][lane & 7];
    } else if (ci == 0) {
      pred_c[0][cj] = dcu;
      pred_c[1][cj] = dcv;
    }
    __syncthreads();
    // ---- transform + quantisation: lanes 0..15 the luma blocks
    // (luma4x4BlkIdx), 16..23 the chroma blocks, 24 the luma DC, 16 / 17 the
    // chroma DC (enc_search's layout)
    int lv[16], z[16], nzb = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) lv[i] = z[i] = 0;
    const int bxl = lane < 16 ? kBlkXd[lane] : 0, byl = lane < 16 ? kBlkYd[lane] : 0;
    const IntraPred pred{pred_y, pred_c};
    if (lane < 16) {
      int x[16];
      luma_block_diff(lane, srcy, pred, x);
      nzb = eres::code_block<true>(x, qp, z, lv, &ydw[byl * 4 + bxl]);
    } else if (lane < 24) {
      nzb = chroma_block_code(lane, srcc, pred, qpc, z, lv, dcw);
    }
    __syncthreads();
    if (lane == 24) {
      // luma DC: its levels, then the decoder's 8.5.10 for the reconstruction
      int lev[16], sc[16];
      eres::code_i16_dc(ydw, qp, lev);
      full::i16_dc_inverse(lev, qp, full::level_scale(qp % 6, 0, 0), sc);
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        ydl[k] = lev[k];
        yds[k] = sc[k];
      }
    } else if (lane == 16 || lane == 17) {
      eres::code_chroma_dc(dcw[lane - 16], qpc, dcl[lane - 16]);
    }
    const uint64_t nzm = __ballot(nzb);
    const bool ac = (nzm & 0xffffu) != 0;  // Intra16x16: the luma coded_block_pattern is 0 or 15
    int tc = 0;
#pragma unroll
    for (int q = 0; q < 15; ++q) tc += lv[q] != 0;
    __syncthreads();
    const int cc = chroma_cbp(nzm, dcl);
    const int cbp = (ac ? 15 : 0) | (cc << 4);
    if (lane < 16) tcy[byl * 4 + bxl] = ac ? tc : 0;
    else if (lane < 24) tcc[(lane - 16) >> 2][(lane - 16) & 3] = cc == 2 ? tc : 0;
    __syncthreads();
    // ---- the macroblock's bits with the writer's own nC contexts (9.2.1)
    int contrib = 0;
    int dlv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) dlv[q] = 0;
    if (lane < 16) {
      if (ac) {
        contrib = ecav::count_block(lv, 15, ecav::nc_luma(byl * 4 + bxl, tcy, lnz));
      }
    } else if (lane < 24) {
      if (cc == 2) {
        contrib = ecav::count_block(lv, 15, ecav::nc_chroma((lane - 16) >> 2, (lane - 16) & 3, tcc, lnzc));
      }
    } else if (lane < 26) {
      if (cc) {
#pragma unroll
        for (int q = 0; q < 4; ++q) dlv[q] = dcl[lane - 24][q];
        contrib = ecav::count_block(dlv, 4, -1);
      }
    } else if (lane == 26) {  // the header and Intra16x16DCLevel (nC of block 0)
#pragma unroll
      for (int q = 0; q < 16; ++q) dlv[q] = ydl[kZz4[q]];
      const int mbt = 1 + lmode + 4 * cc + (ac ? 12 : 0);
      contrib = ecav::ue_bits(static_cast<uint32_t>(a.all ? mbt : 5 + mbt)) + ecav::ue_bits(static_cast<uint32_t>(cmode)) + 1 +
                ecav::count_block(dlv, 16, ecav::nc_luma(0, tcy, lnz));
    }
    // mb_qp_delta of either candidate against the running QP: se(0) is the one bit counted above
    const int dq_extra = kAq ? eaq::se_bits(qp - rq.pred) - 1 : 0;
    if constexpr (kAq)
      if (lane == 26) contrib += dq_extra;
    [[maybe_unused]] int own = 0;  // kI4: lanes 16..25 hold the chroma bits, the same for both candidates
    if constexpr (kI4) own = contrib;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) contrib += __shfl_xor(contrib, off);
    // ---- kI4: the I_NxN candidate
    [[maybe_unused]] bool use4 = false;  // wave-uniform
    [[maybe_unused]] int cbp4 = 0, lv4k[16];
    [[maybe_unused]] uint64_t modes4 = 0;
    if constexpr (kI4) {
#pragma unroll
      for (int q = 0; q < 16; ++q) lv4k[q] = 0;
      __shared__ __attribute__((aligned(16))) uint8_t tile[16 * ei4::kTilePitch];
      __shared__ int eT[9], eL[5];      // the block's neighbouring samples as ei4::pred_row reads them
      __shared__ int16_t lv4[16][16];   // the blocks' levels (luma4x4BlkIdx, scan order)
      __shared__ int tc4[16];           // their total_coeff, raster order
      if (lane < 16) tile[lane * ei4::kTilePitch + 3] = static_cast<uint8_t>(mx > 0 ? left_y[lane] : 0);
      __syncthreads();
      int mbits = 0;
      for (int k = 0; k < 16; ++k) {
        const ei4::Avail av = ei4::avail_of(k, mx > 0);
        const int pm = ei4::pred_mode_of(k, modes4, mx > 0, left_modes);
        const int bx = kBlkXd[k], by = kBlkYd[k];
        if (lane < 13) {
          const int v = ei4::edge_sample(tile, k, av, lane);
          if (lane < 9) eT[lane] = v;
          else eL[lane - 8] = v;
          if (lane == 0) eL[0] = v;
        }
        __syncthreads();
        const int mode = lane >> 2, y = lane & 3;
        uint32_t p4 = 0, s = 0;
        if (lane < 36) {
          p4 = ei4::pred_row(mode, y, eT, eL, av);
          s = __builtin_amdgcn_sad_u8(p4, srcy[(by * 4 + y) * 4 + bx], 0);
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        uint64_t key = ~0ull;
        if (lane < 36 && ((ei4::allowed_modes(av) >> mode) & 1u)) key = ei4::mode_key(s, qp, mode, pm);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const uint64_t o = __shfl_xor(key, off);
          key = o < key ? o : key;
        }
        const int best = ei4::key_mode(key);  // wave-uniform
        uint32_t pr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) pr[r] = static_cast<uint32_t>(__shfl(static_cast<int>(p4), best * 4 + r));
        if (lane == 0) {
          int x[16], z4[16], l4[16], res[16];
#pragma unroll
          for (int r = 0; r < 4; ++r) eres::diff_row4(srcy[(by * 4 + r) * 4 + bx], pr[r], x + 4 * r);
          eres::code_block<false>(x, qp, z4, l4, nullptr);
          full::scale_idct4(z4, qp, false, res);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            *reinterpret_cast<uint32_t *>(tile + (by * 4 + r) * ei4::kTilePitch + 4 + 4 * bx) = eres::recon_row4(pr[r], res + 4 * r);
#pragma unroll
          for (int q = 0; q < 16; ++q) lv4[k][q] = static_cast<int16_t>(l4[q]);
        }
        modes4 |= static_cast<uint64_t>(best) << (4 * k);
        mbits += ei4::mode_bits(best, pm);
        __syncthreads();
      }
      // its bits: the luma blocks of the coded 8x8s with the writer's nC, the chroma bits as above, the header
      int tck = 0;
      if (lane < 16) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          lv4k[q] = lv4[lane][q];
          tck += lv4k[q] != 0;
        }
      }
      const uint32_t nzm4 = static_cast<uint32_t>(__ballot(tck != 0)) & 0xffffu;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if ((nzm4 >> (4 * q)) & 15u) cbp4 |= 1 << q;
      cbp4 |= cc << 4;
      const bool coded8 = lane < 16 && ((cbp4 >> (lane >> 2)) & 1);
      if (lane < 16) tc4[byl * 4 + bxl] = coded8 ? tck : 0;
      __syncthreads();
      int c4 = 0;
      if (lane < 16) {
        if (coded8) {
          c4 = ecav::count_block(lv4k, 16, ecav::nc_luma(byl * 4 + bxl, tc4, lnz));
        }
      } else if (lane < 26) {
        c4 = own;
      } else if (lane == 26) {  // mb_type, the sixteen modes, intra_chroma_pred_mode, coded_block_pattern, mb_qp_delta
        c4 = ecav::ue_bits(a.all ? 0u : 5u) + mbits + ecav::ue_bits(static_cast<uint32_t>(cmode)) +
             ecav::ue_bits(ecav::cbp_intra_code(cbp4)) + (cbp4 ? 1 + dq_extra : 0);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) c4 += __shfl_xor(c4, off);
      use4 = c4 < contrib;  // ties go to Intra16x16
      if (use4) {
        contrib = c4;
        if (lane < 36 && lane >= 32) tcy[(lane - 32) * 4 + 3] = tc4[(lane - 32) * 4 + 3];  // what the right neighbour counts
        recy[lane] = *reinterpret_cast<const uint32_t *>(tile + ly * ei4::kTilePitch + 4 + lx);
      }
      __syncthreads();
    }
    const bool intra = contrib <= kPcmBits;  // wave-uniform
    row_bits += static_cast<uint32_t>(intra ? contrib : kPcmBits);
    if constexpr (kAq) rq.step(intra && (!(kI4 && use4) || cbp4 != 0), qp);  // Intra16x16 always sends its delta, I_NxN with a pattern
    if constexpr (kI4) {
      if (intra && use4) {
        // I_NxN: luma is reconstructed (recy, above); chroma as Intra16x16; luma levels in the inter layout
        if (lane >= 16 && lane < 24) chroma_block_recon(lane, pred, dcl, z, cc == 2, qpc, recc);
        int16_t *cp = a.coef + (mb0 + mx) * kCoefPerMb;
        if (lane < 16) {
#pragma unroll
          for (int q = 0; q < 16; ++q) cp[16 * lane + q] = static_cast<int16_t>(lv4k[q]);
        }
        store_chroma_levels(cp, lane, lv, dcl);
      }
    }
    if (intra && !(kI4 && use4)) {
      // ---- reconstruction through the decoder's inverse path
      if (lane < 16) {
        int res[16];
        eres::residual_dc_done(yds[byl * 4 + bxl], z, ac, qp, res);
        luma_block_recon(lane, pred, res, recy);
      } else if (lane < 24) {  // chroma (8.5.11 DC, then 8.5.12)
        chroma_block_recon(lane, pred, dcl, z, cc == 2, qpc, recc);
      }
      // the levels the slice writer codes: luma DC [0, 16), AC block b at 16 + 15 b, chroma as enc_search
      int16_t *cp = a.coef + (mb0 + mx) * kCoefPerMb;
      if (lane < 16) {
#pragma unroll
        for (int q = 0; q < 15; ++q) cp[16 + 15 * lane + q] = static_cast<int16_t>(lv[q]);
      } else if (lane == 26) {
#pragma unroll
        for (int q = 0; q < 16; ++q) cp[q] = static_cast<int16_t>(dlv[q]);
      }
      store_chroma_levels(cp, lane, lv, dcl);
    }
    __syncthreads();
    if (intra || a.all) {
      *reinterpret_cast<uint32_t *>(dst + lo) = intra ? recy[lane] : sy4;
      *reinterpret_cast<uint16_t *>(dst + co) = intra ? static_cast<uint16_t>(recc[0][lane] | (recc[1][lane] << 8)) : suv;
    }
    if constexpr (kI4) {
      left_modes = intra && use4 ? modes4 : ei4::kNoModes;
      if (lane == 0) {
        a.i4[mb0 + mx] = left_modes;
        if (intra && use4) {
          a.cmd[mb0 + mx] = ei4::kI4Cmd | static_cast<uint32_t>((cmode << 2) | (cbp4 << 4));
          a.cbp[mb0 + mx] = static_cast<uint8_t>(cbp4);
        }
      }
    }
    if (lane == 0 && !(kI4 && intra && use4)) {
      a.cmd[mb0 + mx] = intra ? kIntraCmd | static_cast<uint32_t>(lmode | (cmode << 2) | (cbp << 4)) : kPcmCmd;
      a.cbp[mb0 + mx] = static_cast<uint8_t>(intra ? cbp : 0);
    }
    // what the macroblock to the right sees: this one's right column (from
    // LDS, never read back from dst) and its total_coeff (16 after I_PCM)
    if (lane < 16) {
      left_y[lane] = static_cast<int>((intra ? recy[lane * 4 + 3] : srcy[lane * 4 + 3]) >> 24);
    } else if (lane < 32) {
      const int pl = (lane - 16) >> 3, y = lane & 7;
      left_c[pl][y] = intra ? recc[pl][y * 8 + 7] : static_cast<int>((srcc[y * 8 + 7] >> (8 * pl)) & 255);
    } else if (lane < 36) {
      lnz[lane - 32] = intra ? tcy[(lane - 32) * 4 + 3] : 16;
    } else if (lane < 40) {
      const int pl = (lane - 36) >> 1, r = lane & 1;
      lnzc[pl][r] = intra ? tcc[pl][1 + 2 * r] : 16;
    }
    left_mine = true;
    __syncthreads();
  }
  if (a.est_f && lane == 0 && row_bits) atomicAdd(a.est_f + en.x, row_bits);
}

// ------------------------------------------------------ in-loop deblocking
// vts_transcode_ext2.deblock: every slice carries
// disable_deblocking_filter_idc = 2 and a slice is one macroblock row, so a
// row's filtering (8.7) is a serial chain over its macroblocks that touches no
// other row: one wave per (level entry, macroblock row) walking mx = 0 ..
// mbw - 1, as enc_intra does; all ordering is program order inside the wave
// plus stream order between launches.  Per macroblock, in the standard's
// order: the vertical edges e = 0..3 (0 only with a left neighbour), then the
// horizontal edges 1..3 (the top edge is a slice boundary); an edge step is 16
// luma lines on lanes 0..15 and, for e = 0 and 2, 8 Cb + 8 Cr lines on lanes
// 16..31.  The decisions (bS, indexA / indexB, the line filter) are
// enc_deblock.h's, which the CPU harness walks in the same order.
//
// LDS tile, 24 rows of kDbPitch bytes: rows 0..15 luma, 16..23 the Cb|Cr
// pairs; bytes 0..3 of a row the left macroblock's last four luma columns
// (last two chroma pairs), bytes 4..19 this macroblock.  A macroblock ends
// with one 16-byte store per row: the left macroblock's final columns 12..15
// and this one's columns 0..11 (the next edge 0 still changes 13..15).
constexpr int kDbPitch = 20;

// PT: a macroblock's motion is the four quadrant vectors of a.mv4 (enc_part.h);
// false: the code is the kernel's without partitions
template <bool PT>
__global__ void __launch_bounds__(64) enc_deblock(DeblockArgs a) {
  namespace edb = full::edb;
  __shared__ __attribute__((aligned(16))) uint8_t T[24 * kDbPitch];
  struct alignas(16) Lv {
    int16_t s[16];
  };
  const int lane = threadIdx.x;
  const int e = blockIdx.x / a.mbh, my = blockIdx.x % a.mbh;
  const int4 en = a.ent[e];
  const int qp = a.qp_f ? a.qp_f[en.x] : a.qp;  // SliceQPY; wave-uniform: the picture's own when given
  uint8_t *dst = a.recon + static_cast<int64_t>(en.z) * a.stride;
  const int64_t mb0 = (static_cast<int64_t>(e) * a.mbh + my) * a.mbw;
  // loads and stores: lane (r, q4) moves dword q4 of luma row r and, below 32, of chroma row r
  const int r = lane >> 2, q4 = 4 * (lane & 3);
  uint8_t *gy = dst + static_cast<int64_t>(my * 16 + r) * a.cw + q4;
  uint8_t *gc = dst + static_cast<int64_t>(a.cw) * a.ch + static_cast<int64_t>(my * 8 + (r & 7)) * a.cw + q4;
  uint8_t *ty = T + r * kDbPitch + q4, *tc = T + (16 + (r & 7)) * kDbPitch + q4;
  // filtering: lanes 0..15 luma line `lane`; 16..31 plane pl, chroma line kc (the luma line 2 kc)
  const bool chroma = lane >= 16;
  const int pl = (lane >> 3) & 1, kc = lane & 7, line = chroma ? 2 * kc : lane;
  auto load_lv = [&](int mx, Lv &lv) {
    if (lane < 16) {
      const uint4 *p = reinterpret_cast<const uint4 *>(a.coef + (mb0 + mx) * kCoefPerMb + 16 * lane);
      reinterpret_cast<uint4 *>(lv.s)[0] = p[0];
      reinterpret_cast<uint4 *>(lv.s)[1] = p[1];
    }
  };
  // the next macroblock's samples, command, coded_block_pattern and levels, read one macroblock ahead
  uint32_t pf_y = *reinterpret_cast<const uint32_t *>(gy), pf_c = 0;
  if (lane < 32) pf_c = *reinterpret_cast<const uint32_t *>(gc);
  uint32_t n_cmd = a.cmd[mb0];
  int n_cbp = a.cbp[mb0];
  [[maybe_unused]] uint4 n_mv{};  // PT: the macroblock's quadrant vectors
  if constexpr (PT) n_mv = reinterpret_cast<const uint4 *>(a.mv4)[mb0];
  Lv n_lv{};
  load_lv(0, n_lv);
  // indexA, alpha' and beta' of this lane's plane for the three qPav an edge can have (qP is 0 for
  // I_PCM and the slice QP otherwise), looked up once: both sides I_PCM, one side, neither
  const edb::Idx x_pcm = edb::indices(0, 0, a.off_a, a.off_b, chroma, 0);
  const edb::Idx x_mix = edb::indices(0, qp, a.off_a, a.off_b, chroma, 0);
  const edb::Idx x_qp = edb::indices(qp, qp, a.off_a, a.off_b, chroma, 0);
  // a.aq_off: the macroblocks have their own QPs (enc_aq.h).  QP_Y of one that sent no mb_qp_delta is the
  // slice's running QP, which this walk keeps; an edge's indices are looked up from its two sides' QP_Y
  const int8_t *aqr = a.aq_off ? a.aq_off + (static_cast<int64_t>(en.x) * a.mbh + my) * a.mbw : nullptr;
  eaq::RunQp rq;
  rq.start(qp);
  int qy_left = 0, qy_cur = 0;  // aqr: QP_Y of the left and of this macroblock as the filter reads them (I_PCM 0)
  uint32_t carry = 0;  // lanes 0..23: the row's last dword of the macroblock to the left
  edb::Mb left = edb::mb_of_cmd(kPcmCmd, 0);
  bool prev_filtered = false;  // wave-uniform
  for (int mx = 0; mx < a.mbw; ++mx) {
    *reinterpret_cast<uint32_t *>(ty + 4) = pf_y;
    if (lane < 32) *reinterpret_cast<uint32_t *>(tc + 4) = pf_c;
    if (lane < 24) *reinterpret_cast<uint32_t *>(T + lane * kDbPitch) = carry;
    const uint32_t cmd = n_cmd;
    if (aqr) {  // wave-uniform
      const bool pcm = cmd == kPcmCmd;
      rq.step(eaq::sends_delta(pcm, is_intra_cmd(cmd) && !ei4::is_i4_cmd(cmd), n_cbp), eaq::qp_mb(qp, aqr[mx], a.aq_lo, a.aq_hi));
      qy_cur = rq.filter_qp(pcm);
    }
    const bool nzb = lane < 16 && edb::blk_nz(n_lv.s, n_cbp, lane);
    [[maybe_unused]] const uint4 mv = n_mv;
    if (mx + 1 < a.mbw) {
      pf_y = *reinterpret_cast<const uint32_t *>(gy + (mx + 1) * 16);
      if (lane < 32) pf_c = *reinterpret_cast<const uint32_t *>(gc + (mx + 1) * 16);
      n_cmd = a.cmd[mb0 + mx + 1];
      n_cbp = a.cbp[mb0 + mx + 1];
      if constexpr (PT) n_mv = reinterpret_cast<const uint4 *>(a.mv4)[mb0 + mx + 1];
      load_lv(mx + 1, n_lv);
    }
    const uint32_t nzr = edb::nz_raster(static_cast<uint32_t>(__ballot(nzb)));
    const edb::Mb cur = PT ? edb::mb_of_cmd4(cmd, nzr, mv.x, mv.y, mv.z, mv.w) : edb::mb_of_cmd(cmd, nzr);
    __syncthreads();
    bool filtered = false;
#pragma unroll
    for (int dir = 0; dir < 2; ++dir)
#pragma unroll
      for (int ed = 0; ed < 4; ++ed) {
        if (ed == 0 && (dir == 1 || mx == 0)) continue;
        [[maybe_unused]] const edb::Mb &p = ed == 0 ? left : cur;
        const bool mine = lane < 16 || (lane < 32 && !(ed & 1));
        int bS, qpp;
        if constexpr (PT) {  // left or cur by name, not through p: the larger Mb then stays in registers
          bS = !mine ? 0 : (ed == 0 ? edb::line_bs<true>(left, cur, dir, ed, line) : edb::line_bs<true>(cur, cur, dir, ed, line));
          qpp = ed == 0 ? edb::qp_of(left, qp) : edb::qp_of(cur, qp);
        } else {
          bS = mine ? edb::line_bs<false>(p, cur, dir, ed, line) : 0;
          qpp = edb::qp_of(p, qp);
        }
        const int qpq = edb::qp_of(cur, qp);
        edb::Idx x = qpp != qpq ? x_mix : (qpp ? x_qp : x_pcm);
        if (aqr) x = edb::indices(ed == 0 ? qy_left : qy_cur, qy_cur, a.off_a, a.off_b, chroma, 0);
        const bool act = bS > 0 && x.alpha && x.beta;
        if (__ballot(act)) {  // wave-uniform
          if (act) {
            uint8_t *s;
            int step;
            if (dir == 0) {
              s = T + (chroma ? 16 + kc : lane) * kDbPitch + 4 + 4 * ed + (chroma ? pl : 0);
              step = chroma ? 2 : 1;
            } else {
              s = T + (chroma ? 16 + 2 * ed : 4 * ed) * kDbPitch + 4 + (chroma ? 2 * kc + pl : lane);
              step = kDbPitch;
            }
            filtered |= edb::filter(s, step, bS, chroma, x);
          }
          __syncthreads();
        }
      }
    const bool wave_filtered = __ballot(filtered) != 0;
    const uint32_t oy = *reinterpret_cast<const uint32_t *>(ty);
    const uint32_t oc = lane < 32 ? *reinterpret_cast<const uint32_t *>(tc) : 0;
    if (lane < 24) carry = *reinterpret_cast<const uint32_t *>(T + lane * kDbPitch + 16);
    __syncthreads();
    // columns 12..15 of the macroblock to the left changed here or in its own step; 0..11 of this one here
    if ((wave_filtered || prev_filtered) && (mx > 0 || q4 > 0)) {
      *reinterpret_cast<uint32_t *>(gy + mx * 16 - 4) = oy;
      if (lane < 32) *reinterpret_cast<uint32_t *>(gc + mx * 16 - 4) = oc;
    }
    if (wave_filtered && lane == 0) atomicAdd(a.count, 1ull);
    prev_filtered = wave_filtered;
    left = cur;
    qy_left = qy_cur;
  }
  if (prev_filtered && lane < 24) {  // the last macroblock's columns 12..15
    uint8_t *g = lane < 16 ? dst + static_cast<int64_t>(my * 16 + lane) * a.cw
                           : dst + static_cast<int64_t>(a.cw) * a.ch + static_cast<int64_t>(my * 8 + lane - 16) * a.cw;
    *reinterpret_cast<uint32_t *>(g + a.mbw * 16 - 4) = carry;
  }
}

// The encoder's reconstruction hashed as vts_synth_info.recon_hash: over the
// display-size NV12 bytes j of each of the level's frames f, b_j ((j % 65521)
// + 1) (f + 1) added into *acc (wrap-around addition: any order).
__global__ void __launch_bounds__(256) enc_hash(const int4 *ent, const uint8_t *recon, int64_t stride, int32_t cw,
                                                int32_t ch, int32_t w, int32_t h, int32_t per_frame,
                                                unsigned long long *acc) {
  __shared__ unsigned long long part[4];
  const int4 en = ent[blockIdx.x / per_frame];  // per_frame workgroups share a frame
  const int b0 = blockIdx.x % per_frame;
  const uint8_t *p = recon + static_cast<int64_t>(en.z) * stride;
  // one dword of a display row per pass (rows start 16-aligned and cw >= w
  // rounded up to 4, so the dword is inside the coded row; bytes past w are
  // dropped): NV12 rows y < h luma, then h / 2 rows of Cb|Cr pairs
  const int nd = (w + 3) >> 2, n = (h + h / 2) * nd;
  unsigned long long s = 0;
  for (int i = b0 * 256 + threadIdx.x; i < n; i += per_frame * 256) {
    const int y = i / nd, x = 4 * (i - y * nd);
    const uint8_t *row = y < h ? p + static_cast<int64_t>(y) * cw : p + static_cast<int64_t>(cw) * ch + static_cast<int64_t>(y - h) * cw;
    const uint32_t v = *reinterpret_cast<const uint32_t *>(row + x);
    int m = (y * w + x) % 65521;  // j % 65521 of the dword's first byte
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (x + k < w) s += static_cast<unsigned long long>(((v >> (8 * k)) & 255u) * static_cast<uint32_t>(m + 1));
      m = m + 1 == 65521 ? 0 : m + 1;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicAdd(acc, (part[0] + part[1] + part[2] + part[3]) * static_cast<unsigned long long>(en.x + 1));
}

// I_PCM: pcm_alignment_zero_bits, then 384 sample bytes that enc_pcm fills in
// later (the gap's bytes in the partial words either side are don't-care
// here: enc_pcm runs after enc_gather).  The samples are >= 1 (downscale
// clamp), and the byte before them holds mb_type's last 1 bits, so no
// emulation prevention byte can fall in or next to them and the zero-run
// state after them is 0.
__device__ void pcm_gap(NalOut &o, uint4 *job, int s, int mx) {
  o.align();
  o.flush();
  *job = make_uint4(static_cast<uint32_t>(s), static_cast<uint32_t>(4 + o.n), static_cast<uint32_t>(mx), 0);
  o.n += 384;  // a multiple of 4: the word phase is unchanged
  o.cur = 0;
  if (o.n > o.cap) o.over = true;
  o.zeros = 0;
}

// The CAVLC slices, one lane per slice: the header (enc_rbsp.h), then a
// dispatch over enc_cavlc.h's macroblock kinds, which hold all the syntax and
// the state a slice carries (ecav::Row); here are the counters, the I_PCM
// jobs and the slot.
// kIntra: enc_intra ran on every level, so IDR pictures have commands too and
// a command may be kIntraCmd (the other instance is the encoder without it).
// kDbk: the slices ask for the in-loop filter inside the slice (enc_deblock
// ran on the reconstruction); false: the header, and the code, without it.
// kPart: a command may be a partitioned macroblock's (enc_part.h), its vectors
// in a.mv4; false: the code is the kernel's without partitions
// kAq: the macroblocks have their own QPs (a.aq_off, enc_aq.h) and send
// mb_qp_delta; false: the code is the kernel's without it (a runtime test of
// the pointer costs both writers registers, and some instances a wave)
template <bool kIntra, bool kDbk, bool kPart, bool kAq>
__global__ void __launch_bounds__(64) enc_write(WriteArgs a) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.n_slices) return;
  const int e = s / a.mbh, row = s % a.mbh;
  const int4 en = a.ent[e];
  const bool idr = en.y == 0;  // GOP position 0
  const int qp = a.qp_f ? a.qp_f[en.x] : a.qp;  // the picture's own QP when given
  uint8_t *slot = a.staging + static_cast<int64_t>(s) * a.cap;
  NalOut o = full::erbsp::word_sink(reinterpret_cast<uint32_t *>(slot + 4), a.cap - 4);
  // slice_qp_delta: SliceQPY = the residual's QP; every picture is a reference
  full::erbsp::slice_header(o, false, idr, row * a.mbw, en.y, en.z, qp >= 1 ? qp - 26 : 0, kDbk, a.dbk_alpha, a.dbk_beta);
  unsigned long long npcm = 0, ninter = 0, nskip = 0, nintra = 0, ni4 = 0;
  const uint32_t *cmd = a.cmd + static_cast<int64_t>(e) * a.mbw * a.mbh + static_cast<int64_t>(row) * a.mbw;
  const uint8_t *cbpr = a.cbp + static_cast<int64_t>(e) * a.mbw * a.mbh + static_cast<int64_t>(row) * a.mbw;
  const int16_t *coef_row =
      a.coef + ((static_cast<int64_t>(en.y % a.ring) * a.coef_per_level + en.w) * a.mbh + row) * a.mbw * kCoefPerMb;
  const uint64_t *i4r = kIntra && a.i4 ? a.i4 + static_cast<int64_t>(e) * a.mbw * a.mbh + static_cast<int64_t>(row) * a.mbw : nullptr;
  [[maybe_unused]] const uint32_t *mv4r =
      kPart ? a.mv4 + (static_cast<int64_t>(e) * a.mbw * a.mbh + static_cast<int64_t>(row) * a.mbw) * 4 : nullptr;
  [[maybe_unused]] unsigned long long n16x8 = 0, n8x16 = 0, n8x8 = 0;
  const bool all_pcm = idr && !kIntra;  // level 0 without intra holds no commands
  // reserve this slice's I_PCM jobs
  uint32_t njob = 0;
  if (all_pcm) {
    njob = static_cast<uint32_t>(a.mbw);
  } else {
    for (int mx = 0; mx < a.mbw; ++mx) njob += cmd[mx] == kPcmCmd;
  }
  uint4 *job = a.jobs + (njob ? atomicAdd(a.n_jobs, njob) : 0u);
  ecav::Row z;
  z.start();
  // kAq: the macroblocks' own QPs; mb_qp_delta by the slice's running QP (enc_aq.h), else 0 as ever
  const int8_t *aqr = kAq ? a.aq_off + (static_cast<int64_t>(en.x) * a.mbh + row) * a.mbw : nullptr;
  eaq::RunQp rq;
  rq.start(qp);
  for (int mx = 0; mx < a.mbw; ++mx) {
    const uint32_t c = all_pcm ? kPcmCmd : cmd[mx];
    const int16_t *cp = coef_row + static_cast<int64_t>(mx) * kCoefPerMb;
    int dqp = 0;
    if (aqr)
      dqp = rq.step(eaq::sends_delta(c == kPcmCmd, is_intra_cmd(c) && !ei4::is_i4_cmd(c), cbpr[mx]),
                    eaq::qp_mb(qp, aqr[mx], a.aq_lo, a.aq_hi));
    if (c == kPcmCmd) {
      ecav::mb_pcm_head(o, idr, z);
      pcm_gap(o, job++, s, mx);
      ++npcm;
    } else if (kIntra && ei4::is_i4_cmd(c)) {
      ecav::mb_intra4(o, idr, z, c, i4r[mx], cp, dqp);
      ++nintra;
      ++ni4;
    } else if (kIntra && is_intra_cmd(c)) {
      ecav::mb_intra16(o, idr, z, c, cp, dqp);
      ++nintra;
    } else if (c == 0 && cbpr[mx] == 0) {  // P_Skip: vector (0, 0), nothing coded
      ecav::mb_skip(z);
      ++nskip;
    } else if (kPart && ep::is_part_cmd(c)) {
      ecav::mb_p_part(o, z, c, mv4r + 4 * mx, cbpr[mx], cp, dqp);
      ++ninter;
      const int shape = ep::part_shape(c);
      n16x8 += shape == ep::k16x8;
      n8x16 += shape == ep::k8x16;
      n8x8 += shape == ep::k8x8;
    } else {
      ecav::mb_inter(o, z, c, cbpr[mx], cp, dqp);
      ++ninter;
    }
  }
  ecav::slice_end(o, z);
  o.flush();
  const int64_t len = o.n;
  if (o.over) {
    atomicOr(a.err, 1u);
    a.sizes[s] = 0;
    return;
  }
  *reinterpret_cast<uint32_t *>(slot) = __builtin_bswap32(static_cast<uint32_t>(len));  // big-endian length
  a.sizes[s] = static_cast<int32_t>(len + 4);
  atomicAdd(&a.stats[kStPcm], npcm);
  atomicAdd(&a.stats[kStInter], ninter);
  atomicAdd(&a.stats[kStSkip], nskip);
  if (nintra) atomicAdd(&a.stats[kStIntra], nintra);
  if (ni4) atomicAdd(&a.stats[kStI4], ni4);
  if constexpr (kPart) {
    if (n16x8) atomicAdd(&a.stats[kStP16x8], n16x8);
    if (n8x16) atomicAdd(&a.stats[kStP8x16], n8x16);
    if (n8x8) atomicAdd(&a.stats[kStP8x8], n8x8);
  }
}

// The slices with entropy_coding_mode_flag = 1 (vts_transcode_ext4.cabac,
// DESIGN.md §11): enc_write's arguments, staging slots, sizes, counters, error
// word and I_PCM jobs, the slice data by 7.3.4 / 9.3 through enc_cabac.h.  One
// wave per slice: a slice is a serial chain of bins, so lane 0 walks it; the
// wave initialises the 277 context variables in LDS (9.3.1.1), counts the
// slice's I_PCM jobs and stages each macroblock's levels in LDS ahead of
// lane 0's walk.  Lane 0 records a macroblock's bins in an LDS ring
// (ecab::BinRing: one 16-bit entry per bin) and codes them in ecab::drain's one
// loop, at the latest where the ring has less than a block's worst case free.
// Ordering is program order inside the wave and the two workgroup barriers
// around the walk of a macroblock; no wave waits on another.
//
// I_PCM: mb_type ends in the terminate bin 1 and the flush (9.3.4.5), whose
// last bit is 1; pcm_alignment_zero_bits follow in the same byte or none at
// all, so the byte before the samples is non-zero, the samples are >= 1
// (downscale clamp), and pcm_gap's argument holds as it does for CAVLC: no
// emulation prevention byte falls in or next to the samples and the zero run
// after them is 0.  The encoder restarts behind them (9.3.1.2).
template <bool kIntra, bool kDbk, bool kPart, bool kAq>
__global__ void __launch_bounds__(64) enc_write_cabac(WriteArgs a) {
  namespace ec = full::ecab;
  __shared__ uint8_t st[320];             // ec::kNumCtx context variables
  __shared__ uint32_t lvw[kCoefPerMb / 2];  // the macroblock's levels
  __shared__ uint16_t ring[ec::kRingBins];
  const int s = blockIdx.x, lane = threadIdx.x;  // the grid is n_slices waves
  const int e = s / a.mbh, row = s % a.mbh;
  const int4 en = a.ent[e];
  const bool idr = en.y == 0;
  const int qp = a.qp_f ? a.qp_f[en.x] : a.qp;  // SliceQPY; wave-uniform: the picture's own when given
  for (int i = lane; i < ec::kNumCtx; i += 64) st[i] = ec::init_context(i, idr, qp);
  const uint32_t *cmd = a.cmd + static_cast<int64_t>(e) * a.mbw * a.mbh + static_cast<int64_t>(row) * a.mbw;
  const uint8_t *cbpr = a.cbp + static_cast<int64_t>(e) * a.mbw * a.mbh + static_cast<int64_t>(row) * a.mbw;
  const int16_t *coef_row =
      a.coef + ((static_cast<int64_t>(en.y % a.ring) * a.coef_per_level + en.w) * a.mbh + row) * a.mbw * kCoefPerMb;
  const uint64_t *i4r = kIntra && a.i4 ? a.i4 + static_cast<int64_t>(e) * a.mbw * a.mbh + static_cast<int64_t>(row) * a.mbw : nullptr;
  unsigned long long ni4 = 0;
  const bool all_pcm = idr && !kIntra;  // level 0 without intra holds no commands
  uint32_t njob = 0;
  if (all_pcm) {
    njob = static_cast<uint32_t>(a.mbw);
  } else {
    for (int mx = lane; mx < a.mbw; mx += 64) njob += cmd[mx] == kPcmCmd;
    for (int off = 32; off > 0; off >>= 1) njob += __shfl_xor(njob, off);
  }
  uint8_t *slot = a.staging + static_cast<int64_t>(s) * a.cap;
  NalOut o = full::erbsp::word_sink(reinterpret_cast<uint32_t *>(slot + 4), a.cap - 4);
  ec::Encoder<NalOut> coder{&o, st, 0, 510, 0, true};
  ec::BinRing<NalOut> enc{&coder, ring, 0};
  ec::Left left = ec::left_none();
  uint4 *job = a.jobs;
  unsigned long long npcm = 0, ninter = 0, nskip = 0, nintra = 0;
  bool a_ok = false;
  int amx = 0, amy = 0;
  [[maybe_unused]] int a3x = 0, a3y = 0;  // partitions: the left macroblock's quadrant 3 (amx, amy: its quadrant 1)
  [[maybe_unused]] const uint32_t *mv4r =
      kPart ? a.mv4 + (static_cast<int64_t>(e) * a.mbw * a.mbh + static_cast<int64_t>(row) * a.mbw) * 4 : nullptr;
  [[maybe_unused]] unsigned long long n16x8 = 0, n8x16 = 0, n8x8 = 0;
  if (lane == 0) {
    if (njob) job += atomicAdd(a.n_jobs, njob);
    ec::slice_header(o, idr, row * a.mbw, en.y, en.z, qp, kDbk, a.dbk_alpha, a.dbk_beta);
  }
  const int16_t *lv = reinterpret_cast<const int16_t *>(lvw);
  // kAq: as in enc_write; ctxIdxInc of the delta's first bin travels in ec::Left
  const int8_t *aqr = kAq ? a.aq_off + (static_cast<int64_t>(en.x) * a.mbh + row) * a.mbw : nullptr;
  eaq::RunQp rq;
  rq.start(qp);
  for (int mx = 0; mx < a.mbw; ++mx) {
    const uint32_t c = all_pcm ? kPcmCmd : cmd[mx];  // wave-uniform
    const bool intra = kIntra && is_intra_cmd(c);
    const int cbp = (c == kPcmCmd || intra) ? 0 : cbpr[mx];
    int dqp = 0;
    if (aqr)  // an I_NxN macroblock's pattern is in its command word
      dqp = rq.step(eaq::sends_delta(c == kPcmCmd, intra && !ei4::is_i4_cmd(c), intra ? static_cast<int>(c >> 4) & 63 : cbp),
                    eaq::qp_mb(qp, aqr[mx], a.aq_lo, a.aq_hi));
    __syncthreads();  // lane 0 is done with the previous macroblock's levels (and, first, the contexts are set)
    if (intra || cbp) {
      const uint32_t *src = reinterpret_cast<const uint32_t *>(coef_row + static_cast<int64_t>(mx) * kCoefPerMb);
      for (int i = lane; i < kCoefPerMb / 2; i += 64) lvw[i] = src[i];
    }
    __syncthreads();
    if (lane != 0) continue;
    const bool last = mx == a.mbw - 1;
    if (c == kPcmCmd) {
      ec::mb_pcm_begin(enc, idr, left);
      pcm_gap(o, job++, s, mx);
      ec::mb_pcm_end(enc, left, last);
      a_ok = false;
      ++npcm;
    } else if (intra && ei4::is_i4_cmd(c)) {
      ec::mb_intra4(enc, idr, left, c, i4r[mx], lv, last, dqp);
      a_ok = false;
      ++nintra;
      ++ni4;
    } else if (intra) {
      ec::mb_intra16(enc, idr, left, c, lv, last, dqp);
      a_ok = false;
      ++nintra;
    } else if (kPart && ep::is_part_cmd(c)) {
      const uint32_t *v = mv4r + 4 * mx;
      const int shape = ep::part_shape(c);
      ec::mb_p_part(enc, left, shape, v, ep::Left{a_ok, {amx, amy}, {a3x, a3y}}, cbp, lv, last, dqp);
      ++ninter;
      n16x8 += shape == ep::k16x8;
      n8x16 += shape == ep::k8x16;
      n8x8 += shape == ep::k8x8;
      a_ok = true;
      amx = static_cast<int16_t>(v[1] & 0xffffu);
      amy = static_cast<int16_t>(v[1] >> 16);
      a3x = static_cast<int16_t>(v[3] & 0xffffu);
      a3y = static_cast<int16_t>(v[3] >> 16);
    } else {
      const int mvx = static_cast<int16_t>(c & 0xffffu), mvy = static_cast<int16_t>(c >> 16);
      if (mvx == 0 && mvy == 0 && cbp == 0) {  // P_Skip
        ec::mb_skip(enc, left, last);
        ++nskip;
      } else {
        ec::mb_inter(enc, left, mvx - (a_ok ? amx : 0), mvy - (a_ok ? amy : 0), cbp, lv, last, dqp);  // 8.4.1.3, A alone
        ++ninter;
      }
      a_ok = true;
      amx = a3x = mvx;
      amy = a3y = mvy;
    }
  }
  if (lane != 0) return;
  enc.sync();
  o.align();  // the flush of the last end_of_slice_flag ended in rbsp_stop_one_bit
  o.flush();
  const int64_t len = o.n;
  if (o.over) {
    atomicOr(a.err, 1u);
    a.sizes[s] = 0;
    return;
  }
  *reinterpret_cast<uint32_t *>(slot) = __builtin_bswap32(static_cast<uint32_t>(len));  // big-endian length
  a.sizes[s] = static_cast<int32_t>(len + 4);
  atomicAdd(&a.stats[kStPcm], npcm);
  atomicAdd(&a.stats[kStInter], ninter);
  atomicAdd(&a.stats[kStSkip], nskip);
  if (nintra) atomicAdd(&a.stats[kStIntra], nintra);
  if (ni4) atomicAdd(&a.stats[kStI4], ni4);
  if constexpr (kPart) {
    if (n16x8) atomicAdd(&a.stats[kStP16x8], n16x8);
    if (n8x16) atomicAdd(&a.stats[kStP8x16], n8x16);
    if (n8x8) atomicAdd(&a.stats[kStP8x8], n8x8);
  }
}

// Slice offsets of one level on the device: offs[s] = running output total +
// exclusive scan of the slice sizes (one 1024-thread workgroup), each frame's
// (offset, size), and the running total advanced.  No host round trip.
__global__ void __launch_bounds__(1024) enc_scan(const int32_t *sizes, int ns, const int4 *ent, int mbh,
                                                 int64_t *offs, int64_t *total, int64_t *fr_off,
                                                 int64_t *fr_size) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int per = (ns + 1023) / 1024;
  const int b0 = min(ns, t * per), b1 = min(ns, b0 + per);
  const int64_t base = *total;
  int64_t sum = 0;
  for (int i = b0; i < b1; ++i) sum += sizes[i];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {  // inclusive scan of the partial sums
    const int64_t v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t run = base + part[t] - sum;
  for (int i = b0; i < b1; ++i) {
    offs[i] = run;
    run += sizes[i];
  }
  __syncthreads();
  const int64_t end = base + part[1023];
  const int ne = ns / mbh;
  for (int e = t; e < ne; e += 1024) {
    const int64_t o = offs[static_cast<int64_t>(e) * mbh];
    fr_off[ent[e].x] = o;
    fr_size[ent[e].x] = (e + 1 < ne ? offs[static_cast<int64_t>(e + 1) * mbh] : end) - o;
  }
  if (t == 0) *total = end;
}

// one workgroup per slice: staging slot -> the chunk arena (offsets are
// absolute; the arena starts at *base)
__global__ void __launch_bounds__(256) enc_gather(const uint8_t *staging, int64_t cap, const int32_t *sizes,
                                                  const int64_t *offs, const int64_t *base, uint8_t *out) {
  const int s = blockIdx.x;
  const uint8_t *p = staging + static_cast<int64_t>(s) * cap;
  uint8_t *q = out + (offs[s] - *base);
  const int n = sizes[s];
  for (int i = threadIdx.x; i < n; i += 256) q[i] = p[i];
}

// I_PCM payloads: one wave per job, 6 bytes per lane, straight into the
// packed level output (after enc_gather): luma 16x16, then Cb 8x8, Cr 8x8
// (7.3.5) from the NV12 source.
__global__ void __launch_bounds__(64) enc_pcm(const uint4 *jobs, const uint32_t *n_jobs, const int4 *ent,
                                              const uint8_t *small, int64_t stride, int32_t cw, int32_t ch,
                                              int32_t mbh, const int64_t *offs, const int64_t *base,
                                              uint8_t *out) {
  const uint32_t n = *n_jobs;
  const int64_t b = *base;
  for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
    const uint4 jb = jobs[j];
    const int s = static_cast<int>(jb.x), mx = static_cast<int>(jb.z);
    const int e = s / mbh, my = s % mbh;
    const uint8_t *src = small + static_cast<int64_t>(ent[e].x) * stride;
    const uint8_t *uv = src + static_cast<int64_t>(cw) * ch;
    uint8_t *dst = out + (offs[s] - b) + jb.y;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const int b = 6 * static_cast<int>(threadIdx.x) + q;
      uint8_t v;
      if (b < 256) {
        v = src[static_cast<int64_t>(my * 16 + (b >> 4)) * cw + mx * 16 + (b & 15)];
      } else {
        const int i = (b - 256) & 63, pl = (b - 256) >> 6;
        v = uv[static_cast<int64_t>(my * 8 + (i >> 3)) * cw + 2 * (mx * 8 + (i & 7)) + pl];
      }
      dst[b] = v;
    }
  }
}

// The macroblocks' QP offsets (vts_transcode_ext9; enc_aq.h), once per call
// ahead of level 0.  Pure streaming, one read of the input pictures: a wave
// takes four macroblocks side by side.  Lane (r, m) = (lane / 4, lane % 4)
// loads the 16 bytes of luma row r of macroblock m, so the four lanes of a row
// read 64 contiguous bytes, and below lane 32 the 16 bytes (8 Cb|Cr pairs) of
// its chroma row r.  A dword gives S1 by a SAD against 0 and S2 by a dot
// product with itself; the sixteen lanes of a macroblock are summed by
// butterflies over lane bits 2..5.  No LDS.  The grid covers whole groups of
// four: a lane whose macroblock lies past the picture's width loads nothing.
__global__ void __launch_bounds__(64) enc_aq(AqArgs a) {
  const int lane = threadIdx.x, r = lane >> 2, m = lane & 3;
  const int groups = (a.mbw + 3) >> 2;
  const int g = blockIdx.x % groups, my = (blockIdx.x / groups) % a.mbh;
  const int64_t f = blockIdx.x / (groups * a.mbh);
  const int mx = 4 * g + m;
  const bool in = mx < a.mbw;
  const uint8_t *pic = a.small + f * a.stride;
  uint32_t s1y = 0, s2y = 0, s1u = 0, s2u = 0, s1v = 0, s2v = 0;
  if (in) {
    const uint4 y = *reinterpret_cast<const uint4 *>(pic + static_cast<int64_t>(my * 16 + r) * a.cw + mx * 16);
    const uint32_t yw[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s1y = __builtin_amdgcn_sad_u8(yw[k], 0u, s1y);
      s2y = __builtin_amdgcn_udot4(yw[k], yw[k], s2y, false);
    }
    if (r < 8) {
      const uint4 c = *reinterpret_cast<const uint4 *>(pic + static_cast<int64_t>(a.cw) * a.ch +
                                                       static_cast<int64_t>(my * 8 + r) * a.cw + mx * 16);
      const uint32_t cw4[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t u = cw4[k] & 0x00ff00ffu, v = (cw4[k] >> 8) & 0x00ff00ffu;
        s1u = __builtin_amdgcn_sad_u8(u, 0u, s1u);
        s2u = __builtin_amdgcn_udot4(u, u, s2u, false);
        s1v = __builtin_amdgcn_sad_u8(v, 0u, s1v);
        s2v = __builtin_amdgcn_udot4(v, v, s2v, false);
      }
    }
  }
#pragma unroll
  for (int off = 4; off < 64; off <<= 1) {
    s1y += __shfl_xor(s1y, off);
    s2y += __shfl_xor(s2y, off);
    s1u += __shfl_xor(s1u, off);
    s2u += __shfl_xor(s2u, off);
    s1v += __shfl_xor(s1v, off);
    s2v += __shfl_xor(s2v, off);
  }
  if (in && r == 0)
    a.aq_off[(f * a.mbh + my) * a.mbw + mx] =
        static_cast<int8_t>(eaq::offset_of_energy(eaq::energy(s1y, s2y, s1u, s2u, s1v, s2v), a.strength_q8, a.aq_max));
}

// The rate controllers (vts_transcode_ext7.bitrate_kbps; enc_ratectl.h), one
// per GOP, behind level j on the search stream: thread t takes entry t of
// level j + 1, whose previous picture is frame - 1 of the same GOP.  A GOP's
// state is touched by its own thread alone; stream order is all the ordering.
__global__ void __launch_bounds__(64) enc_rc(RcArgs a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n_ent) return;
  const int4 en = a.ent[t];
  const int g = en.z >> 1;
  const int64_t bits = a.est_f[en.x - 1];
  const int64_t spent = a.spent[g] + bits;
  a.spent[g] = spent;
  a.qp_f[en.x] = static_cast<uint8_t>(
      full::erc::next_qp(a.frame_bits, a.gop_len[g], a.gop_pos, spent, bits, a.qp_f[en.x - 1], a.qp_min, a.qp_max));
}


// f(std::integral_constant<int, V>{}) for the V that equals v; the last V
// stands for every other value.  The launch functions below pick their
// kernel's instance with it, so that each set of instances is written once.
template <int V, int... Rest, class F>
void with_const(int v, F &&f) {
  if constexpr (sizeof...(Rest) == 0) {
    f(std::integral_constant<int, V>{});
  } else {
    if (v == V) f(std::integral_constant<int, V>{});
    else with_const<Rest...>(v, f);
  }
}

}  // namespace

// ------------------------------------------------------------ launches
static_assert(kPcmCmdWord == kPcmCmd && kNoI4Modes == ei4::kNoModes, "transcode.h restates the kernels' two words");
static_assert(kPcmMbBits == kPcmBits, "... and the I_PCM payload's bits");

// An I_PCM macroblock is < 400 bytes, and so is an inter one (its residual is
// coded only under a 3072-bit bound); the rest is headroom for emulation
// prevention bytes in residual data.  With cabac the decisions are still
// bounded in CAVLC bits, which bounds no CABAC length: the slot holds the
// worst case of the bins themselves (full::ecab::kMbBytes, derived there; the
// larger of the two bounds)
// aq: mb_qp_delta is se(v) of up to 11 bits where 1 was counted, 2 bytes more a
// macroblock in CAVLC; in CABAC up to 41 bins where 1 was, 40 x 7 bits = 35
// bytes, 53 with emulation prevention, on top of the 8628 / 8699 that
// enc_cabac.h derives: kMbBytes still bounds it
int64_t slice_slot_bytes(int mbw, bool cabac, bool aq) {
  const int cavlc = aq ? 602 : 600;
  return ((64 + static_cast<int64_t>(mbw) * (cabac ? std::max(cavlc, full::ecab::kMbBytes) : cavlc)) + 255) & ~int64_t(255);
}

int32_t search_lambda16(int qp, int mv_lambda16) { return er::lambda16(qp, mv_lambda16); }

// one wave per macroblock; RT: the range compiled in (0: any), SP: subpel,
// RC: the instances with the rate-aware decisions compiled in
// PT: those with the partitions of enc_part.h on top (they exist with RC only)
void launch_enc_search(const SearchArgs &a, int subpel, bool rate_aware, bool partitions, int64_t entries, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>(entries * a.nmb));
  with_const<4, 8, 16, 0>(a.range, [&](auto rt) {
    with_const<1, 2, 0>(subpel, [&](auto sp) {
      if (partitions) {
        hipLaunchKernelGGL((enc_search<rt(), sp(), true, true>), grid, dim3(64), 0, s, a);
        return;
      }
      with_const<1, 0>(rate_aware, [&](auto rc) {
        hipLaunchKernelGGL((enc_search<rt(), sp(), rc() != 0>), grid, dim3(64), 0, s, a);
      });
    });
  });
}

// one wave per (entry, macroblock row)
void launch_enc_intra(const IntraArgs &a, bool intra4x4, int64_t entries, hipStream_t s) {
  with_const<1, 0>(intra4x4, [&](auto i4) {
    with_const<1, 0>(a.aq_off != nullptr, [&](auto aq) {
      hipLaunchKernelGGL((enc_intra<i4() != 0, aq() != 0>), dim3(static_cast<unsigned>(entries * a.mbh)), dim3(64), 0, s, a);
    });
  });
}

void launch_enc_deblock(const DeblockArgs &a, int64_t entries, hipStream_t s) {
  with_const<1, 0>(a.mv4 != nullptr, [&](auto pt) {
    hipLaunchKernelGGL(enc_deblock<pt() != 0>, dim3(static_cast<unsigned>(entries * a.mbh)), dim3(64), 0, s, a);
  });
}

// one wave per four macroblocks of a row
void launch_enc_aq(const AqArgs &a, int64_t frames, hipStream_t s) {
  if (frames <= 0) return;
  hipLaunchKernelGGL(enc_aq, dim3(static_cast<unsigned>(frames * a.mbh * ((a.mbw + 3) / 4))), dim3(64), 0, s, a);
}

void launch_enc_rc(const RcArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(enc_rc, dim3(static_cast<unsigned>((a.n_ent + 63) / 64)), dim3(64), 0, s, a);
}

// up to 64 workgroups share a picture, 4096 bytes each
void launch_enc_hash(const HashArgs &a, int64_t entries, hipStream_t s) {
  const int hb = std::max(1, std::min(64, (a.w * a.h * 3 / 2 + 4095) / 4096));
  hipLaunchKernelGGL(enc_hash, dim3(static_cast<unsigned>(hb * entries)), dim3(256), 0, s, a.ent, a.pics, a.stride, a.cw,
                     a.ch, a.w, a.h, hb, a.acc);
}

// a.n_slices slices: CAVLC one lane per slice, CABAC one wave per slice
void launch_enc_write(const WriteArgs &a, bool cabac, bool intra, bool deblock, hipStream_t s) {
  const unsigned ns = static_cast<unsigned>(a.n_slices);
  with_const<1, 0>(intra, [&](auto in) {
    with_const<1, 0>(deblock, [&](auto db) {
      with_const<1, 0>(a.mv4 != nullptr, [&](auto pt) {  // partitions: the level has quadrant vectors
        with_const<1, 0>(a.aq_off != nullptr, [&](auto aq) {  // adaptive quantisation: the call has offsets
          if (cabac)
            hipLaunchKernelGGL((enc_write_cabac<in() != 0, db() != 0, pt() != 0, aq() != 0>), dim3(ns), dim3(64), 0, s, a);
          else
            hipLaunchKernelGGL((enc_write<in() != 0, db() != 0, pt() != 0, aq() != 0>), dim3((ns + 63) / 64), dim3(64), 0, s, a);
        });
      });
    });
  });
}

void launch_enc_pack(const PackArgs &a, int64_t entries, int32_t nmb, hipStream_t s) {
  const int ns = static_cast<int>(entries * a.mbh);
  hipLaunchKernelGGL(enc_scan, dim3(1), dim3(1024), 0, s, a.sizes, ns, a.ent, a.mbh, a.offs, a.total, a.fr_off,
                     a.fr_size);
  hipLaunchKernelGGL(enc_gather, dim3(static_cast<unsigned>(ns)), dim3(256), 0, s, a.staging, a.cap, a.sizes, a.offs,
                     a.base, a.out);
  hipLaunchKernelGGL(enc_pcm, dim3(static_cast<unsigned>(std::min<int64_t>(16384, entries * nmb))), dim3(64), 0, s,
                     a.jobs, a.n_jobs, a.ent, a.small, a.stride, a.cw, a.ch, a.mbh, a.offs, a.base, a.out);
}

}  // namespace vts
