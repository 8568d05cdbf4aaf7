/*
 * transcode_oracle.c — CPU restatement of the 360p upload transcode
 * (the reference's _compress_video_for_upload,
 * src/analyzer/content_analyzer.py:167-236, runs `ffmpeg -vf scale=-2:360
 * -c:v libx264 -crf 28`).  Used ONLY as a checker.
 *
 * TEST INFRASTRUCTURE.  Only tests/ may load this (through liboracle.so);
 * the product (libvtseg.so, its transcode.hip) never links or calls it.
 * Plain scalar C, written from the definition in DESIGN.md §11, not from the
 * device code.
 *
 * Parity: x264 is absent from this image and the GPU pool, and its output is
 * not a function anything here could restate, so byte parity with the
 * reference's compressed file is UNPINNED.  What is pinned: the output size
 * rule (ffmpeg's scale=-2:H: w = 2 * av_rescale(H, W, 2 * srcH), round to
 * nearest), and — by this oracle — every output byte of the device encoder,
 * and a decode of the output by the oracle decoder equals the encoder's own
 * reconstruction.
 *
 * The encoder:
 *   - area downscale of the display-size NV12 frame to (sw, sh), per axis
 *     weights = overlap of source and destination pixel footprints (gcd
 *     reduced), rounded (sum + T/2) / T, then max(1, .) so that I_PCM data
 *     never holds a zero byte; coded size 16-aligned, edge rows/columns
 *     replicated;
 *   - IDR at frame 0, when the GOP reaches `keyint` frames and (opt-in) at
 *     every scene cut (score > threshold): every macroblock I_PCM;
 *   - P pictures, one slice per macroblock row: per macroblock the integer
 *     luma motion (dx, dy), |dx|,|dy| <= R, of least luma SAD against the
 *     previous reconstructed picture (samples outside it edge-clamped as the
 *     decoder's 8.4.2.2.1 reads them; (0,0)
 *     first, then raster order; first minimum wins); inter (P_L0_16x16 or
 *     P_Skip, no residual) if luma+chroma SAD of its prediction (chroma by
 *     8.4.2.2.2) <= T_mb, else I_PCM.
 *   - residual coding (qp >= 1, the default since round 3): the best motion
 *     is always tried with a quantised residual at QP qp (flat scaling,
 *     chroma_qp_index_offset 0): per 4x4 block the forward core transform
 *     W = Cf X Cf^T, levels sign(W) min(2047, (|W| MF + f) >> qbits),
 *     qbits = 15 + qp / 6, f = 2^qbits / 6, MF by position class; chroma DC
 *     through the 2x2 Hadamard at (qbits + 1, 2f); the reconstruction is the
 *     decoder's (8.5.12 scaling + inverse transform, chroma DC 8.5.11).  A
 *     macroblock stays inter when an upper bound of its residual's CAVLC bits
 *     (every code exact but coeff_token, taken as the longest over the nC
 *     classes) is <= 3072 (the I_PCM payload), else it is I_PCM; P_Skip when
 *     its motion is (0, 0) and nothing is coded.  cbp, mb_qp_delta 0 and
 *     residual_block_cavlc with nC from the left macroblock (the one above is
 *     another slice) as 7.3.5.3 / 9.2.1 write them.
 *
 * The three opt-in paths (or_transcode_ex; DESIGN.md §11, "The rules the byte
 * oracle restates"), all off by default and then absent from every byte:
 *   - subpel 1 / 2: around the integer winner the eight half-sample
 *     neighbours, then (2) around that winner the eight quarter-sample ones;
 *     every candidate's prediction per sample straight from 8.4.2.2.1 and Table
 *     8-12 (luma_frac: the integer sample and each of the 15 fractional
 *     positions by its own formula, clamped source coordinates; no shared
 *     planes), cost = luma SAD, key (SAD, index) with the centre index 0;
 *   - intra: the IDR picture's macroblocks, and the P macroblocks the search
 *     left as I_PCM, as Intra16x16 (Horizontal or DC from the left macroblock
 *     of the row's slice, by SAD) where its exact bits are <= 3072;
 *   - deblock: clause 8.7 with disable_deblocking_filter_idc 2 on every
 *     picture's reconstruction before the next picture predicts from it
 *     (deblock_picture, written here; Tables 8-16 / 8-17 from
 *     h264_std_tables.h).
 * tests/test_transcode_oracle.py closes each of them through the general
 * oracle decoder (h264_full_oracle.c, which has its own 8.3.3, 8.4.2.2.1 and
 * 8.7); tests/test_transcode_bytes_gpu.py holds the device to these bytes.
 *
 * The rules merged since (or_transcode_ex2; DESIGN.md §11, "Rate-aware motion
 * cost and early P_Skip", "Intra4x4" and "The byte oracle restates the rate
 * rules and Intra4x4"), again off by default and then absent from every byte.
 * They are written from that text and the standard, not from the product's
 * headers or kernels (none is included), and reuse only this file's own fwd4 /
 * quant1 / idct4 / block_bits / put_residual / Intra16x16:
 *   - early_skip: before the search, the residual of the prediction at vector
 *     (0, 0) through residual_mb; no level left: P_Skip, the prediction is the
 *     reconstruction (encode_p);
 *   - mvcost: the integer pass and both refinement steps order their
 *     candidates by (16 SAD + lambda16 (selen(dx) + selen(dy)), index) against
 *     the predictor guess: the left macroblock's final word in the previous
 *     picture of the GOP (word_vector); lambda16 by the formula
 *     (lambda16_formula), selen by 9.1 with a loop;
 *   - intra4x4: every macroblock of the intra pass also as I_NxN
 *     (intra4_candidate): availability by 6.4.x with one slice per row, the
 *     nine predictions of 8.3.1.2.1 .. 9 one sample at a time (pred4_sample)
 *     over reconstructed neighbours, predIntra4x4PredMode by 8.3.1.1
 *     (pred_mode4), key (16 SAD + lambda16 (1 or 4), mode), exact bits by the
 *     writer itself (put_i4_mb: 7.3.5, 7.3.5.1, Table 9-4's Intra column);
 *     I_NxN when its bits < Intra16x16's, the winner coded when <= 3072 bits.
 * It also returns the command and mode words in include/vtseg.h's encodings
 * and counters of what the input made the rules decide.
 * tests/test_transcode_oracle.py closes these through the general decoder
 * (its own 8.3.1.2) and compares the Intra4x4 rule with the product's CPU
 * harness; tests/test_transcode_bytes_rate_intra4_gpu.py holds the device's
 * words, bytes, counts and hash to them.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "h264_std_tables.h" /* Tables 8-16 / 8-17 (the deblocking filter) */

/* ------------------------------------------------------------ sizes */

/* ffmpeg scale=-2:sh: w = av_rescale(sh, W, 2 * H) * 2 (round to nearest). */
int or_small_width(int W, int H, int sh) {
  int64_t a = (int64_t)sh * W, c = 2 * (int64_t)H;
  return (int)((a + c / 2) / c) * 2;
}

static int64_t gcd64(int64_t a, int64_t b) {
  while (b) { int64_t t = a % b; a = b; b = t; }
  return a;
}

/* area weight of source pixel i for destination pixel o (n source -> m dest),
 * divided by g = gcd(n, m) */
static int64_t area_w(int64_t o, int64_t i, int64_t n, int64_t m) {
  int64_t lo = o * n > i * m ? o * n : i * m;
  int64_t hi = (o + 1) * n < (i + 1) * m ? (o + 1) * n : (i + 1) * m;
  return hi > lo ? (hi - lo) / gcd64(n, m) : 0;
}

/* one plane: src (n_x x n_y, pitch sp, element step es) -> dst (coded cx x cy,
 * display m_x x m_y, pitch dp, step ds) */
static void area_plane(const uint8_t *src, int sp, int es, int nx, int ny, uint8_t *dst, int dp,
                       int ds, int mx, int my, int cx, int cy) {
  int64_t tx = nx / gcd64(nx, mx), ty = ny / gcd64(ny, my);
  for (int y = 0; y < cy; y++) {
    int oy = y < my ? y : my - 1;
    for (int x = 0; x < cx; x++) {
      int ox = x < mx ? x : mx - 1;
      int64_t sum = 0;
      for (int j = (int)((int64_t)oy * ny / my); j < ny && (int64_t)j * my < (int64_t)(oy + 1) * ny; j++) {
        int64_t wy = area_w(oy, j, ny, my);
        for (int i = (int)((int64_t)ox * nx / mx); i < nx && (int64_t)i * mx < (int64_t)(ox + 1) * nx; i++)
          sum += wy * area_w(ox, i, nx, mx) * src[(int64_t)j * sp + (int64_t)i * es];
      }
      int64_t T = tx * ty, v = (sum + T / 2) / T;
      dst[(int64_t)y * dp + (int64_t)x * ds] = (uint8_t)(v < 1 ? 1 : v);
    }
  }
}

/* Display-size NV12 (W x H, pitch W) -> coded NV12 (cw x ch, pitch cw, UV at
 * cw * ch) of display size (sw, sh). */
int or_downscale_nv12(const uint8_t *src, int W, int H, uint8_t *dst, int sw, int sh) {
  int cw = (sw + 15) & ~15, ch = (sh + 15) & ~15;
  if (W < 2 || H < 2 || (W & 1) || (H & 1) || sw < 2 || sh < 2 || (sw & 1) || (sh & 1)) return -1;
  area_plane(src, W, 1, W, H, dst, cw, 1, sw, sh, cw, ch);
  const uint8_t *suv = src + (int64_t)W * H;
  uint8_t *duv = dst + (int64_t)cw * ch;
  area_plane(suv, W, 2, W / 2, H / 2, duv, cw, 2, sw / 2, sh / 2, cw / 2, ch / 2);
  area_plane(suv + 1, W, 2, W / 2, H / 2, duv + 1, cw, 2, sw / 2, sh / 2, cw / 2, ch / 2);
  return 0;
}

/* ------------------------------------------------------ bit writer */

typedef struct {
  uint8_t *rbsp;
  int64_t n, cap;
  uint32_t cur;
  int nb;
} or_bw;

static void bw_bit(or_bw *b, uint32_t v) {
  b->cur = (b->cur << 1) | (v & 1u);
  if (++b->nb == 8) {
    if (b->n < b->cap) b->rbsp[b->n] = (uint8_t)b->cur;
    b->n++;
    b->cur = 0;
    b->nb = 0;
  }
}
static void bw_u(or_bw *b, int n, uint32_t v) {
  for (int i = n - 1; i >= 0; i--) bw_bit(b, (v >> i) & 1u);
}
static void bw_ue(or_bw *b, uint32_t v) {
  uint64_t x = (uint64_t)v + 1;
  int len = 0;
  while ((x >> len) > 1) len++;
  for (int i = 0; i < len; i++) bw_bit(b, 0);
  for (int i = len; i >= 0; i--) bw_bit(b, (uint32_t)(x >> i) & 1u);
}
static void bw_se(or_bw *b, int v) { bw_ue(b, v > 0 ? (uint32_t)(2 * v - 1) : (uint32_t)(-2 * v)); }
static void bw_align(or_bw *b) { while (b->nb) bw_bit(b, 0); }
static void bw_trailing(or_bw *b) { bw_bit(b, 1); bw_align(b); }

/* [4-byte length][header][EBSP of rbsp] appended at out[*pos]; returns 0 or -2 */
static int put_nal(uint8_t *out, int64_t cap, int64_t *pos, uint8_t header, const uint8_t *rbsp,
                   int64_t n) {
  int64_t p = *pos + 4, start = p;
  if (p >= cap) return -2;
  out[p++] = header;
  int zeros = 0;
  for (int64_t i = 0; i < n; i++) {
    uint8_t v = rbsp[i];
    if (zeros >= 2 && v <= 3) {
      if (p >= cap) return -2;
      out[p++] = 3;
      zeros = 0;
    }
    if (p >= cap) return -2;
    out[p++] = v;
    zeros = v == 0 ? zeros + 1 : 0;
  }
  int64_t len = p - start;
  out[*pos] = (uint8_t)(len >> 24);
  out[*pos + 1] = (uint8_t)(len >> 16);
  out[*pos + 2] = (uint8_t)(len >> 8);
  out[*pos + 3] = (uint8_t)len;
  *pos = p;
  return 0;
}

/* ------------------------------------------------- parameter sets */

/* Table A-1: smallest level admitting MaxFS / MaxMBPS (levels 3 .. 5.2). */
int or_pick_level(int mbs, double mbps) {
  static const struct { int idc, fs; double mbps; } t[] = {
      {30, 1620, 40500}, {31, 3600, 108000}, {32, 5120, 216000}, {40, 8192, 245760},
      {42, 8704, 522240}, {50, 22080, 589824}, {51, 36864, 983040}, {52, 36864, 2073600}};
  for (int i = 0; i < 8; i++)
    if (mbs <= t[i].fs && mbps <= t[i].mbps) return t[i].idc;
  return 52;
}

/* SPS / PPS NAL units (header byte + EBSP, no length prefix) of the output. */
int or_sps_pps(int mbw, int mbh, int crop_r, int crop_b, int level, uint8_t *sps, int64_t *sn,
               uint8_t *pps, int64_t *pn) {
  uint8_t tmp[64];
  or_bw b = {tmp, 0, sizeof tmp, 0, 0};
  bw_u(&b, 8, 66);      /* profile_idc Baseline */
  bw_u(&b, 8, 0xC0);    /* constraint_set0/1: Constrained Baseline */
  bw_u(&b, 8, (uint32_t)level);
  bw_ue(&b, 0);         /* sps id */
  bw_ue(&b, 12);        /* log2_max_frame_num_minus4: 16-bit frame_num */
  bw_ue(&b, 2);         /* pic_order_cnt_type 2 */
  bw_ue(&b, 1);         /* max_num_ref_frames */
  bw_u(&b, 1, 0);       /* gaps_in_frame_num_value_allowed_flag */
  bw_ue(&b, (uint32_t)(mbw - 1));
  bw_ue(&b, (uint32_t)(mbh - 1));
  bw_u(&b, 1, 1);       /* frame_mbs_only_flag */
  bw_u(&b, 1, 1);       /* direct_8x8_inference_flag */
  if (crop_r || crop_b) {
    bw_u(&b, 1, 1);
    bw_ue(&b, 0);
    bw_ue(&b, (uint32_t)(crop_r / 2));
    bw_ue(&b, 0);
    bw_ue(&b, (uint32_t)(crop_b / 2));
  } else {
    bw_u(&b, 1, 0);
  }
  bw_u(&b, 1, 0);       /* vui_parameters_present_flag */
  bw_trailing(&b);
  uint8_t buf[80];
  int64_t pos = 0;
  if (put_nal(buf, sizeof buf, &pos, 0x67, tmp, b.n)) return -2;
  *sn = pos - 4;
  memcpy(sps, buf + 4, (size_t)*sn);
  or_bw p = {tmp, 0, sizeof tmp, 0, 0};
  bw_ue(&p, 0);         /* pps id */
  bw_ue(&p, 0);         /* sps id */
  bw_u(&p, 1, 0);       /* CAVLC */
  bw_u(&p, 1, 0);       /* bottom_field_pic_order_in_frame_present_flag */
  bw_ue(&p, 0);         /* num_slice_groups_minus1 */
  bw_ue(&p, 0);         /* num_ref_idx_l0_default_active_minus1 */
  bw_ue(&p, 0);         /* num_ref_idx_l1_default_active_minus1 */
  bw_u(&p, 1, 0);       /* weighted_pred_flag */
  bw_u(&p, 2, 0);       /* weighted_bipred_idc */
  bw_se(&p, 0);         /* pic_init_qp_minus26 */
  bw_se(&p, 0);         /* pic_init_qs_minus26 */
  bw_se(&p, 0);         /* chroma_qp_index_offset */
  bw_u(&p, 1, 1);       /* deblocking_filter_control_present_flag */
  bw_u(&p, 1, 0);       /* constrained_intra_pred_flag */
  bw_u(&p, 1, 0);       /* redundant_pic_cnt_present_flag */
  bw_trailing(&p);
  pos = 0;
  if (put_nal(buf, sizeof buf, &pos, 0x68, tmp, p.n)) return -2;
  *pn = pos - 4;
  memcpy(pps, buf + 4, (size_t)*pn);
  return 0;
}

/* ------------------------------------------------------- encoder */

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
/* Table 9-4 (chroma_format_idc 1), inter column: codeNum -> coded_block_pattern */
static const int CBP_P[48] = {0,  16, 1,  2,  4,  8,  32, 3,  5,  10, 12, 15, 47, 7,  11, 13,
                              14, 6,  9,  31, 35, 37, 42, 44, 33, 34, 36, 40, 39, 43, 45, 46,
                              17, 18, 20, 24, 19, 21, 26, 28, 23, 27, 29, 30, 22, 25, 38, 41};

typedef struct {
  int pcm, mvx, mvy;  /* mv in quarter-pel */
  int cbp;            /* coded_block_pattern of an inter or Intra16x16 macroblock */
  int i16;            /* Intra16x16 (pcm = 0, no motion) */
  int lmode, cmode;   /* Intra16x16PredMode, intra_chroma_pred_mode */
  int i4;             /* I_NxN, sixteen Intra_4x4 blocks (pcm = i16 = 0, no motion); levels in the inter layout */
  uint64_t modes;     /* I_NxN: nibble k = Intra4x4PredMode of luma4x4BlkIdx k */
  int16_t lv[384];    /* levels in scan order: luma by luma4x4BlkIdx (16 x 16), Cb / Cr DC (2 x 4),
                         Cb / Cr AC by chroma4x4BlkIdx (8 x 15); Intra16x16: Intra16x16DCLevel in
                         [0, 16), Intra16x16ACLevel of block k in [16 + 15 k, 31 + 15 k) */
} or_mb;

/* ------------------------------------------------------ residual coding */

const char *fo_table_code(int table, int a, int b, int c);  /* h264_full_oracle.c: the standard's strings */
static int code_len(int table, int a, int b, int c) {
  const char *s = fo_table_code(table, a, b, c);
  return s ? (int)strlen(s) : -1;
}
static void put_code(or_bw *b, int table, int a, int bb, int c) {
  const char *s = fo_table_code(table, a, bb, c);
  for (; s && *s; s++) bw_bit(b, (uint32_t)(*s - '0'));
}

static const int ZZ[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15}; /* 8.5.6 */
/* luma4x4BlkIdx -> raster 4x4 position (6.4.3) */
static const int BLK_X[16] = {0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3};
static const int BLK_Y[16] = {0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3};
/* quantisation multipliers by qP % 6 and position class (0: both coordinates
 * even, 1: both odd, 2: mixed); the encoder's choice, the inverse of 8.5.9's
 * v = {10, 16, 13} ... so that (v MF) ~ 2^17 */
static const int MF[6][3] = {{13107, 5243, 8066}, {11916, 4660, 7490}, {10082, 4194, 6554},
                             {9362, 3647, 5825},  {8192, 3355, 5243},  {7282, 2893, 4559}};
static const int NV[6][3] = {{10, 16, 13}, {11, 18, 14}, {13, 20, 16}, {14, 23, 18}, {16, 25, 20}, {18, 29, 23}};
static const int QPC[52] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17,
                            18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32, 32, 33,
                            34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39};
static int pos_class(int i, int j) { return (!(i & 1) && !(j & 1)) ? 0 : ((i & 1) && (j & 1) ? 1 : 2); }

/* W = Cf X Cf^T, Cf = [1 1 1 1; 2 1 -1 -2; 1 -1 -1 1; 1 -2 2 -1]; raster */
static void fwd4(const int *x, int *w) {
  static const int Cf[4][4] = {{1, 1, 1, 1}, {2, 1, -1, -2}, {1, -1, -1, 1}, {1, -2, 2, -1}};
  int t[16];
  for (int i = 0; i < 4; i++)
    for (int k = 0; k < 4; k++) {
      int a = 0;
      for (int j = 0; j < 4; j++) a += x[i * 4 + j] * Cf[k][j];
      t[i * 4 + k] = a;
    }
  for (int k = 0; k < 4; k++)
    for (int c = 0; c < 4; c++) {
      int a = 0;
      for (int i = 0; i < 4; i++) a += Cf[k][i] * t[i * 4 + c];
      w[k * 4 + c] = a;
    }
}
static int quant1(int w, int mf, int qbits, int64_t f) {
  int64_t z = ((int64_t)abs(w) * mf + f) >> qbits;
  if (z > 2047) z = 2047;
  return w < 0 ? -(int)z : (int)z;
}
/* 8.5.12.1 scaling (flat) + 8.5.12.2 inverse transform; dc_done: c[0] already scaled */
static void idct4(const int *c, int qp, int dc_done, int *r) {
  int d[16], f[16];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      int k = i * 4 + j;
      if (k == 0 && dc_done) { d[0] = c[0]; continue; }
      int ls = 16 * NV[qp % 6][pos_class(i, j)];
      d[k] = qp >= 24 ? (c[k] * ls) << (qp / 6 - 4) : (c[k] * ls + (1 << (3 - qp / 6))) >> (4 - qp / 6);
    }
  for (int i = 0; i < 4; i++) {
    int e0 = d[i * 4] + d[i * 4 + 2], e1 = d[i * 4] - d[i * 4 + 2];
    int e2 = (d[i * 4 + 1] >> 1) - d[i * 4 + 3], e3 = d[i * 4 + 1] + (d[i * 4 + 3] >> 1);
    f[i * 4] = e0 + e3; f[i * 4 + 1] = e1 + e2; f[i * 4 + 2] = e1 - e2; f[i * 4 + 3] = e0 - e3;
  }
  for (int j = 0; j < 4; j++) {
    int g0 = f[j] + f[8 + j], g1 = f[j] - f[8 + j];
    int g2 = (f[4 + j] >> 1) - f[12 + j], g3 = f[4 + j] + (f[12 + j] >> 1);
    r[j] = (g0 + g3 + 32) >> 6; r[4 + j] = (g1 + g2 + 32) >> 6;
    r[8 + j] = (g1 - g2 + 32) >> 6; r[12 + j] = (g0 - g3 + 32) >> 6;
  }
}

/* residual_block_cavlc of levels lv[0, maxNum) (scan order) with nC (-1:
 * chroma DC); bits to b, or (b == NULL) only counted; coeff_token counted as
 * the longest code over the nC classes when nC < -1 (the bound) */
static int block_bits(or_bw *b, const int16_t *lv, int maxNum, int nC) {
  int pos[16], lev[16], tc = 0, bits = 0;
  for (int i = maxNum - 1; i >= 0; i--)
    if (lv[i]) { pos[tc] = i; lev[tc++] = lv[i]; }
  int t1 = 0;
  while (t1 < tc && t1 < 3 && (lev[t1] == 1 || lev[t1] == -1)) t1++;
  if (nC < -1) {  /* upper bound over every nC class: Table 9-5 columns and the 6-bit FLC */
    int m = 6;
    for (int c = 0; c < 3; c++) { int l = code_len(0, c, tc, t1); if (l > m) m = l; }
    bits += m;
  } else if (nC >= 8) {
    bits += 6;
    if (b) bw_u(b, 6, tc == 0 ? 3u : (uint32_t)(((tc - 1) << 2) | t1));
  } else {
    int col = nC == -1 ? 3 : (nC < 2 ? 0 : (nC < 4 ? 1 : 2));
    bits += code_len(0, col, tc, t1);
    if (b) put_code(b, 0, col, tc, t1);
  }
  if (tc == 0) return bits;
  for (int i = 0; i < t1; i++) { bits++; if (b) bw_bit(b, lev[i] < 0); }
  int sl = (tc > 10 && t1 < 3) ? 1 : 0;
  for (int i = t1; i < tc; i++) {  /* 9.2.2.1 inverted */
    int level = lev[i];
    int code = level > 0 ? 2 * level - 2 : -2 * level - 1;
    if (i == t1 && t1 < 3) code -= 2;
    int prefix, suffix = 0, ssize = 0;
    if (sl == 0) {
      if (code < 14) prefix = code;
      else if (code < 30) { prefix = 14; suffix = code - 14; ssize = 4; }
      else { prefix = 15; suffix = code - 30; ssize = 12; }
    } else {
      if (code < (15 << sl)) { prefix = code >> sl; suffix = code & ((1 << sl) - 1); ssize = sl; }
      else { prefix = 15; suffix = code - (15 << sl); ssize = 12; }
    }
    bits += prefix + 1 + ssize;
    if (b) {
      for (int z = 0; z < prefix; z++) bw_bit(b, 0);
      bw_bit(b, 1);
      if (ssize) bw_u(b, ssize, (uint32_t)suffix);
    }
    if (sl == 0) sl = 1;
    if (abs(level) > (3 << (sl - 1)) && sl < 6) sl++;
  }
  int zeros = pos[0] + 1 - tc;
  if (tc < maxNum) {
    int t = maxNum == 4 ? 2 : 1;
    bits += code_len(t, tc - 1, zeros, 0);
    if (b) put_code(b, t, tc - 1, zeros, 0);
  }
  for (int i = 0; i < tc - 1 && zeros > 0; i++) {
    int run = pos[i] - pos[i + 1] - 1, row = (zeros < 7 ? zeros : 7) - 1;
    bits += code_len(3, row, run, 0);
    if (b) put_code(b, 3, row, run, 0);
    zeros -= run;
  }
  return bits;
}

/* Quantise the macroblock's residual (src - prediction) at qp, reconstruct
 * into ry / ru / rv (16x16, 8x8, 8x8 samples) and return the residual's
 * CAVLC bit bound; levels and cbp into m. */
static int residual_mb(const uint8_t *sy, const uint8_t *su, const uint8_t *sv, const uint8_t *py,
                       const uint8_t *pu, const uint8_t *pv, int qp, or_mb *m, uint8_t *ry, uint8_t *ru,
                       uint8_t *rv) {
  int qbits = 15 + qp / 6;
  int64_t f = ((int64_t)1 << qbits) / 6;
  int cbp = 0, bound = 0, nz[16];
  memset(m->lv, 0, sizeof m->lv);
  for (int k = 0; k < 16; k++) {  /* luma, luma4x4BlkIdx order */
    int bx = BLK_X[k] * 4, by = BLK_Y[k] * 4, x[16], w[16], z[16], r[16];
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) x[i * 4 + j] = sy[(by + i) * 16 + bx + j] - py[(by + i) * 16 + bx + j];
    fwd4(x, w);
    nz[k] = 0;
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) {
        z[i * 4 + j] = quant1(w[i * 4 + j], MF[qp % 6][pos_class(i, j)], qbits, f);
        nz[k] |= z[i * 4 + j] != 0;
      }
    for (int s = 0; s < 16; s++) m->lv[16 * k + s] = (int16_t)z[ZZ[s]];
    idct4(z, qp, 0, r);
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) {
        int v = py[(by + i) * 16 + bx + j] + r[i * 4 + j];
        ry[(by + i) * 16 + bx + j] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
      }
    if (nz[k]) cbp |= 1 << (k >> 2);
  }
  for (int k8 = 0; k8 < 4; k8++)
    if ((cbp >> k8) & 1)
      for (int k = 4 * k8; k < 4 * k8 + 4; k++) bound += block_bits(NULL, m->lv + 16 * k, 16, -2);
  int qpc = QPC[qp], cqb = 15 + qpc / 6;
  int64_t cf = ((int64_t)1 << cqb) / 6;
  int dcnz = 0, acnz = 0, acz[2][4][16], dcl[2][4];
  for (int pl = 0; pl < 2; pl++) {
    const uint8_t *s = pl ? sv : su, *p = pl ? pv : pu;
    int wdc[4];
    for (int k = 0; k < 4; k++) {
      int bx = (k & 1) * 4, by = (k >> 1) * 4, x[16], w[16];
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) x[i * 4 + j] = s[(by + i) * 8 + bx + j] - p[(by + i) * 8 + bx + j];
      fwd4(x, w);
      wdc[k] = w[0];
      acz[pl][k][0] = 0;
      for (int q = 1; q < 16; q++) {
        int i = q >> 2, j = q & 3;
        acz[pl][k][q] = quant1(w[q], MF[qpc % 6][pos_class(i, j)], cqb, cf);
        acnz |= acz[pl][k][q] != 0;
      }
      for (int sidx = 1; sidx < 16; sidx++) m->lv[264 + pl * 60 + k * 15 + sidx - 1] = (int16_t)acz[pl][k][ZZ[sidx]];
    }
    int fd[4] = {wdc[0] + wdc[1] + wdc[2] + wdc[3], wdc[0] - wdc[1] + wdc[2] - wdc[3],
                 wdc[0] + wdc[1] - wdc[2] - wdc[3], wdc[0] - wdc[1] - wdc[2] + wdc[3]};
    for (int k = 0; k < 4; k++) {
      dcl[pl][k] = quant1(fd[k], MF[qpc % 6][0], cqb + 1, 2 * cf);
      dcnz |= dcl[pl][k] != 0;
      m->lv[256 + 4 * pl + k] = (int16_t)dcl[pl][k];
    }
  }
  int cc = acnz ? 2 : (dcnz ? 1 : 0);
  cbp |= cc << 4;
  if (cc) for (int pl = 0; pl < 2; pl++) bound += block_bits(NULL, m->lv + 256 + 4 * pl, 4, -1);
  if (cc == 2) for (int b = 0; b < 8; b++) bound += block_bits(NULL, m->lv + 264 + 15 * b, 15, -2);
  /* chroma reconstruction (8.5.11: DC through the 2x2 transform, then 8.5.12) */
  for (int pl = 0; pl < 2; pl++) {
    const int *c = dcl[pl];
    int F[4] = {c[0] + c[1] + c[2] + c[3], c[0] - c[1] + c[2] - c[3], c[0] + c[1] - c[2] - c[3],
                c[0] - c[1] - c[2] + c[3]};
    const uint8_t *p = pl ? pv : pu;
    uint8_t *rr = pl ? rv : ru;
    for (int k = 0; k < 4; k++) {
      int co[16], r[16], bx = (k & 1) * 4, by = (k >> 1) * 4;
      for (int q = 0; q < 16; q++) co[q] = cc == 2 ? acz[pl][k][q] : 0;
      co[0] = ((F[k] * 16 * NV[qpc % 6][0]) << (qpc / 6)) >> 5;
      idct4(co, qpc, 1, r);
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
          int v = p[(by + i) * 8 + bx + j] + r[i * 4 + j];
          rr[(by + i) * 8 + bx + j] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    }
  }
  /* without a luma 8x8 bit its levels are not coded: the decoder sees zeros */
  for (int k8 = 0; k8 < 4; k8++)
    if (!((cbp >> k8) & 1))
      for (int k = 4 * k8; k < 4 * k8 + 4; k++) {
        int bx = BLK_X[k] * 4, by = BLK_Y[k] * 4;
        for (int i = 0; i < 4; i++)
          for (int j = 0; j < 4; j++) ry[(by + i) * 16 + bx + j] = py[(by + i) * 16 + bx + j];
      }
  m->cbp = cbp;
  return bound;
}

/* ---- 8.4.2.2.1, one luma sample at a time.  L: the reference sample at
 * (x, y), clamped into the picture (8-239 / 8-240). */
static int ref_l(const uint8_t *ref, int cw, int ch, int x, int y) {
  return ref[(int64_t)clampi(y, 0, ch - 1) * cw + clampi(x, 0, cw - 1)];
}
static int tap6i(int a, int b, int c, int d, int e, int f) { return a - 5 * b + 20 * c + 20 * d - 5 * e + f; }
static int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
/* b1 (8-241): the horizontal intermediate between (x, y) and (x + 1, y) */
static int hz1(const uint8_t *r, int cw, int ch, int x, int y) {
  return tap6i(ref_l(r, cw, ch, x - 2, y), ref_l(r, cw, ch, x - 1, y), ref_l(r, cw, ch, x, y),
               ref_l(r, cw, ch, x + 1, y), ref_l(r, cw, ch, x + 2, y), ref_l(r, cw, ch, x + 3, y));
}
/* h1 (8-242): the vertical intermediate between (x, y) and (x, y + 1) */
static int vt1(const uint8_t *r, int cw, int ch, int x, int y) {
  return tap6i(ref_l(r, cw, ch, x, y - 2), ref_l(r, cw, ch, x, y - 1), ref_l(r, cw, ch, x, y),
               ref_l(r, cw, ch, x, y + 1), ref_l(r, cw, ch, x, y + 2), ref_l(r, cw, ch, x, y + 3));
}
static int half_b(const uint8_t *r, int cw, int ch, int x, int y) { return clip255((hz1(r, cw, ch, x, y) + 16) >> 5); }
static int half_h(const uint8_t *r, int cw, int ch, int x, int y) { return clip255((vt1(r, cw, ch, x, y) + 16) >> 5); }
/* j (8-245 / 8-246): the six horizontal intermediates of rows y - 2 .. y + 3 */
static int half_j(const uint8_t *r, int cw, int ch, int x, int y) {
  int j1 = tap6i(hz1(r, cw, ch, x, y - 2), hz1(r, cw, ch, x, y - 1), hz1(r, cw, ch, x, y),
                 hz1(r, cw, ch, x, y + 1), hz1(r, cw, ch, x, y + 2), hz1(r, cw, ch, x, y + 3));
  return clip255((j1 + 512) >> 10);
}
/* The predicted luma sample for full-sample location (x, y) and fraction
 * (xf, yf), Table 8-12 with Figure 8-4's names: G (x, y), H (x + 1, y), M
 * (x, y + 1); b, s the horizontal half samples of rows y, y + 1; h, m the
 * vertical ones of columns x, x + 1; j the centre. */
static int luma_frac(const uint8_t *r, int cw, int ch, int x, int y, int xf, int yf) {
  int G = ref_l(r, cw, ch, x, y), H = ref_l(r, cw, ch, x + 1, y), M = ref_l(r, cw, ch, x, y + 1);
  switch (4 * xf + yf) {
    case 0: return G;
    case 1: return (G + half_h(r, cw, ch, x, y) + 1) >> 1;                                 /* d */
    case 2: return half_h(r, cw, ch, x, y);                                                /* h */
    case 3: return (M + half_h(r, cw, ch, x, y) + 1) >> 1;                                 /* n */
    case 4: return (G + half_b(r, cw, ch, x, y) + 1) >> 1;                                 /* a */
    case 5: return (half_b(r, cw, ch, x, y) + half_h(r, cw, ch, x, y) + 1) >> 1;           /* e */
    case 6: return (half_h(r, cw, ch, x, y) + half_j(r, cw, ch, x, y) + 1) >> 1;           /* i */
    case 7: return (half_h(r, cw, ch, x, y) + half_b(r, cw, ch, x, y + 1) + 1) >> 1;       /* p = (h + s) */
    case 8: return half_b(r, cw, ch, x, y);                                                /* b */
    case 9: return (half_b(r, cw, ch, x, y) + half_j(r, cw, ch, x, y) + 1) >> 1;           /* f */
    case 10: return half_j(r, cw, ch, x, y);                                               /* j */
    case 11: return (half_j(r, cw, ch, x, y) + half_b(r, cw, ch, x, y + 1) + 1) >> 1;      /* q = (j + s) */
    case 12: return (H + half_b(r, cw, ch, x, y) + 1) >> 1;                                /* c */
    case 13: return (half_b(r, cw, ch, x, y) + half_h(r, cw, ch, x + 1, y) + 1) >> 1;      /* g = (b + m) */
    case 14: return (half_j(r, cw, ch, x, y) + half_h(r, cw, ch, x + 1, y) + 1) >> 1;      /* k = (j + m) */
    default: return (half_h(r, cw, ch, x + 1, y) + half_b(r, cw, ch, x, y + 1) + 1) >> 1;  /* r = (m + s) */
  }
}
/* luma prediction of macroblock (mx, my) at the quarter-sample vector (mvx, mvy) */
static void predict_luma(const uint8_t *ref, int cw, int ch, int mx, int my, int mvx, int mvy, uint8_t *py) {
  for (int j = 0; j < 16; j++)
    for (int i = 0; i < 16; i++)
      py[j * 16 + i] = (uint8_t)luma_frac(ref, cw, ch, mx * 16 + i + (mvx >> 2), my * 16 + j + (mvy >> 2),
                                          mvx & 3, mvy & 3);
}
static int64_t luma_sad(const uint8_t *src, int cw, int mx, int my, const uint8_t *py) {
  int64_t s = 0;
  for (int j = 0; j < 16; j++)
    for (int i = 0; i < 16; i++) s += abs((int)py[j * 16 + i] - (int)src[(int64_t)(my * 16 + j) * cw + mx * 16 + i]);
  return s;
}

/* prediction of one macroblock from ref (coded NV12 cw x ch) at the
 * quarter-sample luma vector (mvx, mvy): luma 8.4.2.2.1 (an integer vector
 * reads the clamped sample itself), chroma 8.4.2.2.2 with edge clamping */
static void predict_mb(const uint8_t *ref, int cw, int ch, int mx, int my, int mvx, int mvy,
                       uint8_t *py, uint8_t *pu, uint8_t *pv) {
  predict_luma(ref, cw, ch, mx, my, mvx, mvy, py);
  const uint8_t *uv = ref + (int64_t)cw * ch;
  int fx = mvx & 7, fy = mvy & 7, ccw = cw / 2, cch = ch / 2;
  for (int j = 0; j < 8; j++)
    for (int i = 0; i < 8; i++) {
      int xi = mx * 8 + i + (mvx >> 3), yi = my * 8 + j + (mvy >> 3);
      int xa = clampi(xi, 0, ccw - 1), xb = clampi(xi + 1, 0, ccw - 1);
      int ya = clampi(yi, 0, cch - 1), yb = clampi(yi + 1, 0, cch - 1);
      for (int pl = 0; pl < 2; pl++) {
        int A = uv[(int64_t)ya * cw + 2 * xa + pl], B = uv[(int64_t)ya * cw + 2 * xb + pl];
        int C = uv[(int64_t)yb * cw + 2 * xa + pl], D = uv[(int64_t)yb * cw + 2 * xb + pl];
        int v = ((8 - fx) * (8 - fy) * A + fx * (8 - fy) * B + (8 - fx) * fy * C + fx * fy * D + 32) >> 6;
        (pl ? pv : pu)[j * 8 + i] = (uint8_t)v;
      }
    }
}

/* ---- the opt-in rules of or_transcode_ex2 ("Rate-aware motion
 * cost and early P_Skip", "Intra4x4") */

/* the decision counters of or_transcode_ex2 (what the inputs of a test made
 * the rules decide) */
enum {
  OC_MODE0 = 0,      /* [0, 9): blocks that chose Intra4x4PredMode 0 .. 8 */
  OC_DISCOUNT = 9,   /* blocks whose winner is not the mode of least (SAD, mode): the rate term decided */
  OC_COST_TIE = 10,  /* blocks whose least cost two or more modes share: the lower mode number decided */
  OC_I4_WON = 11,    /* macroblocks whose I_NxN bits < their Intra16x16 bits */
  OC_I16_WON = 12,   /* macroblocks whose I_NxN bits >= their Intra16x16 bits */
  OC_EQUAL_BITS = 13,/* of those, equal bits (the tie that Intra16x16 wins) */
  OC_I4_PCM = 14,    /* macroblocks left I_PCM by the 3072 bound although I_NxN was the cheaper */
  OC_COST_MV = 15,   /* vector decisions (a pass of one macroblock) whose winner is not that of (SAD, index) */
  OC_EARLY = 16,     /* early P_Skip hits */
  OC_PHAT = 17,      /* searched macroblocks whose predictor guess is a non-zero vector of an inter word */
  OC_N = 18
};

typedef struct {
  int mvcost, early_skip, intra4x4;
  int lambda_mv;  /* 16 lambda of the vector cost */
  int lambda_i4;  /* 16 lambda of the Intra4x4 mode cost: always the formula's */
} or_opts;

/* 16 lambda of a SAD-domain Lagrangian: the square root of 0.85 2^((qp - 12) / 3), rounded */
static int lambda16_formula(int qp) { return (int)(16.0 * sqrt(0.85 * pow(2.0, (qp - 12) / 3.0)) + 0.5); }

/* the length of se(v) for the value k (9.1, 9.1.1): codeNum = 2|k| - (k > 0),
 * leadingZeroBits = floor(log2(codeNum + 1)), 2 leadingZeroBits + 1 bits */
static int selen(int k) {
  uint32_t x = (k > 0 ? (uint32_t)(2 * k - 1) : (uint32_t)(-2 * k)) + 1;
  int lz = 0;
  while ((x >> lz) > 1) lz++;
  return 2 * lz + 1;
}

/* the command word of a macroblock as include/vtseg.h documents it */
static uint32_t mb_word(const or_mb *m) {
  if (m->pcm) return 0x80008000u;
  if (m->i16) return 0x80000000u | (uint32_t)(m->lmode | (m->cmode << 2) | (m->cbp << 4));
  if (m->i4) return 0x80004000u | (uint32_t)((m->cmode << 2) | (m->cbp << 4));
  return ((uint32_t)m->mvx & 0xffffu) | (((uint32_t)m->mvy & 0xffffu) << 16);
}

/* the vector an inter word holds, in quarter samples; (0, 0) for every intra kind */
static void word_vector(uint32_t w, int *vx, int *vy) {
  *vx = *vy = 0;
  if ((w & 0xffff8000u) == 0x80000000u || w == 0x80008000u) return;  /* Intra16x16, I_NxN; I_PCM */
  *vx = (int16_t)(w & 0xffffu);
  *vy = (int16_t)(w >> 16);
}

/* encode one P picture's decisions and reconstruction (qp >= 1: residual coding).
 * o: the opt-in rules (all zero: none); pw: the final command words of the
 * previous picture, j: this picture's position in its GOP (for the predictor
 * guess of the vector cost); cnt: the decision counters */
static void encode_p(const uint8_t *src, const uint8_t *ref, uint8_t *rec, int cw, int ch, int R,
                     int T, int qp, int subpel, const or_opts *o, const uint32_t *pw, int gop_j, or_mb *mbs,
                     int64_t *stats, int64_t *cnt) {
  int mbw = cw / 16, mbh = ch / 16;
  const uint8_t *suv = src + (int64_t)cw * ch;
  uint8_t *ruv = rec + (int64_t)cw * ch;
  int side = 2 * R + 1, ncand = side * side, center = R * side + R;
  int64_t n_frac = 0, n_quarter = 0, n_early = 0, n_costmv = 0, n_phat = 0;
  int rate_ok = qp >= 1 && T >= 0;  /* both rules need residual coding and inter macroblocks */
  int lam = (o->mvcost && rate_ok) ? o->lambda_mv : 0;
  /* the macroblocks of a P picture are independent of each other (each reads
   * the previous picture): threads only shorten the checker's run */
#pragma omp parallel for collapse(2) schedule(dynamic, 4) reduction(+ : n_frac, n_quarter, n_early, n_costmv, n_phat)
  for (int my = 0; my < mbh; my++)
    for (int mx = 0; mx < mbw; mx++) {
      uint8_t py[256], pu[64], pv[64];
      or_mb *m = &mbs[my * mbw + mx];
      if (o->early_skip && rate_ok) {
        /* (a) early P_Skip: the residual at vector (0, 0) quantises to nothing */
        uint8_t sy[256], su[64], sv[64], ry[256], ru[64], rv[64];
        for (int j = 0; j < 16; j++)
          for (int i = 0; i < 16; i++) sy[j * 16 + i] = src[(int64_t)(my * 16 + j) * cw + mx * 16 + i];
        for (int j = 0; j < 8; j++)
          for (int i = 0; i < 8; i++) {
            int64_t q = (int64_t)(my * 8 + j) * cw + 2 * (mx * 8 + i);
            su[j * 8 + i] = suv[q];
            sv[j * 8 + i] = suv[q + 1];
          }
        predict_mb(ref, cw, ch, mx, my, 0, 0, py, pu, pv);
        residual_mb(sy, su, sv, py, pu, pv, qp, m, ry, ru, rv);
        if (m->cbp == 0) {  /* decided: vector (0, 0), word 0, the prediction is the reconstruction */
          m->pcm = m->i16 = m->i4 = m->mvx = m->mvy = 0;
          for (int j = 0; j < 16; j++)
            for (int i = 0; i < 16; i++) rec[(int64_t)(my * 16 + j) * cw + mx * 16 + i] = py[j * 16 + i];
          for (int j = 0; j < 8; j++)
            for (int i = 0; i < 8; i++) {
              int64_t q = (int64_t)(my * 8 + j) * cw + 2 * (mx * 8 + i);
              ruv[q] = pu[j * 8 + i];
              ruv[q + 1] = pv[j * 8 + i];
            }
          n_early++;
          continue;
        }
      }
      /* (b) the predictor guess of the vector cost: (0, 0) in column 0 and in
       * the first P picture of a GOP, else what the final word of the left
       * macroblock in the previous picture holds */
      int phx = 0, phy = 0;
      if (lam && mx > 0 && gop_j > 1) word_vector(pw[my * mbw + mx - 1], &phx, &phy);
      if (phx || phy) n_phat++;
      /* the integer pass: key (16 SAD + lambda16 bits(v - guess), index), index
       * 0 the centre, then raster order; the least key wins (lam = 0: the SAD's order) */
      int64_t best = -1, best_sad = 0, least_sad = -1;
      int bdx = 0, bdy = 0, least_c = 0, best_c = 0;
      for (int c = 0; c < ncand; c++) {
        int r = c == 0 ? center : (c - 1 < center ? c - 1 : c);
        int dy = r / side - R, dx = r % side - R;
        int x0 = mx * 16 + dx, y0 = my * 16 + dy;
        int64_t s = 0;  /* reference samples outside the picture: edge clamped (8.4.2.2.1) */
        for (int j = 0; j < 16; j++)
          for (int i = 0; i < 16; i++)
            s += abs((int)ref[(int64_t)clampi(y0 + j, 0, ch - 1) * cw + clampi(x0 + i, 0, cw - 1)] -
                     (int)src[(int64_t)(my * 16 + j) * cw + mx * 16 + i]);
        int64_t cost = 16 * s + (int64_t)lam * (selen(4 * dx - phx) + selen(4 * dy - phy));
        if (least_sad < 0 || s < least_sad) { least_sad = s; least_c = c; }
        if (best < 0 || cost < best) { best = cost; best_sad = s; best_c = c; bdx = dx; bdy = dy; }
      }
      if (best_c != least_c) n_costmv++;
      /* sub-sample refinement: around the
       * integer winner in steps of 2, then (subpel == 2) around that winner in
       * steps of 1; key (cost, index), the centre index 0 with its bits counted
       * anew, the other eight 1..8 in raster order of (j, i); the least key wins */
      int wmvx = 4 * bdx, wmvy = 4 * bdy;
      int64_t wsad = best_sad;
      for (int step = 2; subpel >= 1 && step >= (subpel == 2 ? 1 : 2); step >>= 1) {
        int cx = wmvx, cy = wmvy;  /* the centre keeps its SAD and wins ties; then raster order */
        int64_t wcost = 16 * wsad + (int64_t)lam * (selen(cx - phx) + selen(cy - phy));
        int64_t lsad = wsad;
        int idx = 0, widx = 0, lidx = 0;
        for (int j = -1; j <= 1; j++)
          for (int i = -1; i <= 1; i++) {
            if (!i && !j) continue;
            idx++;
            int vx = cx + step * i, vy = cy + step * j;
            predict_luma(ref, cw, ch, mx, my, vx, vy, py);
            int64_t s = luma_sad(src, cw, mx, my, py);
            int64_t cost = 16 * s + (int64_t)lam * (selen(vx - phx) + selen(vy - phy));
            if (s < lsad) { lsad = s; lidx = idx; }
            if (cost < wcost) { wcost = cost; wsad = s; widx = idx; wmvx = vx; wmvy = vy; }
          }
        if (widx != lidx) n_costmv++;
      }
      predict_mb(ref, cw, ch, mx, my, wmvx, wmvy, py, pu, pv);
      int64_t cost = 0;
      for (int j = 0; j < 16; j++)
        for (int i = 0; i < 16; i++)
          cost += abs((int)py[j * 16 + i] - (int)src[(int64_t)(my * 16 + j) * cw + mx * 16 + i]);
      for (int j = 0; j < 8; j++)
        for (int i = 0; i < 8; i++) {
          int64_t o = (int64_t)(my * 8 + j) * cw + 2 * (mx * 8 + i);
          cost += abs((int)pu[j * 8 + i] - (int)suv[o]) + abs((int)pv[j * 8 + i] - (int)suv[o + 1]);
        }
      m->cbp = 0;
      int inter;
      if (qp >= 1) {  /* residual coding: inter unless the residual costs more than I_PCM */
        uint8_t sy[256], su[64], sv[64];
        for (int j = 0; j < 16; j++)
          for (int i = 0; i < 16; i++) sy[j * 16 + i] = src[(int64_t)(my * 16 + j) * cw + mx * 16 + i];
        for (int j = 0; j < 8; j++)
          for (int i = 0; i < 8; i++) {
            int64_t o = (int64_t)(my * 8 + j) * cw + 2 * (mx * 8 + i);
            su[j * 8 + i] = suv[o];
            sv[j * 8 + i] = suv[o + 1];
          }
        uint8_t ry[256], ru[64], rv[64];
        int bound = residual_mb(sy, su, sv, py, pu, pv, qp, m, ry, ru, rv);
        inter = T >= 0 && bound <= 3072;
        if (inter) {
          memcpy(py, ry, 256);
          memcpy(pu, ru, 64);
          memcpy(pv, rv, 64);
        } else {
          m->cbp = 0;
        }
      } else {
        inter = T >= 0 && cost <= T;
      }
      m->pcm = !inter;
      m->i16 = m->i4 = 0;
      m->mvx = inter ? wmvx : 0;
      m->mvy = inter ? wmvy : 0;
      if (inter && ((wmvx | wmvy) & 3)) {  /* a fractional vector; one with an odd component */
        n_frac++;
        if ((wmvx | wmvy) & 1) n_quarter++;
      }
      for (int j = 0; j < 16; j++)
        for (int i = 0; i < 16; i++) {
          int64_t o = (int64_t)(my * 16 + j) * cw + mx * 16 + i;
          rec[o] = inter ? py[j * 16 + i] : src[o];
        }
      for (int j = 0; j < 8; j++)
        for (int i = 0; i < 8; i++) {
          int64_t o = (int64_t)(my * 8 + j) * cw + 2 * (mx * 8 + i);
          ruv[o] = inter ? pu[j * 8 + i] : suv[o];
          ruv[o + 1] = inter ? pv[j * 8 + i] : suv[o + 1];
        }
    }
  stats[5] += n_frac;
  stats[6] += n_quarter;
  stats[8] += n_early;
  cnt[OC_EARLY] += n_early;
  cnt[OC_COST_MV] += n_costmv;
  cnt[OC_PHAT] += n_phat;
}

/* residual() of an inter macroblock (7.3.5.3) with nC from the left
 * macroblock (lnz / lnzc: its right-column total_coeff, -1 unavailable) and
 * the blocks above inside this one; cnz / cnzc receive this macroblock's */
static void put_residual(or_bw *b, const or_mb *m, const int *lnz, const int (*lnzc)[2], int *cnz,
                         int (*cnzc)[4]) {
  int cbp = m->cbp;
  for (int i = 0; i < 16; i++) cnz[i] = 0;
  for (int pl = 0; pl < 2; pl++)
    for (int i = 0; i < 4; i++) cnzc[pl][i] = 0;
  for (int k = 0; k < 16; k++) {
    if (!((cbp >> (k >> 2)) & 1)) continue;
    int bx = BLK_X[k], by = BLK_Y[k];
    int na = bx ? cnz[by * 4 + bx - 1] : lnz[by], nb = by ? cnz[(by - 1) * 4 + bx] : -1;
    int nC = (na >= 0 && nb >= 0) ? (na + nb + 1) >> 1 : (na >= 0 ? na : (nb >= 0 ? nb : 0));
    const int16_t *lv = m->lv + 16 * k;
    block_bits(b, lv, 16, nC);
    int tc = 0;
    for (int i = 0; i < 16; i++) tc += lv[i] != 0;
    cnz[by * 4 + bx] = tc;
  }
  if (cbp >> 4)
    for (int pl = 0; pl < 2; pl++) block_bits(b, m->lv + 256 + 4 * pl, 4, -1);
  if ((cbp >> 4) == 2)
    for (int pl = 0; pl < 2; pl++)
      for (int k = 0; k < 4; k++) {
        int bx = k & 1, by = k >> 1;
        int na = bx ? cnzc[pl][by * 2] : lnzc[pl][by], nb = by ? cnzc[pl][bx] : -1;
        int nC = (na >= 0 && nb >= 0) ? (na + nb + 1) >> 1 : (na >= 0 ? na : (nb >= 0 ? nb : 0));
        const int16_t *lv = m->lv + 264 + 60 * pl + 15 * k;
        block_bits(b, lv, 15, nC);
        int tc = 0;
        for (int i = 0; i < 15; i++) tc += lv[i] != 0;
        cnzc[pl][k] = tc;
      }
}

static void put_pcm(or_bw *b, const uint8_t *src, int cw, int ch, int mx, int my) {
  bw_align(b);
  for (int j = 0; j < 16; j++)
    for (int i = 0; i < 16; i++) bw_u(b, 8, src[(int64_t)(my * 16 + j) * cw + mx * 16 + i]);
  const uint8_t *uv = src + (int64_t)cw * ch;
  for (int pl = 0; pl < 2; pl++)
    for (int j = 0; j < 8; j++)
      for (int i = 0; i < 8; i++) bw_u(b, 8, uv[(int64_t)(my * 8 + j) * cw + 2 * (mx * 8 + i) + pl]);
}

/* -------------------------------------------------- Intra16x16 (intra = 1) */

static int nc_of(int na, int nb) {
  return (na >= 0 && nb >= 0) ? (na + nb + 1) >> 1 : (na >= 0 ? na : (nb >= 0 ? nb : 0));
}

/* macroblock_layer() of an Intra16x16 macroblock (7.3.5, Table 7-11) without
 * its mb_skip_run: mb_type (5 more in a P slice), intra_chroma_pred_mode,
 * mb_qp_delta 0, Intra16x16DCLevel (nC of block 0), the 16 Intra16x16ACLevel
 * blocks when the luma coded_block_pattern is 15, chroma DC / AC.  lnz / lnzc:
 * the left macroblock's right column of total_coeff (-1 unavailable); the row
 * above is another slice.  b == NULL only counts.  Returns the bits; cnz / cnzc
 * receive this macroblock's total_coeff (an AC block's counts its 15 levels). */
static int put_intra_mb(or_bw *b, const or_mb *m, int p_slice, const int *lnz, const int (*lnzc)[2], int *cnz,
                        int (*cnzc)[4]) {
  or_bw cnt = {NULL, 0, 0, 0, 0};
  if (!b) b = &cnt;
  int64_t before = b->n * 8 + b->nb;
  int cbp = m->cbp;
  uint32_t mbt = (uint32_t)(1 + m->lmode + 4 * (cbp >> 4) + ((cbp & 15) ? 12 : 0));
  bw_ue(b, p_slice ? 5 + mbt : mbt);
  bw_ue(b, (uint32_t)m->cmode);
  bw_se(b, 0);
  for (int i = 0; i < 16; i++) cnz[i] = 0;
  for (int pl = 0; pl < 2; pl++)
    for (int i = 0; i < 4; i++) cnzc[pl][i] = 0;
  block_bits(b, m->lv, 16, nc_of(lnz[0], -1));
  if (cbp & 15)
    for (int k = 0; k < 16; k++) {
      int bx = BLK_X[k], by = BLK_Y[k];
      int na = bx ? cnz[by * 4 + bx - 1] : lnz[by], nb = by ? cnz[(by - 1) * 4 + bx] : -1;
      const int16_t *lv = m->lv + 16 + 15 * k;
      block_bits(b, lv, 15, nc_of(na, nb));
      int tc = 0;
      for (int i = 0; i < 15; i++) tc += lv[i] != 0;
      cnz[by * 4 + bx] = tc;
    }
  if (cbp >> 4)
    for (int pl = 0; pl < 2; pl++) block_bits(b, m->lv + 256 + 4 * pl, 4, -1);
  if ((cbp >> 4) == 2)
    for (int pl = 0; pl < 2; pl++)
      for (int k = 0; k < 4; k++) {
        int bx = k & 1, by = k >> 1;
        int na = bx ? cnzc[pl][by * 2] : lnzc[pl][by], nb = by ? cnzc[pl][bx] : -1;
        const int16_t *lv = m->lv + 264 + 60 * pl + 15 * k;
        block_bits(b, lv, 15, nc_of(na, nb));
        int tc = 0;
        for (int i = 0; i < 15; i++) tc += lv[i] != 0;
        cnzc[pl][k] = tc;
      }
  return (int)(b->n * 8 + b->nb - before);
}

/* total_coeff of a coded macroblock's right column, as the macroblock to its
 * right reads it for nC (9.2.1): 16 after I_PCM, 0 after P_Skip or an uncoded
 * 8x8 / chroma AC, else the number of non-zero levels of luma4x4BlkIdx 5, 7,
 * 13, 15 and chroma4x4BlkIdx 1, 3 */
static void right_column_nz(const or_mb *m, int *lnz, int (*lnzc)[2]) {
  static const int RB[4] = {5, 7, 13, 15};
  for (int i = 0; i < 4; i++) {
    int k = RB[i], tc = 0;
    if (m->pcm) tc = 16;
    else if (m->i16) { if (m->cbp & 15) for (int q = 0; q < 15; q++) tc += m->lv[16 + 15 * k + q] != 0; }
    else if ((m->cbp >> (k >> 2)) & 1) for (int q = 0; q < 16; q++) tc += m->lv[16 * k + q] != 0;
    lnz[i] = tc;
  }
  for (int pl = 0; pl < 2; pl++)
    for (int r = 0; r < 2; r++) {
      int tc = 0;
      if (m->pcm) tc = 16;
      else if ((m->cbp >> 4) == 2) for (int q = 0; q < 15; q++) tc += m->lv[264 + 60 * pl + 15 * (1 + 2 * r) + q] != 0;
      lnzc[pl][r] = tc;
    }
}

/* 8.5.10: Intra16x16 luma DC levels c (4x4, raster by block row / column) ->
 * the scaled DC dcY of each block */
static void i16_dc_scale(const int *c, int qp, int *dcy) {
  int t[16], f[16];
  for (int i = 0; i < 4; i++) {  /* f = A c A, A = [1 1 1 1; 1 1 -1 -1; 1 -1 -1 1; 1 -1 1 -1] */
    int a0 = c[i * 4], a1 = c[i * 4 + 1], a2 = c[i * 4 + 2], a3 = c[i * 4 + 3];
    t[i * 4] = a0 + a1 + a2 + a3; t[i * 4 + 1] = a0 + a1 - a2 - a3;
    t[i * 4 + 2] = a0 - a1 - a2 + a3; t[i * 4 + 3] = a0 - a1 + a2 - a3;
  }
  for (int j = 0; j < 4; j++) {
    int a0 = t[j], a1 = t[4 + j], a2 = t[8 + j], a3 = t[12 + j];
    f[j] = a0 + a1 + a2 + a3; f[4 + j] = a0 + a1 - a2 - a3;
    f[8 + j] = a0 - a1 - a2 + a3; f[12 + j] = a0 - a1 + a2 - a3;
  }
  int ls = 16 * NV[qp % 6][0];
  for (int k = 0; k < 16; k++)
    dcy[k] = qp >= 36 ? (f[k] * ls) << (qp / 6 - 6) : (f[k] * ls + (1 << (5 - qp / 6))) >> (6 - qp / 6);
}

/* a candidate coding of one macroblock: its reconstruction and what is coded */
typedef struct {
  uint8_t y[256], c[2][64];
  or_mb m;
  int bits;  /* macroblock_layer() without mb_skip_run, exact */
} or_cand;

/* Macroblock (mx, my) as Intra16x16 (the Intra16x16 rules):
 * prediction from the left macroblock's right column of this picture's
 * unfiltered reconstruction rec (the row above is another slice).  Fills the
 * candidate: reconstruction, levels, modes, pattern and exact bits; rec is only
 * read.  lnz / lnzc as put_intra_mb's. */
static void intra16_candidate(const uint8_t *src, const uint8_t *rec, int cw, int ch, int mx, int my, int qp,
                              int p_slice, const int *lnz, const int (*lnzc)[2], or_cand *cd) {
  const uint8_t *suv = src + (int64_t)cw * ch;
  const uint8_t *ruv = rec + (int64_t)cw * ch;
  int py[16], pc[2][8];  /* both modes are constant along a row: the prediction of each row */
  int lmode = 2, cmode = 0;  /* no neighbour: DC (128) for luma and chroma */
  for (int j = 0; j < 16; j++) py[j] = 128;
  for (int pl = 0; pl < 2; pl++)
    for (int j = 0; j < 8; j++) pc[pl][j] = 128;
  if (mx > 0) {
    int ly[16], lc[2][8], sum = 0;
    for (int j = 0; j < 16; j++) {
      ly[j] = rec[(int64_t)(my * 16 + j) * cw + mx * 16 - 1];
      sum += ly[j];
    }
    int dcy = (sum + 8) >> 4;  /* 8.3.3.3, only the left samples available */
    int dcc[2][8];
    for (int pl = 0; pl < 2; pl++) {
      for (int j = 0; j < 8; j++) lc[pl][j] = ruv[(int64_t)(my * 8 + j) * cw + 2 * (mx * 8 - 1) + pl];
      for (int half = 0; half < 2; half++) {  /* 8.3.4.1-3 without the row above: each 4x4 block's own rows */
        int s4 = lc[pl][4 * half] + lc[pl][4 * half + 1] + lc[pl][4 * half + 2] + lc[pl][4 * half + 3];
        for (int j = 0; j < 4; j++) dcc[pl][4 * half + j] = (s4 + 2) >> 2;
      }
    }
    int64_t sad_h = 0, sad_dc = 0, csad_dc = 0, csad_h = 0;
    for (int j = 0; j < 16; j++)
      for (int i = 0; i < 16; i++) {
        int sv = src[(int64_t)(my * 16 + j) * cw + mx * 16 + i];
        sad_h += abs(sv - ly[j]);
        sad_dc += abs(sv - dcy);
      }
    for (int pl = 0; pl < 2; pl++)
      for (int j = 0; j < 8; j++)
        for (int i = 0; i < 8; i++) {
          int sv = suv[(int64_t)(my * 8 + j) * cw + 2 * (mx * 8 + i) + pl];
          csad_dc += abs(sv - dcc[pl][j]);
          csad_h += abs(sv - lc[pl][j]);
        }
    /* the least SAD; a tie goes to the lower mode number (luma: Horizontal 1
     * before DC 2; chroma: DC 0 before Horizontal 1) */
    lmode = sad_h <= sad_dc ? 1 : 2;
    cmode = csad_dc <= csad_h ? 0 : 1;
    for (int j = 0; j < 16; j++) py[j] = lmode == 1 ? ly[j] : dcy;
    for (int pl = 0; pl < 2; pl++)
      for (int j = 0; j < 8; j++) pc[pl][j] = cmode == 1 ? lc[pl][j] : dcc[pl][j];
  }
  or_mb t;
  memset(&t, 0, sizeof t);
  t.i16 = 1;
  t.lmode = lmode;
  t.cmode = cmode;
  int qbits = 15 + qp / 6;
  int64_t f = ((int64_t)1 << qbits) / 6;
  /* luma: AC levels of each block at (qbits, f); the 16 DC terms through the
   * 4x4 Hadamard, halved with (x + 1) >> 1 (arithmetic), then at (qbits + 1, 2f) */
  int zac[16][16], dcw[16], acnz = 0;
  for (int k = 0; k < 16; k++) {
    int bx = BLK_X[k] * 4, by = BLK_Y[k] * 4, x[16], w[16];
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) x[i * 4 + j] = src[(int64_t)(my * 16 + by + i) * cw + mx * 16 + bx + j] - py[by + i];
    fwd4(x, w);
    dcw[BLK_Y[k] * 4 + BLK_X[k]] = w[0];
    zac[k][0] = 0;
    for (int q = 1; q < 16; q++) {
      zac[k][q] = quant1(w[q], MF[qp % 6][pos_class(q >> 2, q & 3)], qbits, f);
      acnz |= zac[k][q] != 0;
    }
    for (int s = 1; s < 16; s++) t.lv[16 + 15 * k + s - 1] = (int16_t)zac[k][ZZ[s]];
  }
  int hd[16], tt[16], dcl[16], dcy_s[16];
  for (int i = 0; i < 4; i++) {
    int a0 = dcw[i * 4], a1 = dcw[i * 4 + 1], a2 = dcw[i * 4 + 2], a3 = dcw[i * 4 + 3];
    tt[i * 4] = a0 + a1 + a2 + a3; tt[i * 4 + 1] = a0 + a1 - a2 - a3;
    tt[i * 4 + 2] = a0 - a1 - a2 + a3; tt[i * 4 + 3] = a0 - a1 + a2 - a3;
  }
  for (int j = 0; j < 4; j++) {
    int a0 = tt[j], a1 = tt[4 + j], a2 = tt[8 + j], a3 = tt[12 + j];
    hd[j] = a0 + a1 + a2 + a3; hd[4 + j] = a0 + a1 - a2 - a3;
    hd[8 + j] = a0 - a1 - a2 + a3; hd[12 + j] = a0 - a1 + a2 - a3;
  }
  for (int k = 0; k < 16; k++) {
    int half = hd[k] >= 0 ? (hd[k] + 1) / 2 : -((-hd[k]) / 2);  /* floor((x + 1) / 2) */
    dcl[k] = quant1(half, MF[qp % 6][0], qbits + 1, 2 * f);
  }
  for (int s = 0; s < 16; s++) t.lv[s] = (int16_t)dcl[ZZ[s]];
  i16_dc_scale(dcl, qp, dcy_s);
  /* chroma: as an inter macroblock's (residual_mb) against the intra prediction */
  int qpc = QPC[qp], cqb = 15 + qpc / 6;
  int64_t cf = ((int64_t)1 << cqb) / 6;
  int cacnz = 0, cdcnz = 0, cz[2][4][16], cdl[2][4];
  for (int pl = 0; pl < 2; pl++) {
    int wdc[4];
    for (int k = 0; k < 4; k++) {
      int bx = (k & 1) * 4, by = (k >> 1) * 4, x[16], w[16];
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
          x[i * 4 + j] = suv[(int64_t)(my * 8 + by + i) * cw + 2 * (mx * 8 + bx + j) + pl] - pc[pl][by + i];
      fwd4(x, w);
      wdc[k] = w[0];
      cz[pl][k][0] = 0;
      for (int q = 1; q < 16; q++) {
        cz[pl][k][q] = quant1(w[q], MF[qpc % 6][pos_class(q >> 2, q & 3)], cqb, cf);
        cacnz |= cz[pl][k][q] != 0;
      }
      for (int s = 1; s < 16; s++) t.lv[264 + pl * 60 + k * 15 + s - 1] = (int16_t)cz[pl][k][ZZ[s]];
    }
    int fd[4] = {wdc[0] + wdc[1] + wdc[2] + wdc[3], wdc[0] - wdc[1] + wdc[2] - wdc[3],
                 wdc[0] + wdc[1] - wdc[2] - wdc[3], wdc[0] - wdc[1] - wdc[2] + wdc[3]};
    for (int k = 0; k < 4; k++) {
      cdl[pl][k] = quant1(fd[k], MF[qpc % 6][0], cqb + 1, 2 * cf);
      cdcnz |= cdl[pl][k] != 0;
      t.lv[256 + 4 * pl + k] = (int16_t)cdl[pl][k];
    }
  }
  /* coded_block_pattern: luma 15 when any AC level of any block is non-zero,
   * else 0; chroma 2 with a non-zero AC level, else 1 with a non-zero DC level */
  int cc = cacnz ? 2 : (cdcnz ? 1 : 0);
  t.cbp = (acnz ? 15 : 0) | (cc << 4);
  int cnz[16], cnzc[2][4];
  cd->bits = put_intra_mb(NULL, &t, p_slice, lnz, lnzc, cnz, cnzc);
  /* reconstruction: the decoder's (8.5.10 DC, 8.5.12; uncoded AC reads as zero) */
  for (int k = 0; k < 16; k++) {
    int bx = BLK_X[k] * 4, by = BLK_Y[k] * 4, co[16], r[16];
    for (int q = 0; q < 16; q++) co[q] = acnz ? zac[k][q] : 0;
    co[0] = dcy_s[BLK_Y[k] * 4 + BLK_X[k]];
    idct4(co, qp, 1, r);
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++)
        cd->y[(by + i) * 16 + bx + j] = (uint8_t)clip255(py[by + i] + r[i * 4 + j]);
  }
  for (int pl = 0; pl < 2; pl++) {
    const int *c = cdl[pl];
    int F[4] = {c[0] + c[1] + c[2] + c[3], c[0] - c[1] + c[2] - c[3], c[0] + c[1] - c[2] - c[3],
                c[0] - c[1] - c[2] + c[3]};
    for (int k = 0; k < 4; k++) {
      int co[16], r[16], bx = (k & 1) * 4, by = (k >> 1) * 4;
      for (int q = 0; q < 16; q++) co[q] = cc == 2 ? cz[pl][k][q] : 0;
      co[0] = ((F[k] * 16 * NV[qpc % 6][0]) << (qpc / 6)) >> 5;
      idct4(co, qpc, 1, r);
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
          cd->c[pl][(by + i) * 8 + bx + j] = (uint8_t)clip255(pc[pl][by + i] + r[i * 4 + j]);
    }
  }
  cd->m = t;
}

/* ---------------------------------------------------- Intra4x4 (intra4x4 = 1) */

/* Table 9-4 (chroma_format_idc 1), Intra_4x4 column: codeNum -> coded_block_pattern */
static const int CBP_I[48] = {47, 31, 15, 0,  23, 27, 29, 30, 7,  11, 13, 14, 39, 43, 45, 46,
                              16, 3,  5,  10, 12, 19, 21, 26, 28, 35, 37, 42, 44, 1,  2,  4,
                              8,  17, 18, 20, 24, 6,  9,  22, 25, 32, 33, 34, 36, 40, 38, 41};

/* luma4x4BlkIdx of the block at raster column bx, row by (6.4.3 inverted) */
static int blk_at(int bx, int by) {
  int k = 0;
  while (BLK_X[k] != bx || BLK_Y[k] != by) k++;
  return k;
}

/* the neighbouring samples p[x, -1], x = -1 .. 7, and p[-1, y], y = 0 .. 3 of a 4x4 block (8.3.1.2) */
typedef struct {
  int top[9];  /* top[x + 1] = p[x, -1] */
  int left[4]; /* left[y] = p[-1, y] */
  int has_left, has_top;
} or_nb4;
static int nbp(const or_nb4 *n, int x, int y) { return y < 0 ? n->top[x + 1] : n->left[y]; }

/* pred4x4L[x, y] of Intra4x4PredMode mode, 8.3.1.2.1 .. 8.3.1.2.9, one sample */
static int pred4_sample(const or_nb4 *n, int mode, int x, int y) {
  switch (mode) {
    case 0: return nbp(n, x, -1);                                                       /* Vertical */
    case 1: return nbp(n, -1, y);                                                       /* Horizontal */
    case 2: {                                                                           /* DC */
      int st = 0, sl = 0;
      for (int i = 0; i < 4; i++) { st += nbp(n, i, -1); sl += nbp(n, -1, i); }
      if (n->has_top && n->has_left) return (st + sl + 4) >> 3;
      if (n->has_left) return (sl + 2) >> 2;
      if (n->has_top) return (st + 2) >> 2;
      return 128;
    }
    case 3:                                                                             /* Diagonal_Down_Left */
      if (x == 3 && y == 3) return (nbp(n, 6, -1) + 3 * nbp(n, 7, -1) + 2) >> 2;
      return (nbp(n, x + y, -1) + 2 * nbp(n, x + y + 1, -1) + nbp(n, x + y + 2, -1) + 2) >> 2;
    case 4:                                                                             /* Diagonal_Down_Right */
      if (x > y) return (nbp(n, x - y - 2, -1) + 2 * nbp(n, x - y - 1, -1) + nbp(n, x - y, -1) + 2) >> 2;
      if (x < y) return (nbp(n, -1, y - x - 2) + 2 * nbp(n, -1, y - x - 1) + nbp(n, -1, y - x) + 2) >> 2;
      return (nbp(n, 0, -1) + 2 * nbp(n, -1, -1) + nbp(n, -1, 0) + 2) >> 2;
    case 5: {                                                                           /* Vertical_Right */
      int z = 2 * x - y, h = y >> 1;
      if (z >= 0 && !(z & 1)) return (nbp(n, x - h - 1, -1) + nbp(n, x - h, -1) + 1) >> 1;
      if (z >= 0) return (nbp(n, x - h - 2, -1) + 2 * nbp(n, x - h - 1, -1) + nbp(n, x - h, -1) + 2) >> 2;
      if (z == -1) return (nbp(n, -1, 0) + 2 * nbp(n, -1, -1) + nbp(n, 0, -1) + 2) >> 2;
      return (nbp(n, -1, y - 1) + 2 * nbp(n, -1, y - 2) + nbp(n, -1, y - 3) + 2) >> 2;
    }
    case 6: {                                                                           /* Horizontal_Down */
      int z = 2 * y - x, h = x >> 1;
      if (z >= 0 && !(z & 1)) return (nbp(n, -1, y - h - 1) + nbp(n, -1, y - h) + 1) >> 1;
      if (z >= 0) return (nbp(n, -1, y - h - 2) + 2 * nbp(n, -1, y - h - 1) + nbp(n, -1, y - h) + 2) >> 2;
      if (z == -1) return (nbp(n, -1, 0) + 2 * nbp(n, -1, -1) + nbp(n, 0, -1) + 2) >> 2;
      return (nbp(n, x - 1, -1) + 2 * nbp(n, x - 2, -1) + nbp(n, x - 3, -1) + 2) >> 2;
    }
    case 7: {                                                                           /* Vertical_Left */
      int h = y >> 1;
      if (!(y & 1)) return (nbp(n, x + h, -1) + nbp(n, x + h + 1, -1) + 1) >> 1;
      return (nbp(n, x + h, -1) + 2 * nbp(n, x + h + 1, -1) + nbp(n, x + h + 2, -1) + 2) >> 2;
    }
    default: {                                                                          /* Horizontal_Up */
      int z = x + 2 * y, h = x >> 1;
      if (z > 5) return nbp(n, -1, 3);
      if (z == 5) return (nbp(n, -1, 2) + 3 * nbp(n, -1, 3) + 2) >> 2;
      if (!(z & 1)) return (nbp(n, -1, y + h) + nbp(n, -1, y + h + 1) + 1) >> 1;
      return (nbp(n, -1, y + h) + 2 * nbp(n, -1, y + h + 1) + nbp(n, -1, y + h + 2) + 2) >> 2;
    }
  }
}

/* predIntra4x4PredMode of block k (8.3.1.1) with one slice per macroblock row:
 * the macroblock above is never available and the one to the left only for mx >
 * 0, so dcPredModePredictedFlag holds for the top row and for column 0 at mx = 0
 * (2); a left macroblock that is not I_NxN counts as 2 (no constrained intra
 * prediction); else Min(A, B).  cur: the modes of this macroblock so far */
static int pred_mode4(int k, uint64_t cur, int mx, const or_mb *left) {
  int bx = BLK_X[k], by = BLK_Y[k];
  if (by == 0 || (bx == 0 && mx == 0)) return 2;
  int a = bx ? (int)((cur >> (4 * blk_at(bx - 1, by))) & 15)
             : (left->i4 ? (int)((left->modes >> (4 * blk_at(3, by))) & 15) : 2);
  int b = (int)((cur >> (4 * blk_at(bx, by - 1))) & 15);
  return a < b ? a : b;
}

/* macroblock_layer() of an I_NxN macroblock (7.3.5, 7.3.5.1) without its
 * mb_skip_run: mb_type 0 (5 in a P slice), the sixteen prev_intra4x4_pred_mode_flag
 * / rem_intra4x4_pred_mode, intra_chroma_pred_mode, coded_block_pattern me(v)
 * by the Intra_4x4 column, mb_qp_delta 0 with a pattern, residual() in the shape
 * of an inter macroblock's.  left: the macroblock to the left (NULL at mx = 0).
 * b == NULL only counts.  Returns the bits; cnz / cnzc as put_intra_mb's. */
static int put_i4_mb(or_bw *b, const or_mb *m, int p_slice, int mx, const or_mb *left, const int *lnz,
                     const int (*lnzc)[2], int *cnz, int (*cnzc)[4]) {
  or_bw cnt = {NULL, 0, 0, 0, 0};
  if (!b) b = &cnt;
  int64_t before = b->n * 8 + b->nb;
  bw_ue(b, p_slice ? 5 : 0);
  uint64_t cur = 0;
  for (int k = 0; k < 16; k++) {
    int mode = (int)((m->modes >> (4 * k)) & 15), pm = pred_mode4(k, cur, mx, left);
    if (mode == pm) {
      bw_bit(b, 1);  /* prev_intra4x4_pred_mode_flag */
    } else {
      bw_bit(b, 0);
      bw_u(b, 3, (uint32_t)(mode < pm ? mode : mode - 1));  /* rem_intra4x4_pred_mode */
    }
    cur |= (uint64_t)mode << (4 * k);
  }
  bw_ue(b, (uint32_t)m->cmode);
  int code = 0;
  while (CBP_I[code] != m->cbp) code++;
  bw_ue(b, (uint32_t)code);
  if (m->cbp) {
    bw_se(b, 0);
    put_residual(b, m, lnz, lnzc, cnz, cnzc);
  } else {
    for (int i = 0; i < 16; i++) cnz[i] = 0;
    for (int pl = 0; pl < 2; pl++)
      for (int i = 0; i < 4; i++) cnzc[pl][i] = 0;
  }
  return (int)(b->n * 8 + b->nb - before);
}

/* Macroblock (mx, my) as I_NxN ("Intra4x4", the rules).  The
 * blocks in luma4x4BlkIdx order, each predicted from the reconstruction of the
 * blocks before it and of the left macroblock's right column in rec; chroma
 * (mode, levels, reconstruction, pattern class) is the Intra16x16 candidate's.
 * Fills the candidate as intra16_candidate does. */
static void intra4_candidate(const uint8_t *src, const uint8_t *rec, int cw, int mx, int my, int qp, int p_slice,
                             int lambda16, const or_mb *left, const int *lnz, const int (*lnzc)[2],
                             const or_cand *c16, or_cand *cd, int64_t *cnt) {
  int qbits = 15 + qp / 6;
  int64_t f = ((int64_t)1 << qbits) / 6;
  or_mb t;
  memset(&t, 0, sizeof t);
  t.i4 = 1;
  t.cmode = c16->m.cmode;
  memcpy(t.lv + 256, c16->m.lv + 256, 128 * sizeof(int16_t));
  memcpy(cd->c, c16->c, sizeof cd->c);
  int cbp = c16->m.cbp & 0x30;
  for (int k = 0; k < 16; k++) {
    int bx = BLK_X[k], by = BLK_Y[k];
    /* availability (6.4.x; the row above the macroblock is another slice) */
    or_nb4 n;
    memset(&n, 0, sizeof n);
    n.has_left = bx > 0 || mx > 0;
    n.has_top = by > 0;
    int has_tl = n.has_left && n.has_top;
    int has_tr = n.has_top && bx < 3 && blk_at(bx + 1, by - 1) < k;  /* inside the macroblock and earlier */
    for (int y = 0; y < 4 && n.has_left; y++)
      n.left[y] = bx ? cd->y[(by * 4 + y) * 16 + bx * 4 - 1] : rec[(int64_t)(my * 16 + by * 4 + y) * cw + mx * 16 - 1];
    if (has_tl) n.top[0] = bx ? cd->y[(by * 4 - 1) * 16 + bx * 4 - 1] : rec[(int64_t)(my * 16 + by * 4 - 1) * cw + mx * 16 - 1];
    for (int x = 0; x < 8 && n.has_top; x++)  /* p[4 .. 7, -1] not available: p[3, -1] in their place */
      n.top[x + 1] = cd->y[(by * 4 - 1) * 16 + bx * 4 + ((x < 4 || has_tr) ? x : 3)];
    int pm = pred_mode4(k, t.modes, mx, left);
    int64_t best = -1, least_sad = -1;
    int bmode = 2, lmode = 2, nbest = 0, s4[16];
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) s4[i * 4 + j] = src[(int64_t)(my * 16 + by * 4 + i) * cw + mx * 16 + bx * 4 + j];
    for (int mode = 0; mode < 9; mode++) {
      int ok = mode == 2 ? 1
               : (mode == 0 || mode == 3 || mode == 7) ? n.has_top
               : (mode == 1 || mode == 8) ? n.has_left
                                          : has_tl;
      if (!ok) continue;
      int64_t sad = 0;
      for (int y = 0; y < 4; y++)
        for (int x = 0; x < 4; x++) sad += abs(s4[y * 4 + x] - pred4_sample(&n, mode, x, y));
      int64_t cost = 16 * sad + (int64_t)lambda16 * (mode == pm ? 1 : 4);
      if (least_sad < 0 || sad < least_sad) { least_sad = sad; lmode = mode; }
      if (best < 0 || cost < best) { best = cost; bmode = mode; nbest = 1; }
      else if (cost == best) nbest++;
    }
    cnt[OC_MODE0 + bmode]++;
    if (bmode != lmode) cnt[OC_DISCOUNT]++;
    if (nbest > 1) cnt[OC_COST_TIE]++;
    t.modes |= (uint64_t)bmode << (4 * k);
    /* residual, levels (the inter layout) and reconstruction before the next block predicts */
    int x[16], w[16], z[16], r[16], nz = 0;
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) x[i * 4 + j] = s4[i * 4 + j] - pred4_sample(&n, bmode, j, i);
    fwd4(x, w);
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) {
        z[i * 4 + j] = quant1(w[i * 4 + j], MF[qp % 6][pos_class(i, j)], qbits, f);
        nz |= z[i * 4 + j] != 0;
      }
    for (int s = 0; s < 16; s++) t.lv[16 * k + s] = (int16_t)z[ZZ[s]];
    idct4(z, qp, 0, r);
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++)
        cd->y[(by * 4 + i) * 16 + bx * 4 + j] = (uint8_t)clip255(pred4_sample(&n, bmode, j, i) + r[i * 4 + j]);
    if (nz) cbp |= 1 << (k >> 2);
  }
  /* an 8x8 whose bit is clear has no non-zero level: its reconstruction is
   * already the prediction, which is what the decoder makes of it */
  t.cbp = cbp;
  int cnz[16], cnzc[2][4];
  cd->bits = put_i4_mb(NULL, &t, p_slice, mx, left, lnz, lnzc, cnz, cnzc);
  cd->m = t;
}

/* The intra pass over one picture: all = 1 (an IDR picture) tries every
 * macroblock, all = 0 (a P picture) those the search left as I_PCM.  A row is
 * a chain: a macroblock predicts from, and takes its nC from, the macroblock
 * to its left as it is finally coded.  i4: also try I_NxN, which the macroblock
 * becomes when its bits are fewer than the Intra16x16 candidate's; the winner
 * is coded when its bits are <= 3072, else the macroblock stays I_PCM (rec
 * holds the source).  cbits (may be NULL): [my][mx][2], the bits of the
 * Intra16x16 and the I_NxN candidate of every macroblock tried. */
static void encode_intra(const uint8_t *src, uint8_t *rec, int cw, int ch, int qp, int all, int i4, int lambda16,
                         or_mb *mbs, int32_t *cbits, int64_t *cnt) {
  int mbw = cw / 16, mbh = ch / 16;
  for (int my = 0; my < mbh; my++) {
    int lnz[4] = {-1, -1, -1, -1}, lnzc[2][2] = {{-1, -1}, {-1, -1}};
    for (int mx = 0; mx < mbw; mx++) {
      or_mb *m = &mbs[my * mbw + mx];
      if (all) {  /* nothing is coded yet: I_PCM, the source */
        memset(m, 0, sizeof *m);
        m->pcm = 1;
        for (int j = 0; j < 16; j++)
          memcpy(rec + (int64_t)(my * 16 + j) * cw + mx * 16, src + (int64_t)(my * 16 + j) * cw + mx * 16, 16);
        for (int j = 0; j < 8; j++)
          memcpy(rec + (int64_t)cw * ch + (int64_t)(my * 8 + j) * cw + mx * 16,
                 src + (int64_t)cw * ch + (int64_t)(my * 8 + j) * cw + mx * 16, 16);
      }
      if (m->pcm) {
        or_cand c16, c4;
        const or_cand *win = &c16;
        intra16_candidate(src, rec, cw, ch, mx, my, qp, !all, lnz, (const int(*)[2])lnzc, &c16);
        if (i4) {
          intra4_candidate(src, rec, cw, mx, my, qp, !all, lambda16, mx ? m - 1 : NULL, lnz, (const int(*)[2])lnzc,
                           &c16, &c4, cnt);
          if (c4.bits < c16.bits) win = &c4;  /* a tie stays Intra16x16 */
          cnt[win == &c4 ? OC_I4_WON : OC_I16_WON]++;
          if (c4.bits == c16.bits) cnt[OC_EQUAL_BITS]++;
          if (win == &c4 && c4.bits > 3072) cnt[OC_I4_PCM]++;
          if (cbits) {
            cbits[2 * (my * mbw + mx)] = c16.bits;
            cbits[2 * (my * mbw + mx) + 1] = c4.bits;
          }
        }
        if (win->bits <= 3072) {
          *m = win->m;
          for (int j = 0; j < 16; j++) memcpy(rec + (int64_t)(my * 16 + j) * cw + mx * 16, win->y + j * 16, 16);
          for (int j = 0; j < 8; j++)
            for (int i = 0; i < 8; i++)
              for (int pl = 0; pl < 2; pl++)
                rec[(int64_t)cw * ch + (int64_t)(my * 8 + j) * cw + 2 * (mx * 8 + i) + pl] = win->c[pl][j * 8 + i];
        }
      }
      right_column_nz(m, lnz, lnzc);
    }
  }
}

/* ------------------------------------------- deblocking filter (deblock = 1) */

/* 8.7.2.3 / 8.7.2.4: one line of samples s[k step], k = -4 .. 3 (p3 .. p0, q0
 * .. q3) across an edge; returns filterSamplesFlag */
static int deblock_line(uint8_t *s, int64_t step, int bS, int chroma, int indexA, int alpha, int beta) {
  int p0 = s[-step], p1 = s[-2 * step], q0 = s[0], q1 = s[step];
  if (bS == 0 || !(abs(p0 - q0) < alpha && abs(p1 - p0) < beta && abs(q1 - q0) < beta)) return 0;
  int p2 = chroma ? 0 : s[-3 * step], q2 = chroma ? 0 : s[2 * step];
  int ap = abs(p2 - p0), aq = abs(q2 - q0);
  if (bS < 4) {
    int tc0 = FO_TC0[indexA][bS - 1];
    int tc = chroma ? tc0 + 1 : tc0 + (ap < beta) + (aq < beta);
    int delta = clampi((((q0 - p0) << 2) + (p1 - q1) + 4) >> 3, -tc, tc);
    s[-step] = (uint8_t)clip255(p0 + delta);
    s[0] = (uint8_t)clip255(q0 - delta);
    if (!chroma && ap < beta) s[-2 * step] = (uint8_t)(p1 + clampi((p2 + ((p0 + q0 + 1) >> 1) - (p1 << 1)) >> 1, -tc0, tc0));
    if (!chroma && aq < beta) s[step] = (uint8_t)(q1 + clampi((q2 + ((p0 + q0 + 1) >> 1) - (q1 << 1)) >> 1, -tc0, tc0));
  } else {
    int strong = abs(p0 - q0) < ((alpha >> 2) + 2);
    if (!chroma && ap < beta && strong) {
      int p3 = s[-4 * step];
      s[-step] = (uint8_t)((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3);
      s[-2 * step] = (uint8_t)((p2 + p1 + p0 + q0 + 2) >> 2);
      s[-3 * step] = (uint8_t)((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3);
    } else {
      s[-step] = (uint8_t)((2 * p1 + p0 + q1 + 2) >> 2);
    }
    if (!chroma && aq < beta && strong) {
      int q3 = s[3 * step];
      s[0] = (uint8_t)((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3);
      s[step] = (uint8_t)((p0 + q0 + q1 + q2 + 2) >> 2);
      s[2 * step] = (uint8_t)((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3);
    } else {
      s[0] = (uint8_t)((2 * q1 + q0 + p1 + 2) >> 2);
    }
  }
  return 1;
}

/* the raster 4x4 luma block (bx, by) of an inter macroblock has a non-zero
 * level that the slice writer codes */
static int blk_coded(const or_mb *m, int bx, int by) {
  int k = 0;
  while (BLK_X[k] != bx || BLK_Y[k] != by) k++;
  if (!((m->cbp >> (k >> 2)) & 1)) return 0;
  for (int q = 0; q < 16; q++)
    if (m->lv[16 * k + q]) return 1;
  return 0;
}

/* bS (8.7.2.1) of a line between block (pbx, pby) of macroblock p and block
 * (qbx, qby) of macroblock q; one reference picture, frame macroblocks */
static int edge_bs(const or_mb *p, int pbx, int pby, const or_mb *q, int qbx, int qby, int mb_edge) {
  if (p->pcm || p->i16 || p->i4 || q->pcm || q->i16 || q->i4) return mb_edge ? 4 : 3;
  if (blk_coded(p, pbx, pby) || blk_coded(q, qbx, qby)) return 2;
  return (abs(p->mvx - q->mvx) >= 4 || abs(p->mvy - q->mvy) >= 4) ? 1 : 0;
}

/* Clause 8.7 over one picture with disable_deblocking_filter_idc = 2 and one
 * slice per macroblock row, in place on rec: per macroblock in raster order
 * the left macroblock edge (when it has a left neighbour) and the three inner
 * vertical luma edges, then the three inner horizontal ones (the top edge is
 * a slice boundary), chroma edges 0 and 2 of each direction likewise.  offa /
 * offb = FilterOffsetA / B.  Returns the macroblocks with a filtered line. */
static int64_t deblock_picture(uint8_t *rec, int cw, int ch, const or_mb *mbs, int qp, int offa, int offb) {
  int mbw = cw / 16, mbh = ch / 16;
  int64_t count = 0;
  for (int my = 0; my < mbh; my++)
    for (int mx = 0; mx < mbw; mx++) {
      const or_mb *q = &mbs[my * mbw + mx];
      int any = 0;
      for (int chroma = 0; chroma < 2; chroma++)
        for (int pl = 0; pl < (chroma ? 2 : 1); pl++)
          for (int dir = 0; dir < 2; dir++)
            for (int e = 0; e < 4; e += chroma ? 2 : 1) {
              if (e == 0 && (dir == 1 || mx == 0)) continue;
              const or_mb *p = e == 0 ? &mbs[my * mbw + mx - 1] : q;
              int qpp = p->pcm ? 0 : qp, qpq = q->pcm ? 0 : qp;  /* qPp, qPq: 0 for I_PCM (8.7.2.2) */
              int qpav = chroma ? (QPC[qpp] + QPC[qpq] + 1) >> 1 : (qpp + qpq + 1) >> 1;
              int indexA = clampi(qpav + offa, 0, 51), indexB = clampi(qpav + offb, 0, 51);
              int alpha = FO_ALPHA[indexA], beta = FO_BETA[indexB];
              for (int k = 0; k < (chroma ? 8 : 16); k++) {
                int lk = chroma ? 2 * k : k;  /* the luma line whose bS the chroma line takes */
                int bS = dir == 0 ? edge_bs(p, (e + 3) & 3, lk >> 2, q, e, lk >> 2, e == 0)
                                  : edge_bs(p, lk >> 2, (e + 3) & 3, q, lk >> 2, e, 0);
                uint8_t *s;
                int64_t step;
                if (!chroma) {
                  s = dir == 0 ? rec + (int64_t)(my * 16 + k) * cw + mx * 16 + 4 * e
                               : rec + (int64_t)(my * 16 + 4 * e) * cw + mx * 16 + k;
                  step = dir == 0 ? 1 : cw;
                } else {
                  uint8_t *uv = rec + (int64_t)cw * ch;
                  s = dir == 0 ? uv + (int64_t)(my * 8 + k) * cw + 2 * (mx * 8 + 2 * e) + pl
                               : uv + (int64_t)(my * 8 + 2 * e) * cw + 2 * (mx * 8 + k) + pl;
                  step = dir == 0 ? 2 : cw;
                }
                any |= deblock_line(s, step, bS, chroma, indexA, alpha, beta);
              }
            }
      count += any;
    }
  return count;
}

/* one picture, one slice per macroblock row, appended to out */
static int write_picture(const uint8_t *src, int cw, int ch, const or_mb *mbs, int idr, int idr_id,
                         int frame_num, int qp, int intra, int deblock, int dalpha, int dbeta, uint8_t *out,
                         int64_t cap, int64_t *pos, uint8_t *rbsp, int64_t rcap, int64_t *stats) {
  int mbw = cw / 16, mbh = ch / 16;
  for (int row = 0; row < mbh; row++) {
    or_bw b = {rbsp, 0, rcap, 0, 0};
    bw_ue(&b, (uint32_t)(row * mbw));  /* first_mb_in_slice */
    bw_ue(&b, idr ? 7 : 5);            /* slice_type I / P (all slices) */
    bw_ue(&b, 0);                      /* pic_parameter_set_id */
    bw_u(&b, 16, (uint32_t)frame_num);
    if (idr) {
      bw_ue(&b, (uint32_t)idr_id);
    } else {
      bw_u(&b, 1, 0);                  /* num_ref_idx_active_override_flag */
      bw_u(&b, 1, 0);                  /* ref_pic_list_modification_flag_l0 */
    }
    if (idr) {
      bw_u(&b, 1, 0);                  /* no_output_of_prior_pics_flag */
      bw_u(&b, 1, 0);                  /* long_term_reference_flag */
    } else {
      bw_u(&b, 1, 0);                  /* adaptive_ref_pic_marking_mode_flag */
    }
    bw_se(&b, qp >= 1 ? qp - 26 : 0);  /* slice_qp_delta: SliceQPY = the residual's QP (pic_init_qp 26) */
    if (deblock) {
      bw_ue(&b, 2);                    /* disable_deblocking_filter_idc: not across slice boundaries */
      bw_se(&b, dalpha);               /* slice_alpha_c0_offset_div2 */
      bw_se(&b, dbeta);                /* slice_beta_offset_div2 */
    } else {
      bw_ue(&b, 1);                    /* disable_deblocking_filter_idc */
    }
    uint32_t skip = 0;
    int amv_ok = 0, amvx = 0, amvy = 0;  /* left neighbour A: inter with this mv */
    /* total_coeff of the left macroblock's right column (nC, 9.2.1): -1 none */
    int lnz[4] = {-1, -1, -1, -1}, lnzc[2][2] = {{-1, -1}, {-1, -1}}, cnz[16], cnzc[2][4];
    for (int mx = 0; mx < mbw; mx++) {
      const or_mb *m = &mbs[row * mbw + mx];
      if (idr && !intra) {
        bw_ue(&b, 25);
        put_pcm(&b, src, cw, ch, mx, row);
        stats[0]++;
        continue;
      }
      if (m->i16 || m->i4) {  /* Intra16x16 or I_NxN in an I or a P slice */
        if (!idr) {
          bw_ue(&b, skip);
          skip = 0;
        }
        if (m->i4) {
          put_i4_mb(&b, m, !idr, mx, mx ? m - 1 : NULL, lnz, (const int(*)[2])lnzc, cnz, cnzc);
          stats[9]++;
        } else {
          put_intra_mb(&b, m, !idr, lnz, (const int(*)[2])lnzc, cnz, cnzc);
        }
        for (int i = 0; i < 4; i++) lnz[i] = cnz[i * 4 + 3];
        for (int pl = 0; pl < 2; pl++) {
          lnzc[pl][0] = cnzc[pl][1];
          lnzc[pl][1] = cnzc[pl][3];
        }
        amv_ok = 0;  /* an intra neighbour predicts no motion (8.4.1.3.2) */
        stats[4]++;
        continue;
      }
      if (idr) {  /* I_PCM in an I slice of the intra encoder */
        bw_ue(&b, 25);
        put_pcm(&b, src, cw, ch, mx, row);
        stats[0]++;
        for (int i = 0; i < 4; i++) lnz[i] = 16;
        for (int pl = 0; pl < 2; pl++) lnzc[pl][0] = lnzc[pl][1] = 16;
        continue;
      }
      if (m->pcm) {
        bw_ue(&b, skip);
        skip = 0;
        bw_ue(&b, 30);
        put_pcm(&b, src, cw, ch, mx, row);
        amv_ok = 0;
        stats[0]++;
        for (int i = 0; i < 4; i++) lnz[i] = 16;
        for (int pl = 0; pl < 2; pl++) lnzc[pl][0] = lnzc[pl][1] = 16;
        continue;
      }
      if (m->mvx == 0 && m->mvy == 0 && m->cbp == 0) {  /* P_Skip: B unavailable -> mv 0 */
        skip++;
        stats[2]++;
        for (int i = 0; i < 4; i++) lnz[i] = 0;
        for (int pl = 0; pl < 2; pl++) lnzc[pl][0] = lnzc[pl][1] = 0;
      } else {
        int px = amv_ok ? amvx : 0, py = amv_ok ? amvy : 0;  /* 8.4.1.3, only A available */
        bw_ue(&b, skip);
        skip = 0;
        bw_ue(&b, 0);                  /* P_L0_16x16 */
        bw_se(&b, m->mvx - px);
        bw_se(&b, m->mvy - py);
        int code = 0;
        while (CBP_P[code] != m->cbp) code++;
        bw_ue(&b, (uint32_t)code);     /* coded_block_pattern me(v) */
        if (m->cbp) {
          bw_se(&b, 0);                /* mb_qp_delta */
          put_residual(&b, m, lnz, (const int(*)[2])lnzc, cnz, cnzc);
        } else {
          for (int i = 0; i < 16; i++) cnz[i] = 0;
          for (int pl = 0; pl < 2; pl++)
            for (int i = 0; i < 4; i++) cnzc[pl][i] = 0;
        }
        for (int i = 0; i < 4; i++) lnz[i] = cnz[i * 4 + 3];
        for (int pl = 0; pl < 2; pl++) {
          lnzc[pl][0] = cnzc[pl][1];
          lnzc[pl][1] = cnzc[pl][3];
        }
        stats[1]++;
      }
      amv_ok = 1;
      amvx = m->mvx;
      amvy = m->mvy;
    }
    if (skip) bw_ue(&b, skip);
    bw_trailing(&b);
    if (b.n > rcap) return -2;
    if (put_nal(out, cap, pos, idr ? 0x65 : 0x41, rbsp, b.n)) return -2;
  }
  return 0;
}

/* The whole transcode.  frames: n display-size NV12 frames (W x H, pitch W);
 * scores: the scene scores.  out: the concatenated MP4
 * samples (AVCC, 4-byte lengths); sample_off/sample_size/sync per frame;
 * recon (may be NULL): n coded NV12 reconstructions (cw x ch x 1.5 each);
 * stats: [pcm MBs, P_L0_16x16 MBs, P_Skip MBs, IDR pictures].
 * Returns 0, -1 bad argument, -2 capacity, -3 out of memory. */
/* or_transcode_ex: the same with the three opt-in paths of DESIGN.md §11.
 * intra (0 / 1): Intra16x16 coding of the IDR pictures and of the P
 * macroblocks the search leaves as I_PCM; subpel (0, 1, 2): half- / quarter-
 * sample refinement of the motion; deblock (0 / 1) with dalpha / dbeta
 * (slice_alpha_c0_offset_div2 / slice_beta_offset_div2, -6 .. 6): the in-loop
 * filter inside each macroblock row's slice.  stats has 8 entries: the four
 * above, then [Intra16x16 MBs, inter MBs with a fractional vector, of those
 * with a quarter-sample component, MBs with a filtered line]; recon is the
 * filtered reconstruction (what a decoder outputs).  All zero: or_transcode.
 * transcode_core is the one body of all three entries: o holds the rules of
 * or_transcode_ex2 (described there; all zero: none), stats has 10 entries,
 * words / modes / cbits may be NULL, cnt receives the OC_N decision counters. */
static int transcode_core(const uint8_t *frames, int64_t n, int W, int H, const float *scores, float thr,
                          int idr_at_cuts, int sh, int R, int T, int keyint, int qp, int intra, int subpel, int deblock,
                          int dalpha, int dbeta, const or_opts *o, uint8_t *out, int64_t cap, int64_t *sample_off,
                          int64_t *sample_size, uint8_t *sync, uint8_t *recon, int64_t *stats, uint32_t *words,
                          uint64_t *modes, int32_t *cbits, int64_t *cnt, int64_t *out_len) {
  if (n <= 0 || sh < 2 || (sh & 1) || R < 0 || R > 16 || keyint < 1 || qp > 51) return -1;
  if ((intra != 0 && intra != 1) || subpel < 0 || subpel > 2 || (deblock != 0 && deblock != 1)) return -1;
  if (dalpha < -6 || dalpha > 6 || dbeta < -6 || dbeta > 6 || (!deblock && (dalpha || dbeta))) return -1;
  if ((intra || deblock) && qp < 1) return -1;
  int sw = or_small_width(W, H, sh);
  int cw = (sw + 15) & ~15, ch = (sh + 15) & ~15, mbw = cw / 16, mbh = ch / 16;
  int64_t fsz = (int64_t)cw * ch * 3 / 2, dsz = (int64_t)W * H * 3 / 2;
  uint8_t *src = (uint8_t *)malloc((size_t)fsz), *rec[2];
  rec[0] = (uint8_t *)malloc((size_t)fsz);
  rec[1] = (uint8_t *)malloc((size_t)fsz);
  or_mb *mbs = (or_mb *)calloc((size_t)mbw * mbh, sizeof(or_mb));
  uint32_t *pw = (uint32_t *)calloc((size_t)mbw * mbh, sizeof(uint32_t));  /* the previous picture's final words */
  int64_t rcap = 64 + (int64_t)mbw * 420;
  uint8_t *rbsp = (uint8_t *)malloc((size_t)rcap);
  int rc = (src && rec[0] && rec[1] && mbs && pw && rbsp) ? 0 : -3;
  int64_t pos = 0, last_idr = 0, n_idr = 0;
  int cur = 0;
  for (int k = 0; k < 10; k++) stats[k] = 0;
  for (int k = 0; k < OC_N; k++) cnt[k] = 0;
  for (int64_t f = 0; f < n && !rc; f++) {
    or_downscale_nv12(frames + f * dsz, W, H, src, sw, sh);
    int idr = f == 0 || (idr_at_cuts && scores[f] > thr) || f - last_idr >= keyint;
    if (idr) last_idr = f;
    int j = (int)(f - last_idr);
    sample_off[f] = pos;
    sync[f] = (uint8_t)idr;
    if (idr) {
      if (intra) {
        encode_intra(src, rec[cur], cw, ch, qp, 1, o->intra4x4, o->lambda_i4, mbs,
                     cbits ? cbits + 2 * f * mbw * mbh : NULL, cnt);
      } else {  /* every macroblock I_PCM: the source */
        memcpy(rec[cur], src, (size_t)fsz);
        for (int k = 0; k < mbw * mbh; k++) {
          mbs[k].pcm = 1;
          mbs[k].i16 = mbs[k].i4 = mbs[k].cbp = mbs[k].mvx = mbs[k].mvy = 0;
        }
      }
      rc = write_picture(src, cw, ch, mbs, 1, (int)(n_idr & 1), 0, qp, intra, deblock, dalpha, dbeta, out, cap,
                         &pos, rbsp, rcap, stats);
      n_idr++;
    } else {
      encode_p(src, rec[cur ^ 1], rec[cur], cw, ch, R, T, qp, subpel, o, pw, j, mbs, stats, cnt);
      if (intra)
        encode_intra(src, rec[cur], cw, ch, qp, 0, o->intra4x4, o->lambda_i4, mbs,
                     cbits ? cbits + 2 * f * mbw * mbh : NULL, cnt);
      rc = write_picture(src, cw, ch, mbs, 0, 0, j & 0xffff, qp, intra, deblock, dalpha, dbeta, out, cap, &pos,
                         rbsp, rcap, stats);
    }
    /* the in-loop filter: the next picture predicts from, and the decoder
     * outputs, the filtered picture.  An all-I_PCM picture has qPav 0 on every
     * edge (alpha' = 0): nothing passes, and the filter leaves it as it is */
    if (deblock && !rc) stats[7] += deblock_picture(rec[cur], cw, ch, mbs, qp, 2 * dalpha, 2 * dbeta);
    sample_size[f] = pos - sample_off[f];
    for (int k = 0; k < mbw * mbh; k++) {  /* the final decisions, as the device reports them */
      pw[k] = mb_word(&mbs[k]);
      if (words) words[f * mbw * mbh + k] = pw[k];
      if (modes) modes[f * mbw * mbh + k] = mbs[k].i4 ? mbs[k].modes : ~(uint64_t)0;
    }
    if (recon) memcpy(recon + f * fsz, rec[cur], (size_t)fsz);
    cur ^= 1;
  }
  stats[3] = n_idr;
  *out_len = pos;
  free(src); free(rec[0]); free(rec[1]); free(mbs); free(pw); free(rbsp);
  return rc;
}

int or_transcode_ex(const uint8_t *frames, int64_t n, int W, int H, const float *scores, float thr,
                    int idr_at_cuts, int sh, int R, int T, int keyint, int qp, int intra, int subpel, int deblock,
                    int dalpha, int dbeta, uint8_t *out, int64_t cap, int64_t *sample_off,
                    int64_t *sample_size, uint8_t *sync, uint8_t *recon, int64_t *stats,
                    int64_t *out_len) {
  or_opts o = {0, 0, 0, 0, 0};
  int64_t st[10], cnt[OC_N];
  int rc = transcode_core(frames, n, W, H, scores, thr, idr_at_cuts, sh, R, T, keyint, qp, intra, subpel, deblock,
                          dalpha, dbeta, &o, out, cap, sample_off, sample_size, sync, recon, st, NULL, NULL, NULL, cnt,
                          out_len);
  for (int k = 0; k < 8 && rc != -1; k++) stats[k] = st[k];
  return rc;
}

/* or_transcode_ex2: or_transcode_ex with the rules merged since (DESIGN.md §11,
 * "Rate-aware motion cost and early P_Skip" and "Intra4x4"): mvcost, early_skip
 * (0 / 1; both need qp >= 1), mv_lambda16 (0: the formula's value for qp; 1 ..
 * 4096 only with mvcost), intra4x4 (0 / 1; needs intra and qp >= 1).  stats has
 * 10 entries: or_transcode_ex's eight (Intra16x16 MBs now counts I_NxN too),
 * early_skip_mbs, intra4x4_mbs.  words / modes (may be NULL): the command word
 * and the 64-bit mode word of every macroblock, [frame][my][mx], in the
 * encodings of include/vtseg.h; cbits (may be NULL): [frame][my][mx][2], the
 * bits of the Intra16x16 and the I_NxN candidate where intra4x4 tried both, else
 * 0; counters: OC_N decision counters (the enum above).  All four zero:
 * or_transcode_ex's bytes. */
int or_transcode_ex2(const uint8_t *frames, int64_t n, int W, int H, const float *scores, float thr,
                     int idr_at_cuts, int sh, int R, int T, int keyint, int qp, int intra, int subpel, int deblock,
                     int dalpha, int dbeta, int mvcost, int early_skip, int mv_lambda16, int intra4x4, uint8_t *out,
                     int64_t cap, int64_t *sample_off, int64_t *sample_size, uint8_t *sync, uint8_t *recon,
                     int64_t *stats, uint32_t *words, uint64_t *modes, int32_t *cbits, int64_t *counters,
                     int64_t *out_len) {
  if ((mvcost != 0 && mvcost != 1) || (early_skip != 0 && early_skip != 1) || (intra4x4 != 0 && intra4x4 != 1)) return -1;
  if (mv_lambda16 < 0 || mv_lambda16 > 4096 || (mv_lambda16 && !mvcost)) return -1;
  if ((mvcost || early_skip || intra4x4) && (qp < 1 || qp > 51)) return -1;
  if (intra4x4 && !intra) return -1;
  or_opts o = {mvcost, early_skip, intra4x4, 0, 0};
  if (qp >= 1 && qp <= 51) {
    o.lambda_mv = mv_lambda16 > 0 ? mv_lambda16 : lambda16_formula(qp);
    o.lambda_i4 = lambda16_formula(qp);
  }
  if (n > 0 && cbits) {
    int sw = or_small_width(W, H, sh), mbw = (sw + 15) / 16, mbh = (sh + 15) / 16;
    memset(cbits, 0, (size_t)n * mbw * mbh * 2 * sizeof(int32_t));
  }
  return transcode_core(frames, n, W, H, scores, thr, idr_at_cuts, sh, R, T, keyint, qp, intra, subpel, deblock,
                        dalpha, dbeta, &o, out, cap, sample_off, sample_size, sync, recon, stats, words, modes, cbits,
                        counters, out_len);
}

int or_transcode(const uint8_t *frames, int64_t n, int W, int H, const float *scores, float thr,
                 int idr_at_cuts, int sh, int R, int T, int keyint, int qp, uint8_t *out, int64_t cap, int64_t *sample_off,
                 int64_t *sample_size, uint8_t *sync, uint8_t *recon, int64_t *stats,
                 int64_t *out_len) {
  int64_t st[8];
  int rc = or_transcode_ex(frames, n, W, H, scores, thr, idr_at_cuts, sh, R, T, keyint, qp, 0, 0, 0, 0, 0, out, cap,
                           sample_off, sample_size, sync, recon, st, out_len);
  for (int k = 0; k < 4 && rc != -1; k++) stats[k] = st[k];
  return rc;
}
