// transcode_driver.cpp — vts_transcode / vts_transcode_ex: the host side of
// the 360p upload transcode.  One Transcoder lives for one
// call and walks the steps check, decode + downscale, plan, allocate, encode,
// finish; the kernels and their launch functions are transcode.hip's
// (transcode.h), the GOP plan and the chunk / ring arithmetic enc_plan.h's.
//
// Two streams: every level's motion search (with its intra coding, deblocking
// and hash) goes on s1, level j needing only level j - 1's reconstruction;
// the slice writing of a chunk of kChunkLevels levels (write, device offset
// scan, gather, I_PCM payloads, drain to the host) runs on s2 behind the
// chunk's last level_done event, overlapping the searches of later chunks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "enc_aq.h"
#include "enc_plan.h"
#include "enc_ratectl.h"
#include "mp4.h"
#include "session.h"
#include "transcode.h"

namespace vts {
namespace {

using clk = std::chrono::steady_clock;
double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

static_assert(sizeof(PlanEntry) == sizeof(int4), "the plan's entries are uploaded as the kernels' int4");

// ------------------------------------------------ the size-tagged structs
// A caller's struct holds `field` of T (T begins with every struct before it)
// when its struct_size reaches the field's end.
#define VTS_END_OF(T, field) (offsetof(T, field) + sizeof(T::field))
// ... then it is read from `ext` / written to `xinfo` (NULL: not wanted)
#define VTS_EXT_GET(dst, T, field) \
  do {                             \
    if (ext->struct_size >= VTS_END_OF(T, field)) (dst) = reinterpret_cast<const T *>(ext)->field; \
  } while (0)
#define VTS_XINFO_PUT(T, field, value) \
  do {                                 \
    if (xinfo && xinfo->struct_size >= VTS_END_OF(T, field)) reinterpret_cast<T *>(xinfo)->field = (value); \
  } while (0)
// The thresholds include/vtseg.h documents, pinned: an 8-byte ext, a 56-byte
// ext3 and every size in between are read as they always were.
static_assert(VTS_END_OF(vts_transcode_ext, subpel) == 8 && VTS_END_OF(vts_transcode_ext2, deblock) == 12 &&
              VTS_END_OF(vts_transcode_ext2, deblock_alpha) == 16 && VTS_END_OF(vts_transcode_ext2, deblock_beta) == 20 &&
              VTS_END_OF(vts_transcode_ext3, mvcost) == 28 && VTS_END_OF(vts_transcode_ext3, mv_lambda16) == 32 &&
              VTS_END_OF(vts_transcode_ext3, early_skip) == 36 && VTS_END_OF(vts_transcode_ext3, cmd_out) == 48 &&
              VTS_END_OF(vts_transcode_ext3, cmd_cap) == 56 && VTS_END_OF(vts_transcode_ext4, cabac) == 60 &&
              VTS_END_OF(vts_transcode_ext5, intra4x4) == 68 && VTS_END_OF(vts_transcode_ext5, i4_out) == 80 &&
              VTS_END_OF(vts_transcode_ext5, i4_cap) == 88 && VTS_END_OF(vts_transcode_ext6, partitions) == 92 &&
              VTS_END_OF(vts_transcode_ext6, mv_out) == 104 && VTS_END_OF(vts_transcode_ext6, mv_cap) == 112 &&
              sizeof(vts_transcode_ext6) == 112,
              "vts_transcode_ext .. ext6: struct_size >= 8, 12, 16, 20, 28, 32, 36, 48, 56, 60, 68, 80, 88, 92, 104, 112");
static_assert(VTS_END_OF(vts_transcode_ext7, bitrate_kbps) == 116 && VTS_END_OF(vts_transcode_ext7, qp_min) == 120 &&
              VTS_END_OF(vts_transcode_ext7, qp_max) == 124 && VTS_END_OF(vts_transcode_ext7, frame_qp) == 136 &&
              VTS_END_OF(vts_transcode_ext7, frame_qp_n) == 144 && VTS_END_OF(vts_transcode_ext7, qp_out) == 152 &&
              VTS_END_OF(vts_transcode_ext7, bits_out) == 160 && VTS_END_OF(vts_transcode_ext7, frame_cap) == 168 &&
              sizeof(vts_transcode_ext7) == 168,
              "vts_transcode_ext7: struct_size >= 116, 120, 124, 136, 144, 152, 160, 168");
static_assert(VTS_END_OF(vts_transcode_ext_info6, qp_sum) == 104 && VTS_END_OF(vts_transcode_ext_info6, qp_lo) == 108 &&
              VTS_END_OF(vts_transcode_ext_info6, qp_hi) == 112 && VTS_END_OF(vts_transcode_ext_info6, est_bits) == 120 &&
              VTS_END_OF(vts_transcode_ext_info6, frame_words) == 128 && sizeof(vts_transcode_ext_info6) == 128,
              "vts_transcode_ext_info6: struct_size >= 104, 108, 112, 120, 128");
static_assert(VTS_END_OF(vts_transcode_ext8, frame_first) == 176 && VTS_END_OF(vts_transcode_ext8, frame_count) == 184 &&
              sizeof(vts_transcode_ext8) == 184 && VTS_END_OF(vts_transcode_ext_info7, frame_first) == 136 &&
              VTS_END_OF(vts_transcode_ext_info7, frame_count) == 144 && sizeof(vts_transcode_ext_info7) == 144,
              "vts_transcode_ext8: struct_size >= 176, 184; vts_transcode_ext_info7: >= 136, 144");
static_assert(VTS_END_OF(vts_transcode_ext9, aq_strength_q8) == 188 && VTS_END_OF(vts_transcode_ext9, aq_max) == 192 &&
              VTS_END_OF(vts_transcode_ext9, mbqp_out) == 200 && VTS_END_OF(vts_transcode_ext9, mbqp_cap) == 208 &&
              sizeof(vts_transcode_ext9) == 208 && VTS_END_OF(vts_transcode_ext_info8, mbqp_words) == 152 &&
              VTS_END_OF(vts_transcode_ext_info8, aq_lo) == 156 && VTS_END_OF(vts_transcode_ext_info8, aq_hi) == 160 &&
              VTS_END_OF(vts_transcode_ext_info8, aq_mbs) == 168 && sizeof(vts_transcode_ext_info8) == 168,
              "vts_transcode_ext9: struct_size >= 188, 192, 200, 208; vts_transcode_ext_info8: >= 152, 156, 160, 168");
static_assert(VTS_END_OF(vts_transcode_ext_info, _pad) == 8 && VTS_END_OF(vts_transcode_ext_info, subpel_mbs) == 16 &&
              VTS_END_OF(vts_transcode_ext_info, qpel_mbs) == 24 && VTS_END_OF(vts_transcode_ext_info2, deblock_mbs) == 32 &&
              VTS_END_OF(vts_transcode_ext_info3, early_skip_mbs) == 40 &&
              VTS_END_OF(vts_transcode_ext_info3, cmd_words) == 48 &&
              VTS_END_OF(vts_transcode_ext_info4, intra4x4_mbs) == 56 && VTS_END_OF(vts_transcode_ext_info4, i4_words) == 64 &&
              VTS_END_OF(vts_transcode_ext_info5, p16x8_mbs) == 72 && VTS_END_OF(vts_transcode_ext_info5, p8x16_mbs) == 80 &&
              VTS_END_OF(vts_transcode_ext_info5, p8x8_mbs) == 88 && VTS_END_OF(vts_transcode_ext_info5, mv_words) == 96 &&
              sizeof(vts_transcode_ext_info5) == 96,
              "vts_transcode_ext_info .. info5: struct_size >= 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96");

// What a vts_transcode_ex call asks for, defaults applied and checked.
struct TranscodeOpts {
  int subpel = 0, deblock = 0, dbk_alpha = 0, dbk_beta = 0;
  int mvcost = 0, mv_lambda16 = 0, early_skip = 0;
  int cabac = 0;
  int intra4x4 = 0;
  uint32_t *cmd_out = nullptr;
  int64_t cmd_cap = 0;
  uint64_t *i4_out = nullptr;
  int64_t i4_cap = 0;
  int partitions = 0;
  uint32_t *mv_out = nullptr;
  int64_t mv_cap = 0;
  int bitrate_kbps = 0, qp_min = 0, qp_max = 0;  // rate control (enc_ratectl.h); the bounds with their defaults applied
  const uint8_t *frame_qp = nullptr;             // the caller's QP of each frame
  int64_t frame_qp_n = 0;
  uint8_t *qp_out = nullptr;
  uint32_t *bits_out = nullptr;
  int64_t frame_cap = 0;
  int64_t f0 = 0, n = 0;   // the frames [f0, f0 + n) of the video are transcoded (vts_transcode_ext8; all by default)
  int aq_strength_q8 = 0, aq_max = 0;  // adaptive quantisation (enc_aq.h); aq_max with its default applied
  int aq_lo = 1, aq_hi = 51;           // ... a macroblock's QP is clamped to them: the caller's qp_min / qp_max where given
  uint8_t *mbqp_out = nullptr;
  int64_t mbqp_cap = 0;
  bool per_frame = false;  // frame_qp or bitrate_kbps: the kernels read a QP per picture and measure its rate
  int rate = 0;         // SearchArgs.rate: mvcost | early_skip << 1
  int sh = 0, R = 0, T = 0, qp = 0, keyint = 0;  // output height, search range, max SAD, residual QP (0: none)
  bool intra = false, idr_at_cuts = false;
  bool hashed = false;  // recon_hash is computed
  float thr = 0;        // scene-cut threshold of idr_at_cuts
};
// The size-tagged structs (only the prefix known here is read) and the
// parameters into `o`; VTS_OK or the error
int read_opts(const vts_ctx *c, const vts_transcode_params *pin, const vts_transcode_ext *ext,
              const vts_transcode_ext_info *xinfo, TranscodeOpts *out) {
  TranscodeOpts &o = *out;
  o.n = c->n_frames;
  if (ext) {
    if (ext->struct_size < VTS_END_OF(vts_transcode_ext, subpel))
      return fail(VTS_E_INVALID, "vts_transcode_ext.struct_size %u < 8", ext->struct_size);
    o.subpel = ext->subpel;
    if (o.subpel < 0 || o.subpel > 2) return fail(VTS_E_INVALID, "subpel %d: 0, 1 or 2", o.subpel);
    // vts_transcode_ext2: each field only when the caller's struct holds it
    VTS_EXT_GET(o.deblock, vts_transcode_ext2, deblock);
    VTS_EXT_GET(o.dbk_alpha, vts_transcode_ext2, deblock_alpha);
    VTS_EXT_GET(o.dbk_beta, vts_transcode_ext2, deblock_beta);
    if (o.deblock != 0 && o.deblock != 1) return fail(VTS_E_INVALID, "deblock %d: 0 or 1", o.deblock);
    if (o.dbk_alpha < -6 || o.dbk_alpha > 6) return fail(VTS_E_INVALID, "deblock_alpha %d: -6 .. 6", o.dbk_alpha);
    if (o.dbk_beta < -6 || o.dbk_beta > 6) return fail(VTS_E_INVALID, "deblock_beta %d: -6 .. 6", o.dbk_beta);
    if (!o.deblock && o.dbk_alpha) return fail(VTS_E_INVALID, "deblock_alpha %d without deblock = 1", o.dbk_alpha);
    if (!o.deblock && o.dbk_beta) return fail(VTS_E_INVALID, "deblock_beta %d without deblock = 1", o.dbk_beta);
    // vts_transcode_ext3, the same way
    VTS_EXT_GET(o.mvcost, vts_transcode_ext3, mvcost);
    VTS_EXT_GET(o.mv_lambda16, vts_transcode_ext3, mv_lambda16);
    VTS_EXT_GET(o.early_skip, vts_transcode_ext3, early_skip);
    VTS_EXT_GET(o.cmd_out, vts_transcode_ext3, cmd_out);
    VTS_EXT_GET(o.cmd_cap, vts_transcode_ext3, cmd_cap);
    if (o.mvcost != 0 && o.mvcost != 1) return fail(VTS_E_INVALID, "mvcost %d: 0 or 1", o.mvcost);
    if (o.early_skip != 0 && o.early_skip != 1) return fail(VTS_E_INVALID, "early_skip %d: 0 or 1", o.early_skip);
    if (o.mv_lambda16 < 0 || o.mv_lambda16 > 4096) return fail(VTS_E_INVALID, "mv_lambda16 %d: 0 .. 4096", o.mv_lambda16);
    if (!o.mvcost && o.mv_lambda16) return fail(VTS_E_INVALID, "mv_lambda16 %d without mvcost = 1", o.mv_lambda16);
    // vts_transcode_ext4, the same way
    VTS_EXT_GET(o.cabac, vts_transcode_ext4, cabac);
    if (o.cabac != 0 && o.cabac != 1) return fail(VTS_E_INVALID, "cabac %d: 0 or 1", o.cabac);
    // vts_transcode_ext5, the same way
    VTS_EXT_GET(o.intra4x4, vts_transcode_ext5, intra4x4);
    VTS_EXT_GET(o.i4_out, vts_transcode_ext5, i4_out);
    VTS_EXT_GET(o.i4_cap, vts_transcode_ext5, i4_cap);
    if (o.intra4x4 != 0 && o.intra4x4 != 1) return fail(VTS_E_INVALID, "intra4x4 %d: 0 or 1", o.intra4x4);
    // vts_transcode_ext6, the same way
    VTS_EXT_GET(o.partitions, vts_transcode_ext6, partitions);
    VTS_EXT_GET(o.mv_out, vts_transcode_ext6, mv_out);
    VTS_EXT_GET(o.mv_cap, vts_transcode_ext6, mv_cap);
    if (o.partitions != 0 && o.partitions != 1) return fail(VTS_E_INVALID, "partitions %d: 0 or 1", o.partitions);
    // vts_transcode_ext7, the same way
    VTS_EXT_GET(o.bitrate_kbps, vts_transcode_ext7, bitrate_kbps);
    VTS_EXT_GET(o.qp_min, vts_transcode_ext7, qp_min);
    VTS_EXT_GET(o.qp_max, vts_transcode_ext7, qp_max);
    VTS_EXT_GET(o.frame_qp, vts_transcode_ext7, frame_qp);
    VTS_EXT_GET(o.frame_qp_n, vts_transcode_ext7, frame_qp_n);
    VTS_EXT_GET(o.qp_out, vts_transcode_ext7, qp_out);
    VTS_EXT_GET(o.bits_out, vts_transcode_ext7, bits_out);
    VTS_EXT_GET(o.frame_cap, vts_transcode_ext7, frame_cap);
    // vts_transcode_ext8, the same way: the range, before what is counted in its frames
    int64_t count = 0;
    VTS_EXT_GET(o.f0, vts_transcode_ext8, frame_first);
    VTS_EXT_GET(count, vts_transcode_ext8, frame_count);
    if (o.f0 < 0 || (o.f0 >= c->n_frames && (o.f0 || count)))  // 0, 0 on an empty video is the call as it was
      return fail(VTS_E_INVALID, "frame_first %lld: 0 .. %lld", static_cast<long long>(o.f0),
                  static_cast<long long>(c->n_frames - 1));
    if (count < 0 || count > c->n_frames - o.f0)
      return fail(VTS_E_INVALID, "frame_count %lld: 0 .. %lld from frame_first %lld", static_cast<long long>(count),
                  static_cast<long long>(c->n_frames - o.f0), static_cast<long long>(o.f0));
    o.n = count ? count : c->n_frames - o.f0;
    // vts_transcode_ext9, the same way
    VTS_EXT_GET(o.aq_strength_q8, vts_transcode_ext9, aq_strength_q8);
    VTS_EXT_GET(o.aq_max, vts_transcode_ext9, aq_max);
    VTS_EXT_GET(o.mbqp_out, vts_transcode_ext9, mbqp_out);
    VTS_EXT_GET(o.mbqp_cap, vts_transcode_ext9, mbqp_cap);
    if (o.aq_strength_q8 < 0 || o.aq_strength_q8 > full::eaq::kStrengthMaxQ8)
      return fail(VTS_E_INVALID, "aq_strength_q8 %d: 0 .. %d", o.aq_strength_q8, full::eaq::kStrengthMaxQ8);
    if (o.aq_max < 0 || o.aq_max > full::eaq::kMaxLimit)
      return fail(VTS_E_INVALID, "aq_max %d: 0 (default) or 1 .. %d", o.aq_max, full::eaq::kMaxLimit);
    if (!o.aq_strength_q8 && o.aq_max) return fail(VTS_E_INVALID, "aq_max %d without aq_strength_q8", o.aq_max);
    if (o.aq_strength_q8 && !o.aq_max) o.aq_max = full::eaq::kMaxDefault;
    if (o.bitrate_kbps < 0 || o.bitrate_kbps > full::erc::kMaxKbps)
      return fail(VTS_E_INVALID, "bitrate_kbps %d: 0 .. %d", o.bitrate_kbps, full::erc::kMaxKbps);
    if (o.qp_min < 0 || o.qp_min > 51) return fail(VTS_E_INVALID, "qp_min %d: 0 (default) or 1 .. 51", o.qp_min);
    if (o.qp_max < 0 || o.qp_max > 51) return fail(VTS_E_INVALID, "qp_max %d: 0 (default) or 1 .. 51", o.qp_max);
    o.per_frame = o.bitrate_kbps != 0 || o.frame_qp != nullptr;
    if (!o.per_frame && o.qp_min) return fail(VTS_E_INVALID, "qp_min %d without bitrate_kbps or frame_qp", o.qp_min);
    if (!o.per_frame && o.qp_max) return fail(VTS_E_INVALID, "qp_max %d without bitrate_kbps or frame_qp", o.qp_max);
    // a macroblock's QP stays inside the bounds the caller gave; a bound left at 0 is 1 or 51 for it, not the
    // controller's default: a frame_qp below 10 must not move a macroblock whose offset is 0
    if (o.qp_min) o.aq_lo = o.qp_min;
    if (o.qp_max) o.aq_hi = o.qp_max;
    if (o.per_frame) {
      if (!o.qp_min) o.qp_min = full::erc::kQpMinDefault;
      if (!o.qp_max) o.qp_max = full::erc::kQpMaxDefault;
      if (o.qp_min > o.qp_max) return fail(VTS_E_INVALID, "qp_min %d > qp_max %d", o.qp_min, o.qp_max);
    }
    if (o.frame_qp && o.bitrate_kbps) return fail(VTS_E_INVALID, "frame_qp together with bitrate_kbps %d", o.bitrate_kbps);
    if (o.frame_qp) {
      if (o.frame_qp_n != o.n)
        return fail(VTS_E_INVALID, "frame_qp_n %lld: the %s has %lld frames", static_cast<long long>(o.frame_qp_n),
                    o.n == c->n_frames ? "video" : "range", static_cast<long long>(o.n));
      for (int64_t f = 0; f < o.frame_qp_n; ++f)
        if (o.frame_qp[f] < 1 || o.frame_qp[f] > 51)
          return fail(VTS_E_INVALID, "frame_qp[%lld] %d: 1 .. 51", static_cast<long long>(f), o.frame_qp[f]);
    }
  }
  o.rate = o.mvcost | (o.early_skip << 1);
  if (xinfo && xinfo->struct_size < VTS_END_OF(vts_transcode_ext_info, _pad))
    return fail(VTS_E_INVALID, "vts_transcode_ext_info.struct_size %u < 8", xinfo->struct_size);
  vts_transcode_params p{};
  if (pin) p = *pin;
  o.sh = p.height > 0 ? p.height : 360;
  o.R = p.search_range == 0 ? 8 : std::max(0, p.search_range);
  o.T = p.max_mb_sad == 0 ? 1536 : p.max_mb_sad;
  o.qp = p.qp == 0 ? 28 : (p.qp < 0 ? 0 : p.qp);  // 0: no residual coding (the round-2 encoder)
  if (o.qp > 51) return fail(VTS_E_INVALID, "qp %d > 51", o.qp);
  if (p.intra != 0 && p.intra != 1) return fail(VTS_E_INVALID, "intra %d: 0 or 1", p.intra);
  o.intra = p.intra == 1;
  o.hashed = o.intra || o.subpel != 0 || o.deblock || o.rate;
  if (o.partitions && o.qp < 1) return fail(VTS_E_INVALID, "partitions = 1 needs residual coding (qp >= 0)");
  if (o.partitions && o.T < 0) return fail(VTS_E_INVALID, "partitions = 1 needs max_mb_sad >= 0 (inter macroblocks)");
  if (o.partitions && !o.mvcost) return fail(VTS_E_INVALID, "partitions = 1 needs mvcost = 1 (a shape is chosen by rate)");
  const char *pf = o.bitrate_kbps ? "bitrate_kbps" : "frame_qp";
  if (o.per_frame && o.qp < 1) return fail(VTS_E_INVALID, "%s needs residual coding (qp >= 0)", pf);
  if (o.per_frame && o.T < 0) return fail(VTS_E_INVALID, "%s needs max_mb_sad >= 0 (inter macroblocks)", pf);
  if (o.per_frame && !o.mvcost) return fail(VTS_E_INVALID, "%s needs mvcost = 1", pf);
  if (o.aq_strength_q8 && o.qp < 1) return fail(VTS_E_INVALID, "aq_strength_q8 needs residual coding (qp >= 0)");
  if (o.aq_strength_q8 && o.T < 0) return fail(VTS_E_INVALID, "aq_strength_q8 needs max_mb_sad >= 0 (inter macroblocks)");
  if (o.aq_strength_q8 && !o.mvcost) return fail(VTS_E_INVALID, "aq_strength_q8 needs mvcost = 1");
  if (o.intra4x4 && o.qp < 1) return fail(VTS_E_INVALID, "intra4x4 = 1 needs residual coding (qp >= 0)");
  if (o.intra4x4 && !o.intra) return fail(VTS_E_INVALID, "intra4x4 = 1 needs intra = 1");
  if (o.intra && o.qp < 1) return fail(VTS_E_INVALID, "intra = 1 needs residual coding (qp >= 0)");
  if (o.deblock && o.qp < 1) return fail(VTS_E_INVALID, "deblock = 1 needs residual coding (qp >= 0)");
  if (o.mvcost && o.qp < 1) return fail(VTS_E_INVALID, "mvcost = 1 needs residual coding (qp >= 0)");
  if (o.early_skip && o.qp < 1) return fail(VTS_E_INVALID, "early_skip = 1 needs residual coding (qp >= 0)");
  if (o.cabac && o.qp < 1) return fail(VTS_E_INVALID, "cabac = 1 needs residual coding (qp >= 0)");
  o.keyint = p.keyint > 0 ? p.keyint : 250;
  o.idr_at_cuts = p.idr_at_cuts != 0;
  o.thr = p.cut_threshold > 0 ? p.cut_threshold : c->params.cut_threshold;
  if ((o.sh & 1) || o.sh < 16 || o.sh > c->height)
    return fail(VTS_E_INVALID, "output height %d: even, 16 .. source height %d", o.sh, c->height);
  if (o.R > kMaxRange) return fail(VTS_E_INVALID, "search_range %d > %d", o.R, kMaxRange);
  return VTS_OK;
}

// ------------------------------------------------------- device scratch
template <class T>
int dev_alloc(T **p, size_t n) {
  HIP_TRY(vts::dmalloc(reinterpret_cast<void **>(p), std::max<size_t>(1, n) * sizeof(T)));
  return VTS_OK;
}

// Transcode scratch, freed on every exit path.  vts::dfree hands a range
// straight back to the process-wide cache (no implicit device synchronisation
// as with hipFree), so the streams whose kernels may still use the buffers
// are drained first: an early return after the searches were queued must not
// let a later allocation reuse memory those kernels still write.
struct DevBufs {
  std::vector<void *> ptrs;
  std::vector<hipStream_t> streams;  // synchronised before anything is freed
  template <class T>
  int get(T **p, size_t n) {
    VTS_TRY(dev_alloc(p, n));
    ptrs.push_back(*p);
    return VTS_OK;
  }
  ~DevBufs() {
    for (hipStream_t s : streams) (void)hipStreamSynchronize(s);
    for (void *p : ptrs) vts::dfree(p);
  }
};

// The call's events, destroyed on every exit path
struct Events {
  std::vector<hipEvent_t> level_done;     // [level] on s1: its search, intra coding, deblocking and hash are queued
  std::vector<hipEvent_t> chunk_written;  // [chunk] on s2: its slices written (its ring slots free again)
  hipEvent_t search_begin = nullptr, search_end = nullptr;  // s1, the span info.ms[1] reports
  hipEvent_t write_begin = nullptr, write_end = nullptr;    // s2, info.ms[2]
  hipEvent_t d2h = nullptr;                                 // s2, reused: the last chunk's copy to the host
  int create(int64_t levels, int64_t chunks) {
    level_done.assign(static_cast<size_t>(levels), nullptr);
    chunk_written.assign(static_cast<size_t>(chunks), nullptr);
    for (hipEvent_t *e : singles()) HIP_TRY(hipEventCreate(e));
    for (auto &e : level_done) HIP_TRY(hipEventCreate(&e));
    for (auto &e : chunk_written) HIP_TRY(hipEventCreate(&e));
    return VTS_OK;
  }
  ~Events() {
    for (hipEvent_t *e : singles())
      if (*e) (void)hipEventDestroy(*e);
    for (const auto *v : {&level_done, &chunk_written})
      for (hipEvent_t e : *v)
        if (e) (void)hipEventDestroy(e);
  }

 private:
  std::vector<hipEvent_t *> singles() { return {&search_begin, &search_end, &write_begin, &write_end, &d2h}; }
};

// ----------------------------------------------------------- the driver
struct Transcoder {
  vts_ctx *c;
  const char *out_path;
  TranscodeOpts opt;
  GopPlan plan;
  // geometry
  int64_t n = 0, delta = 0;  // frames; their constant duration (track timescale)
  int64_t f0 = 0;            // the video's frame that is frame 0 here (the small store's slot 0)
  int mbw = 0, mbh = 0, nmb = 0;
  int64_t cap = 0;           // staging slot per slice
  int64_t cmd_words = 0;     // n * nmb: the command (and Intra4x4PredModes) words of every macroblock
  int64_t mv_words = 0;      // 4 n * nmb: the quadrant vectors of every macroblock
  int64_t max_chunk = 0;     // entries of the largest chunk
  hipStream_t s1 = nullptr, s2 = nullptr;
  double ms[4] = {0, 0, 0, 0}, mux_ms = 0;
  // output drained to the host every chunk (absolute bytes [chunk_start[c],
  // chunk_start[c+1])) and appended to the MP4's mdat while the GPU works on
  // the next chunk; the sample table (display order) points into mdat.
  // Declared before `bufs`, whose destructor drains the copy into host.back()
  Mp4Writer mw;
  std::vector<std::unique_ptr<uint8_t[]>> host;
  std::vector<int64_t> chunk_start{0}, chunk_file;  // chunk c's first output byte; its file offset
  bool pending = false;                             // a chunk's D2H not yet written out
  // device buffers, all from one alloc(); `bufs` drains both streams before it frees them
  DevBufs bufs;
  struct {
    int4 *sent, *went;  // the plan's entries
    int4 *hent;         // level 0's entries with the frame as the slot (hashing the IDR sources)
    uint8_t *recon;     // [2 ngop slots]
    uint32_t *cmd;      // [entry][mb], every frame: searches run ahead
    uint8_t *cbp;       // [entry][mb]
    uint64_t *i4;       // intra4x4: [entry][mb] mode words, ~0 where enc_intra<true> writes none
    uint32_t *mv4;      // partitions: [entry][mb][4] quadrant vectors, every frame as cmd
    int16_t *coef;      // qp >= 1: residual levels, a ring of kRing levels
    uint8_t *stage, *out;        // [max_chunk slices][cap]; the packed chunk
    int64_t *total, *base, *fr;  // running output total; the total before the chunk; per frame: offset, size
    int32_t *sizes;              // [slice]
    int64_t *offs;               // [slice]
    unsigned long long *stats;   // [kStCount] (transcode.h)
    uint32_t *err;
    uint4 *jobs;                 // I_PCM payload jobs of a chunk
    uint32_t *njobs;
    uint8_t *qp_f;               // per_frame: [frame] the QP each picture is coded at
    uint32_t *est_f;             // per_frame: [frame] the rate measure
    int64_t *rc_spent;           // bitrate_kbps: [GOP] the measure of its pictures so far
    int32_t *rc_len;             // bitrate_kbps: [GOP] its pictures
    int8_t *aq_off;              // aq_strength_q8: [frame][mb] the macroblocks' QP offsets
  } d{};
  Events ev;  // destroyed before `bufs` drains and frees
  int64_t next_search = 1;
  bool searches_done = false;

  Transcoder(vts_ctx *ctx, const char *path) : c(ctx), out_path(path) {}
  const SmallStore &S() const { return c->small; }

  int check(vts_transcode_ext_info *xinfo);
  int decode();
  int alloc();
  int alloc_rate();
  int encode();
  int finish(vts_transcode_info *info, vts_transcode_ext_info *xinfo);

  // Level j on the device: its entries and its rows of the per-entry arrays
  struct Level {
    int64_t e0, ne;        // first entry (into sent / went), entries
    const int4 *ent;       // search entries
    uint32_t *cmd;
    uint8_t *cbp;
    uint64_t *i4;          // nullptr without intra4x4
    uint32_t *mv4;         // nullptr without partitions
    int16_t *coef;         // the level's ring slot; nullptr without residual coding
  };
  Level level(int64_t j) const {
    const int64_t e0 = plan.lvl_off[j];
    return {e0, plan.lvl_off[j + 1] - e0, d.sent + e0, d.cmd + e0 * nmb, d.cbp + e0 * nmb,
            d.i4 ? d.i4 + e0 * nmb : nullptr, d.mv4 ? d.mv4 + e0 * nmb * 4 : nullptr,
            d.coef ? d.coef + (j % kRing) * plan.ngop * nmb * kCoefPerMb : nullptr};
  }
  SearchArgs search_args(int64_t j) const;
  IntraArgs intra_args(int64_t j) const;
  DeblockArgs deblock_args(int64_t j) const;
  HashArgs hash_args(int64_t j) const;
  WriteArgs write_args(int64_t c) const;
  PackArgs pack_args(int64_t c) const;
  int enqueue_level(int64_t j);
  int enqueue_searches(int64_t upto);
  int write_chunk(int64_t c);
  int drain_pending();
  int copy_words();
  int mux();
};

// 0. what can be refused before any device work: a variable frame rate (the
// writer's stts is one entry), the output size, word buffers too small
int Transcoder::check(vts_transcode_ext_info *xinfo) {
  n = opt.n;
  f0 = opt.f0;
  const int64_t *pts = c->pts.data() + f0;  // of the range's frames
  delta = n > 1 ? pts[1] - pts[0] : std::max<int64_t>(1, c->info.track_timescale / 30);
  for (int64_t i = 1; i < n; ++i)
    if (pts[i] - pts[i - 1] != delta)
      return fail(VTS_E_UNSUPPORTED, "variable frame rate (frame %lld) is not transcoded",
                  static_cast<long long>(f0 + i));
  VTS_XINFO_PUT(vts_transcode_ext_info7, frame_first, f0);
  VTS_XINFO_PUT(vts_transcode_ext_info7, frame_count, n);
  HIP_TRY(hipSetDevice(c->device));
  VTS_TRY(setup_small(c, opt.sh, f0, f0 + n));
  mbw = S().cw / 16;
  mbh = S().ch / 16;
  nmb = mbw * mbh;
  cap = slice_slot_bytes(mbw, opt.cabac != 0, opt.aq_strength_q8 != 0);
  // the command words of every macroblock, [frame][my][mx]: reported always, copied out when asked
  cmd_words = n * nmb;
  VTS_XINFO_PUT(vts_transcode_ext_info3, cmd_words, cmd_words);
  if (opt.cmd_out && opt.cmd_cap < cmd_words)
    return fail(VTS_E_CAPACITY, "cmd_cap %lld < %lld command words", static_cast<long long>(opt.cmd_cap),
                static_cast<long long>(cmd_words));
  // the Intra4x4PredModes word of every macroblock, the same way
  VTS_XINFO_PUT(vts_transcode_ext_info4, i4_words, cmd_words);
  if (opt.i4_out && opt.i4_cap < cmd_words)
    return fail(VTS_E_CAPACITY, "i4_cap %lld < %lld mode words", static_cast<long long>(opt.i4_cap),
                static_cast<long long>(cmd_words));
  // the four quadrant vectors of every macroblock, the same way
  mv_words = 4 * cmd_words;
  VTS_XINFO_PUT(vts_transcode_ext_info5, mv_words, mv_words);
  if (opt.mv_out && opt.mv_cap < mv_words)
    return fail(VTS_E_CAPACITY, "mv_cap %lld < %lld vector words", static_cast<long long>(opt.mv_cap),
                static_cast<long long>(mv_words));
  // the QP of every macroblock, the same way
  VTS_XINFO_PUT(vts_transcode_ext_info8, mbqp_words, cmd_words);
  if (opt.mbqp_out && opt.mbqp_cap < cmd_words)
    return fail(VTS_E_CAPACITY, "mbqp_cap %lld < %lld macroblocks", static_cast<long long>(opt.mbqp_cap),
                static_cast<long long>(cmd_words));
  // the QP and the rate measure of every frame, the same way
  VTS_XINFO_PUT(vts_transcode_ext_info6, frame_words, n);
  if (opt.qp_out && opt.frame_cap < n)
    return fail(VTS_E_CAPACITY, "frame_cap %lld < %lld frames (qp_out)", static_cast<long long>(opt.frame_cap),
                static_cast<long long>(n));
  if (opt.bits_out && opt.frame_cap < n)
    return fail(VTS_E_CAPACITY, "frame_cap %lld < %lld frames (bits_out)", static_cast<long long>(opt.frame_cap),
                static_cast<long long>(n));
  return VTS_OK;
}

// 1. decode + score + downscale
int Transcoder::decode() {
  const auto t0 = clk::now();
  c->small.on = true;
  const int rc = run_all(c);
  c->small.on = false;
  VTS_TRY(rc);
  VTS_TRY(fetch_scores(c));
  ms[0] = ms_since(t0);
  return VTS_OK;
}

// 3. every device buffer, the entry tables uploaded, the counters zeroed, the
// events.  The uploads and the zeroing block, so they are done before
// anything is queued on either stream: no stream has to order them.
int Transcoder::alloc() {
  const size_t entries = plan.went.size();
  max_chunk = vts::max_chunk(plan);
  VTS_TRY(bufs.get(&d.sent, entries));
  VTS_TRY(bufs.get(&d.went, entries));
  VTS_TRY(bufs.get(&d.recon, static_cast<size_t>(2 * plan.ngop * S().stride + 256)));
  VTS_TRY(bufs.get(&d.cmd, entries * nmb));
  VTS_TRY(bufs.get(&d.cbp, entries * nmb));
  if (opt.intra4x4) VTS_TRY(bufs.get(&d.i4, entries * nmb));
  if (opt.partitions) VTS_TRY(bufs.get(&d.mv4, entries * nmb * 4));
  if (opt.qp >= 1) VTS_TRY(bufs.get(&d.coef, static_cast<size_t>(kRing * plan.ngop * nmb * kCoefPerMb)));
  VTS_TRY(bufs.get(&d.stage, static_cast<size_t>(max_chunk * mbh * cap)));
  VTS_TRY(bufs.get(&d.out, static_cast<size_t>(max_chunk * mbh * cap)));
  VTS_TRY(bufs.get(&d.total, 1));
  VTS_TRY(bufs.get(&d.base, 1));
  VTS_TRY(bufs.get(&d.fr, static_cast<size_t>(2 * n)));
  VTS_TRY(bufs.get(&d.sizes, static_cast<size_t>(max_chunk * mbh)));
  VTS_TRY(bufs.get(&d.offs, static_cast<size_t>(max_chunk * mbh)));
  VTS_TRY(bufs.get(&d.stats, kStCount));
  VTS_TRY(bufs.get(&d.err, 1));
  VTS_TRY(bufs.get(&d.jobs, static_cast<size_t>(max_chunk * nmb)));
  VTS_TRY(bufs.get(&d.njobs, 1));
  if (opt.aq_strength_q8) VTS_TRY(bufs.get(&d.aq_off, static_cast<size_t>(n * nmb)));
  s1 = c->s_dec;
  s2 = c->s_score;
  bufs.streams = {s1, s2};
  HIP_TRY(hipMemcpy(d.sent, plan.sent.data(), entries * sizeof(int4), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.went, plan.went.data(), entries * sizeof(int4), hipMemcpyHostToDevice));
  if (opt.hashed && !opt.intra) {
    std::vector<PlanEntry> hent(plan.sent.begin(), plan.sent.begin() + plan.lvl_off[1]);
    for (PlanEntry &h : hent) h.z = h.x;
    VTS_TRY(bufs.get(&d.hent, hent.size()));
    HIP_TRY(hipMemcpy(d.hent, hent.data(), hent.size() * sizeof(int4), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemset(d.stats, 0, kStCount * sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(d.err, 0, sizeof(uint32_t), s2));
  if (opt.intra4x4) HIP_TRY(hipMemsetAsync(d.i4, 0xff, entries * static_cast<size_t>(nmb) * sizeof(uint64_t), s1));
  // no kernel writes the IDR level's vectors: they read as "no vector", as every intra macroblock's do
  if (opt.per_frame) VTS_TRY(alloc_rate());
  if (opt.partitions)
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d.mv4), static_cast<int>(kPcmCmdWord),
                              entries * static_cast<size_t>(nmb) * 4, s1));
  return ev.create(plan.maxlen, n_chunks(plan));
}

// The per-picture QPs and the rate measure (vts_transcode_ext7).  frame_qp:
// the caller's QPs; bitrate_kbps: every picture starts at picture 0's QP and
// enc_rc sets the others as their GOP goes.  A picture no kernel codes (an IDR
// picture without intra) measures as all I_PCM from the start.
int Transcoder::alloc_rate() {
  const size_t nf = static_cast<size_t>(n);
  VTS_TRY(bufs.get(&d.qp_f, nf));
  VTS_TRY(bufs.get(&d.est_f, nf));
  std::vector<uint8_t> qps(nf, static_cast<uint8_t>(full::erc::first_qp(opt.qp, opt.qp_min, opt.qp_max)));
  if (opt.frame_qp) qps.assign(opt.frame_qp, opt.frame_qp + nf);
  std::vector<uint32_t> est(nf, 0);
  if (!opt.intra)
    for (int64_t f : plan.gop_start) est[f] = static_cast<uint32_t>(kPcmMbBits) * static_cast<uint32_t>(nmb);
  HIP_TRY(hipMemcpy(d.qp_f, qps.data(), nf, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.est_f, est.data(), nf * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (opt.bitrate_kbps) {
    std::vector<int32_t> len(static_cast<size_t>(plan.ngop));
    for (int64_t k = 0; k < plan.ngop; ++k)
      len[k] = static_cast<int32_t>((k + 1 < plan.ngop ? plan.gop_start[k + 1] : n) - plan.gop_start[k]);
    const std::vector<int64_t> none(len.size(), 0);
    VTS_TRY(bufs.get(&d.rc_spent, len.size()));
    VTS_TRY(bufs.get(&d.rc_len, len.size()));
    HIP_TRY(hipMemcpy(d.rc_spent, none.data(), none.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.rc_len, len.data(), len.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  return VTS_OK;
}

SearchArgs Transcoder::search_args(int64_t j) const {
  const Level l = level(j);
  SearchArgs a{};
  a.ent = l.ent;
  a.small = S().d;
  a.stride = S().stride;
  a.recon = d.recon;
  a.cmd = l.cmd;
  a.cbp = l.cbp;
  a.coef = l.coef;
  a.cw = S().cw;
  a.ch = S().ch;
  a.mbw = mbw;
  a.nmb = nmb;
  a.range = opt.R;
  a.max_sad = opt.T;
  a.qp = opt.qp;
  a.sp_stats = d.stats + kStHalf;  // and kStQuarter
  if (opt.rate) {
    a.rate = opt.rate;
    a.cmd_prev = level(j - 1).cmd;
    a.gop_pos = static_cast<int32_t>(j);
    a.lambda16 = search_lambda16(opt.qp, opt.mv_lambda16);
    a.es_stat = d.stats + kStEarlySkip;
    a.mv4 = l.mv4;
    a.mv4_prev = level(j - 1).mv4;
    a.qp_f = d.qp_f;
    a.est_f = d.est_f;
    a.mv_lambda16 = opt.mv_lambda16;
    a.pcm_bits = opt.intra ? 0 : kPcmMbBits;
    a.aq_off = d.aq_off;
    a.aq_lo = opt.aq_lo;
    a.aq_hi = opt.aq_hi;
  }
  return a;
}

IntraArgs Transcoder::intra_args(int64_t j) const {
  const Level l = level(j);
  IntraArgs a{};
  a.ent = l.ent;
  a.small = S().d;
  a.stride = S().stride;
  a.recon = d.recon;
  a.cmd = l.cmd;
  a.cbp = l.cbp;
  a.coef = l.coef;
  a.cw = S().cw;
  a.ch = S().ch;
  a.mbw = mbw;
  a.mbh = mbh;
  a.qp = opt.qp;
  a.all = j == 0;
  a.i4 = l.i4;
  a.qp_f = d.qp_f;
  a.est_f = d.est_f;
  a.aq_off = d.aq_off;
  a.aq_lo = opt.aq_lo;
  a.aq_hi = opt.aq_hi;
  return a;
}

DeblockArgs Transcoder::deblock_args(int64_t j) const {
  const Level l = level(j);
  DeblockArgs a{};
  a.ent = l.ent;
  a.recon = d.recon;
  a.stride = S().stride;
  a.cmd = l.cmd;
  a.cbp = l.cbp;
  a.coef = l.coef;
  a.cw = S().cw;
  a.ch = S().ch;
  a.mbw = mbw;
  a.mbh = mbh;
  a.qp = opt.qp;
  a.off_a = 2 * opt.dbk_alpha;
  a.off_b = 2 * opt.dbk_beta;
  a.count = d.stats + kStDeblocked;
  a.mv4 = l.mv4;
  a.qp_f = d.qp_f;
  a.aq_off = d.aq_off;
  a.aq_lo = opt.aq_lo;
  a.aq_hi = opt.aq_hi;
  return a;
}

// the level's pictures where the next level reads them: the reconstruction
// slots, or (level 0 without intra: the IDR pictures are their source) the
// small store, through entries whose slot is the frame
HashArgs Transcoder::hash_args(int64_t j) const {
  const bool from_source = j == 0 && !opt.intra;
  return {from_source ? d.hent : level(j).ent, from_source ? S().d : d.recon, S().stride, S().cw, S().ch, S().w, S().h,
          d.stats + kStHash};
}

WriteArgs Transcoder::write_args(int64_t ck) const {
  const Level l = level(chunk_first(ck));  // a chunk is one contiguous run of entries
  WriteArgs a{};
  a.ent = d.went + l.e0;
  a.cmd = l.cmd;
  a.cbp = l.cbp;
  a.coef = d.coef;
  a.coef_per_level = plan.ngop;
  a.ring = static_cast<int32_t>(kRing);
  a.qp = opt.qp;
  a.small = S().d;
  a.stride = S().stride;
  a.cw = S().cw;
  a.ch = S().ch;
  a.mbw = mbw;
  a.mbh = mbh;
  a.staging = d.stage;
  a.cap = cap;
  a.sizes = d.sizes;
  a.stats = d.stats;
  a.err = d.err;
  a.jobs = d.jobs;
  a.n_jobs = d.njobs;
  a.n_slices = static_cast<int32_t>((plan.lvl_off[chunk_end(plan, ck)] - l.e0) * mbh);
  a.dbk_alpha = opt.dbk_alpha;
  a.dbk_beta = opt.dbk_beta;
  a.i4 = l.i4;
  a.mv4 = l.mv4;
  a.qp_f = d.qp_f;
  a.aq_off = d.aq_off;
  a.aq_lo = opt.aq_lo;
  a.aq_hi = opt.aq_hi;
  return a;
}

PackArgs Transcoder::pack_args(int64_t ck) const {
  return {d.went + plan.lvl_off[chunk_first(ck)], d.sizes, d.offs, d.total, d.base, d.fr, d.fr + n, d.stage, cap, d.out,
          d.jobs, d.njobs, S().d, S().stride, S().cw, S().ch, mbh};
}

// Level j on s1: the search (level 0 holds the IDR pictures: none); with
// intra, the level's kPcmCmd macroblocks (level 0: every macroblock) become
// Intra16x16 / I_NxN where cheaper; with deblock, the reconstruction is
// filtered in place (8.7, inside each macroblock row's slice) before it is
// hashed and the next level predicts from it; then the hash and the event.
// Level 0 without intra is all I_PCM (qPav 0, alpha' 0: nothing would be
// filtered): it is not deblocked, and it records no event.
int Transcoder::enqueue_level(int64_t j) {
  const int64_t ne = level(j).ne;
  if (j > 0) launch_enc_search(search_args(j), opt.subpel, opt.rate != 0, opt.partitions != 0, ne, s1);
  if (opt.intra) launch_enc_intra(intra_args(j), opt.intra4x4 != 0, ne, s1);
  if (opt.deblock && (j > 0 || opt.intra)) launch_enc_deblock(deblock_args(j), ne, s1);
  if (opt.hashed) launch_enc_hash(hash_args(j), ne, s1);
  // bitrate_kbps: the GOPs' controllers take this level's measure and set the next level's QPs, in stream order
  if (opt.bitrate_kbps && j + 1 < plan.maxlen) {
    const Level nx = level(j + 1);
    RcArgs r{};
    r.ent = nx.ent;
    r.n_ent = static_cast<int32_t>(nx.ne);
    r.gop_pos = static_cast<int32_t>(j);
    r.qp_f = d.qp_f;
    r.est_f = d.est_f;
    r.spent = d.rc_spent;
    r.gop_len = d.rc_len;
    r.frame_bits = full::erc::frame_budget(opt.bitrate_kbps, delta, c->info.track_timescale);
    r.qp_min = opt.qp_min;
    r.qp_max = opt.qp_max;
    launch_enc_rc(r, s1);
  }
  if (j > 0 || opt.intra) HIP_TRY(hipEventRecord(ev.level_done[j], s1));
  return VTS_OK;
}

// the levels < upto not yet queued; level j reuses the ring slot of level
// j - kRing, whose chunk's slice writing must have finished
int Transcoder::enqueue_searches(int64_t upto) {
  for (; next_search < std::min(plan.maxlen, upto); ++next_search) {
    const int64_t j = next_search;
    if (opt.qp >= 1 && j >= kRing) HIP_TRY(hipStreamWaitEvent(s1, ev.chunk_written[chunk_freeing(j)], 0));
    VTS_TRY(enqueue_level(j));
  }
  if (next_search >= plan.maxlen && !searches_done) {
    HIP_TRY(hipEventRecord(ev.search_end, s1));
    searches_done = true;
  }
  return VTS_OK;
}

// the previous chunk's bytes, once its copy has landed, appended to the file
int Transcoder::drain_pending() {
  if (!pending) return VTS_OK;
  HIP_TRY(hipEventSynchronize(ev.d2h));
  const auto tw = clk::now();
  const size_t ck = host.size() - 1;
  int64_t off = 0;
  const std::string we = mw.append(host[ck].get(), static_cast<size_t>(chunk_start[ck + 1] - chunk_start[ck]), &off);
  if (!we.empty()) return fail(VTS_E_IO, "%s: %s", out_path, we.c_str());
  chunk_file.push_back(off);
  host[ck].reset();
  pending = false;
  mux_ms += ms_since(tw);
  return VTS_OK;
}

// Chunk ck on s2, behind its last level: written, scanned, gathered and
// drained together (wide launches instead of one per level); once its write
// is queued the searches move on to the levels whose ring slots it frees
int Transcoder::write_chunk(int64_t ck) {
  const int64_t j0 = chunk_first(ck), j1 = chunk_end(plan, ck);
  const int64_t ne = plan.lvl_off[j1] - plan.lvl_off[j0];
  if (j1 - 1 > 0 || opt.intra) HIP_TRY(hipStreamWaitEvent(s2, ev.level_done[j1 - 1], 0));  // searches run in level order
  HIP_TRY(hipMemcpyAsync(d.base, d.total, sizeof(int64_t), hipMemcpyDeviceToDevice, s2));
  HIP_TRY(hipMemsetAsync(d.njobs, 0, sizeof(uint32_t), s2));
  launch_enc_write(write_args(ck), opt.cabac != 0, opt.intra, opt.deblock != 0, s2);
  HIP_TRY(hipEventRecord(ev.chunk_written[ck], s2));
  VTS_TRY(enqueue_searches(j1 + kRing));  // the ring slots of this chunk's levels are free once it is written
  launch_enc_pack(pack_args(ck), ne, nmb, s2);
  const hipError_t he = hipGetLastError();
  if (he != hipSuccess) return fail(VTS_E_HIP, "encoder launch: %s", hipGetErrorString(he));
  int64_t tot = 0;
  if (hipMemcpyAsync(&tot, d.total, sizeof tot, hipMemcpyDeviceToHost, s2) != hipSuccess)
    return fail(VTS_E_HIP, "encoder levels %lld.. failed", static_cast<long long>(j0));
  VTS_TRY(drain_pending());  // the previous chunk, while this one runs
  if (hipStreamSynchronize(s2) != hipSuccess)
    return fail(VTS_E_HIP, "encoder levels %lld.. failed", static_cast<long long>(j0));
  const int64_t bytes = tot - chunk_start.back();
  host.emplace_back(new uint8_t[static_cast<size_t>(std::max<int64_t>(bytes, 1))]);
  HIP_TRY(hipMemcpyAsync(host.back().get(), d.out, static_cast<size_t>(bytes), hipMemcpyDeviceToHost, s2));
  HIP_TRY(hipEventRecord(ev.d2h, s2));
  pending = true;
  chunk_start.push_back(tot);
  return VTS_OK;
}

// 4. device encode: level 0, the searches as far ahead as the ring allows,
// then chunk by chunk; both streams are drained when it returns VTS_OK
int Transcoder::encode() {
  HIP_TRY(hipEventRecord(ev.search_begin, s1));
  if (opt.aq_strength_q8)  // the offsets of every frame's macroblocks, ahead of every level in stream order
    launch_enc_aq(AqArgs{S().d, S().stride, S().cw, S().ch, mbw, mbh, opt.aq_strength_q8, opt.aq_max, d.aq_off}, n, s1);
  VTS_TRY(enqueue_level(0));
  VTS_TRY(enqueue_searches(opt.qp >= 1 ? kRing : plan.maxlen));
  HIP_TRY(hipGetLastError());
  const std::string e = mw.open(out_path);
  if (!e.empty()) return fail(VTS_E_IO, "%s: %s", out_path, e.c_str());
  HIP_TRY(hipMemsetAsync(d.total, 0, sizeof(int64_t), s2));
  HIP_TRY(hipEventRecord(ev.write_begin, s2));
  for (int64_t ck = 0; ck < n_chunks(plan); ++ck) VTS_TRY(write_chunk(ck));
  VTS_TRY(drain_pending());
  return VTS_OK;
}

// cmd_out / i4_out / mv_out: entry order -> frame order
int Transcoder::copy_words() {
  const size_t entries = plan.went.size(), per = static_cast<size_t>(nmb);
  if (opt.mv_out) {
    // without partitions a macroblock's vectors follow from its command word;
    // a level the encoder writes no words for, and with partitions every IDR
    // picture (no search ran on it), holds no vector
    std::vector<uint32_t> words(entries * per * (opt.partitions ? 4 : 1));
    HIP_TRY(hipMemcpy(words.data(), opt.partitions ? d.mv4 : d.cmd, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < entries; ++i) {
      uint32_t *o = opt.mv_out + static_cast<int64_t>(plan.went[i].x) * nmb * 4;
      if (plan.went[i].y == 0) {
        std::fill(o, o + 4 * per, kPcmCmdWord);
      } else if (opt.partitions) {
        std::memcpy(o, words.data() + i * per * 4, per * 4 * sizeof(uint32_t));
      } else {
        for (size_t m = 0; m < per; ++m) {
          const uint32_t w = words[i * per + m];
          std::fill(o + 4 * m, o + 4 * m + 4, (w >> 16) == 0x8000u ? kPcmCmdWord : w);  // I_PCM and the intra words
        }
      }
    }
  }
  if (opt.cmd_out) {  // a level the encoder writes no words for (the I_PCM IDR pictures) is I_PCM
    std::vector<uint32_t> words(entries * per);
    HIP_TRY(hipMemcpy(words.data(), d.cmd, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < entries; ++i) {
      uint32_t *o = opt.cmd_out + static_cast<int64_t>(plan.went[i].x) * nmb;
      if (plan.went[i].y == 0 && !opt.intra) std::fill(o, o + nmb, kPcmCmdWord);
      else std::memcpy(o, words.data() + i * per, per * sizeof(uint32_t));
    }
  }
  if (opt.i4_out) {  // as cmd_out; without intra4x4 no macroblock is I_NxN
    std::fill(opt.i4_out, opt.i4_out + cmd_words, kNoI4Modes);
    if (opt.intra4x4) {
      std::vector<uint64_t> words(entries * per);
      HIP_TRY(hipMemcpy(words.data(), d.i4, words.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
      for (size_t i = 0; i < entries; ++i)
        std::memcpy(opt.i4_out + static_cast<int64_t>(plan.went[i].x) * nmb, words.data() + i * per,
                    per * sizeof(uint64_t));
    }
  }
  return VTS_OK;
}

// 5. the frames' offsets back, both streams drained, the counters read once;
// the MP4 sample table (display order) over the mdat written by the chunks;
// the report
int Transcoder::finish(vts_transcode_info *info, vts_transcode_ext_info *xinfo) {
  std::vector<int64_t> fr(static_cast<size_t>(2 * n), 0);
  HIP_TRY(hipMemcpyAsync(fr.data(), d.fr, sizeof(int64_t) * 2 * n, hipMemcpyDeviceToHost, s2));
  HIP_TRY(hipEventRecord(ev.write_end, s2));
  if (hipStreamSynchronize(s2) != hipSuccess || hipStreamSynchronize(s1) != hipSuccess)
    return fail(VTS_E_HIP, "encoder failed");
  float a_ms = 0, b_ms = 0;
  (void)hipEventElapsedTime(&a_ms, ev.search_begin, ev.search_end);
  (void)hipEventElapsedTime(&b_ms, ev.write_begin, ev.write_end);
  ms[1] = a_ms;
  ms[2] = b_ms;
  uint32_t err = 0;
  unsigned long long st[kStCount] = {};
  HIP_TRY(hipMemcpy(&err, d.err, sizeof err, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(st, d.stats, sizeof st, hipMemcpyDeviceToHost));
  if (err) return fail(VTS_E_CAPACITY, "a slice exceeded its %lld-byte staging slot", static_cast<long long>(cap));
  VTS_TRY(copy_words());
  // the QP and the measure of every frame: the device's with a per-picture QP, else the call's QP and no measure
  std::vector<uint8_t> qps(static_cast<size_t>(n), static_cast<uint8_t>(opt.qp));
  std::vector<uint32_t> est(static_cast<size_t>(n), 0);
  if (opt.per_frame) {
    HIP_TRY(hipMemcpy(qps.data(), d.qp_f, qps.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(est.data(), d.est_f, est.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  if (opt.qp_out) std::copy(qps.begin(), qps.end(), opt.qp_out);
  if (opt.bits_out) std::copy(est.begin(), est.end(), opt.bits_out);
  int64_t qp_sum = 0, est_bits = 0;
  for (int64_t f = 0; f < n; ++f) {
    qp_sum += qps[f];
    est_bits += est[f];
  }
  VTS_XINFO_PUT(vts_transcode_ext_info6, qp_sum, qp_sum);
  VTS_XINFO_PUT(vts_transcode_ext_info6, qp_lo, n ? *std::min_element(qps.begin(), qps.end()) : 0);
  VTS_XINFO_PUT(vts_transcode_ext_info6, qp_hi, n ? *std::max_element(qps.begin(), qps.end()) : 0);
  VTS_XINFO_PUT(vts_transcode_ext_info6, est_bits, est_bits);
  // the QP of every macroblock: its picture's, moved by its offset (aq off and no mbqp_out: the facts stay 0)
  if (opt.aq_strength_q8 || opt.mbqp_out) {
    std::vector<int8_t> off(static_cast<size_t>(cmd_words), 0);
    if (opt.aq_strength_q8) HIP_TRY(hipMemcpy(off.data(), d.aq_off, off.size(), hipMemcpyDeviceToHost));
    int lo = 0, hi = 0;
    int64_t moved = 0;
    for (int64_t i = 0; i < cmd_words; ++i) {
      lo = std::min<int>(lo, off[i]);
      hi = std::max<int>(hi, off[i]);
      moved += off[i] != 0;
      if (opt.mbqp_out)
        opt.mbqp_out[i] = static_cast<uint8_t>(
            opt.aq_strength_q8 ? full::eaq::qp_mb(qps[i / nmb], off[i], opt.aq_lo, opt.aq_hi) : qps[i / nmb]);
    }
    VTS_XINFO_PUT(vts_transcode_ext_info8, aq_lo, lo);
    VTS_XINFO_PUT(vts_transcode_ext_info8, aq_hi, hi);
    VTS_XINFO_PUT(vts_transcode_ext_info8, aq_mbs, moved);
  } else {
    VTS_XINFO_PUT(vts_transcode_ext_info8, aq_lo, 0);
    VTS_XINFO_PUT(vts_transcode_ext_info8, aq_hi, 0);
    VTS_XINFO_PUT(vts_transcode_ext_info8, aq_mbs, int64_t(0));
  }

  const auto t0 = clk::now();
  std::vector<uint8_t> sps, pps;
  const double fps = static_cast<double>(c->info.track_timescale) / static_cast<double>(delta);
  make_sps_pps(mbw, mbh, S().cw - S().w, S().ch - S().h, h264_pick_level(nmb, nmb * fps), &sps, &pps, 0, opt.cabac != 0);
  std::vector<uint8_t> is_idr(static_cast<size_t>(n), 0);
  for (int64_t f : plan.gop_start) is_idr[f] = 1;
  std::string e;
  for (int64_t f = 0; f < n && e.empty(); ++f) {
    const int64_t off = fr[f], size = fr[n + f];
    const size_t ci = static_cast<size_t>(std::upper_bound(chunk_start.begin(), chunk_start.end(), off) -
                                          chunk_start.begin()) - 1;
    if (ci >= chunk_file.size() || off + size > chunk_start[ci + 1])
      return fail(VTS_E_HIP, "frame %lld: output bookkeeping mismatch", static_cast<long long>(f));
    e = mw.add_sample_at(chunk_file[ci] + (off - chunk_start[ci]), static_cast<size_t>(size), is_idr[f] != 0);
  }
  if (e.empty()) e = mw.finish(S().w, S().h, c->info.track_timescale, delta, sps, pps);
  if (!e.empty()) return fail(VTS_E_IO, "%s: %s", out_path, e.c_str());
  ms[3] = mux_ms + ms_since(t0);

  // a counter whose option is off is reported as 0 whatever its slot holds
  if (info) {
    std::memset(info, 0, sizeof *info);
    info->width = S().w;
    info->height = S().h;
    info->n_frames = n;
    info->n_idr = plan.ngop;
    info->pcm_mbs = static_cast<int64_t>(st[kStPcm]);
    info->inter_mbs = static_cast<int64_t>(st[kStInter]);
    info->skip_mbs = static_cast<int64_t>(st[kStSkip]);
    info->intra_mbs = static_cast<int64_t>(st[kStIntra]);
    info->recon_hash = opt.hashed ? st[kStHash] : 0;
    info->bytes_written = mw.bytes_written();
    for (int i = 0; i < 4; ++i) info->ms[i] = ms[i];
  }
  const auto on = [](int flag, unsigned long long v) { return flag ? static_cast<int64_t>(v) : 0; };
  VTS_XINFO_PUT(vts_transcode_ext_info, subpel_mbs, on(opt.subpel, st[kStHalf] + st[kStQuarter]));
  VTS_XINFO_PUT(vts_transcode_ext_info, qpel_mbs, on(opt.subpel, st[kStQuarter]));
  VTS_XINFO_PUT(vts_transcode_ext_info2, deblock_mbs, on(opt.deblock, st[kStDeblocked]));
  VTS_XINFO_PUT(vts_transcode_ext_info3, early_skip_mbs, on(opt.early_skip, st[kStEarlySkip]));
  VTS_XINFO_PUT(vts_transcode_ext_info4, intra4x4_mbs, on(opt.intra4x4, st[kStI4]));
  VTS_XINFO_PUT(vts_transcode_ext_info5, p16x8_mbs, on(opt.partitions, st[kStP16x8]));
  VTS_XINFO_PUT(vts_transcode_ext_info5, p8x16_mbs, on(opt.partitions, st[kStP8x16]));
  VTS_XINFO_PUT(vts_transcode_ext_info5, p8x8_mbs, on(opt.partitions, st[kStP8x8]));
  return VTS_OK;
}

}  // namespace
}  // namespace vts

using namespace vts;

extern "C" int vts_transcode(vts_ctx *c, const char *out_path, const vts_transcode_params *pin,
                             vts_transcode_info *info) {
  return vts_transcode_ex(c, out_path, pin, nullptr, info, nullptr);
}

extern "C" int vts_transcode_ex(vts_ctx *c, const char *out_path, const vts_transcode_params *pin,
                                const vts_transcode_ext *ext, vts_transcode_info *info,
                                vts_transcode_ext_info *xinfo) {
  clear_error();
  if (!c || !out_path) return fail(VTS_E_INVALID, "NULL argument");
  Transcoder t(c, out_path);
  VTS_TRY(read_opts(c, pin, ext, xinfo, &t.opt));
  VTS_TRY(t.check(xinfo));
  VTS_TRY(t.decode());
  // the range's own scores: frame t.f0 + i is frame i of the plan and of everything after it
  const std::vector<float> scores(c->host_scores.begin() + t.f0, c->host_scores.begin() + t.f0 + t.n);
  t.plan = plan_gops(t.n, scores, t.opt.keyint, t.opt.idr_at_cuts, t.opt.thr, t.opt.intra, t.opt.rate);
  VTS_TRY(t.alloc());
  VTS_TRY(t.encode());
  return t.finish(info, xinfo);
}
