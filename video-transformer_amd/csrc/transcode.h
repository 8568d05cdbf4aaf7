// transcode.h — what the device encoder's kernels (transcode.hip) and its host
// driver (transcode_driver.cpp) share: the kernels' argument structs, the
// counters, and one launch function per stage.  DESIGN.md §11.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vts {

constexpr int kMaxRange = 16;    // search_range
constexpr int kCoefPerMb = 384;  // luma 16 x 16 by luma4x4BlkIdx, Cb / Cr DC 2 x 4, Cb / Cr AC 8 x 15 (scan order)

// The encoder's counters, one array of kStCount that kernels add into and the
// driver reads back once; the driver zeroes all of it before anything is queued.
enum StatSlot : int {
  kStPcm,        // enc_write / enc_write_cabac: I_PCM macroblocks
  kStInter,      // ... coded inter
  kStSkip,       // ... P_Skip
  kStIntra,      // ... Intra16x16 and I_NxN
  kStHash,       // enc_hash: the reconstruction hash
  kStHalf,       // enc_search<., SP > 0>: inter macroblocks with a fractional vector, no odd component
  kStQuarter,    // ... with an odd component
  kStDeblocked,  // enc_deblock: macroblocks with a filtered line
  kStEarlySkip,  // enc_search<., ., true>: macroblocks the early P_Skip probe decided
  kStI4,         // the writers: I_NxN macroblocks
  kStP16x8,      // the writers: inter macroblocks coded as P_L0_L0_16x8 (partitions)
  kStP8x16,      // ... as P_L0_L0_8x16
  kStP8x8,       // ... as P_8x8
  kStCount
};

// ------------------------------------------------------ motion search
struct SearchArgs {
  const int4 *ent;      // per frame of the level: (frame, ref slot or -1 = small[frame-1], dst slot, 0)
  const uint8_t *small;
  int64_t stride;
  uint8_t *recon;       // [slot]
  uint32_t *cmd;        // [entry][mb]
  uint8_t *cbp;         // [entry][mb] coded_block_pattern (residual coding)
  int16_t *coef;        // [entry][mb][kCoefPerMb] levels (this level's ring slot)
  int32_t cw, ch, mbw, nmb;
  int32_t range, max_sad;
  int32_t qp, rate;     // qp >= 1: residual coding at that QP; RC: bit 0 mvcost, bit 1 early_skip (enc_rate.h)
  unsigned long long *sp_stats;  // SP > 0: inter macroblocks with a fractional vector: [0] no odd component, [1] one
  // RC only
  const uint32_t *cmd_prev;      // the previous level's final words [entry][mb]; ent[e].w = the GOP's entry there
  int32_t gop_pos, lambda16;     // the level's GOP position j; lambda16 of the vector cost
  unsigned long long *es_stat;   // macroblocks the early P_Skip probe decided
  // PT only (enc_part.h)
  uint32_t *mv4;                 // [entry][mb][4] the quadrant vectors, kNoMv four times where not inter
  const uint32_t *mv4_prev;      // the previous level's, as cmd_prev
  // RC only (vts_transcode_ext7; NULL: off, and qp / lambda16 above hold)
  const uint8_t *qp_f;           // [frame] the QP of each picture: read in place of qp, lambda16 follows it
  uint32_t *est_f;               // [frame] the rate measure, bits: the final decisions of this kernel add into it
  int32_t mv_lambda16;           // qp_f: the caller's lambda16 (> 0 replaces the table's at every QP)
  int32_t pcm_bits;              // est_f: what a macroblock left as I_PCM adds (0 with intra: enc_intra decides it)
  // RC only (vts_transcode_ext9, enc_aq.h; NULL: off)
  const int8_t *aq_off;          // [frame][mb] the macroblock's QP offset: it is coded at clamp(QP + offset, aq_lo, aq_hi)
  int32_t aq_lo, aq_hi;
};

// ------------------------------------------------------ slice writer
struct WriteArgs {
  const int4 *ent;      // per frame of the level: (frame, GOP position j, IDR parity, index within its level)
  const uint32_t *cmd;  // [entry][mb] (P levels; with intra every level)
  const uint8_t *cbp;   // [entry][mb] coded_block_pattern
  const int16_t *coef;  // level ring: [ring slot][index within level][mb][kCoefPerMb]
  int64_t coef_per_level;  // entries a ring slot holds
  int32_t ring, qp;     // ring slots (levels); qp >= 1: residual coding (slice_qp_delta = qp - 26)
  const uint8_t *small;
  int64_t stride;
  int32_t cw, ch, mbw, mbh;
  uint8_t *staging;     // [slice][cap]
  int64_t cap;
  int32_t *sizes;       // [slice] bytes incl. the 4-byte length prefix
  unsigned long long *stats;  // [kStCount]: the writers add into kStPcm .. kStIntra and kStI4
  uint32_t *err;
  uint4 *jobs;          // I_PCM payloads left for enc_pcm: (slice, byte offset in the slot, mx, 0)
  uint32_t *n_jobs;
  int32_t n_slices;
  int32_t dbk_alpha, dbk_beta, _pad;  // enc_write<., true>: slice_alpha_c0_offset_div2, slice_beta_offset_div2
  const uint64_t *i4;   // [entry][mb] the Intra4x4PredModes of the I_NxN macroblocks (intra4x4; else unread)
  const uint32_t *mv4;  // [entry][mb][4] the quadrant vectors (partitions; else NULL and unread)
  const uint8_t *qp_f;  // [frame] NULL, or the QP of each picture in place of qp (vts_transcode_ext7)
  const int8_t *aq_off; // [frame][mb] NULL, or the macroblocks' QP offsets (vts_transcode_ext9): mb_qp_delta is written
  int32_t aq_lo, aq_hi; // ... a macroblock's QP is clamp(QP + offset, aq_lo, aq_hi)
};

// ------------------------------------------------------ intra coding
struct IntraArgs {
  const int4 *ent;      // the level's search entries: (frame, -, dst slot, 0)
  const uint8_t *small;
  int64_t stride;
  uint8_t *recon;       // [slot]
  uint32_t *cmd;        // [entry][mb]
  uint8_t *cbp;         // [entry][mb]
  int16_t *coef;        // [entry][mb][kCoefPerMb] (this level's ring slot)
  int32_t cw, ch, mbw, mbh;
  int32_t qp;
  int32_t all;          // 1: every macroblock is a candidate and dst is unwritten (level 0, the IDR
                        // pictures); 0: the macroblocks enc_search left as kPcmCmd (dst holds the source)
  uint64_t *i4;         // enc_intra<true>: [entry][mb] the Intra4x4PredModes of an I_NxN macroblock, else ~0
  const uint8_t *qp_f;  // [frame] NULL, or the QP of each picture in place of qp (vts_transcode_ext7)
  uint32_t *est_f;      // [frame] NULL, or the rate measure: the bits of the macroblocks decided here are added
  const int8_t *aq_off; // [frame][mb] NULL, or the macroblocks' QP offsets (vts_transcode_ext9)
  int32_t aq_lo, aq_hi; // ... a macroblock's QP is clamp(QP + offset, aq_lo, aq_hi)
};

// ------------------------------------------------------ in-loop deblocking
struct DeblockArgs {
  const int4 *ent;      // the level's search entries: (frame, -, dst slot, 0)
  uint8_t *recon;       // [slot]
  int64_t stride;
  const uint32_t *cmd;  // [entry][mb]
  const uint8_t *cbp;   // [entry][mb]
  const int16_t *coef;  // [entry][mb][kCoefPerMb] (this level's ring slot)
  int32_t cw, ch, mbw, mbh;
  int32_t qp, off_a, off_b, _pad;  // SliceQPY, FilterOffsetA, FilterOffsetB
  unsigned long long *count;       // macroblocks with a filtered line
  const uint32_t *mv4;             // [entry][mb][4] the quadrant vectors (partitions; else NULL and unread)
  const uint8_t *qp_f;             // [frame] NULL, or the SliceQPY of each picture in place of qp (vts_transcode_ext7)
  const int8_t *aq_off;            // [frame][mb] NULL, or the macroblocks' QP offsets (vts_transcode_ext9): an edge's
  int32_t aq_lo, aq_hi;            // indices come from the QP_Y of the macroblocks on its two sides
};

// ------------------------------------------------------ adaptive quantisation
// enc_aq (enc_aq.h) once per call, ahead of level 0: the offset of every
// macroblock of every frame from the encoder's input pictures
struct AqArgs {
  const uint8_t *small;  // [frame] the encoder's input pictures (NV12, cw x ch)
  int64_t stride;
  int32_t cw, ch, mbw, mbh;
  int32_t strength_q8, aq_max;
  int8_t *aq_off;        // [frame][mb]
};

// ------------------------------------------------------ rate control
// enc_rc (enc_ratectl.h) behind level j, one thread per entry of level j + 1:
// the GOP's running sum takes picture j's measure, the next picture's QP is set
struct RcArgs {
  const int4 *ent;         // level j + 1's search entries: (frame, -, dst slot = 2 GOP + parity, -)
  int32_t n_ent, gop_pos;  // its entries; j, the position of the pictures just coded
  uint8_t *qp_f;           // [frame]
  const uint32_t *est_f;   // [frame]
  int64_t *spent;          // [GOP] the measure of the GOP's pictures so far
  const int32_t *gop_len;  // [GOP] its pictures
  int64_t frame_bits;      // B (enc_ratectl.h frame_budget)
  int32_t qp_min, qp_max;
};

// ------------------------------------------------------ host-side only
// enc_hash over `entries` pictures: picture e is pics + ent[e].z * stride
struct HashArgs {
  const int4 *ent;
  const uint8_t *pics;
  int64_t stride;
  int32_t cw, ch, w, h;       // coded and display size
  unsigned long long *acc;
};
// enc_scan, enc_gather and enc_pcm over a chunk whose slices enc_write left in
// the staging slots: offsets, the packed output, the I_PCM payloads
struct PackArgs {
  const int4 *ent;            // the chunk's write entries
  const int32_t *sizes;       // [slice]
  int64_t *offs;              // [slice] absolute output offset
  int64_t *total;             // running output total, advanced
  const int64_t *base;        // the total before this chunk: d_out starts there
  int64_t *fr_off, *fr_size;  // [frame]
  const uint8_t *staging;
  int64_t cap;
  uint8_t *out;
  const uint4 *jobs;
  const uint32_t *n_jobs;
  const uint8_t *small;
  int64_t stride;
  int32_t cw, ch, mbh;
};

// One launch function per stage, each holding its kernel's template dispatch.
// They only queue (errors surface in hipGetLastError, as with a bare launch).
// entries: the level's (chunk's) entries; a stage's grid follows from it.
void launch_enc_search(const SearchArgs &a, int subpel, bool rate_aware, bool partitions, int64_t entries, hipStream_t s);
void launch_enc_intra(const IntraArgs &a, bool intra4x4, int64_t entries, hipStream_t s);
void launch_enc_deblock(const DeblockArgs &a, int64_t entries, hipStream_t s);
void launch_enc_rc(const RcArgs &a, hipStream_t s);
void launch_enc_aq(const AqArgs &a, int64_t frames, hipStream_t s);
void launch_enc_hash(const HashArgs &a, int64_t entries, hipStream_t s);
void launch_enc_write(const WriteArgs &a, bool cabac, bool intra, bool deblock, hipStream_t s);  // a.n_slices slices
void launch_enc_pack(const PackArgs &a, int64_t entries, int32_t nmb, hipStream_t s);

// What the driver needs of the kernels' headers without reading them
// (transcode.hip asserts the two words against those headers)
constexpr uint32_t kPcmCmdWord = 0x80008000u;  // the command word of an I_PCM macroblock (enc_deblock.h kPcmCmd)
constexpr uint64_t kNoI4Modes = ~0ull;         // the mode word of a macroblock that is not I_NxN (enc_intra4.h kNoModes)
constexpr int32_t kPcmMbBits = 3072;           // the rate measure of an I_PCM macroblock: its payload (kPcmBits)
int64_t slice_slot_bytes(int mbw, bool cabac, bool aq = false);  // staging slot of one slice (a macroblock row)
int32_t search_lambda16(int qp, int mv_lambda16);  // SearchArgs.lambda16 (enc_rate.h lambda16)

}  // namespace vts
