/*
 * vtseg.h — C ABI of libvtseg.so, the MI355X-native long-video segmenter.
 *
 * This is the drop-in boundary for the reference's segmenter hot path
 * (shizhenneko/Video-Transformer).  The reference is pure Python and reaches
 * ffprobe/ffmpeg through subprocess; the build keeps the Python call sites
 * (package `vtseg`, same function names and signatures as the reference
 * modules) and puts everything below them behind this header: plain C types,
 * caller-allocated buffers, int status codes, a thread-local error string.
 * No exception crosses the ABI.  ctypes releases the GIL around every call.
 *
 * Entry point → reference interface it replaces:
 *   vts_plan_segments      utils/video_segmenter.py:42-83   plan_segments
 *   vts_plan_with_budget   utils/budget_planner.py:73-194   plan_segments_with_budget
 *   vts_manifest_json      utils/video_segmenter.py:170-218 create_manifest + save_manifest text
 *   vts_probe_duration     utils/video_utils.py:7-38        probe_duration (ffprobe format=duration)
 *   vts_probe_info         utils/video_utils.py:7-38        (same probe, all stream facts)
 *   vts_extract_segment    utils/video_segmenter.py:86-154  extract_segment (ffmpeg -c copy)
 *   vts_add_tracks         analyzer/content_analyzer.py:206-209 (audio kept in the upload copy)
 *   vts_add_tracks_range   utils/video_segmenter.py:86-154  extract_segment (the re-encode branch's
 *                          audio, beside a vts_transcode_ex of a frame range; a stream copy)
 *   vts_boundary_frames*   (no reference code; video_segmenter.py:157-159 snap_to_keyframe
 *                          is the identity stub this feeds)  segment time -> frame index
 *   vts_open/vts_score/... (no reference code; north_star)   decode + NV12 scene scoring
 *   vts_score_nv12_dev     (no reference code)               the scoring kernel on device NV12
 *   vts_batch_run          pipeline.py:376-393 (the batch loop over analyze_video), as
 *                          vtseg.batch.plan_batch: video i on rank i % world, RCCL exchange
 *   vts_synth_write        (no reference code; tests/test_video_segmenter.py:147-178 builds
 *                          its only synthetic clip with `ffmpeg -f lavfi`, absent here)
 *
 * Status codes: 0 = ok, < 0 = error (see VTS_E_*); vts_last_error() gives a
 * message for the calling thread's last failure.
 */
#ifndef VTSEG_H
#define VTSEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VTS_ABI_VERSION 9

enum {
  VTS_OK = 0,
  VTS_E_INVALID = -1,        /* bad argument (NULL pointer, bad geometry ...)        */
  VTS_E_CAPACITY = -2,       /* output too small; *n_out holds the size needed       */
  VTS_E_NONTERMINATING = -3, /* the reference loop would never end on this input     */
  VTS_E_RANGE = -4,          /* integer result outside int64 (Python would use bigint) */
  VTS_E_VALUE = -5,          /* Python ValueError (e.g. math.ceil(nan))              */
  VTS_E_OVERFLOW = -6,       /* Python OverflowError (e.g. math.ceil(inf))           */
  VTS_E_IO = -7,             /* file cannot be opened / read / written               */
  VTS_E_FORMAT = -8,         /* container or bitstream not understood                */
  VTS_E_UNSUPPORTED = -9,    /* valid H.264 outside the decoder's supported subset   */
  VTS_E_HIP = -10,           /* HIP runtime error                                    */
  VTS_E_NODEVICE = -11,      /* no usable gfx950 device                              */
  VTS_E_DECODE = -12,        /* bitstream error found by the device-side parser      */
  VTS_E_ZERODIV = -13        /* Python ZeroDivisionError (max_continuations == -1)   */
};

/* ---------------------------------------------------------------- planning */

/* One planned window (reference SegmentInfo, video_segmenter.py:12-18). */
typedef struct vts_segment {
  int64_t segment_id;
  double start;            /* extract window start (core start - overlap)  */
  double end;              /* extract window end   (core end + overlap)    */
  double effective_start;  /* core start                                   */
  double effective_end;    /* core end                                     */
  int64_t flags;           /* bit0: `end` is the duration argument itself,
                              bit1: `effective_end` is the duration argument
                              (lets the host mirror return the caller's int
                              object where the reference does)             */
} vts_segment;

/* plan_segments (video_segmenter.py:42-83), bit-exact double arithmetic in
 * the reference's operation order.  Two-call size query: with out == NULL or
 * cap too small returns VTS_E_CAPACITY and sets *n_out to the count needed.
 * Returns VTS_E_NONTERMINATING where the reference `while` never ends
 * (cursor + segment_seconds == cursor, or duration = +inf). */
int vts_plan_segments(double duration, double segment_seconds,
                      double overlap_seconds, vts_segment *out, int64_t cap,
                      int64_t *n_out);

/* Sync-sample (keyframe) presentation timestamps of the first video track,
 * in *timescale units (edit-list shift applied); anchors for the opt-in
 * keyframe-aware snap_to_keyframe (video_segmenter.py:157-159 stays the
 * identity by default).  Two-call size query. */
int vts_keyframe_pts(const char *path, int64_t *pts, int64_t cap, int64_t *n_out,
                     int64_t *timescale);

/* Manifest JSON (create_manifest + save_manifest, video_segmenter.py:170-218):
 * the text json.dumps(manifest, indent=2, ensure_ascii=True) writes, with the
 * plan from vts_plan_segments.  *_int: the caller's int object's decimal repr
 * (Python ints print as ints: SegmentPlan fields, an int duration), NULL for a
 * float.  segment_dir: str(get_segment_dir(...)) (pathlib-normalised).
 * Two-call size query like vts_plan_segments; VTS_E_INVALID for non-UTF-8. */
typedef struct vts_manifest_args {
  const char *video_id;
  const char *segment_dir;
  const char *created_at;
  double duration;
  const char *duration_int;
  double segment_seconds;
  const char *segment_seconds_int;
  double overlap_seconds;
  const char *overlap_seconds_int;
} vts_manifest_args;

int vts_manifest_json(const vts_manifest_args *args, char *out, int64_t cap, int64_t *len);

/* Budget-planner inputs after the reference's _coerce_int/_coerce_bool and
 * float(threshold) (budget_planner.py:20-40, 95-103); the host mirror does the
 * Python-object coercion and passes plain numbers here. */
typedef struct vts_budget_cfg {
  int64_t default_segment_seconds; /* long_video.default_segment_seconds (480) */
  int64_t overlap_seconds;         /* long_video.overlap_seconds (20)          */
  int64_t min_segment_seconds;     /* long_video.min_segment_seconds (90)      */
  int64_t hard_max_api_calls;      /* long_video.hard_max_api_calls (50)       */
  int64_t max_continuations;       /* analyzer.max_continuations (3)           */
  int64_t retry_times;             /* analyzer.retry_times (0)                 */
  int32_t has_threshold;           /* duration_threshold_seconds parsed?       */
  int32_t consolidate;             /* long_video.consolidate (True)            */
  double duration_threshold_seconds;
} vts_budget_cfg;

/* Reference SegmentPlan (budget_planner.py:9-17). */
typedef struct vts_plan {
  int64_t segment_duration;
  int64_t overlap;
  int64_t num_segments;
  int64_t estimated_calls;
  int64_t available_calls;
  int64_t hard_max_calls;
  int32_t fits_budget;
  int32_t _pad;
} vts_plan;

/* plan_segments_with_budget (budget_planner.py:73-194).  `duration` is the
 * reference's float(duration).  VTS_E_VALUE / VTS_E_OVERFLOW where the
 * reference raises ValueError / OverflowError (NaN / inf durations). */
int vts_plan_with_budget(double duration, const vts_budget_cfg *cfg,
                         int64_t current_api_count, vts_plan *out);

/* Segment time -> frame index.  For each t in times[0..ntimes): the index of
 * the first frame (presentation order) whose pts satisfies
 * pts / timescale >= t, compared exactly in integer arithmetic (no rounding);
 * n_frames when no frame qualifies.  pts must be sorted ascending. */
int vts_boundary_frames_pts(const int64_t *pts, int64_t n_frames,
                            int64_t timescale, const double *times,
                            int64_t ntimes, int64_t *frame_idx);

/* ---------------------------------------------------------------- probing */

typedef struct vts_video_info {
  double duration;            /* == vts_probe_duration                       */
  int64_t duration_us;        /* av_rescale(mvhd.duration, 1e6, mvhd.timescale) */
  int64_t movie_timescale;    /* mvhd                                        */
  int64_t movie_duration;     /* mvhd (movie timescale units)                */
  int64_t track_timescale;    /* mdhd of the first video track               */
  int64_t n_frames;           /* samples of the first video track            */
  int64_t n_sync;             /* stss entries (0 = every sample is sync)     */
  int32_t width, height;      /* display size (SPS crop applied)             */
  int32_t coded_width, coded_height; /* macroblock-aligned size             */
  int32_t profile_idc, level_idc;
  int32_t codec;              /* 1 = H.264/avc1, 0 = other                   */
  int32_t _pad;
} vts_video_info;

/* probe_duration (video_utils.py:7-38).  Parses the ISO-BMFF `moov` box: the
 * value is the one ffprobe prints for `format=duration` on a non-fragmented
 * MP4, (double)av_rescale(mvhd.duration, 1000000, mvhd.timescale) / 1e6.
 * Never fails: returns VTS_OK with *seconds = 0.0 on any error, exactly like
 * the reference (the reason is still available from vts_last_error()). */
int vts_probe_duration(const char *path, double *seconds);

/* All container facts of the first video track. Returns < 0 on error. */
int vts_probe_info(const char *path, vts_video_info *info);

/* extract_segment stream copy (video_segmenter.py:86-154, the `-c copy`
 * branch) for ISO-BMFF input: every track from the sync sample at or before
 * `start` to the last sample presented before `end`, an edit list starting
 * presentation at `start`, moov before mdat (+faststart).  0 = ok. */
int vts_extract_segment(const char *in_path, double start, double end,
                        const char *out_path);

/* Every track of video_path plus every non-video track (audio, subtitles,
 * ...) of src_path, whole and stream-copied, into out_path (moov first).  The
 * upload transcode keeps the source's audio with it, as the reference keeps
 * audio (content_analyzer.py:206-209, -c:a aac -b:a 64k; here a stream copy). */
int vts_add_tracks(const char *video_path, const char *src_path, const char *out_path);

/* As vts_add_tracks, with every non-video track of src_path cut to
 * [start, end) by vts_extract_segment's rule: samples from the sync sample at
 * or before `start` to the last one presented before `end`, an edit list that
 * begins presentation at `start`.  Every track of video_path is copied whole
 * (the device re-encode of the same span: its file starts at its first
 * frame); a track of src_path with nothing in range is dropped; moov first.
 * VTS_E_INVALID when end - start <= 0. */
int vts_add_tracks_range(const char *video_path, const char *src_path, double start,
                         double end, const char *out_path);

/* ------------------------------------------------- device scoring kernel */

/* Per-frame scene scoring of NV12 frames already in device memory.
 *   thumbnail (w,h) = (width/k, height/k)   (k even, divides width and height)
 *   Y'  = box mean of the k x k luma block,        (sum + k*k/2) / (k*k)
 *   U',V' = box mean of the (k/2)x(k/2) chroma block, rounded the same way
 *   RGB = BT.709 limited-range 8-bit fixed point of (Y',U',V')
 *   hist[256]  = histogram of Y' over the thumbnail (uint32)
 *   sad        = sum |Y'_t - Y'_{t-1}| over the thumbnail (uint64; 0 for the
 *                first frame when prev_luma == NULL)
 *   score      = (float)(sad / (w * h * 255.0))
 * Frame i's Y plane starts at nv12 + i*frame_stride, its interleaved UV plane
 * at + pitch*uv_row_offset.  Outputs are device pointers; any may be NULL
 * except sad/score.  prev_luma (w*h bytes, device) seeds frame 0's SAD and
 * last_luma (w*h bytes, device, may be NULL) receives the last frame's Y'.
 * Any width that k divides is scored; widths that are multiples of 16 (k = 6:
 * of 48) take the fast kernels, others (cropped pictures such as 202 x 360)
 * per-pixel kernels with the same results and a workspace of one thumbnail per
 * frame (vts_score_workspace_bytes accounts for it). */
typedef struct vts_score_desc {
  const uint8_t *nv12;       /* device                                      */
  int64_t frame_stride;      /* bytes between frames                        */
  int64_t n_frames;
  int32_t width, height;     /* luma size scored (display size)             */
  int32_t pitch;             /* bytes per row, Y and UV                     */
  int32_t uv_row_offset;     /* UV plane = Y + pitch*uv_row_offset          */
  int32_t k;                 /* downscale factor: 2, 4, 6 or 8              */
  int32_t _pad;
  uint8_t *rgb;              /* n_frames * w*h*3, RGB interleaved           */
  uint32_t *hist;            /* n_frames * 256                              */
  uint64_t *sad;             /* n_frames                                    */
  float *score;              /* n_frames                                    */
  const uint8_t *prev_luma;  /* w*h or NULL                                 */
  uint8_t *last_luma;        /* w*h or NULL                                 */
  uint8_t *workspace;        /* device scratch, vts_score_workspace_bytes() */
  int64_t workspace_bytes;
} vts_score_desc;

int64_t vts_score_workspace_bytes(int32_t width, int32_t height, int32_t k,
                                  int64_t n_frames);
/* Enqueue on `hip_stream` (a hipStream_t, NULL = default stream). */
int vts_score_nv12_dev(const vts_score_desc *desc, void *hip_stream);

/* --------------------------------------------- session: decode + score */

typedef struct vts_ctx vts_ctx;

typedef struct vts_params {
  int32_t k;               /* thumbnail downscale; 0 = auto (4 for <=720p, 6 above) */
  int32_t window_frames;   /* decoded-surface ring size in frames; 0 = auto        */
  int32_t keep_rgb;        /* reserved (RGB thumbnails of every frame are kept)    */
  int32_t n_streams;       /* 1 or 2 (2 = decode/score overlap on two HIP streams) */
  float cut_threshold;     /* scene-cut threshold on score (default 0.08 when <=0) */
  int32_t fused;           /* 0 auto, 1 require, -1 never: fuse scoring into
                              reconstruction (k in {2,4,8}, no cropping)       */
  int32_t gops_per_launch; /* GOPs decoded together per reconstruct launch;
                              <= 0 = all GOPs of the window (fastest measured) */
  int32_t parse_chunks;    /* slice parsing on its own stream in N chunks of
                              launches, chunk j+1 overlapping reconstruction of
                              chunk j; <= 1 (default) = one parse launch */
  int32_t level_block;     /* GOP levels decoded per reconstruct launch (k = 4,
                              fused, GOPs that are plain P chains): 0 (auto) =
                              P levels two per launch, the first of a pair
                              handed on in LDS and not stored (DESIGN.md §4.7;
                              no kept frames, no transcode, default launch
                              grouping, pictures up to 1360 wide), else one
                              launch per level; 1 = one launch per level;
                              n >= 2 = up to n levels per launch with the
                              levels between in LDS */
  int32_t keep_frames;     /* level-blocked launches keep only each block's
                              last frame in HBM (the next block's reference),
                              and the general decoder recycles a picture's
                              surface once it is scored and no longer
                              referenced; 1 = store every decoded frame
                              (vts_get_frame_nv12 of any frame; the
                              transcoder sets it itself)                     */
  int32_t decoder;         /* 0 auto: the I_PCM / integer-motion subset kernels
                              when the stream's headers allow, else (or when
                              the device parser meets syntax outside the
                              subset) the general CAVLC decoder; 1 subset
                              only; 2 general              */
  int32_t _pad;
} vts_params;

/* Demux the file's first H.264 video track on the host (MP4 boxes and NAL
 * length prefixes only), upload the elementary stream to device `device`
 * and prepare the decode schedule.  Fails with VTS_E_UNSUPPORTED for streams
 * outside the device decoder's subset (see DESIGN.md §Decoder subset). */
int vts_open(int device, const char *path, const vts_params *params,
             vts_ctx **out);
/* Same, from an in-memory MP4 image (copied). */
int vts_open_memory(int device, const uint8_t *data, int64_t size,
                    const vts_params *params, vts_ctx **out);
int vts_info(const vts_ctx *ctx, vts_video_info *info);

/* Decode every frame on the device and score it.  Host outputs, each may be
 * NULL except scores; cap must be >= n_frames (else VTS_E_CAPACITY with
 * *n_frames set).  pts is in track timescale units, presentation order. */
int vts_score(vts_ctx *ctx, float *scores, uint32_t *hist, uint64_t *sad,
              int64_t *pts, int64_t cap, int64_t *n_frames);
/* Device-resident variant for benchmarking: decode + score all frames,
 * results stay on the device; returns after the work is enqueued and
 * finished (synchronous). */
int vts_run(vts_ctx *ctx);
/* vts_run split in two: vts_run_async enqueues the run on the session's HIP
 * streams and returns; vts_wait blocks until it is done (errors, timings and
 * any re-run as in vts_run).  Several sessions submitted before any waits
 * share the device (plan_batch).  Entry points that read results wait
 * themselves; vts_close waits for a run nobody waited for. */
int vts_run_async(vts_ctx *ctx);
int vts_wait(vts_ctx *ctx);
/* Scene cut frame indices (score > threshold) of the last vts_score/vts_run. */
int vts_scene_cuts(vts_ctx *ctx, int64_t *frame_idx, int64_t cap,
                   int64_t *n_out);
/* Presentation timestamps of every frame (track timescale, presentation
 * order, the order of every result); host data, no device work.  Two-call
 * size query: with pts == NULL or cap < n_frames returns VTS_E_CAPACITY and
 * sets *n_out.  The batch driver (vtseg.batch.plan_batch) turns scene-cut
 * indices into times with it without copying the per-frame results. */
int vts_frame_pts(const vts_ctx *ctx, int64_t *pts, int64_t cap, int64_t *n_out);
/* Frame index of each segment time (see vts_boundary_frames_pts). */
int vts_boundary_frames(vts_ctx *ctx, const double *times, int64_t n,
                        int64_t *frame_idx);
/* Copy frame i's decoded NV12 (display size, pitch = width) of the most
 * recent window to host; only frames still resident in the ring.  A session
 * on the paired schedule (level_block 0) does not store the first frame of
 * each pair: asking for one decodes the video once more with one launch per
 * level, which stores every frame, and the session stays on that schedule
 * for the rest of its life (same results, one extra run). */
int vts_get_frame_nv12(vts_ctx *ctx, int64_t frame, uint8_t *out,
                       int64_t out_bytes);
/* RGB thumbnail (w x h x 3, see vts_score_desc) of frame i of the last run. */
int vts_get_thumbnail_rgb(vts_ctx *ctx, int64_t frame, uint8_t *out,
                          int64_t out_bytes);
/* Timing of the last vts_run/vts_score, milliseconds, HIP events:
 * [0] whole, [1] parse, [2] reconstruct, [3] score. */
int vts_last_timings(const vts_ctx *ctx, double *ms4);
/* Device memory released by closed sessions stays mapped in a process-wide
 * cache that later sessions reuse (re-allocating released HBM waits while the
 * driver clears it); this hands device `device`'s cache back to HIP. */
int vts_empty_cache(int device);
/* Bytes of device memory the sessions' allocator has handed out on `device`
 * (open sessions' buffers; the cache's free ranges excluded). */
int64_t vts_device_bytes(int device);
/* Destroy the idle pooled HIP stream sets of `device` (< 0: every device);
 * sets held by open sessions stay.  Returns the number of sets destroyed.
 * Call before process exit when streams should not outlive the library
 * (the Python loader does, at interpreter exit). */
int vts_release_streams(int device);
/* Host time of the vts_open that made ctx, milliseconds, by stage:
 * [0] demux (moov) + device checks, [1] unused, [2] sample read (parallel
 * pread), [3] host decode schedule, [4] device allocations (+ the general
 * decoder's set-up kernels), [5] wait for the elementary-stream upload (it
 * runs on its own thread beside [3] and [4]), [6] the rest, [7] total.
 * Writes min(cap, 8) entries; returns 8. */
int vts_open_timings(const vts_ctx *ctx, double *ms, int32_t cap);
/* Decode schedule facts: what = 0 reconstruct launches per run, 1 windows,
 * 2 slices, 3 ring frames, 4 fused scoring (1/0), 5 / 6 level-blocked
 * launches / chains, 7 chain slots, 8 general decoder (1/0), 9 runs repeated
 * with the bound's CABAC coefficient arena, 10 coefficient blocks per ring,
 * 11 decoded-picture surfaces per ring when the general decoder recycles them
 * (0: one per window frame), 12 the session's HIP stream set (0 plain
 * streams on the process's shared hardware queues, 1 streams with hardware
 * queues of their own: sessions opened beside others, at most 3 such sets
 * per device), 13 CABAC slices parsed in the windows' long-slice launches
 * (0: every window one parse launch), 14 the intra kernel the general
 * decoder's level launches run (2 h264_intra_v2, lane-parallel; 1
 * h264_intra_full, by block: VTS_INTRA=1, or pictures whose level table does
 * not fit the former's LDS; 0: subset decoder), 15 / 16 paired launches
 * (two P levels each, the default schedule where it applies, see
 * vts_params.level_block) / chains over them per run (0 once the session
 * runs one launch per level); < 0 on error.  Fields are
 * only ever appended: a new index is no ABI break, and a library that does
 * not know an index answers VTS_E_INVALID. */
int64_t vts_schedule_info(const vts_ctx *ctx, int32_t what);  /* 8: general decoder in use (1/0) */
int vts_close(vts_ctx *ctx);

/* ------------------------------------------------------------ batch
 * One call per process plans (and with score = 1 decodes + scores) a batch
 * of videos: video i belongs to rank i % world, this process runs its own
 * (at most max_in_flight sessions open at once, every run submitted before
 * earlier ones are waited for), and two all-gathers over RCCL give every
 * rank the whole batch: the per-video records, then the boundary arrays
 * padded to the batch's widths.  Replaces the reference's sequential loop
 * (src/pipeline.py:376-393 -> ContentAnalyzer.analyze_video per URL); the
 * same records and rules as vtseg.batch.plan_batch (a video whose scoring
 * fails is marked and the batch goes on; a planning error fails the call
 * on the rank that meets it, before any exchange).
 *
 * The communicator: vts_rccl_unique_id on one rank, its 128 bytes sent to
 * the others by the host's own means, then vts_rccl_comm_init on every
 * rank (its device, the world size, its rank).  NULL: this process is the
 * whole batch (rank 0 of 1) and nothing is exchanged.  RCCL (librccl.so.1)
 * is loaded on first use. */
#define VTS_RCCL_ID_BYTES 128
int vts_rccl_unique_id(uint8_t *id /* VTS_RCCL_ID_BYTES */);
int vts_rccl_comm_init(int32_t device, int32_t world, int32_t rank, const uint8_t *id, void **comm);
int vts_rccl_comm_destroy(void *comm);

typedef struct vts_batch vts_batch;
typedef struct vts_batch_params {
  int32_t score;             /* 1: decode + score every video (scene cuts, segment frames)  */
  int32_t device;            /* HIP device of this rank                                     */
  int32_t max_in_flight;     /* sessions open at once on this rank; 0 = 4                   */
  int32_t _pad;
  int64_t current_api_count; /* plan_segments_with_budget's current_api_count               */
  void *rccl_comm;           /* vts_rccl_comm_init's, or NULL (one process, no exchange)    */
} vts_batch_params;
/* BatchItem (vtseg/batch.py) without its arrays */
typedef struct vts_batch_record {
  double duration;           /* probe_duration, through the exchange in microseconds      */
  int64_t n_segments;        /* plan_segments windows                                     */
  int64_t n_cuts;            /* scene cuts; -1 when not scored or scoring failed          */
  int32_t rank;              /* rank that processed the video                             */
  int32_t score_failed;      /* 1: scoring failed (vts_batch_error on that rank says why) */
} vts_batch_record;
int vts_batch_run(const char *const *paths, int64_t n, const vts_budget_cfg *cfg,
                  const vts_batch_params *params, vts_batch **out);
int vts_batch_get(const vts_batch *b, int64_t i, vts_batch_record *rec);
/* video i's arrays (score = 1): segment_frames 2 x n_segments ([start, end)
 * frame of each segment's extract window), cut_frames / cut_times n_cuts
 * (presentation time in seconds); each may be NULL */
int vts_batch_arrays(const vts_batch *b, int64_t i, int64_t *segment_frames,
                     int64_t *cut_frames, double *cut_times);
/* the scoring failure of one of this rank's videos ("" otherwise); two-call
 * size query through *len */
int vts_batch_error(const vts_batch *b, int64_t i, char *msg, int64_t cap, int64_t *len);
void vts_batch_free(vts_batch *b);

/* ------------------------------- upload transcode (360p)
 * Replaces the pixel half of ContentAnalyzer._compress_video_for_upload
 * (src/analyzer/content_analyzer.py:167-236: `ffmpeg -vf scale=-2:360
 * -c:v libx264 -crf 28`).  The session's device decoder decodes every frame,
 * an area filter downscales it to (w, height) with w = ffmpeg's scale=-2
 * width, and a device encoder writes H.264 Constrained Baseline (CAVLC; Main
 * with CABAC when vts_transcode_ext4.cabac = 1): IDR (all
 * I_PCM, or Intra16x16 with intra = 1, or Intra16x16 / Intra_4x4 with
 * vts_transcode_ext5.intra4x4 = 1 as well) every keyint frames (and at scene cuts
 * if asked), P pictures of full-search
 * integer motion (P_L0_16x16 / P_Skip; refined to half or quarter samples
 * with vts_transcode_ext.subpel; vector cost and early P_Skip with
 * vts_transcode_ext3.mvcost / early_skip) with a quantised residual (qp), I_PCM
 * where that residual would cost more; one slice per macroblock row, the
 * in-loop filter off or (vts_transcode_ext2.deblock) on inside each slice; MP4
 * (moov at the end), video only.  DESIGN.md §11. */
typedef struct vts_transcode_params {
  int32_t height;          /* output display height, even; 0 = 360            */
  int32_t search_range;    /* full-search motion range in luma pixels 0..16;
                              < 0 = 0 (zero motion only); 0 = default 8       */
  int32_t max_mb_sad;      /* inter if luma+chroma SAD <= this, else I_PCM;
                              0 = default 1536 (4 per sample; 36 dB PSNR
                              on the synthetic 720p clip); < 0 = all I_PCM */
  int32_t keyint;          /* max frames per GOP; 0 = 250 (x264's default)    */
  float cut_threshold;     /* with idr_at_cuts: IDR where score > this;
                              <= 0 = the session's threshold                  */
  int32_t idr_at_cuts;     /* 1: also an IDR at every scene cut (an IDR is all
                              I_PCM, so off by default: a cut P picture falls
                              back to I_PCM only where motion misses)         */
  int32_t qp;              /* residual coding of P macroblocks at this QP (flat
                              scaling): P_L0_16x16 + quantised 4x4 residual,
                              I_PCM only where the residual's CAVLC bits would
                              exceed the I_PCM payload; 0 = default 28 (the
                              reference's CRF); < 0 = no residual (inter within
                              max_mb_sad, else I_PCM)                        */
  int32_t intra;           /* 0: intra macroblocks are I_PCM (every IDR picture,
                              and P macroblocks whose residual costs more);
                              1: they are coded as Intra16x16 (Horizontal / DC
                              from the left macroblock, Hadamard DC, 4x4
                              residual at qp) where that takes no more bits
                              than I_PCM; needs residual coding (qp >= 0).
                              Any other value: VTS_E_INVALID                 */
} vts_transcode_params;

typedef struct vts_transcode_info {
  int32_t width, height;   /* output display size                              */
  int64_t n_frames;
  int64_t n_idr;
  int64_t pcm_mbs, inter_mbs, skip_mbs;
  int64_t bytes_written;   /* output file size                                 */
  double ms[4];            /* decode+score+downscale (host clock), motion
                              search span (stream 1), slice writing span
                              (stream 2, overlaps the searches), MP4 mux      */
  int64_t intra_mbs;       /* Intra16x16 macroblocks (intra = 1), and with
                              vts_transcode_ext5.intra4x4 the I_NxN ones too;
                              pcm_mbs counts only the macroblocks that stayed
                              I_PCM                                            */
  uint64_t recon_hash;     /* intra = 1, subpel != 0 or deblock = 1: the encoder's own
                              reconstruction, hashed as
                              vts_synth_info.recon_hash (display-size NV12, f =
                              the frame index; an I_PCM IDR picture is its
                              source); else 0                                  */
} vts_transcode_info;

/* Transcode the session's video to `out_path`. */
int vts_transcode(vts_ctx *ctx, const char *out_path, const vts_transcode_params *p,
                  vts_transcode_info *info);

/* Further encoder settings and facts travel in size-tagged structs, so that
 * later ones need neither a new entry point nor a new ABI version: the caller
 * sets struct_size to its own sizeof; a size below 8 is VTS_E_INVALID, a
 * larger one than the library knows is accepted, and only the prefix both
 * sides know is read or written.  Callers detect vts_transcode_ex by its
 * symbol (the version stays 9: the change is purely additive). */
typedef struct vts_transcode_ext {
  uint32_t struct_size;    /* sizeof(vts_transcode_ext) of the caller          */
  int32_t subpel;          /* motion refinement around the integer winner, by
                              luma SAD of the 8.4.2.2.1 prediction: 0 none
                              (every output byte as vts_transcode), 1 half
                              samples, 2 half then quarter samples (DESIGN.md
                              §11); any other value: VTS_E_INVALID            */
} vts_transcode_ext;

typedef struct vts_transcode_ext_info {
  uint32_t struct_size;    /* sizeof(vts_transcode_ext_info) of the caller     */
  int32_t _pad;
  int64_t subpel_mbs;      /* inter macroblocks with a fractional vector       */
  int64_t qpel_mbs;        /* ... with an odd (quarter-sample) component       */
} vts_transcode_ext_info;

/* The in-loop deblocking filter (8.7) in the encoder, DESIGN.md §11.  Both
 * structs begin with the ones above and are passed to vts_transcode_ex by
 * pointer cast with struct_size = their own sizeof; the library reads deblock
 * when struct_size >= 12, deblock_alpha at >= 16, deblock_beta at >= 20 (a
 * field the struct does not reach is 0) and writes deblock_mbs at >= 32.
 * deblock = 1: every slice (one per macroblock row) carries
 * disable_deblocking_filter_idc = 2 and the two offsets, and the encoder
 * filters its own reconstruction the same way before the next picture
 * predicts from it: the left macroblock edge and the inner 4x4 edges, never
 * the top macroblock edge (a slice boundary; idc 0 is not offered).  Needs
 * residual coding (qp >= 0).  VTS_E_INVALID, the field named in the message:
 * deblock not 0 or 1, an offset outside -6..6, a non-zero offset with
 * deblock = 0, deblock = 1 with qp < 0.  recon_hash is also filled when
 * deblock = 1. */
typedef struct vts_transcode_ext2 {
  vts_transcode_ext base;
  int32_t deblock;         /* 0 off (every output byte as before), 1 on         */
  int32_t deblock_alpha;   /* slice_alpha_c0_offset_div2, -6..6                 */
  int32_t deblock_beta;    /* slice_beta_offset_div2, -6..6                     */
  int32_t _pad;
} vts_transcode_ext2;

typedef struct vts_transcode_ext_info2 {
  vts_transcode_ext_info base;
  int64_t deblock_mbs;     /* macroblocks in which the filter ran on at least
                              one sample line (filterSamplesFlag); 0 when
                              deblock is off                                   */
} vts_transcode_ext_info2;

/* Two rate-aware decisions of the motion search and the encoder's command
 * words, DESIGN.md §11.  As the structs above: begun with them, passed by
 * pointer cast, struct_size = their own sizeof.  Read: mvcost when struct_size
 * >= 28, mv_lambda16 at >= 32, early_skip at >= 36, cmd_out at >= 48, cmd_cap
 * at >= 56 (a field the struct does not reach is 0 / NULL); written:
 * early_skip_mbs at >= 40, cmd_words at >= 48.  Both decisions need residual
 * coding (qp >= 0) and run only with max_mb_sad >= 0.
 * mvcost = 1: the search orders its candidates (integer pass and both
 * refinement steps) by 16 SAD + lambda16 * bits(mvd against a predictor guess:
 * the left macroblock's vector in the previous picture) instead of the SAD
 * alone.  early_skip = 1: a macroblock whose residual at vector (0, 0)
 * quantises to nothing is P_Skip before any search.
 * Command words (cmd_out[frame][my][mx] over the coded macroblock grid, the
 * encoder's final decision per macroblock, with any settings): an inter
 * macroblock's is its vector in quarter samples, (uint16_t)mvx |
 * (uint16_t)mvy << 16 (P_Skip is 0); 0x80008000 is I_PCM; Intra16x16 is
 * 0x80000000 | Intra16x16PredMode (1 Horizontal, 2 DC) |
 * intra_chroma_pred_mode (0 DC, 1 Horizontal) << 2 | coded_block_pattern << 4
 * (high half 0x8000, bit 15 clear).  Pictures whose words the
 * encoder never writes (IDR pictures with intra = 0) are reported as I_PCM.
 * VTS_E_INVALID, the field named: mvcost or early_skip not 0 or 1,
 * mv_lambda16 outside 0..4096, mv_lambda16 != 0 with mvcost = 0, either flag
 * with qp < 0.  VTS_E_CAPACITY before any encoding: cmd_out with cmd_cap <
 * cmd_words.  recon_hash is also filled when either flag is set. */
typedef struct vts_transcode_ext3 {
  vts_transcode_ext2 base;
  int32_t mvcost;          /* 0 off (every output byte as before), 1 on         */
  int32_t mv_lambda16;     /* 16 lambda of the vector cost, 1..4096; 0 = the
                              table's value for qp (93.7 -> 94 at qp 28)       */
  int32_t early_skip;      /* 0 off (every output byte as before), 1 on         */
  int32_t _pad;
  uint32_t *cmd_out;       /* NULL, or cmd_cap words that receive the command
                              word of every macroblock                         */
  int64_t cmd_cap;         /* words cmd_out holds                               */
} vts_transcode_ext3;

typedef struct vts_transcode_ext_info3 {
  vts_transcode_ext_info2 base;
  int64_t early_skip_mbs;  /* macroblocks the early P_Skip probe decided; 0
                              when early_skip is off                           */
  int64_t cmd_words;       /* n_frames * macroblocks per picture               */
} vts_transcode_ext_info3;

/* CABAC entropy coding (9.3) in the encoder, DESIGN.md §11.  As the structs
 * above: begun with them, passed by pointer cast, struct_size = its own
 * sizeof; cabac is read when struct_size >= 60 (a 56-byte vts_transcode_ext3
 * or anything smaller: 0).  cabac = 1: the SPS says Main (profile_idc 77,
 * constraint_set1), the PPS entropy_coding_mode_flag = 1, P slices carry
 * cabac_init_idc 0, and the slice data of every slice is written by 7.3.4 /
 * 9.3 instead of CAVLC.  Entropy coding is lossless: every decision of the
 * encoder (still made with the CAVLC bit counts), every count, command word
 * and recon_hash is that of the same call with cabac = 0; only the bytes of
 * the slices and the two parameter sets differ.  A slice's staging slot grows
 * to the CABAC worst case, 9024 bytes per macroblock.  Needs residual coding
 * (qp >= 0).  VTS_E_INVALID, the field named: cabac not 0 or 1, cabac = 1 with
 * qp < 0. */
typedef struct vts_transcode_ext4 {
  vts_transcode_ext3 base;
  int32_t cabac;           /* 0 CAVLC (every output byte as before), 1 CABAC    */
  int32_t _pad2;
} vts_transcode_ext4;

/* Intra_4x4 coding of intra macroblocks, DESIGN.md §11 "Intra4x4".  As the
 * structs above: begun with them, passed by pointer cast, struct_size = their
 * own sizeof.  Read: intra4x4 when struct_size >= 68, i4_out at >= 80, i4_cap
 * at >= 88 (a 64-byte vts_transcode_ext4 or anything smaller: off / NULL);
 * written: intra4x4_mbs at >= 56, i4_words at >= 64.
 * intra4x4 = 1 (needs intra = 1 and residual coding): every macroblock that
 * intra = 1 would code as Intra16x16 or leave I_PCM is also tried as I_NxN
 * with sixteen Intra_4x4 blocks and becomes that when its CAVLC bits are
 * strictly fewer than the Intra16x16 candidate's (chroma is the same for
 * both); the winner is coded when it takes no more bits than I_PCM.  A slice
 * is one macroblock row, so a block has samples above it only inside its own
 * macroblock: the top four blocks choose among Horizontal, DC and
 * Horizontal_Up (DC alone at mx = 0), the other twelve among all nine modes
 * (column 0 at mx = 0: Vertical, DC, Diagonal_Down_Left, Vertical_Left), by
 * 16 SAD + lambda16(qp) * bits of the mode's code, ties to the lower mode.
 * vts_transcode_info.intra_mbs counts Intra16x16 and I_NxN macroblocks
 * together; intra4x4_mbs is the I_NxN share.
 * Command word of an I_NxN macroblock: 0x80004000 | intra_chroma_pred_mode
 * << 2 | coded_block_pattern << 4 (bits 0..1 zero).  i4_out[frame][my][mx]:
 * nibble k of an I_NxN macroblock's word is the Intra4x4PredMode of
 * luma4x4BlkIdx k; every other macroblock's word is ~0.
 * VTS_E_INVALID, the field named: intra4x4 not 0 or 1, intra4x4 = 1 with
 * intra = 0 or qp < 0.  VTS_E_CAPACITY before any encoding: i4_out with
 * i4_cap < i4_words.  recon_hash is filled (intra = 1 does that). */
typedef struct vts_transcode_ext5 {
  vts_transcode_ext4 base;
  int32_t intra4x4;        /* 0 off (every output byte as before), 1 on         */
  int32_t _pad3;
  uint64_t *i4_out;        /* NULL, or i4_cap words, one per macroblock         */
  int64_t i4_cap;          /* words i4_out holds                                */
} vts_transcode_ext5;

typedef struct vts_transcode_ext_info4 {
  vts_transcode_ext_info3 base;
  int64_t intra4x4_mbs;    /* macroblocks coded I_NxN (Intra_4x4); 0 when
                              intra4x4 is off                                  */
  int64_t i4_words;        /* n_frames * macroblocks per picture               */
} vts_transcode_ext_info4;

/* Inter partitions, DESIGN.md §11 "Partitions".  As the structs above: begun
 * with them, passed by pointer cast, struct_size = their own sizeof.  Read:
 * partitions when struct_size >= 92, mv_out at >= 104, mv_cap at >= 112 (an
 * 88-byte vts_transcode_ext5 or anything smaller: off / NULL); written:
 * p16x8_mbs at >= 72, p8x16_mbs at >= 80, p8x8_mbs at >= 88, mv_words at >= 96.
 * partitions = 1 (needs mvcost = 1, residual coding and max_mb_sad >= 0): the
 * motion search keeps every candidate's SAD per 8x8 quadrant and gives a
 * macroblock one vector, a top and a bottom one (16x8), a left and a right one
 * (8x16) or one per quadrant (P_8x8 of four P_L0_8x8; nothing below 8x8, one
 * reference picture).  Each of the nine blocks takes its least (16 SAD +
 * lambda16 bits(v - p), candidate) over the window, p the macroblock's
 * predictor guess; a shape costs its blocks' sum plus lambda16 times its
 * mb_type / sub_mb_type bits (1, 3, 3, 9), the least wins, ties to fewer
 * vectors.  With subpel each block of that shape is refined on its own.  The
 * macroblock is then coded in the coarsest shape its four quadrant vectors
 * allow, so equal vectors are never sent twice; all equal is P_L0_16x16 (or
 * P_Skip by the rule above).  inter_mbs counts partitioned macroblocks too;
 * subpel_mbs / qpel_mbs count a macroblock once (quarter if any vector has an
 * odd component, else half if any is fractional).
 * Command word of a partitioned macroblock: 0x00008000 | shape << 16, shape 1
 * 16x8, 2 8x16, 3 8x8.  mv_out[frame][my][mx][4]: the quadrant vectors (raster
 * order) of every inter macroblock as mvx | mvy << 16, a 16x16 macroblock's
 * word four times, P_Skip four 0; every word of an intra or I_PCM macroblock
 * is 0x80008000.  Reported with any settings, as cmd_out is.
 * VTS_E_INVALID, the field named: partitions not 0 or 1, partitions = 1 with
 * qp < 0, with max_mb_sad < 0 or without mvcost = 1 (a SAD-only split always
 * prefers the finest shape).  VTS_E_CAPACITY before any encoding: mv_out with
 * mv_cap < mv_words.  recon_hash is filled (mvcost = 1 does that). */
typedef struct vts_transcode_ext6 {
  vts_transcode_ext5 base;
  int32_t partitions;      /* 0 off (every output byte as before), 1 on         */
  int32_t _pad4;
  uint32_t *mv_out;        /* NULL, or mv_cap words, four per macroblock        */
  int64_t mv_cap;          /* words mv_out holds                                */
} vts_transcode_ext6;

typedef struct vts_transcode_ext_info5 {
  vts_transcode_ext_info4 base;
  int64_t p16x8_mbs;       /* macroblocks coded P_L0_L0_16x8; these three 0 when */
  int64_t p8x16_mbs;       /* ... P_L0_L0_8x16               partitions is off  */
  int64_t p8x8_mbs;        /* ... P_8x8                                         */
  int64_t mv_words;        /* 4 * n_frames * macroblocks per picture            */
} vts_transcode_ext_info5;

/* Per-picture QP and rate control, DESIGN.md §11 "Rate control".  As the
 * structs above: begun with them, passed by pointer cast, struct_size = their
 * own sizeof.  Read: bitrate_kbps when struct_size >= 116, qp_min at >= 120,
 * qp_max at >= 124, frame_qp at >= 136, frame_qp_n at >= 144, qp_out at >= 152,
 * bits_out at >= 160, frame_cap at >= 168 (a 112-byte vts_transcode_ext6 or
 * anything smaller: off / NULL); written: qp_sum at >= 104, qp_lo at >= 108,
 * qp_hi at >= 112, est_bits at >= 120, frame_words at >= 128.
 * frame_qp: frame f is coded at frame_qp[f] by every stage (the quantiser and
 * the reconstruction, the early P_Skip probe, lambda16 of the vector cost and
 * of the Intra_4x4 modes unless mv_lambda16 is given, SliceQPY of the in-loop
 * filter, slice_qp_delta = frame_qp[f] - 26 and the CABAC context
 * initialisation); mb_qp_delta stays 0 and the parameter sets do not change.
 * A constant frame_qp gives the bytes of the same call with that qp.
 * bitrate_kbps: one controller per GOP sets the QPs on the device
 * (csrc/enc_ratectl.h).  With B = bitrate_kbps * 1000 * frame duration (floor)
 * and L the GOP's pictures: picture 0 is coded at clamp(qp), picture 1 at
 * clamp(qp_0 + 3), picture j + 1 at the QP of picture j moved by at most 4 so
 * that picture j's measure scaled by 2^(-step / 6) meets (B L - measure so
 * far) / (L - j - 1); a picture that measured 0 leaves the QP, an overspent
 * GOP raises it by 4; every QP is clamped to [qp_min, qp_max].  GOPs share no
 * budget.  The measure of a picture, in bits: P_Skip 0; an inter macroblock
 * the CAVLC bound of its residual (what the inter / I_PCM decision compares)
 * plus the bits of its vectors against the search's predictor guess; an
 * Intra16x16 / I_NxN macroblock its exact macroblock_layer() bits in CAVLC;
 * I_PCM 3072.  It bounds inter residuals from above and leaves out slice and
 * macroblock headers of P pictures; no hit tolerance is promised (DESIGN.md
 * has the measured target / achieved ratios).
 * qp_out / bits_out are filled with any settings: with both features off
 * qp_out holds qp everywhere and bits_out 0.
 * VTS_E_INVALID, the field named: bitrate_kbps outside 0 .. 1 000 000; qp_min
 * or qp_max outside 1 .. 51 or qp_min > qp_max; either non-zero with both
 * features off; frame_qp together with bitrate_kbps; frame_qp_n != n_frames;
 * a frame_qp entry outside 1 .. 51; either feature with qp < 0, with
 * max_mb_sad < 0 or without mvcost = 1.  VTS_E_CAPACITY before any encoding:
 * qp_out or bits_out with frame_cap < n_frames.  recon_hash is filled
 * (mvcost = 1 does that). */
typedef struct vts_transcode_ext7 {
  vts_transcode_ext6 base;
  int32_t bitrate_kbps;    /* 0 off (every output byte as before); 1 .. 1 000 000 */
  int32_t qp_min;          /* 0 = 10                                            */
  int32_t qp_max;          /* 0 = 51                                            */
  int32_t _pad5;
  const uint8_t *frame_qp; /* NULL, or frame_qp_n QPs, each 1 .. 51             */
  int64_t frame_qp_n;      /* must equal n_frames                               */
  uint8_t *qp_out;         /* NULL, or frame_cap bytes: the QP of each frame    */
  uint32_t *bits_out;      /* NULL, or frame_cap words: its rate measure        */
  int64_t frame_cap;       /* entries each of the two holds                     */
} vts_transcode_ext7;

typedef struct vts_transcode_ext_info6 {
  vts_transcode_ext_info5 base;
  int64_t qp_sum;          /* sum of the frames' QPs                            */
  int32_t qp_lo;           /* lowest QP used                                    */
  int32_t qp_hi;           /* highest QP used                                   */
  int64_t est_bits;        /* sum of the measure; 0 with both features off      */
  int64_t frame_words;     /* n_frames                                          */
} vts_transcode_ext_info6;

/* A frame range, DESIGN.md §11 "Segment re-encode".  As the structs above:
 * begun with them, passed by pointer cast, struct_size = their own sizeof.
 * Read: frame_first when struct_size >= 176, frame_count at >= 184 (a 168-byte
 * vts_transcode_ext7 or anything smaller: 0, the whole video); written:
 * frame_first at >= 136, frame_count at >= 144 (the range applied).
 * Frames are counted in presentation order, as every result and
 * vts_boundary_frames count them.  The output is what the same call would
 * write for a video made of the frames [frame_first, frame_first +
 * frame_count) alone: frame frame_first is an IDR picture, keyint, the rate
 * controller's GOPs, idr_pic_id and frame_num start there, idr_at_cuts reads
 * the session's scores of the frames after it, recon_hash weighs a frame by
 * its index inside the range, and sample i of the file has the time i * the
 * frame duration.  vts_transcode_info.n_frames, cmd_words, i4_words, mv_words,
 * frame_words, frame_qp_n and the capacities checked for cmd_out, i4_out,
 * mv_out, qp_out and bits_out count the range's frames; the constant frame
 * duration is asked of the range only.  Every window of the video is still
 * decoded and scored (the session's scores stay whole); only the range's
 * frames are kept for the encoder.
 * VTS_E_INVALID, the field named: frame_first < 0 or >= the video's frames,
 * frame_count < 0 or frame_first + frame_count > the video's frames.
 * frame_first = 0 and frame_count = 0 is the call as it was, byte for byte. */
typedef struct vts_transcode_ext8 {
  vts_transcode_ext7 base;
  int64_t frame_first;     /* first frame of the range                          */
  int64_t frame_count;     /* its frames; 0 = through the last frame            */
} vts_transcode_ext8;

typedef struct vts_transcode_ext_info7 {
  vts_transcode_ext_info6 base;
  int64_t frame_first;     /* the range applied                                 */
  int64_t frame_count;
} vts_transcode_ext_info7;

/* Adaptive quantisation, DESIGN.md §11 "Adaptive quantisation".  As the
 * structs above: begun with them, passed by pointer cast, struct_size = their
 * own sizeof.  Read: aq_strength_q8 when struct_size >= 188, aq_max at >= 192,
 * mbqp_out at >= 200, mbqp_cap at >= 208 (a 184-byte vts_transcode_ext8 or
 * anything smaller: off / NULL); written: mbqp_words at >= 152, aq_lo at >=
 * 156, aq_hi at >= 160, aq_mbs at >= 168.
 * aq_strength_q8 > 0: every macroblock of every picture gets a QP offset from
 * the samples of the encoder's input picture alone (csrc/enc_aq.h, after
 * x264's aq-mode 1): with E the sum over the macroblock's luma and two chroma
 * blocks of (sum of squares - (sum)^2 / samples) and L = log2(max(E, 1)) in
 * Q8, offset = clamp(round(aq_strength_q8 (L - 3693) / 65536), -aq_max,
 * aq_max): flat macroblocks below the picture's QP, busy ones above.  The
 * macroblock is coded at clamp(QP + offset, lo, hi), QP being qp, frame_qp[f]
 * or the rate controller's, lo = qp_min where the caller gave one and 1
 * where it is 0, hi = qp_max or 51 (not the controller's default 10: a
 * macroblock with offset 0 keeps a frame_qp below 10; a frame_qp outside a
 * given range is brought into it): the quantiser and the reconstruction, the
 * early P_Skip probe, lambda16 of the vector cost and of the Intra_4x4 modes
 * unless mv_lambda16 is given, and the in-loop filter's indices (from QP_Y of
 * the two macroblocks at an edge) follow it.  The slices carry mb_qp_delta
 * against the running QP of 7.4.5, which starts at SliceQPY (the picture's QP)
 * in every slice; the parameter sets do not change.  The offsets are computed
 * before the first level and do not depend on the rate controller, whose
 * measure counts the true mb_qp_delta bits of intra macroblocks.
 * mbqp_out: the QP of every macroblock, [frame][my][mx], as the offset and the
 * picture's QP give it (a macroblock that sends no mb_qp_delta is decoded at
 * the running QP; nothing of it depends on a QP); filled with any settings.
 * VTS_E_INVALID, the field named: aq_strength_q8 outside 0 .. 768; aq_max
 * outside 0 .. 10 or given without aq_strength_q8; aq_strength_q8 with qp < 0,
 * with max_mb_sad < 0 or without mvcost = 1.  VTS_E_CAPACITY before any
 * encoding: mbqp_out with mbqp_cap < n_frames * macroblocks.
 * aq_strength_q8 = 0 is the call as it was, byte for byte. */
typedef struct vts_transcode_ext9 {
  vts_transcode_ext8 base;
  int32_t aq_strength_q8;  /* 0 off; 1 .. 768 (256 = x264's strength 1.0)      */
  int32_t aq_max;          /* largest |offset|: 0 = 8; 1 .. 10                  */
  uint8_t *mbqp_out;       /* NULL, or mbqp_cap bytes: the QP of each macroblock */
  int64_t mbqp_cap;
} vts_transcode_ext9;

typedef struct vts_transcode_ext_info8 {
  vts_transcode_ext_info7 base;
  int64_t mbqp_words;      /* n_frames * macroblocks                            */
  int32_t aq_lo;           /* lowest offset used (0 with aq off)                */
  int32_t aq_hi;           /* highest offset used                               */
  int64_t aq_mbs;          /* macroblocks with a non-zero offset                */
} vts_transcode_ext_info8;

/* vts_transcode with the settings of `ext` (NULL: none) and the further facts
 * in `ext_info` (NULL: not wanted).  vts_transcode(c, o, p, i) is
 * vts_transcode_ex(c, o, p, NULL, i, NULL). */
int vts_transcode_ex(vts_ctx *ctx, const char *out_path, const vts_transcode_params *p,
                     const vts_transcode_ext *ext, vts_transcode_info *info,
                     vts_transcode_ext_info *ext_info);

/* ------------------------------------------------ synthetic stream writer */

typedef struct vts_synth_params {
  int32_t width, height;        /* multiples of 2; coded size = 16-aligned     */
  int32_t fps_num, fps_den;     /* frame rate, e.g. 30/1                       */
  int64_t n_frames;
  uint64_t seed;                /* PCG32 seed                                   */
  double cut_min_s, cut_max_s;  /* scene length ~ U[cut_min, cut_max] seconds   */
  double gop_max_s;             /* IDR at least every gop_max seconds           */
  int32_t max_motion;           /* |pan| per frame in luma pixels (even)        */
  int32_t slices_per_row;       /* n > 0: n slices per macroblock row; 0: one
                                   slice per picture                            */
  int32_t hash_frames;          /* 1 = compute vts_synth_info.recon_hash        */
  int32_t edge_cases;           /* bit 0: plant runs of zero luma samples in
                                   each scene texture (I_PCM data then holds
                                   emulation-prevention bytes); bit 1: odd-pixel
                                   pans (half-pel chroma, 8.4.2.2.2 bilinear);
                                   max_motion may then be odd; bit 2: the last
                                   picture (if P) loses the slice holding
                                   macroblock row 1 (missing macroblocks);
                                   bit 3: refresh pictures (not scene cuts)
                                   are non-reference non-IDR I pictures, so
                                   the next P picture predicts across them  */
  int32_t chunks;               /* the stream is coded as this many runs of
                                   frames, each starting with an IDR scene cut,
                                   on parallel host threads; 0 = one run per
                                   18 000 frames (10 min at 30 fps; 1 800 for
                                   coding 1)                                    */
  int32_t coding;               /* 0: the I_PCM / P_Skip subset above;
                                   1: full CAVLC syntax, decoded by the general
                                   device decoder: Intra_4x4 / Intra_16x16 /
                                   chroma intra modes, I_PCM, residual blocks
                                   (all coeff_token / level / run codes), P
                                   partitions 16x16 .. 4x4 with quarter-sample
                                   motion, up to 3 reference frames (list
                                   modification, non-reference pictures), QP
                                   changes, the deblocking filter on (idc 0/2,
                                   offsets); bit 4 of edge_cases then turns on
                                   constrained_intra_pred.  Further coding-1
                                   bits: 5 B pictures, 6 / 7 explicit /
                                   implicit weights, 8 temporal direct, 10
                                   CABAC, 11 8x8 transforms, 12 / 13 SPS / PPS
                                   scaling matrices, 14 content mode (with bit
                                   5: pictures coded from textured moving
                                   scenes instead of random syntax)           */
} vts_synth_params;

typedef struct vts_synth_info {
  int64_t bytes_written;
  int64_t n_idr;
  int64_t n_cuts;               /* scene cuts (excluding frame 0)               */
  int64_t timescale;            /* track timescale                              */
  uint64_t recon_hash;          /* sum over frames f, bytes j of the display-size
                                   NV12 frame: b_j * ((j % 65521) + 1) * (f + 1),
                                   mod 2^64 (the encoder's own reconstruction)  */
} vts_synth_info;

/* Write a conforming H.264 (Constrained Baseline, CAVLC, I_PCM intra
 * macroblocks, P_L0_16x16 / P_Skip integer-motion inter macroblocks without
 * residual, deblocking disabled) elementary stream in an MP4 container.
 * cut_frames (may be NULL, cap entries) receives the ground-truth scene-cut
 * frame indices. */
int vts_synth_write(const char *path, const vts_synth_params *p,
                    vts_synth_info *info, int64_t *cut_frames, int64_t cap);

/* ------------------------------------------------------------------ misc */
const char *vts_last_error(void);
int vts_abi_version(void);
/* Number of visible HIP devices (0 when none); never initialises more than
 * the HIP runtime. */
int vts_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* VTSEG_H */
