"""GPU scene scoring: decode + NV12 scoring on MI355X through libvtseg.

Two levels:

* ``score_nv12(...)`` — the scoring kernel on NV12 frames already in device
  memory (torch tensors are used only as device-memory plumbing; the work is
  ``vts_score_nv12_dev``, hand-written HIP for gfx950, enqueued on torch's
  current HIP stream).
* ``VideoScorer`` — a session over one MP4 file: host demux, device H.264
  subset decode, device scoring (``vts_open`` / ``vts_score`` / ``vts_run``).

There is no CPU fallback: without libvtseg.so or without a GPU these raise.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _lib

DEFAULT_CUT_THRESHOLD = 0.08


def _torch():
    import torch  # plumbing only: device allocations and the current stream
    return torch


def _stream_handle(device) -> int:
    torch = _torch()
    return int(torch.cuda.current_stream(device).cuda_stream)


def thumb_size(width: int, height: int, k: int) -> tuple[int, int]:
    return width // k, height // k


def score_nv12(nv12, *, width: int, height: int, pitch: int, uv_row_offset: int,
               frame_stride: int, n_frames: int, k: int, prev_luma=None,
               want_rgb: bool = True, want_hist: bool = True, out: dict | None = None,
               workspace=None) -> dict:
    """Score n_frames NV12 frames resident on the GPU (uint8 tensor, any shape,
    contiguous, 16-byte aligned).  Returns device tensors
    {rgb [F,h,w,3] u8, hist [F,256] i32(u32 bits), sad [F] i64(u64 bits),
    score [F] f32, last_luma [h*w] u8}."""
    torch = _torch()
    if not nv12.is_cuda:
        raise ValueError("nv12 must be a device tensor")
    if nv12.dtype != torch.uint8 or not nv12.is_contiguous():
        raise ValueError("nv12 must be a contiguous uint8 tensor")
    dev = nv12.device
    w, h = thumb_size(width, height, k)
    if out is None:
        out = {
            "rgb": torch.empty((n_frames, h, w, 3), dtype=torch.uint8, device=dev)
            if want_rgb else None,
            "hist": torch.empty((n_frames, 256), dtype=torch.int32, device=dev)
            if want_hist else None,
            "sad": torch.empty(n_frames, dtype=torch.int64, device=dev),
            "score": torch.empty(n_frames, dtype=torch.float32, device=dev),
            "last_luma": torch.empty(h * w, dtype=torch.uint8, device=dev),
        }
    ws_bytes = int(_lib.lib().vts_score_workspace_bytes(width, height, k, n_frames))
    if workspace is None or workspace.numel() < ws_bytes:
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    d = _lib.ScoreDesc()
    d.nv12 = nv12.data_ptr()
    d.frame_stride = frame_stride
    d.n_frames = n_frames
    d.width, d.height, d.pitch, d.uv_row_offset, d.k = width, height, pitch, uv_row_offset, k

    def p(t):
        return None if t is None else t.data_ptr()

    d.rgb = p(out["rgb"])
    d.hist = p(out["hist"])
    d.sad = p(out["sad"])
    d.score = p(out["score"])
    d.prev_luma = p(prev_luma)
    d.last_luma = p(out["last_luma"])
    d.workspace = workspace.data_ptr()
    d.workspace_bytes = workspace.numel()
    _lib.check(_lib.lib().vts_score_nv12_dev(C.byref(d), C.c_void_p(_stream_handle(dev))))
    out["_workspace"] = workspace
    return out


@dataclass
class SceneResult:
    scores: np.ndarray       # float32 [F]
    hist: np.ndarray         # uint32 [F, 256]
    sad: np.ndarray          # uint64 [F]
    pts: np.ndarray          # int64 [F], track timescale, presentation order
    timescale: int

    def cuts(self, threshold: float = DEFAULT_CUT_THRESHOLD) -> np.ndarray:
        return np.nonzero(self.scores > threshold)[0]


class VideoScorer:
    """Decode + score one MP4 file on GPU `device` (vts_open ... vts_close)."""

    def __init__(self, path: str | Path, device: int = 0, *, k: int = 0,
                 window_frames: int = 0, n_streams: int = 2,
                 cut_threshold: float = DEFAULT_CUT_THRESHOLD, fused: int = 0,
                 gops_per_launch: int = 0, parse_chunks: int = 0, level_block: int = 0,
                 keep_frames: bool = False, decoder: str = "auto"):
        self._lib = _lib.lib()
        prm = _lib.Params()
        prm.k = k
        prm.window_frames = window_frames
        prm.keep_rgb = 0
        prm.n_streams = n_streams
        prm.cut_threshold = cut_threshold
        prm.fused = fused
        prm.gops_per_launch = gops_per_launch
        prm.parse_chunks = parse_chunks
        prm.level_block = level_block
        prm.keep_frames = 1 if keep_frames else 0
        prm.decoder = {"auto": 0, "subset": 1, "general": 2}[decoder]
        self._threshold = cut_threshold
        self._path = Path(path)   # transcode_segment copies the other tracks from it
        ctx = C.c_void_p()
        _lib.check(self._lib.vts_open(int(device), str(path).encode(), C.byref(prm),
                                      C.byref(ctx)))
        self._ctx = ctx
        info = _lib.VideoInfo()
        _lib.check(self._lib.vts_info(self._ctx, C.byref(info)))
        self.info = info

    @property
    def n_frames(self) -> int:
        return int(self.info.n_frames)

    def score(self) -> SceneResult:
        n = self.n_frames
        scores = np.zeros(n, np.float32)
        hist = np.zeros((n, 256), np.uint32)
        sad = np.zeros(n, np.uint64)
        pts = np.zeros(n, np.int64)
        got = C.c_int64(0)
        f32 = C.POINTER(C.c_float)
        _lib.check(self._lib.vts_score(
            self._ctx, scores.ctypes.data_as(f32),
            hist.ctypes.data_as(C.POINTER(C.c_uint32)),
            sad.ctypes.data_as(C.POINTER(C.c_uint64)),
            pts.ctypes.data_as(C.POINTER(C.c_int64)), n, C.byref(got)))
        return SceneResult(scores, hist, sad, pts, int(self.info.track_timescale))

    def run(self) -> None:
        """Decode + score with results left on the device (benchmark step)."""
        _lib.check(self._lib.vts_run(self._ctx))

    def run_async(self) -> None:
        """Enqueue a run (decode + score) and return; wait() (or any call that
        reads results) completes it.  Runs of several sessions submitted
        before any wait share the device."""
        _lib.check(self._lib.vts_run_async(self._ctx))

    def wait(self) -> None:
        """Complete a run_async() (errors and re-runs as in run())."""
        _lib.check(self._lib.vts_wait(self._ctx))

    def arena_reruns(self) -> int:
        """Runs repeated because a CABAC window's slices asked for more
        coefficient blocks than its arena held (the session keeps the grown
        arena)."""
        return int(self._lib.vts_schedule_info(self._ctx, 9))

    def timings(self) -> dict:
        t = (C.c_double * 4)()
        _lib.check(self._lib.vts_last_timings(self._ctx, t))
        return {"total_ms": t[0], "parse_ms": t[1], "reconstruct_ms": t[2],
                "score_ms": t[3]}

    def open_timings(self) -> dict:
        """Host time of this session's vts_open by stage (ms)."""
        t = (C.c_double * 8)()
        n = self._lib.vts_open_timings(self._ctx, t, 8)
        if n < 0:
            _lib.check(n)
        return {"demux_ms": t[0], "read_ms": t[2], "schedule_ms": t[3], "alloc_ms": t[4],
                "upload_wait_ms": t[5], "rest_ms": t[6], "total_ms": t[7]}

    def recon_launches(self) -> int:
        """Reconstruct launches per run (one per GOP level per window)."""
        return int(self._lib.vts_schedule_info(self._ctx, 0))

    def general(self) -> bool:
        """The general CAVLC decoder runs (not the I_PCM / integer-motion
        subset kernels)."""
        return bool(self._lib.vts_schedule_info(self._ctx, 8))

    def own_queues(self) -> bool:
        """The session's HIP streams have hardware queues of their own (it was
        opened beside other sessions; session.hip streams_take)."""
        return int(self._lib.vts_schedule_info(self._ctx, 12)) == 1

    def windows(self) -> int:
        """Decode windows per run (1 = the whole video at once; more = the
        streamed two-ring schedule)."""
        return int(self._lib.vts_schedule_info(self._ctx, 1))

    def level_blocks(self) -> tuple[int, int]:
        """(launches, chains) of the level-blocked schedule per run; (0, 0)
        when the per-level schedule runs."""
        return (int(self._lib.vts_schedule_info(self._ctx, 5)),
                int(self._lib.vts_schedule_info(self._ctx, 6)))

    def fused(self) -> bool:
        """Scoring runs fused into reconstruction (k in {2,4,8}, no crop)."""
        return bool(self._lib.vts_schedule_info(self._ctx, 4))

    def boundary_frames(self, times) -> list[int]:
        arr = (C.c_double * len(times))(*[float(t) for t in times])
        out = (C.c_int64 * len(times))()
        _lib.check(self._lib.vts_boundary_frames(self._ctx, arr, len(times), out))
        return list(out)

    def scene_cuts(self) -> list[int]:
        n = C.c_int64(0)
        cap = self.n_frames
        buf = (C.c_int64 * max(cap, 1))()
        _lib.check(self._lib.vts_scene_cuts(self._ctx, buf, cap, C.byref(n)))
        return list(buf[: n.value])

    def frame_pts(self) -> np.ndarray:
        """Presentation timestamps of every frame (int64, track timescale,
        presentation order; host data, no device work)."""
        n = self.n_frames
        pts = np.zeros(max(n, 1), np.int64)
        got = C.c_int64(0)
        _lib.check(self._lib.vts_frame_pts(self._ctx, pts.ctypes.data_as(C.POINTER(C.c_int64)),
                                           n, C.byref(got)))
        return pts[:n]

    def scene_cut_times(self) -> list[float]:
        """Presentation times (s) of the scene-cut frames (decodes + scores):
        anchors for the opt-in scene-aware segment boundaries (vtseg.snap)."""
        from fractions import Fraction
        res = self.score()
        return [float(Fraction(int(res.pts[i]), res.timescale))
                for i in res.cuts(self._threshold)]

    def frame_nv12(self, i: int) -> np.ndarray:
        w, h = int(self.info.width), int(self.info.height)
        out = np.zeros(w * h * 3 // 2, np.uint8)
        _lib.check(self._lib.vts_get_frame_nv12(
            self._ctx, i, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size))
        return out

    def thumbnail_rgb(self, i: int, k: int | None = None) -> np.ndarray:
        kk = k or (4 if int(self.info.height) <= 720 else 6)
        w, h = int(self.info.width) // kk, int(self.info.height) // kk
        out = np.zeros((h, w, 3), np.uint8)
        _lib.check(self._lib.vts_get_thumbnail_rgb(
            self._ctx, i, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size))
        return out

    def transcode(self, out_path: str | Path, *, height: int = 360, search_range: int = 8,
                  max_mb_sad: int = 1536, keyint: int = 250, idr_at_cuts: bool = False,
                  cut_threshold: float = 0.0, qp: int = 28, intra: bool = False,
                  subpel: int = 0, deblock: bool = False,
                  deblock_offsets: tuple[int, int] = (0, 0), mvcost: bool = False,
                  early_skip: bool = False, mv_lambda16: int = 0, want_commands: bool = False,
                  cabac: bool = False, intra4x4: bool = False, want_intra4_modes: bool = False,
                  partitions: bool = False, want_vectors: bool = False,
                  bitrate_kbps: int = 0, qp_range: tuple[int, int] = (0, 0),
                  frame_qp=None, want_rate: bool = False,
                  frames: tuple[int, int] | None = None,
                  aq_strength: float = 0.0, aq_max: int = 0) -> dict:
        """360p upload transcode of this video into `out_path`
        (vts_transcode_ex): decode + score + area downscale +
        device H.264 encode with a quantised residual at `qp` (<= 0: none, the
        round-2 encoder).  `intra`: intra macroblocks (IDR pictures, P
        macroblocks the motion search misses) are coded as Intra16x16 where
        that is cheaper than I_PCM; needs `qp` > 0.  `subpel`: the motion
        vector of every P macroblock is refined around the integer winner to
        half samples (1) or half then quarter samples (2); 0 is the integer
        encoder, byte for byte.  `deblock`: the in-loop deblocking filter,
        inside each macroblock row's slice (disable_deblocking_filter_idc 2),
        with `deblock_offsets` = (slice_alpha_c0_offset_div2,
        slice_beta_offset_div2), each -6..6; needs `qp` > 0; off, every byte
        is as before.  `mvcost`: the motion search charges every candidate
        vector its bits (16 SAD + lambda16 * bits(mvd) against the left
        macroblock's vector in the previous picture; `mv_lambda16` > 0
        replaces the table's lambda); `early_skip`: a macroblock whose
        residual at vector (0, 0) quantises to nothing is P_Skip before any
        search; both need `qp` > 0 and off, every byte is as before.
        `want_commands`: the result also holds `commands`, the encoder's
        final word per macroblock (vtseg.h) as a uint32 array (n_frames, mbh,
        mbw).  `cabac`: the slices are entropy coded with CABAC in a Main
        profile stream instead of CAVLC in a Constrained Baseline one; the
        coding is lossless, so every decision, count, command word and
        `recon_hash` is that of the same call without it; needs `qp` > 0; off,
        every byte is as before.  `intra4x4`: every macroblock `intra` codes is
        also tried as I_NxN with sixteen Intra_4x4 blocks and becomes that when
        it takes strictly fewer bits than the Intra16x16 candidate; needs
        `intra` and `qp` > 0; off, every byte is as before; the result then
        holds `intra4x4_mbs`, the I_NxN share of `intra_mbs`.
        `want_intra4_modes`: the result also holds `intra4_modes`, a uint64
        array (n_frames, mbh, mbw): nibble k of an I_NxN macroblock's word is
        the Intra4x4PredMode of luma4x4BlkIdx k, every other word is ~0.
        `partitions`: the motion search may give a P macroblock a top and a
        bottom vector (16x8), a left and a right one (8x16) or one per 8x8
        quadrant (P_8x8) instead of one, chosen by rate (DESIGN.md §11
        "Partitions"); needs `mvcost` and `qp` > 0; off, every byte is as
        before; the result then holds `p16x8_mbs`, `p8x16_mbs` and `p8x8_mbs`,
        shares of `inter_mbs`.  `want_vectors`: the result also holds
        `vectors`, a uint32 array (n_frames, mbh, mbw, 4): the quadrant vectors
        of every inter macroblock as mvx | mvy << 16 (a 16x16 macroblock's
        four times, P_Skip four 0), 0x80008000 for intra and I_PCM ones.
        `frame_qp`: one QP (1..51) per frame, in frame order; every stage
        codes frame f at frame_qp[f] (slice_qp_delta, no per-macroblock QP); a
        constant one gives the bytes of the same call with that `qp`.
        `bitrate_kbps`: one controller per GOP sets the QPs on the device from
        a per-picture rate measure so that each GOP meets its share of the
        bitrate (DESIGN.md §11 "Rate control" has the measured target /
        achieved ratios; no hit tolerance is promised),
        starting every GOP at `qp` and staying inside `qp_range` = (qp_min,
        qp_max), 0 = the default 10 / 51.  Both need `mvcost` and `qp` > 0 and
        exclude each other.  With one of them or `want_rate` the result also
        holds `frame_qp` (uint8 array, the QP each frame was coded at),
        `frame_bits` (uint32 array, its rate measure: all 0 with both off),
        `qp_lo`, `qp_hi`, `qp_mean` and `est_bits`.
        `frames` = (f0, f1): only the frames [f0, f1) (presentation order, as
        `boundary_frames` counts them) are transcoded, into the file the same
        call would write for a video made of those frames alone: it starts
        with an IDR picture at time 0, `keyint`, the GOPs of `bitrate_kbps`
        and `recon_hash` count from f0, `frame_qp` and every per-frame array
        of the result have f1 - f0 entries, and the result also holds
        `frame_first` and `frame_count`.  The whole video is still decoded and
        scored; only the range is kept for the encoder (DESIGN.md §11
        "Segment re-encode").  None: the whole video, every byte as before.
        `aq_strength` > 0 (up to 3.0; 1.0 is x264's default strength): adaptive
        quantisation, a QP per macroblock from the variance of its source
        samples, flat macroblocks below the picture's QP and busy ones above
        by at most `aq_max` (0: 8; 1..10), inside `qp_range` (1..51 without
        one), sent as mb_qp_delta (DESIGN.md §11 "Adaptive quantisation"); it
        rides on `qp`, `frame_qp` or the rate controller's QP; needs `mvcost`
        and `qp` > 0; 0, every byte is as before.  The result then holds
        `mb_qp` (uint8 array (n_frames, mbh, mbw), the QP of each macroblock),
        `aq_lo` / `aq_hi` (the lowest and highest offset used) and `aq_mbs`
        (macroblocks with a non-zero offset).
        Returns the facts (with `intra`, `subpel`, `deblock`, `mvcost`
        or `early_skip` also the encoder's `recon_hash`) and per-stage
        milliseconds; with one of the last four keywords also
        `early_skip_mbs`."""
        prm = _lib.TranscodeParams()
        prm.height = height
        prm.search_range = search_range if search_range != 0 else -1
        prm.max_mb_sad = max_mb_sad
        prm.keyint = keyint
        prm.cut_threshold = cut_threshold
        prm.idr_at_cuts = 1 if idr_at_cuts else 0
        prm.qp = qp if qp > 0 else -1
        prm.intra = 1 if intra else 0
        info = _lib.TranscodeInfo()
        # the Intra4x4 structs only with their keywords: without them the call is the one it was
        # ... and the partition structs only with theirs
        i4 = bool(intra4x4 or want_intra4_modes)
        pt = bool(partitions or want_vectors)
        # ... and the rate structs only with theirs
        rc = bool(bitrate_kbps or tuple(qp_range) != (0, 0) or frame_qp is not None or want_rate)
        # ... and the range structs only with `frames`; nf: the frames every per-frame array holds
        nf = int(self.info.n_frames)
        if frames is not None:
            f0, f1 = int(frames[0]), int(frames[1])
            if f1 == f0 and 0 <= f0 < nf:   # a count of 0 means "through the last frame" to the library
                raise _lib.VtsegError(_lib.VTS_E_INVALID, f"frame_count 0: frames=({f0}, {f1}) is empty")
            nf = max(f1 - f0, 0)
        aq = bool(aq_strength or aq_max)
        aq_q8 = int(round(float(aq_strength) * 256))
        if aq_strength > 0 and aq_q8 == 0:
            aq_q8 = 1   # the smallest strength the library knows, not "off"
        ext_t = _lib.TranscodeExt9 if aq else _lib.TranscodeExt8 if frames is not None else _lib.TranscodeExt7 if rc else (
            _lib.TranscodeExt6 if pt else (_lib.TranscodeExt5 if i4 else _lib.TranscodeExt4))
        info_t = _lib.TranscodeExtInfo8 if aq else _lib.TranscodeExtInfo7 if frames is not None else _lib.TranscodeExtInfo6 if rc else (
            _lib.TranscodeExtInfo5 if pt else (_lib.TranscodeExtInfo4 if i4 else _lib.TranscodeExtInfo3))
        ext9 = _lib.TranscodeExt9(_lib.TranscodeExt8(_lib.TranscodeExt7(_lib.TranscodeExt6(_lib.TranscodeExt5(_lib.TranscodeExt4(
            _lib.TranscodeExt3(
                _lib.TranscodeExt2(_lib.TranscodeExt(C.sizeof(ext_t), subpel),
                                   1 if deblock else 0, int(deblock_offsets[0]), int(deblock_offsets[1])),
                1 if mvcost else 0, int(mv_lambda16), 1 if early_skip else 0), 1 if cabac else 0),
            1 if intra4x4 else 0), 1 if partitions else 0),
            int(bitrate_kbps), int(qp_range[0]), int(qp_range[1]))))
        ext8 = ext9.base
        ext9.aq_strength_q8, ext9.aq_max = aq_q8, int(aq_max)
        if frames is not None:
            ext8.frame_first, ext8.frame_count = f0, f1 - f0
        ext7 = ext8.base
        ext6 = ext7.base
        ext5 = ext6.base
        ext = ext5.base.base
        xinfo8 = _lib.TranscodeExtInfo8(_lib.TranscodeExtInfo7(_lib.TranscodeExtInfo6(_lib.TranscodeExtInfo5(
            _lib.TranscodeExtInfo4(_lib.TranscodeExtInfo3(_lib.TranscodeExtInfo2(_lib.TranscodeExtInfo(C.sizeof(info_t)))))))))
        xinfo7 = xinfo8.base
        xinfo6 = xinfo7.base
        xinfo5 = xinfo6.base
        xinfo4 = xinfo5.base
        xinfo3 = xinfo4.base
        xinfo2 = xinfo3.base
        xinfo = xinfo2.base
        commands = modes = vectors = mb_qp = None
        if want_commands or want_intra4_modes or want_vectors or aq:
            # the coded macroblock grid of the output: width as ffmpeg's scale=-2, both 16-aligned
            w, h = int(self.info.width), int(self.info.height)
            sw = (height * w + h) // (2 * h) * 2
            mbw, mbh = (sw + 15) // 16, (height + 15) // 16
        if want_commands:
            commands = np.zeros((nf, mbh, mbw), np.uint32)
            ext.cmd_out = commands.ctypes.data_as(C.POINTER(C.c_uint32))
            ext.cmd_cap = commands.size
        if want_intra4_modes:
            modes = np.zeros((nf, mbh, mbw), np.uint64)
            ext5.i4_out = modes.ctypes.data_as(C.POINTER(C.c_uint64))
            ext5.i4_cap = modes.size
        if want_vectors:
            vectors = np.zeros((nf, mbh, mbw, 4), np.uint32)
            ext6.mv_out = vectors.ctypes.data_as(C.POINTER(C.c_uint32))
            ext6.mv_cap = vectors.size
        if aq:
            mb_qp = np.zeros((nf, mbh, mbw), np.uint8)
            ext9.mbqp_out = mb_qp.ctypes.data_as(C.POINTER(C.c_uint8))
            ext9.mbqp_cap = mb_qp.size
        qps_in = qps = bits = None
        if rc:
            if frame_qp is not None:
                wide = np.asarray(frame_qp, dtype=np.int64).reshape(-1)
                # what a byte cannot hold would wrap in the cast (300 to 44) and get past the library's 1..51
                # check; 0 and 52..255 reach the library, which names the entry
                if wide.size and (wide.min() < 0 or wide.max() > 255):
                    raise ValueError(f"frame_qp: every QP is 1..51, got {int(wide.min())}..{int(wide.max())}")
                qps_in = np.ascontiguousarray(wide, dtype=np.uint8)
                ext7.frame_qp = qps_in.ctypes.data_as(C.POINTER(C.c_uint8))
                ext7.frame_qp_n = qps_in.size
            qps = np.zeros(nf, np.uint8)
            bits = np.zeros(nf, np.uint32)
            ext7.qp_out = qps.ctypes.data_as(C.POINTER(C.c_uint8))
            ext7.bits_out = bits.ctypes.data_as(C.POINTER(C.c_uint32))
            ext7.frame_cap = nf
        _lib.check(self._lib.vts_transcode_ex(self._ctx, str(out_path).encode(), C.byref(prm),
                                              C.cast(C.pointer(ext9), C.POINTER(_lib.TranscodeExt)),
                                              C.byref(info),
                                              C.cast(C.pointer(xinfo8), C.POINTER(_lib.TranscodeExtInfo))))
        extra = {}
        if aq:
            if xinfo8.mbqp_words != mb_qp.size:
                raise RuntimeError(f"{xinfo8.mbqp_words} macroblock QPs reported, expected {mb_qp.size}")
            extra.update(mb_qp=mb_qp, aq_lo=xinfo8.aq_lo, aq_hi=xinfo8.aq_hi, aq_mbs=xinfo8.aq_mbs)
        if frames is not None:
            extra.update(frame_first=int(xinfo7.frame_first), frame_count=int(xinfo7.frame_count))
        if rc:
            if xinfo6.frame_words != qps.size:
                raise RuntimeError(f"{xinfo6.frame_words} frames reported, expected {qps.size}")
            extra.update(frame_qp=qps, frame_bits=bits, qp_lo=xinfo6.qp_lo, qp_hi=xinfo6.qp_hi,
                         qp_mean=xinfo6.qp_sum / max(1, qps.size), est_bits=xinfo6.est_bits)
        if pt:
            extra.update(p16x8_mbs=xinfo5.p16x8_mbs, p8x16_mbs=xinfo5.p8x16_mbs, p8x8_mbs=xinfo5.p8x8_mbs)
        if want_vectors:
            if xinfo5.mv_words != vectors.size:
                raise RuntimeError(f"{xinfo5.mv_words} vector words, expected {vectors.size}")
            extra["vectors"] = vectors
        if i4:
            extra["intra4x4_mbs"] = xinfo4.intra4x4_mbs
        if want_intra4_modes:
            if xinfo4.i4_words != modes.size:
                raise RuntimeError(f"{xinfo4.i4_words} mode words, expected {modes.size}")
            extra["intra4_modes"] = modes
        if mvcost or early_skip or mv_lambda16 or want_commands:   # only with a new keyword
            extra["early_skip_mbs"] = xinfo3.early_skip_mbs
        if want_commands:
            if xinfo3.cmd_words != commands.size:
                raise RuntimeError(f"{xinfo3.cmd_words} command words, expected {commands.size}")
            extra["commands"] = commands
        return {**extra, "width": info.width, "height": info.height, "n_frames": info.n_frames,
                "n_idr": info.n_idr, "pcm_mbs": info.pcm_mbs, "inter_mbs": info.inter_mbs,
                "skip_mbs": info.skip_mbs, "intra_mbs": info.intra_mbs,
                "subpel_mbs": xinfo.subpel_mbs, "qpel_mbs": xinfo.qpel_mbs,
                "deblock_mbs": xinfo2.deblock_mbs,
                "recon_hash": int(info.recon_hash), "bytes_written": info.bytes_written,
                "decode_ms": info.ms[0], "search_ms": info.ms[1], "write_ms": info.ms[2],
                "mux_ms": info.ms[3]}

    def transcode_segment(self, out_path: str | Path, start: float, end: float, *, height: int = 0,
                          **encoder) -> dict:
        """Frame-accurate re-encode of [start, end) seconds into `out_path`
        (the reference's extract_segment re-encode branch, DESIGN.md §11
        "Segment re-encode"): the frames from the first one presented at or
        after `start` through the last one presented before `end` (ffmpeg's
        accurate seek; `boundary_frames`), transcoded at `height` lines (0: the
        source's) with `encoder` = transcode's keywords, and every other track
        of the source stream-copied beside them, cut to the kept frames'
        presentation span so that both start at 0 (vts_add_tracks_range).
        Raises VtsegError when no frame lies in the range.  Returns
        transcode's facts with `bytes_written` of the final file and
        `start` / `end`, the span of the kept frames in seconds."""
        out_path = Path(out_path)
        f0, f1 = self.boundary_frames([start, end])
        if f1 <= f0:
            raise _lib.VtsegError(_lib.VTS_E_INVALID, f"no frame is presented in [{start}, {end})")
        pts, ts, n = self.frame_pts(), int(self.info.track_timescale), self.n_frames
        if f0 + 1 < n:
            delta = int(pts[f0 + 1] - pts[f0])
        else:
            delta = int(pts[f0] - pts[f0 - 1]) if f0 > 0 else max(1, ts // 30)
        t0, t1 = int(pts[f0]) / ts, (int(pts[f1 - 1]) + delta) / ts
        video_only = out_path.with_name(out_path.name + ".video.tmp")
        try:
            facts = self.transcode(video_only, height=height or int(self.info.height), frames=(f0, f1), **encoder)
            _lib.check(self._lib.vts_add_tracks_range(str(video_only).encode(), str(self._path).encode(),
                                                      t0, t1, str(out_path).encode()))
        finally:
            if video_only.exists():
                video_only.unlink()
        return {**facts, "bytes_written": out_path.stat().st_size, "start": t0, "end": t1}

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.vts_close(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synth_write(path: str | Path, *, width: int = 1280, height: int = 720,
                fps: int = 30, n_frames: int = 300, seed: int = 0x5EED,
                cut_min_s: float = 2.0, cut_max_s: float = 20.0, gop_max_s: float = 2.0,
                max_motion: int = 4, slices_per_row: int = 1,
                hash_frames: bool = False, pcm_zero_runs: bool = False,
                odd_motion: bool = False, drop_last_slice: bool = False,
                nonref_refresh: bool = False, chunks: int = 0, coding: str = "subset",
                constrained_intra: bool = False, bframes: bool = False,
                weighted: str | None = None, temporal_direct: bool = False,
                chroma_deblock: bool = False, cabac: bool = False,
                transform_8x8: bool = False, scaling: str | None = None,
                content: bool = False) -> dict:
    """Write a synthetic H.264/MP4 clip (see vts_synth_write); returns its facts
    and the ground-truth scene-cut frames.  coding="full" only: ``bframes`` codes
    B pictures (Main profile, POC type 0, composition offsets in the MP4),
    ``weighted`` = "explicit" (pred_weight_table in P and B slices) or
    "implicit" (weighted_bipred_idc 2), ``temporal_direct`` mixes temporal with
    spatial direct prediction.  coding="subset" only: ``chroma_deblock``
    turns the deblocking filter on at QPY 3 with chroma_qp_index_offset 12 and
    filter offsets +12, so only chroma edges filter (a stream the subset
    kernels must refuse).  coding="full" only: ``cabac`` writes the same syntax
    decisions with CABAC (cabac_init_idc 0, Main profile; x264's default entropy
    coder) and ``transform_8x8`` (with cabac, High profile) adds Intra_8x8 and
    8x8-transform inter macroblocks.  coding="full" only: ``scaling`` =
    "sps", "pps" or "both" writes seeded scaling matrices (High profile; lists
    absent, default, ending early or full, exercising fall-back rules A / B).
    coding="full" with ``bframes`` only: ``content`` codes pictures instead of
    random syntax (textured scenes cut at the planted frames, a panning
    background and moving sprites; skip / direct / 16x16 motion / intra
    decisions by SAD, residuals quantised from the source's prediction error;
    synth_content.h)."""
    p = _lib.SynthParams()
    p.width, p.height, p.fps_num, p.fps_den = width, height, fps, 1
    p.n_frames, p.seed = n_frames, seed
    p.cut_min_s, p.cut_max_s, p.gop_max_s = cut_min_s, cut_max_s, gop_max_s
    p.max_motion, p.slices_per_row = max_motion, slices_per_row
    p.hash_frames = 1 if hash_frames else 0
    p.edge_cases = (1 if pcm_zero_runs else 0) | (2 if odd_motion else 0) | \
        (4 if drop_last_slice else 0) | (8 if nonref_refresh else 0)
    p.chunks = chunks
    p.coding = {"subset": 0, "full": 1}[coding]
    if constrained_intra:
        p.edge_cases |= 16
    if cabac or transform_8x8:
        if coding != "full":
            raise ValueError("cabac / transform_8x8 need coding='full'")
        if transform_8x8 and not cabac:
            raise ValueError("transform_8x8 needs cabac (8x8 CAVLC streams are refused)")
        p.edge_cases |= 1024 | (2048 if transform_8x8 else 0)
    if scaling:
        if coding != "full":
            raise ValueError("scaling matrices need coding='full'")
        p.edge_cases |= {"sps": 4096, "pps": 8192, "both": 4096 | 8192}[scaling]
    if chroma_deblock:
        if coding != "subset":
            raise ValueError("chroma_deblock is a subset-stream edge case")
        p.edge_cases |= 512
    if bframes or weighted or temporal_direct:
        if coding != "full":
            raise ValueError("B pictures / weighted prediction need coding='full'")
        p.edge_cases |= 32 | {None: 0, "explicit": 64, "implicit": 128}[weighted] | \
            (256 if temporal_direct else 0)
    if content:
        if coding != "full" or not bframes:
            raise ValueError("content mode needs coding='full' and bframes")
        p.edge_cases |= 16384
    info = _lib.SynthInfo()
    cuts = (C.c_int64 * max(n_frames, 1))()
    _lib.check(_lib.lib().vts_synth_write(str(path).encode(), C.byref(p), C.byref(info),
                                          cuts, n_frames))
    return {"bytes": int(info.bytes_written), "n_idr": int(info.n_idr),
            "n_cuts": int(info.n_cuts), "timescale": int(info.timescale),
            "recon_hash": int(info.recon_hash),
            "cuts": list(cuts[: int(info.n_cuts)])}


def scene_cut_times(path: str | Path, device: int = 0) -> list[float]:
    """Decode + score `path` on the GPU and return its scene-cut times."""
    with VideoScorer(path, device=device) as v:
        return v.scene_cut_times()
