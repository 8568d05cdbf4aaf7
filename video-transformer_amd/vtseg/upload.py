"""Upload compression: drop-in for ContentAnalyzer._compress_video_for_upload
(reference src/analyzer/content_analyzer.py:167-236).

The reference shrinks a video larger than 30 MB before uploading it with
``ffmpeg -y -i IN -vf scale=-2:360 -c:v libx264 -crf 28 -preset fast -c:a aac
-b:a 64k compressed_<name>`` and falls back to the original path when ffmpeg
is missing, fails or times out.  Here the pixel work runs on the MI355X
(``VideoScorer.transcode`` -> ``vts_transcode``: device decode, area
downscale to scale=-2:360, device H.264 encode).  Streams
outside the device decoder's subset, or a GPU failure, take the reference's
own ffmpeg command when ffmpeg exists, and otherwise the reference's
fallback: the original path.  The source's audio (every non-video track)
is stream-copied into the output (``vts_add_tracks``): the reference
re-encodes it to AAC 64k, here it keeps its original coding (no AAC encoder in
the image), so the uploaded file still has the sound track.
"""
from __future__ import annotations

import logging
import shutil
import struct
import subprocess
from pathlib import Path

from ._lib import VtsegError, VtsegLibraryError

MAX_SIZE_MB = 30  # content_analyzer.py:174


def compressed_path_for(video_path: Path) -> Path:
    """content_analyzer.py:185 naming."""
    return video_path.parent / f"compressed_{video_path.name}"


def _ffmpeg(video_path: Path, out: Path, logger: logging.Logger) -> Path:
    """The reference's command and fallbacks (content_analyzer.py:191-236)."""
    cmd = ["ffmpeg", "-y", "-i", str(video_path), "-vf", "scale=-2:360", "-c:v", "libx264",
           "-crf", "28", "-preset", "fast", "-c:a", "aac", "-b:a", "64k", str(out)]
    try:
        result = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    except FileNotFoundError:
        logger.warning("ffmpeg not installed; skipping compression")
        return video_path
    except subprocess.TimeoutExpired:
        logger.warning("ffmpeg compression timed out (5 min); skipping compression")
        if out.exists():
            out.unlink()
        return video_path
    if result.returncode != 0:
        logger.warning(f"ffmpeg compression failed: {(result.stderr or '')[:200]}")
        return video_path
    return out


def _boxes(buf: bytes, at: int, end: int):
    """(type, payload start, box end) of the ISO BMFF boxes in buf[at:end]."""
    while at + 8 <= end:
        size, kind = struct.unpack_from(">I4s", buf, at)
        head = 8
        if size == 1 and at + 16 <= end:
            size, head = struct.unpack_from(">Q", buf, at + 8)[0], 16
        elif size == 0:
            size = end - at
        if size < head or at + size > end:
            return
        yield kind, at + head, at + size
        at += size


def _moov(video_path: Path) -> bytes:
    """The payload of the file's moov box, found by walking the top-level
    box headers with seek: the media data (the whole of a long video) is
    never read."""
    end = Path(video_path).stat().st_size
    with open(video_path, "rb") as f:
        at = 0
        while at + 8 <= end:
            f.seek(at)
            head = f.read(16)
            size, kind = struct.unpack_from(">I4s", head, 0)
            n = 8
            if size == 1 and len(head) == 16:
                size, n = struct.unpack_from(">Q", head, 8)[0], 16
            elif size == 0:
                size = end - at
            if size < n or at + size > end:
                break
            if kind == b"moov":
                f.seek(at + n)
                return f.read(size - n)
            at += size
    return b""


def _sample_bytes(data: bytes, a: int, b: int) -> int:
    """The samples' total size by the stbl's stsz or stz2 box in data[a:b]
    (ISO/IEC 14496-12 8.7.3)."""
    for kind, za, zb in _boxes(data, a, b):
        if kind == b"stsz" and zb - za >= 12:
            fixed, count = struct.unpack_from(">II", data, za + 4)
            if fixed:
                return fixed * count
            count = min(count, (zb - za - 12) // 4)
            return sum(struct.unpack_from(f">{count}I", data, za + 12))
        if kind == b"stz2" and zb - za >= 12:
            field, count = data[za + 7], struct.unpack_from(">I", data, za + 8)[0]
            if field == 4:       # two sizes a byte, the first in the high nibble
                raw = data[za + 12:za + 12 + (count + 1) // 2]
                return sum((x >> 4 if i % 2 == 0 else x & 15) for i, x in
                           ((i, raw[i // 2]) for i in range(min(count, 2 * len(raw)))))
            if field in (8, 16):
                width = field // 8
                count = min(count, (zb - za - 12) // width)
                return sum(struct.unpack_from(f">{count}{'B' if width == 1 else 'H'}", data, za + 12))
    return 0


def other_tracks_bytes(video_path: Path) -> int:
    """The sample bytes of the source's non-video tracks (moov/trak with a
    handler other than 'vide': stsz or stz2), which vts_add_tracks copies into
    the compressed file as they are."""
    data = _moov(video_path)
    total = 0
    for tk, ta, tb in _boxes(data, 0, len(data)):
        if tk != b"trak":
            continue
        handler, size = b"", 0
        for mk, ma, mb in _boxes(data, ta, tb):
            if mk != b"mdia":
                continue
            for hk, ha, hb in _boxes(data, ma, mb):
                if hk == b"hdlr" and hb - ha >= 12:
                    handler = data[ha + 8:ha + 12]
                if hk != b"minf":
                    continue
                for sk, sa, sb in _boxes(data, ha, hb):
                    if sk == b"stbl":
                        size = _sample_bytes(data, sa, sb)
        if handler != b"vide":
            total += size
    return total


def target_bitrate_kbps(video_path: Path, target_size_mb: float, duration: float) -> int:
    """The video bitrate that brings the compressed file to `target_size_mb`:
    (target bytes - the bytes of the other tracks) * 8 / duration, floored,
    at least 1 kbps."""
    budget = int(target_size_mb * 1024 * 1024) - other_tracks_bytes(video_path)
    return max(1, int(budget * 8 / max(duration, 1e-3) / 1000))


def compress_video_for_upload(video_path: Path, *, logger: logging.Logger | None = None,
                              device: int = 0, max_size_mb: float = MAX_SIZE_MB,
                              intra: bool = False, subpel: int = 0, deblock: bool = False,
                              deblock_offsets: tuple[int, int] = (0, 0), mvcost: bool = False,
                              early_skip: bool = False, cabac: bool = False,
                              intra4x4: bool = False, partitions: bool = False,
                              target_size_mb: float | None = None, aq_strength: float = 0.0,
                              aq_max: int = 0) -> Path:
    """Same decisions and return values as the reference method: the input
    path when it is <= 30 MB, an existing non-empty compressed_<name> as is,
    otherwise the new compressed file, or the input path when compression
    is impossible.  `intra`, `subpel`, `deblock` and `deblock_offsets` are
    VideoScorer.transcode's: Intra16x16 instead of I_PCM intra macroblocks,
    half- (1) or quarter-sample (2) motion refinement, and the in-loop
    deblocking filter with its two slice offsets; `mvcost` and `early_skip`
    are its rate-aware motion cost and early P_Skip decision, `cabac` its
    CABAC entropy coding (a Main profile stream), `intra4x4` its Intra_4x4
    coding of intra macroblocks (needs `intra`), `partitions` its 16x8 / 8x16 /
    8x8 inter partitions (needs `mvcost`).  `target_size_mb`: the size the
    compressed file should not exceed; the video bitrate that leaves room for
    the copied tracks goes to the device's rate control (`bitrate_kbps`, with
    `mvcost`, which it needs).  No hit tolerance is promised: near the
    fixed-QP size the file lands within about a tenth of the target, far
    under it above the target (DESIGN.md §11 "Rate control"); target and
    achieved size are logged.  None: the fixed-QP call it was.  `aq_strength`
    > 0: its adaptive quantisation, a QP per macroblock from the variance of
    the source, offsets up to `aq_max` (0: 8); 0: every byte as before.  It
    needs `mvcost`, so, as `target_size_mb` does, it turns `mvcost` on for a
    caller who left it off (logged): the motion decisions are then the
    rate-aware ones, not only the quantiser differs."""
    log = logger or logging.getLogger(__name__)
    video_path = Path(video_path)
    file_size_mb = video_path.stat().st_size / (1024 * 1024)
    if file_size_mb <= max_size_mb:
        log.info(f"video {file_size_mb:.1f}MB <= {max_size_mb}MB, skipping compression")
        return video_path
    log.info(f"video {file_size_mb:.1f}MB > {max_size_mb}MB, compressing on the GPU...")
    out = compressed_path_for(video_path)
    if out.exists() and out.stat().st_size > 0:
        log.info(f"found existing compressed file {out.name}, skipping compression")
        return out
    video_only = out.with_name(out.name + ".video.tmp")
    try:
        from . import _lib
        from .scene import VideoScorer
        with VideoScorer(video_path, device=device) as v:
            rate = {}
            if target_size_mb is not None:
                kbps = target_bitrate_kbps(video_path, target_size_mb, float(v.info.duration))
                log.info(f"target {target_size_mb:.2f}MB: video at {kbps} kbps")
                rate = dict(bitrate_kbps=kbps)
                mvcost = True
            if aq_strength:
                rate.update(aq_strength=aq_strength, aq_max=aq_max)
                if not mvcost:
                    log.info("aq_strength needs mvcost: turned on")
                mvcost = True
            facts = v.transcode(video_only, intra=intra, subpel=subpel, deblock=deblock,
                                deblock_offsets=deblock_offsets, mvcost=mvcost, early_skip=early_skip,
                                cabac=cabac, intra4x4=intra4x4, partitions=partitions, **rate)
        # the source's audio / other tracks, stream-copied beside the new video
        _lib.check(_lib.lib().vts_add_tracks(str(video_only).encode(),
                                             str(video_path).encode(), str(out).encode()))
        video_only.unlink()
        facts["bytes_written"] = out.stat().st_size
    except (VtsegError, VtsegLibraryError, OSError, struct.error) as exc:   # struct.error: a malformed box table
        for p in (out, video_only):
            if p.exists():
                p.unlink()
        log.warning(f"GPU transcode unavailable ({exc}); using ffmpeg")
        if shutil.which("ffmpeg") is None:
            log.warning("ffmpeg not installed; skipping compression")
            return video_path
        return _ffmpeg(video_path, out, log)
    new_size_mb = facts["bytes_written"] / (1024 * 1024)
    log.info(f"compressed: {file_size_mb:.1f}MB -> {new_size_mb:.1f}MB "
             f"({new_size_mb / file_size_mb * 100:.0f}%)")
    if target_size_mb is not None:
        log.info(f"target {target_size_mb:.2f}MB, achieved {new_size_mb:.2f}MB "
                 f"({new_size_mb / target_size_mb * 100:.0f}% of the target; QP {facts['qp_lo']}..{facts['qp_hi']}, "
                 f"mean {facts['qp_mean']:.1f})")
    return out
