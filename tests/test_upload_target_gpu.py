"""compress_video_for_upload(target_size_mb=...): the video bitrate that leaves
room for the copied tracks goes to the device's rate control (DESIGN.md §11
"Rate control"); the result decodes and the target and the achieved size are
logged."""
from __future__ import annotations

import logging

import pytest

import oracle
from test_remux import _audio_mp4
from test_transcode_subpel_gpu import _require_gpu
from vtseg import _lib, scene, upload

pytestmark = pytest.mark.gpu


def test_target_size_reaches_the_rate_control_and_is_logged(tmp_path, caplog):
    _require_gpu()
    video = tmp_path / "v.mp4"
    scene.synth_write(video, width=640, height=360, n_frames=30, cut_min_s=0.7, cut_max_s=1.5, gop_max_s=0.5)
    audio = tmp_path / "a.mp4"
    samples = _audio_mp4(audio, 45)
    src = tmp_path / "clip.mp4"
    _lib.check(_lib.lib().vts_add_tracks(str(video).encode(), str(audio).encode(), str(src).encode()))
    # what vts_add_tracks will copy is what the video's budget leaves out
    assert upload.other_tracks_bytes(src) == sum(len(s) for s in samples) > 0
    assert upload.other_tracks_bytes(video) == 0
    with scene.VideoScorer(src) as v:
        duration = float(v.info.duration)
    target = 0.25
    kbps = upload.target_bitrate_kbps(src, target, duration)
    assert kbps == int((int(target * 1024 * 1024) - upload.other_tracks_bytes(src)) * 8 / duration / 1000) >= 1
    assert upload.target_bitrate_kbps(src, 1e-6, duration) == 1          # never below 1 kbps
    log = logging.getLogger("upload_target_test")
    with caplog.at_level(logging.INFO, logger=log.name):
        out = upload.compress_video_for_upload(src, logger=log, max_size_mb=0.05, intra=True, subpel=2,
                                               target_size_mb=target)
    assert out == tmp_path / "compressed_clip.mp4" and out.stat().st_size > 0
    frames, info = oracle.decode_full(out)
    assert frames.shape[0] == 30 and info["height"] == 360
    text = "\n".join(r.getMessage() for r in caplog.records)
    size_mb = out.stat().st_size / (1024 * 1024)
    assert f"target {target:.2f}MB: video at {kbps} kbps" in text
    assert f"target {target:.2f}MB, achieved {size_mb:.2f}MB" in text
    print(text)
    # the call without the keyword is the fixed-QP one it was: no target in its log
    out.unlink()
    caplog.clear()
    with caplog.at_level(logging.INFO, logger=log.name):
        again = upload.compress_video_for_upload(src, logger=log, max_size_mb=0.05, intra=True, subpel=2)
    assert again == out and "target" not in "\n".join(r.getMessage() for r in caplog.records)
