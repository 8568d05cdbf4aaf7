"""Paired reconstruction (h264_recon_score_pair) vs the C
oracle.

The default schedule of an eligible session decodes a GOP's P levels two per
launch: the first level of a pair goes from the HBM reference into registers
and on to the second through LDS, and is not stored.  Scores, histograms,
SADs, RGB thumbnails and scene cuts must equal the oracle's bit for bit;
every frame must still be readable (the session then decodes once more with
one launch per level and stays there); motion beyond the one-group halo must
fall back to per-level launches with identical results; sessions the schedule
does not apply to must not run it.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from vtseg import scene

pytestmark = pytest.mark.gpu


def _require_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires an MI355X")


def _pair_launches(v) -> int:
    return int(v._lib.vts_schedule_info(v._ctx, 15))


def _pair_chains(v) -> int:
    return int(v._lib.vts_schedule_info(v._ctx, 16))


def _tb_launches(v) -> int:
    return int(v._lib.vts_schedule_info(v._ctx, 5))


def _stream(path, n, k=4, **kw):
    scene.synth_write(path, n_frames=n, **kw)
    frames, _ = oracle.decode_file(path)
    ref = oracle.score_frames(frames.reshape(-1), frames[0].size, n, kw["width"], kw["height"],
                              kw["width"], kw["height"], k, want_rgb=True)
    return path, frames, ref


def _results(v, n, k=4):
    res = v.score()
    rgb = np.stack([v.thumbnail_rgb(i, k) for i in range(n)]).reshape(-1)
    return res, rgb, v.scene_cuts()


def _check(got, ref):
    res, rgb, cuts = got
    assert np.array_equal(rgb, ref["rgb"])
    assert np.array_equal(res.hist, ref["hist"])
    assert np.array_equal(res.sad, ref["sad"])
    assert np.array_equal(res.scores, ref["score"])
    assert cuts == list(np.nonzero(ref["score"] > scene.DEFAULT_CUT_THRESHOLD)[0])


N_SHORT = 150


@pytest.fixture(scope="module")
def short_gops(tmp_path_factory):
    """320x240, GOPs of odd and even length (1-3 frames among them), I_PCM
    sparkles in halo rows, half-pel chroma, edge clamping."""
    _require_gpu()  # before the library loads: it binds to the HIP runtime torch brings
    path = tmp_path_factory.mktemp("pair") / "s.mp4"
    return _stream(path, N_SHORT, width=320, height=240, max_motion=4, odd_motion=True,
                   cut_min_s=0.5, cut_max_s=1.5, gop_max_s=0.9, slices_per_row=2)


def test_default_session_runs_pairs(short_gops):
    _require_gpu()
    path, frames, ref = short_gops
    with scene.VideoScorer(path) as v:
        assert _pair_launches(v) > 0
        assert _pair_chains(v) >= _pair_launches(v)
        assert _tb_launches(v) == 0
        got = _results(v, N_SHORT)
        assert _pair_launches(v) > 0  # motion <= 4 rows: no fallback
        assert _tb_launches(v) == 0
    _check(got, ref)


def test_every_frame_readable_on_default_session(short_gops):
    """Frames the paired launches did not store are served after one more run
    with per-level launches; the scoring results after that are the same."""
    _require_gpu()
    path, frames, ref = short_gops
    with scene.VideoScorer(path) as v:
        v.run()
        assert _pair_launches(v) > 0
        for i in range(N_SHORT):
            assert np.array_equal(v.frame_nv12(i).reshape(frames[i].shape), frames[i]), i
        assert _pair_launches(v) == 0  # the session stays per-level
        got = _results(v, N_SHORT)
    _check(got, ref)


@pytest.mark.parametrize("motion", [8, 24])
def test_motion_beyond_halo_falls_back(tmp_path, motion):
    _require_gpu()
    n = 90
    path, frames, ref = _stream(tmp_path / "m.mp4", n, width=320, height=240, max_motion=motion,
                                cut_min_s=0.5, cut_max_s=1.2, gop_max_s=0.8)
    with scene.VideoScorer(path) as v:
        assert _pair_launches(v) > 0
        got = _results(v, n)
        if motion > 16:  # pans of more than 4 rows per frame certainly occur
            assert _pair_launches(v) == 0
        for i in range(n):
            assert np.array_equal(v.frame_nv12(i).reshape(frames[i].shape), frames[i]), i
    _check(got, ref)


def test_windows_over_two_rings_and_repeat(tmp_path):
    _require_gpu()
    n = 400
    path, frames, ref = _stream(tmp_path / "w.mp4", n, width=480, height=272, max_motion=2,
                                cut_min_s=1, cut_max_s=4, gop_max_s=0.5)
    with scene.VideoScorer(path, window_frames=40, n_streams=2) as v:
        assert v.windows() > 2
        a = _results(v, n)
        assert _pair_launches(v) > 0
        v.run()
        b = _results(v, n)
        assert _pair_launches(v) > 0
    _check(a, ref)
    _check(b, ref)


def test_hd720(tmp_path):
    """The benchmark's shape: 80 macroblocks a row, 480 level-A tasks."""
    _require_gpu()
    n = 70
    path, frames, ref = _stream(tmp_path / "hd.mp4", n, width=1280, height=720, max_motion=4,
                                cut_min_s=0.5, cut_max_s=1.5, gop_max_s=1.0)
    with scene.VideoScorer(path) as v:
        got = _results(v, n)
        assert _pair_launches(v) > 0
        # the last frame of a GOP is always stored
        assert np.array_equal(v.frame_nv12(n - 1).reshape(frames[-1].shape), frames[-1])
        assert _pair_launches(v) > 0
    _check(got, ref)


@pytest.mark.parametrize("width,height", [(256, 144), (256, 16)], ids=["9rows", "1row"])
def test_smallest_band_geometry(tmp_path, width, height):
    """Nine macroblock rows (halo clipped at the top and the bottom band), and
    a picture of one band whose halo is clipped on both sides."""
    _require_gpu()
    n = 90
    path, frames, ref = _stream(tmp_path / "b.mp4", n, width=width, height=height, max_motion=4,
                                odd_motion=True, cut_min_s=0.6, cut_max_s=1.2, gop_max_s=0.8)
    with scene.VideoScorer(path) as v:
        got = _results(v, n)
        assert _pair_launches(v) > 0
    _check(got, ref)
    with scene.VideoScorer(path) as v:
        v.run()
        for i in range(n):
            assert np.array_equal(v.frame_nv12(i).reshape(frames[i].shape), frames[i]), i


@pytest.mark.parametrize("kw", [dict(level_block=1), dict(keep_frames=True)], ids=["level_block1", "keep_frames"])
def test_other_settings_stay_per_level(short_gops, kw):
    _require_gpu()
    path, frames, ref = short_gops
    with scene.VideoScorer(path, **kw) as v:
        assert _pair_launches(v) == 0 and _pair_chains(v) == 0
        got = _results(v, N_SHORT)
        assert _pair_launches(v) == 0
        for i in range(0, N_SHORT, 7):
            assert np.array_equal(v.frame_nv12(i).reshape(frames[i].shape), frames[i]), i
    _check(got, ref)


def test_k6_session_stays_per_level(tmp_path):
    _require_gpu()
    n = 24
    path, frames, ref = _stream(tmp_path / "fhd.mp4", n, k=6, width=1920, height=1080, max_motion=4,
                                cut_min_s=0.3, cut_max_s=0.6, gop_max_s=0.5)
    with scene.VideoScorer(path) as v:
        assert v.fused()
        assert _pair_launches(v) == 0
        got = _results(v, n, 6)
        assert _pair_launches(v) == 0
    _check(got, ref)
