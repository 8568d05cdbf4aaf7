"""Frame-range re-encode (vts_transcode_ext8, DESIGN.md §11 "Segment re-encode").

The frames [f0, f1) of a decoded file, with their scene scores, are a byte
oracle for a segment: oracle.transcode(frames[f0:f1], ..., scores[f0:f1]) is
what the device must write for `frames=(f0, f1)`.  "Equal" below means every
sample byte, SPS and PPS, the IDR / macroblock counts, sample times i * delta,
`recon_hash` against the oracle's reconstruction and oracle.decode_full of the
output against that reconstruction.

Unless a test says otherwise the source is a 90-frame synthetic whose I_PCM
data holds emulation-prevention bytes (the subset decoder refuses it mid-run and
the session re-runs itself on the general decoder, keeping the range), opened
with 31-frame windows, and the range is [17, 64): not IDR-aligned, partial in
the first and last of three windows, what start = 0.55 s, end = 2.12 s give at
30 fps.  Output height = source height goes through the ratio-1 ingest kernel
(`ingest_nv12`), 320x192 with every 16-byte group whole, 328x180 (coded
336x192) with padded columns and rows and a group that crosses the width
(those two sources in one window, see `_window`).
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from test_remux import _audio_mp4, _tracks
from vtseg import VtsegError, _lib, scene
from vtseg import video_segmenter as vs

pytestmark = pytest.mark.gpu

SYNTH = dict(n_frames=90, cut_min_s=0.7, cut_max_s=1.5, gop_max_s=0.5, max_motion=4, pcm_zero_runs=True)
SOURCES = {
    "a": dict(SYNTH, width=320, height=192),
    "b": dict(SYNTH, width=328, height=180),
    "b40": dict(SYNTH, width=328, height=180, n_frames=40),
    "full": dict(width=320, height=240, n_frames=60, cut_min_s=0.7, cut_max_s=1.5, gop_max_s=0.8, seed=3,
                 coding="full", bframes=True, weighted="implicit"),
}
EVERY = dict(qp=23, keyint=16, intra=True, intra4x4=True, subpel=2, deblock=True, mvcost=True, early_skip=True)
RANGE = (17, 64)
WINDOW = 31
COUNTS = ("n_idr", "pcm_mbs", "inter_mbs", "skip_mbs", "intra_mbs", "intra4x4_mbs", "subpel_mbs", "qpel_mbs",
          "deblock_mbs", "early_skip_mbs")
HASHED = ("intra", "subpel", "deblock", "mvcost", "early_skip")


def _require_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires an MI355X")


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("segment"), "src": {}, "dec": {}, "ref": {}, "run": {}}


def _source(work, name):
    if name not in work["src"]:
        path = work["dir"] / f"{name}.mp4"
        scene.synth_write(path, **SOURCES[name])
        work["src"][name] = path
    return work["src"][name]


def _decoded(work, name):
    """The oracle's decode (presentation order) and scene scores of a source, once per module."""
    if name not in work["dec"]:
        path = _source(work, name)
        frames, info = oracle.decode_full(path) if name == "full" else oracle.decode_file(path)
        F, W, H = frames.shape[0], info["width"], info["height"]
        sc = oracle.score_frames(frames.reshape(-1), frames[0].size, F, W, H, W, H, 4, want_rgb=False)["score"]
        pts = sorted(info["pts"])
        work["dec"][name] = (frames, W, H, sc, int(pts[1] - pts[0]), info["timescale"])
    return work["dec"][name]


def _oracle_side(work, name, rng, tk):
    """oracle.transcode of the oracle's frames [f0, f1) and their scores, once per (source, range, settings)."""
    key = (name, rng, tuple(sorted(tk.items())))
    if key not in work["ref"]:
        frames, W, H, sc, _, _ = _decoded(work, name)
        f0, f1 = rng if rng else (0, frames.shape[0])
        kw = {k: v for k, v in tk.items() if k != "height"}
        work["ref"][key] = oracle.transcode(frames[f0:f1], W, H, sc[f0:f1], out_height=tk.get("height", 360),
                                            want_recon=True, **kw)
    return work["ref"][key]


def _samples(path):
    m = oracle.read_mp4(path)
    return m, [bytes(m["data"][o:o + s]) for o, s in zip(m["offsets"], m["sizes"])]


def _display(ref):
    sw, sh, ch = ref["width"], ref["height"], ref["coded_height"]
    rec = ref["recon"]
    return np.concatenate([rec[:, :sh, :sw], rec[:, ch:ch + sh // 2, :sw]], 1)


def _equal(work, name, rng, tk, out, facts):
    ref = _oracle_side(work, name, rng, tk)
    _, _, _, _, delta, timescale = _decoded(work, name)
    m, got = _samples(out)
    n = len(ref["samples"])
    print({k: facts[k] for k in COUNTS if k in facts}, sum(map(len, got)), "bytes; the oracle:",
          {k: ref[k] for k in COUNTS if k in ref}, sum(map(len, ref["samples"])), "bytes")
    assert (facts["width"], facts["height"], facts["n_frames"]) == (ref["width"], ref["height"], n)
    assert len(got) == n
    bad = [i for i in range(n) if got[i] != ref["samples"][i]]
    assert bad == [], f"samples {bad[:8]} differ from the oracle's"
    mbw, mbh = ref["coded_width"] // 16, ref["coded_height"] // 16
    sps, pps = oracle.sps_pps(mbw, mbh, ref["coded_width"] - ref["width"], ref["coded_height"] - ref["height"],
                              timescale / delta)
    assert m["sps"][0] == sps and m["pps"][0] == pps
    for k in COUNTS:
        if k in ref and k in facts:
            assert facts[k] == ref[k], k
    assert m["dts"] == [i * delta for i in range(n)]
    want = _display(ref)
    if any(tk.get(k) for k in HASHED):
        assert facts["recon_hash"] == oracle.recon_hash(want)
    else:
        assert facts["recon_hash"] == 0        # the base encoder computes none
    assert np.array_equal(oracle.decode_full(out)[0], want)
    return ref


def _window(name):
    """31-frame windows, but one window for the 328x180 sources: their 82x45 RGB thumbnails are 11070 bytes, a
    later window's thumbnails then start off a dword, and the scorer refuses that ("rgb not 4-aligned") with or
    without a transcode.  The ranges of those two cases still exercise the ingest kernel's padded paths; the
    windows are exercised on the other sources."""
    return 0 if name.startswith("b") else WINDOW


def _device(work, name, rng, tk, tag, **more):
    """The device's transcode in a fresh session, once per tag; (path, facts)."""
    if tag not in work["run"]:
        out = work["dir"] / f"{tag}.mp4"
        with scene.VideoScorer(_source(work, name), window_frames=_window(name)) as v:
            kw = dict(frames=rng) if rng else {}
            facts = v.transcode(out, **kw, **tk, **more)
            facts["general"], facts["windows"] = v.general(), v.windows()
        work["run"][tag] = (out, facts)
    return work["run"][tag]


# ----------------------------------------------------------------- 1 .. 5
def test_range_at_source_height_whole_groups(work):
    """320x192 at height 192: the ratio-1 kernel with every group whole."""
    _require_gpu()
    tk = dict(height=192, **EVERY)
    out, facts = _device(work, "a", RANGE, tk, "case1", want_commands=True)
    ref = _equal(work, "a", RANGE, tk, out, facts)
    assert (facts["frame_first"], facts["frame_count"]) == (17, 47)
    assert facts["commands"].shape == (47, 12, 20)
    print("windows:", facts["windows"], "general decoder:", facts["general"])
    assert facts["windows"] >= 3       # the range begins inside one window and ends inside a later one
    # the input exercises what the test names (the oracle's own numbers)
    assert ref["n_idr"] == 3 and ref["intra4x4_mbs"] > 0 and ref["inter_mbs"] > 0 and ref["skip_mbs"] > 0
    assert ref["subpel_mbs"] > 0 and sum(map(len, ref["samples"])) == 58216


def test_range_at_source_height_padded_picture(work):
    """328x180 at height 180 (coded 336x192): 8 padded columns, 12 padded rows, a group crossing the width."""
    _require_gpu()
    tk = dict(height=180, **EVERY)
    out, facts = _device(work, "b", RANGE, tk, "case2")
    ref = _equal(work, "b", RANGE, tk, out, facts)
    assert (ref["width"], ref["height"], ref["coded_width"], ref["coded_height"]) == (328, 180, 336, 192)
    assert ref["n_idr"] == 3 and sum(map(len, ref["samples"])) == 65505


def test_range_through_the_box_path(work):
    """320x192 at height 96, default options: the K = 2 box kernel and the plain oracle entry."""
    _require_gpu()
    tk = dict(height=96)
    out, facts = _device(work, "a", RANGE, tk, "case3")
    _equal(work, "a", RANGE, tk, out, facts)


def test_range_on_the_general_decoder(work):
    """B pictures with implicit weights: the range counts presentation order."""
    _require_gpu()
    tk = dict(height=240, **EVERY)
    out, facts = _device(work, "full", (13, 41), tk, "case4")
    assert facts["general"]
    _equal(work, "full", (13, 41), tk, out, facts)


def test_whole_file_at_source_height(work):
    """No range, 328x180, 40 frames: the ingest kernel writes what the tap path wrote (the oracle's bytes)."""
    _require_gpu()
    tk = dict(height=180, **EVERY)
    out, facts = _device(work, "b40", None, tk, "case5")
    assert "frame_first" not in facts
    _equal(work, "b40", None, tk, out, facts)


# --------------------------------------------------------------------- 6, 7
def test_the_whole_range_is_the_call_without_one(work):
    _require_gpu()
    tk = dict(height=96, **EVERY)
    plain, _ = _device(work, "a", None, tk, "case6_plain")
    ranged, facts = _device(work, "a", (0, 90), tk, "case6_range")
    assert (facts["frame_first"], facts["frame_count"], facts["n_frames"]) == (0, 90, 90)
    assert ranged.read_bytes() == plain.read_bytes()


def test_one_session_changes_its_range(work):
    """[17, 64), [5, 80), the whole file, [17, 64) again (the store kept, its range moved), then score()."""
    _require_gpu()
    tk = dict(height=192, **EVERY)
    fresh = {RANGE: _device(work, "a", RANGE, tk, "case1", want_commands=True)[0],
             (5, 80): _device(work, "a", (5, 80), tk, "case7_5_80")[0],
             None: _device(work, "a", None, tk, "case7_whole")[0]}
    with scene.VideoScorer(_source(work, "a"), window_frames=WINDOW) as v:
        before = v.score()
        for i, rng in enumerate((RANGE, (5, 80), None, RANGE)):
            out = work["dir"] / f"case7_session_{i}.mp4"
            facts = v.transcode(out, **(dict(frames=rng) if rng else {}), **tk)
            assert facts["n_frames"] == (rng[1] - rng[0] if rng else 90)
            assert out.read_bytes() == fresh[rng].read_bytes(), f"call {i}, range {rng}"
        after = v.score()
    assert np.array_equal(before.scores, after.scores) and np.array_equal(before.sad, after.sad)
    assert np.array_equal(before.hist, after.hist)
    sc = _decoded(work, "a")[3]
    assert np.array_equal(after.scores, sc)


# ------------------------------------------------------------------------ 8
def test_cabac_codes_what_cavlc_codes_on_a_range(work):
    _require_gpu()
    tk = dict(height=192, **EVERY)
    cavlc, a = _device(work, "a", RANGE, tk, "case1", want_commands=True)
    cabac, b = _device(work, "a", RANGE, dict(tk, cabac=True), "case8", want_commands=True)
    for k in COUNTS + ("n_frames", "width", "height", "recon_hash", "frame_first", "frame_count"):
        assert a[k] == b[k], k
    assert np.array_equal(a["commands"], b["commands"])
    assert cabac.read_bytes() != cavlc.read_bytes()
    fa, fb = oracle.decode_full(cavlc)[0], oracle.decode_full(cabac)[0]
    assert fa.shape[0] == 47 and np.array_equal(fa, fb)


# -------------------------------------------------------------------- 9, 10
def _kept_span(work):
    _, _, _, _, delta, ts = _decoded(work, "a")
    return RANGE[0] * delta / ts, ((RANGE[1] - 1) * delta + delta) / ts


def test_transcode_segment_keeps_the_audio_of_the_span(work, tmp_path):
    _require_gpu()
    audio, src, out, cut = (tmp_path / n for n in ("a.mp4", "clip.mp4", "seg.mp4", "cut.mp4"))
    _audio_mp4(audio, 141)                                     # 3.008 s beside 3 s of video
    _lib.check(_lib.lib().vts_add_tracks(str(_source(work, "a")).encode(), str(audio).encode(), str(src).encode()))
    with scene.VideoScorer(src, window_frames=WINDOW) as v:
        facts = v.transcode_segment(out, 0.55, 2.12)
    t0, t1 = _kept_span(work)
    assert (facts["frame_first"], facts["frame_count"], facts["start"], facts["end"]) == (17, 47, t0, t1)
    assert (facts["width"], facts["height"]) == (320, 192) and facts["bytes_written"] == out.stat().st_size
    _lib.check(_lib.lib().vts_extract_segment(str(src).encode(), t0, t1, str(cut).encode()))
    got, want = _tracks(out), _tracks(cut)
    assert [h for h, _ in got] == [b"vide", b"soun"]
    assert len(got[0][1]) == 47
    assert got[1][1] == want[1][1] and len(got[1][1]) > 0
    # the video is the range's, by the default options' oracle
    ref = _oracle_side(work, "a", RANGE, dict(height=192))
    assert got[0][1] == ref["samples"]
    data = out.read_bytes()
    assert [t for t, _, _ in oracle._boxes(data, 0, len(data))][:2] == ["ftyp", "moov"]
    assert not list(tmp_path.glob("*.tmp"))
    # nothing in range: an error, and nothing left behind
    with scene.VideoScorer(src, window_frames=WINDOW) as v:
        with pytest.raises(VtsegError):
            v.transcode_segment(tmp_path / "none.mp4", 2.12, 2.12)
        with pytest.raises(VtsegError):
            v.transcode_segment(tmp_path / "none.mp4", 5.0, 6.0)
    assert not (tmp_path / "none.mp4").exists() and not list(tmp_path.glob("*.tmp"))


def test_extract_segment_with_the_device_reencode(work, tmp_path, monkeypatch):
    _require_gpu()
    src = _source(work, "a")
    monkeypatch.setenv("PATH", str(tmp_path))                   # no ffmpeg
    cavlc, cabac, none = tmp_path / "seg" / "cavlc.mp4", tmp_path / "seg" / "cabac.mp4", tmp_path / "seg" / "none.mp4"
    assert vs.extract_segment(src, 0.55, 2.12, cavlc, stream_copy=False, device_reencode=True,
                              encoder=dict(cabac=False)) is True
    tk = {k: v for k, v in vs.SEGMENT_ENCODER.items() if k != "cabac"}
    ref = _oracle_side(work, "a", RANGE, dict(height=192, **tk))
    m, got = _samples(cavlc)
    assert got == ref["samples"]
    assert m["dts"] == [i * 1000 for i in range(47)]
    assert vs.extract_segment(src, 0.55, 2.12, cabac, stream_copy=False, device_reencode=True) is True
    assert cabac.read_bytes() != cavlc.read_bytes()
    assert np.array_equal(oracle.decode_full(cabac)[0], oracle.decode_full(cavlc)[0])
    assert np.array_equal(oracle.decode_full(cavlc)[0], _display(ref))
    assert vs.extract_segment(src, 0.55, 2.12, none, stream_copy=False, device_reencode=False) is False
    assert vs.extract_segment(src, 5.0, 6.0, none, stream_copy=False, device_reencode=True) is False   # past the end
    assert not none.exists() and not list((tmp_path / "seg").glob("*.tmp"))


# ----------------------------------------------------------------------- 11
def test_range_errors_name_the_field_and_leave_the_session_usable(work, tmp_path):
    _require_gpu()
    tk = dict(height=192, **EVERY)
    fresh, _ = _device(work, "a", RANGE, tk, "case1", want_commands=True)
    out = tmp_path / "x.mp4"
    with scene.VideoScorer(_source(work, "a"), window_frames=WINDOW) as v:
        for rng, field in (((90, 90), "frame_first"), ((-1, 5), "frame_first"), ((10, 91), "frame_count"),
                           ((95, 99), "frame_first"), ((20, 10), "frame_count"), ((20, 20), "frame_count")):
            with pytest.raises(VtsegError) as err:
                v.transcode(out, frames=rng, **tk)
            assert err.value.code == _lib.VTS_E_INVALID and field in err.value.message, (rng, err.value.message)
        with pytest.raises(VtsegError) as err:      # frame_qp counts the range's frames
            v.transcode(out, frames=RANGE, frame_qp=[23] * 90, **tk)
        assert err.value.code == _lib.VTS_E_INVALID and "frame_qp_n" in err.value.message
        assert not out.exists()
        facts = v.transcode(out, frames=RANGE, frame_qp=[23] * 47, **tk)    # a constant frame_qp: the bytes at that qp
        assert facts["frame_qp"].shape == (47,) and facts["frame_bits"].shape == (47,)
        assert out.read_bytes() == fresh.read_bytes()
        v.transcode(out, frames=RANGE, **tk)
        assert out.read_bytes() == fresh.read_bytes()
