"""vts_add_tracks_range (no GPU): a new video copied whole beside the source's
other tracks cut to [start, end) by the stream-copy cutter's own rule, which is
what the device re-encode of a segment keeps of the source's audio
(DESIGN.md §11 "Segment re-encode")."""
from __future__ import annotations

import struct
from pathlib import Path

import pytest

import oracle
from test_remux import _audio_mp4, _tracks
from vtseg import VtsegError, _lib, scene


def _call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*[str(a).encode() if isinstance(a, Path) else a for a in args]))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("range")
    video, audio, src = d / "v.mp4", d / "a.mp4", d / "src.mp4"
    scene.synth_write(video, width=64, height=48, n_frames=60)
    samples = _audio_mp4(audio, 94)
    _call("vts_add_tracks", video, audio, src)        # the "downloaded" file: video + audio
    new_video = d / "n.mp4"                           # stands for the re-encoded range
    scene.synth_write(new_video, width=32, height=32, n_frames=25, seed=9)
    return {"dir": d, "src": src, "video": new_video, "audio_samples": samples}


def _timing(path, handler):
    """(elst entries as (duration, media_time), mdhd duration, tkhd duration) of the first track of `handler`."""
    data = Path(path).read_bytes()
    top = {t: (a, b) for t, a, b in oracle._boxes(data, 0, len(data))}
    kids = lambda a, b: {n: (x, y) for n, x, y in oracle._boxes(data, a, b)}  # noqa: E731
    for t, ta, tb in oracle._boxes(data, *top["moov"]):
        if t != "trak":
            continue
        trak = kids(ta, tb)
        mdia = kids(*trak["mdia"])
        hd = mdia["hdlr"][0]
        if data[hd + 8:hd + 12] != handler:
            continue
        el = kids(*trak["edts"])["elst"][0]
        assert data[el] == 1                                           # version 1: 64-bit entries
        n = struct.unpack(">I", data[el + 4:el + 8])[0]
        entries = [struct.unpack(">Qq", data[el + 8 + 20 * i:el + 24 + 20 * i]) for i in range(n)]
        md = mdia["mdhd"][0]
        assert data[md] == 1
        mdhd_duration = struct.unpack(">Q", data[md + 24:md + 32])[0]
        tk = trak["tkhd"][0]
        assert data[tk] == 1
        tkhd_duration = struct.unpack(">Q", data[tk + 28:tk + 36])[0]
        return entries, mdhd_duration, tkhd_duration
    raise AssertionError(f"no {handler!r} track in {path}")


def test_other_tracks_are_cut_as_the_stream_copy_cuts_them(files):
    out, cut = files["dir"] / "out.mp4", files["dir"] / "cut.mp4"
    _call("vts_add_tracks_range", files["video"], files["src"], 0.55, 1.4, out)
    _call("vts_extract_segment", files["src"], 0.55, 1.4, cut)
    got, want = _tracks(out), _tracks(cut)
    assert [h for h, _ in got] == [b"vide", b"soun"] and [h for h, _ in want] == [b"vide", b"soun"]
    # the video file's samples, whole
    assert got[0][1] == _tracks(files["video"])[0][1] and len(got[0][1]) == 25
    # the audio: the cutter's samples and timing; 1024 / 48000 s a sample, so 0.55 s lies in sample 25
    assert got[1][1] == want[1][1]
    assert got[1][1] == files["audio_samples"][25:66]
    assert _timing(out, b"soun") == _timing(cut, b"soun")
    entries, mdhd_duration, _ = _timing(out, b"soun")
    assert entries == [(850, 26400 - 25 * 1024)] and mdhd_duration == 41 * 1024
    # ftyp then moov lead the file
    data = out.read_bytes()
    order = [t for t, _, _ in oracle._boxes(data, 0, len(data))]
    assert order[:2] == ["ftyp", "moov"] and order[-1] == "mdat"
    # and the video still reads as the video file does
    a, b = oracle.read_mp4(out), oracle.read_mp4(files["video"])
    assert a["dts"] == b["dts"] and a["sps"] == b["sps"] and a["sizes"] == b["sizes"]


def test_a_range_past_the_audio_drops_the_track(files):
    out = files["dir"] / "late.mp4"
    _call("vts_add_tracks_range", files["video"], files["src"], 3.0, 4.0, out)   # the audio ends at 2.005 s
    got = _tracks(out)
    assert [h for h, _ in got] == [b"vide"]
    assert got[0][1] == _tracks(files["video"])[0][1]


@pytest.mark.parametrize("start,end", [(1.0, 1.0), (1.5, 0.5), (float("nan"), 1.0)])
def test_an_empty_range_fails(files, start, end):
    out = files["dir"] / "none.mp4"
    with pytest.raises(VtsegError) as err:
        _call("vts_add_tracks_range", files["video"], files["src"], start, end, out)
    assert err.value.code == _lib.VTS_E_INVALID and "range" in err.value.message
    assert not out.exists()


def test_whole_copy_is_unchanged(files):
    """vts_add_tracks writes what it wrote: every audio sample, and the bytes of a range that covers everything."""
    whole, ranged = files["dir"] / "whole.mp4", files["dir"] / "ranged.mp4"
    _call("vts_add_tracks", files["video"], files["src"], whole)
    got = _tracks(whole)
    assert [h for h, _ in got] == [b"vide", b"soun"] and got[1][1] == files["audio_samples"]
    assert _timing(whole, b"soun") == ([(2005, 0)], 94 * 1024, 2005)
    _call("vts_add_tracks_range", files["video"], files["src"], 0.0, 1e9, ranged)
    assert ranged.read_bytes() == whole.read_bytes()
