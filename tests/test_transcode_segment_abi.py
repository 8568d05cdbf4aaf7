"""The frame range of the upload transcode at the ABI (no GPU): two structs that
begin with `vts_transcode_ext7` / `vts_transcode_ext_info6` and travel through
the existing `vts_transcode_ex`, beside an unchanged version 9 and the unchanged
older structs, and the Python keywords that reach them (DESIGN.md §11 "Segment
re-encode")."""
from __future__ import annotations

import ctypes as C
import inspect
import subprocess
from pathlib import Path

from vtseg import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtseg.h"

EXT8 = ([("base", 0), ("frame_first", 168), ("frame_count", 176)], 184)
INFO7 = ([("base", 0), ("frame_first", 128), ("frame_count", 136)], 144)


def test_new_structs_have_the_stated_layout():
    for py, (fields, size) in ((_lib.TranscodeExt8, EXT8), (_lib.TranscodeExtInfo7, INFO7)):
        assert [n for n, _ in py._fields_] == [n for n, _ in fields]
        for n, off in fields:
            assert getattr(py, n).offset == off, n
        assert C.sizeof(py) == size
    f8, i7 = dict(_lib.TranscodeExt8._fields_), dict(_lib.TranscodeExtInfo7._fields_)
    assert f8["base"] is _lib.TranscodeExt7 and i7["base"] is _lib.TranscodeExtInfo6
    assert all(f[n] is C.c_int64 for f in (f8, i7) for n in ("frame_first", "frame_count"))


def test_old_structs_and_the_version_are_unchanged():
    assert C.sizeof(_lib.TranscodeExt) == 8 and C.sizeof(_lib.TranscodeExtInfo) == 24
    assert C.sizeof(_lib.TranscodeExt2) == 24 and C.sizeof(_lib.TranscodeExtInfo2) == 32
    assert C.sizeof(_lib.TranscodeExt3) == 56 and C.sizeof(_lib.TranscodeExtInfo3) == 48
    assert C.sizeof(_lib.TranscodeExt4) == 64
    assert C.sizeof(_lib.TranscodeExt5) == 88 and C.sizeof(_lib.TranscodeExtInfo4) == 64
    assert C.sizeof(_lib.TranscodeExt6) == 112 and C.sizeof(_lib.TranscodeExtInfo5) == 96
    assert C.sizeof(_lib.TranscodeExt7) == 168 and C.sizeof(_lib.TranscodeExtInfo6) == 128
    assert _lib.ABI_VERSION == 9 and _lib.lib().vts_abi_version() == 9
    # no new transcode entry point: the structs go through vts_transcode_ex by pointer cast
    assert [n for n in _lib.SIGNATURES if "transcode" in n] == ["vts_transcode", "vts_transcode_ex"]
    so = Path(_lib.__file__).resolve().parent / "libvtseg.so"
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], check=True, capture_output=True, text=True).stdout
    exported = [line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("vts_")]
    assert sorted(n for n in exported if "transcode" in n) == ["vts_transcode", "vts_transcode_ex"]
    # the one new entry point, declared and exported
    assert "vts_add_tracks_range" in exported and "vts_add_tracks_range" in _lib.SIGNATURES
    assert "int vts_add_tracks_range(const char *video_path, const char *src_path, double start," in HEADER.read_text()
    assert _lib.SIGNATURES["vts_add_tracks_range"] == (
        C.c_int, [C.c_char_p, C.c_char_p, C.c_double, C.c_double, C.c_char_p])


def test_structs_match_the_header(tmp_path):
    """Sizes and offsets equal a gcc probe compiled against include/vtseg.h."""
    structs = {"vts_transcode_ext8": _lib.TranscodeExt8, "vts_transcode_ext_info7": _lib.TranscodeExtInfo7,
               "vts_transcode_ext7": _lib.TranscodeExt7, "vts_transcode_ext_info6": _lib.TranscodeExtInfo6}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"',
             "int main(void) {", 'printf("abi %d\\n", VTS_ABI_VERSION);']
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True,
               capture_output=True, text=True).stdout.splitlines())
    assert int(got["abi"]) == 9
    assert int(got["vts_transcode_ext8"]) == 184 and int(got["vts_transcode_ext_info7"]) == 144
    assert int(got["vts_transcode_ext7"]) == 168 and int(got["vts_transcode_ext_info6"]) == 128
    for fields, cname in ((EXT8[0], "vts_transcode_ext8"), (INFO7[0], "vts_transcode_ext_info7")):
        for n, off in fields:
            assert int(got[f"{cname}.{n}"]) == off, (cname, n)
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)


def test_python_entry_points_accept_the_keywords():
    from vtseg import dropin, scene
    from vtseg import video_segmenter as vs
    tr = inspect.signature(scene.VideoScorer.transcode).parameters
    assert tr["frames"].kind is inspect.Parameter.KEYWORD_ONLY and tr["frames"].default is None
    # the earlier keywords stay what they were
    for name in ("intra", "deblock", "mvcost", "early_skip", "cabac", "intra4x4", "partitions", "want_rate"):
        assert tr[name].default is False
    assert tr["height"].default == 360 and tr["qp"].default == 28 and tr["frame_qp"].default is None
    ts = inspect.signature(scene.VideoScorer.transcode_segment).parameters
    assert list(ts)[:4] == ["self", "out_path", "start", "end"]
    assert ts["height"].kind is inspect.Parameter.KEYWORD_ONLY and ts["height"].default == 0
    assert ts["encoder"].kind is inspect.Parameter.VAR_KEYWORD
    ex = inspect.signature(vs.extract_segment).parameters
    assert list(ex)[:5] == ["input_path", "start", "end", "output_path", "stream_copy"]
    assert all(ex[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in list(ex)[:5])
    assert [ex[n].default for n in list(ex)[:5]] == [inspect.Parameter.empty] * 4 + [True]
    for name, default in (("device_reencode", False), ("device", 0), ("encoder", None)):
        assert ex[name].kind is inspect.Parameter.KEYWORD_ONLY and ex[name].default == default, name
    assert vs.SEGMENT_ENCODER == dict(qp=23, intra=True, intra4x4=True, subpel=2, deblock=True, mvcost=True,
                                      early_skip=True, cabac=True)
    assert set(vs.SEGMENT_ENCODER) <= set(tr)
    ins = inspect.signature(dropin.install).parameters
    assert ins["segment_reencode"].default is False and ins["upload_transcode"].default is False


def test_install_binds_the_reencoding_extract_segment():
    import sys

    from vtseg import dropin
    from vtseg import video_segmenter as vs
    plain = vs.extract_segment
    saved = {n: sys.modules.get(n) for n in dropin.MODULES}
    try:
        dropin.install(segment_reencode=True)
        bound = sys.modules["utils.video_segmenter"].extract_segment
        assert bound is not plain
        assert list(inspect.signature(bound).parameters) == ["input_path", "start", "end", "output_path", "stream_copy"]
        dropin.install()
        assert sys.modules["utils.video_segmenter"].extract_segment is plain
    finally:
        vs.extract_segment = plain
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def test_without_the_device_reencode_nothing_changes(tmp_path, monkeypatch):
    """device_reencode=False, no ffmpeg on PATH, stream_copy=False: still False, and nothing is left behind."""
    from vtseg import scene
    from vtseg import video_segmenter as vs
    src, out = tmp_path / "in.mp4", tmp_path / "seg" / "out.mp4"
    scene.synth_write(src, width=64, height=48, n_frames=30)
    monkeypatch.setenv("PATH", str(tmp_path))
    assert vs.extract_segment(src, 0.2, 0.8, out, stream_copy=False) is False
    assert vs.extract_segment(src, 0.2, 0.8, out, False, device_reencode=False) is False
    assert not out.exists() and not list(out.parent.glob("*.tmp"))
    # the copy is what it was
    assert vs.extract_segment(src, 0.2, 0.8, out) is True
