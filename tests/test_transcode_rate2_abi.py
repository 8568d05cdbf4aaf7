"""Per-picture QP and rate control of the upload transcode at the ABI (no GPU):
two structs that begin with `vts_transcode_ext6` / `vts_transcode_ext_info5`
and travel through the existing `vts_transcode_ex`, beside an unchanged
version 9 and the unchanged older structs, and the Python keywords that reach
them (DESIGN.md §11 "Rate control")."""
from __future__ import annotations

import ctypes as C
import inspect
import subprocess
from pathlib import Path

from vtseg import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtseg.h"

EXT7 = ([("base", 0), ("bitrate_kbps", 112), ("qp_min", 116), ("qp_max", 120), ("_pad5", 124), ("frame_qp", 128),
         ("frame_qp_n", 136), ("qp_out", 144), ("bits_out", 152), ("frame_cap", 160)], 168)
INFO6 = ([("base", 0), ("qp_sum", 96), ("qp_lo", 104), ("qp_hi", 108), ("est_bits", 112), ("frame_words", 120)], 128)


def test_new_structs_have_the_stated_layout():
    for py, (fields, size) in ((_lib.TranscodeExt7, EXT7), (_lib.TranscodeExtInfo6, INFO6)):
        assert [n for n, _ in py._fields_] == [n for n, _ in fields]
        for n, off in fields:
            assert getattr(py, n).offset == off, n
        assert C.sizeof(py) == size
    f7, i6 = dict(_lib.TranscodeExt7._fields_), dict(_lib.TranscodeExtInfo6._fields_)
    assert f7["base"] is _lib.TranscodeExt6
    assert all(f7[n] is C.c_int32 for n in ("bitrate_kbps", "qp_min", "qp_max", "_pad5"))
    assert f7["frame_qp"] is C.POINTER(C.c_uint8) and f7["qp_out"] is C.POINTER(C.c_uint8)
    assert f7["bits_out"] is C.POINTER(C.c_uint32)
    assert f7["frame_qp_n"] is C.c_int64 and f7["frame_cap"] is C.c_int64
    assert i6["base"] is _lib.TranscodeExtInfo5
    assert all(i6[n] is C.c_int64 for n in ("qp_sum", "est_bits", "frame_words"))
    assert i6["qp_lo"] is C.c_int32 and i6["qp_hi"] is C.c_int32


def test_old_structs_and_the_version_are_unchanged():
    assert C.sizeof(_lib.TranscodeExt) == 8 and C.sizeof(_lib.TranscodeExtInfo) == 24
    assert C.sizeof(_lib.TranscodeExt2) == 24 and C.sizeof(_lib.TranscodeExtInfo2) == 32
    assert C.sizeof(_lib.TranscodeExt3) == 56 and C.sizeof(_lib.TranscodeExtInfo3) == 48
    assert C.sizeof(_lib.TranscodeExt4) == 64
    assert C.sizeof(_lib.TranscodeExt5) == 88 and C.sizeof(_lib.TranscodeExtInfo4) == 64
    assert C.sizeof(_lib.TranscodeExt6) == 112 and C.sizeof(_lib.TranscodeExtInfo5) == 96
    assert _lib.ABI_VERSION == 9 and _lib.lib().vts_abi_version() == 9
    # no new entry point: the structs go through vts_transcode_ex by pointer cast
    assert [n for n in _lib.SIGNATURES if "transcode" in n] == ["vts_transcode", "vts_transcode_ex"]
    assert not any(w in name for name in _lib.SIGNATURES for w in ("ratectl", "bitrate", "ext7"))
    so = Path(_lib.__file__).resolve().parent / "libvtseg.so"
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], check=True, capture_output=True, text=True).stdout
    names = sorted(line.split()[-1] for line in out.splitlines() if "transcode" in line.split()[-1]
                   and line.split()[-1].startswith("vts_"))
    assert names == ["vts_transcode", "vts_transcode_ex"]


def test_structs_match_the_header(tmp_path):
    """Sizes and offsets equal a gcc probe compiled against include/vtseg.h."""
    structs = {"vts_transcode_ext7": _lib.TranscodeExt7, "vts_transcode_ext_info6": _lib.TranscodeExtInfo6,
               "vts_transcode_ext6": _lib.TranscodeExt6, "vts_transcode_ext_info5": _lib.TranscodeExtInfo5}
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
    assert int(got["vts_transcode_ext7"]) == 168 and int(got["vts_transcode_ext_info6"]) == 128
    assert int(got["vts_transcode_ext6"]) == 112 and int(got["vts_transcode_ext_info5"]) == 96
    for fields, cname in ((EXT7[0], "vts_transcode_ext7"), (INFO6[0], "vts_transcode_ext_info6")):
        for n, off in fields:
            assert int(got[f"{cname}.{n}"]) == off, (cname, n)
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)


def test_other_tracks_are_sized_from_moov_alone(tmp_path):
    """The bytes vts_add_tracks will copy: stsz (fixed and per sample) and stz2 (4, 8, 16 bits) of every track
    that is not video, read from moov without touching the media data."""
    import struct

    from vtseg import upload

    def box(kind, payload):
        return struct.pack(">I4s", 8 + len(payload), kind) + payload

    def trak(handler, size_box):
        hdlr = box(b"hdlr", bytes(8) + handler + bytes(12) + b"x\x00")
        return box(b"trak", box(b"mdia", hdlr + box(b"minf", box(b"stbl", size_box))))
    sizes = [3, 15, 7, 1, 9]
    stsz = box(b"stsz", struct.pack(">III", 0, 0, 5) + struct.pack(">5I", *sizes))
    fixed = box(b"stsz", struct.pack(">III", 0, 100, 7))
    z4 = box(b"stz2", struct.pack(">I3xBI", 0, 4, 5) + bytes([0x3f, 0x71, 0x90]))
    z8 = box(b"stz2", struct.pack(">I3xBI", 0, 8, 5) + bytes(sizes))
    z16 = box(b"stz2", struct.pack(">I3xBI", 0, 16, 5) + struct.pack(">5H", *sizes))
    video = trak(b"vide", box(b"stsz", struct.pack(">III", 0, 5000, 9)))
    moov = box(b"moov", video + b"".join(trak(b"soun", b) for b in (stsz, fixed, z4, z8, z16)))
    # a 64-bit mdat header in front of moov: the walk goes by the headers
    mdat = struct.pack(">I4sQ", 1, b"mdat", 16 + 1000) + bytes(1000)
    path = tmp_path / "t.mp4"
    path.write_bytes(box(b"ftyp", b"isom" + bytes(4)) + mdat + moov)
    assert upload.other_tracks_bytes(path) == 4 * sum(sizes) + 700
    assert upload._moov(path) == moov[8:]
    path.write_bytes(box(b"ftyp", b"isom" + bytes(4)) + mdat)          # no moov: nothing to leave room for
    assert upload.other_tracks_bytes(path) == 0
    assert upload.target_bitrate_kbps(path, 1.0, 8.0) == 1024 * 1024 * 8 // 8 // 1000


def test_python_entry_points_accept_the_keywords():
    from vtseg import scene, upload
    tr = inspect.signature(scene.VideoScorer.transcode).parameters
    up = inspect.signature(upload.compress_video_for_upload).parameters
    for name, default in (("bitrate_kbps", 0), ("qp_range", (0, 0)), ("frame_qp", None), ("want_rate", False)):
        assert tr[name].kind is inspect.Parameter.KEYWORD_ONLY and tr[name].default == default, name
    assert up["target_size_mb"].default is None
    assert not any(n in up for n in ("bitrate_kbps", "frame_qp", "want_rate"))
    # the earlier keywords stay what they were
    for name in ("intra", "deblock", "mvcost", "early_skip", "cabac", "intra4x4", "partitions"):
        assert tr[name].default is False and up[name].default is False
    assert tr["subpel"].default == 0 and up["subpel"].default == 0
