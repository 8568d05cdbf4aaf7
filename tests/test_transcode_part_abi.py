"""Inter partitions of the upload transcode at the ABI (no GPU): two structs
that begin with `vts_transcode_ext5` / `vts_transcode_ext_info4` and travel
through the existing `vts_transcode_ex`, beside an unchanged version 9 and the
unchanged older structs, and the Python keywords that reach them (DESIGN.md
§11 "Partitions")."""
from __future__ import annotations

import ctypes as C
import inspect
import subprocess
from pathlib import Path

from vtseg import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtseg.h"

EXT6 = ([("base", 0), ("partitions", 88), ("_pad4", 92), ("mv_out", 96), ("mv_cap", 104)], 112)
INFO5 = ([("base", 0), ("p16x8_mbs", 64), ("p8x16_mbs", 72), ("p8x8_mbs", 80), ("mv_words", 88)], 96)


def test_new_structs_have_the_stated_layout():
    for py, (fields, size) in ((_lib.TranscodeExt6, EXT6), (_lib.TranscodeExtInfo5, INFO5)):
        assert [n for n, _ in py._fields_] == [n for n, _ in fields]
        for n, off in fields:
            assert getattr(py, n).offset == off, n
        assert C.sizeof(py) == size
    f6, i5 = dict(_lib.TranscodeExt6._fields_), dict(_lib.TranscodeExtInfo5._fields_)
    assert f6["base"] is _lib.TranscodeExt5 and f6["partitions"] is C.c_int32 and f6["_pad4"] is C.c_int32
    assert f6["mv_out"] is C.POINTER(C.c_uint32) and f6["mv_cap"] is C.c_int64
    assert i5["base"] is _lib.TranscodeExtInfo4
    assert all(i5[n] is C.c_int64 for n in ("p16x8_mbs", "p8x16_mbs", "p8x8_mbs", "mv_words"))


def test_old_structs_and_the_version_are_unchanged():
    assert C.sizeof(_lib.TranscodeExt) == 8 and C.sizeof(_lib.TranscodeExtInfo) == 24
    assert C.sizeof(_lib.TranscodeExt2) == 24 and C.sizeof(_lib.TranscodeExtInfo2) == 32
    assert C.sizeof(_lib.TranscodeExt3) == 56 and C.sizeof(_lib.TranscodeExtInfo3) == 48
    assert C.sizeof(_lib.TranscodeExt4) == 64
    assert C.sizeof(_lib.TranscodeExt5) == 88 and C.sizeof(_lib.TranscodeExtInfo4) == 64
    assert _lib.ABI_VERSION == 9 and _lib.lib().vts_abi_version() == 9
    # no new entry point: the structs go through vts_transcode_ex by pointer cast
    assert not any(w in name for name in _lib.SIGNATURES for w in ("part", "mv4", "ext6"))
    assert [n for n in _lib.SIGNATURES if "transcode" in n] == ["vts_transcode", "vts_transcode_ex"]
    res, args = _lib.SIGNATURES["vts_transcode_ex"]
    assert res is C.c_int and args[3] is C.POINTER(_lib.TranscodeExt) and args[5] is C.POINTER(_lib.TranscodeExtInfo)


def test_the_library_exports_nothing_new():
    """The dynamic symbols named vts_*transcode* are the two entry points there were."""
    so = Path(_lib.__file__).resolve().parent / "libvtseg.so"
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], check=True, capture_output=True, text=True).stdout
    names = sorted(line.split()[-1] for line in out.splitlines() if "transcode" in line.split()[-1]
                   and line.split()[-1].startswith("vts_"))
    assert names == ["vts_transcode", "vts_transcode_ex"]


def test_structs_match_the_header(tmp_path):
    """Sizes and offsets equal a gcc probe compiled against include/vtseg.h."""
    structs = {"vts_transcode_ext6": _lib.TranscodeExt6, "vts_transcode_ext_info5": _lib.TranscodeExtInfo5,
               "vts_transcode_ext5": _lib.TranscodeExt5, "vts_transcode_ext_info4": _lib.TranscodeExtInfo4,
               "vts_transcode_ext4": _lib.TranscodeExt4, "vts_transcode_ext3": _lib.TranscodeExt3,
               "vts_transcode_ext_info3": _lib.TranscodeExtInfo3}
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
    assert int(got["vts_transcode_ext6"]) == 112 and int(got["vts_transcode_ext_info5"]) == 96
    assert int(got["vts_transcode_ext5"]) == 88 and int(got["vts_transcode_ext_info4"]) == 64
    for fields, cname in ((EXT6[0], "vts_transcode_ext6"), (INFO5[0], "vts_transcode_ext_info5")):
        for n, off in fields:
            assert int(got[f"{cname}.{n}"]) == off, (cname, n)
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)


def test_python_entry_points_accept_the_keywords():
    from vtseg import scene, upload
    tr = inspect.signature(scene.VideoScorer.transcode).parameters
    up = inspect.signature(upload.compress_video_for_upload).parameters
    for prm in (tr, up):
        assert prm["partitions"].kind is inspect.Parameter.KEYWORD_ONLY
        assert prm["partitions"].default is False and prm["partitions"].annotation in (bool, "bool")
    assert tr["want_vectors"].kind is inspect.Parameter.KEYWORD_ONLY and tr["want_vectors"].default is False
    assert "want_vectors" not in up
    # the earlier keywords stay what they were
    for name in ("intra", "deblock", "mvcost", "early_skip", "cabac", "intra4x4"):
        assert tr[name].default is False and up[name].default is False
    assert tr["subpel"].default == 0 and up["subpel"].default == 0
    from vtseg import dropin
    assert "partitions" not in inspect.getsource(dropin)
