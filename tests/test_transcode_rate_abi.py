"""The rate-aware motion decisions of the upload transcode at the ABI (no GPU):
two structs that begin with `vts_transcode_ext2` / `_ext_info2` and travel
through the existing `vts_transcode_ex`, beside an unchanged version 9 and the
unchanged older structs, and the Python keywords that reach them (DESIGN.md
§11)."""
from __future__ import annotations

import ctypes as C
import inspect
import subprocess
from pathlib import Path

from vtseg import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtseg.h"

EXT3 = ([("base", 0), ("mvcost", 24), ("mv_lambda16", 28), ("early_skip", 32), ("_pad", 36),
         ("cmd_out", 40), ("cmd_cap", 48)], 56)
INFO3 = ([("base", 0), ("early_skip_mbs", 32), ("cmd_words", 40)], 48)


def test_new_structs_have_the_stated_layout():
    for py, (fields, size) in ((_lib.TranscodeExt3, EXT3), (_lib.TranscodeExtInfo3, INFO3)):
        assert [n for n, _ in py._fields_] == [n for n, _ in fields], py
        for n, off in fields:
            assert getattr(py, n).offset == off, (py, n)
        assert C.sizeof(py) == size, py
    f3, i3 = dict(_lib.TranscodeExt3._fields_), dict(_lib.TranscodeExtInfo3._fields_)
    assert f3["base"] is _lib.TranscodeExt2 and i3["base"] is _lib.TranscodeExtInfo2
    for n in ("mvcost", "mv_lambda16", "early_skip", "_pad"):
        assert f3[n] is C.c_int32
    assert f3["cmd_out"] is C.POINTER(C.c_uint32) and f3["cmd_cap"] is C.c_int64
    assert i3["early_skip_mbs"] is C.c_int64 and i3["cmd_words"] is C.c_int64


def test_old_structs_and_the_version_are_unchanged():
    assert C.sizeof(_lib.TranscodeExt) == 8 and C.sizeof(_lib.TranscodeExtInfo) == 24
    assert C.sizeof(_lib.TranscodeExt2) == 24 and C.sizeof(_lib.TranscodeExtInfo2) == 32
    assert _lib.ABI_VERSION == 9 and _lib.lib().vts_abi_version() == 9
    # no new entry point: the structs go through vts_transcode_ex by pointer cast
    assert not any(w in name for name in _lib.SIGNATURES for w in ("mvcost", "skip", "rate", "cmd", "ext3"))
    assert [n for n in _lib.SIGNATURES if "transcode" in n] == ["vts_transcode", "vts_transcode_ex"]


def test_structs_match_the_header(tmp_path):
    """Sizes and offsets equal a gcc probe compiled against include/vtseg.h."""
    structs = {"vts_transcode_ext3": _lib.TranscodeExt3, "vts_transcode_ext_info3": _lib.TranscodeExtInfo3,
               "vts_transcode_ext2": _lib.TranscodeExt2, "vts_transcode_ext_info2": _lib.TranscodeExtInfo2,
               "vts_transcode_ext": _lib.TranscodeExt, "vts_transcode_ext_info": _lib.TranscodeExtInfo}
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
    assert int(got["vts_transcode_ext"]) == 8 and int(got["vts_transcode_ext_info"]) == 24
    assert int(got["vts_transcode_ext2"]) == 24 and int(got["vts_transcode_ext_info2"]) == 32
    assert int(got["vts_transcode_ext3"]) == 56 and int(got["vts_transcode_ext_info3"]) == 48
    for (n, off) in EXT3[0]:
        assert int(got[f"vts_transcode_ext3.{n}"]) == off, n
    for (n, off) in INFO3[0]:
        assert int(got[f"vts_transcode_ext_info3.{n}"]) == off, n
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)


def test_python_entry_points_accept_the_keywords():
    from vtseg import scene, upload
    tr = inspect.signature(scene.VideoScorer.transcode).parameters
    up = inspect.signature(upload.compress_video_for_upload).parameters
    for prm in (tr, up):
        for name in ("mvcost", "early_skip"):
            assert prm[name].kind is inspect.Parameter.KEYWORD_ONLY
            assert prm[name].default is False and prm[name].annotation in (bool, "bool")
    assert tr["mv_lambda16"].kind is inspect.Parameter.KEYWORD_ONLY
    assert tr["mv_lambda16"].default == 0 and tr["mv_lambda16"].annotation in (int, "int")
    assert tr["want_commands"].kind is inspect.Parameter.KEYWORD_ONLY
    assert tr["want_commands"].default is False and tr["want_commands"].annotation in (bool, "bool")
    assert "mv_lambda16" not in up and "want_commands" not in up   # the upload path forwards the two decisions only
