"""The opt-in in-loop deblocking filter of the upload transcode at the ABI (no
GPU): two structs that begin with `vts_transcode_ext` / `_ext_info` and travel
through the existing `vts_transcode_ex`, beside an unchanged version 9 and the
unchanged 8- and 24-byte structs, and the Python keywords that reach them
(DESIGN.md §11)."""
from __future__ import annotations

import ctypes as C
import inspect
import subprocess
from pathlib import Path

from vtseg import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtseg.h"

EXT2 = ([("base", 0), ("deblock", 8), ("deblock_alpha", 12), ("deblock_beta", 16), ("_pad", 20)], 24)
INFO2 = ([("base", 0), ("deblock_mbs", 24)], 32)


def test_new_structs_have_the_stated_layout():
    for py, (fields, size) in ((_lib.TranscodeExt2, EXT2), (_lib.TranscodeExtInfo2, INFO2)):
        assert [n for n, _ in py._fields_] == [n for n, _ in fields], py
        for n, off in fields:
            assert getattr(py, n).offset == off, (py, n)
        assert C.sizeof(py) == size, py
    assert dict(_lib.TranscodeExt2._fields_)["base"] is _lib.TranscodeExt
    assert dict(_lib.TranscodeExtInfo2._fields_)["base"] is _lib.TranscodeExtInfo
    for n in ("deblock", "deblock_alpha", "deblock_beta", "_pad"):
        assert dict(_lib.TranscodeExt2._fields_)[n] is C.c_int32
    assert dict(_lib.TranscodeExtInfo2._fields_)["deblock_mbs"] is C.c_int64


def test_old_structs_and_the_version_are_unchanged():
    assert C.sizeof(_lib.TranscodeExt) == 8 and C.sizeof(_lib.TranscodeExtInfo) == 24
    assert _lib.ABI_VERSION == 9 and _lib.lib().vts_abi_version() == 9
    # no new entry point: the structs go through vts_transcode_ex by pointer cast
    assert not any("deblock" in name for name in _lib.SIGNATURES)


def test_structs_match_the_header(tmp_path):
    """Sizes and offsets equal a gcc probe compiled against include/vtseg.h."""
    structs = {"vts_transcode_ext2": _lib.TranscodeExt2, "vts_transcode_ext_info2": _lib.TranscodeExtInfo2,
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
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)


def test_python_entry_points_accept_deblock():
    from vtseg import scene, upload
    for fn in (scene.VideoScorer.transcode, upload.compress_video_for_upload):
        prm = inspect.signature(fn).parameters
        assert prm["deblock"].kind is inspect.Parameter.KEYWORD_ONLY
        assert prm["deblock"].default is False and prm["deblock"].annotation in (bool, "bool")
        assert prm["deblock_offsets"].kind is inspect.Parameter.KEYWORD_ONLY
        assert prm["deblock_offsets"].default == (0, 0)
