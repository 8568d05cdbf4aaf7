"""CABAC entropy coding of the upload transcode at the ABI (no GPU): one struct
that begins with `vts_transcode_ext3` and travels through the existing
`vts_transcode_ex`, beside an unchanged version 9 and the unchanged older
structs, and the Python keyword that reaches it."""
from __future__ import annotations

import ctypes as C
import inspect
import subprocess
from pathlib import Path

from vtseg import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtseg.h"

EXT4 = ([("base", 0), ("cabac", 56), ("_pad2", 60)], 64)


def test_new_struct_has_the_stated_layout():
    py, (fields, size) = _lib.TranscodeExt4, EXT4
    assert [n for n, _ in py._fields_] == [n for n, _ in fields]
    for n, off in fields:
        assert getattr(py, n).offset == off, n
    assert C.sizeof(py) == size
    f4 = dict(py._fields_)
    assert f4["base"] is _lib.TranscodeExt3 and f4["cabac"] is C.c_int32 and f4["_pad2"] is C.c_int32


def test_old_structs_and_the_version_are_unchanged():
    assert C.sizeof(_lib.TranscodeExt) == 8 and C.sizeof(_lib.TranscodeExtInfo) == 24
    assert C.sizeof(_lib.TranscodeExt2) == 24 and C.sizeof(_lib.TranscodeExtInfo2) == 32
    assert C.sizeof(_lib.TranscodeExt3) == 56 and C.sizeof(_lib.TranscodeExtInfo3) == 48
    assert _lib.ABI_VERSION == 9 and _lib.lib().vts_abi_version() == 9
    # no new entry point: the struct goes through vts_transcode_ex by pointer cast
    assert not any(w in name for name in _lib.SIGNATURES for w in ("cabac", "ext4", "entropy"))
    assert [n for n in _lib.SIGNATURES if "transcode" in n] == ["vts_transcode", "vts_transcode_ex"]
    res, args = _lib.SIGNATURES["vts_transcode_ex"]
    assert res is C.c_int and args[3] is C.POINTER(_lib.TranscodeExt) and args[5] is C.POINTER(_lib.TranscodeExtInfo)


def test_structs_match_the_header(tmp_path):
    """Sizes and offsets equal a gcc probe compiled against include/vtseg.h."""
    structs = {"vts_transcode_ext4": _lib.TranscodeExt4, "vts_transcode_ext3": _lib.TranscodeExt3,
               "vts_transcode_ext_info3": _lib.TranscodeExtInfo3, "vts_transcode_ext2": _lib.TranscodeExt2,
               "vts_transcode_ext_info2": _lib.TranscodeExtInfo2, "vts_transcode_ext": _lib.TranscodeExt,
               "vts_transcode_ext_info": _lib.TranscodeExtInfo}
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
    assert int(got["vts_transcode_ext4"]) == 64
    for (n, off) in EXT4[0]:
        assert int(got[f"vts_transcode_ext4.{n}"]) == off, n
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)


def test_python_entry_points_accept_the_keyword():
    from vtseg import scene, upload
    tr = inspect.signature(scene.VideoScorer.transcode).parameters
    up = inspect.signature(upload.compress_video_for_upload).parameters
    for prm in (tr, up):
        assert prm["cabac"].kind is inspect.Parameter.KEYWORD_ONLY
        assert prm["cabac"].default is False and prm["cabac"].annotation in (bool, "bool")
    # the earlier keywords stay what they were
    for name in ("intra", "deblock", "mvcost", "early_skip"):
        assert tr[name].default is False and up[name].default is False
    assert tr["subpel"].default == 0 and up["subpel"].default == 0
    from vtseg import dropin
    assert "cabac" not in inspect.getsource(dropin)
