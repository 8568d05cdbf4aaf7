"""The opt-in Intra16x16 coder of the upload transcode at the ABI (no GPU):
version 9, `vts_transcode_params.intra`, `vts_transcode_info.intra_mbs` /
`recon_hash`, and the Python keywords that reach them."""
from __future__ import annotations

import ctypes as C
import inspect
import shutil
import subprocess
from pathlib import Path

import pytest

from vtseg import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtseg.h"


def test_abi_version_is_9():
    assert _lib.ABI_VERSION == 9
    assert _lib.lib().vts_abi_version() == 9


def test_transcode_structs_carry_the_intra_fields(tmp_path):
    """The ctypes mirrors have the new fields, and their sizes and offsets
    equal a probe compiled against include/vtseg.h."""
    p = dict(_lib.TranscodeParams._fields_)
    i = dict(_lib.TranscodeInfo._fields_)
    assert p["intra"] is C.c_int32
    assert i["intra_mbs"] is C.c_int64 and i["recon_hash"] is C.c_uint64
    # appended: every earlier field keeps its place
    assert [n for n, _ in _lib.TranscodeParams._fields_][-1] == "intra"
    assert [n for n, _ in _lib.TranscodeInfo._fields_][-2:] == ["intra_mbs", "recon_hash"]
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    structs = {"vts_transcode_params": _lib.TranscodeParams,
               "vts_transcode_info": _lib.TranscodeInfo}
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
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)


def test_python_entry_points_accept_intra():
    from vtseg import scene, upload
    for fn in (scene.VideoScorer.transcode, upload.compress_video_for_upload):
        prm = inspect.signature(fn).parameters["intra"]
        assert prm.kind is inspect.Parameter.KEYWORD_ONLY
        assert prm.default is False
