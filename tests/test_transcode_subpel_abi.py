"""The opt-in sub-sample motion refinement of the upload transcode at the ABI
(no GPU): `vts_transcode_ex` with its two size-tagged structs, beside an
unchanged version 9, `vts_transcode_params` and `vts_transcode_info`, and the
Python keywords that reach it."""
from __future__ import annotations

import ctypes as C
import inspect
import shutil
import subprocess
from pathlib import Path

import pytest

from vtseg import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtseg.h"

# the layouts of the parent (ABI 9): (name, ctype, offset), and the size
PARAMS_V9 = ([("height", C.c_int32, 0), ("search_range", C.c_int32, 4), ("max_mb_sad", C.c_int32, 8),
              ("keyint", C.c_int32, 12), ("cut_threshold", C.c_float, 16), ("idr_at_cuts", C.c_int32, 20),
              ("qp", C.c_int32, 24), ("intra", C.c_int32, 28)], 32)
INFO_V9 = ([("width", C.c_int32, 0), ("height", C.c_int32, 4), ("n_frames", C.c_int64, 8),
            ("n_idr", C.c_int64, 16), ("pcm_mbs", C.c_int64, 24), ("inter_mbs", C.c_int64, 32),
            ("skip_mbs", C.c_int64, 40), ("bytes_written", C.c_int64, 48), ("ms", C.c_double * 4, 56),
            ("intra_mbs", C.c_int64, 88), ("recon_hash", C.c_uint64, 96)], 104)


def test_library_exports_vts_transcode_ex_at_abi_9():
    lib = _lib.lib()
    assert _lib.ABI_VERSION == 9 and lib.vts_abi_version() == 9
    assert "vts_transcode_ex" in _lib.SIGNATURES
    fn = lib.vts_transcode_ex  # AttributeError when the symbol is missing
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_char_p, C.POINTER(_lib.TranscodeParams),
                                 C.POINTER(_lib.TranscodeExt), C.POINTER(_lib.TranscodeInfo),
                                 C.POINTER(_lib.TranscodeExtInfo)]
    assert lib.vts_transcode is not None  # the old entry point stays


def test_existing_transcode_structs_are_unchanged():
    for py, (fields, size) in ((_lib.TranscodeParams, PARAMS_V9), (_lib.TranscodeInfo, INFO_V9)):
        assert [(n, t) for n, t in py._fields_] == [(n, t) for n, t, _ in fields], py
        for n, _, off in fields:
            assert getattr(py, n).offset == off, (py, n)
        assert C.sizeof(py) == size, py


def test_ext_structs_match_the_header(tmp_path):
    """Sizes and offsets of the two new structs (and of the two old ones)
    equal a probe compiled against include/vtseg.h."""
    assert _lib.TranscodeExt._fields_ == [("struct_size", C.c_uint32), ("subpel", C.c_int32)]
    assert _lib.TranscodeExtInfo._fields_ == [("struct_size", C.c_uint32), ("_pad", C.c_int32),
                                              ("subpel_mbs", C.c_int64), ("qpel_mbs", C.c_int64)]
    assert C.sizeof(_lib.TranscodeExt) == 8 and C.sizeof(_lib.TranscodeExtInfo) == 24
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    structs = {"vts_transcode_ext": _lib.TranscodeExt, "vts_transcode_ext_info": _lib.TranscodeExtInfo,
               "vts_transcode_params": _lib.TranscodeParams, "vts_transcode_info": _lib.TranscodeInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"',
             # the declaration is there and has this type (compile time: nothing is linked)
             "typedef int (*ex_fn)(vts_ctx *, const char *, const vts_transcode_params *,",
             "                     const vts_transcode_ext *, vts_transcode_info *, vts_transcode_ext_info *);",
             "_Static_assert(__builtin_types_compatible_p(__typeof__(&vts_transcode_ex), ex_fn),",
             '               "vts_transcode_ex signature");',
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


def test_python_entry_points_accept_subpel():
    from vtseg import scene, upload
    for fn in (scene.VideoScorer.transcode, upload.compress_video_for_upload):
        prm = inspect.signature(fn).parameters["subpel"]
        assert prm.kind is inspect.Parameter.KEYWORD_ONLY
        assert prm.default == 0 and prm.annotation in (int, "int")
