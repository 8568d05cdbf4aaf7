"""Adaptive quantisation at the ABI: two structs that begin with
`vts_transcode_ext8` / `vts_transcode_ext_info7` and travel through the
existing `vts_transcode_ex`, beside an unchanged version 9 and the unchanged
older structs; the Python keywords that reach them; and (on the device) the
argument errors, each naming its field, and an all-zero 208-byte struct as the
184-byte call (DESIGN.md §11 "Adaptive quantisation")."""
from __future__ import annotations

import ctypes as C
import inspect
import subprocess
from pathlib import Path

import numpy as np
import pytest

from vtseg import VtsegError, _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtseg.h"

EXT9 = ([("base", 0), ("aq_strength_q8", 184), ("aq_max", 188), ("mbqp_out", 192), ("mbqp_cap", 200)], 208)
INFO8 = ([("base", 0), ("mbqp_words", 144), ("aq_lo", 152), ("aq_hi", 156), ("aq_mbs", 160)], 168)


def test_new_structs_have_the_stated_layout():
    for py, (fields, size) in ((_lib.TranscodeExt9, EXT9), (_lib.TranscodeExtInfo8, INFO8)):
        assert [n for n, _ in py._fields_] == [n for n, _ in fields]
        for n, off in fields:
            assert getattr(py, n).offset == off, n
        assert C.sizeof(py) == size
    f9, i8 = dict(_lib.TranscodeExt9._fields_), dict(_lib.TranscodeExtInfo8._fields_)
    assert f9["base"] is _lib.TranscodeExt8 and i8["base"] is _lib.TranscodeExtInfo7
    assert f9["aq_strength_q8"] is C.c_int32 and f9["aq_max"] is C.c_int32 and f9["mbqp_cap"] is C.c_int64
    assert i8["mbqp_words"] is C.c_int64 and i8["aq_lo"] is C.c_int32 and i8["aq_hi"] is C.c_int32 and i8["aq_mbs"] is C.c_int64


def test_old_structs_and_the_version_are_unchanged():
    assert C.sizeof(_lib.TranscodeExt7) == 168 and C.sizeof(_lib.TranscodeExtInfo6) == 128
    assert C.sizeof(_lib.TranscodeExt8) == 184 and C.sizeof(_lib.TranscodeExtInfo7) == 144
    assert _lib.ABI_VERSION == 9 and _lib.lib().vts_abi_version() == 9
    # no new entry point: the structs go through vts_transcode_ex by pointer cast
    assert [n for n in _lib.SIGNATURES if "transcode" in n] == ["vts_transcode", "vts_transcode_ex"]
    so = Path(_lib.__file__).resolve().parent / "libvtseg.so"
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], check=True, capture_output=True, text=True).stdout
    exported = [line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("vts_")]
    assert sorted(n for n in exported if "transcode" in n) == ["vts_transcode", "vts_transcode_ex"]


def test_structs_match_the_header(tmp_path):
    """Sizes and offsets equal a gcc probe compiled against include/vtseg.h."""
    structs = {"vts_transcode_ext9": _lib.TranscodeExt9, "vts_transcode_ext_info8": _lib.TranscodeExtInfo8,
               "vts_transcode_ext8": _lib.TranscodeExt8, "vts_transcode_ext_info7": _lib.TranscodeExtInfo7}
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
    assert int(got["vts_transcode_ext9"]) == 208 and int(got["vts_transcode_ext_info8"]) == 168
    assert int(got["vts_transcode_ext8"]) == 184 and int(got["vts_transcode_ext_info7"]) == 144
    for fields, cname in ((EXT9[0], "vts_transcode_ext9"), (INFO8[0], "vts_transcode_ext_info8")):
        for n, off in fields:
            assert int(got[f"{cname}.{n}"]) == off, (cname, n)
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)


def test_python_entry_points_accept_the_keywords():
    from vtseg import scene, upload
    from vtseg import video_segmenter as vs
    tr = inspect.signature(scene.VideoScorer.transcode).parameters
    up = inspect.signature(upload.compress_video_for_upload).parameters
    assert tr["aq_strength"].kind is inspect.Parameter.KEYWORD_ONLY and tr["aq_strength"].default == 0.0
    assert tr["aq_max"].kind is inspect.Parameter.KEYWORD_ONLY and tr["aq_max"].default == 0
    assert up["aq_strength"].kind is inspect.Parameter.KEYWORD_ONLY and up["aq_strength"].default == 0.0
    # the earlier keywords and the segment encoder stay what they were
    for name in ("intra", "deblock", "mvcost", "early_skip", "cabac", "intra4x4", "partitions", "want_rate"):
        assert tr[name].default is False
    assert tr["frames"].default is None and tr["qp"].default == 28
    assert vs.SEGMENT_ENCODER == dict(qp=23, intra=True, intra4x4=True, subpel=2, deblock=True, mvcost=True,
                                      early_skip=True, cabac=True)
    assert {"aq_strength", "aq_max"} <= set(tr)            # what transcode_segment / extract_segment(encoder=...) pass on
    assert inspect.signature(scene.VideoScorer.transcode_segment).parameters["encoder"].kind is inspect.Parameter.VAR_KEYWORD


# ------------------------------------------------------------ on the device
def _source(tmp_path):
    from vtseg import scene
    path = tmp_path / "src.mp4"
    scene.synth_write(path, width=96, height=64, n_frames=8, cut_min_s=0.7, cut_max_s=1.5, gop_max_s=0.5)
    return path


def _raw_ext9(v, out, size, *, mvcost=1, qp=0, max_mb_sad=0, mbqp=None, cap=0, **fields):
    prm = _lib.TranscodeParams()
    prm.height = 64
    prm.qp = qp
    prm.max_mb_sad = max_mb_sad
    ext = _lib.TranscodeExt9(_lib.TranscodeExt8(_lib.TranscodeExt7(_lib.TranscodeExt6(_lib.TranscodeExt5(_lib.TranscodeExt4(
        _lib.TranscodeExt3(_lib.TranscodeExt2(_lib.TranscodeExt(size, 0)), mvcost)))))))
    for k, val in fields.items():
        setattr(ext, k, val)
    if mbqp is not None:
        ext.mbqp_out = mbqp.ctypes.data_as(C.POINTER(C.c_uint8))
    ext.mbqp_cap = cap
    info = _lib.TranscodeInfo()
    xinfo = _lib.TranscodeExtInfo8(_lib.TranscodeExtInfo7(_lib.TranscodeExtInfo6(_lib.TranscodeExtInfo5(
        _lib.TranscodeExtInfo4(_lib.TranscodeExtInfo3(_lib.TranscodeExtInfo2(_lib.TranscodeExtInfo(
            C.sizeof(_lib.TranscodeExtInfo8)))))))))
    rc = v._lib.vts_transcode_ex(v._ctx, str(out).encode(), C.byref(prm),
                                 C.cast(C.pointer(ext), C.POINTER(_lib.TranscodeExt)), C.byref(info),
                                 C.cast(C.pointer(xinfo), C.POINTER(_lib.TranscodeExtInfo)))
    return rc, info, xinfo


@pytest.mark.gpu
def test_an_all_zero_208_byte_struct_is_the_184_byte_call(tmp_path):
    from test_transcode_subpel_gpu import _require_gpu
    from vtseg import scene
    _require_gpu()
    src = _source(tmp_path)
    files = {}
    nmb = 6 * 4
    for size in (184, 208):
        out = tmp_path / f"s{size}.mp4"
        with scene.VideoScorer(src) as v:
            rc, _, xi = _raw_ext9(v, out, size)
            _lib.check(rc)
        files[size] = out.read_bytes()
        assert xi.mbqp_words == 8 * nmb and xi.aq_lo == xi.aq_hi == xi.aq_mbs == 0
    assert files[184] == files[208]
    with scene.VideoScorer(src) as v:                                # the keywords' default file
        v.transcode(tmp_path / "base.mp4", height=64, mvcost=True)
    assert files[208] == (tmp_path / "base.mp4").read_bytes()
    # 184 bytes with a strength behind them: not read
    with scene.VideoScorer(src) as v:
        rc, _, _ = _raw_ext9(v, tmp_path / "behind.mp4", 184, aq_strength_q8=256, aq_max=77)
        _lib.check(rc)
    assert (tmp_path / "behind.mp4").read_bytes() == files[184]
    # mbqp_out is filled with any settings: aq off, the call's QP
    with scene.VideoScorer(src) as v:
        buf = np.zeros(8 * nmb, np.uint8)
        rc, _, xi = _raw_ext9(v, tmp_path / "ok.mp4", 208, qp=35, mbqp=buf, cap=buf.size)
        _lib.check(rc)
        assert (buf == 35).all()


@pytest.mark.gpu
def test_argument_errors(tmp_path):
    from test_transcode_subpel_gpu import _require_gpu
    from vtseg import scene
    _require_gpu()
    src = _source(tmp_path)
    bad = tmp_path / "bad.mp4"
    cases = [
        (dict(aq_strength=-1 / 256), "aq_strength_q8"), (dict(aq_strength=769 / 256), "aq_strength_q8"),
        (dict(aq_strength=1.0, aq_max=-1), "aq_max"), (dict(aq_strength=1.0, aq_max=11), "aq_max"),
        (dict(aq_max=4), "aq_max"),                                            # without a strength
        (dict(aq_strength=1.0, mvcost=False), "mvcost"),
        (dict(aq_strength=1.0, qp=-1), "aq_strength_q8"),
        (dict(aq_strength=1.0, max_mb_sad=-1), "max_mb_sad"),
    ]
    for fields, named in cases:
        kw = dict(dict(height=64, mvcost=True), **fields)
        with scene.VideoScorer(src) as v:
            with pytest.raises(VtsegError) as ei:
                v.transcode(bad, **kw)
        assert ei.value.code == _lib.VTS_E_INVALID, fields
        assert named in str(ei.value), (fields, str(ei.value))
        assert not bad.exists()
    # the extremes are accepted
    with scene.VideoScorer(src) as v:
        facts = v.transcode(tmp_path / "top.mp4", height=64, mvcost=True, aq_strength=3.0, aq_max=10)
        assert facts["aq_lo"] >= -10 and facts["aq_hi"] <= 10
    # mbqp_out too short: before any encoding
    with scene.VideoScorer(src) as v:
        buf = np.zeros(8 * 24, np.uint8)
        rc, _, xi = _raw_ext9(v, bad, 208, aq_strength_q8=256, mbqp=buf, cap=buf.size - 1)
        assert rc == _lib.VTS_E_CAPACITY and "mbqp_cap" in _lib.last_error()
        assert xi.mbqp_words == buf.size and not bad.exists() and (buf == 0).all()
