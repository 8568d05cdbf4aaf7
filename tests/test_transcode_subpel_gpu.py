"""The opt-in half- and quarter-sample motion refinement of the device upload
transcode (vts_transcode_ext.subpel).

The bytes are pinned in tests/test_transcode_bytes_gpu.py.  As for Intra16x16,
the pin here is a closed loop through two independent decoders: the output of
`transcode(subpel=1 | 2)` is decoded by the CPU general oracle
(oracle/h264_full_oracle.c) and by the device's general decoder, which both
implement the luma interpolation of 8.4.2.2.1; the two must agree, and the
hash of the oracle's decode must equal the hash the encoder computed of its
own reconstruction (`recon_hash`), so an interpolated prediction in the
encoder that differs from a conforming decoder's in one sample fails.
Every transcode runs in a fresh VideoScorer.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import oracle
from vtseg import VtsegError, _lib, scene

pytestmark = pytest.mark.gpu

REAL = Path(__file__).resolve().parent / "golden" / "real" / "realshort.mp4"
SYNTH = dict(cut_min_s=0.7, cut_max_s=1.5, gop_max_s=0.5)
SOURCES = {
    "odd": dict(width=320, height=240, n_frames=60, max_motion=5, odd_motion=True),
    "s70": dict(width=320, height=192, n_frames=70),
    "s40": dict(width=320, height=192, n_frames=40),
    "s60": dict(width=320, height=192, n_frames=60),
    "pan": dict(width=320, height=192, n_frames=60, max_motion=24),
    "crop": dict(width=640, height=480, n_frames=30),
    "content": dict(width=640, height=360, n_frames=30, coding="full", bframes=True, content=True,
                    slices_per_row=0, seed=7),
    "real": None,
}
# name -> (source, transcode kwargs, runs with intra=True too)
CASES = {
    "halfpel": ("odd", dict(height=120, search_range=4), True),      # 2:1: odd pans -> half samples; <4, SP>
    "small": ("s70", dict(height=96), True),                         # <8, SP>
    "keyint8_r16": ("s70", dict(height=96, keyint=8, search_range=16), True),  # largest window + margin
    "r5": ("s40", dict(height=96, search_range=5), True),            # the any-range instance <0, SP>
    "r0": ("s40", dict(height=96, search_range=-1), True),           # range 0: the smallest window
    "bigpan_edges": ("pan", dict(height=96), True),                  # vectors across all four clamped edges
    "crop": ("crop", dict(), True),                                  # 480x360 in 480x368, tap-table downscale
    "no_residual": ("s60", dict(height=96, qp=0), False),            # the qp < 1 branch
    "content": ("content", dict(), True),
    "real": ("real", dict(height=240), True),
}
LOOP = [(c, sp, i) for c, (_, _, both) in CASES.items() for sp in (1, 2) for i in ((False, True) if both else (False,))]
USED = ["halfpel", "content", "real"]
QUALITY = ["small", "content", "real"]


def _require_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires an MI355X")


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("subpel"), "src": {}, "run": {}, "ref": {}}


def _source(work, name):
    if name not in work["src"]:
        if name == "real":
            work["src"][name] = REAL
        else:
            path = work["dir"] / f"{name}.mp4"
            scene.synth_write(path, **dict(SYNTH, **SOURCES[name]))
            work["src"][name] = path
    return work["src"][name]


def _is_idr(m):
    """Per sample: its first NAL is an IDR slice (4-byte length prefixes)."""
    return [(m["data"][o + 4] & 31) == 5 for o in m["offsets"]]


def _run(work, case, subpel, intra):
    """Transcode once per (case, subpel, intra) in a fresh session; the output
    is decoded by the oracle."""
    key = (case, subpel, intra)
    if key not in work["run"]:
        sname, tk, _ = CASES[case]
        out = work["dir"] / f"{case}_{subpel}_{int(intra)}.mp4"
        with scene.VideoScorer(_source(work, sname)) as v:
            facts = v.transcode(out, intra=intra, subpel=subpel, **tk)
        frames, _ = oracle.decode_full(out)
        m = oracle.read_mp4(out)
        work["run"][key] = dict(out=out, facts=facts, frames=frames, idr=_is_idr(m), size=out.stat().st_size)
    return work["run"][key]


def _reference(work, case):
    """The encoder's input: the oracle's downscale of the oracle's decode of
    the source, cropped to the display size (NV12 [F, h*3/2, w])."""
    sname, tk, _ = CASES[case]
    key = (sname, tk.get("height", 360))
    if key not in work["ref"]:
        frames, info = oracle.decode_full(_source(work, sname))
        W, H, sh = info["width"], info["height"], key[1]
        sw = oracle.small_width(W, H, sh)
        ch = (sh + 15) & ~15
        ref = []
        for f in frames:
            d = oracle.downscale_nv12(f, W, H, sh)
            ref.append(np.concatenate([d[:sh, :sw], d[ch:ch + sh // 2, :sw]]))
        work["ref"][key] = np.stack(ref)
    return work["ref"][key]


def _psnr(a, b):
    """PSNR over every NV12 byte (Y, Cb and Cr together) of the pictures."""
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.parametrize("case,subpel,intra", LOOP)
def test_subpel_output_decodes_to_the_encoders_reconstruction(work, case, subpel, intra):
    _require_gpu()
    on, off = _run(work, case, subpel, intra), _run(work, case, 0, intra)
    facts, frames = on["facts"], on["frames"]
    n = facts["n_frames"]
    assert frames.shape[0] == n
    # the device's general decoder reads the same pictures as the oracle
    with scene.VideoScorer(on["out"], keep_frames=True) as d:
        d.score()
        assert d.general()
        got = np.stack([d.frame_nv12(i).reshape(frames[i].shape) for i in range(n)])
    bad = [i for i in range(n) if not np.array_equal(got[i], frames[i])]
    assert bad == [], f"device decode differs from the oracle at frames {bad[:8]}"
    # ... and they are the encoder's own reconstruction
    assert oracle.recon_hash(frames) == facts["recon_hash"]
    mbw, mbh = (facts["width"] + 15) // 16, (facts["height"] + 15) // 16
    assert facts["intra_mbs"] + facts["pcm_mbs"] + facts["inter_mbs"] + facts["skip_mbs"] == n * mbw * mbh
    assert 0 <= facts["qpel_mbs"] <= facts["subpel_mbs"] <= facts["inter_mbs"]
    if subpel == 1:
        assert facts["qpel_mbs"] == 0
    assert sum(on["idr"]) == facts["n_idr"] and on["idr"] == off["idr"]
    print(f"{case} subpel={subpel} intra={int(intra)}: {on['size']} bytes, subpel=0 {off['size']}; facts {facts}")


@pytest.mark.parametrize("intra", [False, True])
@pytest.mark.parametrize("case", USED)
def test_subpel_refinement_is_used(work, case, intra):
    _require_gpu()
    half, quarter = _run(work, case, 1, intra)["facts"], _run(work, case, 2, intra)["facts"]
    print(f"{case} intra={int(intra)}: subpel=1 {half['subpel_mbs']} of {half['inter_mbs']} inter; "
          f"subpel=2 {quarter['subpel_mbs']} ({quarter['qpel_mbs']} quarter) of {quarter['inter_mbs']}")
    assert half["subpel_mbs"] > 0 and quarter["subpel_mbs"] > 0
    if case in ("content", "real"):
        assert quarter["qpel_mbs"] > 0


@pytest.mark.parametrize("intra", [False, True])
def test_subpel_off_is_the_parent_encoder(work, tmp_path, intra):
    """transcode(out), transcode(out, subpel=0) and vts_transcode_ex with
    ext = NULL write equal bytes (tests/test_transcode_gpu.py pins those to
    the byte oracle)."""
    _require_gpu()
    sname, tk, _ = CASES["small"]
    off = _run(work, "small", 0, intra)
    assert off["facts"]["subpel_mbs"] == 0 and off["facts"]["qpel_mbs"] == 0
    if not intra:
        assert off["facts"]["recon_hash"] == 0
    plain = tmp_path / "plain.mp4"
    with scene.VideoScorer(_source(work, sname)) as v:
        v.transcode(plain, intra=intra, **tk)
    assert plain.read_bytes() == off["out"].read_bytes()
    raw = tmp_path / "raw.mp4"
    with scene.VideoScorer(_source(work, sname)) as v:
        prm = _lib.TranscodeParams()
        prm.height = tk["height"]
        prm.intra = int(intra)
        info = _lib.TranscodeInfo()
        _lib.check(v._lib.vts_transcode_ex(v._ctx, str(raw).encode(), C.byref(prm), None, C.byref(info), None))
        assert info.recon_hash == off["facts"]["recon_hash"]
    assert raw.read_bytes() == off["out"].read_bytes()


@pytest.mark.parametrize("intra", [False, True])
@pytest.mark.parametrize("case", USED)
def test_subpel_output_is_smaller(work, case, intra):
    """Quarter-sample refinement must shrink the file the integer encoder
    (the parent's, byte-pinned above) writes of the same input."""
    _require_gpu()
    size = [_run(work, case, sp, intra)["size"] for sp in (0, 1, 2)]
    print(f"{case} intra={int(intra)}: subpel 0 / 1 / 2 = {size[0]} / {size[1]} / {size[2]} bytes, "
          f"source {_source(work, CASES[case][0]).stat().st_size}")
    assert size[2] < size[0]


def test_subpel_sizes_of_every_case(work):
    """The sizes of every case (a record, printed; the assertions are above)."""
    _require_gpu()
    for case, (_, _, both) in CASES.items():
        for intra in (False, True) if both else (False,):
            size = [_run(work, case, sp, intra)["size"] for sp in (0, 1, 2)]
            print(f"{case} intra={int(intra)}: subpel 0 / 1 / 2 = {size[0]} / {size[1]} / {size[2]} bytes")
            assert min(size) > 0


# The spread of PSNR(subpel=0) - PSNR(subpel=2) of the P pictures measured on
# the MI355X across the three inputs (intra=False), -0.93 - (-1.42) = 0.49 dB,
# plus 0.5 dB for input variation (figures in the test's docstring).
QUALITY_MARGIN_DB = 0.99


@pytest.mark.parametrize("case", QUALITY)
def test_subpel_quality_is_not_traded_away(work, case):
    """A smaller file must not be bought with worse pictures: the P pictures
    of the subpel=2 output sit no lower than those of the subpel=0 output
    (the parent encoder) of the same input, less the margin.

    Measured on the MI355X, PSNR over every NV12 byte of the P pictures
    against the oracle's downscale of the oracle's decode of the source,
    qp 28, intra=False (dB):

        case      subpel=0   subpel=2   PSNR(0) - PSNR(2)
        small       41.76      42.79         -1.03
        content     43.53      44.46         -0.93
        real        37.96      39.38         -1.42

    The refined prediction leaves a smaller residual under the same
    quantiser, so quality rises with every input.  Margin = the spread of the
    last column, 0.49 dB, + 0.5 dB; the intra=True pair of each input is held
    to the same margin."""
    _require_gpu()
    ref = _reference(work, case)
    for intra in (False, True):
        r0, r2 = _run(work, case, 0, intra), _run(work, case, 2, intra)
        p = ~np.array(r0["idr"])
        p0, p2 = _psnr(r0["frames"][p], ref[p]), _psnr(r2["frames"][p], ref[p])
        print(f"{case} intra={int(intra)}: P pictures {p0:.2f} dB at subpel=0, {p2:.2f} dB at subpel=2, "
              f"PSNR(0) - PSNR(2) = {p0 - p2:+.2f} dB")
        assert p2 >= p0 - QUALITY_MARGIN_DB


def test_subpel_argument_errors(work, tmp_path):
    _require_gpu()
    sname, tk, _ = CASES["small"]
    src = _source(work, sname)
    for bad in (3, -1):
        with scene.VideoScorer(src) as v:
            with pytest.raises(VtsegError) as ei:
                v.transcode(tmp_path / "a.mp4", subpel=bad, **tk)
            assert ei.value.code == _lib.VTS_E_INVALID
            assert "subpel" in _lib.last_error()
    prm = _lib.TranscodeParams()
    prm.height = tk["height"]
    with scene.VideoScorer(src) as v:
        ext = _lib.TranscodeExt(4, 1)
        rc = v._lib.vts_transcode_ex(v._ctx, str(tmp_path / "b.mp4").encode(), C.byref(prm), C.byref(ext), None, None)
        assert rc == _lib.VTS_E_INVALID

    # a struct 8 bytes larger than the library's, the extra zeroed, is the exact size
    class BigExt(C.Structure):
        _fields_ = [("ext", _lib.TranscodeExt), ("more", C.c_uint64)]

    class BigExtInfo(C.Structure):
        _fields_ = [("info", _lib.TranscodeExtInfo), ("more", C.c_uint64)]

    exact = _run(work, "small", 1, False)
    big = tmp_path / "big.mp4"
    with scene.VideoScorer(src) as v:
        ext, xinfo, info = BigExt(), BigExtInfo(), _lib.TranscodeInfo()
        ext.ext.struct_size, ext.ext.subpel = C.sizeof(BigExt), 1
        xinfo.info.struct_size = C.sizeof(BigExtInfo)
        _lib.check(v._lib.vts_transcode_ex(v._ctx, str(big).encode(), C.byref(prm),
                                           C.cast(C.pointer(ext), C.POINTER(_lib.TranscodeExt)), C.byref(info),
                                           C.cast(C.pointer(xinfo), C.POINTER(_lib.TranscodeExtInfo))))
        assert xinfo.more == 0
        assert (xinfo.info.subpel_mbs, xinfo.info.qpel_mbs) == (exact["facts"]["subpel_mbs"], 0)
        assert info.recon_hash == exact["facts"]["recon_hash"]
    assert big.read_bytes() == exact["out"].read_bytes()
