"""The opt-in in-loop deblocking filter of the device upload transcode
(vts_transcode_ext2.deblock).

With `deblock=True` every slice (one per macroblock row) carries
disable_deblocking_filter_idc = 2 and the two slice offsets, and `enc_deblock`
filters each level's reconstruction before the next level predicts from it.
The bytes are pinned in tests/test_transcode_bytes_gpu.py.  As for Intra16x16 and the sub-sample
refinement, the pin is a closed loop through two independent decoders: the
output is decoded by the CPU general oracle (oracle/h264_full_oracle.c) and by
the device's general decoder, which both implement clause 8.7; the two must
agree, and the hash of the oracle's decode must equal the hash the encoder
computed of its own filtered reconstruction (`recon_hash`), so one sample the
encoder filters differently from a conforming decoder fails, at once or in
every picture predicted from it.  Every transcode runs in a fresh VideoScorer.
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
    "s70": dict(width=320, height=192, n_frames=70),
    "s40": dict(width=320, height=192, n_frames=40),
    "pan": dict(width=320, height=192, n_frames=60, max_motion=24),
    "crop": dict(width=640, height=480, n_frames=30),
    "content": dict(width=640, height=360, n_frames=30, coding="full", bframes=True, content=True,
                    slices_per_row=0, seed=7),
    "real": None,
}
# name -> (source, transcode kwargs, deblock_offsets, also with subpel=2)
CASES = {
    "small": ("s70", dict(height=96), (0, 0), True),                   # the default setting
    "hiqp": ("s70", dict(height=96, qp=40), (0, 0), True),             # bS 4, the strong filter; I_PCM neighbours
    "qp51": ("s40", dict(height=96, qp=51), (6, 6), False),            # index clipping at 51
    "soft": ("s70", dict(height=96), (-6, -6), False),                 # indexA exactly 16
    "lowqp_on": ("s40", dict(height=96, qp=12), (2, 2), False),        # index 16 reached from below
    "keyint8_r16": ("s70", dict(height=96, keyint=8, search_range=16), (0, 0), False),   # many IDR pictures
    "bigpan_edges": ("pan", dict(height=96), (0, 0), False),           # vectors across the clamped edges
    "crop": ("crop", dict(), (0, 0), False),                           # 480x360 in 480x368
    "content": ("content", dict(), (0, 0), True),                      # B-picture content source
    "real": ("real", dict(height=240), (0, 0), True),                  # the real clip
}
LOOP = [(c, i, sp) for c, (_, _, _, sub) in CASES.items() for i in (False, True) for sp in ((0, 2) if sub else (0,))]
QUALITY = ["small", "content", "real"]


def _require_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires an MI355X")


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("deblock"), "src": {}, "run": {}, "ref": {}}


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


def _transcode(work, sname, out, **kw):
    with scene.VideoScorer(_source(work, sname)) as v:
        facts = v.transcode(out, **kw)
    frames, _ = oracle.decode_full(out)
    m = oracle.read_mp4(out)
    return dict(out=out, facts=facts, frames=frames, idr=_is_idr(m), size=out.stat().st_size)


def _run(work, case, deblock, intra, subpel=0):
    """Transcode once per (case, deblock, intra, subpel) in a fresh session;
    the output is decoded by the oracle."""
    key = (case, deblock, intra, subpel)
    if key not in work["run"]:
        sname, tk, offs, _ = CASES[case]
        out = work["dir"] / f"{case}_{int(deblock)}_{int(intra)}_{subpel}.mp4"
        kw = dict(tk, intra=intra, subpel=subpel)
        if deblock:
            kw.update(deblock=True, deblock_offsets=offs)
        work["run"][key] = _transcode(work, sname, out, **kw)
    return work["run"][key]


def _reference(work, case):
    """The encoder's input: the oracle's downscale of the oracle's decode of
    the source, cropped to the display size (NV12 [F, h*3/2, w])."""
    sname, tk, _, _ = CASES[case]
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


def _device_frames(path, n, shape):
    with scene.VideoScorer(path, keep_frames=True) as d:
        d.score()
        general = d.general()
        got = np.stack([d.frame_nv12(i).reshape(shape) for i in range(n)])
    return got, general


@pytest.mark.parametrize("case,intra,subpel", LOOP)
def test_deblocked_output_decodes_to_the_encoders_reconstruction(work, case, intra, subpel):
    _require_gpu()
    on, off = _run(work, case, True, intra, subpel), _run(work, case, False, intra, subpel)
    facts, frames = on["facts"], on["frames"]
    n = facts["n_frames"]
    assert frames.shape[0] == n
    # the device's general decoder reads the same pictures as the oracle
    got, general = _device_frames(on["out"], n, frames[0].shape)
    assert general
    bad = [i for i in range(n) if not np.array_equal(got[i], frames[i])]
    assert bad == [], f"device decode differs from the oracle at frames {bad[:8]}"
    # ... and they are the encoder's own (filtered) reconstruction
    assert oracle.recon_hash(frames) == facts["recon_hash"]
    mbw, mbh = (facts["width"] + 15) // 16, (facts["height"] + 15) // 16
    assert facts["intra_mbs"] + facts["pcm_mbs"] + facts["inter_mbs"] + facts["skip_mbs"] == n * mbw * mbh
    assert sum(on["idr"]) == facts["n_idr"] and on["idr"] == off["idr"]
    print(f"{case} intra={int(intra)} subpel={subpel}: {on['size']} bytes, deblock off {off['size']}; facts {facts}")
    assert 0 < facts["deblock_mbs"] <= n * mbw * mbh
    assert off["facts"]["deblock_mbs"] == 0


def test_deblock_below_index_16_filters_nothing(work, tmp_path):
    """qp 12 with zero offsets: indexA <= 12 everywhere, alpha' = 0.  The
    slices still ask for the filter, no sample moves, and the pictures are
    those of the deblock=False output."""
    _require_gpu()
    on = _transcode(work, "s40", tmp_path / "on.mp4", height=96, qp=12, deblock=True)
    off = _transcode(work, "s40", tmp_path / "off.mp4", height=96, qp=12)
    assert on["facts"]["deblock_mbs"] == 0
    assert np.array_equal(on["frames"], off["frames"])
    assert on["facts"]["recon_hash"] == oracle.recon_hash(on["frames"])
    got, _ = _device_frames(on["out"], on["facts"]["n_frames"], on["frames"][0].shape)
    assert np.array_equal(got, on["frames"])
    assert on["out"].read_bytes() != off["out"].read_bytes()   # the slice headers differ


@pytest.mark.parametrize("intra", [False, True])
def test_deblock_off_is_the_parent_encoder(work, tmp_path, intra):
    """transcode(out), transcode(out, deblock=False) and vts_transcode_ex with
    a plain 8-byte vts_transcode_ext write equal bytes (tests/test_transcode_gpu.py
    pins those to the byte oracle), and deblock_mbs is 0 in each."""
    _require_gpu()
    sname, tk, _, _ = CASES["small"]
    off = _run(work, "small", False, intra)
    assert off["facts"]["deblock_mbs"] == 0
    if not intra:
        assert off["facts"]["recon_hash"] == 0
    explicit = tmp_path / "explicit.mp4"
    with scene.VideoScorer(_source(work, sname)) as v:
        facts = v.transcode(explicit, intra=intra, deblock=False, deblock_offsets=(0, 0), **tk)
    assert facts["deblock_mbs"] == 0
    assert explicit.read_bytes() == off["out"].read_bytes()
    raw = tmp_path / "raw.mp4"
    with scene.VideoScorer(_source(work, sname)) as v:
        prm = _lib.TranscodeParams()
        prm.height = tk["height"]
        prm.intra = int(intra)
        info = _lib.TranscodeInfo()
        ext = _lib.TranscodeExt(C.sizeof(_lib.TranscodeExt), 0)
        xinfo = _lib.TranscodeExtInfo2(_lib.TranscodeExtInfo(C.sizeof(_lib.TranscodeExtInfo2)))
        xinfo.deblock_mbs = -1
        _lib.check(v._lib.vts_transcode_ex(v._ctx, str(raw).encode(), C.byref(prm), C.byref(ext), C.byref(info),
                                           C.cast(C.pointer(xinfo), C.POINTER(_lib.TranscodeExtInfo))))
        assert xinfo.deblock_mbs == 0
        assert info.recon_hash == off["facts"]["recon_hash"]
    assert raw.read_bytes() == off["out"].read_bytes()


def _raw_ext2(v, out, height, size, deblock, alpha, beta, qp=0):
    prm = _lib.TranscodeParams()
    prm.height = height
    prm.qp = qp
    ext = _lib.TranscodeExt2(_lib.TranscodeExt(size, 0), deblock, alpha, beta)
    xinfo = _lib.TranscodeExtInfo2(_lib.TranscodeExtInfo(C.sizeof(_lib.TranscodeExtInfo2)))
    info = _lib.TranscodeInfo()
    rc = v._lib.vts_transcode_ex(v._ctx, str(out).encode(), C.byref(prm),
                                 C.cast(C.pointer(ext), C.POINTER(_lib.TranscodeExt)), C.byref(info),
                                 C.cast(C.pointer(xinfo), C.POINTER(_lib.TranscodeExtInfo)))
    return rc, info, xinfo


def test_deblock_argument_errors(work, tmp_path):
    _require_gpu()
    sname, tk, _, _ = CASES["small"]
    src = _source(work, sname)
    full = C.sizeof(_lib.TranscodeExt2)
    # (deblock, alpha, beta, qp) -> the field the message names
    bad = [((2, 0, 0, 0), "deblock "), ((-1, 0, 0, 0), "deblock "),
           ((1, 7, 0, 0), "deblock_alpha"), ((1, -7, 0, 0), "deblock_alpha"),
           ((1, 0, 7, 0), "deblock_beta"), ((1, 0, -7, 0), "deblock_beta"),
           ((0, 1, 0, 0), "deblock_alpha"), ((0, 0, -1, 0), "deblock_beta"),
           ((1, 0, 0, -1), "deblock")]
    for (dbk, al, be, qp), name in bad:
        with scene.VideoScorer(src) as v:
            rc, _, _ = _raw_ext2(v, tmp_path / "bad.mp4", tk["height"], full, dbk, al, be, qp)
            assert rc == _lib.VTS_E_INVALID, (dbk, al, be, qp)
            assert name in _lib.last_error(), (_lib.last_error(), name)
    # the same through the Python keywords
    for kw in (dict(deblock=True, deblock_offsets=(7, 0)), dict(deblock_offsets=(0, 1)), dict(deblock=True, qp=0)):
        with scene.VideoScorer(src) as v:
            with pytest.raises(VtsegError) as ei:
                v.transcode(tmp_path / "bad.mp4", height=tk["height"], **kw)
            assert ei.value.code == _lib.VTS_E_INVALID
            assert "deblock" in _lib.last_error()


def test_deblock_partial_struct(work, tmp_path):
    """struct_size 12 reaches `deblock` alone: the filter is on with zero
    offsets, whatever lies behind it."""
    _require_gpu()
    sname, tk, _, _ = CASES["small"]
    exact = _run(work, "small", True, False)
    part = tmp_path / "part.mp4"
    with scene.VideoScorer(_source(work, sname)) as v:
        rc, info, xinfo = _raw_ext2(v, part, tk["height"], 12, 1, 5, -5)
        _lib.check(rc)
        assert xinfo.deblock_mbs == exact["facts"]["deblock_mbs"] > 0
        assert info.recon_hash == exact["facts"]["recon_hash"]
    assert part.read_bytes() == exact["out"].read_bytes()


def test_deblock_sizes_of_every_case(work):
    """The sizes of every case, deblock off / on (a record, printed: a
    filtered reference can move bits either way, so nothing is asserted on
    the direction)."""
    _require_gpu()
    for case, intra, subpel in LOOP:
        off, on = _run(work, case, False, intra, subpel), _run(work, case, True, intra, subpel)
        print(f"{case} intra={int(intra)} subpel={subpel}: deblock off / on = {off['size']} / {on['size']} bytes, "
              f"deblock_mbs {on['facts']['deblock_mbs']}")
        assert min(off["size"], on["size"]) > 0


# The spread of PSNR(deblock off) - PSNR(deblock on) of the P pictures measured
# on the MI355X across the three inputs (intra=False), -0.73 - (-1.45) = 0.72 dB,
# plus 0.5 dB for input variation (figures in the test's docstring).
QUALITY_MARGIN_DB = 1.22


@pytest.mark.parametrize("case", QUALITY)
def test_deblock_quality_is_not_traded_away(work, case):
    """The P pictures of the deblock=True output sit no lower than those of
    the deblock=False output (the parent encoder, byte-pinned) of the same
    input, less the margin.  PSNR over every NV12 byte of the P pictures
    against the oracle's downscale of the oracle's decode of the source,
    qp 28.

    Measured on the MI355X (dB):

        case     intra   deblock off   deblock on   PSNR(off) - PSNR(on)
        small    False      41.76        42.95           -1.19
        content  False      43.53        44.97           -1.45
        real     False      37.96        38.68           -0.73
        small    True       38.52        39.96           -1.44
        content  True       40.58        43.04           -2.47
        real     True       37.65        38.54           -0.89

    The filtered reference predicts better and the filtered picture is closer
    to the source, so quality rises with every input (the Intra16x16 IDR
    pictures too: 37.91 -> 38.97, 39.56 -> 41.71, 39.13 -> 39.75).  Margin =
    the spread of the last column over the three intra=False rows, 0.72 dB,
    + 0.5 dB; the intra=True pair of each input is held to the same margin."""
    _require_gpu()
    ref = _reference(work, case)
    for intra in (False, True):
        r0, r1 = _run(work, case, False, intra), _run(work, case, True, intra)
        p = ~np.array(r0["idr"])
        p0, p1 = _psnr(r0["frames"][p], ref[p]), _psnr(r1["frames"][p], ref[p])
        i0, i1 = _psnr(r0["frames"][~p], ref[~p]), _psnr(r1["frames"][~p], ref[~p])
        print(f"{case} intra={int(intra)}: P pictures {p0:.2f} dB off, {p1:.2f} dB on, "
              f"PSNR(off) - PSNR(on) = {p0 - p1:+.2f} dB; IDR pictures {i0:.2f} dB off, {i1:.2f} dB on")
        assert p1 >= p0 - QUALITY_MARGIN_DB
