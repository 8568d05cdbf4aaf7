"""The opt-in Intra16x16 coder of the device upload transcode
(vts_transcode_params.intra).

The bytes are pinned in tests/test_transcode_bytes_gpu.py.  The pin here is a closed loop through
two independent decoders: the output of `transcode(intra=True)` is decoded by
the CPU general oracle (oracle/h264_full_oracle.c) and by the device's general
decoder; the two must agree, and the hash of the oracle's decode must equal
the hash the encoder computed of its own reconstruction (`recon_hash`), so
any drift between the encoder's reconstruction and a conforming decoder fails.
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
SMALL = dict(width=320, height=192, n_frames=70)
SOURCES = {
    "small": SMALL,
    "crop": dict(width=640, height=480, n_frames=30),
    # content mode needs B pictures; 640x360 is the smallest source the default
    # 360-line output accepts
    "content": dict(width=640, height=360, n_frames=30, coding="full", bframes=True, content=True,
                    slices_per_row=0, seed=7),
    "real": None,
}
# name -> (source, transcode kwargs)
CASES = {
    "small": ("small", dict(height=96)),
    "keyint8": ("small", dict(height=96, keyint=8, search_range=16)),
    "crop": ("crop", dict()),
    "qp20": ("small", dict(height=96, qp=20)),
    "qp36": ("small", dict(height=96, qp=36)),
    "idr_at_cuts": ("small", dict(height=96, idr_at_cuts=True)),
    "content": ("content", dict()),
    "real": ("real", dict(height=240)),  # the clip is 320x240: its own height
}
QUALITY = ["small", "content", "real"]


def _require_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires an MI355X")


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("intra"), "src": {}, "run": {}, "ref": {}}


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


def _run(work, case, intra):
    """Transcode once per (case, intra); the output is decoded by the oracle."""
    key = (case, intra)
    if key not in work["run"]:
        sname, tk = CASES[case]
        out = work["dir"] / f"{case}_{int(intra)}.mp4"
        with scene.VideoScorer(_source(work, sname)) as v:
            facts = v.transcode(out, intra=intra, **tk)
        frames, _ = oracle.decode_full(out)
        m = oracle.read_mp4(out)
        work["run"][key] = dict(out=out, facts=facts, frames=frames, sizes=list(m["sizes"]), idr=_is_idr(m))
    return work["run"][key]


def _reference(work, case):
    """The encoder's input: the oracle's downscale of the oracle's decode of
    the source, cropped to the display size (NV12 [F, h*3/2, w])."""
    sname, tk = CASES[case]
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


@pytest.mark.parametrize("case", list(CASES))
def test_intra_output_decodes_to_the_encoders_reconstruction(work, case):
    _require_gpu()
    on, off = _run(work, case, True), _run(work, case, False)
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
    assert facts["intra_mbs"] > 0
    assert sum(on["idr"]) == facts["n_idr"] and on["idr"] == off["idr"]
    for i, (size, idr) in enumerate(zip(on["sizes"], on["idr"])):
        if idr:
            assert size < 384 * mbw * mbh, f"IDR sample {i}"
    # a macroblock is intra-coded only under the I_PCM bit bound
    assert on["out"].stat().st_size < off["out"].stat().st_size
    print(f"{case}: {on['out'].stat().st_size} bytes with intra, {off['out'].stat().st_size} without, "
          f"source {_source(work, CASES[case][0]).stat().st_size}; facts {facts}")


def test_intra_off_is_the_default_encoder(work, tmp_path):
    _require_gpu()
    off = _run(work, "small", False)
    assert off["facts"]["intra_mbs"] == 0 and off["facts"]["recon_hash"] == 0
    plain = tmp_path / "plain.mp4"
    with scene.VideoScorer(_source(work, "small")) as v:
        v.transcode(plain, **CASES["small"][1])
    assert plain.read_bytes() == off["out"].read_bytes()


def test_intra_argument_errors(work, tmp_path):
    _require_gpu()
    with scene.VideoScorer(_source(work, "small")) as v:
        with pytest.raises(VtsegError) as ei:
            v.transcode(tmp_path / "a.mp4", height=96, qp=0, intra=True)  # qp 0: no residual
        assert ei.value.code == _lib.VTS_E_INVALID
        prm = _lib.TranscodeParams()
        prm.height = 96
        prm.intra = 2
        info = _lib.TranscodeInfo()
        rc = v._lib.vts_transcode(v._ctx, str(tmp_path / "b.mp4").encode(), C.byref(prm), C.byref(info))
        assert rc == _lib.VTS_E_INVALID
        assert "intra" in _lib.last_error()


# The spread of (IDR PSNR with intra) - (P PSNR of the intra=False encoder)
# measured on the MI355X across the three inputs, 1.18 - (-3.96) = 5.14 dB,
# plus 0.5 dB for input variation (figures in the test's docstring).
QUALITY_MARGIN_DB = 5.64


@pytest.mark.parametrize("case", QUALITY)
def test_intra_idr_quality_near_the_p_pictures(work, case):
    """The quantiser is the same for intra and inter macroblocks, so the IDR
    pictures of the intra=True output should sit near the P pictures of the
    intra=False output (the parent encoder) of the same input.

    Measured on the MI355X, PSNR over every NV12 byte against the oracle's
    downscale of the oracle's decode of the source, qp 28 (dB):

        case     IDR, intra   P, intra   P, intra=False   IDR - P(intra=False)
        small       37.91       38.52        41.76              -3.85
        content     39.56       40.58        43.53              -3.96
        real        39.13       37.65        37.96              +1.18

    Within one intra=True file the IDR and P pictures are 0.6 .. 1.5 dB apart.
    The intra=False encoder's P pictures of the two synthetic inputs sit
    higher because they predict from a lossless (I_PCM) IDR picture that the
    flat synthetic scenes then mostly copy.  Margin = the spread of the last
    column, 5.14 dB, + 0.5 dB."""
    _require_gpu()
    on, off = _run(work, case, True), _run(work, case, False)
    ref = _reference(work, case)
    idr = np.array(on["idr"])
    idr_on = _psnr(on["frames"][idr], ref[idr])
    p_on = _psnr(on["frames"][~idr], ref[~idr])
    p_off = _psnr(off["frames"][~idr], ref[~idr])
    print(f"{case}: IDR {idr_on:.2f} dB, P {p_on:.2f} dB with intra; parent P {p_off:.2f} dB; "
          f"IDR - parent P = {idr_on - p_off:+.2f} dB")
    assert idr_on >= p_off - QUALITY_MARGIN_DB
