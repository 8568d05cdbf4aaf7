"""CABAC entropy coding in the device encoder (vts_transcode_ext4.cabac,
DESIGN.md §11).

Entropy coding is lossless, so the pin is the same call with `cabac=False`,
whose bytes tests/test_transcode_bytes_gpu.py holds to the written rules:

1. every count, `recon_hash` and command word equals those of that call, and
   the CPU general oracle and the device's general decoder decode the CABAC
   file to the pictures of the CAVLC file;
2. the avcC says Main and entropy_coding_mode_flag = 1, and `cabac=False` is
   the file written without the keyword;
3. I_PCM macroblocks (each a flush, the samples and a restart of the
   arithmetic encoder) in IDR pictures and inside P slices;
4. the bytes do not change between sessions or within one;
5. at qp 28 with `intra` the CABAC file of `real` and of `content` is smaller;
6. the argument errors and the struct sizes.

Every transcode runs in a fresh VideoScorer unless the test says otherwise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
from test_transcode_rate_gpu import SOURCES, _device_frames, _is_idr, _source, _transcode  # noqa: F401
from test_transcode_subpel_gpu import _require_gpu
from vtseg import VtsegError, _lib, scene

pytestmark = pytest.mark.gpu

PCM = 0x80008000
ALL_ON = dict(intra=True, subpel=2, deblock=True)
RATE = dict(mvcost=True, early_skip=True)
EVERY = dict(**ALL_ON, **RATE)
# name -> (source, transcode kwargs of both runs)
CASES = {
    # `small`, 320x192 -> 160x96: all flags off, each alone, everything
    "small_off": ("s70", dict(height=96)),
    "small_intra": ("s70", dict(height=96, intra=True)),
    "small_sp2": ("s70", dict(height=96, subpel=2)),
    "small_dbk": ("s70", dict(height=96, deblock=True)),
    "small_rate": ("s70", dict(height=96, **RATE)),
    "small_every": ("s70", dict(height=96, **EVERY)),
    # the quantiser's ends: large levels (the UEG0 suffix) and none at all
    "qp1_every": ("s40", dict(height=96, qp=1, **EVERY)),
    "qp40_every": ("s70", dict(height=96, qp=40, **EVERY)),
    "qp51_every": ("s40", dict(height=96, qp=51, deblock_offsets=(6, 6), **EVERY)),
    "r0_every": ("s40", dict(height=96, search_range=-1, **EVERY)),
    "keyint8_r16_every": ("s70", dict(height=96, keyint=8, search_range=16, **EVERY)),   # many IDR pictures
    "allpcm": ("s40", dict(height=96, max_mb_sad=-1)),                          # every macroblock of every P slice I_PCM
    "allpcm_intra": ("s40", dict(height=96, max_mb_sad=-1, intra=True)),       # Intra16x16 rows in P slices
    "tiny_every": ("tiny", dict(height=24, search_range=4, **EVERY)),           # 2 x 2 macroblocks
    "column_every": ("column", dict(height=48, search_range=4, **EVERY)),       # 1 x 3: never a left neighbour
    "bigpan_edges_every": ("pan", dict(height=96, **EVERY)),
    "crop_every": ("crop", dict(**EVERY)),                                     # 30 macroblocks a slice
    "real_intra": ("real", dict(height=240, intra=True)),
    "real_every": ("real", dict(height=240, **EVERY)),
    "content_intra": ("content", dict(intra=True)),
    "content_every": ("content", dict(**EVERY)),
    # built frames: every macroblock kind inside P slices (I_PCM at a low qp); a constant picture
    "crafted_qp4_intra": ("crafted", dict(height=64, qp=4, intra=True)),
    "crafted_qp12_every": ("crafted", dict(height=64, qp=12, **EVERY)),
    "crafted_off": ("crafted", dict(height=64)),
    "flat_every": ("flat", dict(height=64, **EVERY)),
    # display widths that are no multiple of 16: 72x128 coded 80x128, 88x72 coded 96x80
    "portrait_every": ("portrait", dict(height=128, **EVERY)),
    "qcif_every": ("qcif", dict(height=72, **EVERY)),
}
SAME = ("width", "height", "n_frames", "n_idr", "pcm_mbs", "inter_mbs", "skip_mbs", "intra_mbs", "subpel_mbs",
        "qpel_mbs", "deblock_mbs", "early_skip_mbs", "recon_hash")


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("cabac"), "src": {}, "dec": {}, "run": {}}


def _pair(work, case):
    """The case transcoded with cabac off and on (a fresh session each), once per module."""
    if case not in work["run"]:
        sname, kw = CASES[case]
        r = {}
        for on in (False, True):
            out = work["dir"] / f"{case}_{int(on)}.mp4"
            r[on] = (out, _transcode(work, sname, out, cabac=on, want_commands=True, **kw))
        work["run"][case] = r
    return work["run"][case]


def _parameter_sets(path):
    m = oracle.read_mp4(path)
    return m["sps"][0], m["pps"][0]


# ------------------------------------------------- 1. lossless against CAVLC
@pytest.mark.parametrize("case", list(CASES))
def test_cabac_codes_what_cavlc_codes(work, case):
    _require_gpu()
    (off_path, off), (on_path, on) = _pair(work, case)[False], _pair(work, case)[True]
    for k in SAME:
        assert on[k] == off[k], f"{k}: {on[k]} with cabac, {off[k]} without"
    assert np.array_equal(on["commands"], off["commands"])
    want, _ = oracle.decode_full(off_path)
    frames, _ = oracle.decode_full(on_path)
    n = on["n_frames"]
    assert frames.shape == want.shape and frames.shape[0] == n
    bad = [i for i in range(n) if not np.array_equal(frames[i], want[i])]
    assert bad == [], f"the oracle's decode of the CABAC file differs at frames {bad[:8]}"
    got, general = _device_frames(on_path, n, frames[0].shape)
    assert general
    bad = [i for i in range(n) if not np.array_equal(got[i], frames[i])]
    assert bad == [], f"the device decode of the CABAC file differs at frames {bad[:8]}"
    kw = CASES[case][1]
    if any(kw.get(k) for k in ("intra", "subpel", "deblock", "mvcost", "early_skip")):
        assert on["recon_hash"] != 0 and oracle.recon_hash(frames) == on["recon_hash"]
    else:
        assert on["recon_hash"] == 0
    print(f"{case}: cavlc {off_path.stat().st_size} bytes, cabac {on_path.stat().st_size} bytes; "
          f"pcm {on['pcm_mbs']} intra {on['intra_mbs']} inter {on['inter_mbs']} skip {on['skip_mbs']}; "
          f"write_ms {off['write_ms']:.2f} -> {on['write_ms']:.2f}")


def test_default_qp_through_the_c_interface(work, tmp_path):
    """vts_transcode_params.qp = 0 is the default 28: the raw call with cabac = 1 writes the keyword's file."""
    _require_gpu()
    on_path, _ = _pair(work, "small_off")[True]
    with scene.VideoScorer(_source(work, "s70")) as v:
        rc, _ = _raw_ext4(v, tmp_path / "raw.mp4", 96, C.sizeof(_lib.TranscodeExt4), cabac=1, qp=0)
        _lib.check(rc)
    assert (tmp_path / "raw.mp4").read_bytes() == on_path.read_bytes()


# ------------------------------------------- 2. the stream says what it is
@pytest.mark.parametrize("case", ["small_off", "small_every", "crop_every"])
def test_parameter_sets_and_the_default(work, tmp_path, case):
    _require_gpu()
    (off_path, _), (on_path, _) = _pair(work, case)[False], _pair(work, case)[True]
    sps, pps = _parameter_sets(on_path)
    sps0, pps0 = _parameter_sets(off_path)
    assert sps[0] & 31 == 7 and sps[1] == 77 and sps[2] == 0x40          # Main, constraint_set1_flag
    assert sps0[1] == 66 and sps0[2] == 0xC0 and sps[3:] == sps0[3:]     # level and everything behind it as before
    # PPS RBSP: ue(0) ue(0) entropy_coding_mode_flag ...
    assert pps[0] & 31 == 8 and pps[1] >> 5 == 0b111 and pps0[1] >> 5 == 0b110
    assert pps[1] & 31 == pps0[1] & 31 and pps[2:] == pps0[2:]
    m = oracle.read_mp4(on_path)
    first = m["data"][m["offsets"][0]:m["offsets"][0] + m["sizes"][0]]
    assert first[4] == 0x65                                               # an IDR slice, not in-band parameter sets
    sname, kw = CASES[case]
    _transcode(work, sname, tmp_path / "plain.mp4", **kw)                 # no cabac keyword, no want_commands
    assert (tmp_path / "plain.mp4").read_bytes() == off_path.read_bytes()


# ------------------------------------------------------------ 3. I_PCM paths
def test_every_idr_macroblock_i_pcm(work):
    """intra = 0: each macroblock of an IDR picture is I_PCM, so each one flushes and restarts the encoder."""
    _require_gpu()
    (_, off), (on_path, on) = _pair(work, "small_off")[False], _pair(work, "small_off")[True]
    idr = np.array(_is_idr(on_path))
    assert (on["commands"][idr] == PCM).all() and on["pcm_mbs"] >= idr.sum() * 60 and on["pcm_mbs"] == off["pcm_mbs"]


@pytest.mark.parametrize("case", ["allpcm", "crafted_qp4_intra"])
def test_i_pcm_inside_p_slices(work, case):
    _require_gpu()
    on_path, on = _pair(work, case)[True]
    p = ~np.array(_is_idr(on_path))
    cmds = on["commands"][p]
    assert (cmds == PCM).any()
    if case == "allpcm":
        assert (cmds == PCM).all()
    else:            # I_PCM next to Intra16x16 and inter macroblocks in the same slices
        i16 = (cmds & 0xffff8000) == 0x80000000
        assert i16.any() and ((cmds != PCM) & ~i16).any()
        rows = cmds.reshape(-1, cmds.shape[-1])
        assert any((r == PCM).any() and (r != PCM).any() for r in rows)


# -------------------------------------------------------------- 4. stability
@pytest.mark.parametrize("case", ["small_every", "crafted_qp4_intra", "content_every"])
def test_the_bytes_repeat_in_fresh_sessions(work, tmp_path, case):
    _require_gpu()
    want = _pair(work, case)[True][0].read_bytes()
    sname, kw = CASES[case]
    for i in range(3):
        out = tmp_path / f"again{i}.mp4"
        _transcode(work, sname, out, cabac=True, **kw)
        assert out.read_bytes() == want, f"run {i}"


def test_off_on_off_on_in_one_session(work, tmp_path):
    _require_gpu()
    sname, kw = CASES["small_every"]
    want = {on: _pair(work, "small_every")[on][0].read_bytes() for on in (False, True)}
    with scene.VideoScorer(_source(work, sname)) as v:
        for i, on in enumerate((False, True, False, True)):
            out = tmp_path / f"o{i}.mp4"
            v.transcode(out, cabac=on, **kw)
            assert out.read_bytes() == want[on], f"transcode {i} (cabac={on})"


# ------------------------------------------------------------------- 5. size
@pytest.mark.parametrize("case", ["real_intra", "content_intra"])
def test_cabac_is_smaller_at_qp28_with_intra(work, case):
    _require_gpu()
    off, on = (_pair(work, case)[k][0].stat().st_size for k in (False, True))
    print(f"{case}: cavlc {off} bytes, cabac {on} bytes ({on / off:.4f})")
    assert on < off


# ----------------------------------------------------------------- 6. errors
def _raw_ext4(v, out, height, size, *, cabac=0, qp=0, intra=0):
    prm = _lib.TranscodeParams()
    prm.height = height
    prm.qp = qp
    prm.intra = intra
    ext = _lib.TranscodeExt4(_lib.TranscodeExt3(_lib.TranscodeExt2(_lib.TranscodeExt(size, 0))), cabac, 0x55555555)
    info = _lib.TranscodeInfo()
    rc = v._lib.vts_transcode_ex(v._ctx, str(out).encode(), C.byref(prm),
                                 C.cast(C.pointer(ext), C.POINTER(_lib.TranscodeExt)), C.byref(info), None)
    return rc, info


def test_argument_errors_and_struct_sizes(work, tmp_path):
    _require_gpu()
    src = _source(work, "s40")
    full = C.sizeof(_lib.TranscodeExt4)
    assert full == 64
    for fields in (dict(cabac=2), dict(cabac=-1), dict(cabac=1, qp=-1)):
        with scene.VideoScorer(src) as v:
            rc, _ = _raw_ext4(v, tmp_path / "bad.mp4", 96, full, **fields)
            assert rc == _lib.VTS_E_INVALID, fields
            assert "cabac" in _lib.last_error(), _lib.last_error()
    with scene.VideoScorer(src) as v:
        with pytest.raises(VtsegError) as ei:
            v.transcode(tmp_path / "bad.mp4", height=96, qp=0, cabac=True)
        assert ei.value.code == _lib.VTS_E_INVALID
    # a 56-byte struct (vts_transcode_ext3) with cabac = 1 behind it: not read; 60 bytes: honoured; 64: the same file
    files = {}
    for size in (56, 60, 64):
        out = tmp_path / f"s{size}.mp4"
        with scene.VideoScorer(src) as v:
            rc, _ = _raw_ext4(v, out, 96, size, cabac=1)
            _lib.check(rc)
        files[size] = out.read_bytes()
        assert _parameter_sets(out)[0][1] == (66 if size == 56 else 77)
    with scene.VideoScorer(src) as v:
        prm = _lib.TranscodeParams()
        prm.height = 96
        _lib.check(v._lib.vts_transcode(v._ctx, str(tmp_path / "base.mp4").encode(), C.byref(prm), None))
    assert files[56] == (tmp_path / "base.mp4").read_bytes()
    assert files[60] == files[64] != files[56]
    with scene.VideoScorer(src) as v:      # cabac = 2 behind a 56-byte struct is not an error either
        rc, _ = _raw_ext4(v, tmp_path / "ok.mp4", 96, 56, cabac=2)
        _lib.check(rc)
