"""Intra_4x4 coding of intra macroblocks in the device encoder
(vts_transcode_ext5.intra4x4, DESIGN.md §11 "Intra4x4").

1. Closed loop: the output is decoded by the CPU general oracle and by the
   device's general decoder; the two agree, the hash of the decode is the
   encoder's `recon_hash`, and the counts add up.
2. CABAC is still lossless: every count, `recon_hash`, command word and mode
   word of the `cabac=True` run equals the `cabac=False` run's, and the two
   files decode to the same pictures.
3. Every mode the encoder reports lies in the set its block may use.
4. Off is the parent: `intra4x4 = 0` through the 88-byte struct writes the
   byte oracle's bytes.
5. On `real` and `content` the output is smaller and the IDR pictures lose no
   more than 0.5 dB.
6. The argument errors and the struct sizes.

Every transcode runs in a fresh VideoScorer unless the test says otherwise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
from test_transcode_bytes_gpu import _oracle_side
from test_transcode_rate_gpu import SOURCES, _device_frames, _is_idr, _source, _transcode  # noqa: F401
from test_transcode_subpel_gpu import _psnr, _require_gpu
from vtseg import VtsegError, _lib, scene

pytestmark = pytest.mark.gpu

PCM = 0x80008000
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
EVERY = dict(intra=True, subpel=2, deblock=True, mvcost=True, early_skip=True)
# name -> (source, transcode kwargs besides intra4x4 / cabac, the case must contain I_NxN macroblocks)
CASES = {
    "small_intra": ("s70", dict(height=96, intra=True), True),
    "small_every": ("s70", dict(height=96, **EVERY), True),
    "keyint8_r16_every": ("s70", dict(height=96, keyint=8, search_range=16, **EVERY), True),   # many IDR levels
    "allpcm_intra": ("s40", dict(height=96, max_mb_sad=-1, intra=True), True),     # intra rows in P slices: mb_type 5
    "crafted_qp4_intra": ("crafted", dict(height=64, qp=4, intra=True), True),     # I_PCM neighbours: nC 16, predictor 2
    "qp1_every": ("s40", dict(height=96, qp=1, **EVERY), False),
    "qp51_every": ("s40", dict(height=96, qp=51, deblock_offsets=(6, 6), **EVERY), False),
    "tiny_every": ("tiny", dict(height=24, search_range=4, **EVERY), False),       # 2 x 2 macroblocks
    "column_every": ("column", dict(height=48, search_range=4, **EVERY), False),   # never a left neighbour
    "portrait_every": ("portrait", dict(height=128, **EVERY), False),              # 72 wide, coded 80
    "qcif_every": ("qcif", dict(height=72, **EVERY), False),                       # 88 wide, coded 96
    "flat_every": ("flat", dict(height=64, **EVERY), False),
    "real_every": ("real", dict(height=240, **EVERY), True),
    "content_every": ("content", dict(**EVERY), True),
}
SAME = ("width", "height", "n_frames", "n_idr", "pcm_mbs", "inter_mbs", "skip_mbs", "intra_mbs", "intra4x4_mbs",
        "subpel_mbs", "qpel_mbs", "deblock_mbs", "early_skip_mbs", "recon_hash")
# luma4x4BlkIdx -> (column, row) of the block in the macroblock (6.4.3)
BLK_XY = [(2 * ((k >> 2) & 1) + (k & 1), 2 * (k >> 3) + ((k >> 1) & 1)) for k in range(16)]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("intra4"), "src": {}, "dec": {}, "ref": {}, "run": {}, "frames": {}}


def _pair(work, case):
    """The case transcoded with intra4x4 on, cabac off and on (a fresh session each), once per module."""
    if case not in work["run"]:
        sname, kw, _ = CASES[case]
        r = {}
        for cabac in (False, True):
            out = work["dir"] / f"{case}_{int(cabac)}.mp4"
            r[cabac] = (out, _transcode(work, sname, out, intra4x4=True, cabac=cabac, want_commands=True,
                                        want_intra4_modes=True, **kw))
        work["run"][case] = r
    return work["run"][case]


def _decoded(work, path):
    if path not in work["frames"]:
        work["frames"][path] = oracle.decode_full(path)[0]
    return work["frames"][path]


def _allowed(k, mx):
    """The Intra4x4PredModes of block k at macroblock column mx: the row above the macroblock is another slice."""
    bx, by = BLK_XY[k]
    top, left = by > 0, bx > 0 or mx > 0
    ok = {2}
    if top:
        ok |= {0, 3, 7}
    if left:
        ok |= {1, 8}
    if top and left:
        ok |= {4, 5, 6}
    return ok


# ------------------------------------------------------------- 1. closed loop
@pytest.mark.parametrize("cabac", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_output_decodes_to_the_encoders_reconstruction(work, case, cabac):
    _require_gpu()
    out, facts = _pair(work, case)[cabac]
    frames = _decoded(work, out)
    n = facts["n_frames"]
    assert frames.shape[0] == n
    got, general = _device_frames(out, n, frames[0].shape)
    assert general
    bad = [i for i in range(n) if not np.array_equal(got[i], frames[i])]
    assert bad == [], f"device decode differs from the oracle at frames {bad[:8]}"
    assert facts["recon_hash"] != 0 and oracle.recon_hash(frames) == facts["recon_hash"]
    mbw, mbh = (facts["width"] + 15) // 16, (facts["height"] + 15) // 16
    assert facts["intra_mbs"] + facts["pcm_mbs"] + facts["inter_mbs"] + facts["skip_mbs"] == n * mbw * mbh
    assert 0 <= facts["intra4x4_mbs"] <= facts["intra_mbs"]
    if CASES[case][2]:
        assert facts["intra4x4_mbs"] > 0
    print(f"{case} cabac={cabac}: {out.stat().st_size} bytes; I_NxN {facts['intra4x4_mbs']} of intra "
          f"{facts['intra_mbs']}, pcm {facts['pcm_mbs']} inter {facts['inter_mbs']} skip {facts['skip_mbs']}")


def test_intra_rows_inside_p_slices_hold_i_nxn(work):
    """max_mb_sad = -1: every P macroblock goes through enc_intra, so P slices carry mb_type 5."""
    _require_gpu()
    out, facts = _pair(work, "allpcm_intra")[False]
    p = ~np.array(_is_idr(out))
    assert ((facts["commands"][p] & 0xffffc000) == 0x80004000).any()
    assert facts["inter_mbs"] == 0 and facts["skip_mbs"] == 0


def test_i_pcm_next_to_i_nxn(work):
    _require_gpu()
    _, facts = _pair(work, "crafted_qp4_intra")[False]
    cmds = facts["commands"]
    rows = cmds.reshape(-1, cmds.shape[-1])
    i4 = (rows & 0xffffc000) == 0x80004000
    assert ((rows[:, :-1] == PCM) & i4[:, 1:]).any(), "no I_NxN macroblock right of an I_PCM one"


# ------------------------------------------------ 2. CABAC is still lossless
@pytest.mark.parametrize("case", list(CASES))
def test_cabac_codes_what_cavlc_codes(work, case):
    _require_gpu()
    (off_path, off), (on_path, on) = _pair(work, case)[False], _pair(work, case)[True]
    for k in SAME:
        assert on[k] == off[k], f"{k}: {on[k]} with cabac, {off[k]} without"
    assert np.array_equal(on["commands"], off["commands"])
    assert np.array_equal(on["intra4_modes"], off["intra4_modes"])
    assert np.array_equal(_decoded(work, on_path), _decoded(work, off_path))


# ------------------------------------------------------------ 3. mode legality
@pytest.mark.parametrize("case", list(CASES))
def test_modes_are_allowed_for_their_block(work, case):
    _require_gpu()
    _, facts = _pair(work, case)[False]
    cmds, words = facts["commands"], facts["intra4_modes"]
    assert words.dtype == np.uint64 and words.shape == cmds.shape
    i4 = (cmds & 0xffffc000) == 0x80004000
    # bit 14 of an intra word (high half 0x8000, bit 15 clear; an inter word is a vector)
    intra_word = (cmds & 0xffff0000) == 0x80000000
    assert np.array_equal(i4, intra_word & ((cmds >> 14) & 1 == 1))
    assert np.array_equal(words != NONE, i4)
    assert ((cmds[i4] & 3) == 0).all()
    assert int(i4.sum()) == facts["intra4x4_mbs"]
    seen, col0 = set(), set()
    for f, my, mx in zip(*np.nonzero(i4)):
        w = int(words[f, my, mx])
        for k in range(16):
            m = (w >> (4 * k)) & 15
            assert m in _allowed(k, mx), f"frame {f} macroblock ({mx}, {my}) block {k}: mode {m}"
            seen.add(m)
            if BLK_XY[k][0] == 0:
                col0.add(m)
                assert BLK_XY[k][1] > 0 or mx > 0 or m == 2     # block 0 without a left macroblock: DC
    if case == "column_every":      # one macroblock wide: block column 0 never has samples to its left
        assert col0 <= {0, 2, 3, 7}
    if case == "content_every":
        assert any(m >= 3 for m in seen), "no directional mode was chosen"
    print(f"{case}: {int(i4.sum())} I_NxN macroblocks, modes {sorted(seen)}")


# ------------------------------------------------------- 4. off is the parent
OFF_CASES = {"small": ("s70", dict(height=96)), "small_intra": ("s70", dict(height=96, intra=True)),
             "small_every": ("s70", dict(height=96, intra=True, subpel=2, deblock=True))}


def _samples(path):
    m = oracle.read_mp4(path)
    return [bytes(m["data"][o:o + s]) for o, s in zip(m["offsets"], m["sizes"])]


@pytest.mark.parametrize("case", list(OFF_CASES))
def test_off_through_the_88_byte_struct_is_the_byte_oracle(work, tmp_path, case):
    _require_gpu()
    sname, tk = OFF_CASES[case]
    ref = _oracle_side(work, sname, tk)
    out = tmp_path / "off.mp4"
    facts = _transcode(work, sname, out, intra4x4=False, want_intra4_modes=True, **tk)
    assert _samples(out) == ref["samples"]
    assert facts["intra4x4_mbs"] == 0 and (facts["intra4_modes"] == NONE).all()
    for k in ("pcm_mbs", "inter_mbs", "skip_mbs", "intra_mbs"):
        assert facts[k] == ref[k], k


def test_off_on_off_on_in_one_session_and_again_in_a_fresh_one(work, tmp_path):
    _require_gpu()
    sname, kw, _ = CASES["small_every"]
    on = _pair(work, "small_every")[False][0].read_bytes()
    off_path = tmp_path / "off.mp4"
    _transcode(work, sname, off_path, **kw)                    # the call without the keyword
    off = off_path.read_bytes()
    assert off != on
    want = {False: off, True: on}
    with scene.VideoScorer(_source(work, sname)) as v:
        for i, flag in enumerate((False, True, False, True)):
            out = tmp_path / f"o{i}.mp4"
            v.transcode(out, intra4x4=flag, **kw)
            assert out.read_bytes() == want[flag], f"transcode {i} (intra4x4={flag})"
    again = tmp_path / "again.mp4"
    _transcode(work, sname, again, intra4x4=True, **kw)
    assert again.read_bytes() == on


# ---------------------------------------------------------- 5. size and quality
def _reference(work, sname, sh):
    """The encoder's input: the oracle's downscale of the oracle's decode, cropped to the display size."""
    frames, info = oracle.decode_full(_source(work, sname))
    W, H = info["width"], info["height"]
    sw = oracle.small_width(W, H, sh)
    ch = (sh + 15) & ~15
    ref = []
    for f in frames:
        d = oracle.downscale_nv12(f, W, H, sh)
        ref.append(np.concatenate([d[:sh, :sw], d[ch:ch + sh // 2, :sw]]))
    return np.stack(ref)


@pytest.mark.parametrize("sname,height", [("real", 240), ("content", 360)])
def test_smaller_at_qp28_and_the_idr_pictures_keep_their_quality(work, tmp_path, sname, height):
    """intra = 1 at qp 28, intra4x4 1 against 0 (the parent's output).  Measured on the MI355X: see the
    "Intra4x4" section of DESIGN.md §11."""
    _require_gpu()
    runs = {}
    for flag in (False, True):
        out = tmp_path / f"{sname}_{int(flag)}.mp4"
        facts = _transcode(work, sname, out, height=height, intra=True, intra4x4=flag)
        m = oracle.read_mp4(out)
        idr = np.array(_is_idr(out))
        runs[flag] = dict(size=out.stat().st_size, idr=idr, idr_bytes=int(np.array(m["sizes"])[idr].sum()),
                          frames=oracle.decode_full(out)[0], facts=facts)
    ref = _reference(work, sname, height)
    idr = runs[True]["idr"]
    assert np.array_equal(idr, runs[False]["idr"])
    p0, p1 = (_psnr(runs[f]["frames"][idr], ref[idr]) for f in (False, True))
    f1 = runs[True]["facts"]
    print(f"{sname}: {runs[False]['size']} -> {runs[True]['size']} bytes ({runs[True]['size'] / runs[False]['size']:.4f}); "
          f"IDR pictures {runs[False]['idr_bytes']} -> {runs[True]['idr_bytes']} bytes, PSNR {p0:.2f} -> {p1:.2f} dB; "
          f"I_NxN {f1['intra4x4_mbs']} of {f1['intra_mbs']} intra macroblocks")
    assert runs[True]["size"] < runs[False]["size"]
    assert p1 >= p0 - 0.5


# ----------------------------------------------------------------- 6. errors
def _raw_ext5(v, out, height, size, *, intra4x4=0, intra=1, qp=0, modes=None, cap=None, info_size=None):
    prm = _lib.TranscodeParams()
    prm.height = height
    prm.qp = qp
    prm.intra = intra
    ext = _lib.TranscodeExt5(_lib.TranscodeExt4(_lib.TranscodeExt3(_lib.TranscodeExt2(_lib.TranscodeExt(size, 0)))),
                             intra4x4, 0x55555555)
    if modes is not None:
        ext.i4_out = modes.ctypes.data_as(C.POINTER(C.c_uint64))
        ext.i4_cap = modes.size if cap is None else cap
    info = _lib.TranscodeInfo()
    xinfo = _lib.TranscodeExtInfo4(_lib.TranscodeExtInfo3(_lib.TranscodeExtInfo2(
        _lib.TranscodeExtInfo(C.sizeof(_lib.TranscodeExtInfo4) if info_size is None else info_size))))
    xinfo.intra4x4_mbs = xinfo.i4_words = -7
    rc = v._lib.vts_transcode_ex(v._ctx, str(out).encode(), C.byref(prm),
                                 C.cast(C.pointer(ext), C.POINTER(_lib.TranscodeExt)), C.byref(info),
                                 C.cast(C.pointer(xinfo), C.POINTER(_lib.TranscodeExtInfo)))
    return rc, info, xinfo


def test_argument_errors_and_struct_sizes(work, tmp_path):
    _require_gpu()
    src = _source(work, "s40")
    full = C.sizeof(_lib.TranscodeExt5)
    assert full == 88 and C.sizeof(_lib.TranscodeExtInfo4) == 64
    for fields in (dict(intra4x4=2), dict(intra4x4=-1), dict(intra4x4=1, intra=0), dict(intra4x4=1, qp=-1)):
        with scene.VideoScorer(src) as v:
            rc, _, _ = _raw_ext5(v, tmp_path / "bad.mp4", 96, full, **fields)
            assert rc == _lib.VTS_E_INVALID, fields
            assert "intra4x4" in _lib.last_error(), _lib.last_error()
    with scene.VideoScorer(src) as v:
        with pytest.raises(VtsegError) as ei:
            v.transcode(tmp_path / "bad.mp4", height=96, intra4x4=True)        # intra is off
        assert ei.value.code == _lib.VTS_E_INVALID
    nmb = 40 * 6 * 10
    with scene.VideoScorer(src) as v:                                          # a short i4_out: before any encoding
        modes = np.zeros(nmb, np.uint64)
        rc, _, xi = _raw_ext5(v, tmp_path / "short.mp4", 96, full, intra4x4=1, modes=modes, cap=nmb - 1)
        assert rc == _lib.VTS_E_CAPACITY and "i4_cap" in _lib.last_error()
        assert xi.i4_words == nmb and not (tmp_path / "short.mp4").exists()
    # 64 bytes (vts_transcode_ext4) with intra4x4 = 1 behind it: not read; 68: the flag, i4_out behind it not
    # read; 80: i4_out is read and its capacity is not (NULL here; a buffer has capacity 0); 88: everything
    files, words = {}, {}
    for size in (64, 68, 80, 88):
        out = tmp_path / f"s{size}.mp4"
        modes = None if size == 80 else np.zeros(nmb, np.uint64)
        with scene.VideoScorer(src) as v:
            rc, _, xi = _raw_ext5(v, out, 96, size, intra4x4=1, modes=modes)
            _lib.check(rc)
        files[size], words[size] = out.read_bytes(), modes
        assert xi.i4_words == nmb
        assert (xi.intra4x4_mbs > 0) == (size >= 68)
    assert files[68] == files[80] == files[88] != files[64]
    assert (words[64] == 0).all() and (words[68] == 0).all()                  # i4_out is not reached: untouched
    assert (words[88] != NONE).sum() > 0
    with scene.VideoScorer(src) as v:
        rc, _, _ = _raw_ext5(v, tmp_path / "c80.mp4", 96, 80, intra4x4=1, modes=np.zeros(nmb, np.uint64))
        assert rc == _lib.VTS_E_CAPACITY
    with scene.VideoScorer(src) as v:                                          # the keyword's default file
        v.transcode(tmp_path / "base.mp4", height=96, intra=True)
    assert files[64] == (tmp_path / "base.mp4").read_bytes()
    with scene.VideoScorer(src) as v:      # a 56-byte ext_info3 is not written past its end
        rc, _, xi = _raw_ext5(v, tmp_path / "i.mp4", 96, full, intra4x4=1, info_size=48)
        _lib.check(rc)
        assert xi.intra4x4_mbs == -7 and xi.i4_words == -7
