"""Inter partitions in the device encoder (vts_transcode_ext6.partitions,
DESIGN.md §11 "Partitions"): P_L0_L0_16x8, P_L0_L0_8x16 and P_8x8 of four
P_L0_8x8 beside P_L0_16x16 and P_Skip.

1. Closed loop: the output is decoded by the CPU general oracle and by the
   device's general decoder; the two agree, the hash of the decode is the
   encoder's `recon_hash`, and the counts add up.
2. Words and vectors: a partitioned word stands exactly where the four
   quadrant vectors need one, the shape is the coarsest they allow, and the
   counters are the word counts.
3. CABAC is still lossless.
4. Off is the parent: `partitions = 0` through the 112-byte struct gives the
   byte oracle's samples.
5. The argument errors and the struct sizes.
6. On a source whose quadrants move apart the output is smaller; on `real` and
   `content` the sizes and the P pictures' PSNR measured on the MI355X.

Every transcode runs in a fresh VideoScorer unless the test says otherwise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
from test_transcode_bytes_gpu import _oracle_side
from test_transcode_intra4_gpu import _reference, _samples
from test_transcode_rate_gpu import SOURCES as RATE_SOURCES, _device_frames, _is_idr
from test_transcode_subpel_gpu import REAL, SYNTH, _psnr, _require_gpu
from vtseg import VtsegError, _lib, scene

pytestmark = pytest.mark.gpu

PCM = 0x80008000
NOMV = 0x80008000


def quads_frames(F=8, W=96, H=64, seed=21):
    """Display-size NV12 frames (samples >= 1): one texture, and in every macroblock the four 8x8 quadrants
    show it displaced by their own motion, f times an offset in half samples: by macroblock (mx + my) % 4 all
    four together, in pairs by rows, in pairs by columns, all four apart.  One vector cannot predict a
    macroblock whose quadrants move apart; a vector per quadrant predicts all but the strip its motion
    uncovers."""
    rng = np.random.default_rng(seed)
    pad = 64
    # a texture at twice the resolution, smooth at that scale: a half-sample position of the picture is a sample
    coarse = rng.integers(20, 236, ((H + 2 * pad) // 4 + 2, (W + 2 * pad) // 4 + 2)).astype(np.float64)
    t2 = np.kron(coarse, np.ones((8, 8)))
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    for _ in range(2):
        t2 = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 0, t2)
        t2 = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, t2)
    moves = [(2, 0), (-3, 1), (0, -2), (1, 3), (4, -1), (-2, -2)]     # half samples a frame: integer and half
    fr = np.full((F, H * 3 // 2, W), 128, np.uint8)
    for f in range(F):
        for my in range(H // 16):
            for mx in range(W // 16):
                kind = (mx + my) % 4
                for q in range(4):
                    g = {0: 0, 1: q >> 1, 2: q & 1, 3: q}[kind]
                    dx, dy = moves[(g + mx + 2 * my) % len(moves)]
                    y0, x0 = my * 16 + 8 * (q >> 1), mx * 16 + 8 * (q & 1)
                    ys = 2 * (pad + y0 + np.arange(8)) - f * dy
                    xs = 2 * (pad + x0 + np.arange(8)) - f * dx
                    fr[f, y0:y0 + 8, x0:x0 + 8] = np.clip(np.rint(t2[np.ix_(ys, xs)]), 1, 255)
    return fr


SOURCES = dict(RATE_SOURCES, quads=quads_frames)
BASE = dict(mvcost=True)
EVERY = dict(intra=True, subpel=2, deblock=True, mvcost=True, early_skip=True)
# name -> (source, transcode kwargs besides partitions / cabac)
CASES = {
    "quads_sp0": ("quads", dict(height=64, **BASE)),
    "quads_sp2": ("quads", dict(height=64, subpel=2, **BASE)),
    "quads_sp0_intra_dbk": ("quads", dict(height=64, intra=True, deblock=True, **BASE)),
    "quads_sp2_every_i4": ("quads", dict(height=64, intra4x4=True, **EVERY)),
    "keyint8_r16": ("s70", dict(height=96, keyint=8, search_range=16, **EVERY)),
    "r4_sp2": ("s40", dict(height=96, search_range=4, subpel=2, **BASE)),
    "r5_sp2": ("s40", dict(height=96, search_range=5, subpel=2, early_skip=True, **BASE)),     # the any-range instance
    "r5_sp0": ("s40", dict(height=96, search_range=5, **BASE)),
    "r0_sp2": ("s40", dict(height=96, search_range=-1, subpel=2, **BASE)),                     # the refinement alone
    "tiny": ("tiny", dict(height=24, search_range=4, **EVERY)),                                # 2 x 2 macroblocks
    "column": ("column", dict(height=48, search_range=4, **EVERY)),                            # never a left neighbour
    "portrait": ("portrait", dict(height=128, **EVERY)),                                       # 72 wide, coded 80
    "pan": ("pan", dict(height=96, **EVERY)),                                                  # vectors over every edge
    "qp1": ("s40", dict(height=96, qp=1, **EVERY)),
    "qp51": ("s40", dict(height=96, qp=51, deblock_offsets=(6, 6), **EVERY)),
    "real": ("real", dict(height=240, **EVERY)),
    "content": ("content", dict(**EVERY)),
}
SAME = ("width", "height", "n_frames", "n_idr", "pcm_mbs", "inter_mbs", "skip_mbs", "intra_mbs", "subpel_mbs", "qpel_mbs",
        "deblock_mbs", "early_skip_mbs", "p16x8_mbs", "p8x16_mbs", "p8x8_mbs", "recon_hash")


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("part"), "src": {}, "dec": {}, "ref": {}, "run": {}, "frames": {}}


def _source(work, name):
    if name not in work["src"]:
        spec = SOURCES[name]
        path = work["dir"] / f"{name}.mp4"
        if spec is None:
            path = REAL
        elif callable(spec):     # a lossless I_PCM stream that decodes to exactly these frames
            fr = spec()
            r = oracle.transcode(fr, 96, 64, np.zeros(len(fr), np.float32), out_height=64, max_mb_sad=-1)
            sps, pps = oracle.sps_pps(6, 4, 0, 0, 30.0)
            n = len(fr)
            oracle.write_mp4(path, sps, pps, r["samples"], [i * 1000 for i in range(n)], [0] * n, 30000, 96, 64)
        else:
            scene.synth_write(path, **dict(SYNTH, **spec))
        work["src"][name] = path
    return work["src"][name]


def _transcode(work, sname, out, **kw):
    with scene.VideoScorer(_source(work, sname)) as v:
        return v.transcode(out, **kw)


def _pair(work, case):
    """The case transcoded with partitions on, cabac off and on (a fresh session each), once per module."""
    if case not in work["run"]:
        sname, kw = CASES[case]
        r = {}
        for cabac in (False, True):
            out = work["dir"] / f"{case}_{int(cabac)}.mp4"
            r[cabac] = (out, _transcode(work, sname, out, partitions=True, cabac=cabac, want_commands=True,
                                        want_vectors=True, **kw))
        work["run"][case] = r
    return work["run"][case]


def _decoded(work, path):
    if path not in work["frames"]:
        work["frames"][path] = oracle.decode_full(path)[0]
    return work["frames"][path]


def _part_mask(cmds):
    hi = cmds >> 16
    return ((cmds & 0xffff) == 0x8000) & (hi >= 1) & (hi <= 3)


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
    parts = facts["p16x8_mbs"] + facts["p8x16_mbs"] + facts["p8x8_mbs"]
    assert 0 <= parts <= facts["inter_mbs"]
    print(f"{case} cabac={cabac}: {out.stat().st_size} bytes; 16x8 {facts['p16x8_mbs']} 8x16 {facts['p8x16_mbs']} 8x8 "
          f"{facts['p8x8_mbs']} of inter {facts['inter_mbs']}, skip {facts['skip_mbs']} intra {facts['intra_mbs']} "
          f"pcm {facts['pcm_mbs']}, half {facts['subpel_mbs'] - facts['qpel_mbs']} quarter {facts['qpel_mbs']}")


@pytest.mark.parametrize("case", ["quads_sp0", "quads_sp2", "quads_sp2_every_i4"])
def test_quadrants_that_move_apart_get_their_own_vectors(work, case):
    _require_gpu()
    _, facts = _pair(work, case)[False]
    assert facts["p16x8_mbs"] > 0 and facts["p8x16_mbs"] > 0 and facts["p8x8_mbs"] > 0
    v, cmds = facts["vectors"], facts["commands"]
    p = ~np.array(_is_idr(_pair(work, case)[False][0]))
    # macroblocks (mx + my) % 4 == 3 move all four quadrants apart: most of them carry four different vectors
    my, mx = np.mgrid[0:v.shape[1], 0:v.shape[2]]
    apart = (mx + my) % 4 == 3
    late = v[2:][:, apart]
    four = [len({int(w) for w in m}) == 4 for m in late.reshape(-1, 4) if (m != NOMV).all()]
    assert sum(four) > len(four) // 2, f"{sum(four)} of {len(four)}"
    assert (cmds[p] != PCM).any()


# ------------------------------------------------------ 2. words and vectors
@pytest.mark.parametrize("case", list(CASES))
def test_words_vectors_and_counts_agree(work, case):
    _require_gpu()
    out, facts = _pair(work, case)[False]
    cmds, v = facts["commands"], facts["vectors"]
    assert v.dtype == np.uint32 and v.shape == cmds.shape + (4,)
    part = _part_mask(cmds)
    intra = (cmds >> 16) == 0x8000                       # I_PCM and the intra words
    assert not (part & intra).any()
    assert (v[intra] == NOMV).all() and not (v[~intra] == NOMV).any()
    # the canonical form: the coarsest shape the four vectors allow
    rows = (v[..., 0] == v[..., 1]) & (v[..., 2] == v[..., 3])
    cols = (v[..., 0] == v[..., 2]) & (v[..., 1] == v[..., 3])
    shape = np.where(rows & cols, 0, np.where(rows, 1, np.where(cols, 2, 3)))
    inter = ~intra
    assert np.array_equal(part[inter], shape[inter] > 0)
    assert np.array_equal((cmds >> 16)[part], shape[part])
    one = inter & ~part                                  # 16x16 and P_Skip: the command word four times
    assert (v[one] == cmds[one][:, None]).all()
    for s, key in ((1, "p16x8_mbs"), (2, "p8x16_mbs"), (3, "p8x8_mbs")):
        assert int((part & (shape == s)).sum()) == facts[key], key
    assert int(inter.sum()) == facts["inter_mbs"] + facts["skip_mbs"]
    # sub-sample counts: a macroblock once, quarter if any component is odd, else half if any is fractional
    comp = np.stack([v & 0xffff, v >> 16], -1)[inter].reshape(-1, 8)
    odd, frac = (comp & 1).any(axis=1), (comp & 3).any(axis=1)
    if CASES[case][1].get("subpel"):
        assert facts["qpel_mbs"] == int(odd.sum()) and facts["subpel_mbs"] == int(frac.sum())
    else:
        assert not frac.any() and facts["subpel_mbs"] == 0


# ------------------------------------------------ 3. CABAC is still lossless
@pytest.mark.parametrize("case", list(CASES))
def test_cabac_codes_what_cavlc_codes(work, case):
    _require_gpu()
    (off_path, off), (on_path, on) = _pair(work, case)[False], _pair(work, case)[True]
    for k in SAME:
        assert on[k] == off[k], f"{k}: {on[k]} with cabac, {off[k]} without"
    assert np.array_equal(on["commands"], off["commands"])
    assert np.array_equal(on["vectors"], off["vectors"])
    assert np.array_equal(_decoded(work, on_path), _decoded(work, off_path))


# ------------------------------------------------------- 4. off is the parent
OFF_CASES = {"small": ("s70", dict(height=96)), "small_intra": ("s70", dict(height=96, intra=True)),
             "small_every": ("s70", dict(height=96, intra=True, subpel=2, deblock=True))}


@pytest.mark.parametrize("case", list(OFF_CASES))
def test_off_through_the_112_byte_struct_is_the_byte_oracle(work, tmp_path, case):
    _require_gpu()
    sname, tk = OFF_CASES[case]
    ref = _oracle_side(work, sname, tk)
    out = tmp_path / "off.mp4"
    facts = _transcode(work, sname, out, partitions=False, want_vectors=True, want_commands=True, **tk)
    assert _samples(out) == ref["samples"]
    assert facts["p16x8_mbs"] == facts["p8x16_mbs"] == facts["p8x8_mbs"] == 0
    for k in ("pcm_mbs", "inter_mbs", "skip_mbs", "intra_mbs"):
        assert facts[k] == ref[k], k
    # the vectors without partitions: the command word four times, 0x80008000 for intra and I_PCM
    cmds, v = facts["commands"], facts["vectors"]
    intra = (cmds >> 16) == 0x8000
    assert (v[intra] == NOMV).all() and (v[~intra] == cmds[~intra][:, None]).all()


def test_off_on_off_on_in_one_session_and_again_in_a_fresh_one(work, tmp_path):
    _require_gpu()
    sname, kw = CASES["keyint8_r16"]
    on = _pair(work, "keyint8_r16")[False][0].read_bytes()
    off_path = tmp_path / "off.mp4"
    _transcode(work, sname, off_path, **kw)                    # the call without the keyword
    off = off_path.read_bytes()
    assert off != on
    want = {False: off, True: on}
    with scene.VideoScorer(_source(work, sname)) as v:
        for i, flag in enumerate((False, True, False, True)):
            out = tmp_path / f"o{i}.mp4"
            v.transcode(out, partitions=flag, **kw)
            assert out.read_bytes() == want[flag], f"transcode {i} (partitions={flag})"
    again = tmp_path / "again.mp4"
    _transcode(work, sname, again, partitions=True, **kw)
    assert again.read_bytes() == on


# ----------------------------------------------------------------- 5. errors
def _raw_ext6(v, out, height, size, *, partitions=0, mvcost=1, qp=0, max_mb_sad=0, vectors=None, cap=None, info_size=None):
    prm = _lib.TranscodeParams()
    prm.height = height
    prm.qp = qp
    prm.max_mb_sad = max_mb_sad
    ext = _lib.TranscodeExt6(_lib.TranscodeExt5(_lib.TranscodeExt4(_lib.TranscodeExt3(
        _lib.TranscodeExt2(_lib.TranscodeExt(size, 0)), mvcost))), partitions, 0x55555555)
    if vectors is not None:
        ext.mv_out = vectors.ctypes.data_as(C.POINTER(C.c_uint32))
        ext.mv_cap = vectors.size if cap is None else cap
    info = _lib.TranscodeInfo()
    xinfo = _lib.TranscodeExtInfo5(_lib.TranscodeExtInfo4(_lib.TranscodeExtInfo3(_lib.TranscodeExtInfo2(
        _lib.TranscodeExtInfo(C.sizeof(_lib.TranscodeExtInfo5) if info_size is None else info_size)))))
    xinfo.p16x8_mbs = xinfo.p8x16_mbs = xinfo.p8x8_mbs = xinfo.mv_words = -7
    rc = v._lib.vts_transcode_ex(v._ctx, str(out).encode(), C.byref(prm),
                                 C.cast(C.pointer(ext), C.POINTER(_lib.TranscodeExt)), C.byref(info),
                                 C.cast(C.pointer(xinfo), C.POINTER(_lib.TranscodeExtInfo)))
    return rc, info, xinfo


def test_argument_errors_and_struct_sizes(work, tmp_path):
    _require_gpu()
    src = _source(work, "quads")
    full = C.sizeof(_lib.TranscodeExt6)
    assert full == 112 and C.sizeof(_lib.TranscodeExtInfo5) == 96
    for fields, named in ((dict(partitions=2), "partitions"), (dict(partitions=-1), "partitions"),
                          (dict(partitions=1, qp=-1), "partitions"), (dict(partitions=1, max_mb_sad=-1), "max_mb_sad"),
                          (dict(partitions=1, mvcost=0), "mvcost")):
        with scene.VideoScorer(src) as v:
            rc, _, _ = _raw_ext6(v, tmp_path / "bad.mp4", 64, full, **fields)
            assert rc == _lib.VTS_E_INVALID, fields
            assert "partitions" in _lib.last_error() and named in _lib.last_error(), _lib.last_error()
            assert not (tmp_path / "bad.mp4").exists()
    with scene.VideoScorer(src) as v:
        with pytest.raises(VtsegError) as ei:
            v.transcode(tmp_path / "bad.mp4", height=64, partitions=True)       # mvcost is off
        assert ei.value.code == _lib.VTS_E_INVALID
    nw = 8 * 4 * 6 * 4
    with scene.VideoScorer(src) as v:                                          # a short mv_out: before any encoding
        vec = np.zeros(nw, np.uint32)
        rc, _, xi = _raw_ext6(v, tmp_path / "short.mp4", 64, full, partitions=1, vectors=vec, cap=nw - 1)
        assert rc == _lib.VTS_E_CAPACITY and "mv_cap" in _lib.last_error()
        assert xi.mv_words == nw and not (tmp_path / "short.mp4").exists()
    # 88 bytes (vts_transcode_ext5) with partitions = 1 behind it: not read; 92: the flag, mv_out behind it not
    # read; 104: mv_out is read and its capacity is not (NULL here; a buffer has capacity 0); 112: everything
    files, words = {}, {}
    for size in (88, 92, 104, 112):
        out = tmp_path / f"s{size}.mp4"
        vec = None if size == 104 else np.zeros(nw, np.uint32)
        with scene.VideoScorer(src) as v:
            rc, _, xi = _raw_ext6(v, out, 64, size, partitions=1, vectors=vec)
            _lib.check(rc)
        files[size], words[size] = out.read_bytes(), vec
        assert xi.mv_words == nw
        assert (xi.p8x8_mbs > 0) == (size >= 92)
    assert files[92] == files[104] == files[112] != files[88]
    assert (words[88] == 0).all() and (words[92] == 0).all()                  # mv_out is not reached: untouched
    assert (words[112] == NOMV).any() and (words[112] != NOMV).any()
    with scene.VideoScorer(src) as v:
        rc, _, _ = _raw_ext6(v, tmp_path / "c104.mp4", 64, 104, partitions=1, vectors=np.zeros(nw, np.uint32))
        assert rc == _lib.VTS_E_CAPACITY
    with scene.VideoScorer(src) as v:                                          # the keyword's default file
        v.transcode(tmp_path / "base.mp4", height=64, mvcost=True)
    assert files[88] == (tmp_path / "base.mp4").read_bytes()
    with scene.VideoScorer(src) as v:      # a 64-byte ext_info4 is not written past its end
        rc, _, xi = _raw_ext6(v, tmp_path / "i.mp4", 64, full, partitions=1, info_size=64)
        _lib.check(rc)
        assert xi.p16x8_mbs == -7 and xi.p8x16_mbs == -7 and xi.p8x8_mbs == -7 and xi.mv_words == -7


# ---------------------------------------------------------- 6. size and quality
RATE = dict(intra=True, subpel=2, mvcost=True, early_skip=True)


def _on_off(work, tmp_path, sname, height):
    runs = {}
    for flag in (False, True):
        out = tmp_path / f"{sname}_{int(flag)}.mp4"
        facts = _transcode(work, sname, out, height=height, partitions=flag, **RATE)
        runs[flag] = dict(size=out.stat().st_size, idr=np.array(_is_idr(out)), frames=oracle.decode_full(out)[0], facts=facts)
    return runs


def test_smaller_where_one_vector_cannot_predict(work, tmp_path):
    _require_gpu()
    runs = _on_off(work, tmp_path, "quads", 64)
    f1 = runs[True]["facts"]
    print(f"quads: {runs[False]['size']} -> {runs[True]['size']} bytes; 16x8 {f1['p16x8_mbs']} 8x16 {f1['p8x16_mbs']} "
          f"8x8 {f1['p8x8_mbs']} of inter {f1['inter_mbs']}; intra {runs[False]['facts']['intra_mbs']} -> {f1['intra_mbs']}")
    assert runs[True]["size"] < runs[False]["size"]


# measured on the MI355X (DESIGN.md §11 "Partitions"): bytes off, bytes on, the P pictures' PSNR drop rounded up to 0.1 dB
MEASURED = {"real": (75775, 75403, 0.0), "content": (86104, 83899, 0.0)}


@pytest.mark.parametrize("sname,height", [("real", 240), ("content", 360)])
def test_sizes_and_p_picture_quality_as_measured(work, tmp_path, sname, height):
    """partitions 1 against 0 at intra, subpel 2, mvcost, early_skip, qp 28.  The output is deterministic, so the
    sizes are asserted to the byte; the P pictures lose no more than the measured drop."""
    _require_gpu()
    runs = _on_off(work, tmp_path, sname, height)
    ref = _reference(work, sname, height)
    p = ~runs[True]["idr"]
    assert np.array_equal(p, ~runs[False]["idr"])
    p0, p1 = (_psnr(runs[f]["frames"][p], ref[p]) for f in (False, True))
    f1 = runs[True]["facts"]
    print(f"{sname}: {runs[False]['size']} -> {runs[True]['size']} bytes ({runs[True]['size'] / runs[False]['size']:.4f}); "
          f"P pictures PSNR {p0:.3f} -> {p1:.3f} dB; 16x8 {f1['p16x8_mbs']} 8x16 {f1['p8x16_mbs']} 8x8 {f1['p8x8_mbs']} "
          f"of inter {f1['inter_mbs']}")
    off, on, drop = MEASURED[sname]
    assert (runs[False]["size"], runs[True]["size"]) == (off, on)
    assert p1 >= p0 - drop
