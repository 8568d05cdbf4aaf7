"""The two rate-aware decisions of the device encoder's motion search
(vts_transcode_ext3.mvcost / early_skip).

1. Closed loop, as for Intra16x16, the sub-sample refinement and the
   deblocking filter: the output is decoded by the CPU general oracle and by
   the device's general decoder; the two agree and the hash of the decode is
   the encoder's `recon_hash`.
2. Every vector decision restated: with `want_commands=True` the encoder
   returns its final word per macroblock; the test recomputes, in numpy and
   from the text of §11 (clamped 8.4.2.2.1 interpolation, the candidate order,
   the cost, the predictor guess, the probe), the vector of every macroblock
   the encoder coded with a vector.
3. Outcomes that follow from the rules on a crafted input, the new fields at
   zero against the existing entry point, and the argument errors.

Every transcode runs in a fresh VideoScorer."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
from test_transcode_bytes_gpu import SOURCES as BYTES_SOURCES
from test_transcode_subpel_gpu import REAL, SYNTH, _require_gpu
from vtseg import VtsegError, _lib, scene

pytestmark = pytest.mark.gpu

PCM = 0x80008000
MODES = {"mv": dict(mvcost=True), "es": dict(early_skip=True), "both": dict(mvcost=True, early_skip=True)}


SOURCES = dict(BYTES_SOURCES)      # s70, s40, tiny, column, content, real, crafted, noisy ...

ALL_ON = dict(intra=True, subpel=2, deblock=True)
# name -> (source, transcode kwargs)
LOOP = {}
for _m in MODES:
    for _sp in (0, 2):
        for _i in (False, True):
            LOOP[f"s70_{_m}_sp{_sp}_i{int(_i)}"] = ("s70", dict(height=96, subpel=_sp, intra=_i, **MODES[_m]))
LOOP.update({
    "r0_both_sp2": ("s40", dict(height=96, search_range=-1, subpel=2, **MODES["both"])),     # the refinement alone
    "r0_mv_all": ("s40", dict(height=96, search_range=-1, **ALL_ON, **MODES["mv"])),
    "r4_both_sp2": ("s40", dict(height=96, search_range=4, subpel=2, **MODES["both"])),
    "r4_mv_sp0_dbk": ("s40", dict(height=96, search_range=4, deblock=True, **MODES["mv"])),
    "r5_both_sp2": ("s40", dict(height=96, search_range=5, subpel=2, **MODES["both"])),       # the any-range instance
    "r5_both_sp0": ("s40", dict(height=96, search_range=5, **MODES["both"])),
    "r16_both_all": ("s40", dict(height=96, search_range=16, **ALL_ON, **MODES["both"])),
    # 70 frames in GOPs of 8, the last of 6: many j = 1 pictures, entry indices that differ between levels
    "keyint8_r16_both_sp2": ("s70", dict(height=96, keyint=8, search_range=16, subpel=2, **MODES["both"])),
    "keyint8_both_all": ("s70", dict(height=96, keyint=8, **ALL_ON, **MODES["both"])),
    "keyint8_mv_sp0": ("s70", dict(height=96, keyint=8, **MODES["mv"])),
    "tiny_both_all": ("tiny", dict(height=24, search_range=4, **ALL_ON, **MODES["both"])),
    "column_both_all": ("column", dict(height=48, search_range=4, **ALL_ON, **MODES["both"])),  # mx = 0 everywhere
    "real_both_all": ("real", dict(height=240, **ALL_ON, **MODES["both"])),
    "content_both_all": ("content", dict(**ALL_ON, **MODES["both"])),
    # display widths that are no multiple of 16: 72x128 coded 80x128, 88x72 coded 96x80
    "portrait_both_all": ("portrait", dict(height=128, **ALL_ON, **MODES["both"])),
    "qcif_both_all": ("qcif", dict(height=72, **ALL_ON, **MODES["both"])),
})


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("rate"), "src": {}, "dec": {}}


def _source(work, name):
    if name not in work["src"]:
        spec = SOURCES[name]
        if spec is None:
            work["src"][name] = REAL
        elif callable(spec):     # a lossless I_PCM stream that decodes to exactly these frames
            fr = spec()
            r = oracle.transcode(fr, 96, 64, np.zeros(len(fr), np.float32), out_height=64, max_mb_sad=-1)
            sps, pps = oracle.sps_pps(6, 4, 0, 0, 30.0)
            path = work["dir"] / f"{name}.mp4"
            n = len(fr)
            oracle.write_mp4(path, sps, pps, r["samples"], [i * 1000 for i in range(n)], [0] * n, 30000, 96, 64)
            work["src"][name] = path
        else:
            path = work["dir"] / f"{name}.mp4"
            scene.synth_write(path, **dict(SYNTH, **spec))
            work["src"][name] = path
    return work["src"][name]


def _transcode(work, sname, out, **kw):
    with scene.VideoScorer(_source(work, sname)) as v:
        return v.transcode(out, **kw)


def _is_idr(path):
    m = oracle.read_mp4(path)
    return [(m["data"][o + 4] & 31) == 5 for o in m["offsets"]]


def _device_frames(path, n, shape):
    with scene.VideoScorer(path, keep_frames=True) as d:
        d.score()
        general = d.general()
        got = np.stack([d.frame_nv12(i).reshape(shape) for i in range(n)])
    return got, general


# ------------------------------------------------------------- 1. closed loop
@pytest.mark.parametrize("case", list(LOOP))
def test_output_decodes_to_the_encoders_reconstruction(work, tmp_path, case):
    _require_gpu()
    sname, kw = LOOP[case]
    out = tmp_path / "out.mp4"
    facts = _transcode(work, sname, out, **kw)
    frames, _ = oracle.decode_full(out)
    n = facts["n_frames"]
    assert frames.shape[0] == n
    got, general = _device_frames(out, n, frames[0].shape)
    assert general
    bad = [i for i in range(n) if not np.array_equal(got[i], frames[i])]
    assert bad == [], f"device decode differs from the oracle at frames {bad[:8]}"
    assert facts["recon_hash"] != 0 and oracle.recon_hash(frames) == facts["recon_hash"]
    mbw, mbh = (facts["width"] + 15) // 16, (facts["height"] + 15) // 16
    assert facts["intra_mbs"] + facts["pcm_mbs"] + facts["inter_mbs"] + facts["skip_mbs"] == n * mbw * mbh
    print(f"{case}: {out.stat().st_size} bytes; facts {facts}")
    if kw.get("early_skip"):
        assert 0 <= facts["early_skip_mbs"] <= facts["skip_mbs"]
    else:
        assert facts["early_skip_mbs"] == 0


# ------------------------------------------- 2. every vector decision restated
CF = np.array([[1, 1, 1, 1], [2, 1, -1, -2], [1, -1, -1, 1], [1, -2, 2, -1]], np.int64)
MF = {0: (13107, 5243, 8066), 1: (11916, 4660, 7490), 2: (10082, 4194, 6554),
      3: (9362, 3647, 5825), 4: (8192, 3355, 5243), 5: (7282, 2893, 4559)}
PADM = 40    # edge replication around a plane: more than R + the filter's reach for every R <= 16


def _mf_grid(qp):
    a, b, c = MF[qp % 6]
    g = np.full((4, 4), c, np.int64)
    g[::2, ::2] = a
    g[1::2, 1::2] = b
    return g


def _blocks_nz(res, qp, skip_dc):
    """res [H, W] residual, H and W multiples of 4: per 4x4 block, the
    transform coefficients and whether a level (without DC if skip_dc) is
    non-zero: (|w| MF + f) >> qbits != 0, f = 2^qbits / 6."""
    H, W = res.shape
    x = res.reshape(H // 4, 4, W // 4, 4).transpose(0, 2, 1, 3).astype(np.int64)
    w = CF @ x @ CF.T
    qbits = 15 + qp // 6
    lv = (np.abs(w) * _mf_grid(qp) + (1 << qbits) // 6) >> qbits
    if skip_dc:
        lv[..., 0, 0] = 0
    return w, lv.reshape(H // 4, W // 4, 16).any(axis=2)


def _probe_hits(src, ref, x, y, cw, ch, qp):
    """Rule (a): the residual of the co-located prediction leaves no level."""
    assert qp < 30   # QPc = qp
    _, nzy = _blocks_nz(src[y:y + 16, x:x + 16].astype(int) - ref[y:y + 16, x:x + 16].astype(int), qp, False)
    if nzy.any():
        return False
    cy = ch + y // 2
    for pl in (0, 1):
        r = src[cy:cy + 8, x + pl:x + 16:2].astype(int) - ref[cy:cy + 8, x + pl:x + 16:2].astype(int)
        w, nz = _blocks_nz(r, qp, True)
        if nz.any():
            return False
        c = w[..., 0, 0].reshape(4)
        fd = np.array([c[0] + c[1] + c[2] + c[3], c[0] - c[1] + c[2] - c[3], c[0] + c[1] - c[2] - c[3],
                       c[0] - c[1] - c[2] + c[3]], np.int64)
        qbits = 15 + qp // 6
        if (((np.abs(fd) * MF[qp % 6][0] + 2 * ((1 << qbits) // 6)) >> (qbits + 1)) != 0).any():
            return False
    return True


def _tap6(a, b, c, d, e, f):
    return a - 5 * b + 20 * c + 20 * d - 5 * e + f


class _Luma:
    """8.4.2.2.1 over one reference luma plane with clamped coordinates
    (edge replication): integer samples G, half samples b (x + 1/2), h
    (y + 1/2), j (both), and the quarter samples as the averages of Table 8-12."""

    def __init__(self, plane):
        P = np.pad(plane.astype(np.int64), PADM, mode="edge")
        self.G = P
        b1 = np.zeros_like(P)
        b1[:, 2:-3] = _tap6(P[:, :-5], P[:, 1:-4], P[:, 2:-3], P[:, 3:-2], P[:, 4:-1], P[:, 5:])
        h1 = np.zeros_like(P)
        h1[2:-3, :] = _tap6(P[:-5], P[1:-4], P[2:-3], P[3:-2], P[4:-1], P[5:])
        j1 = np.zeros_like(P)
        j1[2:-3, :] = _tap6(b1[:-5], b1[1:-4], b1[2:-3], b1[3:-2], b1[4:-1], b1[5:])
        self.b = np.clip((b1 + 16) >> 5, 0, 255)
        self.h = np.clip((h1 + 16) >> 5, 0, 255)
        self.j = np.clip((j1 + 512) >> 10, 0, 255)

    def block(self, x, y, mvx, mvy):
        """The 16x16 prediction of the block at (x, y) with vector (mvx, mvy) in quarter samples."""
        fx, fy = mvx & 3, mvy & 3
        X, Y = x + (mvx >> 2) + PADM, y + (mvy >> 2) + PADM
        at = lambda A, dx=0, dy=0: A[Y + dy:Y + dy + 16, X + dx:X + dx + 16]
        avg = lambda p, q: (p + q + 1) >> 1
        G, H, M = at(self.G), at(self.G, 1, 0), at(self.G, 0, 1)
        b, h, j, m, s = at(self.b), at(self.h), at(self.j), at(self.h, 1, 0), at(self.b, 0, 1)
        return {(0, 0): lambda: G, (1, 0): lambda: avg(G, b), (2, 0): lambda: b, (3, 0): lambda: avg(b, H),
                (0, 1): lambda: avg(G, h), (0, 2): lambda: h, (0, 3): lambda: avg(h, M),
                (1, 1): lambda: avg(b, h), (2, 1): lambda: avg(b, j), (3, 1): lambda: avg(b, m),
                (1, 2): lambda: avg(h, j), (2, 2): lambda: j, (3, 2): lambda: avg(j, m),
                (1, 3): lambda: avg(h, s), (2, 3): lambda: avg(j, s), (3, 3): lambda: avg(m, s)}[(fx, fy)]()


def _s16(v):
    v &= 0xffff
    return v - 65536 if v >= 32768 else v


def _selen(k):
    code = 2 * abs(k) - (1 if k > 0 else 0)
    return 2 * (code + 1).bit_length() - 1


def _lambda16(qp):
    return int(16 * np.sqrt(0.85 * 2 ** ((qp - 12) / 3)) + 0.5)


def _expected_vector(luma, srcblk, x, y, R, subpel, lam, pred):
    """Rule (b): integer pass over (2R + 1)^2 candidates, index 0 the centre
    then raster order, then the refinement steps (8 neighbours at half, then
    quarter samples, index 0 the step's centre, its cost recomputed), all by
    (16 SAD + lam bits(v - pred), index)."""
    def key(vx, vy, idx):
        sad = int(np.abs(luma.block(x, y, vx, vy) - srcblk).sum())
        return (16 * sad + lam * (_selen(vx - pred[0]) + _selen(vy - pred[1])), idx)
    best, idx = (key(0, 0, 0), (0, 0)), 0
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dx == 0 and dy == 0:
                continue
            idx += 1
            best = min(best, (key(4 * dx, 4 * dy, idx), (4 * dx, 4 * dy)))
    v = best[1]
    for step in ((2, 1) if subpel == 2 else (2,) if subpel == 1 else ()):
        cand = [(key(v[0], v[1], 0), v)]
        k = 0
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                if ox == 0 and oy == 0:
                    continue
                k += 1
                w = (v[0] + step * ox, v[1] + step * oy)
                cand.append((key(w[0], w[1], k), w))
        v = min(cand)[1]
    return v


def _decode_coded(path, mbw, mbh):
    """The oracle's decode over the whole coded macroblock grid: the stream's
    own slices under an SPS of the same grid without cropping."""
    m = oracle.read_mp4(path)
    L = oracle.lib()
    L.fo_decode.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, C.c_int, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p]
    sps, _ = oracle.sps_pps(mbw, mbh, 0, 0, 30.0)
    pps = m["pps"][0]
    n = len(m["sizes"])
    out = np.zeros((n, mbh * 24, mbw * 16), np.uint8)
    offs, sizes = np.asarray(m["offsets"], np.int64), np.asarray(m["sizes"], np.int64)
    data = np.frombuffer(m["data"], np.uint8)
    bad, err = C.c_int64(-1), C.create_string_buffer(256)
    rc = L.fo_decode(sps, len(sps), pps, len(pps), m["nal_length_size"], data.ctypes.data, offs.ctypes.data,
                     sizes.ctypes.data, n, 0, out.ctypes.data, C.byref(bad), err)
    assert rc == 0, (rc, bad.value, err.value)
    return out


def _coded_source(work, sname, out_height):
    key = (sname, out_height)
    if key not in work["dec"]:
        frames, info = oracle.decode_full(_source(work, sname))
        W, H = info["width"], info["height"]
        work["dec"][key] = np.stack([oracle.downscale_nv12(f, W, H, out_height) for f in frames])
    return work["dec"][key]


RESTATED = {
    "s40_both_sp0": ("s40", dict(height=96, search_range=4, keyint=7, **MODES["both"]), 12),
    "s40_both_sp2": ("s40", dict(height=96, search_range=4, subpel=2, keyint=7, **MODES["both"]), 12),
    "s40_mv_sp2": ("s40", dict(height=96, search_range=4, subpel=2, **MODES["mv"]), 8),
    "s40_es_sp2": ("s40", dict(height=96, search_range=4, subpel=2, **MODES["es"]), 8),
    "s40_off_sp2": ("s40", dict(height=96, search_range=4, subpel=2), 6),          # the words of the parent's decisions
    "tiny_both_sp2": ("tiny", dict(height=24, search_range=4, subpel=2, keyint=9, **MODES["both"]), 14),
    "s40_both_all": ("s40", dict(height=96, search_range=4, keyint=7, **ALL_ON, **MODES["both"]), 10),
    "s40_lambda_sp2": ("s40", dict(height=96, search_range=4, subpel=2, mvcost=True, mv_lambda16=400), 6),
}


@pytest.mark.parametrize("case", list(RESTATED))
def test_every_vector_decision_restated(work, tmp_path, case):
    _require_gpu()
    sname, kw, nf = RESTATED[case]
    out = tmp_path / "out.mp4"
    facts = _transcode(work, sname, out, want_commands=True, **kw)
    cmds = facts["commands"]
    n, sh = facts["n_frames"], kw["height"]
    mbw, mbh = (facts["width"] + 15) // 16, (sh + 15) // 16
    assert cmds.shape == (n, mbh, mbw) and cmds.dtype == np.uint32
    cw, ch = 16 * mbw, 16 * mbh
    src = _coded_source(work, sname, sh)
    assert src.shape == (n, ch * 3 // 2, cw)
    dec = _decode_coded(out, mbw, mbh)
    disp, _ = oracle.decode_full(out)
    assert np.array_equal(dec[:, :sh, :facts["width"]], disp[:, :sh])        # the same pictures, uncropped
    idr = _is_idr(out)
    intra, subpel, qp = kw.get("intra", False), kw.get("subpel", 0), 28
    R = max(kw["search_range"], 0)
    lam = (kw.get("mv_lambda16") or _lambda16(qp)) if kw.get("mvcost") else 0
    if not intra:
        assert (cmds[np.array(idr)] == PCM).all()       # words the encoder never wrote are reported as I_PCM
    checked = left_out = hits = p_mbs = 0
    wrong = []
    j = 0
    for t in range(n):
        j = 0 if idr[t] else j + 1
        if j == 0:
            continue
        p_mbs += mbw * mbh
        if t >= nf and not kw.get("early_skip"):
            continue
        ref = src[t - 1] if (j == 1 and not intra) else dec[t - 1]
        luma = _Luma(ref[:ch]) if t < nf else None
        for my in range(mbh):
            for mx in range(mbw):
                x, y = 16 * mx, 16 * my
                word = int(cmds[t, my, mx])
                hit = bool(kw.get("early_skip")) and _probe_hits(src[t], ref, x, y, cw, ch, qp)
                hits += hit
                if t >= nf:
                    continue
                if word == PCM or (word & 0xffff8000) == 0x80000000:
                    left_out += 1
                    continue
                checked += 1
                if hit:
                    want = (0, 0)
                else:
                    pred = (0, 0)
                    if kw.get("mvcost") and mx > 0 and j > 1:
                        c = int(cmds[t - 1, my, mx - 1])
                        if c != PCM and (c & 0xffff8000) != 0x80000000:
                            pred = (_s16(c), _s16(c >> 16))
                    want = _expected_vector(luma, src[t][y:y + 16, x:x + 16].astype(np.int64), x, y, R, subpel,
                                            lam, pred)
                got = (_s16(word), _s16(word >> 16))
                if got != want:
                    wrong.append((t, my, mx, got, want))
    print(f"{case}: {checked} vectors restated, {left_out} intra macroblocks left out, probe hits {hits}, "
          f"early_skip_mbs {facts['early_skip_mbs']}, skip_mbs {facts['skip_mbs']}, {out.stat().st_size} bytes")
    assert wrong == [], f"{len(wrong)} of {checked} vectors differ (t, my, mx, got, want): {wrong[:6]}"
    assert checked > 0 and left_out <= 0.10 * (checked + left_out)
    assert facts["early_skip_mbs"] == hits
    if kw.get("early_skip"):
        assert hits > 0


# ------------------------------------------------------ 3. derivable outcomes
def test_noise_inside_the_dead_zone_is_all_p_skip(work, tmp_path):
    """A textured picture plus noise in {-1, 0, +1}: against the first
    picture every residual sample is within +-2, far inside the quantiser's
    dead zone at qp 28 (a 4x4 DC needs |sum| >= 54), so the probe decides
    every P macroblock, whose reconstruction stays the first picture.  A
    picture of skip runs only is the shortest the syntax allows: the output is
    strictly smaller than with the quarter-sample search alone, which gives up
    some of those skips for fractional vectors."""
    _require_gpu()
    kw = dict(height=64, subpel=2)
    on = _transcode(work, "noisy", tmp_path / "on.mp4", early_skip=True, **kw)
    off = _transcode(work, "noisy", tmp_path / "off.mp4", **kw)
    p_mbs = (on["n_frames"] - on["n_idr"]) * 6 * 4
    assert on["n_idr"] == 1 and p_mbs == 7 * 24
    print(f"P macroblocks {p_mbs}; early_skip: skip {on['skip_mbs']}, early {on['early_skip_mbs']}, "
          f"{on['bytes_written']} bytes; off: skip {off['skip_mbs']}, {off['bytes_written']} bytes")
    assert off["skip_mbs"] < p_mbs                       # the precondition
    assert on["skip_mbs"] == p_mbs and on["early_skip_mbs"] == p_mbs
    assert on["bytes_written"] < off["bytes_written"]
    frames, _ = oracle.decode_full(tmp_path / "on.mp4")
    assert oracle.recon_hash(frames) == on["recon_hash"]
    assert all(np.array_equal(f, frames[0]) for f in frames)


def _raw_ext3(v, out, height, size, *, mvcost=0, lam=0, early_skip=0, qp=0, cmd=None, cap=0, info_size=None):
    prm = _lib.TranscodeParams()
    prm.height = height
    prm.qp = qp
    ext = _lib.TranscodeExt3(_lib.TranscodeExt2(_lib.TranscodeExt(size, 0)), mvcost, lam, early_skip)
    if cmd is not None:
        ext.cmd_out = cmd.ctypes.data_as(C.POINTER(C.c_uint32))
    ext.cmd_cap = cap
    xinfo = _lib.TranscodeExtInfo3(_lib.TranscodeExtInfo2(_lib.TranscodeExtInfo(
        C.sizeof(_lib.TranscodeExtInfo3) if info_size is None else info_size)))
    xinfo.early_skip_mbs = xinfo.cmd_words = -1
    info = _lib.TranscodeInfo()
    rc = v._lib.vts_transcode_ex(v._ctx, str(out).encode(), C.byref(prm),
                                 C.cast(C.pointer(ext), C.POINTER(_lib.TranscodeExt)), C.byref(info),
                                 C.cast(C.pointer(xinfo), C.POINTER(_lib.TranscodeExtInfo)))
    return rc, info, xinfo


def test_new_fields_at_zero_are_the_existing_entry_point(work, tmp_path):
    _require_gpu()
    src = _source(work, "s70")
    base = tmp_path / "base.mp4"
    with scene.VideoScorer(src) as v:      # the existing entry point
        prm = _lib.TranscodeParams()
        prm.height = 96
        info = _lib.TranscodeInfo()
        _lib.check(v._lib.vts_transcode(v._ctx, str(base).encode(), C.byref(prm), C.byref(info)))
        assert info.recon_hash == 0
    want = base.read_bytes()
    full = C.sizeof(_lib.TranscodeExt3)
    # every new field 0; an ext of 24 bytes with non-zero bytes behind it, which must not be read
    for i, (size, fields) in enumerate(((full, {}), (24, dict(mvcost=1, lam=77, early_skip=1)))):
        out = tmp_path / f"raw{i}.mp4"
        with scene.VideoScorer(src) as v:
            rc, info, xinfo = _raw_ext3(v, out, 96, size, **fields)
            _lib.check(rc)
            assert info.recon_hash == 0 and xinfo.early_skip_mbs == 0 and xinfo.cmd_words == 70 * 60
        assert out.read_bytes() == want
    # an info struct of 32 bytes: the new facts are not written
    with scene.VideoScorer(src) as v:
        rc, _, xinfo = _raw_ext3(v, tmp_path / "short.mp4", 96, full, info_size=32)
        _lib.check(rc)
        assert xinfo.early_skip_mbs == -1 and xinfo.cmd_words == -1
    assert (tmp_path / "short.mp4").read_bytes() == want
    # no keyword; want_commands alone
    plain = _transcode(work, "s70", tmp_path / "plain.mp4", height=96)
    assert (tmp_path / "plain.mp4").read_bytes() == want
    assert "early_skip_mbs" not in plain and "commands" not in plain
    wc = _transcode(work, "s70", tmp_path / "wc.mp4", height=96, want_commands=True)
    assert (tmp_path / "wc.mp4").read_bytes() == want
    assert {k: wc[k] for k in plain if not k.endswith("_ms")} == {k: plain[k] for k in plain if not k.endswith("_ms")}
    cmds = wc["commands"]
    assert cmds.shape == (70, 6, 10) and (cmds[0] == PCM).all() and wc["early_skip_mbs"] == 0
    assert int((cmds == PCM).sum()) == wc["pcm_mbs"]
    assert int((cmds != PCM).sum()) == wc["inter_mbs"] + wc["skip_mbs"]


def test_argument_errors(work, tmp_path):
    _require_gpu()
    src = _source(work, "s40")
    full = C.sizeof(_lib.TranscodeExt3)
    bad = [(dict(mvcost=2), "mvcost"), (dict(mvcost=-1), "mvcost"),
           (dict(early_skip=2), "early_skip"), (dict(early_skip=-1), "early_skip"),
           (dict(mvcost=1, lam=4097), "mv_lambda16"), (dict(mvcost=1, lam=-1), "mv_lambda16"),
           (dict(lam=5), "mv_lambda16"),
           (dict(mvcost=1, qp=-1), "mvcost"), (dict(early_skip=1, qp=-1), "early_skip")]
    for fields, name in bad:
        with scene.VideoScorer(src) as v:
            rc, _, _ = _raw_ext3(v, tmp_path / "bad.mp4", 96, full, **fields)
            assert rc == _lib.VTS_E_INVALID, fields
            assert name in _lib.last_error(), (_lib.last_error(), name)
    words = 40 * 60
    buf = np.zeros(words, np.uint32)
    with scene.VideoScorer(src) as v:
        rc, _, xinfo = _raw_ext3(v, tmp_path / "bad.mp4", 96, full, cmd=buf, cap=words - 1)
        assert rc == _lib.VTS_E_CAPACITY and "cmd_cap" in _lib.last_error()
        assert xinfo.cmd_words == words and not buf.any()
    with scene.VideoScorer(src) as v:
        rc, _, xinfo = _raw_ext3(v, tmp_path / "ok.mp4", 96, full, cmd=buf, cap=words)
        _lib.check(rc)
        assert xinfo.cmd_words == words and (buf[:60] == PCM).all()
    for kw in (dict(mvcost=True, qp=0), dict(early_skip=True, qp=0), dict(mv_lambda16=9), dict(mvcost=True, mv_lambda16=5000)):
        with scene.VideoScorer(src) as v:
            with pytest.raises(VtsegError) as ei:
                v.transcode(tmp_path / "bad.mp4", height=96, **kw)
            assert ei.value.code == _lib.VTS_E_INVALID
