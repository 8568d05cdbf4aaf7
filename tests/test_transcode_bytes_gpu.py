"""Byte parity of the device encoder's opt-in paths with the CPU oracle
(DESIGN.md §11): Intra16x16 (`intra`), the half- / quarter-sample refinement
(`subpel`) and the in-loop deblocking filter (`deblock`).

The closed-loop tests of the three paths (test_transcode_intra_gpu.py,
test_transcode_subpel_gpu.py, test_transcode_deblock_gpu.py) prove that the
stream decodes to the encoder's own reconstruction.  They cannot see whether
the encoder decided what §11 says it decides: a refinement that misses a
candidate, a tie broken the other way, a prediction mode picked wrongly, a bit
count that differs from the bits written, a bS of 1 where 2 is due all still
decode.  Here every output byte, every macroblock count and the hash of the
reconstruction are compared with oracle/transcode_oracle.c, which restates the
rules of §11 in scalar C, one sample at a time, and whose own closed loop
tests/test_transcode_oracle.py checks without a GPU.

Per case, in a fresh VideoScorer: the oracle's decode of the source, the
oracle's scene scores, oracle.transcode(...), and the device's
transcode(...) with the same settings.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from test_transcode_oracle import crafted_frames, diagonal_frames, noisy_frames
from test_transcode_subpel_gpu import REAL, SOURCES as SUBPEL_SOURCES, SYNTH, _require_gpu
from vtseg import scene

pytestmark = pytest.mark.gpu

SOURCES = dict(SUBPEL_SOURCES)   # odd, s70, s40, s60, pan, crop, content, real
SOURCES.update({
    # 64x48 -> 32x24 (coded 32x32): every macroblock touches two picture edges
    "tiny": dict(width=64, height=48, n_frames=40, max_motion=8, coding="full"),
    # 48x144 -> 16x48: one macroblock a row, never a left neighbour
    "column": dict(width=48, height=144, n_frames=30, max_motion=6, coding="full"),
    # frames written as a lossless I_PCM stream (96x64): P pictures with every macroblock
    # kind; a constant picture, where every decision is a tie
    "crafted": crafted_frames,
    "flat": lambda: np.full((6, 96, 96), 128, np.uint8),
    # sources of tests/test_transcode_bytes_rate_intra4_gpu.py and test_transcode_rate_gpu.py: noise inside
    # the quantiser's dead zone (early P_Skip); edges at many angles, ramps, constants and noise (Intra_4x4)
    "noisy": noisy_frames,
    "diag": diagonal_frames,
    # display widths that are no multiple of 16 (crop_r != 0), what every portrait upload
    # gives: 144x256 -> 72x128 coded 80x128; 176x144 -> 88x72 coded 96x80 (both crops)
    "portrait": dict(width=144, height=256, n_frames=20),
    "qcif": dict(width=176, height=144, n_frames=20),
})
ALL_ON = dict(intra=True, subpel=2, deblock=True)
S70 = dict(height=96)

# name -> (source, transcode kwargs of both sides)
CASES = {}
for _i in (False, True):
    for _sp in (0, 2):
        for _d in (False, True):
            CASES[f"s70_i{int(_i)}_sp{_sp}_d{int(_d)}"] = ("s70", dict(S70, intra=_i, subpel=_sp, deblock=_d))
CASES.update({
    "s70_sp1": ("s70", dict(S70, subpel=1)),
    "s70_sp1_intra": ("s70", dict(S70, subpel=1, intra=True)),
    "halfpel_sp1": ("odd", dict(height=120, search_range=4, subpel=1)),          # odd pans at 2:1; <4, SP>
    "halfpel_all": ("odd", dict(height=120, search_range=4, **ALL_ON)),
    "r5_sp2": ("s40", dict(height=96, search_range=5, subpel=2)),                # the any-range instance
    "r5_all": ("s40", dict(height=96, search_range=5, **ALL_ON)),
    "r0_sp1": ("s40", dict(height=96, search_range=-1, subpel=1)),               # range 0: the refinement alone
    "r0_sp2": ("s40", dict(height=96, search_range=-1, subpel=2)),
    "r0_all": ("s40", dict(height=96, search_range=-1, **ALL_ON)),
    "keyint8_r16_sp2": ("s70", dict(height=96, keyint=8, search_range=16, subpel=2)),   # largest window
    "keyint8_r16_all": ("s70", dict(height=96, keyint=8, search_range=16, **ALL_ON)),   # many IDR pictures
    "bigpan_edges_sp2": ("pan", dict(height=96, subpel=2)),                      # vectors over all four edges
    "bigpan_edges_all": ("pan", dict(height=96, **ALL_ON)),
    "crop_sp2": ("crop", dict(subpel=2)),                                        # 480x360 inside 480x368
    "crop_all": ("crop", dict(**ALL_ON)),
    "no_residual_sp1": ("s60", dict(height=96, qp=0, subpel=1)),                 # the qp < 1 branch
    "no_residual_sp2": ("s60", dict(height=96, qp=0, subpel=2)),
    "allpcm_intra": ("s40", dict(height=96, max_mb_sad=-1, intra=True, deblock=True)),  # Intra16x16 rows in P slices
    "content_all": ("content", dict(**ALL_ON)),
    "real_all": ("real", dict(height=240, **ALL_ON)),
    "tiny_all": ("tiny", dict(height=24, search_range=4, **ALL_ON)),
    "crafted_qp4_intra": ("crafted", dict(height=64, qp=4, intra=True)),
    "crafted_qp12_all": ("crafted", dict(height=64, qp=12, deblock_offsets=(6, 6), **ALL_ON)),
    "crafted_qp28_all": ("crafted", dict(height=64, **ALL_ON)),
    "flat_all": ("flat", dict(height=64, **ALL_ON)),                             # ties: the centre, the lower mode
    "flat_r16_sp2": ("flat", dict(height=64, search_range=16, subpel=2)),        # 1089 + 16 equal candidates
})
for _i in (False, True):
    _s = "_intra" if _i else ""
    CASES.update({
        f"hiqp{_s}": ("s70", dict(S70, qp=40, deblock=True, intra=_i)),                           # bS 4, the strong filter
        f"qp51{_s}": ("s40", dict(S70, qp=51, deblock=True, deblock_offsets=(6, 6), intra=_i)),   # index clipping at 51
        f"soft{_s}": ("s70", dict(S70, deblock=True, deblock_offsets=(-6, -6), intra=_i)),        # indexA exactly 16
        f"lowqp_on{_s}": ("s40", dict(S70, qp=12, deblock=True, deblock_offsets=(2, 2), intra=_i)),  # 16 from below
    })
# a right edge that is coded but not displayed: downscale padding, search-window
# clamping, Intra16x16 and deblocking there
CROPPED_WIDTH = {"portrait": (128, (72, 128, 80, 128)), "qcif": (72, (88, 72, 96, 80))}
for _s, (_h, _) in CROPPED_WIDTH.items():
    CASES.update({
        f"{_s}_off": (_s, dict(height=_h)),
        f"{_s}_all": (_s, dict(height=_h, **ALL_ON)),
        f"{_s}_r16_all": (_s, dict(height=_h, search_range=16, **ALL_ON)),
        f"{_s}_qp40_all": (_s, dict(height=_h, qp=40, **ALL_ON)),
    })
COLUMN = dict(height=48, search_range=4, **ALL_ON)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("bytes"), "src": {}, "dec": {}, "ref": {}}


def _source(work, name):
    if name not in work["src"]:
        spec = SOURCES[name]
        if spec is None:
            work["src"][name] = REAL
        elif callable(spec):
            # the base encoder with max_mb_sad < 0 writes every macroblock as
            # I_PCM: a stream that decodes to exactly these frames
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


def _decoded(work, name):
    """The oracle's decode and scene scores of a source, once per module."""
    if name not in work["dec"]:
        frames, info = oracle.decode_full(_source(work, name))
        F, W, H = frames.shape[0], info["width"], info["height"]
        sc = oracle.score_frames(frames.reshape(-1), frames[0].size, F, W, H, W, H, 4, want_rgb=False)["score"]
        if callable(SOURCES[name]):
            assert np.array_equal(frames, SOURCES[name]())
        work["dec"][name] = (frames, W, H, sc)
    return work["dec"][name]


def _oracle_side(work, sname, tk):
    """oracle.transcode of the oracle's decode, once per (source, settings)."""
    key = (sname, tuple(sorted(tk.items())))
    if key not in work["ref"]:
        frames, W, H, sc = _decoded(work, sname)
        kw = {k: v for k, v in tk.items() if k not in ("height", "search_range")}
        R = tk.get("search_range", 8)
        work["ref"][key] = oracle.transcode(frames, W, H, sc, want_recon=True, out_height=tk.get("height", 360),
                                            search_range=max(R, 0), **kw)   # the device's -1 is range 0
    return work["ref"][key]


def _nals(sample):
    out, p = [], 0
    while p + 4 <= len(sample):
        n = int.from_bytes(sample[p:p + 4], "big")
        out.append(sample[p + 4:p + 4 + n])
        p += 4 + n
    return out


def _first_difference(got, want):
    """(frame, macroblock row, byte in the slice NAL) of the first slice that
    differs; a slice is one macroblock row."""
    for f, (a, b) in enumerate(zip(got, want)):
        if a == b:
            continue
        na, nb = _nals(a), _nals(b)
        for row, (x, y) in enumerate(zip(na, nb)):
            if x != y:
                at = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
                return (f"frame {f} ({'IDR' if (x[0] & 31) == 5 else 'P'}), macroblock row {row}: slice of {len(x)} "
                        f"bytes, the oracle's {len(y)}, first differing byte {at}")
        return f"frame {f}: {len(na)} slices, the oracle's {len(nb)}"
    return f"{len(got)} samples, the oracle's {len(want)}"


COUNTS = ("pcm_mbs", "inter_mbs", "skip_mbs", "intra_mbs", "subpel_mbs", "qpel_mbs", "deblock_mbs", "n_idr")


def _check(work, sname, tk, out, session=None):
    ref = _oracle_side(work, sname, tk)
    if session is None:
        with scene.VideoScorer(_source(work, sname)) as v:
            facts = v.transcode(out, **tk)
    else:
        facts = session.transcode(out, **tk)
    m = oracle.read_mp4(out)
    got = [bytes(m["data"][o:o + s]) for o, s in zip(m["offsets"], m["sizes"])]
    print({k: facts[k] for k in COUNTS}, sum(map(len, got)), "bytes; the oracle:", {k: ref[k] for k in COUNTS},
          sum(map(len, ref["samples"])), "bytes")
    assert (facts["width"], facts["height"]) == (ref["width"], ref["height"])
    assert got == ref["samples"], _first_difference(got, ref["samples"])
    assert {k: facts[k] for k in COUNTS} == {k: ref[k] for k in COUNTS}
    sw, sh, ch = ref["width"], ref["height"], ref["coded_height"]
    rec = ref["recon"]
    want = oracle.recon_hash(np.concatenate([rec[:, :sh, :sw], rec[:, ch:ch + sh // 2, :sw]], 1))
    if tk.get("intra") or tk.get("subpel") or tk.get("deblock"):
        assert facts["recon_hash"] == want
    else:
        assert facts["recon_hash"] == 0   # the base encoder computes none (its bytes are pinned above)
    return facts, ref


@pytest.mark.parametrize("case", list(CASES))
def test_optin_paths_write_the_oracles_bytes(work, tmp_path, case):
    _require_gpu()
    sname, tk = CASES[case]
    _check(work, sname, tk, tmp_path / "out.mp4")


@pytest.mark.parametrize("sname", list(CROPPED_WIDTH))
def test_cropped_width_pictures(work, tmp_path, sname):
    """The display width is no multiple of 16: the coded picture has columns
    past the display's right edge, and with all paths on every macroblock kind
    and the filter occur (the bytes themselves: the *_off / *_all cases)."""
    _require_gpu()
    h, geometry = CROPPED_WIDTH[sname]
    facts, ref = _check(work, sname, dict(height=h, **ALL_ON), tmp_path / "out.mp4")
    assert (ref["width"], ref["height"], ref["coded_width"], ref["coded_height"]) == geometry
    assert ref["coded_width"] > ref["width"]
    assert facts["intra_mbs"] > 0 and facts["inter_mbs"] > 0 and facts["deblock_mbs"] > 0


def test_one_macroblock_wide_picture(work, tmp_path):
    """16x48 output: no macroblock has a left neighbour, so every row is
    Intra16x16 DC from 128 or inter with the zero motion predictor, and the
    filter has inner edges only."""
    _require_gpu()
    facts, ref = _check(work, "column", COLUMN, tmp_path / "out.mp4")
    assert (ref["coded_width"], ref["coded_height"]) == (16, 48)
    assert facts["intra_mbs"] > 0 and facts["subpel_mbs"] > 0 and facts["deblock_mbs"] > 0


REPEATED = ["s70_i1_sp2_d1", "keyint8_r16_all", "crafted_qp12_all"]


@pytest.mark.parametrize("case", REPEATED)
def test_fresh_sessions_repeat_the_bytes(work, tmp_path, case):
    """A result that varies from run to run (a lane, tie or ordering defect)
    can decode every time: three more fresh sessions each write the oracle's
    bytes, counts and hash."""
    _require_gpu()
    sname, tk = CASES[case]
    for i in range(3):
        _check(work, sname, tk, tmp_path / f"out{i}.mp4")


def test_one_session_alternating_settings(work, tmp_path):
    """One session that transcodes four times, the paths off, all on, off, all
    on: buffers left by a run with other settings (command words, levels,
    reconstruction slots, the hash) change no byte of the next."""
    _require_gpu()
    sname = "s70"
    off, on = dict(S70), dict(S70, **ALL_ON)
    with scene.VideoScorer(_source(work, sname)) as v:
        for i, tk in enumerate((off, on, off, on)):
            _check(work, sname, tk, tmp_path / f"out{i}.mp4", session=v)
