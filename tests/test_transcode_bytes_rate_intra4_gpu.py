"""Byte parity of the device encoder's rate-aware motion decisions (`mvcost`,
`early_skip`) and of its Intra_4x4 coding (`intra4x4`) with the CPU oracle
(oracle/transcode_oracle.c, `or_transcode_ex2`).

tests/test_transcode_bytes_gpu.py holds `intra`, `subpel` and `deblock` to the
oracle byte for byte; the three rules merged after it were pinned by closed
loops, by a partial restatement of the vectors and by the legality of each
reported mode.  None of those sees a block whose least-key mode was missed, a
predicted mode that is stale, a bit count that differs from the bits written,
an I_NxN / Intra16x16 / I_PCM choice resolved the other way, or a vector whose
cost used the wrong predictor guess: all of them still decode.  Here the
oracle restates the rules and, per case and in this order (so that a failure
names a macroblock before it names a byte):

1. every command word equals the oracle's;
2. every Intra_4x4 mode word equals the oracle's;
3. every output byte equals the oracle's;
4. every count does, `early_skip_mbs` and `intra4x4_mbs` included;
5. `recon_hash` is the hash of the oracle's reconstruction.

Then the same settings with `cabac=True`: entropy coding is lossless, so its
words, counts and hash must equal the *oracle's* (the oracle writes no CABAC
bytes).  Every transcode runs in a fresh VideoScorer unless the test says
otherwise; the oracle's side is computed once per (source, settings).
tests/test_transcode_oracle.py checks the oracle itself without a GPU, and
that these cases make each rule decide (`test_gpu_cases_exercise_every_decision`).
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from test_transcode_bytes_gpu import ALL_ON, _decoded, _first_difference, _source
from test_transcode_intra4_gpu import CASES as INTRA4_CASES
from test_transcode_subpel_gpu import _require_gpu
from vtseg import scene

pytestmark = pytest.mark.gpu

RATE = {"mv": dict(mvcost=True), "es": dict(early_skip=True), "both": dict(mvcost=True, early_skip=True)}
EVERY = dict(ALL_ON, mvcost=True, early_skip=True, intra4x4=True)
S70 = dict(height=96)

# name -> (source, transcode kwargs of both sides)
CASES = {}
for _m, _f in RATE.items():
    for _sp in (0, 2):
        for _i in (False, True):
            CASES[f"s70_{_m}_sp{_sp}_i{int(_i)}"] = ("s70", dict(S70, subpel=_sp, intra=_i, **_f))
CASES.update({
    "s70_both_all": ("s70", dict(S70, **ALL_ON, **RATE["both"])),
    "s70_lambda400_sp2": ("s70", dict(S70, subpel=2, mvcost=True, mv_lambda16=400)),
    # the search ranges: 0 (the refinement alone), the <4> and <16> instances and the any-range one
    "r0_both_sp2": ("s40", dict(S70, search_range=-1, subpel=2, **RATE["both"])),
    "r4_both_sp2": ("s40", dict(S70, search_range=4, subpel=2, **RATE["both"])),
    "r5_both_sp2": ("s40", dict(S70, search_range=5, subpel=2, **RATE["both"])),
    "r16_both_sp2": ("s40", dict(S70, search_range=16, subpel=2, **RATE["both"])),
})
# the fourteen of test_transcode_intra4_gpu.py (keyint8_r16_every: many IDR levels, the guess resets at j = 1)
for _name, (_src, _kw, _) in INTRA4_CASES.items():
    CASES[f"i4_{_name}"] = (_src, dict(_kw, intra4x4=True))
CASES.update({
    "i4_pan_intra": ("pan", dict(S70, intra=True, intra4x4=True)),
    "i4_odd_intra": ("odd", dict(height=120, search_range=4, intra=True, intra4x4=True)),
    # what the decision counters asked for (tests/test_transcode_oracle.py): edges at many angles for the modes 3 .. 8,
    # constants for ties and equal bits, noise at qp 1 for the 3072 bound, the dead zone for the probe
    "i4_diag_every": ("diag", dict(height=64, **EVERY)),
    "i4_diag_qp1_every": ("diag", dict(height=64, qp=1, **EVERY)),
    "i4_diag_allpcm_qp40": ("diag", dict(height=64, qp=40, max_mb_sad=-1, intra=True, intra4x4=True, deblock=True)),
    "i4_noisy_every": ("noisy", dict(height=64, **EVERY)),
})
COUNTS = ("pcm_mbs", "inter_mbs", "skip_mbs", "intra_mbs", "subpel_mbs", "qpel_mbs", "deblock_mbs", "n_idr",
          "early_skip_mbs", "intra4x4_mbs")
NEW = ("mvcost", "early_skip", "mv_lambda16", "intra4x4")


def oracle_side(decoded, tk):
    """oracle.transcode of a decoded source (frames, W, H, scores) with the device's keywords."""
    frames, W, H, sc = decoded
    kw = {k: v for k, v in tk.items() if k not in ("height", "search_range")}
    return oracle.transcode(frames, W, H, sc, want_recon=True, want_words=True, out_height=tk.get("height", 360),
                            search_range=max(tk.get("search_range", 8), 0), **kw)   # the device's -1 is range 0


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("bytes_ri4"), "src": {}, "dec": {}, "ref": {}}


def _oracle_side(work, sname, tk):
    key = (sname, tuple(sorted(tk.items())))
    if key not in work["ref"]:
        work["ref"][key] = oracle_side(_decoded(work, sname), tk)
    return work["ref"][key]


def _first_word(got, want):
    f, my, mx = (int(v[0]) for v in np.nonzero(got != want))
    return f, my, mx


def _check(work, sname, tk, out, session=None, cabac=False):
    ref = _oracle_side(work, sname, tk)
    kw = dict(tk, cabac=cabac, want_commands=True, want_intra4_modes=True)
    if session is None:
        with scene.VideoScorer(_source(work, sname)) as v:
            facts = v.transcode(out, **kw)
    else:
        facts = session.transcode(out, **kw)
    m = oracle.read_mp4(out)
    got = [bytes(m["data"][o:o + s]) for o, s in zip(m["offsets"], m["sizes"])]
    print({k: facts[k] for k in COUNTS}, sum(map(len, got)), "bytes, cabac", cabac, "; the oracle:",
          {k: ref[k] for k in COUNTS}, sum(map(len, ref["samples"])), "bytes")
    assert (facts["width"], facts["height"]) == (ref["width"], ref["height"])
    cmds, words = facts["commands"], facts["intra4_modes"]
    assert cmds.shape == ref["commands"].shape and words.shape == ref["intra4_modes"].shape
    if not np.array_equal(cmds, ref["commands"]):
        f, my, mx = _first_word(cmds, ref["commands"])
        pytest.fail(f"command word of frame {f} macroblock (mx {mx}, my {my}): {int(cmds[f, my, mx]):#010x}, "
                    f"the oracle's {int(ref['commands'][f, my, mx]):#010x}; "
                    f"{int((cmds != ref['commands']).sum())} words differ")
    if not np.array_equal(words, ref["intra4_modes"]):
        f, my, mx = _first_word(words, ref["intra4_modes"])
        a, b = int(words[f, my, mx]), int(ref["intra4_modes"][f, my, mx])
        k = next(k for k in range(16) if (a >> (4 * k)) & 15 != (b >> (4 * k)) & 15)
        pytest.fail(f"frame {f} macroblock (mx {mx}, my {my}) block {k}: Intra4x4PredMode {(a >> (4 * k)) & 15}, "
                    f"the oracle's {(b >> (4 * k)) & 15} (words {a:#018x}, {b:#018x})")
    if not cabac:
        assert got == ref["samples"], _first_difference(got, ref["samples"])
    assert {k: facts[k] for k in COUNTS} == {k: ref[k] for k in COUNTS}
    sw, sh, ch = ref["width"], ref["height"], ref["coded_height"]
    rec = ref["recon"]
    want = oracle.recon_hash(np.concatenate([rec[:, :sh, :sw], rec[:, ch:ch + sh // 2, :sw]], 1))
    if any(tk.get(k) for k in NEW + ("intra", "subpel", "deblock")):
        assert facts["recon_hash"] == want
    else:
        assert facts["recon_hash"] == 0   # the base encoder computes none (its bytes are pinned above)
    return facts, ref


@pytest.mark.parametrize("case", list(CASES))
def test_rate_and_intra4_write_the_oracles_bytes(work, tmp_path, case):
    _require_gpu()
    sname, tk = CASES[case]
    assert any(tk.get(k) for k in NEW)
    _check(work, sname, tk, tmp_path / "out.mp4")


@pytest.mark.parametrize("case", list(CASES))
def test_cabac_decides_what_the_oracle_decides(work, tmp_path, case):
    """CABAC codes the same decisions: its words, counts and hash against the
    oracle's, not against the CAVLC run's."""
    _require_gpu()
    sname, tk = CASES[case]
    _check(work, sname, tk, tmp_path / "out.mp4", cabac=True)


REPEATED = ["i4_small_every", "i4_keyint8_r16_every"]


@pytest.mark.parametrize("case", REPEATED)
def test_fresh_sessions_repeat_the_bytes(work, tmp_path, case):
    """A lane or tie defect may vary from run to run and still decode: three
    more fresh sessions each write the oracle's words, bytes, counts and hash."""
    _require_gpu()
    sname, tk = CASES[case]
    for i in range(3):
        _check(work, sname, tk, tmp_path / f"out{i}.mp4")


def test_one_session_alternating_settings(work, tmp_path):
    """One session that transcodes off, everything on, off, everything on:
    what a run leaves behind (command and mode words, levels, reconstruction
    slots, the previous level's words that the predictor guess reads) changes
    nothing of the next; each against its own oracle."""
    _require_gpu()
    off, on = dict(S70), dict(S70, **EVERY)
    with scene.VideoScorer(_source(work, "s70")) as v:
        for i, tk in enumerate((off, on, off, on)):
            facts, ref = _check(work, "s70", tk, tmp_path / f"out{i}.mp4", session=v)
            assert (facts["intra4x4_mbs"] > 0) == (tk is on)
