"""The edges of the transcode driver (csrc/transcode_driver.cpp, DESIGN.md
§11) on the device, each against the CPU byte oracle.

The driver queues levels on one stream and chunks of 16 levels on another,
with a ring of 32 levels of residual data between them.  The byte tests beside
this one use GOPs of at most 70 frames and mostly one or two of them; here the
plans are chosen for the driver's own arithmetic (csrc/enc_plan.h, whose
properties tests/test_enc_plan_host.py checks without a GPU):

  gop50    one GOP of 50 levels = four chunks; levels 32..49 reuse ring slots
           and wait on chunk events;
  keyint1  a plan of one level: the first chunk waits on no search event;
  k33      levels 17..32 hold one entry, level 32 lands on ring slot 0;
  k33_all  the same with every stat slot live;
  cuts     three GOPs of different lengths, with the rate-aware search's
           previous-level index in use.

The picture is 48x32 (3 x 2 macroblocks), so a case takes a fraction of a
second.  Per CAVLC case: every sample byte, SPS / PPS, the counts, the command
and mode words and recon_hash against oracle/transcode_oracle.c, and the
counts the oracle gave when the cases were chosen.  k33_all again with CABAC:
words, counts and hash (the bytes are lossless against the CAVLC stream of the
same call, tests/test_transcode_cabac_gpu.py).
"""
from __future__ import annotations

import pytest

import oracle
from test_transcode_bytes_rate_intra4_gpu import _check
from test_transcode_subpel_gpu import SYNTH, _require_gpu
from vtseg import scene

pytestmark = pytest.mark.gpu

SMALL = dict(width=96, height=64, max_motion=4)
SOURCES = {
    "f50": dict(SYNTH, n_frames=50, **SMALL),
    "f3": dict(SYNTH, n_frames=3, **SMALL),
    "f50cuts": dict(SYNTH, n_frames=50, **SMALL, cut_min_s=0.3, cut_max_s=0.9),
}
ALL = dict(intra=True, intra4x4=True, subpel=2, deblock=True, mvcost=True, early_skip=True)
# name -> (source, transcode keywords, the oracle's n_idr, (pcm, inter, skip) macroblocks)
CASES = {
    "gop50": ("f50", dict(height=32), 1, (6, 48, 246)),
    "keyint1": ("f3", dict(height=32, keyint=1), 3, (18, 0, 0)),
    "k33": ("f50", dict(height=32, keyint=33), 2, (12, 48, 240)),
    "k33_all": ("f50", dict(height=32, keyint=33, **ALL), 2, (0, 62, 226)),
    "cuts": ("f50cuts", dict(height=32, idr_at_cuts=True, mvcost=True, intra=True), 3, (0, 105, 177)),
}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    _require_gpu()
    w = {"dir": tmp_path_factory.mktemp("driver"), "src": {}, "dec": {}, "ref": {}}
    for name, spec in SOURCES.items():  # _source / _decoded of the byte tests look sources up here first
        w["src"][name] = w["dir"] / f"{name}.mp4"
        scene.synth_write(w["src"][name], **spec)
        frames, info = oracle.decode_full(w["src"][name])
        F, W, H = frames.shape[0], info["width"], info["height"]
        sc = oracle.score_frames(frames.reshape(-1), frames[0].size, F, W, H, W, H, 4, want_rgb=False)["score"]
        w["dec"][name] = (frames, W, H, sc)
    return w


def _pinned(facts, ref, n_idr, mbs):
    for side in (ref, facts):
        assert side["n_idr"] == n_idr
        assert (side["pcm_mbs"], side["inter_mbs"], side["skip_mbs"]) == mbs


@pytest.mark.parametrize("case", list(CASES))
def test_driver_edges_write_the_oracles_bytes(work, tmp_path, case):
    _require_gpu()
    sname, tk, n_idr, mbs = CASES[case]
    out = tmp_path / "out.mp4"
    facts, ref = _check(work, sname, tk, out)
    _pinned(facts, ref, n_idr, mbs)
    assert (ref["width"], ref["height"], ref["coded_width"], ref["coded_height"]) == (48, 32, 48, 32)
    m = oracle.read_mp4(out)
    src = oracle.read_mp4(work["src"][sname])
    fps = src["timescale"] / (src["dts"][1] - src["dts"][0])
    sps, pps = oracle.sps_pps(3, 2, 0, 0, fps)
    assert m["sps"][0] == sps and m["pps"][0] == pps
    if case == "k33_all":  # every stat slot live
        for k in ("intra_mbs", "subpel_mbs", "qpel_mbs", "deblock_mbs", "early_skip_mbs", "intra4x4_mbs"):
            assert facts[k] > 0, k


def test_every_stat_slot_with_cabac(work, tmp_path):
    _require_gpu()
    sname, tk, n_idr, mbs = CASES["k33_all"]
    facts, ref = _check(work, sname, tk, tmp_path / "out.mp4", cabac=True)
    _pinned(facts, ref, n_idr, mbs)
