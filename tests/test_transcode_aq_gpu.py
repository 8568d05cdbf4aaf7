"""Adaptive quantisation in the device encoder (vts_transcode_ext9.aq_strength_q8,
DESIGN.md §11 "Adaptive quantisation"): a QP per macroblock, sent as mb_qp_delta.

1. A strength of 1 / 256 moves no macroblock: the file of the same call
   without `aq_strength`, byte for byte, with equal facts.
2. `mb_qp` is the CPU law (csrc/enc_aq.h through its harness) on the encoder's
   input: directly, under a `frame_qp` that changes every picture, under a
   `qp_range` whose two ends the offsets hit, and under a `frame_qp` below 10
   without a `qp_range` (the bounds are then 1 .. 51).
3. Closed loop: the output is decoded by the CPU general oracle and by the
   device's general decoder; the two agree and their hash is the encoder's
   `recon_hash`.  Without mb_qp_delta, the running QP and the per-edge filter
   indices in every stage, this fails.
4. CABAC codes what CAVLC codes.
5. With `bitrate_kbps` the controller is still its CPU twin, and `mb_qp` rides
   on its QPs.
6. IDR pictures with `intra`: the measure is the bytes less the headers.
7. Direction: the faintly textured third of the designed source is coded
   better with `aq_strength`, the noisy third not.

Every transcode runs in a fresh VideoScorer."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import oracle
from test_enc_aq_host import designed_frames, harness_offsets, load
from test_enc_part_host import FLAGS, NATIVE
from test_transcode_intra4_gpu import _samples
from test_transcode_rate_gpu import _is_idr
from test_transcode_ratectl_gpu import ON, SAME, _closed_loop, _twin, law  # noqa: F401  (law: a fixture)
from test_transcode_subpel_gpu import REAL, SYNTH, _require_gpu
from vtseg import scene

pytestmark = pytest.mark.gpu

# name -> (what _source makes of it, the transcode's height)
SOURCES = {"designed": (designed_frames, 64), "s20": (dict(width=320, height=192, n_frames=20), 96), "real": (None, 240)}
INTRA = dict(intra=True, mvcost=True)       # `intra` only: mvcost is what aq needs
SETTINGS = {"intra": INTRA, "on": ON}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("aq"), "src": {}, "run": {}, "input": {}}


@pytest.fixture(scope="module")
def aqlib(tmp_path_factory):
    """The CPU harness of csrc/enc_aq.h (tests/native/enc_aq_host.cpp)."""
    so = tmp_path_factory.mktemp("eaqg") / "libencaqhost.so"
    subprocess.run(["g++", "-Og", "-fPIC", "-shared", *FLAGS, str(NATIVE / "enc_aq_host.cpp"), "-o", str(so)], check=True)
    return load(so)


def _source(work, name):
    if name not in work["src"]:
        spec = SOURCES[name][0]
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


def _input(work, name):
    """The encoder's input pictures [F, ch * 3 / 2, cw]: the source's frames through the oracle's downscale."""
    if name not in work["input"]:
        frames, _ = oracle.decode_full(_source(work, name))
        h, w = frames.shape[1] * 2 // 3, frames.shape[2]
        work["input"][name] = np.stack([oracle.downscale_nv12(f, w, h, SOURCES[name][1]) for f in frames])
    return work["input"][name]


def _offsets(work, aqlib, name, strength_q8=256, aq_max=8):
    return np.stack([harness_offsets(aqlib, p, strength_q8, aq_max) for p in _input(work, name)]).astype(np.int64)


def _transcode(work, sname, out, **kw):
    with scene.VideoScorer(_source(work, sname)) as v:
        return v.transcode(out, height=SOURCES[sname][1], **kw)


def _run(work, key, sname, **kw):
    """One transcode per (key), shared by the tests of this module and never modified."""
    if key not in work["run"]:
        out = work["dir"] / f"{key}.mp4"
        work["run"][key] = (out, _transcode(work, sname, out, **kw))
    return work["run"][key]


def _loop_run(work, sname, setting, cabac):
    return _run(work, f"loop_{sname}_{setting}_{int(cabac)}", sname, aq_strength=1.0, cabac=cabac, want_commands=True,
                **SETTINGS[setting])


# -------------------------------------- 1. the smallest strength moves nothing
@pytest.mark.parametrize("cabac", [False, True])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_a_strength_of_one_256th_is_the_call_without_aq(work, tmp_path, setting, cabac):
    _require_gpu()
    base_out, aq_out = tmp_path / "base.mp4", tmp_path / "aq.mp4"
    base = _transcode(work, "designed", base_out, cabac=cabac, **SETTINGS[setting])
    assert "mb_qp" not in base
    facts = _transcode(work, "designed", aq_out, cabac=cabac, aq_strength=1 / 256, **SETTINGS[setting])
    assert aq_out.read_bytes() == base_out.read_bytes()
    for k in base:
        if not k.endswith("_ms"):
            assert facts[k] == base[k], f"{k}: {facts[k]} with aq, {base[k]} without"
    assert (facts["mb_qp"] == 28).all() and facts["aq_lo"] == facts["aq_hi"] == facts["aq_mbs"] == 0


# ------------------------------------------------- 2. mb_qp is the CPU law
@pytest.mark.parametrize("sname", ["designed", "s20"])
def test_mb_qp_is_the_cpu_law_on_the_encoders_input(work, aqlib, sname):
    _require_gpu()
    _, facts = _loop_run(work, sname, "on", False)
    off = _offsets(work, aqlib, sname)
    assert facts["mb_qp"].shape == off.shape
    assert np.array_equal(facts["mb_qp"], np.clip(28 + off, 1, 51))
    assert facts["aq_lo"] == off.min() and facts["aq_hi"] == off.max() and facts["aq_mbs"] == np.count_nonzero(off)
    if sname == "designed":
        assert off.min() == -8 and off.max() > 0


def test_mb_qp_under_a_changing_frame_qp_and_under_a_qp_range(work, aqlib, tmp_path):
    _require_gpu()
    off = _offsets(work, aqlib, "designed")
    n = off.shape[0]
    fq = np.array([20, 51, 1, 33, 28, 45][:n], np.uint8)
    out = tmp_path / "fq.mp4"
    facts = _transcode(work, "designed", out, frame_qp=fq, aq_strength=1.0, **ON)
    assert np.array_equal(facts["frame_qp"], fq)
    assert np.array_equal(facts["mb_qp"], np.clip(fq.astype(np.int64)[:, None, None] + off, 1, 51))
    _closed_loop(out, facts)
    # offsets of -8 and of +6 and more around 26 inside (20, 30): both ends are hit
    out = tmp_path / "range.mp4"
    facts = _transcode(work, "designed", out, frame_qp=[26] * n, qp_range=(20, 30), aq_strength=1.0, **ON)
    want = np.clip(26 + off, 20, 30)
    assert np.array_equal(facts["mb_qp"], want)
    assert (26 + off).min() < 20 == want.min() and (26 + off).max() > 30 == want.max()
    _closed_loop(out, facts)
    # another strength and another aq_max
    facts = _transcode(work, "designed", tmp_path / "s.mp4", aq_strength=0.5, aq_max=3, **INTRA)
    off = _offsets(work, aqlib, "designed", 128, 3)
    assert np.array_equal(facts["mb_qp"], 28 + off) and facts["aq_lo"] == -3


@pytest.mark.parametrize("cabac", [False, True])
def test_a_frame_qp_below_10_without_a_qp_range_is_clamped_to_1_51_only(work, aqlib, tmp_path, cabac):
    """Without a `qp_range` the macroblocks' bounds are 1 .. 51, not the rate controller's default 10 .. 51: a
    macroblock whose offset is 0 keeps its picture's QP, and the smallest strength is still the call without aq."""
    _require_gpu()
    off = _offsets(work, aqlib, "designed")
    fq = np.array([5, 3, 9, 1, 7, 12], np.uint8)
    out = tmp_path / "low.mp4"
    facts = _transcode(work, "designed", out, frame_qp=fq, aq_strength=1.0, cabac=cabac, **ON)
    assert np.array_equal(facts["mb_qp"], np.clip(fq.astype(np.int64)[:, None, None] + off, 1, 51))
    assert (facts["mb_qp"][off == 0] == np.broadcast_to(fq[:, None, None], off.shape)[off == 0]).all() and (off == 0).any()
    _closed_loop(out, facts)
    base_out, tiny_out = tmp_path / "base.mp4", tmp_path / "tiny.mp4"
    base = _transcode(work, "designed", base_out, frame_qp=fq, cabac=cabac, **ON)
    tiny = _transcode(work, "designed", tiny_out, frame_qp=fq, aq_strength=1 / 256, cabac=cabac, **ON)
    assert tiny_out.read_bytes() == base_out.read_bytes()
    assert tiny["recon_hash"] == base["recon_hash"] and np.array_equal(tiny["frame_bits"], base["frame_bits"])
    assert np.array_equal(tiny["mb_qp"], np.broadcast_to(fq[:, None, None], off.shape))
    # one bound given: the other one is still 1 or 51
    facts = _transcode(work, "designed", tmp_path / "lo.mp4", frame_qp=[12] * 6, qp_range=(8, 0), aq_strength=1.0, **INTRA)
    assert np.array_equal(facts["mb_qp"], np.clip(12 + off, 8, 51)) and facts["mb_qp"].min() == 8


# ----------------------------------------------------------- 3. closed loop
@pytest.mark.parametrize("cabac", [False, True])
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("sname", list(SOURCES))
def test_output_with_aq_decodes_to_the_encoders_reconstruction(work, sname, setting, cabac):
    _require_gpu()
    out, facts = _loop_run(work, sname, setting, cabac)
    _closed_loop(out, facts)
    print(f"{sname} {setting} cabac={cabac}: {out.stat().st_size} bytes; inter {facts['inter_mbs']} skip {facts['skip_mbs']} "
          f"intra {facts['intra_mbs']} pcm {facts['pcm_mbs']}; offsets {facts['aq_lo']}..{facts['aq_hi']}, {facts['aq_mbs']} moved")
    # the rule's branches are met
    assert facts["skip_mbs"] > 0 and facts["inter_mbs"] > 0 and facts["intra_mbs"] > 0 and facts["aq_mbs"] > 0


@pytest.mark.parametrize("cabac", [False, True])
def test_closed_loop_with_a_bitrate_and_with_a_frame_range(work, tmp_path, cabac):
    _require_gpu()
    out = tmp_path / "kbps.mp4"
    facts = _transcode(work, "s20", out, keyint=8, bitrate_kbps=60, aq_strength=1.0, cabac=cabac, **ON)
    _closed_loop(out, facts)
    assert facts["aq_mbs"] > 0 and len(set(facts["frame_qp"].tolist())) > 1
    out = tmp_path / "range.mp4"
    facts = _transcode(work, "s20", out, frames=(2, 5), aq_strength=1.0, cabac=cabac, **ON)
    assert facts["n_frames"] == 3 and facts["mb_qp"].shape[0] == 3
    _closed_loop(out, facts)
    assert facts["aq_mbs"] > 0


def test_a_frame_range_takes_the_offsets_of_its_own_frames(work, aqlib, tmp_path):
    _require_gpu()
    off = _offsets(work, aqlib, "s20")
    facts = _transcode(work, "s20", tmp_path / "r.mp4", frames=(2, 5), aq_strength=1.0, **INTRA)
    assert np.array_equal(facts["mb_qp"], np.clip(28 + off[2:5], 1, 51))


# ------------------------------------------- 4. CABAC codes what CAVLC codes
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("sname", list(SOURCES))
def test_cabac_codes_what_cavlc_codes_with_aq(work, sname, setting):
    _require_gpu()
    _, off = _loop_run(work, sname, setting, False)
    _, on = _loop_run(work, sname, setting, True)
    for k in SAME:
        if k in off:
            assert on[k] == off[k], f"{k}: {on[k]} with cabac, {off[k]} without"
    assert np.array_equal(on["commands"], off["commands"]) and np.array_equal(on["mb_qp"], off["mb_qp"])


# ------------------------------------------- 5. the controller is its twin
def test_device_qps_are_the_cpu_replay_and_mb_qp_rides_on_them(work, law, aqlib):  # noqa: F811
    _require_gpu()
    out, facts = _run(work, "twin", "s20", keyint=8, bitrate_kbps=40, qp=26, qp_range=(22, 40), aq_strength=1.0, **ON)
    want, lens = _twin(law, out, facts, 40, 26, 22, 40)
    print(f"GOPs {lens}; QPs {facts['frame_qp'].tolist()}; bits {facts['frame_bits'].tolist()}")
    assert np.array_equal(facts["frame_qp"], want)
    assert len(set(facts["frame_qp"].tolist())) > 2                  # the controller moved
    off = _offsets(work, aqlib, "s20")
    assert np.array_equal(facts["mb_qp"], np.clip(facts["frame_qp"].astype(np.int64)[:, None, None] + off, 22, 40))
    _closed_loop(out, facts)


# ------------------------------------------------------------ 6. the measure
@pytest.mark.parametrize("q", [12, 28, 45])
def test_idr_pictures_with_aq_measure_their_bytes_less_the_headers(work, q):
    """As the same test without aq (test_transcode_ratectl_gpu.py): the measure counts the true se(mb_qp_delta)."""
    _require_gpu()
    out, facts = _run(work, f"idr_measure{q}", "s20", keyint=8, frame_qp=[q] * 20, aq_strength=1.0, **ON)
    mbh = 6
    samples = _samples(out)
    assert [i for i, idr in enumerate(_is_idr(out)) if idr] == [0, 8, 16] and facts["aq_mbs"] > 0
    for f in (0, 8, 16):
        nbytes, e = len(samples[f]), samples[f].count(b"\x00\x00\x03")
        bits = int(facts["frame_bits"][f])
        print(f"qp {q} frame {f}: {nbytes} bytes, {e} emulation prevention bytes, measure {bits} bits = {bits / 8:.1f} bytes")
        assert 8 * nbytes - 8 * (16 * mbh + e) <= bits <= 8 * nbytes


# -------------------------------------------------------------- 7. direction
def test_aq_spends_its_bits_on_the_faint_texture(work, tmp_path):
    """Designed source, every picture IDR, `intra` only, QP 30: the middle third (a ramp with faint noise, offsets
    below 0) is closer to the source with aq than without, the right third (noise, offsets above 0) is not."""
    _require_gpu()
    src = _input(work, "designed")[:, :64].astype(np.int64)          # luma of the encoder's input
    sse = {}
    for name, s in (("off", 0.0), ("on", 1.0)):
        out = tmp_path / f"{name}.mp4"
        _transcode(work, "designed", out, keyint=1, qp=30, aq_strength=s, **INTRA)
        rec, _ = oracle.decode_full(out)
        d = (rec[:, :64].astype(np.int64) - src) ** 2
        sse[name] = [int(d[:, :, 32 * t:32 * t + 32].sum()) for t in range(3)]
    print(f"squared error by third (left, middle, right): off {sse['off']}, on {sse['on']}")
    assert sse["on"][1] < sse["off"][1]
    assert sse["on"][2] >= sse["off"][2]
