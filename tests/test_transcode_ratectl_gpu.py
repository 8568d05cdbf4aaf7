"""Per-picture QP and per-GOP rate control in the device encoder
(vts_transcode_ext7.frame_qp / bitrate_kbps, DESIGN.md §11 "Rate control").

1. A constant `frame_qp`, and a controller pinned by `qp_range = (q, q)`, are
   the fixed-QP path: the same MP4 bytes, counts and hash.
2. Pictures depend only on their own GOP's QPs.
3. Closed loop at a QP that changes on every picture: the output is decoded by
   the CPU general oracle and by the device's general decoder; the two agree
   and their hash is the encoder's `recon_hash`; CABAC codes what CAVLC codes.
4. The rate measure: I_PCM pictures, all-P_Skip pictures, and IDR pictures
   against the bytes written.
5. The controller is its CPU twin: `frame_qp` of a `bitrate_kbps` call equals
   the harness's replay of the law on the call's own `frame_bits`.
6. Response: a quarter of the fixed-QP size asks for fewer bytes and gets
   them, four times the size gets more.
7. Off is the parent, the argument errors.

Every transcode runs in a fresh VideoScorer."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

import oracle
from test_enc_part_host import FLAGS, NATIVE
from test_transcode_intra4_gpu import _samples
from test_transcode_part_gpu import SOURCES as PART_SOURCES, quads_frames
from test_transcode_rate_gpu import _device_frames, _is_idr
from test_transcode_subpel_gpu import REAL, SYNTH, _require_gpu
from vtseg import VtsegError, _lib, scene

pytestmark = pytest.mark.gpu

SOURCES = dict(PART_SOURCES,
               s20=dict(width=320, height=192, n_frames=20),       # keyint 8: GOPs of 8, 8 and 4
               s17=dict(width=320, height=192, n_frames=17),       # keyint 8: the last GOP is one picture
               still=lambda: np.repeat(quads_frames(F=1), 6, axis=0))
ON = dict(intra=True, intra4x4=True, subpel=2, deblock=True, mvcost=True, early_skip=True, partitions=True)
CYCLE = (20, 51, 1, 33, 28, 45, 12)
SAME = ("width", "height", "n_frames", "n_idr", "pcm_mbs", "inter_mbs", "skip_mbs", "intra_mbs", "subpel_mbs", "qpel_mbs",
        "deblock_mbs", "early_skip_mbs", "intra4x4_mbs", "p16x8_mbs", "p8x16_mbs", "p8x8_mbs", "recon_hash")


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("ratectl"), "src": {}, "run": {}}


@pytest.fixture(scope="module")
def law(tmp_path_factory):
    """The CPU harness of csrc/enc_ratectl.h (tests/native/enc_ratectl_host.cpp)."""
    so = tmp_path_factory.mktemp("erch") / "libencratectlhost.so"
    subprocess.run(["g++", "-Og", "-fPIC", "-shared", *FLAGS, str(NATIVE / "enc_ratectl_host.cpp"), "-o", str(so)],
                   check=True)
    L = C.CDLL(str(so))
    L.erch_frame_budget.argtypes = [C.c_int, C.c_int64, C.c_int64]
    L.erch_frame_budget.restype = C.c_int64
    L.erch_replay.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.erch_replay.restype = None
    return L


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


def _run(work, key, sname, **kw):
    """One transcode per (key), shared by the tests of this module and never modified."""
    if key not in work["run"]:
        out = work["dir"] / f"{key}.mp4"
        work["run"][key] = (out, _transcode(work, sname, out, **kw))
    return work["run"][key]


def _closed_loop(out, facts):
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
    return frames


# ---------------------------------- 1. a constant frame_qp is the fixed-QP path
# the last case: the caller's mv_lambda16 replaces the table's lambda at every picture's QP too
@pytest.mark.parametrize("q,cabac,lam", [(1, False, 0), (1, True, 0), (28, False, 0), (28, True, 0), (51, False, 0),
                                         (51, True, 0), (28, False, 40)])
def test_constant_frame_qp_and_a_pinned_controller_are_the_fixed_qp_path(work, tmp_path, q, cabac, lam):
    _require_gpu()
    kw = dict(height=96, cabac=cabac, mv_lambda16=lam, **ON)
    base_out = tmp_path / "base.mp4"
    base = _transcode(work, "s40", base_out, qp=q, **kw)            # no new struct
    assert "frame_qp" not in base
    n = base["n_frames"]
    for name, extra in (("frame_qp", dict(frame_qp=[q] * n)), ("pinned", dict(bitrate_kbps=500, qp_range=(q, q)))):
        out = tmp_path / f"{name}.mp4"
        facts = _transcode(work, "s40", out, qp=33, **extra, **kw)  # the call's own qp is not what codes a picture
        assert out.read_bytes() == base_out.read_bytes(), name
        for k in SAME:
            assert facts[k] == base[k], f"{name}: {k} {facts[k]}, {base[k]} at qp {q}"
        assert (facts["frame_qp"] == q).all() and facts["qp_lo"] == facts["qp_hi"] == q and facts["qp_mean"] == q
        assert facts["est_bits"] == int(facts["frame_bits"].astype(np.int64).sum()) > 0
    if lam:     # the case is not vacuous: the table's lambda at this QP (74) gives other bytes
        _, table = _run(work, f"table_lambda_{q}", "s40", qp=q, **dict(kw, mv_lambda16=0))
        assert table["recon_hash"] != base["recon_hash"]


# -------------------------------- 2. pictures depend on their own GOP's QPs only
def test_a_gop_is_coded_as_the_constant_call_at_its_qp(work):
    _require_gpu()
    kw = dict(height=96, keyint=8, **ON)
    gops = ((0, 8, 20), (8, 16, 40), (16, 20, 31))
    fq = np.concatenate([np.full(b - a, q, np.uint8) for a, b, q in gops])
    out, facts = _run(work, "gops", "s20", frame_qp=fq, **kw)
    assert facts["n_idr"] == 3 and np.array_equal(facts["frame_qp"], fq)
    mixed = _samples(out)
    assert [i for i, idr in enumerate(_is_idr(out)) if idr] == [0, 8, 16]
    for a, b, q in gops:
        const_out, _ = _run(work, f"const{q}", "s20", qp=q, **kw)
        assert mixed[a:b] == _samples(const_out)[a:b], f"GOP [{a}, {b}) at QP {q}"
    # a QP that changes on every frame: the IDR picture is the constant call's at frame_qp[0]
    cyc = [CYCLE[f % len(CYCLE)] for f in range(20)]
    cyc_out, _ = _run(work, "cycle_s20", "s20", frame_qp=cyc, **kw)
    assert _samples(cyc_out)[0] == _samples(_run(work, "const20", "s20", qp=20, **kw)[0])[0]
    assert _samples(cyc_out)[1] != _samples(_run(work, "const20", "s20", qp=20, **kw)[0])[1]


# ------------------------------------------- 3. closed loop at a changing QP
LOOP = {
    "tiny": ("tiny", dict(height=24, search_range=4, **ON)),                       # 2 x 2 macroblocks
    "column": ("column", dict(height=48, search_range=4, **ON)),                   # mbw = 1
    "quads": ("quads", dict(height=64, **ON)),
    "s70_keyint8_r16": ("s70", dict(height=96, keyint=8, search_range=16, **ON)),
}


def _cycle_run(work, case, cabac):
    sname, kw = LOOP[case]
    with scene.VideoScorer(_source(work, sname)) as v:
        n = int(v.info.n_frames)
    fq = np.array([CYCLE[f % len(CYCLE)] for f in range(n)], np.uint8)
    return fq, _run(work, f"loop_{case}_{int(cabac)}", sname, frame_qp=fq, cabac=cabac, want_commands=True,
                    want_vectors=True, **kw)


@pytest.mark.parametrize("cabac", [False, True])
@pytest.mark.parametrize("case", list(LOOP))
def test_output_at_a_changing_qp_decodes_to_the_encoders_reconstruction(work, case, cabac):
    _require_gpu()
    fq, (out, facts) = _cycle_run(work, case, cabac)
    _closed_loop(out, facts)
    assert np.array_equal(facts["frame_qp"], fq)
    assert facts["qp_lo"] == min(fq) and facts["qp_hi"] == max(fq) and facts["qp_mean"] == pytest.approx(fq.mean())
    print(f"{case} cabac={cabac}: {out.stat().st_size} bytes, est {facts['est_bits'] // 8} bytes; inter {facts['inter_mbs']} "
          f"skip {facts['skip_mbs']} intra {facts['intra_mbs']} pcm {facts['pcm_mbs']}")


@pytest.mark.parametrize("case", list(LOOP))
def test_cabac_codes_what_cavlc_codes_at_a_changing_qp(work, case):
    _require_gpu()
    _, (_, off) = _cycle_run(work, case, False)
    _, (_, on) = _cycle_run(work, case, True)
    for k in SAME:
        assert on[k] == off[k], f"{k}: {on[k]} with cabac, {off[k]} without"
    assert np.array_equal(on["commands"], off["commands"]) and np.array_equal(on["vectors"], off["vectors"])
    assert np.array_equal(on["frame_bits"], off["frame_bits"])       # the measure is counted in CAVLC bits


# ------------------------------------------------------------ 4. the measure
def test_pcm_pictures_measure_3072_a_macroblock_and_skipped_pictures_nothing(work, tmp_path):
    _require_gpu()
    # a still source without intra: the IDR picture is I_PCM (no kernel codes it), every P picture predicts it exactly
    out = tmp_path / "still.mp4"
    facts = _transcode(work, "still", out, height=64, mvcost=True, frame_qp=[28] * 6, want_commands=True)
    nmb = 6 * 4
    assert facts["pcm_mbs"] == nmb and facts["skip_mbs"] == 5 * nmb
    assert (facts["commands"][1:] == 0).all()                        # vector (0, 0); with skip_mbs: nothing coded
    assert facts["frame_bits"].tolist() == [3072 * nmb] + [0] * 5
    assert facts["est_bits"] == 3072 * nmb
    # the same with early_skip: the probe's P_Skip measures 0 too
    facts = _transcode(work, "still", tmp_path / "es.mp4", height=64, mvcost=True, early_skip=True, frame_qp=[28] * 6)
    assert facts["early_skip_mbs"] == 5 * nmb and facts["frame_bits"].tolist() == [3072 * nmb] + [0] * 5
    # GOPs of a moving source without intra: every IDR picture, and the feature off measures nothing
    facts = _transcode(work, "s20", tmp_path / "s20.mp4", height=96, keyint=8, mvcost=True, frame_qp=[28] * 20)
    nmb = 10 * 6
    assert [int(facts["frame_bits"][f]) for f in (0, 8, 16)] == [3072 * nmb] * 3
    off = _transcode(work, "s20", tmp_path / "off.mp4", height=96, keyint=8, mvcost=True, qp=31, want_rate=True)
    assert (off["frame_bits"] == 0).all() and off["est_bits"] == 0 and (off["frame_qp"] == 31).all()
    assert off["qp_lo"] == off["qp_hi"] == 31


@pytest.mark.parametrize("q", [12, 28, 45])
def test_idr_pictures_measure_their_bytes_less_the_headers(work, q):
    """With intra, CAVLC and a constant QP the measure of an IDR picture is the exact macroblock_layer() bits:
    the sample's bytes less, per slice, the length prefix, the NAL and slice headers and the trailing bits (at
    most 16 bytes) and the emulation prevention bytes."""
    _require_gpu()
    out, facts = _run(work, f"idr_measure{q}", "s20", height=96, keyint=8, frame_qp=[q] * 20, **ON)
    mbh = 6
    samples = _samples(out)
    for f in (0, 8, 16):
        nbytes, e = len(samples[f]), samples[f].count(b"\x00\x00\x03")
        bits = int(facts["frame_bits"][f])
        print(f"qp {q} frame {f}: {nbytes} bytes, {e} emulation prevention bytes, measure {bits} bits = {bits / 8:.1f} bytes")
        assert 8 * nbytes - 8 * (16 * mbh + e) <= bits <= 8 * nbytes
    assert facts["est_bits"] == int(facts["frame_bits"].astype(np.int64).sum())


# ------------------------------------------------ 5. the controller is its twin
def _twin(law, out, facts, kbps, qp, lo, hi):
    m = oracle.read_mp4(out)
    delta = m["dts"][1] - m["dts"][0] if len(m["dts"]) > 1 else m["timescale"] // 30
    B = law.erch_frame_budget(kbps, delta, m["timescale"])
    assert B == kbps * 1000 * delta // m["timescale"]
    starts = [i for i, idr in enumerate(_is_idr(out)) if idr] + [facts["n_frames"]]
    want = np.zeros(facts["n_frames"], np.uint8)
    for a, b in zip(starts[:-1], starts[1:]):
        bits = np.ascontiguousarray(facts["frame_bits"][a:b], dtype=np.uint32)
        qps = np.zeros(b - a, np.uint8)
        law.erch_replay(B, b - a, qp, lo, hi, bits.ctypes.data, qps.ctypes.data)
        want[a:b] = qps
    return want, [b - a for a, b in zip(starts[:-1], starts[1:])]


@pytest.mark.parametrize("case", ["s17_keyint8", "s70_cuts", "s17_keyint8_cabac_range"])
def test_device_qps_are_the_cpu_replay_of_the_law_on_the_calls_own_measure(work, law, case):
    _require_gpu()
    sname, kbps, qp, rng_, kw = {
        "s17_keyint8": ("s17", 60, 28, (0, 0), dict(keyint=8)),
        "s70_cuts": ("s70", 40, 24, (0, 0), dict(idr_at_cuts=True)),
        "s17_keyint8_cabac_range": ("s17", 25, 30, (26, 36), dict(keyint=8, cabac=True)),
    }[case]
    out, facts = _run(work, f"twin_{case}", sname, height=96, bitrate_kbps=kbps, qp=qp, qp_range=rng_, **kw, **ON)
    lo, hi = (rng_[0] or 10), (rng_[1] or 51)
    want, lens = _twin(law, out, facts, kbps, qp, lo, hi)
    print(f"{case}: GOPs {lens}; QPs {facts['frame_qp'].tolist()}; bits {facts['frame_bits'].tolist()}; "
          f"{out.stat().st_size} bytes")
    assert np.array_equal(facts["frame_qp"], want)
    if case == "s17_keyint8":
        assert lens == [8, 8, 1]
    if case == "s70_cuts":
        assert len(set(lens)) > 1                                   # unequal GOPs: entry indices differ between levels
    assert len(set(facts["frame_qp"].tolist())) > 2                  # the controller moved
    assert facts["qp_lo"] >= lo and facts["qp_hi"] <= hi
    _closed_loop(out, facts)


# ----------------------------------------------------------------- 6. response
def test_a_lower_bitrate_gives_fewer_bytes_and_a_higher_one_more(work, tmp_path):
    _require_gpu()
    kw = dict(intra=True, subpel=2, mvcost=True, early_skip=True)
    base_out = tmp_path / "qp28.mp4"
    base = _transcode(work, "content", base_out, qp=28, **kw)
    s0 = base_out.stat().st_size
    m = oracle.read_mp4(base_out)
    idr = np.array(_is_idr(base_out))
    p_bytes = int(np.array(m["sizes"])[~idr].sum())
    mbh = (base["height"] + 15) // 16
    # the precondition: the P pictures carry residual at QP 28 (they hold several times their slices' overhead)
    assert p_bytes > 4 * 16 * mbh * int((~idr).sum()), p_bytes
    duration = base["n_frames"] * (m["dts"][1] - m["dts"][0]) / m["timescale"]
    got = {}
    for name, worth in (("quarter", s0 / 4), ("four", 4 * s0)):
        kbps = max(1, int(worth * 8 / duration / 1000))
        out = tmp_path / f"{name}.mp4"
        facts = _transcode(work, "content", out, qp=28, bitrate_kbps=kbps, **kw)
        size = out.stat().st_size
        got[name] = (size, facts["qp_mean"])
        print(f"content {name}: {kbps} kbps = {worth:.0f} bytes; achieved {size} bytes ({size / worth:.3f} of the target); "
              f"fixed QP 28 {s0} bytes; QP {facts['qp_lo']}..{facts['qp_hi']} mean {facts['qp_mean']:.2f}; "
              f"measure / bytes {facts['est_bits'] / (8 * size):.3f}")
    assert got["quarter"][0] < s0 and got["quarter"][1] > 28
    assert got["four"][0] > s0 and got["four"][1] < 28


# ------------------------------------------------- 7. off is the parent; errors
def _raw_ext7(v, out, height, size, *, mvcost=1, qp=0, max_mb_sad=0, qp_out=None, bits_out=None, cap=0, **fields):
    prm = _lib.TranscodeParams()
    prm.height = height
    prm.qp = qp
    prm.max_mb_sad = max_mb_sad
    ext = _lib.TranscodeExt7(_lib.TranscodeExt6(_lib.TranscodeExt5(_lib.TranscodeExt4(_lib.TranscodeExt3(
        _lib.TranscodeExt2(_lib.TranscodeExt(size, 0)), mvcost)))))
    for k, val in fields.items():
        setattr(ext, k, val)
    if qp_out is not None:
        ext.qp_out = qp_out.ctypes.data_as(C.POINTER(C.c_uint8))
    if bits_out is not None:
        ext.bits_out = bits_out.ctypes.data_as(C.POINTER(C.c_uint32))
    ext.frame_cap = cap
    info = _lib.TranscodeInfo()
    xinfo = _lib.TranscodeExtInfo6(_lib.TranscodeExtInfo5(_lib.TranscodeExtInfo4(_lib.TranscodeExtInfo3(
        _lib.TranscodeExtInfo2(_lib.TranscodeExtInfo(C.sizeof(_lib.TranscodeExtInfo6)))))))
    rc = v._lib.vts_transcode_ex(v._ctx, str(out).encode(), C.byref(prm),
                                 C.cast(C.pointer(ext), C.POINTER(_lib.TranscodeExt)), C.byref(info),
                                 C.cast(C.pointer(xinfo), C.POINTER(_lib.TranscodeExtInfo)))
    return rc, info, xinfo


def test_an_all_zero_168_byte_struct_is_the_112_byte_call(work, tmp_path):
    _require_gpu()
    src = _source(work, "quads")
    files = {}
    for size in (112, 168):
        out = tmp_path / f"s{size}.mp4"
        with scene.VideoScorer(src) as v:
            rc, _, xi = _raw_ext7(v, out, 64, size)
            _lib.check(rc)
        files[size] = out.read_bytes()
        assert xi.frame_words == 8 and xi.est_bits == 0 and xi.qp_lo == xi.qp_hi == 28 and xi.qp_sum == 8 * 28
    assert files[112] == files[168]
    with scene.VideoScorer(src) as v:                                # the keywords' default file
        v.transcode(tmp_path / "base.mp4", height=64, mvcost=True)
    assert files[168] == (tmp_path / "base.mp4").read_bytes()
    # 112 bytes with a bitrate behind them: not read
    with scene.VideoScorer(src) as v:
        rc, _, _ = _raw_ext7(v, tmp_path / "behind.mp4", 64, 112, bitrate_kbps=5, qp_min=77)
        _lib.check(rc)
    assert (tmp_path / "behind.mp4").read_bytes() == files[112]


def test_argument_errors(work, tmp_path):
    _require_gpu()
    src = _source(work, "quads")
    n = 8
    bad = tmp_path / "bad.mp4"
    cases = [
        (dict(bitrate_kbps=-1), "bitrate_kbps"), (dict(bitrate_kbps=1000001), "bitrate_kbps"),
        (dict(bitrate_kbps=100, qp_range=(52, 0)), "qp_min"), (dict(bitrate_kbps=100, qp_range=(0, 52)), "qp_max"),
        (dict(bitrate_kbps=100, qp_range=(-1, 0)), "qp_min"), (dict(bitrate_kbps=100, qp_range=(40, 30)), "qp_min"),
        (dict(qp_range=(10, 0)), "qp_min"), (dict(qp_range=(0, 40)), "qp_max"),
        (dict(bitrate_kbps=100, frame_qp=[28] * n), "frame_qp"),
        (dict(frame_qp=[28] * (n - 1)), "frame_qp_n"), (dict(frame_qp=[28] * (n + 1)), "frame_qp_n"),
        (dict(frame_qp=[28] * (n - 1) + [0]), "frame_qp["), (dict(frame_qp=[52] + [28] * (n - 1)), "frame_qp["),
        (dict(bitrate_kbps=100, qp=-1), "bitrate_kbps"), (dict(frame_qp=[28] * n, qp=-1), "frame_qp"),
        (dict(bitrate_kbps=100, max_mb_sad=-1), "max_mb_sad"), (dict(frame_qp=[28] * n, max_mb_sad=-1), "max_mb_sad"),
        (dict(bitrate_kbps=100, mvcost=False), "mvcost"), (dict(frame_qp=[28] * n, mvcost=False), "mvcost"),
    ]
    for fields, named in cases:
        kw = dict(dict(height=64, mvcost=True), **fields)
        with scene.VideoScorer(src) as v:
            with pytest.raises(VtsegError) as ei:
                v.transcode(bad, **kw)
        assert ei.value.code == _lib.VTS_E_INVALID, fields
        assert named in str(ei.value), (fields, str(ei.value))
        assert not bad.exists()
    # a QP no byte holds is refused before the cast to uint8 could wrap it (300 -> 44) past the library's check
    for qps in ([28] * (n - 1) + [300], np.array([-228] + [28] * (n - 1))):
        with scene.VideoScorer(src) as v:
            with pytest.raises(ValueError, match="frame_qp"):
                v.transcode(bad, height=64, mvcost=True, frame_qp=qps)
        assert not bad.exists()
    # qp_out / bits_out too short: before any encoding
    for which in ("qp_out", "bits_out"):
        with scene.VideoScorer(src) as v:
            buf = np.zeros(n, np.uint8 if which == "qp_out" else np.uint32)
            rc, _, xi = _raw_ext7(v, bad, 64, 168, cap=n - 1, **{which: buf})
            assert rc == _lib.VTS_E_CAPACITY and "frame_cap" in _lib.last_error() and which in _lib.last_error()
            with pytest.raises(VtsegError):
                _lib.check(rc)
            assert xi.frame_words == n and not bad.exists() and (buf == 0).all()
    # both filled with any settings: the features off, the call's QP and no measure
    with scene.VideoScorer(src) as v:
        qps, bits = np.zeros(n, np.uint8), np.full(n, 7, np.uint32)
        rc, _, xi = _raw_ext7(v, tmp_path / "ok.mp4", 64, 168, qp=35, qp_out=qps, bits_out=bits, cap=n)
        _lib.check(rc)
        assert (qps == 35).all() and (bits == 0).all() and xi.qp_sum == 35 * n
