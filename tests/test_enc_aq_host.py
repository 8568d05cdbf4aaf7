"""Adaptive quantisation of the device encoder on the CPU (csrc/enc_aq.h through
tests/native/enc_aq_host.cpp; DESIGN.md §11 "Adaptive quantisation").

1. The law against a Python big-integer restatement: E = 0 and 1, every power
   of two and its neighbours up to the largest E that 8-bit samples give,
   random macroblocks, each clamp, strength_q8 1 (all zero) and 768.
2. The running-QP rule (7.4.5) and the CABAC ctxIdxInc of mb_qp_delta's first
   bin on hand-made rows, the first macroblock of a row included.
3. The designed source of the GPU test: its offsets at strength 1.0 take both
   signs, hit -aq_max and take at least four distinct values.
4. Rows with a different QP on every macroblock (P_Skip, inter with pattern 0
   and with a pattern, Intra16x16, I_NxN, I_PCM), written as CAVLC and as CABAC
   by the shared writers with the in-loop filter on: decoded by the general
   oracle they are the harness's reconstruction.
5. The stand-alone driver under the sanitizers."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

from test_enc_part_host import FLAGS, NATIVE, SRCS, _parameter_sets, _pictures, _rows

CENTRE = 3693
E_MAX = 4161600 + 2 * 1040400      # half the samples 0 and half 255 in each plane


# ------------------------------------------------ the law, restated in Python
def energy(mb_y, mb_u, mb_v) -> int:
    """E of one macroblock from its 256 luma and 2 x 64 chroma samples (Python integers)."""
    e = 0
    for plane, shift in ((mb_y, 8), (mb_u, 6), (mb_v, 6)):
        v = [int(x) for x in np.asarray(plane).reshape(-1)]
        s1, s2 = sum(v), sum(x * x for x in v)
        e += s2 - ((s1 * s1) >> shift)
    return e


def log2_q8(e: int) -> int:
    e = max(e, 1)
    k = e.bit_length() - 1
    return 256 * k + (((e - (1 << k)) << 8) >> k)


def offset(e: int, strength_q8: int, aq_max: int) -> int:
    x = strength_q8 * (log2_q8(e) - CENTRE)
    r = (abs(x) + 32768) >> 16
    r = -r if x < 0 else r
    return max(-aq_max, min(aq_max, r))


def picture_offsets(pic: np.ndarray, strength_q8: int = 256, aq_max: int = 8) -> np.ndarray:
    """The offsets [mbh, mbw] of one coded NV12 picture [ch * 3 / 2, cw] by the Python law."""
    ch, cw = pic.shape[0] * 2 // 3, pic.shape[1]
    out = np.zeros((ch // 16, cw // 16), np.int8)
    for my in range(ch // 16):
        for mx in range(cw // 16):
            uv = pic[ch + 8 * my:ch + 8 * my + 8, 16 * mx:16 * mx + 16]
            out[my, mx] = offset(energy(pic[16 * my:16 * my + 16, 16 * mx:16 * mx + 16], uv[:, 0::2], uv[:, 1::2]),
                                 strength_q8, aq_max)
    return out


def designed_frames(F: int = 6, W: int = 96, H: int = 64, seed: int = 5) -> np.ndarray:
    """Display-size NV12 frames (samples >= 1) of a still background in three thirds of 2 x 4 macroblocks, the
    left one constant, the middle one a ramp (a level a sample) plus noise of -2 .. 2, the right one uniform
    noise 1 .. 255 in luma and chroma; over each third a 16 x 16 block of fine texture (-8 .. 8 around 110) moves
    3 samples a frame (one block cannot cross 96 samples in 6 frames, so each third has its own, on its own
    rows; the texture is faint, so that a macroblock of the middle third stays below the centre with it)."""
    rng = np.random.default_rng(seed)
    third = W // 3
    y = np.zeros((H, W), np.int64)
    y[:, :third] = 90
    y[:, third:2 * third] = 100 + np.arange(third)[None, :] + rng.integers(-2, 3, (H, third))
    y[:, 2 * third:] = rng.integers(1, 256, (H, W - 2 * third))
    uv = np.full((H // 2, W), 128, np.int64)
    uv[:, 2 * third:] = rng.integers(1, 256, (H // 2, W - 2 * third))
    tex = 110 + rng.integers(-8, 9, (16, 16))
    fr = np.zeros((F, H * 3 // 2, W), np.uint8)
    for f in range(F):
        pic = y.copy()
        for t in range(3):
            x0, y0 = t * third + 1 + 3 * f, 4 + 16 * t
            pic[y0:y0 + 16, x0:x0 + 16] = tex
        fr[f, :H] = np.clip(pic, 1, 255)
        fr[f, H:] = uv
    return fr


# ------------------------------------------------------------------ harness
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("eaqh") / "libencaqhost.so"
    subprocess.run(["g++", "-Og", "-fPIC", "-shared", *FLAGS, str(NATIVE / "enc_aq_host.cpp"), "-o", str(so)], check=True)
    return load(so)


def load(so):
    L = C.CDLL(str(so))
    L.eaqh_energy.argtypes = [C.c_uint32] * 6
    L.eaqh_energy.restype = C.c_uint32
    L.eaqh_log2_q8.argtypes = [C.c_uint32]
    L.eaqh_offset.argtypes = [C.c_uint32, C.c_int, C.c_int]
    L.eaqh_qp_mb.argtypes = [C.c_int] * 4
    L.eaqh_se_bits.argtypes = [C.c_int]
    L.eaqh_picture.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.eaqh_picture.restype = None
    L.eaqh_row.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 7
    L.eaqh_row.restype = None
    return L


def harness_offsets(L, pic: np.ndarray, strength_q8: int = 256, aq_max: int = 8) -> np.ndarray:
    pic = np.ascontiguousarray(pic, np.uint8)
    ch, cw = pic.shape[0] * 2 // 3, pic.shape[1]
    out = np.zeros((ch // 16, cw // 16), np.int8)
    L.eaqh_picture(pic.ctypes.data, cw, ch, strength_q8, aq_max, out.ctypes.data)
    return out


# --------------------------------------------------------------- 1. the law
def test_log2_and_offset_at_the_powers_of_two_and_their_neighbours(lib):
    es = {0, 1, 2, 3, E_MAX - 1, E_MAX, E_MAX + 1}
    k = 1
    while (1 << k) <= 2 * E_MAX:
        es |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
        k += 1
    for e in sorted(es):
        assert lib.eaqh_log2_q8(e) == log2_q8(e), e
        for s in (1, 128, 256, 768):
            for m in (1, 8, 10):
                assert lib.eaqh_offset(e, s, m) == offset(e, s, m), (e, s, m)
    assert log2_q8(0) == log2_q8(1) == 0 and log2_q8(2) == 256 and log2_q8(3) == 384 and log2_q8(1 << 22) == 22 * 256
    # the two consequences the GPU tests rely on
    assert lib.eaqh_offset(0, 256, 8) == -8 and lib.eaqh_offset(0, 256, 10) == -10
    assert all(lib.eaqh_offset(e, 1, 10) == 0 for e in sorted(es))


def test_each_clamp_and_the_rounding(lib):
    # L - 3693 = 7 at E = 20480 + ...: walk E over a stretch where the unclamped value crosses halves
    for s in (256, 768):
        seen = set()
        for e in range(1, 1 << 16, 7):
            got = lib.eaqh_offset(e, s, 10)
            assert got == offset(e, s, 10)
            seen.add(got)
        assert min(seen) == -10 and len(seen) >= 10
    assert lib.eaqh_offset(E_MAX, 768, 10) == 10 == offset(E_MAX, 768, 10)       # the upper clamp
    assert lib.eaqh_offset(E_MAX, 256, 3) == 3 and lib.eaqh_offset(0, 256, 3) == -3
    # round half away from zero, both signs: strength 128 makes x / 65536 = (L - 3693) / 512
    assert offset(_e_with_log(CENTRE + 256), 128, 10) == 1 and offset(_e_with_log(CENTRE - 256), 128, 10) == -1
    assert offset(_e_with_log(CENTRE + 255), 128, 10) == 0 and offset(_e_with_log(CENTRE - 255), 128, 10) == 0
    for t in (CENTRE + 256, CENTRE - 256, CENTRE + 255, CENTRE - 255):
        assert lib.eaqh_offset(_e_with_log(t), 128, 10) == offset(_e_with_log(t), 128, 10)
    assert lib.eaqh_qp_mb(28, -8, 1, 51) == 20 and lib.eaqh_qp_mb(28, -8, 24, 30) == 24 and lib.eaqh_qp_mb(28, 7, 24, 30) == 30
    assert lib.eaqh_qp_mb(3, -8, 1, 51) == 1 and lib.eaqh_qp_mb(49, 8, 1, 51) == 51
    assert [lib.eaqh_se_bits(v) for v in (0, 1, -1, 2, -2, 3, -3, 4, 20, -20)] == [1, 3, 3, 5, 5, 5, 5, 7, 11, 11]


def _e_with_log(target: int) -> int:
    """An E whose log2 in Q8 is exactly `target` (the mantissa is exact where 2^k >= 256)."""
    k, m = target // 256, target % 256
    e = (1 << k) + ((m << k) >> 8)
    assert k >= 8 and log2_q8(e) == target
    return e


def test_random_macroblocks_and_pictures(lib):
    rng = np.random.default_rng(9)
    for i in range(60):
        amp = int(rng.integers(0, 256))
        y, u, v = (rng.integers(0, amp + 1, n) for n in (256, 64, 64))
        if i == 0:       # the largest E: half the samples 0 and half 255
            y, u, v = (np.repeat([0, 255], n // 2) for n in (256, 64, 64))
        e = energy(y, u, v)
        sums = [int(f(p.astype(np.int64))) for p in (y, u, v) for f in (np.sum, lambda a: np.sum(a * a))]
        assert lib.eaqh_energy(*sums) == e
        if i == 0:
            assert e == E_MAX
    for mbw, mbh in ((1, 1), (5, 3)):
        pic = rng.integers(0, 256, (mbh * 24, mbw * 16)).astype(np.uint8)
        pic[:16, :16] = 77                              # a constant macroblock (its chroma too)
        pic[mbh * 16:mbh * 16 + 8, :16] = 200
        for s, m in ((256, 8), (768, 10), (1, 8), (90, 2)):
            got = harness_offsets(lib, pic, s, m)
            assert np.array_equal(got, picture_offsets(pic, s, m)), (mbw, s, m)
            assert got[0, 0] == (-m if s >= 256 else got[0, 0])
            if s == 1:
                assert not got.any()


# ----------------------------------------------------- 2. the running-QP rule
def _row(lib, slice_qp, mbs):
    """mbs: (kind, cbp, qp) with kind 0 I_PCM, 1 Intra16x16, 2 anything else."""
    n = len(mbs)
    kind, cbp, qp = (np.array([m[i] for m in mbs], np.uint8) for i in range(3))
    delta, qpy = np.zeros(n, np.int32), np.zeros(n, np.int32)
    sent, inc = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    lib.eaqh_row(n, slice_qp, kind.ctypes.data, cbp.ctypes.data, qp.ctypes.data, delta.ctypes.data, sent.ctypes.data,
                 inc.ctypes.data, qpy.ctypes.data)
    return delta.tolist(), sent.tolist(), inc.tolist(), qpy.tolist()


def test_running_qp_and_ctx_inc_on_hand_made_rows(lib):
    # the first macroblock of a row predicts from SliceQPY, with ctxIdxInc 0
    d, s, i, q = _row(lib, 28, [(1, 0, 20)])
    assert (d, s, i, q) == ([-8], [1], [0], [20])
    d, s, i, q = _row(lib, 28, [(2, 0, 20)])             # P_Skip / pattern 0 first: nothing sent, QP_Y is the slice's
    assert (d, s, i, q) == ([0], [0], [0], [28])
    d, s, i, q = _row(lib, 28, [(0, 0, 20)])             # I_PCM first: qP 0 for the filter
    assert (d, s, i, q) == ([0], [0], [0], [0])
    # Intra16x16 without a pattern sends; pattern-0 inter, P_Skip and I_PCM leave the running QP; the
    # macroblock behind them predicts from the last one that sent; ctxIdxInc follows the previous macroblock only
    mbs = [(2, 15, 30), (2, 0, 22), (2, 47, 30), (0, 0, 36), (1, 0, 36), (1, 0, 36), (2, 1, 25), (2, 0, 40), (2, 16, 25)]
    d, s, i, q = _row(lib, 26, mbs)
    assert d == [4, 0, 0, 0, 6, 0, -11, 0, 0]
    assert s == [1, 0, 1, 0, 1, 1, 1, 0, 1]
    assert i == [0, 1, 0, 0, 0, 1, 0, 1, 0]
    assert q == [30, 30, 30, 0, 36, 36, 25, 25, 25]
    # |offset| <= 10 on both sides of a picture's QP: |delta| <= 20
    d, _, _, _ = _row(lib, 30, [(1, 0, 40), (1, 0, 20), (1, 0, 40)])
    assert d == [10, -20, 20]


# --------------------------------------------------- 3. the designed source
def test_designed_source_offsets_take_both_signs_and_hit_the_clamp(lib):
    fr = designed_frames()
    assert fr.min() >= 1
    for f in (0, 5):
        off = harness_offsets(lib, fr[f])
        assert np.array_equal(off, picture_offsets(fr[f]))
        assert off.min() == -8 and off.max() > 0 and len(set(off.reshape(-1).tolist())) >= 4
        assert (off[:, 2:4] < 0).all() and (off[:, 4:] > 0).all()      # the middle third below, the right third above
    # each third has 8 macroblocks
    assert harness_offsets(lib, fr[0]).shape == (4, 6)


# ------------------------------------- 4. rows with a QP per macroblock
@pytest.fixture(scope="module")
def rows_lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("eaqr") / "libencaqrows.so"
    subprocess.run(["g++", "-Og", "-fPIC", "-shared", *FLAGS, str(NATIVE / "enc_aq_rows_host.cpp"), *map(str, SRCS),
                    "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.eaqr_encode.argtypes = [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 9
    L.eaqr_encode.restype = None
    L.eaqr_write.argtypes = [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int64, C.c_void_p]
    L.eaqr_write.restype = C.c_int64
    L.ei4h_sps_pps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _write_rows(lib, mbw, mbh, npic, sq, qp, dbk, cabac, src, r):
    n = npic * mbh * mbw
    out = np.zeros(n * 9024 + 1024, np.uint8)
    sizes = np.zeros(npic, np.int64)
    got = lib.eaqr_write(mbw, mbh, npic, sq.ctypes.data, qp.ctypes.data, dbk, cabac, r["src"].ctypes.data if src is None
                         else src.ctypes.data, r["cmd"].ctypes.data, r["cbp"].ctypes.data, r["coef"].ctypes.data,
                         r["modes"].ctypes.data, r["mv4"].ctypes.data, out.ctypes.data, out.size, sizes.ctypes.data)
    assert got > 0
    at, samples = 0, []
    for s in sizes:
        samples.append(out[at:at + s].tobytes())
        at += int(s)
    return samples


@pytest.mark.parametrize("dbk", [0, 1])
@pytest.mark.parametrize("sq", [(28, 28, 28), (12, 40, 26)])
@pytest.mark.parametrize("mbw", [1, 2, 12])
def test_rows_with_a_qp_per_macroblock_decode_to_the_harness_reconstruction(rows_lib, tmp_path, mbw, sq, dbk):
    """Every macroblock of every row has its own QP, up to 10 either side of the slice's; the rows hold every
    kind (_rows: I_PCM, Intra16x16, I_NxN, P_Skip, inter with and without a pattern, the partition shapes)."""
    import oracle
    lib = rows_lib
    rng = np.random.default_rng(77 * mbw + sq[1])
    mbh, npic = 2, 3
    src = _pictures(rng, mbw, mbh, npic)
    kind, vec, label = _rows(rng, mbw, mbh, npic)
    n = npic * mbh * mbw
    sqa = np.array(sq, np.int32)
    qp = np.clip(sqa[:, None, None] + rng.integers(-10, 11, (npic, mbh, mbw)), 1, 51).astype(np.uint8)
    if mbw == 12:                                   # a different QP on every macroblock of a row
        qp[1, 0] = np.clip(sq[1] + np.array([-10, 10, -9, 9, -8, 8, -7, 7, -6, 6, -5, 5]), 1, 51)
        assert len(set(qp[1, 0].tolist())) == 12
    r = dict(cmd=np.zeros(n, np.uint32), cbp=np.zeros(n, np.uint8), coef=np.zeros((n, 384), np.int16),
             modes=np.zeros(n, np.uint64), mv4=np.zeros((n, 4), np.uint32), rec=np.zeros_like(src))
    lib.eaqr_encode(mbw, mbh, npic, sqa.ctypes.data, qp.ctypes.data, dbk, src.ctypes.data, kind.ctypes.data, vec.ctypes.data,
                    r["cmd"].ctypes.data, r["cbp"].ctypes.data, r["coef"].ctypes.data, r["modes"].ctypes.data,
                    r["mv4"].ctypes.data, r["rec"].ctypes.data)
    if mbw == 12:
        assert {"pcm", "i16", "i4", "skip", "p16"} <= set(label[1, 0].tolist())
        cbp_all = r["cbp"].reshape(npic, mbh, mbw)
        nores = np.isin(label, ["p16x8_nores", "p8x8_nores"])             # inter with pattern 0 and vectors
        assert nores.any() and (cbp_all[nores] == 0).all()
        assert (cbp_all[np.isin(label, ["p16", "p16x8", "p8x16", "p8x8"])] != 0).any()     # and with a pattern
    by = {}
    for cabac in (0, 1, 2):
        samples = _write_rows(lib, mbw, mbh, npic, sqa, qp, dbk, cabac, src, r)
        sps, pps = _parameter_sets(lib, mbw, mbh, cabac)
        path = tmp_path / f"c{cabac}.mp4"
        oracle.write_mp4(path, sps, pps, samples, list(range(npic)), [0] * npic, 30, 16 * mbw, 16 * mbh)
        frames, _ = oracle.decode_full(path)
        assert frames.shape == r["rec"].shape
        bad = [i for i in range(npic) if not np.array_equal(frames[i], r["rec"][i])]
        assert bad == [], f"cabac {cabac}: the oracle's pictures differ from the harness's at {bad}"
        by[cabac] = b"".join(samples)
    assert by[1] == by[2]
    # the check is not vacuous: the same data written as if every macroblock had the slice's QP (mb_qp_delta 0)
    # is another stream
    flat = np.broadcast_to(sqa[:, None, None], qp.shape).astype(np.uint8).copy()
    if not np.array_equal(flat, qp):
        assert b"".join(_write_rows(lib, mbw, mbh, npic, sqa, flat, dbk, 0, src, r)) != by[0]


# ----------------------------------------------------------- 5. sanitizers
def test_sanitizer_run_of_the_stand_alone_driver(tmp_path):
    """enc_aq_main.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, run as a program."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtimes")       # an empty program does not link with them
    exe = tmp_path / "enc_aq_main"
    r = subprocess.run(["g++", "-O1", "-g", *san, *FLAGS, str(NATIVE / "enc_aq_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]                       # with the runtimes there, an error is an error
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "enc_aq_main: ok" in run.stdout, run.stdout[-1000:] + run.stderr[-3000:]
