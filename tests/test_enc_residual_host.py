"""The device encoder's residual arithmetic on the CPU (no GPU).

`csrc/enc_residual.h` holds the one copy of what `enc_search` and `enc_intra`
transform, quantise and reconstruct with, and the predicates of the early
P_Skip probe.  The harness (tests/native/enc_residual_host.cpp) exposes the
header's functions; their values are compared, at every QP, with the standard's
formulas restated here in numpy (8.5.10 - 8.5.12 for the inverse path; the
forward transform and quantiser of DESIGN.md §11)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "video-transformer_amd" / "csrc"

QPS = range(52)
N_RANDOM = 2048          # per QP: half over the whole range, half of small amplitude (levels near zero)

CF = np.array([[1, 1, 1, 1], [2, 1, -1, -2], [1, -1, -1, 1], [1, -2, 2, -1]], np.int64)
H4 = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], np.int64)
MF = np.array([[13107, 5243, 8066], [11916, 4660, 7490], [10082, 4194, 6554],
               [9362, 3647, 5825], [8192, 3355, 5243], [7282, 2893, 4559]], np.int64)
NORM_V = np.array([[10, 16, 13], [11, 18, 14], [13, 20, 16], [14, 23, 18], [16, 25, 20], [18, 29, 23]], np.int64)
# position class of (i, j): both even 0, both odd 1, mixed 2
CLASS = np.array([[0 if not (i & 1 or j & 1) else (1 if (i & 1 and j & 1) else 2) for j in range(4)] for i in range(4)])
ZIGZAG = [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15]
QPC = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _p(a, t=C.c_int):
    return a.ctypes.data_as(C.POINTER(t))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("ersh") / "libencresidualhost.so"
    subprocess.run(["g++", "-Og", "-std=c++20", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                    f"-I{CSRC}", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "native" / "enc_residual_host.cpp"),
                    "-o", str(so)], check=True)
    return C.CDLL(str(so))


@pytest.fixture(scope="module")
def blocks():
    """Residual blocks [n, 16] (raster), the same at every QP: the fixed ones first."""
    rng = np.random.default_rng(20260)
    thr = np.zeros(16, int)
    thr[:6] = 9                                            # DC coefficient 54: the first luma level at qp 28
    checker = np.array([255 if (i + j) % 2 == 0 else -255 for i in range(4) for j in range(4)])
    fixed = [np.full(16, 255), np.full(16, -255), checker, -checker, np.zeros(16, int),
             np.full(16, 1), np.full(16, 3), thr]
    wide = rng.integers(-255, 256, (N_RANDOM // 2, 16))
    amp = rng.integers(1, 25, (N_RANDOM // 2, 1))          # around the quantiser's dead zone at most QPs
    small = rng.integers(-amp, amp + 1, (N_RANDOM // 2, 16))
    x = np.concatenate([np.array(fixed), wide, small])
    x = x[: len(x) // 16 * 16]                             # whole macroblocks of 16 (and planes of 4)
    assert x.min() == -255 and x.max() == 255
    return _i32(x)


# ---- the formulas
def np_fwd4(x):
    return CF @ x.reshape(-1, 4, 4).astype(np.int64) @ CF.T


def np_quant(w, mf, qbits, f):
    return np.sign(w) * np.minimum(2047, (np.abs(w) * mf + f) >> qbits)


def np_levels(x, qp):
    """[n, 4, 4] levels (raster) and the transform of residual blocks x."""
    w = np_fwd4(x)
    qbits = 15 + qp // 6
    return np_quant(w, MF[qp % 6][CLASS], qbits, (1 << qbits) // 6), w


def np_chroma_dc(c, qpc):
    c = c.reshape(-1, 4).astype(np.int64)
    fd = np.stack([c[:, 0] + c[:, 1] + c[:, 2] + c[:, 3], c[:, 0] - c[:, 1] + c[:, 2] - c[:, 3],
                   c[:, 0] + c[:, 1] - c[:, 2] - c[:, 3], c[:, 0] - c[:, 1] - c[:, 2] + c[:, 3]], 1)
    qbits = 15 + qpc // 6
    return np_quant(fd, MF[qpc % 6][0], qbits + 1, 2 * ((1 << qbits) // 6))


def np_i16_dc(d, qp):
    h = H4 @ d.reshape(-1, 4, 4).astype(np.int64) @ H4
    qbits = 15 + qp // 6
    return np_quant((h + 1) >> 1, MF[qp % 6][0], qbits + 1, 2 * ((1 << qbits) // 6))


def np_idct4(c, qp, dc_done):
    """8.5.12: scaling (Flat_16) and the inverse transform of [n, 4, 4] levels; dc_done: c[0, 0] is scaled."""
    c = c.astype(np.int64)
    ls = 16 * NORM_V[qp % 6][CLASS]
    d = (c * ls) << (qp // 6 - 4) if qp >= 24 else (c * ls + (1 << (3 - qp // 6))) >> (4 - qp // 6)
    if dc_done:
        d[:, 0, 0] = c[:, 0, 0]

    def half(m):                                           # along the last axis
        e0, e1 = m[..., 0] + m[..., 2], m[..., 0] - m[..., 2]
        e2, e3 = (m[..., 1] >> 1) - m[..., 3], m[..., 1] + (m[..., 3] >> 1)
        return np.stack([e0 + e3, e1 + e2, e1 - e2, e0 - e3], -1)

    h = half(half(d).transpose(0, 2, 1)).transpose(0, 2, 1)
    return (h + 32) >> 6


# ---- the header against them
def code_blocks(lib, x, qp, dc_out):
    n = len(x)
    z, lv, dc, nz = (np.zeros((n, 16), np.int32), np.zeros((n, 16), np.int32), np.zeros(n, np.int32),
                     np.zeros(n, np.int32))
    lib.ersh_code_blocks(n, _p(x), qp, int(dc_out), _p(z), _p(lv), _p(dc), _p(nz))
    return z, lv, dc, nz


def test_transform_and_quantiser_at_every_qp(lib, blocks):
    n = len(blocks)
    w = np.zeros((n, 16), np.int32)
    lib.ersh_fwd4(n, _p(blocks), _p(w))
    assert (w.reshape(-1, 4, 4) == np_fwd4(blocks)).all()
    assert abs(np_fwd4(blocks)).max() == 255 * 36          # the checkerboard: the largest coefficient
    for qp in QPS:
        want, wt = np_levels(blocks, qp)
        z, lv, _, nz = code_blocks(lib, blocks, qp, False)
        assert (z.reshape(-1, 4, 4) == want).all(), qp
        assert (lv == want.reshape(n, 16)[:, ZIGZAG]).all(), qp
        assert (nz.astype(bool) == (want != 0).any((1, 2))).all(), qp
        # the DC term held out (chroma; Intra16x16 luma): 15 AC levels from index 0, the coefficient apart
        z, lv, dc, nz = code_blocks(lib, blocks, qp, True)
        ac = want.copy()
        ac[:, 0, 0] = 0
        assert (z.reshape(-1, 4, 4) == ac).all(), qp
        assert (lv[:, :15] == want.reshape(n, 16)[:, ZIGZAG[1:]]).all() and (lv[:, 15] == 0).all(), qp
        assert (dc == wt[:, 0, 0]).all(), qp
        assert (nz.astype(bool) == (ac != 0).any((1, 2))).all(), qp
    # the largest level there is, all +255 at qp 0: 4080 * 13107 >> 15; an 8-bit residual never reaches the clamp
    assert abs(np_levels(blocks, 0)[0]).max() == 1632


def test_dc_quantisers_at_every_qp(lib, blocks):
    dc = _i32(np_fwd4(blocks)[:, 0, 0])                    # the blocks' DC coefficients: planes of 4, macroblocks of 16
    n4, n16 = len(dc) // 4, len(dc) // 16
    for qp in QPS:
        lv, nz = np.zeros((n4, 4), np.int32), np.zeros(n4, np.int32)
        lib.ersh_chroma_dc(n4, _p(dc), qp, _p(lv), _p(nz))
        want = np_chroma_dc(dc, qp)
        assert (lv == want).all(), qp
        assert (nz.astype(bool) == (want != 0).any(1)).all(), qp
        lv = np.zeros((n16, 16), np.int32)
        lib.ersh_i16_dc(n16, _p(dc), qp, _p(lv))
        assert (lv.reshape(-1, 4, 4) == np_i16_dc(dc, qp)).all(), qp


def test_probe_predicates_agree_with_the_quantiser(lib, blocks):
    """all_zero_block is true exactly when every level the header codes for the block is zero, and
    all_zero_chroma_dc exactly when every chroma DC level is: what the probe skips, the residual stage codes
    nothing for."""
    n = len(blocks)
    dcs = _i32(np_fwd4(blocks)[:, 0, 0])
    seen = set()
    for qp in QPS:
        for dc_out in (False, True):
            zero, dc = np.zeros(n, np.int32), np.zeros(n, np.int32)
            lib.ersh_all_zero(n, _p(blocks), qp, int(dc_out), _p(zero), _p(dc))
            z, lv, dcw, nz = code_blocks(lib, blocks, qp, dc_out)
            assert (zero.astype(bool) == ~(z != 0).any(1)).all(), (qp, dc_out)
            assert (zero.astype(bool) == ~(lv != 0).any(1)).all(), (qp, dc_out)
            assert (zero != nz).all(), (qp, dc_out)
            if dc_out:
                assert (dc == dcs).all(), qp
            seen |= set(zero.tolist())
        zero = np.zeros(n // 4, np.int32)
        lib.ersh_all_zero_chroma_dc(n // 4, _p(dcs), qp, _p(zero))
        lv, nz = np.zeros((n // 4, 4), np.int32), np.zeros(n // 4, np.int32)
        lib.ersh_chroma_dc(n // 4, _p(dcs), qp, _p(lv), _p(nz))
        assert (zero.astype(bool) == ~(lv != 0).any(1)).all(), qp
        seen |= set(zero.tolist())
    assert seen == {0, 1}                                  # both answers occur


def _u8(a):
    return np.ascontiguousarray(a, np.uint8)


def test_packed_rows(lib, blocks):
    rng = np.random.default_rng(7)
    n = 512
    src, pred = _u8(rng.integers(0, 256, (n, 16))), _u8(rng.integers(0, 256, (n, 16)))
    src[0], pred[0], src[1], pred[1] = 255, 0, 0, 255
    x = np.zeros((n, 16), np.int32)
    lib.ersh_diff(n, _p(src, C.c_uint8), _p(pred, C.c_uint8), _p(x))
    assert (x == src.astype(int) - pred.astype(int)).all()


def test_reconstruction_is_the_decoders_at_every_qp(lib, blocks):
    """prediction + the 8.5.12 residual of the dequantised levels, clipped: inter luma, chroma (DC through
    8.5.11) and Intra16x16 luma (DC through 8.5.10)."""
    rng = np.random.default_rng(11)
    n = len(blocks)
    pred = _u8(rng.integers(0, 256, (n, 16)))
    pred[:4] = np.array([0, 255, 0, 255])[:, None]         # the clip, against the largest residuals
    rows = _u8(pred[:, ::4])                               # Intra16x16: one prediction value per block row
    out = np.zeros((n, 16), np.uint8)
    for qp in QPS:
        z, _, _, _ = code_blocks(lib, blocks, qp, False)
        lib.ersh_recon_inter(n, _p(z), qp, _p(pred, C.c_uint8), _p(out, C.c_uint8))
        want = np.clip(pred.reshape(-1, 4, 4) + np_idct4(z.reshape(-1, 4, 4), qp, False), 0, 255)
        assert (out.reshape(-1, 4, 4) == want).all(), qp

        z, _, dcw, _ = code_blocks(lib, blocks, qp, True)
        # chroma at this QP as QPc: planes of 4 blocks; 8.5.11.1 f = the 2x2 Hadamard of the levels, 8.5.11.2
        # dcC = ((f LevelScale(qPc % 6, 0, 0)) << (qPc / 6)) >> 5
        dcl = _i32(np_chroma_dc(dcw, qp))
        f = np_chroma_dc_f(dcl)
        dcc = ((f * 16 * NORM_V[qp % 6][0]) << (qp // 6)) >> 5
        for ac in (1, 0):
            lib.ersh_recon_chroma(n // 4, _p(dcl), _p(z), ac, qp, _p(pred, C.c_uint8), _p(out, C.c_uint8))
            c = z.reshape(-1, 4, 4).astype(np.int64) * ac
            c[:, 0, 0] = dcc.reshape(-1)
            want = np.clip(pred.reshape(-1, 4, 4) + np_idct4(c, qp, True), 0, 255)
            assert (out.reshape(-1, 4, 4) == want).all(), (qp, ac)
        # Intra16x16 luma: macroblocks of 16 blocks; 8.5.10 f = H c H, dcY = (f LS(0, 0)) << (qP / 6 - 6) from
        # qP 36, else (f LS(0, 0) + 2^(5 - qP / 6)) >> (6 - qP / 6)
        ydl = _i32(np_i16_dc(dcw, qp))
        f = H4 @ ydl.astype(np.int64) @ H4
        ls = 16 * NORM_V[qp % 6][0]
        dcy = (f * ls) << (qp // 6 - 6) if qp >= 36 else (f * ls + (1 << (5 - qp // 6))) >> (6 - qp // 6)
        for ac in (1, 0):
            lib.ersh_recon_i16(n // 16, _p(ydl), _p(z), ac, qp, _p(rows, C.c_uint8), _p(out, C.c_uint8))
            c = z.reshape(-1, 4, 4).astype(np.int64) * ac
            c[:, 0, 0] = dcy.reshape(-1)
            flat = np.repeat(rows.astype(int), 4, 1).reshape(-1, 4, 4)
            want = np.clip(flat + np_idct4(c, qp, True), 0, 255)
            assert (out.reshape(-1, 4, 4) == want).all(), (qp, ac)


def np_chroma_dc_f(dcl):
    c = dcl.reshape(-1, 4).astype(np.int64)
    return np.stack([c[:, 0] + c[:, 1] + c[:, 2] + c[:, 3], c[:, 0] - c[:, 1] + c[:, 2] - c[:, 3],
                     c[:, 0] + c[:, 1] - c[:, 2] - c[:, 3], c[:, 0] - c[:, 1] - c[:, 2] + c[:, 3]], 1)


def test_thresholds_at_qp_28(lib):
    """The blocks of test_probe_thresholds_at_qp_28 (test_enc_rate_host.py) through the quantiser itself: qbits
    19, MF(0, 0) 8192, a DC coefficient is coded from |w| >= 54; the chroma DC of four flat +3 blocks is 192 at
    qbits + 1, a level."""
    thr = np.zeros(16, int)
    thr[:6] = 9
    x = _i32([[1] * 16, [3] * 16, thr, [0] * 16])
    z, lv, _, nz = code_blocks(lib, x, 28, False)
    assert nz.tolist() == [0, 0, 1, 0] and z[2, 0] == 1 and lv[2, 0] == 1
    assert QPC[28] == 28
    c = _i32([[16] * 4, [48] * 4, [0] * 4])
    lv, nz = np.zeros((3, 4), np.int32), np.zeros(3, np.int32)
    lib.ersh_chroma_dc(3, _p(c), QPC[28], _p(lv), _p(nz))
    assert nz.tolist() == [0, 1, 0] and lv[1].tolist() == [1, 0, 0, 0]
