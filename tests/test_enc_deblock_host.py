"""The encoder's in-loop deblocking decisions on the CPU (no GPU).

`csrc/enc_deblock.h` holds what the `enc_deblock` kernel decides with: bS from
the command words, coded_block_pattern and levels of a level, indexA / indexB,
and the line filter (the decoder's `full::filter_line`).  The harness
(tests/native/enc_deblock_host.cpp) filters seeded random macroblock rows
twice: a scalar walk over the header's functions in the kernel's edge order,
and the general decoder's `full::deblock_mb` (recon_full.h) over MbRecs that
say the same thing, with disable_deblocking_filter_idc = 2 and one slice per
macroblock row.  Luma and chroma must be byte-equal."""
from __future__ import annotations

import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "video-transformer_amd" / "csrc"

PCM = 0x80008000
INTRA = 0x80000000
WIDTHS = (1, 2, 10)
QPS = (12, 16, 28, 40, 51)
OFFSETS = (-6, 0, 2, 6)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("edh") / "libencdeblockhost.so"
    subprocess.run(["g++", "-Og", "-std=c++20", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                    f"-I{CSRC}", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "native" / "enc_deblock_host.cpp"),
                    "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    args = [C.c_int] * 5 + [C.c_void_p] * 4
    lib.edh_walk.argtypes = args
    lib.edh_walk.restype = C.c_int64
    lib.edh_ref.argtypes = args
    lib.edh_ref.restype = None

    def run(mbw, mbh, qp, a, b, cmd, cbp, coef, pic):
        walk, ref = pic.copy(), pic.copy()
        ptrs = (cmd.ctypes.data, cbp.ctypes.data, coef.ctypes.data)
        n = lib.edh_walk(mbw, mbh, qp, a, b, *ptrs, walk.ctypes.data)
        lib.edh_ref(mbw, mbh, qp, a, b, *ptrs, ref.ctypes.data)
        return walk, ref, n
    return run


def _cmd_of(mvx, mvy):
    return (mvx & 0xffff) | ((mvy & 0xffff) << 16)


def _picture(rng, mbw, mbh):
    """Random macroblocks of every kind the encoder's levels hold, and
    samples smooth enough for the filter to switch on at most QPs."""
    nmb = mbw * mbh
    cmd = np.zeros(nmb, np.uint32)
    cbp = np.zeros(nmb, np.uint8)
    coef = rng.integers(-3, 4, (nmb, 384)).astype(np.int16)   # stale levels where nothing is coded
    base = rng.integers(-8, 9, 2)
    for a in range(nmb):
        kind = rng.integers(0, 6)
        if kind == 0:
            cmd[a] = PCM
        elif kind == 1:                                       # Intra16x16: modes and its own cbp in the word
            cmd[a] = INTRA | int(rng.integers(0, 1 << 10))
            cbp[a] = rng.integers(0, 48)
        elif kind == 2:                                       # P_Skip
            cmd[a] = _cmd_of(0, 0)
        else:                                                 # inter: vectors 0..8 quarter samples apart
            d = rng.integers(0, 9, 2) * rng.choice([-1, 1], 2)
            cmd[a] = _cmd_of(int(base[0] + d[0]), int(base[1] + d[1]))
            if kind >= 4:                                     # ... with coded blocks, some of them all zero
                cbp[a] = rng.integers(1, 48)
                keep = rng.random((16, 1)) < 0.4
                lv = coef[a, :256].reshape(16, 16) * keep
                lv *= rng.random((16, 16)) < 0.2
                coef[a, :256] = lv.reshape(-1)
    H, W = 16 * mbh, 16 * mbw
    amp, noise = rng.choice([0, 1, 3, 8, 30]), rng.choice([0, 1, 2])
    y = 128 + 40 * np.sin(np.arange(W) / 20.0)[None, :] + 30 * np.cos(np.arange(H * 3 // 2) / 15.0)[:, None]
    steps = rng.integers(-amp, amp + 1, (H * 3 // 2, W // 4)).repeat(4, axis=1)   # block edges
    pic = np.clip(y + steps + rng.integers(-noise, noise + 1, y.shape), 0, 255).astype(np.uint8)
    return cmd, cbp, coef, np.ascontiguousarray(pic)


@pytest.mark.parametrize("mbw", WIDTHS)
def test_walk_of_the_shared_header_equals_deblock_mb(harness, mbw):
    rng = np.random.default_rng(1000 + mbw)
    filtered = {}
    key = {(28, 0, 0), (51, 6, 6), (28, -6, -6), (12, 2, 2), (40, 0, 0), (12, 0, 0), (12, -6, 0)}
    for qp, a, b in itertools.product(QPS, OFFSETS, OFFSETS):
        for _ in range(40 if (qp, a, b) in key else 4):   # the settings asserted on below get more pictures
            cmd, cbp, coef, pic = _picture(rng, mbw, 1)
            walk, ref, n = harness(mbw, 1, qp, a, b, cmd, cbp, coef, pic)
            assert np.array_equal(walk, ref), f"mbw {mbw} qp {qp} offsets ({a}, {b}): the walk differs from deblock_mb"
            if n == 0:
                assert np.array_equal(walk, pic)
            filtered[(qp, a, b)] = filtered.get((qp, a, b), 0) + n
    # the comparison is not vacuous: the filter ran wherever alpha' can be non-zero ...
    assert filtered[(28, 0, 0)] > 0 and filtered[(51, 6, 6)] > 0 and filtered[(28, -6, -6)] > 0
    assert filtered[(12, 2, 2)] > 0 and filtered[(40, 0, 0)] > 0
    # ... and nowhere below indexA 16 (qp 12, offsets 0: alpha' = 0)
    assert filtered[(12, 0, 0)] == 0 and filtered[(12, -6, 0)] == 0


def test_rows_do_not_touch_each_other(harness):
    """A two-row picture: each row filtered alone gives the same samples, and
    the samples either side of the row boundary keep the walk equal to
    deblock_mb (which skips the top edge of the second slice)."""
    rng = np.random.default_rng(77)
    mbw = 10
    cmd, cbp, coef, pic = _picture(rng, mbw, 2)
    walk, ref, n = harness(mbw, 2, 28, 0, 0, cmd, cbp, coef, pic)
    assert n > 0 and np.array_equal(walk, ref)
    W = 16 * mbw
    for row in range(2):
        one = np.concatenate([pic[16 * row:16 * row + 16], pic[32 + 8 * row:32 + 8 * row + 8]])
        sl = slice(row * mbw, (row + 1) * mbw)
        w1, r1, _ = harness(mbw, 1, 28, 0, 0, cmd[sl].copy(), cbp[sl].copy(), coef[sl].copy(),
                            np.ascontiguousarray(one))
        assert np.array_equal(w1, r1)
        assert np.array_equal(w1[:16], walk[16 * row:16 * row + 16])
        assert np.array_equal(w1[16:], walk[32 + 8 * row:32 + 8 * row + 8])
        assert w1.shape == (24, W)
