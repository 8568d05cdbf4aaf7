"""The device encoder's inter partitions on the CPU (no GPU).

`csrc/enc_part.h` holds what `enc_search<.., PT = true>` decides with and what
both slice writers and `enc_deblock` read the quadrant vectors by; the harness
(tests/native/enc_part_host.cpp) exposes it and the writers' `mb_p_part`.

  predictors: every block of every shape against the restatement of 8.4.1.3
              under one-row slices below, for each kind of left macroblock;
  decision:   seeded per-candidate quadrant SADs through the nine blocks' keys
              and the shape rule, with exact ties; the canonical form for every
              pattern of equal and unequal vectors;
  rows:       seeded macroblock rows mixing the three partitioned shapes with
              P_Skip, P_L0_16x16, Intra16x16, I_NxN and I_PCM, with negative and
              quarter-sample vectors past all four picture edges, written as
              CAVLC and as CABAC (directly and through BinRing, the same bytes),
              with and without the deblocking filter: the CPU oracle decodes
              both to the harness's reconstruction;
  counts:     what `enc_cavlc.h` counts is what it writes;
  bS:         every inner and left edge line over pairs of vector sets against
              a restatement of the motion part of 8.7.2.1.
"""
from __future__ import annotations

import ctypes as C
import itertools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "video-transformer_amd" / "csrc"
NATIVE = ROOT / "tests" / "native"
sys.path.insert(0, str(ROOT / "oracle"))

PCM = 0x80008000
NONE = 0xFFFFFFFFFFFFFFFF
SRCS = [CSRC / f for f in ("synth.cpp", "synth_full.cpp", "mp4.cpp", "plan.cpp")]
FLAGS = ["-std=c++20", "-Wno-unknown-pragmas", "-pthread", f"-I{CSRC}", f"-I{ROOT / 'include'}", f"-I{NATIVE}"]
# the quadrants of the nine blocks; a shape's blocks in syntax order
BLOCKS = [(0, 1, 2, 3), (0, 1), (2, 3), (0, 2), (1, 3), (0,), (1,), (2,), (3,)]
SHAPE_BLOCKS = [(0,), (1, 2), (3, 4), (5, 6, 7, 8)]
SHAPE_BITS = [1, 3, 3, 5 + 4]          # ue(v) of mb_type 0..3 in a P slice; P_8x8 with four sub_mb_type of 1 bit


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("eph") / "libencparthost.so"
    subprocess.run(["g++", "-Og", "-fPIC", "-shared", *FLAGS, str(NATIVE / "enc_part_host.cpp"),
                    *map(str, SRCS), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.eph_pred.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.eph_pred.restype = None
    L.eph_canonical.argtypes = [C.c_void_p]
    L.eph_frac_class.argtypes = [C.c_void_p]
    L.eph_part_cmd.argtypes = [C.c_int]
    L.eph_part_cmd.restype = C.c_uint32
    L.eph_is_part_cmd.argtypes = [C.c_uint32]
    L.eph_guess.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    L.eph_guess.restype = None
    L.eph_pick.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
    L.eph_bs.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.eph_encode.argtypes = [C.c_int] * 5 + [C.c_void_p] * 9
    L.eph_encode.restype = None
    L.eph_write.argtypes = [C.c_int] * 6 + [C.c_void_p] * 7 + [C.c_int64, C.c_void_p]
    L.eph_write.restype = C.c_int64
    L.eph_count.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 8
    L.ei4h_sps_pps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _word(v):
    return (int(v[0]) & 0xffff) | ((int(v[1]) & 0xffff) << 16)


# ------------------------------------------------ 8.4.1.3, restated
def _median(a, b, c):
    return tuple(sorted(t)[1] for t in zip(a, b, c))


def _mvp(nbs, directional=None):
    """8.4.1.3 for refIdx 0: nbs = [A, B, C], each None (the partition is not available), ("intra",) (available,
    refIdx -1) or a vector; directional: the index of the neighbour a 16x8 / 8x16 partition prefers."""
    a, b, c = nbs
    if b is None and c is None and a is not None:      # 8.4.1.3: B and C absent take A's vector and refIdx
        b = c = a
    ref = [n is not None and n != ("intra",) for n in (a, b, c)]
    mv = [n if r else (0, 0) for n, r in zip((a, b, c), ref)]
    if directional is not None and ref[directional]:
        return mv[directional]
    if sum(ref) == 1:
        return mv[ref.index(True)]
    return _median(*mv)


def _predictors(shape, q, left):
    """The predictor of every partition of a macroblock with the quadrant vectors q.  left: None (mx = 0),
    ("intra",) or (q1, q3) of the left macroblock.  The row above and the macroblock to the right are not
    available; C falls back to D (8.4.1.3.2)."""
    la = lambda i: None if left is None else (left if left == ("intra",) else left[i])   # noqa: E731
    if shape == 0:
        return [_mvp([la(0), None, None])]
    if shape == 1:      # 16x8: top prefers B, bottom prefers A; the bottom's C is the right macroblock: D = left q1
        return [_mvp([la(0), None, None], directional=1), _mvp([la(1), q[0], la(0)], directional=0)]
    if shape == 2:      # 8x16: left prefers A, right prefers C (above right, then D = above: both another slice)
        return [_mvp([la(0), None, None], directional=0), _mvp([q[0], None, None], directional=2)]
    return [_mvp([la(0), None, None]), _mvp([q[0], None, None]), _mvp([la(1), q[0], q[1]]),
            _mvp([q[2], q[1], q[0]])]                  # 8x8 3: C is the right macroblock, D = quadrant 0


LEFTS = ["none", "intra", "pcm", "skip", "16x16", "16x8", "8x16", "8x8"]


def _left_of(kind, rng):
    """What the writer knows of a left macroblock of that kind: (ok, q1, q3) and the restatement's view."""
    if kind == "none":
        return (0, (0, 0), (0, 0)), None
    if kind in ("intra", "pcm"):
        return (0, (0, 0), (0, 0)), ("intra",)
    if kind == "skip":
        return (1, (0, 0), (0, 0)), ((0, 0), (0, 0))
    v = [tuple(int(x) for x in rng.integers(-70, 71, 2)) for _ in range(4)]
    if kind == "16x16":
        v = [v[0]] * 4
    elif kind == "16x8":
        v = [v[0], v[0], v[2], v[2]]
    elif kind == "8x16":
        v = [v[0], v[1], v[0], v[1]]
    return (1, v[1], v[3]), (v[1], v[3])


@pytest.mark.parametrize("left_kind", LEFTS)
def test_predictor_of_every_block_of_every_shape(lib, left_kind):
    rng = np.random.default_rng(LEFTS.index(left_kind))
    for trial in range(200):
        (ok, l1, l3), view = _left_of(left_kind, rng)
        q = [tuple(int(x) for x in rng.integers(-70, 71, 2)) for _ in range(4)]
        if trial % 5 == 0:                       # equal vectors: medians with ties
            q[1] = q[0]
        if trial % 7 == 0 and ok:
            q[0] = l3
        for shape in range(4):
            want = _predictors(shape, q, view)
            for part, w in enumerate(want):
                qa = np.array(q, np.int32)
                la = np.array([*l1, *l3], np.int32)
                out = np.zeros(2, np.int32)
                lib.eph_pred(shape, part, qa.ctypes.data, ok, la.ctypes.data, out.ctypes.data)
                assert tuple(out) == w, f"left {left_kind} shape {shape} part {part}: q {q}, left {view}"


def test_a_16x16_macroblock_reads_quadrant_1_of_a_partitioned_left_one(lib):
    out = np.zeros(2, np.int32)
    q = np.zeros(8, np.int32)
    la = np.array([5, -6, 7, 8], np.int32)
    lib.eph_pred(0, 0, q.ctypes.data, 1, la.ctypes.data, out.ctypes.data)
    assert tuple(out) == (5, -6)
    # ... and so does the search's guess of it, from the previous picture's words
    for shape in (1, 2, 3):
        word = lib.eph_part_cmd(shape)
        assert word == 0x8000 | shape << 16 and lib.eph_is_part_cmd(word)
        lib.eph_guess(word, _word((9, -3)), 2, 2, out.ctypes.data)
        assert tuple(out) == (9, -3)
        lib.eph_guess(word, _word((9, -3)), 0, 2, out.ctypes.data)     # column 0, and the picture after the IDR
        assert tuple(out) == (0, 0)
        lib.eph_guess(word, _word((9, -3)), 2, 1, out.ctypes.data)
        assert tuple(out) == (0, 0)
    for word in (PCM, 0x80000000, 0x80004010, 0, _word((3, 4)), _word((-32768 + 1, 2)), 0x00048000):
        assert not lib.eph_is_part_cmd(word)
    lib.eph_guess(_word((3, -4)), 0, 2, 2, out.ctypes.data)
    assert tuple(out) == (3, -4)
    lib.eph_guess(PCM, 0, 2, 2, out.ctypes.data)
    assert tuple(out) == (0, 0)


# ------------------------------------------------ the decision
def _selen(k):
    code = 2 * k - 1 if k > 0 else -2 * k
    return 2 * ((code + 1).bit_length() - 1) + 1


def _decide(quads, vec, lam16, p):
    """Every block's least (16 SAD + lambda16 bits(v - p), index); the shape of least summed cost plus
    lambda16 x its overhead, ties to fewer vectors."""
    rate = [lam16 * (_selen(int(v[0]) - p[0]) + _selen(int(v[1]) - p[1])) for v in vec]
    win = []
    for b in BLOCKS:
        keys = [(16 * sum(int(quads[c][i]) for i in b) + rate[c], c) for c in range(len(vec))]
        win.append(min(keys))
    cost = [sum(win[b][0] for b in SHAPE_BLOCKS[s]) + lam16 * SHAPE_BITS[s] for s in range(4)]
    return win, cost.index(min(cost)), cost


def test_shape_decision_over_seeded_quadrant_sads(lib):
    rng = np.random.default_rng(11)
    shapes, ties = set(), 0
    for trial in range(600):
        n = int(rng.integers(1, 40))
        vec = rng.integers(-32, 33, (n, 2)).astype(np.int32) * 4
        lam16 = int(rng.choice([4, 16, 74, 300, 1335]))
        mode = trial % 6
        base = rng.integers(0, 4000, (n, 4))
        if mode == 1:                            # one candidate is best for every quadrant: 16x16 must win
            base[rng.integers(0, n)] = 0
        elif mode == 2:                          # rows pair up
            base[:, 1] = base[:, 0]
            base[:, 3] = base[:, 2]
        elif mode == 3:                          # columns pair up
            base[:, 2] = base[:, 0]
            base[:, 3] = base[:, 1]
        elif mode == 4:                          # few distinct values: ties between candidates
            base = rng.integers(0, 3, (n, 4)) * 100
        elif mode == 5:                          # exact ties between shapes: 16 SAD in steps of lam16, as the bits
            lam16 = 16
            base = rng.integers(0, 8, (n, 4))
        quads = base.astype(np.uint32)
        p = (int(rng.integers(-8, 9)), int(rng.integers(-8, 9)))
        cost9, idx9, sad9 = np.zeros(9, np.uint32), np.zeros(9, np.int32), np.zeros(9, np.uint32)
        got = lib.eph_pick(n, quads.ctypes.data, vec.ctypes.data, lam16, p[0], p[1], cost9.ctypes.data, idx9.ctypes.data,
                           sad9.ctypes.data)
        win, want, cost = _decide(quads, vec, lam16, p)
        assert [(int(c), int(i)) for c, i in zip(cost9, idx9)] == win
        assert [int(s) for s in sad9] == [sum(int(quads[i][k]) for k in b) for (_, i), b in zip(win, BLOCKS)]
        assert got == want, f"trial {trial}: costs {cost}"
        shapes.add(got)
        ties += sorted(cost)[0] == sorted(cost)[1]
    assert shapes == {0, 1, 2, 3}
    assert ties > 0                              # exact ties between shapes went to the one with fewer vectors


def test_a_tie_between_all_shapes_goes_to_one_vector(lib):
    # one candidate, SAD 0, at the predictor: shape costs are lam16 x (2 + 1), (4 + 3), (4 + 3), (8 + 9); with
    # lam16 = 0 every shape costs 0 and 16x16 wins
    quads, vec = np.zeros((1, 4), np.uint32), np.zeros((1, 2), np.int32)
    out = [np.zeros(9, np.uint32), np.zeros(9, np.int32), np.zeros(9, np.uint32)]
    assert lib.eph_pick(1, quads.ctypes.data, vec.ctypes.data, 0, 0, 0, *(o.ctypes.data for o in out)) == 0
    # two candidates at lam16 = 16, p = (0, 0): (0, 0) costs 2 bits = 32, (4, 0) 8 bits = 128.  The bottom half
    # matches at (4, 0) only and costs 16 x 5 a quadrant at (0, 0): one vector 160 + 32 + 16 = 208, top and bottom
    # 32 + 128 + 48 = 208: the tie goes to one vector; one SAD less at (4, 0)'s side and 16x8 wins
    quads, vec = np.array([[0, 0, 5, 5], [900, 900, 0, 0]], np.uint32), np.array([[0, 0], [4, 0]], np.int32)
    assert lib.eph_pick(2, quads.ctypes.data, vec.ctypes.data, 16, 0, 0, *(o.ctypes.data for o in out)) == 0
    assert [int(c) for c in out[0][:3]] == [192, 32, 128]
    quads[0, 2] = 6
    assert lib.eph_pick(2, quads.ctypes.data, vec.ctypes.data, 16, 0, 0, *(o.ctypes.data for o in out)) == 1
    assert [lib.eph_shape_bits(s) for s in range(4)] == SHAPE_BITS
    assert [lib.eph_block_quads(b) for b in range(9)] == [sum(1 << i for i in b) for b in BLOCKS]


def test_canonical_form_for_every_pattern_of_equal_vectors(lib):
    vals = [_word((4, -8)), _word((5, -8)), _word((4, -7)), _word((-1, 2))]
    seen = set()
    for pat in itertools.product(range(4), repeat=4):          # which of four distinct vectors each quadrant has
        v = np.array([vals[i] for i in pat], np.uint32)
        if pat[0] == pat[1] == pat[2] == pat[3]:
            want = 0
        elif pat[0] == pat[1] and pat[2] == pat[3]:
            want = 1
        elif pat[0] == pat[2] and pat[1] == pat[3]:
            want = 2
        else:
            want = 3
        assert lib.eph_canonical(v.ctypes.data) == want, pat
        seen.add(want)
    assert seen == {0, 1, 2, 3}
    for v, want in (([0, 0, 0, 0], 0), ([_word((4, 8))] * 4, 0), ([_word((4, 8)), _word((2, 0)), 0, 0], 1),
                    ([_word((4, 8)), _word((2, 0)), _word((1, 0)), 0], 2), ([0, 0, 0, _word((0, -3))], 2),
                    ([_word((-2, 0))] * 4, 1)):
        assert lib.eph_frac_class(np.array(v, np.uint32).ctypes.data) == want


# ------------------------------------------------------------ whole rows
def _pictures(rng, mbw, mbh, npic):
    """Textured pictures (so that a displaced prediction differs from the co-located one), each the previous
    one plus noise; samples in 1..255."""
    W, H = 16 * mbw, 16 * mbh
    yy, xx = np.mgrid[0:H * 3 // 2, 0:W]
    base = 128 + 60 * np.sin((xx + 2 * yy) / 3.0) + 40 * ((xx // 5 + yy // 3) % 2) + rng.integers(-10, 11, xx.shape)
    pics = [np.clip(base, 1, 255)]
    for _ in range(npic - 1):
        pics.append(np.clip(pics[-1] + rng.integers(-25, 26, xx.shape) * (rng.random(xx.shape) < 0.5), 1, 255))
    return np.stack(pics).astype(np.uint8)


def _vectors(rng, want):
    """Quadrant vectors (quarter samples) whose canonical shape is `want`; up to +-80 samples: past every
    picture edge of these small pictures, with every fraction."""
    while True:
        v = rng.integers(-320, 321, (4, 2))
        if rng.random() < 0.3:
            v = rng.integers(-9, 10, (4, 2))
        if want == 0:
            v[:] = v[0]
        elif want == 1:
            v[1], v[3] = v[0], v[2]
        elif want == 2:
            v[2], v[3] = v[0], v[1]
        w = [_word(x) for x in v]
        got = 0 if len(set(w)) == 1 else 1 if (w[0] == w[1] and w[2] == w[3]) else 2 if (w[0] == w[2] and w[1] == w[3]) else 3
        if got == want:
            return v


# per macroblock (kind of eph_encode, canonical shape wanted)
ROW_KINDS = {"pcm": (0, 0), "i16": (1, 0), "i4": (2, 0), "skip": (3, 0), "p16": (4, 0), "p16x8": (4, 1),
             "p8x16": (4, 2), "p8x8": (4, 3), "p16x8_nores": (3, 1), "p8x8_nores": (3, 3)}


def _rows(rng, mbw, mbh, npic):
    names = list(ROW_KINDS)
    kind = np.zeros((npic, mbh, mbw), np.uint8)
    vec = np.zeros((npic, mbh, mbw, 4, 2), np.int32)
    label = np.full((npic, mbh, mbw), "", object)
    for p in range(npic):
        for my in range(mbh):
            for mx in range(mbw):
                name = str(rng.choice(names[:3] if p == 0 else names))
                if p == 1 and my == 0 and mbw == 12:       # every kind once beside every shape
                    name = ["p16x8", "pcm", "p8x16", "i16", "p8x8", "i4", "p16x8", "skip", "p8x8", "p16", "p8x16", "p8x8"][mx]
                k, shape = ROW_KINDS[name]
                kind[p, my, mx] = k
                label[p, my, mx] = name
                if k >= 3 and name != "skip":
                    vec[p, my, mx] = _vectors(rng, shape)
    return kind, vec, label


def _encode(lib, mbw, mbh, npic, qp, dbk, src, kind, vec):
    n = npic * mbh * mbw
    r = dict(cmd=np.zeros(n, np.uint32), cbp=np.zeros(n, np.uint8), coef=np.zeros((n, 384), np.int16),
             modes=np.zeros(n, np.uint64), mv4=np.zeros((n, 4), np.uint32), rec=np.zeros_like(src))
    lib.eph_encode(mbw, mbh, npic, qp, dbk, src.ctypes.data, kind.ctypes.data, vec.ctypes.data, r["cmd"].ctypes.data,
                   r["cbp"].ctypes.data, r["coef"].ctypes.data, r["modes"].ctypes.data, r["mv4"].ctypes.data,
                   r["rec"].ctypes.data)
    return r


def _write(lib, mbw, mbh, npic, qp, dbk, cabac, src, r):
    out = np.zeros(npic * mbh * mbw * 9024 + 1024, np.uint8)
    sizes = np.zeros(npic, np.int64)
    n = lib.eph_write(mbw, mbh, npic, qp, dbk, cabac, src.ctypes.data, r["cmd"].ctypes.data, r["cbp"].ctypes.data,
                      r["coef"].ctypes.data, r["modes"].ctypes.data, r["mv4"].ctypes.data, out.ctypes.data, out.size,
                      sizes.ctypes.data)
    assert n > 0
    at, samples = 0, []
    for s in sizes:
        samples.append(out[at:at + s].tobytes())
        at += int(s)
    return samples


def _parameter_sets(lib, mbw, mbh, cabac):
    sps, pps, k = np.zeros(64, np.uint8), np.zeros(64, np.uint8), np.zeros(2, np.int32)
    lib.ei4h_sps_pps(mbw, mbh, int(cabac != 0), sps.ctypes.data, pps.ctypes.data, k.ctypes.data)
    return sps[:k[0]].tobytes(), pps[:k[1]].tobytes()


@pytest.mark.parametrize("dbk", [0, 1])
@pytest.mark.parametrize("qp", [1, 28, 51])
@pytest.mark.parametrize("mbw", [1, 2, 12])
def test_rows_decode_to_the_harness_reconstruction(lib, tmp_path, mbw, qp, dbk):
    import oracle
    rng = np.random.default_rng(1000 * mbw + qp)
    mbh, npic = 2, 4
    src = _pictures(rng, mbw, mbh, npic)
    kind, vec, label = _rows(rng, mbw, mbh, npic)
    r = _encode(lib, mbw, mbh, npic, qp, dbk, src, kind, vec)
    cmd, flat = r["cmd"], label.reshape(-1)
    part = ((cmd & 0xffff) == 0x8000) & ((cmd >> 16) >= 1) & ((cmd >> 16) <= 3)
    for a, name in enumerate(flat):
        shape = ROW_KINDS[name][1]
        assert bool(part[a]) == (shape > 0) and (not shape or int(cmd[a]) == (0x8000 | shape << 16)), (a, name, hex(cmd[a]))
        if ROW_KINDS[name][0] >= 3:
            assert [int(x) for x in r["mv4"][a]] == [_word(v) for v in vec.reshape(-1, 4, 2)[a]]
        else:
            assert (r["mv4"][a] == PCM).all()
    if mbw == 12:
        assert {n for n in flat} == set(ROW_KINDS)
        # fractions in both components, and blocks that reach past each of the four picture edges
        pp, my, mx = np.nonzero(kind >= 3)
        v = vec[pp, my, mx]                                  # [n, 4 quadrants, (x, y)] quarter samples
        x0 = (16 * mx)[:, None] + np.array([0, 8, 0, 8])     # the quadrants' first samples
        y0 = (16 * my)[:, None] + np.array([0, 0, 8, 8])
        vx, vy = v[..., 0], v[..., 1]
        assert (vx % 4 != 0).any() and (vy % 4 != 0).any() and (vx % 2 != 0).any() and (vy % 2 != 0).any()
        assert (x0 + (vx >> 2) < 0).any() and (x0 + 7 + ((vx + 3) >> 2) >= 16 * mbw).any()
        assert (y0 + (vy >> 2) < 0).any() and (y0 + 7 + ((vy + 3) >> 2) >= 16 * mbh).any()
    files = {}
    for cabac in (0, 1, 2):
        samples = _write(lib, mbw, mbh, npic, qp, dbk, cabac, src, r)
        sps, pps = _parameter_sets(lib, mbw, mbh, cabac)
        path = tmp_path / f"c{cabac}.mp4"
        oracle.write_mp4(path, sps, pps, samples, list(range(npic)), [0] * npic, 30, 16 * mbw, 16 * mbh)
        frames, _ = oracle.decode_full(path)
        assert frames.shape == r["rec"].shape
        bad = [i for i in range(npic) if not np.array_equal(frames[i], r["rec"][i])]
        assert bad == [], f"cabac {cabac}: the oracle's pictures differ from the harness's at {bad}"
        files[cabac] = b"".join(samples)
    assert files[1] == files[2]                          # BinRing and drain(): the bytes of the direct coder
    if dbk:                                              # the filter changed something: the check above is not vacuous
        plain = _encode(lib, mbw, mbh, npic, qp, 0, src, kind, vec)
        assert qp == 1 or not np.array_equal(plain["rec"], r["rec"])
    print(f"mbw {mbw} qp {qp} dbk {dbk}: CAVLC {len(files[0])} bytes, CABAC {len(files[1])} bytes; "
          f"partitioned {int(part.sum())} of {part.size}")


@pytest.mark.parametrize("mbw", [1, 2, 6])
def test_counted_bits_equal_the_bits_written(lib, mbw):
    """Every macroblock kind adds to the counting sink exactly the RBSP bits it gives the byte sink, the
    partitioned ones included, whatever the left macroblock was."""
    rng = np.random.default_rng(7100 + mbw)
    seen = set()
    for trial in range(200):
        names = [str(rng.choice(["pcm", "i16", "skip", "p16", "p16x8", "p8x16", "p8x8"])) for _ in range(mbw)]
        cmd, cbp = np.zeros(mbw, np.uint32), np.zeros(mbw, np.uint8)
        modes, mv4 = np.full(mbw, NONE, np.uint64), np.full((mbw, 4), PCM, np.uint32)
        on = rng.random((mbw, 24, 16)) < rng.choice([0.0, 0.2, 0.8], (mbw, 24, 1))
        coef = (on * rng.integers(1, 40, on.shape) * rng.choice([-1, 1], on.shape)).astype(np.int16).reshape(mbw, 384)
        pcm = rng.integers(1, 256, (mbw, 384)).astype(np.uint8)
        for mx, name in enumerate(names):
            if name == "pcm":
                cmd[mx] = PCM
            elif name == "i16":
                cmd[mx] = 0x80000000 | 2 | (int(rng.integers(0, 3)) << 8)
            elif name == "skip":
                mv4[mx] = 0
            else:
                shape = ROW_KINDS[name][1]
                v = _vectors(rng, shape)
                mv4[mx] = [_word(x) for x in v]
                cbp[mx] = int(rng.integers(0, 48))
                cmd[mx] = (0x8000 | shape << 16) if shape else mv4[mx][0]
                if cmd[mx] == 0 and cbp[mx] == 0:
                    cbp[mx] = 1
        counted, written = np.zeros(mbw, np.int64), np.zeros(mbw, np.int64)
        assert lib.eph_count(0, mbw, cmd.ctypes.data, cbp.ctypes.data, coef.ctypes.data, modes.ctypes.data, mv4.ctypes.data,
                             pcm.ctypes.data, counted.ctypes.data, written.ctypes.data) == 0
        assert counted.tolist() == written.tolist(), f"trial {trial}: {names}"
        for mx, name in enumerate(names):
            seen.add(("none" if mx == 0 else names[mx - 1], name))
            assert (counted[mx] == 0) == (name == "skip")
    if mbw == 6:
        parts = ("p16x8", "p8x16", "p8x8")
        assert {(l, k) for l in ("pcm", "i16", "skip", "p16") + parts for k in parts} <= seen


# ------------------------------------------------------------ bS
def _bs(p, q, bp, bq, mb_edge):
    """8.7.2.1 for frame macroblocks and one reference picture; p, q: ("intra",) or (nz mask, four vectors)."""
    if p == ("intra",) or q == ("intra",):
        return 4 if mb_edge else 3
    if (p[0] >> bp) & 1 or (q[0] >> bq) & 1:
        return 2
    quad = lambda b: (b // 8) * 2 + (b % 4) // 2          # noqa: E731
    a, b = p[1][quad(bp)], q[1][quad(bq)]
    return int(abs(a[0] - b[0]) >= 4 or abs(a[1] - b[1]) >= 4)


def test_bs_of_every_inner_and_left_edge_line(lib):
    rng = np.random.default_rng(5)
    got_one_inner = False
    # a 16x8 left macroblock beside a 16x16 one: the left edge's upper half is 0, its lower half 1
    pv = np.array([0, 0, _word((8, 0)), _word((8, 0))], np.uint32)
    qv = np.zeros(4, np.uint32)
    assert [lib.eph_bs(0x18000, 0, pv.ctypes.data, 0, 0, qv.ctypes.data, 0, 0, k) for k in (0, 7, 8, 15)] == [0, 0, 1, 1]
    # ... and inside the 16x8 one the edge at y = 8 is 1, the edges at y = 4 and 12 are 0
    assert [lib.eph_bs(0, 0, qv.ctypes.data, 0x18000, 0, pv.ctypes.data, 1, e, 3) for e in (1, 2, 3)] == [0, 1, 0]
    assert [lib.eph_bs(0, 0, qv.ctypes.data, 0x18000, 0, pv.ctypes.data, 0, e, 3) for e in (1, 2, 3)] == [0, 0, 0]
    for trial in range(150):
        def mb():
            if rng.random() < 0.15:
                return ("intra",), int(rng.choice([PCM, 0x80000020])), 0, np.full(4, PCM, np.uint32)
            v = _vectors(rng, int(rng.integers(0, 4)))
            if rng.random() < 0.6:
                v = v[0] + rng.integers(-5, 6, (4, 2))      # differences around the threshold of 4
            nz = int(rng.integers(0, 1 << 16)) if rng.random() < 0.4 else 0
            w = np.array([_word(x) for x in v], np.uint32)
            shape = lib.eph_canonical(w.ctypes.data)
            return (nz, [tuple(int(c) for c in x) for x in v]), (0x8000 | shape << 16) if shape else int(w[0]), nz, w
        P, Q = mb(), mb()
        for dirn in (0, 1):
            for e in range(4):
                if e == 0 and dirn == 1:
                    continue                               # the top edge is a slice boundary: never filtered
                for k in range(16):
                    bq = e * 4 + k // 4 if dirn else (k // 4) * 4 + e
                    bp = ((e + 3) % 4) * 4 + k // 4 if dirn else (k // 4) * 4 + (e + 3) % 4
                    pp = P if e == 0 else Q
                    want = _bs(pp[0], Q[0], bp, bq, e == 0)
                    got = lib.eph_bs(P[1], P[2], P[3].ctypes.data, Q[1], Q[2], Q[3].ctypes.data, dirn, e, k)
                    assert got == want, f"trial {trial} dir {dirn} edge {e} line {k}"
                    got_one_inner |= e == 2 and got == 1
    assert got_one_inner                         # bS 1 on an inner edge in the seeded pairs too


def test_sanitizer_run_of_the_stand_alone_driver(tmp_path):
    """enc_part_main.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, run as a program."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtimes")       # an empty program does not link with them
    exe = tmp_path / "enc_part_main"
    r = subprocess.run(["g++", "-O1", "-g", *san, *FLAGS, str(NATIVE / "enc_part_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]                       # with the runtimes there, an error is an error
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "enc_part_main: ok" in run.stdout, run.stdout[-1000:] + run.stderr[-3000:]
