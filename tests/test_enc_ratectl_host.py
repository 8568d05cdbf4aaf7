"""The device encoder's rate control on the CPU (no GPU).

`csrc/enc_ratectl.h` holds the law the kernel `enc_rc` runs, one controller per
GOP (DESIGN.md §11 "Rate control"); the harness
(tests/native/enc_ratectl_host.cpp) exposes it.

  law:    seeded per-picture measures over GOPs of 1, 2, 3 and 250 pictures:
          every step within +-4, every QP inside [qp_min, qp_max], qp_min ==
          qp_max constant, a picture that measured 0 keeps the QP, an overspent
          GOP raises it by 4, the step monotone in the measure, the table's
          boundaries exact, no overflow at the largest budget;
  model:  against a source whose pictures cost C 2^(-qp / 6) bits a GOP's total
          moves towards B L from both sides;
  rows:   three pictures (IDR, P, P) at three different QPs written as CAVLC and
          as CABAC (tests/native/enc_ratectl_rows_host.cpp): the CPU oracle's
          general decoder decodes both to the harness's reconstruction, which
          pins slice_qp_delta and the CABAC context initialisation at a QP that
          changes between pictures.
"""
from __future__ import annotations

import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_enc_part_host import FLAGS, NATIVE, ROOT, SRCS, _parameter_sets, _pictures, _rows

sys.path.insert(0, str(ROOT / "oracle"))

T = [1024, 1149, 1290, 1448, 1625]          # 2^(k / 6) in Q10
I64 = C.c_int64


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("erch") / "libencratectlhost.so"
    subprocess.run(["g++", "-Og", "-fPIC", "-shared", *FLAGS, str(NATIVE / "enc_ratectl_host.cpp"), "-o", str(so)],
                   check=True)
    L = C.CDLL(str(so))
    L.erch_next_qp.argtypes = [I64, I64, I64, I64, I64, C.c_int, C.c_int, C.c_int]
    L.erch_first_qp.argtypes = [C.c_int] * 3
    L.erch_frame_budget.argtypes = [C.c_int, I64, I64]
    L.erch_frame_budget.restype = I64
    L.erch_step_q10.argtypes = [C.c_int]
    L.erch_step_q10.restype = I64
    L.erch_replay.argtypes = [I64, I64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.erch_replay.restype = None
    return L


def replay(lib, B, bits, qp, lo, hi):
    """The QPs of one GOP whose pictures measured `bits` (the harness's erch_replay)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    qps = np.zeros(len(bits), np.uint8)
    lib.erch_replay(B, len(bits), qp, lo, hi, bits.ctypes.data, qps.ctypes.data)
    return qps


def test_the_table_is_two_to_the_k_sixths():
    assert T == [int(round(1024 * 2 ** (k / 6))) for k in range(5)]


def test_budget_is_the_floor_of_bits_per_frame(lib):
    assert [lib.erch_step_q10(k) for k in range(5)] == T
    for kbps, delta, ts in ((500, 1000, 30000), (1, 1, 240), (1000000, 1, 1), (777, 1001, 30000), (3, 512, 12800)):
        assert lib.erch_frame_budget(kbps, delta, ts) == kbps * 1000 * delta // ts
    assert lib.erch_first_qp(28, 10, 51) == 28 and lib.erch_first_qp(5, 10, 51) == 10 and lib.erch_first_qp(51, 10, 40) == 40


@pytest.mark.parametrize("L", [1, 2, 3, 250])
def test_steps_and_bounds_over_seeded_measures(lib, L):
    rng = np.random.default_rng(100 + L)
    moved = set()
    for trial in range(300):
        lo = int(rng.integers(1, 52))
        hi = int(rng.integers(lo, 52))
        qp = int(rng.integers(1, 52))
        B = int(rng.choice([0, 4, 1000, 16666, 400000, 10 ** 9]))
        scale = int(rng.choice([1, 1000, 100000, 2 ** 32 - 1]))
        bits = (rng.random(L) * scale).astype(np.uint32)
        bits[rng.random(L) < 0.1] = 0
        qps = replay(lib, B, bits, qp, lo, hi).astype(int)
        assert qps[0] == min(max(qp, lo), hi)
        assert (qps >= lo).all() and (qps <= hi).all()
        assert (np.abs(np.diff(qps)) <= 4).all()
        if L > 1:
            assert qps[1] == min(qps[0] + 3, hi)
        moved |= set(np.diff(qps).tolist())
        # every picture again through the one-step function: a picture that measured 0 keeps the QP, an
        # overspent GOP raises it by 4
        spent = 0
        for j in range(L - 1):
            spent += int(bits[j])
            assert lib.erch_next_qp(B, L, j, spent, int(bits[j]), int(qps[j]), lo, hi) == qps[j + 1]
            if j >= 1 and bits[j] == 0:
                assert qps[j + 1] == qps[j]
            elif j >= 1 and B * L - spent < L - j - 1:        # want <= 0
                assert qps[j + 1] == min(qps[j] + 4, hi)
    if L == 250:
        assert moved == set(range(-4, 5))


@pytest.mark.parametrize("q", [1, 10, 28, 51])
def test_equal_bounds_give_that_constant(lib, q):
    rng = np.random.default_rng(q)
    for L in (1, 2, 3, 250):
        bits = rng.integers(0, 2 ** 32, L, dtype=np.uint64).astype(np.uint32)
        assert (replay(lib, 16666, bits, 28, q, q) == q).all()


def _step_by_the_text(bits, want):
    """The rule for want > 0 and bits > 0: up by the largest k with bits 1024 >= want T[k], else down by the
    largest k with want 1024 >= bits T[k]."""
    up = [k for k in range(5) if bits * 1024 >= want * T[k]]
    return up[-1] if up else -[k for k in range(5) if want * 1024 >= bits * T[k]][-1]


def test_step_is_monotone_in_the_measure_and_exact_at_the_table(lib):
    rng = np.random.default_rng(5)
    for trial in range(200):
        B, L = int(rng.integers(1, 10 ** 6)), int(rng.integers(3, 251))
        j = int(rng.integers(1, L - 1))
        spent = int(rng.integers(0, B * L))
        want = (B * L - spent) // (L - j - 1)
        assert want > 0
        step = lambda b: lib.erch_next_qp(B, L, j, spent, b, 28, 1, 51) - 28      # noqa: E731
        grid = sorted({1, want // 8, want // 2, want - 1, want, want + 1, 2 * want, 8 * want, 2 ** 32 - 1} - {0})
        steps = [step(b) for b in grid]
        assert steps == sorted(steps), (grid, steps)
        assert steps == [_step_by_the_text(b, want) for b in grid]
        assert step(want) == 0 and step(2 ** 32 - 1 if want < 2 ** 31 else want) >= 0
        for k in range(1, 5):
            up = -(-want * T[k] // 1024)            # the least measure with bits 1024 >= want T[k]
            down = want * 1024 // T[k]              # the largest measure with want 1024 >= bits T[k]
            for b in (up - 1, up, down, down + 1):
                if b >= 1:
                    assert step(b) == _step_by_the_text(b, want), (want, k, b)
            if want >= 64:                          # the table's steps are then distinct measures
                assert step(up) == k and step(up - 1) == k - 1, (want, k)
                assert step(down) == -k and step(down + 1) == -(k - 1), (want, k)
    # exactly want T[k] / 1024 where that is whole, and one below it
    B, L, j, spent = 1024, 10, 1, 1024 * 2          # want = 1024
    for k in range(1, 5):
        assert lib.erch_next_qp(B, L, j, spent, T[k], 28, 1, 51) == 28 + k
        assert lib.erch_next_qp(B, L, j, spent, T[k] - 1, 28, 1, 51) == 28 + k - 1
    # the measure 0 keeps the QP although the measure 1 asks for the largest step down
    assert lib.erch_next_qp(B, L, j, spent, 0, 28, 1, 51) == 28 and lib.erch_next_qp(B, L, j, spent, 1, 28, 1, 51) == 24
    # an overspent GOP: want <= 0, whatever the picture measured
    for b in (1, 1000, 2 ** 32 - 1):
        assert lib.erch_next_qp(B, L, j, B * L, b, 28, 1, 51) == 32
        assert lib.erch_next_qp(B, L, j, B * L + 5, b, 49, 1, 51) == 51


def test_no_overflow_at_the_largest_budget(lib):
    B = lib.erch_frame_budget(1000000, 1, 1)          # one picture a second at the top bitrate
    assert B == 10 ** 9
    L = 250
    big = 2 ** 32 - 1
    # nothing spent yet: want = B L / 248 = 1 008 064 516 < 2^32 - 1 by a factor 4.26: four steps up
    assert lib.erch_next_qp(B, L, 1, 2 * big, big, 28, 1, 51) == 32
    want = (B * L - 2 * big) // 248
    for k in range(1, 5):
        up = -(-want * T[k] // 1024)
        assert lib.erch_next_qp(B, L, 1, 2 * big, up, 28, 1, 51) == 28 + k
        assert lib.erch_next_qp(B, L, 1, 2 * big, up - 1, 28, 1, 51) == 28 + k - 1
    # the whole GOP at the largest measure
    qps = replay(lib, B, np.full(L, big, np.uint32), 28, 1, 51).astype(int)
    assert qps[0] == 28 and qps[1] == 31 and (np.abs(np.diff(qps)) <= 4).all() and qps[-1] == 51
    # the last picture of a long GOP has the whole budget left: want is far above any measure
    assert lib.erch_next_qp(B, 10 ** 7, 10 ** 7 - 2, 0, big, 28, 1, 51) == 24


def _model_bits(C0, qp):
    """C0 2^(-qp / 6), the halvings exact (a shift), six linear steps between them."""
    a, b = C0 >> (qp // 6), C0 >> (qp // 6 + 1)
    return a - (a - b) * (qp % 6) // 6


def _model_gop(lib, B, L, qp0, C0):
    qps, bits, spent = [lib.erch_first_qp(qp0, 1, 51)], [], 0
    for j in range(L):
        bits.append(_model_bits(C0, qps[-1]))
        spent += bits[-1]
        if j + 1 < L:
            qps.append(lib.erch_next_qp(B, L, j, spent, bits[-1], qps[-1], 1, 51))
    return qps, spent


def test_a_model_source_moves_towards_the_budget_from_both_sides(lib):
    """A source whose pictures cost C 2^(-qp / 6): started too cheap (a high QP) or too dear (a low one), the
    GOP's total ends nearer B L than the fixed-QP total.  Only the direction is asserted; the end ratios are in
    DESIGN.md §11 "Rate control"."""
    L, C0 = 250, 40_000_000
    B = _model_bits(C0, 30)                         # the budget the source meets at QP 30
    for qp0 in (16, 22, 38, 44):
        fixed = L * _model_bits(C0, qp0)
        qps, total = _model_gop(lib, B, L, qp0, C0)
        print(f"model qp0 {qp0}: fixed-QP total / budget {fixed / (B * L):.3f}, controlled {total / (B * L):.3f}, "
              f"QPs {min(qps)}..{max(qps)}, last {qps[-1]}")
        assert abs(total - B * L) < abs(fixed - B * L)
        if qp0 < 30:
            assert total < fixed and qps[-1] > qp0
        else:
            assert total > fixed and qps[-1] < qp0


def test_sanitizer_run_of_the_stand_alone_driver(tmp_path):
    """enc_ratectl_main.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, run as a program."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtimes")       # an empty program does not link with them
    exe = tmp_path / "enc_ratectl_main"
    r = subprocess.run(["g++", "-O1", "-g", *san, *FLAGS, str(NATIVE / "enc_ratectl_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]                       # with the runtimes there, an error is an error
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "enc_ratectl_main: ok" in run.stdout, run.stdout[-1000:] + run.stderr[-3000:]


# ------------------------------------------------- rows at a changing QP
@pytest.fixture(scope="module")
def rows_lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("erq") / "libencratectlrows.so"
    subprocess.run(["g++", "-Og", "-fPIC", "-shared", *FLAGS, str(NATIVE / "enc_ratectl_rows_host.cpp"),
                    *map(str, SRCS), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.erq_encode.argtypes = [C.c_int] * 3 + [C.c_void_p, C.c_int] + [C.c_void_p] * 9
    L.erq_encode.restype = None
    L.erq_write.argtypes = [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int64, C.c_void_p]
    L.erq_write.restype = C.c_int64
    L.ei4h_sps_pps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.mark.parametrize("dbk", [0, 1])
@pytest.mark.parametrize("qps", [(20, 51, 1), (45, 12, 33), (28, 28, 28)])
@pytest.mark.parametrize("mbw", [1, 2, 12])
def test_rows_at_a_changing_qp_decode_to_the_harness_reconstruction(rows_lib, tmp_path, mbw, qps, dbk):
    import oracle
    lib = rows_lib
    rng = np.random.default_rng(31 * mbw + qps[0])
    mbh, npic = 2, 3
    src = _pictures(rng, mbw, mbh, npic)
    kind, vec, _ = _rows(rng, mbw, mbh, npic)
    n = npic * mbh * mbw
    qp = np.array(qps, np.int32)
    r = dict(cmd=np.zeros(n, np.uint32), cbp=np.zeros(n, np.uint8), coef=np.zeros((n, 384), np.int16),
             modes=np.zeros(n, np.uint64), mv4=np.zeros((n, 4), np.uint32), rec=np.zeros_like(src))
    lib.erq_encode(mbw, mbh, npic, qp.ctypes.data, dbk, src.ctypes.data, kind.ctypes.data, vec.ctypes.data,
                   r["cmd"].ctypes.data, r["cbp"].ctypes.data, r["coef"].ctypes.data, r["modes"].ctypes.data,
                   r["mv4"].ctypes.data, r["rec"].ctypes.data)
    sizes_by = {}
    for cabac in (0, 1, 2):
        out = np.zeros(n * 9024 + 1024, np.uint8)
        sizes = np.zeros(npic, np.int64)
        got = lib.erq_write(mbw, mbh, npic, qp.ctypes.data, dbk, cabac, src.ctypes.data, r["cmd"].ctypes.data,
                            r["cbp"].ctypes.data, r["coef"].ctypes.data, r["modes"].ctypes.data, r["mv4"].ctypes.data,
                            out.ctypes.data, out.size, sizes.ctypes.data)
        assert got > 0
        at, samples = 0, []
        for s in sizes:
            samples.append(out[at:at + s].tobytes())
            at += int(s)
        sps, pps = _parameter_sets(lib, mbw, mbh, cabac)
        path = tmp_path / f"c{cabac}.mp4"
        oracle.write_mp4(path, sps, pps, samples, list(range(npic)), [0] * npic, 30, 16 * mbw, 16 * mbh)
        frames, _ = oracle.decode_full(path)
        assert frames.shape == r["rec"].shape
        bad = [i for i in range(npic) if not np.array_equal(frames[i], r["rec"][i])]
        assert bad == [], f"cabac {cabac}: the oracle's pictures differ from the harness's at {bad}"
        sizes_by[cabac] = b"".join(samples)
    assert sizes_by[1] == sizes_by[2]
    if len(set(qps)) > 1:
        # the check is not vacuous: the same data written with picture 0's QP in every header decodes to other
        # pictures (the levels are scaled at the wrong QP) or not at all
        flat = np.full(npic, qps[0], np.int32)
        out = np.zeros(n * 9024 + 1024, np.uint8)
        sizes = np.zeros(npic, np.int64)
        lib.erq_write(mbw, mbh, npic, flat.ctypes.data, dbk, 0, src.ctypes.data, r["cmd"].ctypes.data, r["cbp"].ctypes.data,
                      r["coef"].ctypes.data, r["modes"].ctypes.data, r["mv4"].ctypes.data, out.ctypes.data, out.size,
                      sizes.ctypes.data)
        assert out[:int(sizes.sum())].tobytes() != sizes_by[0]
