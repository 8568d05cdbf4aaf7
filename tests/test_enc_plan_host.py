"""The device encoder's GOP plan and chunk / ring arithmetic on the CPU (no GPU).

`csrc/enc_plan.h` holds `plan_gops` and the helpers by which
`csrc/transcode_driver.cpp` cuts the levels into chunks and reuses the ring of
residual levels.  The harness (tests/native/enc_plan_host.cpp) exposes them;
the properties below are what the kernels and the driver rely on.
"""
from __future__ import annotations

import ctypes as C
import itertools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "video-transformer_amd" / "csrc"
NATIVE = ROOT / "tests" / "native"
FLAGS = ["-std=c++17", "-Wall", "-Wextra", f"-I{CSRC}", f"-I{NATIVE}"]
THR = 0.08
NS = (1, 2, 3, 17, 33, 49, 50, 70)
KEYINTS = (1, 2, 16, 33, 250)


def _score_vectors(n):
    """0, 1 and several values over the threshold; cuts at frames 1 and n - 1 among them."""
    out = {"none": []}
    if n > 1:
        out["first"] = [1]
        out["last"] = [n - 1]
    if n > 5:
        out["five"] = [5]   # with keyint 33 and n = 50: GOPs of 5, 33 and 12 frames
        out["several"] = sorted({1, 5, n // 2, n - 1})
    return {k: np.array([1.0 if f in v else 0.0 for f in range(n)], np.float32) for k, v in out.items()}


INPUTS = [(n, k, name, cuts, intra, rate) for n in NS for k in KEYINTS for name in _score_vectors(n)
          for cuts, intra, rate in itertools.product((False, True), (False, True), (0, 3))]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("eph") / "libencplanhost.so"
    subprocess.run(["g++", "-Og", "-fPIC", "-shared", *FLAGS, str(NATIVE / "enc_plan_host.cpp"), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    for f in (L.eph_ring, L.eph_chunk_levels, L.eph_chunk_freeing):
        f.restype = C.c_int64
    L.eph_chunk_freeing.argtypes = [C.c_int64]
    L.eph_plan.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int64, C.c_int64] + \
        [C.c_void_p] * 6
    return L


def _plan(L, n, scores, keyint, cuts, intra, rate):
    cap = n + 2   # >= entries, levels, GOPs and chunks
    sent, went = np.full((cap, 4), -7, np.int32), np.full((cap, 4), -7, np.int32)
    lvl_off, gop_start = np.full(cap + 1, -7, np.int64), np.full(cap, -7, np.int64)
    chunks, dims = np.full((cap, 2), -7, np.int64), np.zeros(5, np.int64)
    rc = L.eph_plan(n, scores.ctypes.data, keyint, int(cuts), THR, int(intra), rate, cap, cap, sent.ctypes.data,
                    went.ctypes.data, lvl_off.ctypes.data, gop_start.ctypes.data, chunks.ctypes.data, dims.ctypes.data)
    assert rc == 0
    entries, maxlen, ngop, nchunks, max_chunk = (int(v) for v in dims)
    return dict(sent=sent[:entries], went=went[:entries], lvl_off=lvl_off[:maxlen + 1], gop_start=gop_start[:ngop],
                chunks=chunks[:nchunks], maxlen=maxlen, ngop=ngop, max_chunk=max_chunk)


def _gop_starts(n, scores, keyint, cuts):
    """The rule: frame 0, a score over the threshold when idr_at_cuts, and a distance of keyint."""
    starts = []
    for f in range(n):
        if f == 0 or (cuts and scores[f] > THR) or f - starts[-1] >= keyint:
            starts.append(f)
    return starts


@pytest.fixture(scope="module")
def plans(lib):
    """Every input planned once: (n, keyint, scores' name, idr_at_cuts, intra, rate) -> (plan, scores)."""
    out = {}
    for key in INPUTS:
        n, keyint, name, cuts, intra, rate = key
        sc = _score_vectors(n)[name]
        out[key] = (_plan(lib, n, sc, keyint, cuts, intra, rate), sc)
    return out


def _levels(p):
    """Per level j: the slice of its entries."""
    return [slice(int(p["lvl_off"][j]), int(p["lvl_off"][j + 1])) for j in range(p["maxlen"])]


def test_gops_and_levels(plans):
    for (n, keyint, _, cuts, intra, rate), (p, sc) in plans.items():
        starts = _gop_starts(n, sc, keyint, cuts)
        assert list(p["gop_start"]) == starts and p["ngop"] == len(starts)
        lens = [(starts[k + 1] if k + 1 < len(starts) else n) - starts[k] for k in range(len(starts))]
        assert p["maxlen"] == max(lens)
        # every frame exactly once among the write entries, and among the search entries (all levels >= 0)
        assert sorted(p["went"][:, 0]) == list(range(n)) and sorted(p["sent"][:, 0]) == list(range(n))
        off = p["lvl_off"]
        assert off[0] == 0 and off[-1] == len(p["went"]) == n and np.all(np.diff(off) >= 0)
        for j, sl in enumerate(_levels(p)):
            gops = [k for k in range(len(starts)) if lens[k] > j]   # exactly the GOPs longer than j, in GOP order
            want = [starts[k] + j for k in gops]
            assert list(p["went"][sl, 0]) == want and list(p["sent"][sl, 0]) == want
            assert np.all(p["went"][sl, 1] == j)
            assert list(p["went"][sl, 2]) == [k & 1 for k in gops]            # IDR parity
            assert list(p["went"][sl, 3]) == list(range(len(gops)))          # index within the level


def test_slots(plans):
    for (n, keyint, _, cuts, intra, rate), (p, sc) in plans.items():
        starts = list(p["gop_start"])
        gop_of = {f: max(k for k, s in enumerate(starts) if s <= f) for f in range(n)}
        prev_dst = {}
        for j, sl in enumerate(_levels(p)):
            ent = p["sent"][sl]
            ks = [gop_of[int(f)] for f in ent[:, 0]]
            assert list(ent[:, 2]) == [2 * k + (j & 1) for k in ks]
            assert list(ent[:, 1]) == [-1 if j == 1 and not intra else 2 * k + ((j - 1) & 1) for k in ks]
            assert len(set(ent[:, 2])) == len(ent)          # no two entries of a level share a dst slot
            if j >= 1 and not (j == 1 and not intra):      # the ref slots: the previous level's dst slots of the same GOPs
                assert [int(r) for r in ent[:, 1]] == [prev_dst[k] for k in ks]
            prev_dst = {k: int(d) for k, d in zip(ks, ent[:, 2])}


def test_previous_level_index(plans):
    differs = 0
    for (n, keyint, _, cuts, intra, rate), (p, sc) in plans.items():
        lv = _levels(p)
        if not rate:
            assert np.all(p["sent"][:, 3] == 0)
            continue
        assert np.all(p["sent"][lv[0], 3] == 0)
        for j in range(1, p["maxlen"]):
            prev = p["went"][lv[j - 1]]
            for i, (f, _, _, w) in enumerate(p["sent"][lv[j]]):
                assert prev[w, 0] == f - 1 and prev[w, 3] == w
                differs += int(w != i)
    assert differs > 0   # GOPs of different lengths: the index moves between levels
    # the issue's example: a cut at frame 5 of 50 with keyint 33
    p, _ = plans[(50, 33, "five", True, False, 3)]
    assert list(p["gop_start"]) == [0, 5, 38]
    assert any(w != i for j in range(1, p["maxlen"]) for i, w in enumerate(p["sent"][_levels(p)[j], 3]))


def test_chunks_and_ring(lib, plans):
    ring, per = lib.eph_ring(), lib.eph_chunk_levels()
    assert (ring, per) == (32, 16) and ring % per == 0
    for (n, keyint, *_), (p, sc) in plans.items():
        ch, off = p["chunks"], p["lvl_off"]
        assert len(ch) == -(-p["maxlen"] // per)
        assert ch[0, 0] == 0 and ch[-1, 1] == p["maxlen"] and np.all(ch[1:, 0] == ch[:-1, 1])   # they tile the levels
        assert np.all(ch[:, 1] > ch[:, 0]) and np.all(ch[:, 1] - ch[:, 0] <= per)
        assert p["max_chunk"] == max(int(off[b] - off[a]) for a, b in ch)
        for j in range(ring, p["maxlen"]):
            w = lib.eph_chunk_freeing(j)
            assert ch[w, 0] <= j - ring < ch[w, 1]          # the chunk it waits for holds level j - ring
            # the driver queues level j in enqueue_searches(end(c) + ring), right after it has queued chunk c's
            # write: c is the first chunk with j < end(c) + ring.  The chunk waited for is written by then
            # (w <= c), so it is below c + 1, the next chunk to be written, whose event is not recorded yet
            c = next(c for c, (_, b) in enumerate(ch) if j < b + ring)
            assert w <= c
    assert any(p["maxlen"] > ring for p, _ in plans.values())


def test_sanitizer_run_of_the_stand_alone_driver(tmp_path):
    """enc_plan_main.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, run as a program."""
    exe = tmp_path / "enc_plan_main"
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *FLAGS,
                        str(NATIVE / "enc_plan_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the compiler has no sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "enc_plan_main: ok" in run.stdout, run.stdout[-1000:] + run.stderr[-3000:]
