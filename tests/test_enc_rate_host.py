"""The motion search's rate-aware decisions on the CPU (no GPU).

`csrc/enc_rate.h` holds what `enc_search` decides with when `mvcost` or
`early_skip` is on: the length of se(v), the Lagrangian table, the candidate
key, the predictor guess from a command word, and the "no level survives"
predicate of the early P_Skip probe.  The harness
(tests/native/enc_rate_host.cpp) exposes the header's functions; their values
are compared with ones restated here."""
from __future__ import annotations

import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "video-transformer_amd" / "csrc"

PCM = 0x80008000
INTRA = 0x80000000


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("erh") / "libencratehost.so"
    subprocess.run(["g++", "-Og", "-std=c++20", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                    f"-I{CSRC}", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "native" / "enc_rate_host.cpp"),
                    "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.erh_key.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32]
    lib.erh_key.restype = C.c_uint64
    lib.erh_key_of.argtypes = [C.c_uint32] * 3
    lib.erh_key_of.restype = C.c_uint64
    lib.erh_key_index.argtypes = lib.erh_key_sad.argtypes = [C.c_uint64]
    lib.erh_key_index.restype = lib.erh_key_sad.restype = C.c_uint32
    lib.erh_pred.argtypes = [C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.erh_probe.argtypes = [C.POINTER(C.c_int), C.c_int]
    return lib


def _se(k: int) -> str:
    """se(v) of k as a bit string (9.1, 9.1.1)."""
    code = 2 * abs(k) - (1 if k > 0 else 0)
    info = bin(code + 1)[2:]
    return "0" * (len(info) - 1) + info


def test_selen_is_the_length_of_the_exp_golomb_string(lib):
    assert _se(0) == "1" and _se(1) == "010" and _se(-1) == "011" and _se(2) == "00100"
    for k in range(-300, 301):
        assert lib.erh_selen(k) == len(_se(k)), k
    for dx, dy in ((0, 0), (1, -1), (-300, 17), (64, 64)):
        assert lib.erh_mv_bits(dx, dy) == len(_se(dx)) + len(_se(dy))


def test_lambda_table_is_the_formula(lib):
    for qp in range(52):
        assert lib.erh_lambda16(qp, 0) == int(16 * math.sqrt(0.85 * 2 ** ((qp - 12) / 3)) + 0.5), qp
    assert lib.erh_lambda16(28, 0) == 94      # 93.66 rounded
    assert lib.erh_lambda16(28, 47) == 47 and lib.erh_lambda16(0, 4096) == 4096


def test_key_order(lib):
    lam = 94
    k = lambda sad, v, i, p=(0, 0): lib.erh_key(sad, lam, v[0], v[1], p[0], p[1], i)
    # the cost is 16 SAD + lambda16 bits(v - p)
    key = k(1234, (8, -12), 777, (4, 4))
    assert key >> 32 == 16 * 1234 + lam * (len(_se(4)) + len(_se(-16)))
    # the SAD rides below the index, and both come back out
    assert lib.erh_key_index(key) == 777 and lib.erh_key_sad(key) == 1234
    # equal cost: the lower index wins, the centre (0) first, then raster order
    assert k(100, (4, 0), 0) < k(100, (4, 0), 1) < k(100, (4, 0), 2) < k(100, (4, 0), 1088)
    # ... whatever the SADs underneath: 16 * 10 + 16 * 2 = 16 * 8 + 16 * 4 = 192
    a, b = lib.erh_key(10, 16, 0, 0, 0, 0, 3), lib.erh_key(8, 16, 1, 0, 0, 0, 2)
    assert a >> 32 == b >> 32 == 192 and b < a
    # a cost difference of 1 beats any index (and any SAD below it)
    for cost in (0, 1, 322, (1 << 21) - 2):
        assert lib.erh_key_of(cost, 0xffff, 0xffff) < lib.erh_key_of(cost + 1, 0, 0)
    # a vector nearer the predictor wins against a slightly lower SAD ...
    assert k(100, (8, 8), 5, (8, 8)) < k(99, (0, 0), 0, (8, 8))
    # ... and with lambda 0 the order is the SAD's
    assert lib.erh_key(5, 0, 64, 64, 0, 0, 9) < lib.erh_key(6, 0, 0, 0, 0, 0, 0)


def _pred(lib, word, mx, j):
    out = (C.c_int * 2)()
    lib.erh_pred(word, mx, j, out)
    return out[0], out[1]


def test_predictor_guess(lib):
    vec = lambda x, y: (x & 0xffff) | ((y & 0xffff) << 16)
    w = vec(-7, 13)
    assert _pred(lib, w, 3, 2) == (-7, 13)                 # a negative-component vector
    assert _pred(lib, vec(5, -32), 1, 9) == (5, -32)
    assert _pred(lib, w, 0, 2) == (0, 0)                   # mx = 0: the writer's own predictor
    assert _pred(lib, w, 3, 1) == (0, 0)                   # j = 1: the previous picture is the IDR
    assert _pred(lib, PCM, 3, 2) == (0, 0)                 # I_PCM
    assert _pred(lib, INTRA | 0x2f6, 3, 2) == (0, 0)       # Intra16x16 (modes, cbp in the low bits)
    assert _pred(lib, INTRA, 3, 2) == (0, 0)
    assert _pred(lib, 0, 3, 2) == (0, 0)                   # P_Skip


def test_probe_thresholds_at_qp_28(lib):
    """quant1: a level is non-zero iff |w| MF >= (5/6) 2^qbits.  qp 28: qbits
    19, MF(0,0) 8192, so a DC coefficient w is coded from |w| >= 54 (5/6 2^19 /
    8192 = 53.3).  A flat residual r has w(0,0) = 16 r and nothing else."""
    def probe(x):
        arr = (C.c_int * 16)(*[int(v) for v in x])
        return lib.erh_probe(arr, 28)
    assert probe([1] * 16) == 0                            # w = 16: nothing, luma or chroma
    # +3: w = 48 < 54: no luma and no chroma AC level; the chroma DC Hadamard of four such blocks is 192,
    # quantised at qbits + 1: 192 * 8192 >= 5/6 2^20, a level
    assert probe([3] * 16) == 4
    # a DC coefficient of 54: a level
    x = np.zeros(16, int)
    x[:6] = 9
    assert x.sum() == 54 and probe(x) & 1
    assert probe(np.zeros(16, int)) == 0
