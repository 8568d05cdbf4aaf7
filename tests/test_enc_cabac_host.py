"""The device encoder's CABAC writer on the CPU (no GPU).

`csrc/enc_cabac.h` holds what the `enc_write_cabac` kernel writes with: the
arithmetic encoder of 9.3.4, the context initialisation of 9.3.1.1 and one
function per syntax element.  The harness (tests/native/enc_cabac_host.cpp)
exposes them.

  engine:   seeded sequences of decisions, bypass and terminate bins are
            encoded by the header and by the restatement of Figures 9-7 ..
            9-12 below; the bytes are equal, and the restated decoder of
            9.3.3.2 returns the bins.
  contexts: the I and the cabac_init_idc 0 columns against the formula.
  slices:   seeded macroblock rows of every kind the encoder has are written
            as CABAC through the header and as CAVLC through `csrc/enc_cavlc.h`,
            the header the `enc_write` kernel calls; the CPU oracle's general
            decoder gives the same pictures for both.
  sinks:    the kernels' dword sink against the byte sink (`csrc/enc_rbsp.h`).
"""
from __future__ import annotations

import ctypes as C
import re
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
INTRA = 0x80000000
NCTX = 277
SRCS = [CSRC / f for f in ("synth.cpp", "synth_full.cpp", "mp4.cpp", "plan.cpp")]
FLAGS = ["-std=c++20", "-Wno-unknown-pragmas", "-pthread", f"-I{CSRC}", f"-I{ROOT / 'include'}", f"-I{NATIVE}"]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("ech") / "libenccabachost.so"
    subprocess.run(["g++", "-Og", "-fPIC", "-shared", *FLAGS, str(NATIVE / "enc_cabac_host.cpp"),
                    *map(str, SRCS), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.ech_engine.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    L.ech_engine.restype = C.c_int64
    L.ech_contexts.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.ech_sps_pps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ech_pictures.argtypes = [C.c_int] * 6 + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]
    L.ech_pictures.restype = C.c_int64
    L.ech_sinks.argtypes = [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 3
    return L


# ------------------------------------------------------------- the tables
def _macro(name: str) -> list[int]:
    """The integers of a data macro of h264_cabac_tables.h (field-coding zero blocks expanded)."""
    text = (CSRC / "h264_cabac_tables.h").read_text()
    body = re.search(r"#define " + name + r"\s*\\\n(.*?)\n\n", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = body.replace("VTS_CABAC_FIELD_ZEROS_277_398", "0, 0, " * 122).replace("VTS_CABAC_FIELD_ZEROS_436_459", "0, 0, " * 24)
    return [int(x) for x in re.findall(r"-?\d+", body)]


RANGE_LPS = np.array(_macro("VTS_CABAC_RANGE_LPS_DATA")).reshape(64, 4)
TRANS_LPS = _macro("VTS_CABAC_TRANS_LPS_DATA")
INIT = {1: np.array(_macro("VTS_CABAC_INIT_I_DATA")).reshape(460, 2),
        0: np.array(_macro("VTS_CABAC_INIT_P0_DATA")).reshape(460, 2)}


def contexts(islice: int, qp: int) -> list[int]:
    """9.3.1.1: preCtxState = Clip3(1, 126, ((m * Clip3(0, 51, SliceQPY)) >> 4) + n)."""
    st = []
    for m, n in INIT[islice][:NCTX]:
        pre = min(126, max(1, ((int(m) * min(51, max(0, qp))) >> 4) + int(n)))
        st.append((63 - pre) << 1 if pre <= 63 else ((pre - 64) << 1) | 1)
    return st


# ---------------------------------------- Figures 9-7 .. 9-12, restated
class Enc:
    def __init__(self, st):
        self.st = [(s >> 1, s & 1) for s in st]
        self.bits: list[int] = []
        self.start()

    def start(self):                        # 9.3.4.1
        self.low, self.range, self.first, self.outstanding = 0, 510, True, 0

    def put(self, b):                       # Figure 9-10
        if self.first:
            self.first = False
        else:
            self.bits.append(b)
        self.bits.extend([1 - b] * self.outstanding)
        self.outstanding = 0

    def renorm(self):                       # Figure 9-9
        while self.range < 256:
            if self.low < 256:
                self.put(0)
            elif self.low >= 512:
                self.low -= 512
                self.put(1)
            else:
                self.low -= 256
                self.outstanding += 1
            self.range <<= 1
            self.low <<= 1

    def decision(self, ctx, b):             # Figure 9-7
        p, mps = self.st[ctx]
        lps = int(RANGE_LPS[p][(self.range >> 6) & 3])
        self.range -= lps
        if b != mps:
            self.low += self.range
            self.range = lps
            if p == 0:
                mps = 1 - mps
            p = TRANS_LPS[p]
        else:
            p = min(p + 1, 62)
        self.st[ctx] = (p, mps)
        self.renorm()

    def bypass(self, b):                    # Figure 9-11
        self.low <<= 1
        if b:
            self.low += self.range
        if self.low >= 1024:
            self.put(1)
            self.low -= 1024
        elif self.low < 512:
            self.put(0)
        else:
            self.low -= 512
            self.outstanding += 1

    def terminate(self, b):                 # Figure 9-12, 9.3.4.5
        self.range -= 2
        if b:
            self.low += self.range
            self.range = 2
            self.renorm()
            self.put((self.low >> 9) & 1)
            self.bits.extend([(self.low >> 8) & 1, 1])
        else:
            self.renorm()


def ebsp(bits: list[int]) -> bytes:
    bits = bits + [0] * (-len(bits) % 8)
    raw = np.packbits(np.array(bits, np.uint8)).tobytes() if bits else b""
    out, zeros = bytearray(), 0
    for b in raw:
        if zeros >= 2 and b <= 3:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def rbsp(data: bytes) -> list[int]:
    out, zeros = bytearray(), 0
    for b in data:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return np.unpackbits(np.frombuffer(bytes(out), np.uint8)).tolist()


class Dec:                                  # 9.3.1.2, 9.3.3.2
    def __init__(self, st, bits):
        self.st = [(s >> 1, s & 1) for s in st]
        self.b, self.at = bits + [0] * 32, 0
        self.start()

    def read(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.b[self.at]
            self.at += 1
        return v

    def start(self):
        self.range, self.offset = 510, self.read(9)

    def renorm(self):
        while self.range < 256:
            self.range <<= 1
            self.offset = (self.offset << 1) | self.read(1)

    def decision(self, ctx):
        p, mps = self.st[ctx]
        lps = int(RANGE_LPS[p][(self.range >> 6) & 3])
        self.range -= lps
        if self.offset >= self.range:
            b = 1 - mps
            self.offset -= self.range
            self.range = lps
            if p == 0:
                mps = 1 - mps
            p = TRANS_LPS[p]
        else:
            b = mps
            p = min(p + 1, 62)
        self.st[ctx] = (p, mps)
        self.renorm()
        return b

    def bypass(self):
        self.offset = (self.offset << 1) | self.read(1)
        if self.offset >= self.range:
            self.offset -= self.range
            return 1
        return 0

    def terminate(self):
        self.range -= 2
        if self.offset >= self.range:
            return 1
        self.renorm()
        return 0


def _ops(rng, n, with_pcm):
    """(kind, a, b) triples as ech_engine reads them: biased towards a few contexts, with
    runs of the most probable symbol (outstanding bits build up while low sits near the
    middle) and, with_pcm, a terminate(1), alignment, raw bytes and a restart."""
    ops = []
    while len(ops) < n:
        k = rng.integers(0, 12)
        if k < 6:
            ops.append((0, int(rng.integers(0, NCTX - 1)), int(rng.random() < 0.3)))
        elif k < 8:                          # a run on one context: mostly its likely value
            ctx, v = int(rng.integers(60, 110)), int(rng.integers(0, 2))
            ops += [(0, ctx, v if rng.random() < 0.97 else 1 - v) for _ in range(int(rng.integers(20, 400)))]
        elif k < 10:                         # a bypass run: alternating bins keep low near the middle
            ops += [(1, 0, int(rng.integers(0, 2))) for _ in range(int(rng.integers(1, 40)))]
            ops += [(1, 0, i & 1) for i in range(int(rng.integers(0, 64)))]
        elif k == 10:
            ops.append((2, 0, 0))
        elif with_pcm:
            ops += [(2, 0, 1), (4, 0, 0)]
            ops += [(3, int(rng.integers(1, 256)), 0) for _ in range(int(rng.integers(1, 48)))]
            ops.append((5, 0, 0))
    ops.append((2, 0, 1))
    return ops


def _restated(ops, st):
    """The bytes of the sequence by the restatement: the engine's bits, then at a raw byte the bits so far
    are final (ech_engine aligned them); emulation prevention runs over the whole stream."""
    e = Enc(st)
    for k, a, b in ops:
        if k == 0:
            e.decision(a, b)
        elif k == 1:
            e.bypass(b)
        elif k == 2:
            e.terminate(b)
        elif k == 3:
            e.bits.extend(int(x) for x in np.unpackbits(np.array([a], np.uint8)))
        elif k == 4:
            e.bits.extend([0] * (-len(e.bits) % 8))
        else:
            e.start()
    return ebsp(e.bits)


@pytest.mark.parametrize("seed,islice,qp,with_pcm", [(1, 1, 28, False), (2, 0, 28, False), (3, 1, 0, True),
                                                    (4, 0, 51, True), (5, 0, 33, True), (6, 1, 17, True)])
def test_engine_bytes_equal_the_restated_figures_and_decode_back(lib, seed, islice, qp, with_pcm):
    rng = np.random.default_rng(seed)
    ops = _ops(rng, 6000, with_pcm)
    arr = np.array(ops, np.int32)
    out = np.zeros(len(ops) * 2 + 64, np.uint8)
    n = lib.ech_engine(arr.ctypes.data, len(ops), islice, qp, out.ctypes.data, out.size)
    assert n > 0
    got = out[:n].tobytes()
    st = contexts(islice, qp)
    assert got == _restated(ops, st)
    # one byte less: the overflow is reported and nothing lands past the end
    short = np.full(n + 8, 0xAB, np.uint8)
    assert lib.ech_engine(arr.ctypes.data, len(ops), islice, qp, short.ctypes.data, n - 1) == -1
    assert (short[n - 1:] == 0xAB).all()
    # the restated decoder reads the same bins back, byte-aligned raw bytes included
    d = Dec(st, rbsp(got))
    for i, (k, a, b) in enumerate(ops):
        if k == 0:
            assert d.decision(a) == b, f"op {i}"
        elif k == 1:
            assert d.bypass() == b, f"op {i}"
        elif k == 2:
            assert d.terminate() == b, f"op {i}"
            if b:                            # the 9 + shifts bits read so far end in the flush's last 1
                assert d.b[d.at - 1] == 1
        elif k == 3:
            assert d.read(8) == a, f"op {i}"
        elif k == 4:
            d.at += -d.at % 8
        else:
            d.start()


def test_outstanding_bits_run_past_one_word(lib):
    """Bypass bins chosen so that low stays in [512, 1024): 100 outstanding bits, resolved at the flush."""
    st = contexts(1, 28)
    e, ops = Enc(st), [(1, 0, 1)]
    e.bypass(1)                              # low = 510: from here a bin that keeps 2 low (+ range) in range exists
    for _ in range(100):
        b = 1 if 512 <= 2 * e.low + e.range < 1024 else 0
        assert 512 <= 2 * e.low + b * e.range < 1024
        e.bypass(b)
        ops.append((1, 0, b))
    assert e.outstanding == 100
    ops.append((2, 0, 1))
    arr = np.array(ops, np.int32)
    out = np.zeros(256, np.uint8)
    n = lib.ech_engine(arr.ctypes.data, len(ops), 1, 28, out.ctypes.data, out.size)
    assert out[:n].tobytes() == _restated(ops, st)


@pytest.mark.parametrize("qp", [0, 28, 51])
def test_context_initialisation_follows_the_formula(lib, qp):
    for islice in (1, 0):
        st = np.zeros(NCTX, np.uint8)
        lib.ech_contexts(islice, qp, st.ctypes.data)
        assert st.tolist() == contexts(islice, qp)


def test_sps_pps_say_main_and_cabac_and_the_default_is_unchanged(lib):
    import oracle
    sps, pps, n = np.zeros(64, np.uint8), np.zeros(64, np.uint8), np.zeros(2, np.int32)
    lib.ech_sps_pps(10, 6, 0, sps.ctypes.data, pps.ctypes.data, n.ctypes.data)
    base = (sps[:n[0]].tobytes(), pps[:n[1]].tobytes())
    assert base[0][1:3] == bytes([66, 0xC0])
    ref = oracle.sps_pps(10, 6, 0, 0, 30.0)              # the byte oracle's own SPS / PPS (level by fps)
    assert base[0][:3] == ref[0][:3] and base[0][4:] == ref[0][4:] and base[1] == ref[1]
    lib.ech_sps_pps(10, 6, 1, sps.ctypes.data, pps.ctypes.data, n.ctypes.data)
    main = (sps[:n[0]].tobytes(), pps[:n[1]].tobytes())
    assert main[0][1:3] == bytes([77, 0x40]) and main[0][3:] == base[0][3:]
    # PPS: ue(0) ue(0) then entropy_coding_mode_flag, the third bit
    assert main[1][1] == base[1][1] | 0x20 and main[1][2:] == base[1][2:]


# ------------------------------------------------------------ whole slices
def _rows(rng, mbw, mbh, npic, big):
    n = npic * mbh * mbw
    cmd, cbp = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    k = rng.integers(0, 40, (n, 384))
    coef = np.where(k < 27, 0, np.where(k < 35, rng.integers(-1, 2, k.shape),
                    np.where(k < 39, rng.integers(-20, 21, k.shape), rng.integers(-big, big + 1, k.shape)))).astype(np.int16)
    pcm = rng.integers(1, 256, (n, 384)).astype(np.uint8)
    kinds = []
    for a in range(n):
        idr, mx = a < mbh * mbw, a % mbw
        kind = int(rng.integers(0, 2)) if idr else int(rng.integers(0, 6))
        kinds.append(kind)
        if kind == 0:
            cmd[a] = PCM
        elif kind == 1:                      # Intra16x16: Horizontal / DC, both luma classes, chroma 0 / 1 / 2
            pm = 2 if mx == 0 else int(rng.integers(1, 3))
            cm = 0 if mx == 0 else int(rng.integers(0, 2))
            c = int(rng.choice([0, 15])) | (int(rng.integers(0, 3)) << 4)
            cmd[a] = INTRA | pm | (cm << 2) | (c << 4)
        elif kind == 2:
            cmd[a] = 0                       # P_Skip
        else:                                # inter, up to +-(4 * 16 + 3) quarter samples
            mv = rng.integers(-67, 68, 2)
            if kind == 3 and not mv.any():
                mv[0] = 67
            cmd[a] = (int(mv[0]) & 0xffff) | ((int(mv[1]) & 0xffff) << 16)
            cbp[a] = int(rng.integers(1, 48)) if kind >= 4 else 0
            if kind == 5:                    # sparse blocks: coded_block_flag 0 inside a coded 8x8
                coef[a, :256] *= np.repeat(rng.random(16) < 0.5, 16)
    return cmd, cbp, np.ascontiguousarray(coef), pcm, kinds


def _decode(lib, tmp, name, mbw, mbh, npic, qp, dbk, cabac, rows):
    import oracle
    cmd, cbp, coef, pcm, _ = rows
    out = np.zeros(npic * mbh * mbw * 9024 + 1024, np.uint8)
    sizes = np.zeros(npic, np.int64)
    n = lib.ech_pictures(mbw, mbh, npic, qp, dbk, cabac, cmd.ctypes.data, cbp.ctypes.data, coef.ctypes.data,
                         pcm.ctypes.data, out.ctypes.data, out.size, sizes.ctypes.data)
    assert n > 0
    at, samples = 0, []
    for s in sizes:
        samples.append(out[at:at + s].tobytes())
        at += int(s)
    sps, pps, k = np.zeros(64, np.uint8), np.zeros(64, np.uint8), np.zeros(2, np.int32)
    lib.ech_sps_pps(mbw, mbh, int(cabac != 0), sps.ctypes.data, pps.ctypes.data, k.ctypes.data)
    path = tmp / name
    oracle.write_mp4(path, sps[:k[0]].tobytes(), pps[:k[1]].tobytes(), samples, list(range(npic)), [0] * npic, 30,
                     16 * mbw, 16 * mbh)
    frames, _ = oracle.decode_full(path)
    return frames, n


@pytest.mark.parametrize("mbw", [1, 2, 10])
def test_slices_decode_to_the_pictures_of_the_same_rows_as_cavlc(lib, tmp_path, mbw):
    rng = np.random.default_rng(500 + mbw)
    seen, sizes = set(), [0, 0]
    for i, (qp, dbk, mbh) in enumerate([(10, 0, 1), (28, 1, 2), (40, 0, 1), (28, 0, 1), (33, 1, 1), (22, 0, 2)]):
        npic = 4
        rows = _rows(rng, mbw, mbh, npic, 1500 if qp == 10 else 200)
        seen |= set(rows[4])
        a, na = _decode(lib, tmp_path, f"v{i}.mp4", mbw, mbh, npic, qp, dbk, 0, rows)
        b, nb = _decode(lib, tmp_path, f"b{i}.mp4", mbw, mbh, npic, qp, dbk, 1, rows)
        assert a.shape == b.shape == (npic, 24 * mbh, 16 * mbw)
        assert np.array_equal(a, b), f"mbw {mbw} case {i}: the CABAC pictures differ from the CAVLC ones"
        # the kernel's path, the bins through BinRing and drain(): the same bytes
        _decode(lib, tmp_path, f"r{i}.mp4", mbw, mbh, npic, qp, dbk, 2, rows)
        assert (tmp_path / f"r{i}.mp4").read_bytes() == (tmp_path / f"b{i}.mp4").read_bytes()
        assert np.abs(rows[2]).max() >= 15
        sizes[0] += na
        sizes[1] += nb
    assert seen == set(range(6))             # every kind of macroblock was written
    print(f"mbw {mbw}: CAVLC {sizes[0]} bytes, CABAC {sizes[1]} bytes")


def _sinks(lib, idr, mbw, qp, dbk, row, cap, room):
    """ech_sinks into buffers of `room` bytes filled with 0xAB: (bytes, dword sink's bytes, res)."""
    cmd, cbp, coef, pcm = row
    by, wd, res = np.full(room, 0xAB, np.uint8), np.full(room // 4, 0xABABABAB, np.uint32), np.zeros(4, np.int64)
    lib.ech_sinks(idr, mbw, qp, dbk, cmd.ctypes.data, cbp.ctypes.data, coef.ctypes.data, pcm.ctypes.data, cap,
                  by.ctypes.data, wd.ctypes.data, res.ctypes.data)
    return by, wd.view(np.uint8), res.tolist()


def test_the_dword_sink_and_the_byte_sink_agree(lib):
    """The kernel's sink (four bytes per aligned dword store) against the harness's byte sink over the same
    CAVLC slices: the same bytes and length, with emulation prevention bytes and every length mod 4; short
    of the length by 1 .. 5 bytes both report the overflow and nothing is stored at or past `cap`."""
    residues, escaped = set(), 0
    for seed in range(24):
        rng = np.random.default_rng(900 + seed)
        mbw = (1, 2, 5)[seed % 3]
        cmd, cbp, coef, pcm, _ = _rows(rng, mbw, 1, 2, 1500 if seed % 4 == 0 else 60)
        pcm[rng.random(pcm.shape) < 0.5] = 0             # zero runs: emulation prevention inside the samples
        coef[rng.random(coef.shape) < 0.5] = 0
        for idr in (1, 0):                               # picture 0 holds the kinds of an I slice
            sl = slice(0, mbw) if idr else slice(mbw, 2 * mbw)
            row = tuple(np.ascontiguousarray(a[sl]) for a in (cmd, cbp, coef, pcm))
            room = mbw * 9024 + 64
            by, wd, (nb, ob, nw, ow) = _sinks(lib, idr, mbw, 20 + seed, seed & 1, row, room, room + 64)
            assert (ob, ow) == (0, 0) and nb == nw > 0
            full = by[:nb].tobytes()
            assert wd[:nb].tobytes() == full
            assert (by[nb:] == 0xAB).all() and (wd[(nb + 3) // 4 * 4:] == 0xAB).all()
            residues.add(nb % 4)
            escaped += full.count(b"\x00\x00\x03")
            for short in (1, 2, 3, 4, 5):
                cap = nb - short
                by, wd, (n1, o1, n2, o2) = _sinks(lib, idr, mbw, 20 + seed, seed & 1, row, cap, room + 64)
                assert (n1, o1, n2, o2) == (nb, 1, nb, 1), f"seed {seed} idr {idr} cap -{short}"
                assert (by[cap:] == 0xAB).all() and (wd[cap:] == 0xAB).all()
                assert by[:cap].tobytes() == full[:cap] and wd[:cap // 4 * 4].tobytes() == full[:cap // 4 * 4]
    assert residues == {0, 1, 2, 3} and escaped > 100


def test_sanitizer_run_of_the_stand_alone_driver(tmp_path):
    """enc_cabac_main.cpp under AddressSanitizer + UndefinedBehaviorSanitizer, run as a program."""
    exe = tmp_path / "enc_cabac_main"
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *FLAGS,
                        str(NATIVE / "enc_cabac_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the compiler has no sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "enc_cabac_main: ok" in run.stdout, run.stdout[-1000:] + run.stderr[-3000:]
