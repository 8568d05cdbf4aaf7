"""The ratio-1 ingest kernel's dword clamp on the CPU (no GPU).

`ingest_nv12` (csrc/downscale.hip) makes every sample max(s, 1), four bytes at
a time, with `clamp_min1_x4` of csrc/pixel_clamp.h.  The stand-alone program
tests/native/ingest_clamp_main.cpp compiles that header for the host and writes
its result for every dword whose bytes come from {0, 1, 2, 0x7f, 0x80, 0xff}
and for every 16-bit low half under each high half made of those bytes; each
must equal the per-byte max(b, 1) computed here.

No stream test can stand in for this: the synthetic streams never put a 0x01
sample above a 0x00 one in a dword, which is where the well-known
`(v - 0x01010101) & ~v & 0x80808080` zero-byte test goes wrong (its borrow
marks the 0x01), and that case is pinned below too."""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
SET = np.array([0, 1, 2, 0x7F, 0x80, 0xFF], np.uint32)


def _inputs() -> np.ndarray:
    b3, b2, b1, b0 = np.meshgrid(SET, SET, SET, SET, indexing="ij")
    first = (b3 << 24 | b2 << 16 | b1 << 8 | b0).reshape(-1)
    h3, h2, lo = np.meshgrid(SET, SET, np.arange(65536, dtype=np.uint32), indexing="ij")
    second = (h3 << 24 | h2 << 16 | lo).reshape(-1)
    return np.concatenate([first, second]).astype(np.uint32)


def _per_byte(v: np.ndarray) -> np.ndarray:
    b = v.view(np.uint8).reshape(-1, 4)
    return np.maximum(b, 1).astype(np.uint8).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    d = tmp_path_factory.mktemp("clamp")
    exe, out = d / "ingest_clamp_main", d / "out.bin"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(ROOT / "video-transformer_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "ingest_clamp_main.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe), str(out)], capture_output=True, text=True)
    return run, np.fromfile(out, np.uint32) if out.exists() else None


def test_every_test_dword_is_clamped_per_byte(result):
    run, got = result
    assert run.returncode == 0, run.stderr
    v = _inputs()
    assert v.size == 6 ** 4 + 36 * 65536 and run.stdout.split()[0] == str(v.size)
    assert got is not None and got.size == v.size
    want = _per_byte(v)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"0x{int(v[bad[0]]):08x}: 0x{int(got[bad[0]]):08x}, per byte 0x{int(want[bad[0]]):08x}"
    # the inputs hold what matters: a 0x01 above a 0x00 in every byte position, and all-zero / no-zero dwords
    for shift in (0, 8, 16):
        assert ((v >> shift) & 0xFFFF == 0x0100).any()
    assert (v == 0).any() and (want == v).any() and (want != v).any()


def test_the_borrowing_zero_byte_test_is_not_exact():
    """Why the header does not use it: its mask calls the 0x01 of 0x0100 a zero byte, so whatever is done with
    the mask has to be harmless on a 0x01; the header's mask marks the zero bytes and nothing else."""
    v = _inputs()
    zero = np.zeros_like(v)
    for shift in (0, 8, 16, 24):
        zero |= (((v >> shift) & 0xFF) == 0).astype(np.uint32) << np.uint32(shift + 7)
    borrowing = (v - np.uint32(0x01010101)) & ~v & np.uint32(0x80808080)
    exact = ~(((v & np.uint32(0x7F7F7F7F)) + np.uint32(0x7F7F7F7F)) | v) & np.uint32(0x80808080)
    assert np.array_equal(exact, zero)
    i = int(np.nonzero(v == 0x0100)[0][0])
    assert int(borrowing[i]) == 0x80808080 and int(zero[i]) == 0x80800080
    assert (borrowing != zero).any()
