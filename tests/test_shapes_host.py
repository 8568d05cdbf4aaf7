"""Edge picture shapes through the general decoder's own code on the CPU.

The suite's other streams are all landscape and at most 68 macroblock rows
tall.  Here: pictures of one macroblock, one row, one column (no left, top or
any neighbour), and tall narrow pictures whose height alone selects the 2-, 3-
and 4-wave forms of h264_derive and a second, third and fourth pass of the
deblocking wavefront.  The device code (parse_full.h, recon_full.h,
intra_lanes.h, driven by tests/native/full_host.cpp) must equal the oracle
before and after the deblocking filter, and the filter must be active.  The
GPU counterpart is tests/test_shapes_gpu.py."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
from vtseg import scene

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "video-transformer_amd" / "csrc"

# display size (mbw x mbh)
SHAPES = [
    (16, 16),      # 1x1: no neighbours at all
    (272, 16),     # 17x1: single row, one full block of 16 macroblocks and a tail of 1
    (1024, 16),    # 64x1
    (16, 1040),    # 1x65: second deblock pass of one row, 2-wave derive, no left neighbour
    (32, 1104),    # 2x69: full second pass plus one row
    (48, 2064),    # 3x129: third pass, 3-wave derive
    (64, 4096),    # 4x256: the tallest picture derive_launch accepts
]
KINDS = {
    "cavlc": dict(coding="full"),
    "cavlc_b": dict(coding="full", bframes=True, weighted="implicit", temporal_direct=True),
    "cabac_b": dict(coding="full", cabac=True, bframes=True, transform_8x8=True, weighted="implicit",
                    slices_per_row=0),
}
COMMON = dict(n_frames=12, seed=7, max_motion=4, cut_min_s=0.1, cut_max_s=0.3, gop_max_s=0.2)


@pytest.fixture(scope="module")
def harness_lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("fhs") / "libfullhost.so"
    srcs = [ROOT / "tests" / "native" / "full_host.cpp"] + [CSRC / f for f in
                                                             ("mp4.cpp", "h264.cpp", "h264_sched.cpp",
                                                              "plan.cpp")]
    subprocess.run(["g++", "-O1", "-std=c++20", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-pthread",
                    f"-I{CSRC}", f"-I{ROOT / 'include'}", *map(str, srcs), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.fh_decode.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_char_p, C.c_int]
    lib.fh_shape_error.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int]
    return lib


@pytest.fixture(scope="module")
def harness(harness_lib):
    lib = harness_lib

    def decode(path, flags, n, W, H):
        w, h = C.c_int(0), C.c_int(0)
        cap = n * W * H * 3 // 2
        out = np.zeros(cap, np.uint8)
        got = C.c_int64(0)
        err = C.create_string_buffer(256)
        rc = lib.fh_decode(str(path).encode(), flags, out.ctypes.data, cap, C.byref(got),
                           C.byref(w), C.byref(h), err, 256)
        if rc:
            raise RuntimeError(err.value.decode())
        assert (w.value, h.value) == (W, H)
        return out[:got.value * W * H * 3 // 2].reshape(got.value, H * 3 // 2, W)
    return decode


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
@pytest.mark.parametrize("kind", list(KINDS))
def test_edge_shapes_on_cpu_equal_oracle(tmp_path, harness, kind, shape):
    W, H = shape
    n = COMMON["n_frames"]
    path = tmp_path / f"{kind}_{W}x{H}.mp4"
    scene.synth_write(path, width=W, height=H, **COMMON, **KINDS[kind])
    filtered, _ = oracle.decode_full(path, flags=0)
    unfiltered, _ = oracle.decode_full(path, flags=1)
    assert filtered.shape == (n, H * 3 // 2, W)
    assert not np.array_equal(filtered, unfiltered), "the deblocking filter changed nothing"
    # by-block intra, lane-parallel intra, and for CABAC the exact arena
    runs = [(1, unfiltered), (0, filtered), (2, filtered)]
    if kind == "cabac_b":
        runs += [(9, unfiltered), (8, filtered)]
    for flags, want in runs:
        got = harness(path, flags, n, W, H)
        assert got.shape == want.shape
        bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(1))[0]
        assert bad.size == 0, f"flags {flags}: frames {bad[:8].tolist()} differ"


def test_session_guard_refuses_from_the_model_threshold(harness_lib):
    """general_shape_error(), what the session calls at open: the shipped
    16-wave deblocking hand-off deadlocks from 331 macroblocks a row on once
    the picture has a whole row group in its second pass, 16 later with one to
    three rows there, never with one pass (tests/test_dbk_sched_host.py: the
    model and dp_shape_ok); h264_derive takes 256 rows."""
    def refused(mbw, mbh):
        err = C.create_string_buffer(256)
        rc = harness_lib.fh_shape_error(mbw, mbh, err, 256)
        assert (rc != 0) == bool(err.value)
        return err.value.decode()
    T = 331
    assert refused(T - 1, 68) == "" and refused(T - 1, 69) == "" and refused(T - 1, 256) == ""
    assert "at most 330 macroblocks per row" in refused(T, 68)
    assert "at most 330 macroblocks per row" in refused(T, 69)      # the GPU test's stream
    assert "330" in refused(T, 256) and "330" in refused(1024, 68)
    assert refused(T + 15, 65) == "" and refused(T + 15, 67) == ""
    assert "at most 346 macroblocks per row" in refused(T + 16, 65)
    assert "346" in refused(T + 16, 67)
    assert refused(1024, 64) == "" and refused(1024, 1) == ""
    assert refused(360, 180) != ""            # 5760x2880
    assert refused(240, 135) == ""            # 3840x2160
    assert refused(320, 69) == ""             # 5120x1104
    assert "at most 256" in refused(4, 257) and refused(4, 256) == ""
    for w, h in SHAPES:                       # every shape this module and the GPU module decode
        assert refused(w // 16, h // 16) == ""
