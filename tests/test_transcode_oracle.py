"""Upload transcode on the CPU side: the oracle's definition
checked for self-consistency, the output-size rule against ffmpeg's
scale=-2:H formula, and the drop-in's decision flow against the reference's
_compress_video_for_upload (content_analyzer.py:167-236)."""
from __future__ import annotations

import logging

import numpy as np
import pytest

import oracle
from vtseg import scene, upload


def _ffmpeg_minus2_width(W, H, h):
    """libavfilter scale_eval: w = av_rescale(h, W, H * 2) * 2, av_rescale
    rounding to nearest with ties away from zero."""
    from fractions import Fraction
    q = Fraction(h * W, H * 2)
    return int(q + Fraction(1, 2)) * 2


@pytest.mark.parametrize("W,H", [(1280, 720), (1920, 1080), (640, 480), (320, 240), (1366, 768),
                                 (720, 576), (3840, 2160), (854, 480), (426, 240)])
def test_small_width_is_ffmpeg_scale_minus2(W, H):
    assert oracle.small_width(W, H, 360) == _ffmpeg_minus2_width(W, H, 360)


def _box(frame, W, H, k):
    """Integer-ratio area filter = box mean, rounded half up, min 1."""
    y = frame[:H].astype(np.int64)
    uv = frame[H:].astype(np.int64)
    by = (y.reshape(H // k, k, W // k, k).sum(axis=(1, 3)) + k * k // 2) // (k * k)
    u = uv[:, 0::2].reshape(H // 2 // k, k, W // 2 // k, k).sum(axis=(1, 3))
    v = uv[:, 1::2].reshape(H // 2 // k, k, W // 2 // k, k).sum(axis=(1, 3))
    bu, bv = (u + k * k // 2) // (k * k), (v + k * k // 2) // (k * k)
    return np.maximum(by, 1), np.maximum(bu, 1), np.maximum(bv, 1)


@pytest.mark.parametrize("k", [2, 3])
def test_area_downscale_integer_ratio_is_box_mean(k):
    rng = np.random.default_rng(k)
    W, H = 96 * k, 64 * k
    fr = rng.integers(0, 256, (H * 3 // 2, W), dtype=np.uint8)
    fr[:8, :8] = 0  # zeros clamp to 1
    out = oracle.downscale_nv12(fr, W, H, 64)
    by, bu, bv = _box(fr, W, H, k)
    assert np.array_equal(out[:64, :96], by)
    assert np.array_equal(out[64:96, 0:96:2], bu)
    assert np.array_equal(out[64:96, 1:96:2], bv)
    assert out.min() >= 1


def test_area_downscale_fractional_ratio_matches_exact_weights():
    """640x480 -> 480x360: weights (3,1) (2,2) (1,3) per axis, total 16."""
    rng = np.random.default_rng(7)
    fr = rng.integers(1, 256, (720, 640), dtype=np.uint8)
    out = oracle.downscale_nv12(fr, 640, 480, 360)
    y = fr[:480].astype(np.int64)
    wts = [(0, (3, 1)), (1, (2, 2)), (2, (1, 3))]

    def ax(n_out):
        m = np.zeros((n_out, n_out * 4 // 3), np.int64)
        for o in range(n_out):
            base, (a, b) = (o // 3) * 4 + o % 3, wts[o % 3][1]
            m[o, base], m[o, base + 1] = a, b
        return m
    Mx, My = ax(480), ax(360)
    want = (My @ y @ Mx.T + 8) // 16
    assert np.array_equal(out[:360, :480], np.maximum(want, 1))
    assert np.array_equal(out[360, :480], out[359, :480])  # replicated padding rows


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    p = tmp_path_factory.mktemp("tc") / "clip.mp4"
    scene.synth_write(p, width=320, height=192, n_frames=90, cut_min_s=0.7, cut_max_s=1.5,
                      gop_max_s=0.5)
    frames, info = oracle.decode_file(p)
    sc = oracle.score_frames(frames.reshape(-1), frames[0].size, 90, 320, 192, 320, 192, 4,
                             want_rgb=False)["score"]
    return frames, sc, info


@pytest.mark.parametrize("T,R", [(768, 8), (0, 8), (768, 0), (-1, 8), (5000, 16)])
def test_oracle_round_trip_and_error_bound(clip, T, R):
    """The round-2 encoder (qp 0: no residual): I_PCM where the motion
    misses by more than T, every output decodes (subset decoder) to the
    encoder's reconstruction."""
    frames, sc, info = clip
    r = oracle.transcode(frames, 320, 192, sc, out_height=96, search_range=R, max_mb_sad=T,
                         want_recon=True, qp=0)
    cw, ch, sw, sh = r["coded_width"], r["coded_height"], r["width"], r["height"]
    sps, pps = oracle.sps_pps(cw // 16, ch // 16, cw - sw, ch - sh, 30.0)
    dec = oracle.decode_samples(sps, pps, r["samples"])
    rec = r["recon"]
    assert np.array_equal(dec, np.concatenate([rec[:, :sh, :sw], rec[:, ch:ch + sh // 2, :sw]], 1))
    ds = np.stack([oracle.downscale_nv12(f, 320, 192, 96) for f in frames])
    err = np.abs(ds.astype(np.int64) - rec.astype(np.int64))
    # per macroblock luma+chroma SAD <= T (T < 0: everything I_PCM, exact)
    for f in range(len(frames)):
        for my in range(ch // 16):
            for mx in range(cw // 16):
                s = err[f, my * 16:my * 16 + 16, mx * 16:mx * 16 + 16].sum() + \
                    err[f, ch + my * 8:ch + my * 8 + 8, mx * 16:mx * 16 + 16].sum()
                assert s <= max(T, 0)
    n_mb = len(frames) * (cw // 16) * (ch // 16)
    assert r["pcm_mbs"] + r["inter_mbs"] + r["skip_mbs"] == n_mb
    assert r["sync"][0] and r["sync"].sum() == r["n_idr"]
    if T < 0:
        assert r["pcm_mbs"] == n_mb


def _decode_full_samples(tmp_path, r, name="o.mp4"):
    cw, ch, sw, sh = r["coded_width"], r["coded_height"], r["width"], r["height"]
    sps, pps = oracle.sps_pps(cw // 16, ch // 16, cw - sw, ch - sh, 30.0)
    n = len(r["samples"])
    path = tmp_path / name
    oracle.write_mp4(path, sps, pps, r["samples"], [i * 1000 for i in range(n)], [0] * n, 30000, sw, sh)
    dec, _ = oracle.decode_full(path)
    return dec


@pytest.mark.parametrize("qp,R,T", [(28, 8, 1536), (20, 8, 1536), (36, 4, 1536), (28, 0, 1536),
                                    (28, 8, -1)])
def test_oracle_residual_coding_round_trip(tmp_path, clip, qp, R, T):
    """Residual coding (P_L0_16x16 + quantised 4x4 residual, CAVLC
    residual_block with nC from the left macroblock): the general oracle
    decoder reads the output back to exactly the encoder's reconstruction,
    every inter macroblock's residual bound stays within the I_PCM payload,
    and the result is smaller than the residual-free encoder's."""
    frames, sc, _ = clip
    r = oracle.transcode(frames, 320, 192, sc, out_height=96, search_range=R, max_mb_sad=T,
                         want_recon=True, qp=qp)
    cw, ch, sw, sh = r["coded_width"], r["coded_height"], r["width"], r["height"]
    rec = r["recon"]
    dec = _decode_full_samples(tmp_path, r)
    assert np.array_equal(dec, np.concatenate([rec[:, :sh, :sw], rec[:, ch:ch + sh // 2, :sw]], 1))
    n_mb = len(frames) * (cw // 16) * (ch // 16)
    assert r["pcm_mbs"] + r["inter_mbs"] + r["skip_mbs"] == n_mb
    if T < 0:
        assert r["pcm_mbs"] == n_mb
        return
    old = oracle.transcode(frames, 320, 192, sc, out_height=96, search_range=R, max_mb_sad=T, qp=0)
    assert sum(map(len, r["samples"])) < sum(map(len, old["samples"]))
    assert r["pcm_mbs"] <= old["pcm_mbs"]
    ds = np.stack([oracle.downscale_nv12(f, 320, 192, 96) for f in frames]).astype(np.float64)
    mse = np.mean((ds[:, :sh, :sw] - rec[:, :sh, :sw].astype(np.float64)) ** 2)
    assert 10 * np.log10(255.0 ** 2 / max(mse, 1e-9)) > 30.0


# ------------------ the opt-in paths: intra, subpel, deblock
# The oracle's own closed loop, before it judges the device
# (tests/test_transcode_bytes_gpu.py): the general oracle decoder, which has its
# own 8.3.3 / 8.4.2.2.1 / 8.7, reads the output back to the encoder's
# reconstruction, and the counts are consistent.

def _closed_loop(tmp_path, frames, W, H, sc, *, out_height, intra, subpel, deblock, **kw):
    r = oracle.transcode(frames, W, H, sc, out_height=out_height, want_recon=True, intra=bool(intra),
                         subpel=subpel, deblock=bool(deblock), **kw)
    cw, ch, sw, sh = r["coded_width"], r["coded_height"], r["width"], r["height"]
    rec = r["recon"]
    dec = _decode_full_samples(tmp_path, r)
    want = np.concatenate([rec[:, :sh, :sw], rec[:, ch:ch + sh // 2, :sw]], 1)
    bad = [i for i in range(len(want)) if not np.array_equal(dec[i], want[i])]
    assert bad == [], f"the oracle decoder differs from the encoder's reconstruction at frames {bad[:8]}"
    n_mb = len(frames) * (cw // 16) * (ch // 16)
    print({k: v for k, v in r.items() if k.endswith("_mbs") or k == "n_idr"}, sum(map(len, r["samples"])), "bytes")
    assert r["pcm_mbs"] + r["inter_mbs"] + r["skip_mbs"] + r["intra_mbs"] == n_mb
    assert 0 <= r["qpel_mbs"] <= r["subpel_mbs"] <= r["inter_mbs"]
    assert (r["subpel_mbs"] > 0) == (subpel > 0)
    assert r["qpel_mbs"] == 0 or subpel == 2
    assert (r["intra_mbs"] > 0) == bool(intra)
    if not deblock:
        assert r["deblock_mbs"] == 0
    return r


@pytest.mark.parametrize("deblock", [0, 1])
@pytest.mark.parametrize("subpel", [0, 1, 2])
@pytest.mark.parametrize("intra", [0, 1])
def test_oracle_optin_paths_closed_loop(tmp_path, clip, intra, subpel, deblock):
    frames, sc, _ = clip
    r = _closed_loop(tmp_path, frames, 320, 192, sc, out_height=96, intra=intra, subpel=subpel, deblock=deblock)
    if deblock:
        assert 0 < r["deblock_mbs"] <= len(frames) * 60   # qp 28
    if subpel == 2:
        assert r["qpel_mbs"] > 0
    if not (intra or subpel or deblock):
        # all off: today's bytes, through either entry
        old = oracle.transcode(frames, 320, 192, sc, out_height=96, want_recon=True)
        assert r["samples"] == old["samples"] and np.array_equal(r["recon"], old["recon"])
        assert (r["pcm_mbs"], r["inter_mbs"], r["skip_mbs"], r["n_idr"]) == \
            (old["pcm_mbs"], old["inter_mbs"], old["skip_mbs"], old["n_idr"])


def test_oracle_all_off_ex_entry_is_or_transcode(clip):
    """or_transcode_ex with every new argument zero writes or_transcode's
    bytes (oracle.transcode takes the old entry when nothing is set)."""
    import ctypes as C
    frames, sc, _ = clip
    old = oracle.transcode(frames, 320, 192, sc, out_height=96, want_recon=True, keyint=16, qp=28)
    F, cw, ch = len(frames), old["coded_width"], old["coded_height"]
    cap = sum(map(len, old["samples"])) + 64
    out, off, size = np.zeros(cap, np.uint8), np.zeros(F, np.int64), np.zeros(F, np.int64)
    sync, recon, stats = np.zeros(F, np.uint8), np.zeros((F, ch * 3 // 2, cw), np.uint8), np.zeros(8, np.int64)
    n = C.c_int64(0)
    fr, s32 = np.ascontiguousarray(frames, np.uint8), np.ascontiguousarray(sc, np.float32)
    rc = oracle.lib().or_transcode_ex(fr.ctypes.data, F, 320, 192, s32.ctypes.data, 0.08, 0, 96, 8, 1536, 16, 28,
                                      0, 0, 0, 0, 0, out.ctypes.data, cap, off.ctypes.data, size.ctypes.data,
                                      sync.ctypes.data, recon.ctypes.data, stats.ctypes.data, C.byref(n))
    assert rc == 0
    assert bytes(out[:n.value]) == b"".join(old["samples"])
    assert np.array_equal(recon, old["recon"])
    assert list(stats) == [old["pcm_mbs"], old["inter_mbs"], old["skip_mbs"], old["n_idr"], 0, 0, 0, 0]


def test_oracle_intra_deblock_high_qp(tmp_path, clip):
    """qp 40 with Intra16x16 and the filter: bS 4 / 3 edges and the strong
    filter (alpha' 101, beta' 13 pass on smooth content)."""
    frames, sc, _ = clip
    r = _closed_loop(tmp_path, frames, 320, 192, sc, out_height=96, intra=1, subpel=0, deblock=1, qp=40)
    assert r["deblock_mbs"] > 0


@pytest.mark.parametrize("R", [0, 16])
def test_oracle_subpel_at_the_range_limits(tmp_path, clip, R):
    """search_range 0 (the refinement is the whole search) and 16 (vectors up
    to 4 * 16 + 3 quarter samples, far over the clamped edges)."""
    frames, sc, _ = clip
    _closed_loop(tmp_path, frames, 320, 192, sc, out_height=96, intra=0, subpel=2, deblock=0, search_range=R)


def test_oracle_two_by_two_macroblocks(tmp_path):
    """64x48 -> 32x24, coded 32x32: every macroblock touches two picture edges
    and a row is the shortest chain that still has a left neighbour.
    max_motion 8 leaves the search misses that a P picture codes as intra."""
    p = tmp_path / "tiny.mp4"
    scene.synth_write(p, width=64, height=48, n_frames=40, cut_min_s=0.7, cut_max_s=1.5, gop_max_s=0.5,
                      max_motion=8)
    frames, _ = oracle.decode_file(p)
    sc = oracle.score_frames(frames.reshape(-1), frames[0].size, 40, 64, 48, 64, 48, 4, want_rgb=False)["score"]
    r = _closed_loop(tmp_path, frames, 64, 48, sc, out_height=24, intra=1, subpel=2, deblock=1, search_range=4)
    assert (r["coded_width"], r["coded_height"]) == (32, 32)
    assert r["deblock_mbs"] > 0


@pytest.mark.parametrize("on", [0, 1], ids=["off", "all_on"])
@pytest.mark.parametrize("name,W,H,h,geometry", [("portrait", 144, 256, 128, (72, 128, 80, 128)),
                                                 ("qcif", 176, 144, 72, (88, 72, 96, 80))])
def test_oracle_cropped_width(tmp_path, name, W, H, h, geometry, on):
    """A display width that is no multiple of 16 (what every portrait upload
    gives): the coded picture has columns right of the display edge, filled by
    the downscale's padding, searched, predicted and filtered like the rest
    and cropped by the SPS.  The sources of the byte tests
    (tests/test_transcode_bytes_gpu.py `portrait`, `qcif`)."""
    p = tmp_path / f"{name}.mp4"
    scene.synth_write(p, width=W, height=H, n_frames=20, cut_min_s=0.7, cut_max_s=1.5, gop_max_s=0.5)
    frames, _ = oracle.decode_file(p)
    sc = oracle.score_frames(frames.reshape(-1), frames[0].size, 20, W, H, W, H, 4, want_rgb=False)["score"]
    r = _closed_loop(tmp_path, frames, W, H, sc, out_height=h, intra=on, subpel=2 * on, deblock=on)
    assert (r["width"], r["height"], r["coded_width"], r["coded_height"]) == geometry
    if on:
        assert r["deblock_mbs"] > 0


def crafted_frames(F=12, W=96, H=64, seed=11):
    """Display-size NV12 frames (samples >= 1) whose P pictures need every
    decision: per macroblock and frame a ramp (the motion search predicts it),
    fresh noise (nothing predicts it: I_PCM at a low qp), or rows that are
    constant along x and new in every frame (the search misses, Intra16x16
    Horizontal predicts them from the left column)."""
    rng = np.random.default_rng(seed)
    fr = np.zeros((F, H * 3 // 2, W), np.uint8)
    for f in range(F):
        y = np.tile(np.linspace(60, 180, W).astype(np.uint8), (H, 1))
        uv = np.full((H // 2, W), 128, np.uint8)
        for my in range(H // 16):
            for mx in range(W // 16):
                kind = rng.integers(0, 4)
                ys, xs, cs = slice(my * 16, my * 16 + 16), slice(mx * 16, mx * 16 + 16), slice(my * 8, my * 8 + 8)
                if kind == 1:
                    y[ys, xs] = rng.integers(1, 256, (16, 16))
                    uv[cs, xs] = rng.integers(1, 256, (8, 16))
                elif kind == 2:
                    y[ys, xs] = rng.integers(1, 256, (16, 1))
                    uv[cs, xs] = np.repeat(rng.integers(1, 256, (8, 1, 2)), 8, 1).reshape(8, 16)
        fr[f, :H], fr[f, H:] = y, uv
    return np.maximum(fr, 1)


def noisy_frames(F=8, W=96, H=64, seed=5):
    """One textured picture plus seeded noise in {-1, 0, +1}, luma and chroma,
    samples kept in 1..254 (display-size NV12)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H * 3 // 2, 0:W]
    # smooth enough that a quarter-sample vector, whose prediction averages the reference's noise
    # away, beats the centre by a few units of SAD in some macroblocks (the CPU oracle: 134 of 168
    # P macroblocks stay P_Skip with subpel = 2, all 168 with subpel = 0)
    base = np.clip(128 + 60 * np.sin(xx / 11.0) * np.cos(yy / 9.0), 2, 253).astype(np.int16)
    fr = np.stack([base + rng.integers(-1, 2, base.shape) for _ in range(F)])
    assert fr.min() >= 1 and fr.max() <= 254
    return fr.astype(np.uint8)


def diagonal_frames(F=6, W=96, H=64, seed=3):
    """Display-size NV12 frames (samples >= 1) for the Intra_4x4 decisions:
    per macroblock a seeded kind: hard edges at one of eight angles (the
    directional modes 3 .. 8 predict them), a smooth ramp (DC and the predicted
    mode's discount), a constant (every mode predicts the same samples: cost
    ties, and I_NxN against Intra16x16 on few bits) or noise (nothing predicts
    it: at qp 1 both candidates pass 3072 bits).  The whole pattern moves by
    (3, 1) samples a frame, so the P pictures search, and every third frame has
    two macroblocks of fresh noise that the search misses (intra in a P slice)."""
    rng = np.random.default_rng(seed)
    mbw, mbh, pad = W // 16, H // 16, 32
    kinds = rng.integers(0, 12, (mbh + 4, mbw + 4))
    ang = rng.uniform(0, np.pi, kinds.shape)
    lo, hi = rng.integers(20, 110, kinds.shape), rng.integers(140, 250, kinds.shape)
    yy, xx = np.mgrid[0:H + 2 * pad, 0:W + 2 * pad]
    big = np.zeros(yy.shape, np.int64)
    for my in range(kinds.shape[0]):
        for mx in range(kinds.shape[1]):
            ys, xs = slice(my * 16, my * 16 + 16), slice(mx * 16, mx * 16 + 16)
            y, x, k = yy[ys, xs], xx[ys, xs], kinds[my, mx]
            if k < 7:      # stripes 5 samples wide across the direction ang
                t = np.floor((x * np.cos(ang[my, mx]) + y * np.sin(ang[my, mx])) / 5.0).astype(np.int64)
                big[ys, xs] = np.where(t & 1, hi[my, mx], lo[my, mx])
            elif k < 9:
                big[ys, xs] = lo[my, mx] + (x % 16) * 3 + (y % 16) * 2
            elif k < 11:
                big[ys, xs] = lo[my, mx]
            else:
                big[ys, xs] = rng.integers(1, 256, (16, 16))
    fr = np.zeros((F, H * 3 // 2, W), np.uint8)
    for f in range(F):
        oy, ox = pad // 2 + f, pad // 2 + 3 * f
        fr[f, :H] = big[oy:oy + H, ox:ox + W]
        c = big[oy:oy + H:2, ox:ox + W:2]
        fr[f, H:, 0::2], fr[f, H:, 1::2] = 128 + (c - 128) // 4, 128 - (c - 128) // 8
        if f % 3 == 2:
            for mx in (1, 4):
                fr[f, 16:32, mx * 16:mx * 16 + 16] = rng.integers(1, 256, (16, 16))
    return np.maximum(fr, 1)


@pytest.mark.parametrize("qp,kw", [(4, dict(subpel=0, deblock=0)),
                                   (12, dict(subpel=2, deblock=1, deblock_offsets=(6, 6))),
                                   (4, dict(subpel=2, deblock=1, deblock_offsets=(6, 6)))])
def test_oracle_p_pictures_with_every_macroblock_kind(tmp_path, qp, kw):
    """P pictures that mix inter, P_Skip, Intra16x16 and (at a low qp) I_PCM
    macroblocks: Intra16x16 with an inter or an I_PCM left neighbour (its
    prediction, its nC, mb_type + 5), the filter across I_PCM edges (qPp 0)."""
    fr = crafted_frames()
    sc = np.zeros(len(fr), np.float32)
    r = _closed_loop(tmp_path, fr, 96, 64, sc, out_height=64, intra=1, qp=qp, **kw)
    assert r["n_idr"] == 1 and r["inter_mbs"] > 0 and r["skip_mbs"] > 0 and r["pcm_mbs"] > 0
    if qp == 4:
        assert r["intra_mbs"] > 24          # more than the IDR picture's 6 x 4
    if qp == 12:
        assert r["deblock_mbs"] > 0         # indexA 24 between coded macroblocks, 18 beside I_PCM


class _Bits:
    """A bit string written by hand from 7.3.3 / 7.3.5 (the test's own, not the oracle's writer)."""

    def __init__(self):
        self.s = ""

    def u(self, n, v):
        self.s += format(v, f"0{n}b") if n else ""
        return self

    def ue(self, v):
        b = format(v + 1, "b")
        self.s += "0" * (len(b) - 1) + b
        return self

    def se(self, v):
        return self.ue(2 * v - 1 if v > 0 else -2 * v)

    def nal(self, header):
        s = self.s + "1"
        s += "0" * (-len(s) % 8)
        out, zeros = bytearray([header]), 0
        for i in range(0, len(s), 8):
            v = int(s[i:i + 8], 2)
            if zeros >= 2 and v <= 3:
                out.append(3)
                zeros = 0
            out.append(v)
            zeros = zeros + 1 if v == 0 else 0
        return len(out).to_bytes(4, "big") + bytes(out)


def test_oracle_ties_on_a_flat_picture(tmp_path):
    """Two frames of constant 128, where every decision is a tie, against
    slices written out by hand.  IDR picture: macroblock 0 of a row has no
    neighbour (Intra16x16 DC from 128, mb_type 3); to its right Horizontal and
    DC predict the same samples and the lower mode number, Horizontal, wins
    (mb_type 2); nothing is coded, so each macroblock is mb_type,
    intra_chroma_pred_mode 0 (DC, the lower of its tie), mb_qp_delta 0 and an
    empty Intra16x16DCLevel at nC 0 (coeff_token '1').  P picture: all 17
    sub-sample candidates of both steps have SAD 0, the centre wins, the vector
    stays (0, 0) and the row is one mb_skip_run."""
    W, H, mbw, mbh = 64, 32, 4, 2
    fr = np.full((2, H * 3 // 2, W), 128, np.uint8)
    r = oracle.transcode(fr, W, H, np.zeros(2, np.float32), out_height=H, want_recon=True, intra=True, subpel=2)
    assert (r["intra_mbs"], r["skip_mbs"], r["inter_mbs"], r["pcm_mbs"]) == (mbw * mbh, mbw * mbh, 0, 0)
    assert (r["subpel_mbs"], r["qpel_mbs"]) == (0, 0)
    assert np.array_equal(r["recon"], fr)
    idr, p = b"", b""
    for row in range(mbh):
        b = _Bits().ue(row * mbw).ue(7).ue(0).u(16, 0).ue(0).u(2, 0).se(28 - 26).ue(1)
        b.ue(3).ue(0).se(0).u(1, 1)
        for _ in range(mbw - 1):
            b.ue(2).ue(0).se(0).u(1, 1)
        idr += b.nal(0x65)
        p += _Bits().ue(row * mbw).ue(5).ue(0).u(16, 1).u(3, 0).se(28 - 26).ue(1).ue(mbw).nal(0x41)
    assert r["samples"][0] == idr
    assert r["samples"][1] == p
    assert np.array_equal(_decode_full_samples(tmp_path, r), fr)


def test_oracle_intra_of_all_pcm_p_pictures(tmp_path, clip):
    """max_mb_sad < 0 leaves every P macroblock to the intra pass: rows of
    Intra16x16 macroblocks in P slices."""
    frames, sc, _ = clip
    r = _closed_loop(tmp_path, frames[:30], 320, 192, sc[:30], out_height=96, intra=1, subpel=0, deblock=1,
                     max_mb_sad=-1)
    assert r["intra_mbs"] == 30 * 60


@pytest.mark.parametrize("at_cuts", [False, True])
def test_oracle_idr_at_keyint_and_optionally_cuts(clip, at_cuts):
    frames, sc, _ = clip
    r = oracle.transcode(frames, 320, 192, sc, out_height=96, keyint=7, idr_at_cuts=at_cuts)
    idr = np.nonzero(r["sync"])[0]
    last = 0
    for f in range(len(frames)):
        is_idr = f == 0 or (at_cuts and sc[f] > 0.08) or f - last >= 7
        last = f if is_idr else last
        assert bool(r["sync"][f]) == is_idr
    assert len(idr) == r["n_idr"]


# ------- the rules of or_transcode_ex2: mvcost, early_skip, intra4x4
# As above, the oracle is checked before it judges the device
# (tests/test_transcode_bytes_rate_intra4_gpu.py): (a) its output decodes, through
# h264_full_oracle.c's own 8.3.1.2 and CAVLC, to its own reconstruction; (b) the
# GPU cases make every rule decide; (c) it agrees with the product's CPU harness,
# a restatement by another hand; (d) with the new keywords at their defaults it
# writes or_transcode_ex's bytes.

PCM_WORD, I4_NONE = 0x80008000, np.uint64(0xFFFFFFFFFFFFFFFF)
NEW_RULES = {"mv": dict(mvcost=True), "es": dict(early_skip=True), "both": dict(mvcost=True, early_skip=True),
             "i4": dict(intra=True, intra4x4=True),
             "every": dict(intra=True, intra4x4=True, mvcost=True, early_skip=True)}


def _closed_loop_ex2(tmp_path, frames, W, H, sc, **kw):
    r = oracle.transcode(frames, W, H, sc, want_recon=True, want_words=True, **kw)
    cw, ch, sw, sh = r["coded_width"], r["coded_height"], r["width"], r["height"]
    rec = r["recon"]
    dec = _decode_full_samples(tmp_path, r)
    want = np.concatenate([rec[:, :sh, :sw], rec[:, ch:ch + sh // 2, :sw]], 1)
    bad = [i for i in range(len(want)) if not np.array_equal(dec[i], want[i])]
    assert bad == [], f"the oracle decoder differs from the encoder's reconstruction at frames {bad[:8]}"
    # the words say what the counts say
    cmd, modes = r["commands"], r["intra4_modes"]
    assert cmd.shape == modes.shape == (len(frames), ch // 16, cw // 16)
    intra = (cmd & 0xffff8000) == 0x80000000
    i4 = (cmd & 0xffffc000) == 0x80004000
    assert int((cmd == PCM_WORD).sum()) == r["pcm_mbs"] and int(intra.sum()) == r["intra_mbs"]
    assert int(i4.sum()) == r["intra4x4_mbs"] and np.array_equal(modes != I4_NONE, i4)
    assert int((cmd == 0).sum()) >= r["skip_mbs"] >= r["early_skip_mbs"] == r["counters"]["early_skip_hits"]
    assert r["pcm_mbs"] + r["inter_mbs"] + r["skip_mbs"] + r["intra_mbs"] == cmd.size
    assert r["counters"]["i4_won_mbs"] - r["counters"]["i4_pcm_mbs"] == r["intra4x4_mbs"]
    assert sum(r["counters"][f"mode{m}"] for m in range(9)) == \
        16 * (r["counters"]["i4_won_mbs"] + r["counters"]["i16_won_mbs"])
    return r


@pytest.mark.parametrize("qp", [1, 28, 51])
@pytest.mark.parametrize("deblock", [0, 1])
@pytest.mark.parametrize("subpel", [0, 2])
@pytest.mark.parametrize("rules", list(NEW_RULES))
def test_oracle_rate_and_intra4_closed_loop(tmp_path, clip, rules, subpel, deblock, qp):
    frames, sc, _ = clip
    kw = NEW_RULES[rules]
    r = _closed_loop_ex2(tmp_path, frames[:24], 320, 192, sc[:24], out_height=96, subpel=subpel, deblock=bool(deblock),
                         qp=qp, **kw)
    assert (r["early_skip_mbs"] > 0) == bool(kw.get("early_skip"))
    if kw.get("intra4x4") and qp < 51:     # at qp 51 almost nothing is coded and Intra16x16's shorter header wins
        assert r["intra4x4_mbs"] > 0
    if not kw.get("intra4x4"):
        assert r["intra4x4_mbs"] == 0 and sum(r["counters"][f"mode{m}"] for m in range(9)) == 0
    if not kw.get("mvcost"):
        assert r["counters"]["cost_decided_vectors"] == 0 and r["counters"]["inter_predictor_mbs"] == 0


@pytest.mark.parametrize("qp", [1, 28, 51])
@pytest.mark.parametrize("name,W,H,h,R,coded", [("tiny", 64, 48, 24, 4, (32, 32)), ("column", 48, 144, 48, 4, (16, 48)),
                                                ("qcif", 176, 144, 72, 8, (96, 80))])
def test_oracle_rate_and_intra4_edge_shapes(tmp_path, name, W, H, h, R, coded, qp):
    """Everything on over 2 x 2 macroblocks, a one-macroblock-wide column
    (never a left macroblock: block column 0 has the modes 0, 2, 3, 7 only)
    and a width that is cropped."""
    p = tmp_path / f"{name}.mp4"
    scene.synth_write(p, width=W, height=H, n_frames=20, cut_min_s=0.7, cut_max_s=1.5, gop_max_s=0.5, max_motion=6)
    frames, _ = oracle.decode_full(p)
    sc = oracle.score_frames(frames.reshape(-1), frames[0].size, 20, W, H, W, H, 4, want_rgb=False)["score"]
    r = _closed_loop_ex2(tmp_path, frames, W, H, sc, out_height=h, search_range=R, subpel=2, deblock=True, qp=qp,
                         **NEW_RULES["every"])
    assert (r["coded_width"], r["coded_height"]) == coded
    if name == "column":
        for w in r["intra4_modes"][r["intra4_modes"] != I4_NONE]:
            assert {(int(w) >> (4 * k)) & 15 for k in (0, 2, 8, 10)} <= {0, 2, 3, 7}


@pytest.mark.parametrize("qp", [1, 28, 51])
def test_oracle_i_nxn_in_p_slices(tmp_path, clip, qp):
    """max_mb_sad < 0 leaves every P macroblock to the intra pass: I_NxN with
    mb_type 5 beside Intra16x16 in P slices."""
    frames, sc, _ = clip
    r = _closed_loop_ex2(tmp_path, frames[:12], 320, 192, sc[:12], out_height=96, max_mb_sad=-1, qp=qp, intra=True,
                         intra4x4=True)
    assert r["intra_mbs"] + r["pcm_mbs"] == 12 * 60
    if qp < 51:     # at qp 51 almost nothing is coded and Intra16x16's shorter header wins
        assert ((r["commands"][1:] & 0xffffc000) == 0x80004000).any()


def test_oracle_ex2_defaults_are_or_transcode_ex(clip):
    """Every new keyword at its default: or_transcode_ex's bytes, counts and
    reconstruction, also when the call goes through the new entry (want_words)."""
    frames, sc, _ = clip
    for kw in (dict(), dict(intra=True, subpel=2, deblock=True, deblock_offsets=(2, -2)), dict(qp=0, subpel=1)):
        old = oracle.transcode(frames[:30], 320, 192, sc[:30], out_height=96, want_recon=True, keyint=16, **kw)
        new = oracle.transcode(frames[:30], 320, 192, sc[:30], out_height=96, want_recon=True, keyint=16,
                               want_words=True, **kw)
        assert "counters" not in old and new["early_skip_mbs"] == 0 and new["intra4x4_mbs"] == 0
        assert new["samples"] == old["samples"] and np.array_equal(new["recon"], old["recon"])
        assert {k: new[k] for k in old if k.endswith("_mbs") or k == "n_idr"} == \
            {k: old[k] for k in old if k.endswith("_mbs") or k == "n_idr"}
        assert (new["intra4_modes"] == I4_NONE).all() and not any(new["counters"].values())
        assert (new["commands"][0] == PCM_WORD).all() or kw.get("intra")
    with pytest.raises(RuntimeError):      # the rules need residual coding; intra4x4 needs intra
        oracle.transcode(frames[:2], 320, 192, sc[:2], out_height=96, qp=0, early_skip=True)
    with pytest.raises(RuntimeError):
        oracle.transcode(frames[:2], 320, 192, sc[:2], out_height=96, intra4x4=True)
    with pytest.raises(RuntimeError):
        oracle.transcode(frames[:2], 320, 192, sc[:2], out_height=96, mv_lambda16=400)


def test_oracle_vector_cost_keeps_a_true_pan():
    """Noise that pans by (3, 1) samples a frame: only the true vector predicts
    it (16 SAD of any other candidate is some 350 000), so even the largest
    mv_lambda16, 4096, whose 16 bits for (-12, -4) against a zero guess cost
    65 536, leaves the vector alone; the words hold it in quarter samples,
    two's complement halves (include/vtseg.h)."""
    rng = np.random.default_rng(2)
    big = rng.integers(1, 256, (64 + 16, 96 + 32), dtype=np.uint8)
    fr = np.zeros((4, 96, 96), np.uint8)
    for f in range(4):
        fr[f, :64] = big[8 - f:72 - f, 16 - 3 * f:112 - 3 * f]
        fr[f, 64:] = 128
    r = oracle.transcode(fr, 96, 64, np.zeros(4, np.float32), out_height=64, qp=28, mvcost=True, mv_lambda16=4096,
                         want_words=True)
    inner = r["commands"][1:, 1:-1, 1:-1]
    assert (inner == ((-4 & 0xffff) << 16 | (-12 & 0xffff))).all()     # the content came from (x - 3, y - 1)
    assert r["counters"]["inter_predictor_mbs"] > 0                    # pictures 2 and 3 guess that vector


def _ei4h(tmp_path_factory):
    import ctypes as C
    import subprocess
    from test_enc_intra4_host import FLAGS, NATIVE, SRCS
    so = tmp_path_factory.mktemp("ei4h_oracle") / "libencintra4host.so"
    subprocess.run(["g++", "-Og", "-fPIC", "-shared", *FLAGS, str(NATIVE / "enc_intra4_host.cpp"),
                    *map(str, SRCS), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.ei4h_encode.argtypes = [C.c_int] * 4 + [C.c_void_p] * 8
    L.ei4h_encode.restype = None
    return L


@pytest.fixture(scope="module")
def ei4h(tmp_path_factory):
    return _ei4h(tmp_path_factory)


@pytest.mark.parametrize("qp", [1, 28, 51])
@pytest.mark.parametrize("mbw", [1, 2, 10])
def test_oracle_agrees_with_the_encoder_harness(ei4h, mbw, qp):
    """Two restatements of the Intra4x4 rules by different hands: the product's
    CPU harness (tests/native/enc_intra4_host.cpp over csrc/enc_intra4.h, every
    macroblock at kind 5, the encoder's own choice) and the oracle, on one IDR
    picture.  out_height = the source's height makes the downscale the identity
    on samples >= 1.  Equal command words, mode words, bit counts of both
    candidates and reconstruction."""
    mbh = 3
    W, H = 16 * mbw, 16 * mbh
    fr = np.ascontiguousarray(diagonal_frames(F=1, W=max(W, 32), H=H, seed=40 + mbw)[:, :, :W])
    assert np.array_equal(oracle.downscale_nv12(fr[0], W, H, H), fr[0])
    r = oracle.transcode(fr, W, H, np.zeros(1, np.float32), out_height=H, qp=qp, intra=True, intra4x4=True,
                         want_recon=True, want_words=True)
    assert (r["coded_width"], r["coded_height"]) == (W, H)
    n = mbw * mbh
    kind = np.full(n, 5, np.uint8)
    cmd, cbp, coef = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n * 384, np.int16)
    modes, bits, rec = np.zeros(n, np.uint64), np.zeros(2 * n, np.int32), np.zeros_like(fr[0])
    src = np.ascontiguousarray(fr[0])
    ei4h.ei4h_encode(mbw, mbh, 1, qp, src.ctypes.data, kind.ctypes.data, cmd.ctypes.data, cbp.ctypes.data,
                     coef.ctypes.data, modes.ctypes.data, bits.ctypes.data, rec.ctypes.data)
    c = r["counters"]
    print(f"{mbw} x {mbh} macroblocks at qp {qp}: I_NxN {r['intra4x4_mbs']}, Intra16x16 "
          f"{r['intra_mbs'] - r['intra4x4_mbs']}, I_PCM {r['pcm_mbs']}; modes {[c[f'mode{m}'] for m in range(9)]}")
    want_cmd, want_modes = r["commands"][0].reshape(-1), r["intra4_modes"][0].reshape(-1)
    for i in range(n):
        where = f"macroblock (mx {i % mbw}, my {i // mbw})"
        assert int(cmd[i]) == int(want_cmd[i]), f"{where}: harness {int(cmd[i]):#x}, oracle {int(want_cmd[i]):#x}"
        assert int(modes[i]) == int(want_modes[i]), f"{where}: harness {int(modes[i]):#x}, oracle {int(want_modes[i]):#x}"
    assert np.array_equal(bits.reshape(mbh, mbw, 2), r["candidate_bits"][0])
    assert np.array_equal(rec, r["recon"][0])


def test_gpu_cases_exercise_every_decision():
    """A condition on the inputs of tests/test_transcode_bytes_rate_intra4_gpu.py,
    not a measurement: over its (source, settings) pairs the oracle must have
    chosen every Intra4x4PredMode, let the predicted mode's discount decide a
    block, met a cost tie, decided a macroblock each way, met equal bits (won by
    Intra16x16), sent an I_NxN winner back to I_PCM over 3072 bits, let the
    vector cost overrule the least SAD, hit the early-skip probe, and used a
    non-zero predictor guess taken from an inter word.  A case that a defect of
    the device could not fail for lack of such input is no pin."""
    import tempfile
    from pathlib import Path

    from test_transcode_bytes_gpu import _decoded
    from test_transcode_bytes_rate_intra4_gpu import CASES, oracle_side
    with tempfile.TemporaryDirectory() as d:
        work = {"dir": Path(d), "src": {}, "dec": {}, "ref": {}}
        total = dict.fromkeys(oracle.DECISION_COUNTERS, 0)
        print("case | " + " ".join(oracle.DECISION_COUNTERS))
        for name, (sname, tk) in CASES.items():
            c = oracle_side(_decoded(work, sname), tk)["counters"]
            print(f"{name} | " + " ".join(str(c[k]) for k in oracle.DECISION_COUNTERS))
            for k in total:
                total[k] += c[k]
    print("all | " + " ".join(str(total[k]) for k in oracle.DECISION_COUNTERS))
    assert [k for k, v in total.items() if v == 0] == []


# ------------------------------------------------ drop-in decision flow

def test_upload_small_file_is_returned(tmp_path):
    p = tmp_path / "v.mp4"
    p.write_bytes(b"x" * 1000)
    assert upload.compress_video_for_upload(p) == p
    assert not (tmp_path / "compressed_v.mp4").exists()


def test_upload_existing_compressed_is_reused(tmp_path):
    p = tmp_path / "v.mp4"
    p.write_bytes(b"x" * (2 << 20))
    c = tmp_path / "compressed_v.mp4"
    c.write_bytes(b"y")
    assert upload.compress_video_for_upload(p, max_size_mb=1) == c


def test_upload_without_gpu_or_ffmpeg_returns_input(tmp_path, monkeypatch, caplog):
    """No usable device (or a stream outside the decoder subset) and no
    ffmpeg: the reference's FileNotFoundError branch -> the input path, and
    no partial output left behind."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    p = tmp_path / "v.mp4"
    scene.synth_write(p, width=320, height=192, n_frames=30)
    monkeypatch.setattr(upload.shutil, "which", lambda name: None)
    with caplog.at_level(logging.WARNING):
        assert upload.compress_video_for_upload(p, max_size_mb=0.01) == p
    assert not (tmp_path / "compressed_v.mp4").exists()
    assert "ffmpeg not installed" in caplog.text
