"""Edge picture shapes on the device, both decoders, against the oracle.

Geometry alone selects several kernel paths no other GPU test reaches:
pictures of one macroblock, one macroblock row or one macroblock column (no
left, top or any neighbour; the 16-macroblock blocks of h264_inter_full /
h264_bs_full with a tail, the level-blocked kernel's variants), and tall
narrow pictures: 65, 69, 129 and 256 macroblock rows run h264_derive with 2, 3
and 4 waves and h264_deblock_plane with a second pass of one row, of a full
row group plus one, a third pass and a fourth.  tests/test_shapes_host.py
runs the same streams through the device code on the CPU.

Every frame, histogram, SAD, score and RGB thumbnail must equal the oracle's.
The by-block intra kernel (VTS_INTRA=1), which otherwise only runs on pictures
whose level table does not fit the lane-parallel kernel's LDS, is run here on
purpose and the session must report which kernel it runs.  No shape here is
one the deblocking hand-off's model (tests/test_dbk_sched_host.py) reports a
deadlock for; the one stream that is must be refused at open."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from vtseg import VtsegError, scene

pytestmark = pytest.mark.gpu

# display size (mbw x mbh)
SHAPES = [
    (16, 16),      # 1x1: no neighbours at all
    (272, 16),     # 17x1: single row, a block of 16 macroblocks and a tail of 1
    (1024, 16),    # 64x1
    (16, 1040),    # 1x65: second deblock pass of one row, 2-wave derive, no left neighbour
    (32, 1104),    # 2x69: full second pass plus one row
    (48, 2064),    # 3x129: third pass, 3-wave derive
    (64, 4096),    # 4x256: the tallest picture derive_launch accepts
]
SHAPE_IDS = [f"{w}x{h}" for w, h in SHAPES]
KINDS = {
    "cavlc": dict(coding="full"),
    "cavlc_b": dict(coding="full", bframes=True, weighted="implicit", temporal_direct=True),
    "cabac_b": dict(coding="full", cabac=True, bframes=True, transform_8x8=True, weighted="implicit",
                    slices_per_row=0),
    "subset": dict(),
}
GENERAL_KINDS = ["cavlc", "cavlc_b", "cabac_b"]
N = 12
COMMON = dict(n_frames=N, seed=7, max_motion=4, cut_min_s=0.1, cut_max_s=0.3, gop_max_s=0.2)
K = 4   # the default k = 6 above 720 rows does not divide these heights


def _require_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires an MI355X")


def _first_diff(a, b):
    bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(1))[0]
    return bad[:8].tolist()


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    """(kind, W, H, extra writer arguments) -> (path, oracle frames, oracle
    scores); written and decoded once per module, never modified."""
    root = tmp_path_factory.mktemp("shapes")
    made = {}

    def get(kind, W, H, **extra):
        key = (kind, W, H, tuple(sorted(extra.items())))
        if key not in made:
            path = root / f"{kind}_{W}x{H}_{len(made)}.mp4"
            scene.synth_write(path, width=W, height=H, **{**COMMON, **KINDS[kind], **extra})
            frames, _ = oracle.decode_full(path)
            if kind == "subset":   # the subset oracle is a second reference
                sub, _ = oracle.decode_file(path)
                assert np.array_equal(sub, frames)
            n = frames.shape[0]
            ref = oracle.score_frames(frames.reshape(-1), frames[0].size, n, W, H, W, H, K)
            frames.setflags(write=False)
            made[key] = (path, frames, ref)
        return made[key]
    return get


def _scores_equal(res, ref):
    assert np.array_equal(res.hist, ref["hist"])
    assert np.array_equal(res.sad, ref["sad"])
    assert np.array_equal(res.scores, ref["score"])


def _kept_equal(v, frames, ref):
    """A keep_frames session against the oracle: frames, scores, thumbnails."""
    n = frames.shape[0]
    res = v.score()
    got = np.stack([v.frame_nv12(i).reshape(frames[i].shape) for i in range(n)])
    assert _first_diff(got, frames) == []
    _scores_equal(res, ref)
    rgb = np.stack([v.thumbnail_rgb(i, K) for i in range(n)]).reshape(-1)
    assert np.array_equal(rgb, ref["rgb"])


def _recycled_equal(path, ref):
    """Without keep_frames the general decoder recycles its surfaces: only the
    scoring outputs can be compared (tests/test_full_gpu.py _recycled_equal)."""
    with scene.VideoScorer(path, k=K) as v:
        assert v.general() and v._lib.vts_schedule_info(v._ctx, 11) > 0
        res = v.score()
        _scores_equal(res, ref)
        n = res.scores.shape[0]
        rgb = np.stack([v.thumbnail_rgb(i, K) for i in range(n)]).reshape(-1)
        assert np.array_equal(rgb, ref["rgb"])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", GENERAL_KINDS)
def test_general_decoder_edge_shapes(stream, kind, shape):
    _require_gpu()
    path, frames, ref = stream(kind, *shape)
    with scene.VideoScorer(path, keep_frames=True, k=K) as v:
        assert v.general()
        assert v._lib.vts_schedule_info(v._ctx, 14) == 2   # the lane-parallel intra kernel
        _kept_equal(v, frames, ref)
    _recycled_equal(path, ref)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("mode", ["level_block_1", "level_block_4", "general"])
def test_subset_streams_edge_shapes(stream, mode, shape):
    """Subset-syntax streams on the subset decoder, per level (level_block 1)
    and level-blocked (4: tb_launch picks its kernel variant from the picture's
    width and height), and on the general decoder."""
    _require_gpu()
    path, frames, ref = stream("subset", *shape)
    kw = dict(decoder="general") if mode == "general" else dict(level_block=int(mode[-1]))
    with scene.VideoScorer(path, keep_frames=True, k=K, **kw) as v:
        assert v.general() == (mode == "general")
        assert v._lib.vts_schedule_info(v._ctx, 14) == (2 if mode == "general" else 0)
        if mode == "level_block_4":
            assert v.level_blocks()[0] > 0
        elif mode == "level_block_1":
            assert v.level_blocks()[0] == 0
        _kept_equal(v, frames, ref)


@pytest.mark.parametrize("shape", [(16, 1040), (64, 4096)], ids=["16x1040", "64x4096"])
def test_tall_cabac_pictures_in_windows_on_two_groups(stream, monkeypatch, shape):
    """Two GOP groups on their own streams, windows of 6 frames on two rings;
    the paced bS launches on their own stream (default) and on the score
    stream (VTS_BS_STREAM=0) give the same, the oracle's, results."""
    _require_gpu()
    path, frames, ref = stream("cabac_b", *shape)
    monkeypatch.setenv("VTS_GENERAL_GROUPS", "2")
    for bs_stream in (None, "0"):
        if bs_stream is not None:
            monkeypatch.setenv("VTS_BS_STREAM", bs_stream)
        with scene.VideoScorer(path, k=K, window_frames=6, n_streams=2, keep_frames=True) as v:
            assert v.general() and v.windows() >= 2
            res = v.score()
            _scores_equal(res, ref)
            assert np.array_equal(v.frame_nv12(N - 1).reshape(frames[-1].shape), frames[-1])


# ------------------------------------------------------------ cropped display widths
CROPPED = [(72, 128), (88, 72)]   # coded 80x128 and 96x80: what the device encoder writes for portrait uploads


@pytest.mark.parametrize("shape", CROPPED, ids=[f"{w}x{h}" for w, h in CROPPED])
@pytest.mark.parametrize("kind", ["cavlc", "cabac_b", "subset"])
def test_display_width_no_multiple_of_16(stream, kind, shape):
    """The scoring kernels work in chunks of 16 row bytes; a display width
    that is no multiple of 16 is scored by the per-pixel kernels instead, on
    both decoders, with and without kept frames (the general decoder then
    does not recycle its surfaces: thumb_pics is chunked too)."""
    _require_gpu()
    path, frames, ref = stream(kind, *shape)
    with scene.VideoScorer(path, keep_frames=True, k=K) as v:
        assert v.general() == (kind != "subset") and not v.fused()
        _kept_equal(v, frames, ref)
    with scene.VideoScorer(path, k=K) as v:
        assert v._lib.vts_schedule_info(v._ctx, 11) == 0
        res = v.score()
        _scores_equal(res, ref)
        rgb = np.stack([v.thumbnail_rgb(i, K) for i in range(N)]).reshape(-1)
        assert np.array_equal(rgb, ref["rgb"])
    if kind == "subset":
        with scene.VideoScorer(path, decoder="general", keep_frames=True, k=K) as v:
            assert v.general()
            _kept_equal(v, frames, ref)


# ------------------------------------------------------------ the by-block intra kernel
BY_BLOCK = [
    ("cavlc_cip_qcif", "cavlc", 176, 144, dict(constrained_intra=True)),
    ("cabac_t8_scaled_b_qcif", "cabac_b", 176, 144, dict(scaling="both")),
    ("cavlc_16x1040", "cavlc", 16, 1040, {}),
    ("cavlc_272x16", "cavlc", 272, 16, {}),
    ("cabac_16x1040", "cabac_b", 16, 1040, {}),
    ("cabac_272x16", "cabac_b", 272, 16, {}),
]


@pytest.mark.parametrize("name,kind,W,H,extra", BY_BLOCK, ids=[b[0] for b in BY_BLOCK])
def test_by_block_intra_kernel(stream, monkeypatch, name, kind, W, H, extra):
    """h264_intra_full (VTS_INTRA=1, read at open) on the device equals the
    oracle, and the session says which intra kernel it runs, in both
    directions: a renamed variable cannot make this a second run of the
    default kernel."""
    _require_gpu()
    path, frames, ref = stream(kind, W, H, **extra)
    monkeypatch.delenv("VTS_INTRA", raising=False)
    with scene.VideoScorer(path, k=K) as v:
        assert v.general() and v._lib.vts_schedule_info(v._ctx, 14) == 2
    monkeypatch.setenv("VTS_INTRA", "1")
    with scene.VideoScorer(path, keep_frames=True, k=K) as v:
        assert v.general() and v._lib.vts_schedule_info(v._ctx, 14) == 1
        _kept_equal(v, frames, ref)
    monkeypatch.setenv("VTS_INTRA", "2")
    with scene.VideoScorer(path, k=K) as v:
        assert v._lib.vts_schedule_info(v._ctx, 14) == 2


# ------------------------------------------------------------ the deblocking hand-off's guard
def test_width_the_deblocking_hand_off_cannot_take_is_refused_at_open(tmp_path):
    """331 x 69 macroblocks: from this width on a picture with a second
    deblocking pass deadlocks the shipped 16-wave hand-off (dbk_sched.h, the
    model in tests/test_dbk_sched_host.py).  The session must refuse it when it
    is opened, before anything is launched; it is never decoded."""
    _require_gpu()
    T = 331
    path = tmp_path / "wide.mp4"
    scene.synth_write(path, width=16 * T, height=1104, n_frames=2, seed=7, coding="full")
    with pytest.raises(VtsegError, match="deblocking hand-off takes at most 330 macroblocks"):
        scene.VideoScorer(path, decoder="general")
