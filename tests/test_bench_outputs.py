"""bench.py --dump-outputs and the plain / --full split.

CPU: the dump helpers keep every value's precision (float32, float64 for
32- and 64-bit integers and doubles), stay under the 64 MB limit by a seeded sample
that is the same on every call, and a plain run switches off everything that
takes runs of its own.  GPU: one plain run of the smallest configuration
writes the last step's BatchItems, equal to the oracle's cuts and the plan.
"""
from __future__ import annotations

import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


B = _bench()


def test_dump_keeps_small_arrays_whole_and_exact(tmp_path):
    arrays = {"u8": np.arange(256, dtype=np.uint8).reshape(16, 16),
              "i16": np.array([-32768, 0, 32767], np.int16),
              "i32": np.array([0, (1 << 24) + 1, (1 << 31) - 1], np.int32),
              "i64": np.array([0, (1 << 53) - 1, -5], np.int64),
              "f32": np.array([1e-7, 0.08, 3.5], np.float32),
              "f64": np.array([1 / 3, 600.0], np.float64),
              "empty": np.zeros((0, 2), np.int64)}
    written = B.dump_outputs(tmp_path / "d", arrays)
    assert sorted(written) == sorted(f"{k}.npy" for k in arrays)
    for k, a in arrays.items():
        got = np.load(tmp_path / "d" / f"{k}.npy")
        assert got.dtype == (np.float32 if k in ("u8", "i16", "f32") else np.float64), k
        assert got.shape == a.shape and np.array_equal(got, a.astype(got.dtype)), k
        assert np.array_equal(got.astype(a.dtype), a), k  # nothing rounded


def test_dump_samples_large_arrays_within_the_limit_and_repeats(tmp_path, monkeypatch):
    monkeypatch.setattr(B, "DUMP_LIMIT_BYTES", 40_000)
    rng = np.random.default_rng(3)
    arrays = {"rows": rng.integers(0, 255, size=(1000, 30), dtype=np.uint8),   # sampled by row
              "wide": rng.integers(0, 255, size=(2, 20_000), dtype=np.uint8),  # one row too large
              "vec": rng.integers(0, 1 << 40, size=5000, dtype=np.int64),      # 1-D, float64
              "small": np.arange(10, dtype=np.float32)}
    w1 = B.dump_outputs(tmp_path / "a", arrays)
    w2 = B.dump_outputs(tmp_path / "b", arrays)
    assert w1 == w2 and sum(w1.values()) <= 40_000
    assert "small.rows.npy" not in w1
    for name in w1:
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
    for k in ("rows", "wide", "vec"):
        vals = np.load(tmp_path / "a" / f"{k}.npy")
        idx = np.load(tmp_path / "a" / f"{k}.rows.npy")
        assert idx.dtype == np.float64 and len(idx) == len(vals) > 0
        assert np.all(np.diff(idx) > 0)
        src = arrays[k] if k == "rows" else arrays[k].reshape(-1)
        assert np.array_equal(vals, src[idx.astype(np.int64)].astype(vals.dtype)), k
    assert np.load(tmp_path / "a" / "rows.npy").shape[1:] == (30,)


def test_step_outputs_of_a_batch():
    from vtseg.batch import BatchItem
    items = [BatchItem(index=0, path="a", duration=600.0, n_segments=2, n_cuts=3, rank=0,
                       segment_frames=((0, 15000), (13800, 18000)), cut_frames=(7, 90, 17999),
                       cut_times=(7 / 30, 3.0, 17999 / 30)),
             BatchItem(index=1, path="b", duration=1.5, n_segments=1, n_cuts=-1, rank=0,
                       score_failed=True)]
    arr = B.step_outputs("decode_score", {"items": items})
    assert sorted(arr) == ["records"] + sorted(f"v{i}_{n}" for i in (0, 1)
                                               for n in ("cut_frames", "cut_times", "segment_frames"))
    assert arr["records"].tolist() == [[2, 3, 600.0, 0.0], [1, -1, 1.5, 1.0]]
    assert arr["v0_segment_frames"].tolist() == [[0, 15000], [13800, 18000]]
    assert arr["v0_cut_frames"].tolist() == [7, 90, 17999]
    assert arr["v0_cut_times"].tolist() == [7 / 30, 3.0, 17999 / 30]
    assert arr["v1_segment_frames"].shape == (0, 2) and arr["v1_cut_frames"].shape == (0,)


def test_plain_run_measures_only_the_headline(monkeypatch):
    """Without --full every part that takes runs of its own is off, whatever
    else is asked for; --full leaves the single switches to the caller."""
    seen = {}

    class Stop(Exception):
        pass

    def plan(gpus, env, ndev, backend, argv, port=None):
        raise Stop

    real = B.argparse.ArgumentParser.parse_args

    def parse(self, *a, **k):
        seen["args"] = real(self, *a, **k)
        return seen["args"]

    monkeypatch.setattr(B, "rank_launch_plan", plan)
    monkeypatch.setattr(B.argparse.ArgumentParser, "parse_args", parse)
    for argv, full in ((["--gpus", "1", "--steps", "7", "--warmup", "2", "--extras", "all"], False),
                       (["--steps", "7", "--full"], True),
                       (["--steps", "7", "--full", "--no-pmc", "--extras", "none"], True)):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        with pytest.raises(Stop):
            B.main()
        a = seen["args"]
        assert a.steps == 7 and a.full is full
        if not full:
            assert a.no_parity and a.no_cpu_baseline and a.no_pmc and a.extras == "none"
        else:
            assert not a.no_parity and not a.no_cpu_baseline
            assert a.no_pmc == ("--no-pmc" in argv)
            assert a.extras == ("none" if "--extras" in argv else "all")


def test_profile_children_keep_the_rooflines_runs():
    # CHILD_RUNS counts the roofline's runs, which only a --full child makes
    import inspect
    src = inspect.getsource(B.profile_passes)
    assert '"--full"' in src and B.CHILD_RUNS == 2 + B.ROOF_RUNS


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_batch(tmp_path):
    import oracle
    from vtseg import budget_planner as bp
    from vtseg import video_segmenter as vs
    frames, steps = 900, 2
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--config", "480p-60s", "--frames", str(frames),
                        "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k != "WORLD_SIZE"})
    assert p.returncode == 0, p.stderr[-2000:]
    # RCCL may announce its version on stdout beside the result line
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-500:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    # value = frames per step / time per step
    assert line["value"] == pytest.approx(frames / (line["ms_per_step"] / 1e3), rel=1e-3)
    # nothing beside the headline was measured
    assert line["roofline"] is None and line["parity"] is None and line["cpu_baseline"] is None
    assert "e2e" not in line and "general" not in line

    files = sorted(f.name for f in out.iterdir())
    assert files == ["records.npy", "v0_cut_frames.npy", "v0_cut_times.npy", "v0_segment_frames.npy"]
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64 * 1000 * 1000
    got = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())

    # the same video (the benchmark's seed) through the oracle and the planner
    path = tmp_path / "same.mp4"
    B.synth_videos([(path, 0x5EED)], 640, 480, frames)
    ref = oracle.decode_score_gops(path, 4, 4)
    cuts = np.nonzero(ref["score"] > 0.08)[0]
    assert len(cuts) > 0
    duration = frames / B.FPS
    plan = bp.plan_segments_with_budget(duration, B.REF_CONFIG, 0)
    segs = vs.plan_segments(duration, plan.segment_duration, plan.overlap)
    times = [t for sg in segs for t in (sg.start, sg.end)]
    want_sf = oracle.boundary_frames(ref["pts"], ref["timescale"], times)
    assert got["records"].tolist() == [[len(segs), len(cuts), duration, 0.0]]
    assert got["v0_cut_frames"].tolist() == cuts.tolist()
    assert got["v0_cut_times"].tolist() == [ref["pts"][c] / ref["timescale"] for c in cuts]
    assert got["v0_segment_frames"].reshape(-1).tolist() == list(want_sf)
