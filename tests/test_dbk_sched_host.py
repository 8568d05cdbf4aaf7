"""The deblocking wavefront's hand-off (csrc/dbk_sched.h) as a model on the CPU.

h264_deblock_plane's waves wait for each other through prog[]; with too few
waves for the picture's width the pass-start wait and the ring hand-off wait
for each other for ever (VERDICT "What's weak" item 3: the 256-thread build
hung on 720p).  No GPU test may go looking for that, so the rules live in a
header the kernel, the host's shape guard and a stand-alone model
(tests/native/dbk_sched_main.cpp, built with the address and undefined
behaviour sanitizers) share:
  - the model's known answers: the hang that was seen, the shapes that run;
  - the ring stays consistent under every schedule, and the model notices
    when either per-macroblock wait is weakened by one column;
  - dp_shape_ok(), the closed form the guard and the static_assert use, equals
    the model over the whole table of shapes;
  - the closed form's thresholds are the model's (general_shape_error(), what
    the session calls at open, is tested on them in tests/test_shapes_host.py)."""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "video-transformer_amd" / "csrc"

# first deadlocking width in macroblocks for 4 / 8 / 16 waves, pictures with
# at least one whole row group in the second pass; 16 more with 1..3 rows
THRESHOLD = {4: 67, 8: 155, 16: 331}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dbk") / "dbk_sched_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}",
                    str(ROOT / "tests" / "native" / "dbk_sched_main.cpp"), "-o", str(exe)], check=True)

    def run(*args):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
        # a sanitizer report would be on stderr or extra lines: nothing but the result line
        assert p.returncode == 0 and p.stderr == "" and p.stdout.count("\n") == 1, (p.returncode, p.stdout, p.stderr)
        kind, *fields = p.stdout.split()
        assert kind == args[0]
        out = dict(f.split("=") for f in fields)
        return {k: (int(v) if re.fullmatch(r"-?\d+", v) else v) for k, v in out.items()}
    return run


@pytest.mark.parametrize("waves,mbw,mbh,want", [
    (4, 80, 45, "deadlock"),     # the 256-thread build on 720p: the hang that was seen
    (8, 80, 45, "complete"),
    (16, 80, 45, "complete"),
    (16, 120, 68, "complete"),   # 1080p
    (16, 1, 65, "complete"),
    (16, 4, 256, "complete"),
    (16, 330, 256, "complete"),
    (16, 331, 256, "deadlock"),
    (16, 360, 180, "deadlock"),  # 5760x2880
    (8, 240, 135, "deadlock"),   # 3840x2160 on the 512-thread build
    (16, 240, 135, "complete"),
])
def test_known_answers(model, waves, mbw, mbh, want):
    r = model("run", mbw, mbh, waves)
    assert r["result"] == want, r
    assert r["schedules"] >= 11
    assert r["stale_reads"] == 0 and r["lost_lines"] == 0, r


@pytest.mark.parametrize("waves,mbw,mbh", [(16, 120, 68), (8, 80, 45), (16, 40, 256)])
def test_weakened_waits_break_the_ring(model, waves, mbw, mbh):
    """need_up one column early reads a line whose last word is not written;
    need_dn one column early overwrites a line that has not been read."""
    assert model("run", mbw, mbh, waves, 0, 0)["stale_reads"] == 0
    up = model("run", mbw, mbh, waves, 1, 0)
    assert up["stale_reads"] > 0, up
    dn = model("run", mbw, mbh, waves, 0, 1)
    assert dn["lost_lines"] > 0, dn


@pytest.mark.parametrize("waves", [4, 8, 16])
def test_shape_predicate_equals_the_model(model, waves):
    """Every mbw in 1..1024 at mbh in {64, 65, 67, 68, 129, 256} and every mbh
    in 1..256 at mbw in {1, 16, 17, T - 1, T, 1024}."""
    t = model("table", waves)
    assert t["checked"] == 6 * 1024 + 6 * 256
    assert t["mismatches"] == 0, t
    assert t["T"] == THRESHOLD[waves] and t["T_short"] == THRESHOLD[waves] + 16, t
