"""Measurements of the Intra4x4 section of DESIGN.md §11 (vts_transcode_ext5.intra4x4).

    python tools/gpu/intra4_measure.py bytes OUT.json        the small inputs, every setting, intra4x4 0 -> 1
    python tools/gpu/intra4_measure.py big OUT.json [REPS]   the 10-min 720p synthetic: bytes and call times
    python tools/gpu/intra4_measure.py once I4 CABAC         one transcode of it, everything on (profiler runs)
    python tools/gpu/intra4_measure.py summary TRACE.csv     per-kernel summary of a rocprofv3 kernel trace,
                                                             enc_intra split into its IDR and P levels

Every transcode runs in a fresh session.  The inputs are those of the tests (tests/test_transcode_subpel_gpu.py)
and bench.py's 10-min 720p video (seed 0x5EED), written to the directory named by VTS_MEASURE_TMP or the
system's temporary directory and reused when present.
"""
from __future__ import annotations

import csv
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT / "video-transformer_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

EVERY = dict(intra=True, subpel=2, deblock=True, mvcost=True, early_skip=True)
SETTINGS = {"intra": dict(intra=True), "every": EVERY}
INPUTS = ["real", "content", "small", "halfpel", "bigpan_edges", "crop", "keyint8_r16"]
KEEP = ("pcm_mbs", "intra_mbs", "inter_mbs", "skip_mbs", "recon_hash", "decode_ms", "search_ms", "write_ms", "mux_ms")


def _tmp() -> Path:
    d = Path(os.environ.get("VTS_MEASURE_TMP", tempfile.gettempdir())) / "vts_intra4_measure"
    d.mkdir(parents=True, exist_ok=True)
    return d


def _big() -> Path:
    from vtseg import scene
    path = _tmp() / "synth_720p_10min.mp4"
    if not path.exists():
        scene.synth_write(path, width=1280, height=720, fps=30, n_frames=18000, seed=0x5EED)
    return path


def _one(src, out, **kw) -> dict:
    from vtseg import scene
    t0 = time.perf_counter()
    with scene.VideoScorer(src) as v:
        t1 = time.perf_counter()
        facts = v.transcode(out, **kw)
        t2 = time.perf_counter()
    r = {k: facts[k] for k in KEEP}
    r.update(bytes=out.stat().st_size, open_ms=(t1 - t0) * 1e3, call_ms=(t2 - t1) * 1e3,
             intra4x4_mbs=facts.get("intra4x4_mbs", 0))
    return r


def bytes_table(out_json: str) -> None:
    import test_transcode_subpel_gpu as T
    work = {"dir": _tmp(), "src": {}}
    res = {}
    for name in INPUTS:
        sname, tk, _ = T.CASES[name]
        src = T._source(work, sname)
        res[name] = {"source_bytes": Path(src).stat().st_size}
        for sk, sv in SETTINGS.items():
            for cabac in (0, 1):
                for i4 in (0, 1):
                    kw = dict(tk, **sv)
                    if i4:
                        kw["intra4x4"] = True
                    if cabac:
                        kw["cabac"] = True
                    res[name][f"{sk}_cabac{cabac}_i4{i4}"] = _one(src, _tmp() / "o.mp4", **kw)
        print(name, {k: v["bytes"] for k, v in res[name].items() if isinstance(v, dict)}, flush=True)
    Path(out_json).write_text(json.dumps(res, indent=1))


def big_table(out_json: str, reps: int) -> None:
    src = _big()
    res = {"source_bytes": src.stat().st_size}
    for sk, sv in SETTINGS.items():
        for cabac in (0, 1):
            for i4 in (0, 1):
                kw = dict(sv)
                if i4:
                    kw["intra4x4"] = True
                if cabac:
                    kw["cabac"] = True
                key = f"{sk}_cabac{cabac}_i4{i4}"
                res[key] = [_one(src, _tmp() / "big.mp4", **kw) for _ in range(reps)]
                print(key, [(r["bytes"], round(r["call_ms"], 1), round(r["search_ms"], 1), round(r["write_ms"], 1))
                            for r in res[key]], res[key][0]["intra4x4_mbs"], res[key][0]["intra_mbs"], flush=True)
    Path(out_json).write_text(json.dumps(res, indent=1))


def once(i4: int, cabac: int) -> None:
    print(_one(_big(), _tmp() / "once.mp4", cabac=bool(cabac), intra4x4=bool(i4), **EVERY), flush=True)


def summary(trace: str) -> None:
    rows = list(csv.DictReader(open(trace)))
    t0 = min(int(r["Start_Timestamp"]) for r in rows)
    by: dict[str, list[tuple[int, int]]] = {}
    launches = 0
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].replace("void ", "").replace("vts::(anonymous namespace)::", "").replace("vts::", "")
        name = name.rsplit("(", 1)[0] if name.endswith(")") else name
        if name.startswith("enc_intra"):       # the first launch of a transcode is level 0, the IDR pictures
            name += " P levels" if launches else " IDR level"
            launches += 1
        by.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    print(f"{'kernel':<64}{'n':>5}{'total_ms':>11}{'median_ms':>11}{'max_ms':>10}{'first_ms':>10}{'last_end_ms':>12}")
    for name, iv in sorted(by.items(), key=lambda kv: -sum(e - s for s, e in kv[1])):
        d = [(e - s) / 1e6 for s, e in iv]
        print(f"{name:<64}{len(iv):>5}{sum(d):>11.2f}{statistics.median(d):>11.3f}{max(d):>10.3f}"
              f"{(iv[0][0] - t0) / 1e6:>10.1f}{(max(e for _, e in iv) - t0) / 1e6:>12.1f}")


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "bytes":
        bytes_table(sys.argv[2])
    elif cmd == "big":
        big_table(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    elif cmd == "once":
        once(int(sys.argv[2]), int(sys.argv[3]))
    else:
        summary(sys.argv[2])
