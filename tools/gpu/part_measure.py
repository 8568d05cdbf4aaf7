"""Measurements of the Partitions section of DESIGN.md §11 (vts_transcode_ext6.partitions).

    python tools/gpu/part_measure.py bytes OUT.json        small, content, real: partitions 0 -> 1 at subpel 0 / 2,
                                                           CAVLC / CABAC: bytes, counts, the P pictures' PSNR
    python tools/gpu/part_measure.py big OUT.json [REPS]   the 10-min 720p synthetic: bytes, counts, call times
    python tools/gpu/part_measure.py bigpsnr OUT.json      the P pictures' PSNR of it, partitions 0 -> 1 at subpel 0 / 2
    python tools/gpu/part_measure.py once PT SUBPEL        one transcode of it (profiler runs)
    python tools/gpu/part_measure.py summary TRACE.csv     per-kernel summary of a rocprofv3 kernel trace

Every transcode runs in a fresh session.  The inputs are those of the tests (tests/test_transcode_subpel_gpu.py)
and bench.py's 10-min 720p video (seed 0x5EED), written to the directory named by VTS_MEASURE_TMP or the
system's temporary directory and reused when present.  Settings: intra, mvcost, early_skip at qp 28.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT / "video-transformer_amd", ROOT / "oracle", ROOT / "tests", ROOT / "tools" / "gpu"):
    sys.path.insert(0, str(p))

BASE = dict(intra=True, mvcost=True, early_skip=True)
INPUTS = {"small": ("s70", 96), "content": ("content", 360), "real": ("real", 240)}
KEEP = ("pcm_mbs", "intra_mbs", "inter_mbs", "skip_mbs", "subpel_mbs", "qpel_mbs", "recon_hash", "decode_ms", "search_ms",
        "write_ms", "mux_ms")


def _tmp() -> Path:
    d = Path(os.environ.get("VTS_MEASURE_TMP", tempfile.gettempdir())) / "vts_part_measure"
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
             **{k: facts.get(k, 0) for k in ("p16x8_mbs", "p8x16_mbs", "p8x8_mbs")})
    return r


def _settings():
    for sp in (0, 2):
        for cabac in (0, 1):
            for pt in (0, 1):
                yield f"sp{sp}_cabac{cabac}_pt{pt}", dict(BASE, subpel=sp, cabac=bool(cabac), partitions=bool(pt))


def bytes_table(out_json: str) -> None:
    import numpy as np
    import oracle
    import test_transcode_intra4_gpu as I4
    import test_transcode_subpel_gpu as T
    work = {"dir": _tmp(), "src": {}}
    res = {}
    for name, (sname, height) in INPUTS.items():
        src = T._source(work, sname)
        ref = I4._reference(work, sname, height)
        res[name] = {"source_bytes": Path(src).stat().st_size}
        for key, kw in _settings():
            out = _tmp() / "o.mp4"
            r = _one(src, out, height=height, **kw)
            m = oracle.read_mp4(out)
            p = ~np.array([(m["data"][o + 4] & 31) == 5 for o in m["offsets"]])
            r["p_psnr"] = float(T._psnr(oracle.decode_full(out)[0][p], ref[p]))
            res[name][key] = r
        print(name, {k: (v["bytes"], round(v["p_psnr"], 3), v["p16x8_mbs"], v["p8x16_mbs"], v["p8x8_mbs"])
                     for k, v in res[name].items() if isinstance(v, dict)}, flush=True)
    Path(out_json).write_text(json.dumps(res, indent=1))


def big_table(out_json: str, reps: int) -> None:
    src = _big()
    res = {"source_bytes": src.stat().st_size}
    for key, kw in _settings():
        n = reps if "cabac0" in key else 1      # the call times: CAVLC, three fresh sessions each way
        res[key] = [_one(src, _tmp() / "big.mp4", **kw) for _ in range(n)]
        print(key, [(r["bytes"], round(r["call_ms"], 1), round(r["search_ms"], 1), round(r["write_ms"], 1)) for r in res[key]],
              [res[key][0][k] for k in ("p16x8_mbs", "p8x16_mbs", "p8x8_mbs", "inter_mbs", "skip_mbs", "intra_mbs")], flush=True)
    Path(out_json).write_text(json.dumps(res, indent=1))


# ---- the 10-min input's PSNR.  18 000 frames through the CPU oracle is minutes of one core, so the frames go
# to a pool in ranges that start at an IDR picture of the outputs (every 250th frame): a worker cuts those
# frames out of each output, and out of the source from the last IDR picture at or before the range, as small
# MP4 files of their own, decodes them with the CPU oracle and adds up the squared error of the P pictures
# against the oracle's downscale of the source.  CABAC is lossless, so its pictures are the CAVLC run's.
def _mp4_samples(path):
    import oracle
    m = oracle.read_mp4(path)
    off, size = list(m["offsets"]), list(m["sizes"])
    idr = [(m["data"][o + 4] & 31) == 5 for o in off]
    return m, off, size, idr


def _cut(m, off, size, a, b, path, w, h):
    import oracle
    samples = [bytes(m["data"][off[i]:off[i] + size[i]]) for i in range(a, b)]
    oracle.write_mp4(path, m["sps"][0], m["pps"][0], samples, [i * 1000 for i in range(b - a)], [0] * (b - a), 30000, w, h)


def _range_sse(job):
    import numpy as np
    import oracle
    src, outs, a, b, tag = job
    m, off, size, idr = _mp4_samples(src)
    lead = max(i for i in range(a + 1) if idr[i])
    seg = _tmp() / f"seg_{tag}_src.mp4"
    _cut(m, off, size, lead, b, seg, 1280, 720)
    frames = oracle.decode_full(seg)[0][a - lead:]
    seg.unlink()
    sw = oracle.small_width(1280, 720, 360)
    ref = []
    for f in frames:
        d = oracle.downscale_nv12(f, 1280, 720, 360)
        ch = d.shape[0] * 2 // 3
        ref.append(np.concatenate([d[:360, :sw], d[ch:ch + 180, :sw]]))
    ref = np.stack(ref)
    res = {}
    for key, path in outs.items():
        mo, oo, so, io = _mp4_samples(path)
        assert io[a], (key, a)
        seg = _tmp() / f"seg_{tag}_{key}.mp4"
        _cut(mo, oo, so, a, b, seg, sw, 360)
        got = oracle.decode_full(seg)[0]
        seg.unlink()
        p = ~np.array(io[a:b])
        assert got.shape == ref.shape, (got.shape, ref.shape)
        sse = sum(int(((got[i].astype(np.int32) - ref[i]) ** 2).sum()) for i in np.nonzero(p)[0])
        res[key] = (sse, int(p.sum()) * int(ref[0].size))
    return res


def big_psnr(out_json: str) -> None:
    import math
    import multiprocessing as mp
    src = _big()
    outs = {}
    for sp in (0, 2):
        for pt in (0, 1):
            key = f"sp{sp}_pt{pt}"
            outs[key] = _tmp() / f"big_{key}.mp4"
            _one(src, outs[key], partitions=bool(pt), subpel=sp, **BASE)
    step = 750
    jobs = [(src, outs, a, min(a + step, 18000), str(a)) for a in range(0, 18000, step)]
    with mp.get_context("spawn").Pool(14) as pool:
        parts = pool.map(_range_sse, jobs, chunksize=1)
    res = {}
    for key in outs:
        sse, n = sum(p[key][0] for p in parts), sum(p[key][1] for p in parts)
        res[key] = {"p_psnr": 10 * math.log10(255.0 ** 2 * n / sse), "p_bytes_compared": n, "bytes": outs[key].stat().st_size}
        outs[key].unlink()
    print(res, flush=True)
    Path(out_json).write_text(json.dumps(res, indent=1))


def once(pt: int, subpel: int) -> None:
    print(_one(_big(), _tmp() / "once.mp4", partitions=bool(pt), subpel=subpel, **BASE), flush=True)


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "bytes":
        bytes_table(sys.argv[2])
    elif cmd == "big":
        big_table(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    elif cmd == "bigpsnr":
        big_psnr(sys.argv[2])
    elif cmd == "once":
        once(int(sys.argv[2]), int(sys.argv[3]))
    else:
        import intra4_measure
        intra4_measure.summary(sys.argv[2])
