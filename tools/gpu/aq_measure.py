"""Measurements of the Adaptive quantisation section of DESIGN.md §11 (vts_transcode_ext9).

    python tools/gpu/aq_measure.py table OUT.json             content and the 10-min 720p synthetic, everything on, at QP
                                                              23 and 28 with aq_strength 0, 0.5 and 1.0: the bytes and
                                                              the mean and range of mb_qp; on the content source also the
                                                              P pictures' PSNR and their luma PSNR split by the sign of
                                                              the macroblock's offset at strength 1.0 (the 10-min input's
                                                              18 000 frames are not put through the CPU oracle: bytes and
                                                              mb_qp only)
    python tools/gpu/aq_measure.py speed OLD OUT.jsonl [N [CASES]]
                                                              this tree against the tree at OLD (its own package and
                                                              in-tree libvtseg.so), interleaved, N fresh processes each
                                                              (default 5): default, everything on, bench.py --workload
                                                              transcode, and for this tree everything on with
                                                              aq_strength 1.0; medians with min..max; the sweep ends at
                                                              the first process that fails; CASES: a comma list of
                                                              default, every, every_aq, bench
    python tools/gpu/aq_measure.py one TREE CASE              one transcode of the 10-min input with TREE's package

Every transcode runs in a fresh session.  The inputs are those of the rate-control table (tools/gpu/ratectl_measure.py).
"""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from ratectl_measure import EVERY, ROOT, _big, _one, _tmp, _use  # noqa: E402

CASES = {"default": {}, "every": EVERY, "every_aq": dict(EVERY, aq_strength=1.0)}
ORDER = ("default", "every", "every_aq", "bench")


def table(out_json: str) -> None:
    _use(ROOT)
    import numpy as np
    import oracle
    import test_transcode_intra4_gpu as I4
    import test_transcode_subpel_gpu as T
    from vtseg import scene
    work = {"dir": _tmp(), "src": {}}
    res = {}
    for name in ("content", "big"):
        src = _big() if name == "big" else T._source(work, "content")
        ref = I4._reference(work, "content", 360) if name == "content" else None
        out = _tmp() / "aq.mp4"
        res[name] = {}
        for qp in (23, 28):
            runs = {}
            sign = None                     # [F, mbh, mbw]: the sign of a macroblock's offset at strength 1.0
            if ref is not None:             # the classes of all three runs, from a call of their own
                with scene.VideoScorer(src) as v:
                    sign = np.sign(v.transcode(out, qp=qp, aq_strength=1.0, **EVERY)["mb_qp"].astype(np.int64) - qp)
            for s in (0.0, 0.5, 1.0):
                with scene.VideoScorer(src) as v:
                    facts = v.transcode(out, qp=qp, aq_strength=s, **EVERY)
                r = {"bytes": out.stat().st_size, "search_ms": facts["search_ms"], "write_ms": facts["write_ms"]}
                if s:
                    q = facts["mb_qp"].astype(np.int64)
                    r.update(mb_qp_mean=float(q.mean()), mb_qp_lo=int(q.min()), mb_qp_hi=int(q.max()),
                             aq_lo=int(facts["aq_lo"]), aq_hi=int(facts["aq_hi"]), aq_mbs=int(facts["aq_mbs"]))
                else:
                    r.update(mb_qp_mean=float(qp), mb_qp_lo=qp, mb_qp_hi=qp)
                if ref is not None:
                    m = oracle.read_mp4(out)
                    p = ~np.array([(m["data"][o + 4] & 31) == 5 for o in m["offsets"]])
                    rec = oracle.decode_full(out)[0]
                    r["p_psnr"] = float(T._psnr(rec[p], ref[p]))
                    H, W = ref.shape[1] * 2 // 3, ref.shape[2]
                    d = (rec[:, :H].astype(np.float64) - ref[:, :H]) ** 2
                    # a sample's class: its macroblock's (the display size crops the last macroblocks)
                    cls = np.kron(sign, np.ones((16, 16), np.int64))[:, :H, :W]
                    for label, val in (("below", -1), ("at", 0), ("above", 1)):
                        sel = (cls == val) & p[:, None, None]
                        if sel.any():
                            mse = d[sel].mean()
                            r[f"p_luma_psnr_{label}"] = float(99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse))
                            r[f"samples_{label}"] = int(sel.sum())
                runs[f"aq{s}"] = r
            res[name][f"qp{qp}"] = runs
            print(name, qp, json.dumps(runs), flush=True)
    Path(out_json).write_text(json.dumps(res, indent=1))


def one(tree: str, case: str) -> None:
    _use(Path(tree))
    print(json.dumps(_one(_big(), _tmp() / f"one_{os.getpid()}.mp4", **CASES[case])), flush=True)
    (_tmp() / f"one_{os.getpid()}.mp4").unlink()


def speed(old: str, out_jsonl: str, reps: int, cases=ORDER) -> None:
    """Ends at the first process that does not exit 0 (an error, an abort, a signal or the time limit): its row
    is written, nothing more is started on the card, and the medians are over what finished."""
    _use(ROOT)
    _big()
    trees = {"parent": Path(old).resolve(), "new": ROOT}
    jobs = [(rep, case, tree, root) for rep in range(1, reps + 1) for case in cases for tree, root in trees.items()
            if not (case == "every_aq" and tree == "parent")]
    rows, failed = [], None
    with open(out_jsonl, "w") as f:
        for rep, case, tree, root in jobs:
            if case == "bench":
                cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--workload",
                       "transcode", "--no-cpu-baseline", "--no-pmc"]
            else:
                cmd = [sys.executable, str(Path(__file__).resolve()), "one", str(root), case]
            row = {"tree": tree, "rep": rep, "case": case}
            try:
                p = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
                status, err = p.returncode, p.stderr
            except subprocess.TimeoutExpired:
                status, err = "timeout", ""
            if status != 0:
                tail = err.strip().splitlines()
                failed = dict(row, status=status, failed=tail[-1][-300:] if tail else "")
                f.write(json.dumps(failed) + "\n")
                print(failed, flush=True)
                break
            r = json.loads(p.stdout.strip().splitlines()[-1])
            row.update(ms=r["ms_per_step"] if case == "bench" else r["call_ms"],
                       **{k: r[k] for k in ("bytes", "search_ms", "write_ms", "recon_hash", "value") if k in r})
            rows.append(row)
            f.write(json.dumps(row) + "\n")
            f.flush()
            print(row, flush=True)
    for case in cases:
        for tree in trees:
            for field in ("ms", "search_ms", "write_ms"):
                v = [r[field] for r in rows if r["tree"] == tree and r["case"] == case and field in r]
                if v:
                    print(f"{case:10s} {tree:7s} {field:10s} median {statistics.median(v):9.2f}  min {min(v):9.2f}  max {max(v):9.2f}")
    if failed:
        raise SystemExit(f"ended at {failed['tree']} {failed['case']} rep {failed['rep']}: status {failed['status']}")


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "table":
        table(sys.argv[2])
    elif cmd == "one":
        one(sys.argv[2], sys.argv[3])
    else:
        speed(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 5,
              tuple(sys.argv[5].split(",")) if len(sys.argv) > 5 else ORDER)
