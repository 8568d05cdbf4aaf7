# A/B of bench.py argument sets on the in-tree library (GPU tests first):
#   bash tools/gpu/run_args_ab.sh "<args 1>" "<args 2>" ...
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT"
mkdir -p bench_out
timeout -k 10 600 python -m pytest tests -m gpu -q -x > bench_out/pytest_gpu.log 2>&1 || { tail -40 bench_out/pytest_gpu.log; exit 1; }
tail -2 bench_out/pytest_gpu.log
for pass in $(seq ${PASSES:-2}); do
  i=0
  for a in "$@"; do
    i=$((i+1))
    timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-pmc $a > bench_out/args_$i.json 2> bench_out/args_$i.err || { tail -20 bench_out/args_$i.err; exit 1; }
    python - "$i" "$a" <<'PY'
import json,sys
d=json.load(open(f"bench_out/args_{sys.argv[1]}.json"))
r=d["roofline"]; st=d["config"]["stage_ms"]
print(f"{sys.argv[2]:>28} {d['value']:>11.0f} fps {d['ms_per_step']:7.3f} ms  kernel {r['kernel_ms']:.4f} ms frac {r['frac']:.4f}  parse {st['parse_ms']:.3f} recon {st['reconstruct_ms']:.3f} score {st['score_ms']:.3f} total {st['total_ms']:.3f}")
PY
  done
done
