set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT"
mkdir -p bench_out
timeout -k 10 300 python tools/gpu/score_diag.py > bench_out/diag.log 2>&1 || { tail -30 bench_out/diag.log; exit 1; }
timeout -k 10 300 python bench.py --full --workload score --steps 10 --warmup 2 --no-cpu-baseline > bench_out/bench_score.log 2>&1 || { tail -30 bench_out/bench_score.log; exit 1; }
cat bench_out/bench_score.log
