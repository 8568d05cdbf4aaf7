set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT"
mkdir -p bench_out
timeout -k 10 300 python tools/gpu/score_diag.py > bench_out/diag2.log 2>&1 || { tail -30 bench_out/diag2.log; exit 1; }
cat bench_out/diag2.log
timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 > bench_out/bench.json 2> bench_out/bench.err || { tail -30 bench_out/bench.err; exit 1; }
cat bench_out/bench.json
