# Round GPU session: tests, bench (decode+score and score-only), rocprof.
# Every GPU step has its own time limit; the first failure ends the script.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT"
mkdir -p bench_out
step() { echo "== $1"; }
step pytest
timeout -k 10 600 python -m pytest tests -m gpu -x -q > bench_out/pytest_gpu.log 2>&1 \
  || { tail -60 bench_out/pytest_gpu.log; exit 1; }
tail -3 bench_out/pytest_gpu.log
step bench_decode_score
timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 > bench_out/bench.json 2> bench_out/bench.err \
  || { tail -30 bench_out/bench.err; exit 1; }
cat bench_out/bench.json
step bench_score
timeout -k 10 300 python bench.py --full --workload score --steps 10 --warmup 2 --no-cpu-baseline > bench_out/bench_score.json 2> bench_out/bench_score.err \
  || { tail -30 bench_out/bench_score.err; exit 1; }
cat bench_out/bench_score.json
step rocprof
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$ROOT/bench_out/prof" -o run -- python3 "$ROOT/bench.py" --full --steps 3 --warmup 1 --no-cpu-baseline > "$ROOT/bench_out/prof.log" 2>&1 \
  || { tail -30 "$ROOT/bench_out/prof.log"; exit 1; }
find "$ROOT/bench_out/prof" -name '*stats*' | head
echo done
