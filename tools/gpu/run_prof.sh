# GPU tests, then rocprofv3 kernel-trace/stats of the decode+score bench.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT"
mkdir -p bench_out
timeout -k 10 600 python -m pytest tests -m gpu -q > bench_out/pytest_gpu.log 2>&1
rc=$?
tail -5 bench_out/pytest_gpu.log
[ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc   # 1 = test failures: still profile
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$ROOT/bench_out/prof" -o run -- python3 "$ROOT/bench.py" --full --steps 3 --warmup 1 --no-cpu-baseline > "$ROOT/bench_out/prof.log" 2>&1 \
  || { tail -30 "$ROOT/bench_out/prof.log"; exit 1; }
find "$ROOT/bench_out/prof" -name '*kernel_stats.csv' -exec cat {} \;
