# 1080p (k = 6) bench line with live PMC traffic, and the rocprofv3 kernel stats of the same config.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT"
mkdir -p bench_out
timeout -k 10 400 python bench.py --full --config 1080p-2h --frames 54000 --steps 3 --warmup 1 --no-cpu-baseline > bench_out/b1080.json 2> bench_out/b1080.err || { tail -20 bench_out/b1080.err; exit 1; }
cat bench_out/b1080.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$ROOT/bench_out/prof1080" -o run -- python3 "$ROOT/bench.py" --full --config 1080p-2h --frames 54000 --steps 3 --warmup 1 --no-cpu-baseline --no-pmc > "$ROOT/bench_out/prof1080.json" 2> "$ROOT/bench_out/prof1080.err" \
  || { tail -30 "$ROOT/bench_out/prof1080.err"; exit 1; }
cd "$ROOT"
head -4 bench_out/prof1080/run_kernel_stats.csv
