# One bench line (with its PMC traffic passes) per argument set, plus the
# rocprofv3 kernel stats of the same command.  bash tools/gpu/run_bench_cfg.sh TAG "<args>"
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT"
mkdir -p bench_out
TAG=$1; ARGS=$2
timeout -k 10 600 python bench.py --full --no-cpu-baseline $ARGS > bench_out/bench_$TAG.json 2> bench_out/bench_$TAG.err || { tail -30 bench_out/bench_$TAG.err; exit 1; }
cat bench_out/bench_$TAG.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$ROOT/bench_out/prof_$TAG" -o run -- python3 "$ROOT/bench.py" --full --no-cpu-baseline --no-pmc --steps 5 --warmup 1 $ARGS > "$ROOT/bench_out/prof_$TAG.log" 2>&1 || { tail -30 "$ROOT/bench_out/prof_$TAG.log"; exit 1; }
cat "$ROOT/bench_out/prof_$TAG/run_kernel_stats.csv"
