# Round check: GPU tests, default bench line (with CPU baseline), rocprofv3
# kernel stats of the same bench, then a 2-rank torchrun rehearsal (both ranks
# on the one GPU of the box, gloo for the count exchange).
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT"
mkdir -p bench_out
timeout -k 10 600 python -m pytest tests -m gpu -q > bench_out/pytest_gpu.log 2>&1
rc=$?
tail -5 bench_out/pytest_gpu.log
[ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc
timeout -k 10 300 python bench.py --full > bench_out/bench.json 2> bench_out/bench.err || { tail -20 bench_out/bench.err; exit 1; }
cat bench_out/bench.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$ROOT/bench_out/prof" -o run -- python3 "$ROOT/bench.py" --full --steps 10 --warmup 2 --no-cpu-baseline > "$ROOT/bench_out/prof.json" 2> "$ROOT/bench_out/prof.err" \
  || { tail -30 "$ROOT/bench_out/prof.err"; exit 1; }
cat "$ROOT/bench_out/prof.json"
find "$ROOT/bench_out/prof" -name '*kernel_stats.csv' -exec cat {} \;
cd "$ROOT"
timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 3 --warmup 1 --no-cpu-baseline --dist-backend gloo > bench_out/bench2.json 2> bench_out/bench2.err || { tail -20 bench_out/bench2.err; exit 1; }
cat bench_out/bench2.json
