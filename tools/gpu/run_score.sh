set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT"
mkdir -p bench_out
( ls /opt/rocm/lib | grep -i -E 'decode|va' ; ls /usr/lib/x86_64-linux-gnu | grep -i -E 'libva|avcodec' ; which ffmpeg ffprobe ; rocm-smi --showproductname ; nproc ) > bench_out/box_probe.txt 2>&1 || true
timeout -k 10 400 python -m pytest tests/test_score_gpu.py -x -q > bench_out/pytest_gpu.log 2>&1 || { echo "pytest failed"; tail -40 bench_out/pytest_gpu.log; exit 1; }
timeout -k 10 300 python bench.py --full --workload score --steps 10 --warmup 2 > bench_out/bench_score.log 2>&1 || { echo "bench failed"; tail -30 bench_out/bench_score.log; exit 1; }
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$ROOT/bench_out/prof_score" -o prof -- python3 "$ROOT/bench.py" --full --workload score --steps 3 --warmup 1 --no-cpu-baseline > "$ROOT/bench_out/prof_score.log" 2>&1 || { echo "rocprof failed"; tail -30 "$ROOT/bench_out/prof_score.log"; exit 1; }
echo done
