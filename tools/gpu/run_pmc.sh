# PMC counter passes (one counter group per run, kernel-trace only, no
# sys/runtime trace) over a short decode+score bench, then the summary.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT"
mkdir -p bench_out/pmc
cd /tmp && export TMPDIR=/tmp
i=0
for set in "FETCH_SIZE" "WRITE_SIZE" "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_SMEM" "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_BUSY_CYCLES GRBM_GUI_ACTIVE" "TCC_HIT_sum TCC_MISS_sum TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum"; do
  i=$((i+1))
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc $set --output-format csv -d "$ROOT/bench_out/pmc/p$i" -o run -- python3 "$ROOT/bench.py" --full --steps 1 --warmup 1 --no-cpu-baseline "$@" > "$ROOT/bench_out/pmc/p$i.log" 2>&1 \
    || { echo "pass $i ($set) failed"; tail -20 "$ROOT/bench_out/pmc/p$i.log"; exit 1; }
done
cd "$ROOT"
python tools/pmc_summary.py bench_out/pmc/p1 bench_out/pmc/p2 bench_out/pmc/p3 bench_out/pmc/p4 bench_out/pmc/p5 --json bench_out/pmc/summary.json
