# A/B of libvtseg variants, then the default bench (with its PMC passes).
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT"
PASSES=${PASSES:-2} bash tools/gpu/run_variants.sh "$1" ${@:2} || exit 1
timeout -k 10 600 python bench.py --full > bench_out/bench_pmc.json 2> bench_out/bench_pmc.err || { tail -30 bench_out/bench_pmc.err; exit 1; }
cat bench_out/bench_pmc.json
