# Other BASELINE configurations per GPU: bash run_configs.sh "<bench args>" ...
# (each argument is one bench.py invocation's extra arguments)
set -o pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd "$ROOT"
mkdir -p bench_out
df -h /tmp | tail -1
free -g | head -2
i=0
for args in "$@"; do
  i=$((i+1))
  echo "== $args"
  timeout -k 10 1000 python bench.py --full --no-cpu-baseline $args > bench_out/cfg_$i.json 2> bench_out/cfg_$i.err || { tail -20 bench_out/cfg_$i.err; exit 1; }
  cat bench_out/cfg_$i.json
done
