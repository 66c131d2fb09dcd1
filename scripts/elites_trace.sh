#!/bin/bash
# The selection kernel's own durations beside the lambda search's on the same cost buffer (the
# elites table): one rocprofv3 kernel trace per shape of tools/elites_bench.py --trace (30 launches of each kernel at
# n_elite = K / 10 and at K / 2).
#   bash scripts/elites_trace.sh [out_dir]        (from the repository root, on the GPU box)
set -o pipefail
out=${1:-bench_out/elites_trace}
mkdir -p "$out"
for shape in config4 config4-shard config5 kMaxK; do
  d=$out/$shape
  timeout -k 10 240 rocprofv3 --kernel-trace --stats -d "$d" -o run --output-format csv -- \
    python3 tools/elites_bench.py --trace --only $shape > "$d.log" 2>&1 || { echo "$shape failed"; tail -5 "$d.log"; exit 1; }
  echo "## $shape"
  find "$d" -name '*kernel_stats.csv' | head -1 | xargs -r grep -E 'Name|elite_|lambda_' | cut -c1-260
  find "$d" -name '*kernel_trace.csv' -delete
done
