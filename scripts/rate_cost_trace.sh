#!/bin/bash
# The rate term's kernels' own durations beside the control-cost term's on the same noise buffer (DESIGN.md section 4,
# the rate-cost table): one rocprofv3 kernel trace per shape of tools/rate_cost_bench.py --trace (30 plain counter
# solves with both terms on).
#   bash scripts/rate_cost_trace.sh [out_dir]        (from the repository root, on the GPU box)
set -o pipefail
out=${1:-bench_out/rate_cost_trace}
mkdir -p "$out"
for shape in config4 config4-shard config2; do
  d=$out/$shape
  timeout -k 10 240 rocprofv3 --kernel-trace --stats -d "$d" -o run --output-format csv -- \
    python3 tools/rate_cost_bench.py --trace --only $shape > "$d.log" 2>&1 || { echo "$shape failed"; tail -5 "$d.log"; exit 1; }
  echo "## $shape"
  find "$d" -name '*kernel_stats.csv' | head -1 | xargs -r grep -E 'Name|rate_|ctrl_|reduce_kernel' | cut -c1-260
  find "$d" -name '*kernel_trace.csv' -delete
done
