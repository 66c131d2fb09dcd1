#!/bin/bash
# The bounds kernels' own durations beside the control-cost term kernel's on the same noise buffer (the
# control-bounds section; profiles/control_bounds.log): one rocprofv3 kernel trace per shape and box of
# tools/bounds_bench.py --trace (30 plain counter solves with the bounds and the control-cost term on).
#   bash scripts/bounds_trace.sh [out_dir]        (from the repository root, on the GPU box)
set -o pipefail
out=${1:-bench_out/bounds_trace}
mkdir -p "$out"
for shape in config4 config4-shard config5 config2; do
  for box in never main; do
    d=$out/$shape-$box
    timeout -k 10 240 rocprofv3 --kernel-trace --stats -d "$d" -o run --output-format csv -- \
      python3 tools/bounds_bench.py --trace $box --only $shape > "$d.log" 2>&1 || { echo "$shape $box failed"; tail -5 "$d.log"; exit 1; }
    echo "## $shape, box $box"
    find "$d" -name '*kernel_stats.csv' | head -1 | xargs -r grep -E 'Name|bounds_|ctrl_term|reduce_kernel|rollout|fc_|cartpole' | cut -c1-260
    find "$d" -name '*kernel_trace.csv' -delete
  done
done
