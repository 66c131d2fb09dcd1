#!/bin/bash
# The gather and inject kernels' own durations beside the control-cost term kernel's on the same noise buffer (DESIGN.md
# section 4, the kept-elites table): one rocprofv3 kernel trace (kernel trace only, a run of its own) per shape of
# tools/elite_keep_bench.py --trace (20 launches of each kernel at n_keep = K / 32 and at K / 8).
#   bash scripts/elite_keep_trace.sh [out_dir]        (from the repository root, on the GPU box)
set -o pipefail
out=${1:-bench_out/elite_keep_trace}
mkdir -p "$out"
for shape in config4 config4-shard config5 config2; do
  d=$out/$shape
  timeout -k 10 240 rocprofv3 --kernel-trace --stats -d "$d" -o run --output-format csv -- \
    python3 tools/elite_keep_bench.py --trace --only $shape > "$d.log" 2>&1 || { echo "$shape failed"; tail -5 "$d.log"; exit 1; }
  echo "## $shape"
  find "$d" -name '*kernel_stats.csv' | head -1 | xargs -r grep -E 'Name|keep_|elite_|ctrl_' | cut -c1-260
  find "$d" -name '*kernel_trace.csv' -delete
done
