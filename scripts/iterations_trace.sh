#!/bin/bash
# The tracking kernel's own durations beside the selection's on the same costs (the inner-iterations
# section): one rocprofv3 kernel trace per shape of tools/iterations_bench.py --trace (20 launches of each kernel),
# then, each in a run of its own, counter passes over the same launches of config #4.
#   bash scripts/iterations_trace.sh [out_dir]        (from the repository root, on the GPU box)
set -o pipefail
out=${1:-bench_out/iterations_trace}
mkdir -p "$out"
for shape in config4 kMaxK; do
  d=$out/$shape
  timeout -k 10 240 rocprofv3 --kernel-trace --stats -d "$d" -o run --output-format csv -- \
    python3 tools/iterations_bench.py --trace --only $shape > "$d.log" 2>&1 || { echo "$shape failed"; tail -5 "$d.log"; exit 1; }
  echo "## $shape"
  find "$d" -name '*kernel_stats.csv' | head -1 | xargs -r grep -E 'Name|elite_|iter_' | cut -c1-260
  find "$d" -name '*kernel_trace.csv' -delete
done
i=0
for pass in "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VMEM_RD" "TCP_UTCL1_TRANSLATION_MISS_sum TCP_UTCL1_REQUEST_sum" \
            "TCC_MISS_sum TCC_HIT_sum TCC_EA_RDREQ_sum" "TCP_TCC_READ_REQ_LATENCY_sum TCP_TCC_READ_REQ_sum"; do
  i=$((i + 1))
  d=$out/pmc$i
  timeout -k 10 240 rocprofv3 --pmc $pass -d "$d" -o pmc --output-format csv -- \
    python3 tools/iterations_bench.py --trace --only config4 > "$d.log" 2>&1 || { echo "pass '$pass' failed"; tail -3 "$d.log"; exit 1; }
  python3 - "$d" <<'PY'
import collections, csv, os, sys
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for root, _, fs in os.walk(sys.argv[1]):
    for f in fs:
        if f.endswith("counter_collection.csv"):
            for r in csv.DictReader(open(os.path.join(root, f))):
                if "elite_" in r["Kernel_Name"] or "iter_" in r["Kernel_Name"]:
                    acc[r["Kernel_Name"][:48]][r["Counter_Name"]].append(float(r["Counter_Value"]))
for k, c in acc.items():
    print(k, {n: round(sum(v) / len(v)) for n, v in sorted(c.items())})
PY
done
