#!/bin/bash
# A row-panel chain against the launches it replaces under PMC counters: L2 hit rate and fabric bytes per launch, and the sum per arm.  Counters only
# (no trace domain beside them), two passes per arm.  Run ON THE GPU BOX from the repo root: bash tools/pmc_panel_chain.sh [chain]
#   chain 0 (default) = E4 against enc4.conv1-3 per layer, 1 = D3T against dec3.conv2-3, 2 = D43 against lin 15 + lin 16 per layer + D3T
set -e
CHAIN=${1:-0}
ROOT=$(pwd)
OUT=${PMC_OUT:-$ROOT/build/pmc_panel}      # (build/ is git-ignored)
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
for arm in chain layers; do
  timeout -k 10 120 rocprofv3 --pmc FETCH_SIZE -d $OUT/f_$arm -o f --output-format csv -- python3 $ROOT/tools/one_panel_chain.py $arm $CHAIN 10 > $OUT/f_$arm.log 2>&1
  timeout -k 10 120 rocprofv3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum -d $OUT/w_$arm -o w --output-format csv -- python3 $ROOT/tools/one_panel_chain.py $arm $CHAIN 10 > $OUT/w_$arm.log 2>&1
done
cd $ROOT
python3 - <<PY
import csv, glob, collections
def per_kernel(root, counter):
    f = glob.glob(f"{root}/**/*_counter_collection.csv", recursive=True)[0]
    v = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        if ("gemm_x" in r["Kernel_Name"] or "panel_chain" in r["Kernel_Name"]) and r["Counter_Name"] == counter:
            v[r["Kernel_Name"].split("(")[0][:60]].append(float(r["Counter_Value"]))
    return {k: (sum(x[len(x) // 3:]) / len(x[len(x) // 3:]), len(x)) for k, x in v.items()}
o = "$OUT"
for arm in ("chain", "layers"):
    fetch, write = per_kernel(f"{o}/f_{arm}", "FETCH_SIZE"), per_kernel(f"{o}/w_{arm}", "WRITE_SIZE")
    hit, miss = per_kernel(f"{o}/w_{arm}", "TCC_HIT_sum"), per_kernel(f"{o}/w_{arm}", "TCC_MISS_sum")
    tot_r = tot_w = 0.0
    for k in fetch:
        n = fetch[k][1] // 10
        tot_r += n * fetch[k][0] * 2048 / 1e6; tot_w += n * write[k][0] * 1024 / 1e6
        print(f"{arm}: {k} ({n} launch(es) per pass): per launch fabric read {fetch[k][0] * 2048 / 1e6:7.1f} MB (FETCH_SIZE x 2 KiB) write {write[k][0] * 1024 / 1e6:6.1f} MB | "
              f"L2 hit rate {hit[k][0] / (hit[k][0] + miss[k][0]):.3f} (hits {hit[k][0]:.3e} misses {miss[k][0]:.3e})")
    print(f"{arm}: all its launches, per pass: fabric read {tot_r:7.1f} MB write {tot_w:7.1f} MB")
PY
