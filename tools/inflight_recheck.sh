#!/bin/bash
# Batches in flight re-checked on the round-6 kernels (timed schedule only, 50 steps, B = 512).
# usage: tools/inflight_recheck.sh [OUTDIR]
set -o pipefail
OUT=${1:-bench_out/inflight}
mkdir -p $OUT
for r in 1 2; do for inf in 2 3 4; do
  timeout -k 10 200 python bench.py --inflight $inf --full --cpu-seconds 0 --serial-steps 0 --steps 50 > $OUT/inf_${inf}_$r.json 2>/dev/null || { echo "FAILED $inf"; exit 1; }
  python -c "import json;j=json.loads(open('$OUT/inf_${inf}_$r.json').read().strip().splitlines()[-1]);print($r,'inflight=$inf',round(j['value']),round(j['ms_per_step'],4),j['verified'])"
done; done
