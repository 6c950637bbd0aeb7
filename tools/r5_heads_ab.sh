#!/bin/bash
# config 4 with the small-launch heads at the default cap, off, and below 1024 rows only
set -o pipefail
mkdir -p ${OUT_DIR:-build/out}/r5hd
for r in 1; do
for cap in -1 0; do
  GZ_GN_SMALL_HEADS=$cap timeout -k 10 300 python -u bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --fp32-steps 0 --no-elided --config5-games 0 --config4-steps 6 > ${OUT_DIR:-build/out}/r5hd/ab_${cap}_$r.json 2> ${OUT_DIR:-build/out}/r5hd/ab_${cap}_$r.err || { tail -20 ${OUT_DIR:-build/out}/r5hd/ab_${cap}_$r.err; exit 1; }
  python -c "
import json; d=json.loads(open('${OUT_DIR:-build/out}/r5hd/ab_${cap}_$r.json').read().strip().splitlines()[-1]); print('cap $cap rep $r config4', d['config4']['value'], d['config4']['ms_per_step'])"
done
done
