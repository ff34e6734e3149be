#!/bin/bash
# The N > 1 code path on one GPU (a 1-rank RCCL group), --full: every gather mode's rate and the configs[4] block.
# Usage, from the repo root:  tools/dist1_check.sh <out dir>
OUT=${1:?usage: tools/dist1_check.sh <out dir>}
export ATMO_BENCH_FORCE_DIST=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29517 RANK=0 WORLD_SIZE=1 LOCAL_RANK=0
mkdir -p $OUT
python bench.py --full --steps 20 --warmup 5 > $OUT/dist1_k20.out 2> $OUT/dist1_k20.err
python bench.py --full --steps 200 --warmup 20 > $OUT/dist1_k200.out 2> $OUT/dist1_k200.err
grep -h '^{' $OUT/dist1_k20.out $OUT/dist1_k200.out | python -c "
import sys, json
for l in sys.stdin:
    d = json.loads(l); c = d['config']
    print(d['steps'], round(d['value']), c['gather'][:40], round(c['mrays_per_s_no_gather']), round(c['mrays_per_s_final_gather']), round(c['mrays_per_s_gather_every']), list(d.get('extra', {}).get('config4_clouds_high_rm_3840x2160', {}).items())[:8])
"
