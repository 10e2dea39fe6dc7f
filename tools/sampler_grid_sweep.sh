#!/bin/bash
# Step time of the default bench against the side sampler's launch geometry (gpurun, repo root):
#   SGS="256 1024" SHIFTS="8 11 12" bash tools/sampler_grid_sweep.sh     (SHIFTS: KGW_TS_MIN_SHIFT, log2 of the sort's rows per bucket;
#   the key-block count was swept with a temporary knob in round 6 -- 128 / 256 / 512: 1.035 / 1.034 / 1.048 ms -- and stays 256)
# The bench lines and their logs go to $OUT_DIR (default: a new temporary directory).
o=${OUT_DIR:-$(mktemp -d)}
for sg in ${SGS:-256 512 1024}; do
 for sh in ${SHIFTS:-11}; do
  KGW_TS_MIN_SHIFT=$sh KGW_SIDE_SAMPLER_GRID=$sg python bench.py --full --steps 200 --warmup 10 --no-cpu-baseline --no-pmc --no-epoch --no-kernel-timing > $o/sg_$sg.json 2> $o/sg_$sg.err
  python - $o $sg $sh <<'PY'
import json, sys
od, sg, sh = sys.argv[1:4]
try:
    d = json.loads(open('%s/sg_%s.json' % (od, sg)).read().strip().splitlines()[-1])
    o = d['config'].get('sampler_overlap') or {}
    print('SG %5s shift %2s  ms/step %.4f   with %.4f  alone %.4f  sampler alone %.4f' % (sg, sh, d['ms_per_step'], o.get('step_with_side_sampler_ms', 0), o.get('step_alone_ms', 0), o.get('sampler_alone_ms', 0)))
except Exception as e:
    print('SG', sg, sh, 'failed', e)
PY
 done
done
echo "lines and logs: $o"
