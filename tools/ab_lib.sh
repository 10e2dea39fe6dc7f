#!/bin/bash
# A/B of two builds on one box: the default bench alternating between kgwas_amd/csrc/libkgwas_hip_prev.so (KGW_LIB_PATH) and the
# current library.  usage (gpurun, repo root): bash tools/ab_lib.sh [rounds] [extra bench args]
# AB_PLAIN=1: one plain `bench.py --gpus 1 --steps 40 --warmup 5` line per entry, alternating like AB_TRAITS (the yardstick of a
# feature's default step against its parent: profiles/*/ab_prev_vs_cur.txt).
# AB_TRAITS=T: the captured step of tools/bench_multitrait.py with T shared-weight label columns instead of the default bench; odd
# rounds run prev then cur, even rounds cur then prev, so that the prev lines show what the position in a pair alone does.
n=${1:-3}; shift
if [ -n "$AB_PLAIN" ]; then
  for i in $(seq $n); do
    if [ $((i % 2)) = 1 ]; then order="prev cur"; else order="cur prev"; fi
    pos=0
    for which in $order; do
      pos=$((pos + 1))
      if [ $which = prev ]; then export KGW_LIB_PATH=$PWD/kgwas_amd/csrc/libkgwas_hip_prev.so; else unset KGW_LIB_PATH; fi
      python bench.py --gpus 1 --steps 40 --warmup 5 "$@" 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
print('round $i position $pos  $which  ms/step %.4f' % d['ms_per_step'])" || exit 1
    done
  done
  exit 0
fi
if [ -n "$AB_TRAITS" ]; then
  for i in $(seq $n); do
    if [ $((i % 2)) = 1 ]; then order="prev cur"; else order="cur prev"; fi
    for which in $order; do
      if [ $which = prev ]; then export KGW_LIB_PATH=$PWD/kgwas_amd/csrc/libkgwas_hip_prev.so; else unset KGW_LIB_PATH; fi
      python tools/bench_multitrait.py --traits $AB_TRAITS --out '' "$@" 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
print('$which  T=%d  ms/step %.4f' % (d['traits'], d['ms_per_step']))" || exit 1
    done
  done
  exit 0
fi
for i in $(seq $n); do
  for which in prev cur; do
    if [ $which = prev ]; then export KGW_LIB_PATH=$PWD/kgwas_amd/csrc/libkgwas_hip_prev.so; else unset KGW_LIB_PATH; fi
    python bench.py --full --steps 200 --warmup 10 --no-cpu-baseline --no-pmc --no-epoch --no-kernel-timing "$@" 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); o=d['config']['sampler_overlap']
print('$which  ms/step %.4f   alone %.4f  sampler alone %.4f' % (d['ms_per_step'], o['step_alone_ms'], o['sampler_alone_ms']))"
  done
done
