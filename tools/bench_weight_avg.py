#!/usr/bin/env python
"""The benchmark workload's captured training step with and without weight averaging (weight averaging):
'none' (the step bench.py measures), 'ema' and 'swa' (GraphTrainStep(weight_average=...): the same route plus one launch at the end
of the step, every update an averaging event) and, on request, 'idle' (an EMA whose first event lies beyond the run: the launch is
there and exits at once -- what the launch itself costs).  One JSON line per setting -- ms per step (HIP events around ``steps``
replayed steps, side-stream sampler beside them), whether the step kept the fused optimiser launch, the kernel launches of one step
issued eagerly (the profiler's count) and the device time of the averaging kernel in it, the parameter elements the launch covers
and the bytes an event moves (12 per element: parameter and shadow read, shadow written).  Each setting runs in a child process of
its own (in one process the position of a model, not its configuration, was measured to set its number: tools/bench_multitrait.py).
Recorded, not promised: no target goes with these numbers.
usage: python tools/bench_weight_avg.py [--steps 200] [--warmup 10] [--settings none,ema,swa[,idle]]
                                        [--out profiles/weight_avg/bench_weight_avg.jsonl]"""
import argparse
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kgwas_amd.graph_step import GraphTrainStep
from kgwas_amd.kgwas import KGWAS
from kgwas_amd.kgwas_data import KGWAS_Data

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--scale', type=float, default=1.0)
ap.add_argument('--batch-size', type=int, default=512)
ap.add_argument('--settings', default='none,ema,swa')
ap.add_argument('--out', default=os.path.join('profiles', 'weight_avg', 'bench_weight_avg.jsonl'))
args = ap.parse_args()

bs = args.batch_size
lines = []
ps = args.settings.split(',')
if len(ps) > 1:
    for p in ps:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--warmup', str(args.warmup),
                            '--scale', str(args.scale), '--batch-size', str(bs), '--settings', p, '--out', ''],
                           stdout=subprocess.PIPE, text=True, check=True)
        print(r.stdout.strip(), flush=True)
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    ps = []


def launches_of_one_step(gs):
    """Kernel launches of one training step issued eagerly through the body the trainer captured, how many of them are the
    averaging kernel, its device time and the optimiser launch's (None: no profiler here)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        gs._sample_now(0, 0)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            gs._step_body(0)
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        kernels = [e for e in ev if 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
        return (len(kernels), sum(1 for e in kernels if 'k_weight_avg' in e.name),
                round(sum(e.device_time for e in kernels if 'k_weight_avg' in e.name), 2),
                round(sum(e.device_time for e in kernels if 'k_adam' in e.name), 2))
    except Exception as e:                           # the count is a by-product: the timing above it stands
        print(f'no launch count: {e}', file=sys.stderr)
        return None, None, None, None


for p in ps:
    total = args.steps + args.warmup
    kw = {'none': {}, 'ema': dict(weight_average='ema'), 'swa': dict(weight_average='swa'),
          'idle': dict(weight_average={'kind': 'ema', 'start_step': 2 ** 30})}[p]
    with contextlib.redirect_stdout(sys.stderr):
        data = KGWAS_Data.from_synthetic(scale=args.scale, seed=1, mode='fast', gwas_kind='causal', data_path='/tmp/kgwas_bench_0')
        ids = np.asarray(data.train_input_nodes[1])[:bs * total]
        run = KGWAS(data, device='cuda:0', seed=1)
        run.initialize_model()
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-4, weight_decay=5e-4, sample_seed=1, **kw)
    assert (gs.avg_model is not None) == (p != 'none')
    for i in range(args.warmup):
        gs.step(i)
    gs.check()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(args.steps):
        gs.step(args.warmup + i)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    gs.check()                                    # raises if a batch outgrew the static capacities
    loss_last = float(gs.loss[(args.warmup + args.steps - 1) % 2])
    elements = sum(q.numel() for q in run.model.parameters())
    moved = None
    if gs.avg_model is not None:                  # how far the shadow is from the raw weights, relative to the weights
        num = sum(float((s.double() - q.double()).pow(2).sum()) for s, q in zip(gs.avg_model.parameters(), run.model.parameters()))
        den = sum(float(q.double().pow(2).sum()) for q in run.model.parameters())
        moved = (num / den) ** 0.5
    line = {'setting': p, 'ms_per_step': round(ms, 4), 'steps': args.steps, 'batch_size': bs,
            'fused_adam': bool(gs.fused_adam), 'deferred_gradients': int(gs.deferred_gradients),
            'parameter_tensors': sum(1 for _ in run.model.parameters()), 'parameter_elements': elements,
            'bytes_per_event': 12 * elements, 'shadow_distance_rel': moved, 'loss_last': loss_last}
    n_launch, n_avg, us_avg, us_adam = launches_of_one_step(gs)
    line.update({'kernel_launches_eager_step': n_launch, 'of_them_k_weight_avg': n_avg, 'k_weight_avg_us_eager_step': us_avg,
                 'k_adam_us_eager_step': us_adam})
    print(json.dumps(line), flush=True)
    lines.append(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')
