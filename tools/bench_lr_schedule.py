#!/usr/bin/env python
"""The benchmark workload's captured training step three ways (learning-rate schedules and gradient clipping):
'default' (one rate, no clipping: the step bench.py measures), 'cosine' (GraphTrainStep(lr_schedule=cosine with a warm-up): the same
route, the fused optimiser launch in its kgw_adam_fused_ctl form) and 'cosine+clip' (grad_clip_norm as well: the unfused optimiser
route plus the two norm launches).  One JSON line per setting -- ms per step (HIP events around ``steps`` replayed steps, side-stream
sampler beside them), whether the step kept the fused optimiser launch, how many gradients that launch finishes, the kernel launches
of one step issued eagerly (the profiler's count), the rate after the last step, and for the clipped step the last norm and
coefficient.  Each setting runs in a child process of its own (in one process the position of a model, not its configuration, was
measured to set its number: tools/bench_multitrait.py).  Recorded, not promised: no target goes with these numbers.
usage: python tools/bench_lr_schedule.py [--steps 200] [--warmup 10] [--settings default,cosine,cosine+clip] [--clip 1.0]
                                         [--out profiles/lr_schedule/bench.jsonl]"""
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
ap.add_argument('--clip', type=float, default=1.0)
ap.add_argument('--settings', default='default,cosine,cosine+clip')
ap.add_argument('--out', default=os.path.join('profiles', 'lr_schedule', 'bench.jsonl'))
args = ap.parse_args()

bs = args.batch_size
lines = []
ps = args.settings.split(',')
if len(ps) > 1:
    for p in ps:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--warmup', str(args.warmup),
                            '--scale', str(args.scale), '--batch-size', str(bs), '--clip', str(args.clip), '--settings', p, '--out', ''],
                           stdout=subprocess.PIPE, text=True, check=True)
        print(r.stdout.strip(), flush=True)
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    ps = []


def launches_of_one_step(gs):
    """Kernel launches of one training step issued eagerly through the body the trainer captured, and how many of them are the
    norm kernels (None: no profiler here)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        gs._sample_now(0, 0)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            gs._step_body(0)
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        kernels = [e for e in ev if 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
        return (len(kernels), sum(1 for e in kernels if 'k_grad_norm' in e.name),
                round(sum(e.device_time for e in kernels if 'k_grad_norm' in e.name), 2),
                round(sum(e.device_time for e in kernels if 'k_adam' in e.name), 2))
    except Exception as e:                           # the count is a by-product: the timing above it stands
        print(f'no launch count: {e}', file=sys.stderr)
        return None, None, None, None


for p in ps:
    total = args.steps + args.warmup
    sched = {'kind': 'cosine', 'warmup_steps': max(1, total // 20), 'min_lr': 1e-6, 'total_steps': total}
    kw = {'default': {}, 'cosine': dict(lr_schedule=sched), 'cosine+clip': dict(lr_schedule=sched, grad_clip_norm=args.clip)}[p]
    with contextlib.redirect_stdout(sys.stderr):
        data = KGWAS_Data.from_synthetic(scale=args.scale, seed=1, mode='fast', gwas_kind='causal', data_path='/tmp/kgwas_bench_0')
        ids = np.asarray(data.train_input_nodes[1])[:bs * total]
        run = KGWAS(data, device='cuda:0', seed=1)
        run.initialize_model()
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-4, weight_decay=5e-4, sample_seed=1, **kw)
    assert (gs.lr_schedule is not None) == ('cosine' in p) and (gs.grad_clip_norm is not None) == ('clip' in p)
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
    line = {'setting': p, 'ms_per_step': round(ms, 4), 'steps': args.steps, 'batch_size': bs,
            'fused_adam': bool(gs.fused_adam), 'deferred_gradients': int(gs.deferred_gradients),
            'trainable_tensors': sum(1 for q in run.model.parameters() if q.requires_grad),
            'last_lr': float(gs.opt.last_lr) if hasattr(gs.opt, 'last_lr') else None,
            'last_grad_norm': float(gs.opt.last_grad_norm) if 'clip' in p else None,
            'last_clip_scale': float(gs.opt.last_clip_scale) if 'clip' in p else None, 'loss_last': loss_last}
    n_launch, n_norm, us_norm, us_adam = launches_of_one_step(gs)
    line.update({'kernel_launches_eager_step': n_launch, 'of_them_k_grad_norm': n_norm, 'k_grad_norm_us_eager_step': us_norm,
                 'k_adam_us_eager_step': us_adam})
    print(json.dumps(line), flush=True)
    lines.append(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')
