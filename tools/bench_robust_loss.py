#!/usr/bin/env python
"""The benchmark workload's captured training step with the default loss and with the Huber loss (Huber loss):
'mse1' (the step bench.py measures), 'huber1' (GraphTrainStep(loss='huber'): the same route, the read-out node's Huber instance),
'mse4' and 'huber4' (four label columns with per-trait LD weights and per-trait SNP lists, one delta per trait).  One JSON line per
setting -- ms per step (HIP events around ``steps`` replayed steps, side-stream sampler beside them), whether the step kept the
fused optimiser launch, the kernel launches of one step issued eagerly (the profiler's count, and the names without template
arguments hashed so that two settings' lists compare) and the device time of the read-out node's kernels in it.  Each setting runs
in a child process of its own (in one process the position of a model, not its configuration, was measured to set its number:
tools/bench_multitrait.py).  Against the PARENT commit's default step: tools/ab_lib.sh with the parent's library.  Recorded, not
promised: no target goes with these numbers; the launch list is what the tests hold.
usage: python tools/bench_robust_loss.py [--steps 200] [--warmup 10] [--settings mse1,huber1,mse4,huber4]
                                         [--out profiles/robust_loss/bench_robust_loss.jsonl]"""
import argparse
import contextlib
import hashlib
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
ap.add_argument('--settings', default='mse1,huber1,mse4,huber4')
ap.add_argument('--out', default=os.path.join('profiles', 'robust_loss', 'bench_robust_loss.jsonl'))
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
    """Kernel launches of one training step issued eagerly through the body the trainer captured: their count, a hash of their names
    without template arguments, how many are the read-out node's kernels and those kernels' device time (None: no profiler here)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        gs._sample_now(0, 0)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            gs._step_body(0)
            torch.cuda.synchronize()
        ev = sorted((e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA), key=lambda e: e.time_range.start)
        kernels = [e for e in ev if 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
        names = [e.name.split('<')[0] for e in kernels]
        node = [e for e in kernels if 'k_readout' in e.name]
        return (len(kernels), hashlib.sha256('\n'.join(names).encode()).hexdigest()[:12], len(node),
                round(sum(e.device_time for e in node), 2), sum(1 for e in kernels if 'k_adam_fused' in e.name))
    except Exception as e:                           # the count is a by-product: the timing above it stands
        print(f'no launch count: {e}', file=sys.stderr)
        return None, None, None, None, None


for p in ps:
    total = args.steps + args.warmup
    kind, T = p.rstrip('0123456789'), int(p[len(p.rstrip('0123456789')):] or 1)
    if kind not in ('mse', 'huber') or not 1 <= T <= 32:
        raise SystemExit(f'setting {p!r}: mse<T> or huber<T>, T from 1 to 32')
    delta = [(0.5, 1.0, 2.0, 4.0)[t % 4] for t in range(T)] if T > 1 else 1.0
    loss = None if kind == 'mse' else {'kind': 'huber', 'delta': delta}
    with contextlib.redirect_stdout(sys.stderr):
        per_trait = {}
        if T > 1:
            per_trait = {'n_traits': T, 'trait_sample_sizes': [(5000, 20000, 387113)[t % 3] for t in range(T)],
                         'trait_coverage': [(1.0, 0.6, 0.3)[t % 3] for t in range(T)]}
        data = KGWAS_Data.from_synthetic(scale=args.scale, seed=1, mode='fast', gwas_kind='causal', data_path='/tmp/kgwas_bench_0',
                                         **per_trait)
        ids = np.asarray(data.train_input_nodes[1])[:bs * total]
        run = KGWAS(data, device='cuda:0', seed=1)
        run.initialize_model(**({'out_channels': T} if T > 1 else {}))
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-4, weight_decay=5e-4, sample_seed=1, loss=loss)
    assert (gs.loss_rule is not None) == (kind == 'huber')
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
    line = {'setting': p, 'loss': kind, 'traits': T, 'delta': delta if kind == 'huber' else None, 'ms_per_step': round(ms, 4),
            'steps': args.steps, 'batch_size': bs, 'fused_adam': bool(gs.fused_adam), 'deferred_gradients': int(gs.deferred_gradients),
            'loss_last': loss_last}
    n_launch, names_hash, n_node, us_node, n_adam = launches_of_one_step(gs)
    line.update({'kernel_launches_eager_step': n_launch, 'launch_names_sha': names_hash, 'of_them_k_readout': n_node,
                 'k_readout_us_eager_step': us_node, 'of_them_k_adam_fused': n_adam})
    print(json.dumps(line), flush=True)
    lines.append(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')
