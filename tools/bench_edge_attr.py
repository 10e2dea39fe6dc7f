#!/usr/bin/env python
"""The benchmark workload's captured training step without edge attributes and with D = 1, 4 and 8 attribute columns on every
relation (HeteroGNN(gat_edge_dim=D)): one JSON line per configuration -- ms per step (HIP events around
``steps`` replayed steps, side-stream sampler beside them), whether the step kept the FC_output fold and the fused optimiser
launch, and the kernel launches of one step issued eagerly (the profiler's count; the difference to ``none`` is what the feature
adds: per layer k_edge_term, k_edge_term_bwd and its fold, plus the element-wise framework ops that form w_r and take its
gradient apart).  Each configuration runs in a child process of its own (in one process the position of a model, not its
configuration, was measured to set its number: tools/bench_multitrait.py).  Recorded, not promised: no target goes with these
numbers.
usage: python tools/bench_edge_attr.py [--steps 200] [--warmup 10] [--configs none,D1,D4,D8]
                                       [--out profiles/edge_attr/bench_edge_attr.jsonl]"""
import argparse
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {'none': None, 'D1': 1, 'D4': 4, 'D8': 8}

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--scale', type=float, default=1.0)
ap.add_argument('--batch-size', type=int, default=512)
ap.add_argument('--configs', default='none,D1,D4,D8')
ap.add_argument('--out', default=os.path.join('profiles', 'edge_attr', 'bench_edge_attr.jsonl'))
args = ap.parse_args()

bs = args.batch_size
lines = []
names = args.configs.split(',')
for n in names:
    if n not in CONFIGS:
        raise SystemExit(f'unknown configuration {n!r}: one of {", ".join(CONFIGS)}')
if len(names) > 1:
    for n in names:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--warmup', str(args.warmup),
                            '--scale', str(args.scale), '--batch-size', str(bs), '--configs', n, '--out', ''],
                           stdout=subprocess.PIPE, text=True, check=True)
        print(r.stdout.strip(), flush=True)
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    names = []


def launches_of_one_step(gs):
    """Kernel launches of one training step issued eagerly through the body the trainer captured (None: no profiler here)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        gs._sample_now(0, 0)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            gs._step_body(0)
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        kernels = [e for e in ev if 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
        return len(kernels), sum(1 for e in kernels if 'k_edge_term' in e.name or ('k_agg_fwd' in e.name and 'combine' not in e.name))
    except Exception as e:                           # the count is a by-product: the timing above it stands
        print(f'no launch count: {e}', file=sys.stderr)
        return None, None


for n in names:
    D = CONFIGS[n]
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.kgwas_data import KGWAS_Data
    with contextlib.redirect_stdout(sys.stderr):
        data = KGWAS_Data.from_synthetic(scale=args.scale, seed=1, mode='fast', gwas_kind='causal', data_path='/tmp/kgwas_bench_0',
                                         edge_dim=D)
        ids = np.asarray(data.train_input_nodes[1])[:bs * (args.steps + args.warmup)]
        run = KGWAS(data, device='cuda:0', seed=1)
        run.initialize_model(gat_edge_dim=D)
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-4, weight_decay=5e-4, sample_seed=1)
    assert run.model.edge_dim == D
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
    n_launch, n_named = launches_of_one_step(gs)
    line = {'config': n, 'gat_edge_dim': D, 'attributed_relations': len(run.model.attr_rels), 'fold_fc': bool(run.model.fold_fc),
            'fused_adam': bool(gs.fused_adam), 'ms_per_step': round(ms, 4), 'steps': args.steps, 'batch_size': bs,
            'edges_per_step': [int(v) for v in (gs.stats[:2].cpu() // max(args.warmup + args.steps, 1))],
            'kernel_launches_eager_step': n_launch, 'of_them_k_agg_fwd_and_k_edge_term': n_named, 'loss_last': loss_last}
    print(json.dumps(line), flush=True)
    lines.append(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')
