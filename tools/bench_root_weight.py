#!/usr/bin/env python
"""The benchmark workload's captured training step without and with the root weight (HeteroGNN(gnn_root_weight=True), DESIGN.md
section 8): one JSON line per setting -- ms per step (HIP events around ``steps`` replayed steps, side-stream sampler beside them),
whether the step kept the FC_output fold and the fused optimiser launch, the number of trainable tensors, and the kernel launches of
one step issued eagerly (the profiler's count, as tools/bench_layer_norm.py takes it).  'none' is the default step (no root launch);
'root' adds per layer k_root_linear<false> to the forward, k_root_linear<true> and the weight-gradient product's launch pair to the
backward and one [n_node_types, 128, 128] tensor to the optimiser's launch, and runs layer 1 unfolded; 'root+norm' has
gnn_norm='layer' as well.  Each setting runs in a child process of its own (in one process the position of a model, not its
configuration, was measured to set its number: tools/bench_multitrait.py).  Recorded, not promised: no target goes with these
numbers.
usage: python tools/bench_root_weight.py [--steps 200] [--warmup 10] [--settings none,root,root+norm]
                                         [--out profiles/root_weight/bench_root_weight.jsonl]"""
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
ap.add_argument('--settings', default='none,root,root+norm')
ap.add_argument('--out', default=os.path.join('profiles', 'root_weight', 'bench_root_weight.jsonl'))
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
    """Kernel launches of one training step issued eagerly through the body the trainer captured, how many of them are
    k_root_linear, and how many weight-gradient launches (k_tn_gemm / k_tn_reduce) there are (None: no profiler here)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        gs._sample_now(0, 0)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            gs._step_body(0)
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        kernels = [e for e in ev if 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
        return (len(kernels), sum(1 for e in kernels if 'k_root_linear' in e.name),
                sum(1 for e in kernels if 'k_tn_gemm' in e.name or 'k_tn_reduce' in e.name),
                round(sum(e.device_time for e in kernels if 'k_root_linear' in e.name), 2))
    except Exception as e:                           # the count is a by-product: the timing above it stands
        print(f'no launch count: {e}', file=sys.stderr)
        return None, None, None, None


for p in ps:
    kw = {'none': {}, 'root': dict(gnn_root_weight=True), 'root+norm': dict(gnn_root_weight=True, gnn_norm='layer')}[p]
    with contextlib.redirect_stdout(sys.stderr):
        data = KGWAS_Data.from_synthetic(scale=args.scale, seed=1, mode='fast', gwas_kind='causal', data_path='/tmp/kgwas_bench_0')
        ids = np.asarray(data.train_input_nodes[1])[:bs * (args.steps + args.warmup)]
        run = KGWAS(data, device='cuda:0', seed=1)
        run.initialize_model(**kw)
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-4, weight_decay=5e-4, sample_seed=1)
    assert gs.root_weight == ('root' in p) and gs.layer_norm == ('norm' in p) and not gs.dropout and not gs.hidden_dropout
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
    m = gs.meta
    nt = len(run.model.node_types)
    rows = [[int(m.lay_rows[l][t]) for t in range(nt)] for l in range(run.model.num_layers)]   # (static layout: the capacities the launches cover)
    n_launch, n_root, n_tn, us_root = launches_of_one_step(gs)
    line = {'setting': p, 'ms_per_step': round(ms, 4), 'steps': args.steps, 'batch_size': bs,
            'fold_fc': bool(run.model.fold_fc), 'fused_adam': bool(gs.fused_adam),
            'trainable_tensors': sum(1 for q in run.model.parameters() if q.requires_grad),
            'kernel_launches_eager_step': n_launch, 'of_them_k_root_linear': n_root, 'of_them_k_tn': n_tn,
            'k_root_linear_us_eager_step': us_root, 'output_rows_by_layer_and_type': rows, 'loss_last': loss_last}
    print(json.dumps(line), flush=True)
    lines.append(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')
