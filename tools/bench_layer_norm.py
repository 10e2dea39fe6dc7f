#!/usr/bin/env python
"""The benchmark workload's captured training step without and with layer normalisation (HeteroGNN(gnn_norm='layer'), DESIGN.md
section 8): one JSON line per setting -- ms per step (HIP events around ``steps`` replayed steps, side-stream sampler beside them),
whether the step kept the FC_output fold and the fused optimiser launch, and the kernel launches of one step issued eagerly (the
profiler's count, as tools/bench_edge_attr.py takes it).  'none' is the default step (no norm launch); 'layer' adds, for the one
site of the two-layer model, k_layer_norm_relu_fwd to the forward and k_layer_norm_bwd + k_layer_norm_fold to the backward, and two
[n_node_types, 128] tensors to the optimiser's launch.  Each setting runs in a child process of its own (in one process the position
of a model, not its configuration, was measured to set its number: tools/bench_multitrait.py).  Recorded, not promised: no target
goes with these numbers.
usage: python tools/bench_layer_norm.py [--steps 200] [--warmup 10] [--norm none,layer]
                                        [--out profiles/layer_norm/bench_layer_norm.jsonl]"""
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
ap.add_argument('--norm', default='none,layer')
ap.add_argument('--out', default=os.path.join('profiles', 'layer_norm', 'bench_layer_norm.jsonl'))
args = ap.parse_args()

bs = args.batch_size
lines = []
ps = args.norm.split(',')
if len(ps) > 1:
    for p in ps:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--warmup', str(args.warmup),
                            '--scale', str(args.scale), '--batch-size', str(bs), '--norm', p, '--out', ''],
                           stdout=subprocess.PIPE, text=True, check=True)
        print(r.stdout.strip(), flush=True)
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    ps = []


def launches_of_one_step(gs):
    """Kernel launches of one training step issued eagerly through the body the trainer captured, and how many of them are
    k_layer_norm_* (None: no profiler here)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        gs._sample_now(0, 0)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            gs._step_body(0)
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        kernels = [e for e in ev if 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
        return len(kernels), sum(1 for e in kernels if 'k_layer_norm' in e.name)
    except Exception as e:                           # the count is a by-product: the timing above it stands
        print(f'no launch count: {e}', file=sys.stderr)
        return None, None


for p in ps:
    with contextlib.redirect_stdout(sys.stderr):
        data = KGWAS_Data.from_synthetic(scale=args.scale, seed=1, mode='fast', gwas_kind='causal', data_path='/tmp/kgwas_bench_0')
        ids = np.asarray(data.train_input_nodes[1])[:bs * (args.steps + args.warmup)]
        run = KGWAS(data, device='cuda:0', seed=1)
        run.initialize_model(gnn_norm=None if p == 'none' else p)
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-4, weight_decay=5e-4, sample_seed=1)
    assert gs.layer_norm == (p != 'none') and not gs.dropout and not gs.hidden_dropout
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
    rows1 = [int(m.lay_rows[0][t]) for t in range(len(run.model.node_types))]      # (static layout: the capacities the launch covers)
    n_launch, n_lnorm = launches_of_one_step(gs)
    line = {'gnn_norm': p, 'ms_per_step': round(ms, 4), 'steps': args.steps, 'batch_size': bs,
            'fold_fc': bool(run.model.fold_fc), 'fused_adam': bool(gs.fused_adam),
            'kernel_launches_eager_step': n_launch, 'of_them_k_layer_norm': n_lnorm,
            'layer1_output_rows_by_type': rows1, 'loss_last': loss_last}
    print(json.dumps(line), flush=True)
    lines.append(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')
