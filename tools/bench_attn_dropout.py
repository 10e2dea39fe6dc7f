#!/usr/bin/env python
"""The benchmark workload's captured training step without and with attention dropout (HeteroGNN(gat_dropout=p), DESIGN.md
section 8): one JSON line per p -- ms per step (HIP events around ``steps`` replayed steps, side-stream sampler beside them).
p = 0 is the default step (dropout=None: the plain kernels, no word copy); p > 0 takes the DROP instantiations of k_agg_fwd and
k_agg_bwd_dst in both layers plus one 8-byte device copy per step.  Each p runs in a child process of its own (in one process
the position of a model, not its configuration, was measured to set its number: tools/bench_multitrait.py).  Recorded, not
promised: no target goes with these numbers.
usage: python tools/bench_attn_dropout.py [--steps 200] [--warmup 10] [--p 0,0.1,0.5]
                                          [--out profiles/attn_dropout/bench_attn_dropout.jsonl]"""
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
ap.add_argument('--p', default='0,0.1,0.5')
ap.add_argument('--out', default=os.path.join('profiles', 'attn_dropout', 'bench_attn_dropout.jsonl'))
args = ap.parse_args()

bs = args.batch_size
lines = []
ps = [float(p) for p in args.p.split(',')]
if len(ps) > 1:
    for p in ps:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--warmup', str(args.warmup),
                            '--scale', str(args.scale), '--batch-size', str(bs), '--p', str(p), '--out', ''],
                           stdout=subprocess.PIPE, text=True, check=True)
        print(r.stdout.strip(), flush=True)
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    ps = []
for p in ps:
    with contextlib.redirect_stdout(sys.stderr):
        data = KGWAS_Data.from_synthetic(scale=args.scale, seed=1, mode='fast', gwas_kind='causal', data_path='/tmp/kgwas_bench_0')
        ids = np.asarray(data.train_input_nodes[1])[:bs * (args.steps + args.warmup)]
        run = KGWAS(data, device='cuda:0', seed=1)
        run.initialize_model(gat_dropout=p)
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-4, weight_decay=5e-4, sample_seed=1)
    assert gs.dropout == (p > 0)
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
    line = {'gat_dropout': p, 'ms_per_step': round(ms, 4), 'steps': args.steps, 'batch_size': bs,
            'aggregate': 'k_agg_fwd<DROP> + k_agg_bwd_dst<DROP>, one 8-byte word copy per step' if p > 0 else 'plain kernels',
            'fused_adam': bool(gs.fused_adam), 'loss_last': float(gs.loss[(args.warmup + args.steps - 1) % 2])}
    print(json.dumps(line), flush=True)
    lines.append(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')
