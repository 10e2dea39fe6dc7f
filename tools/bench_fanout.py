#!/usr/bin/env python
"""The benchmark workload's captured training step at full neighbourhoods and at finite fan-outs: one JSON line per
num_neighbors -- ms per step (HIP events around ``steps`` replayed steps, side-stream sampler beside them), edges aggregated
per layer and step, and the sampler replayed alone.  Recorded, not promised: no target goes with these numbers.
usage: python tools/bench_fanout.py [--steps 200] [--warmup 10] [--out profiles/fanout/bench_fanout.jsonl]"""
import argparse
import contextlib
import json
import os
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
ap.add_argument('--fanouts', default='-1,-1;25,10;10,10;10,5')
ap.add_argument('--out', default=os.path.join('profiles', 'fanout', 'bench_fanout.jsonl'))
args = ap.parse_args()

with contextlib.redirect_stdout(sys.stderr):
    data = KGWAS_Data.from_synthetic(scale=args.scale, seed=1, mode='fast', gwas_kind='causal', data_path='/tmp/kgwas_bench_0')
bs = args.batch_size
ids = np.asarray(data.train_input_nodes[1])[:bs * (args.steps + args.warmup)]
lines = []
for spec in args.fanouts.split(';'):
    nn = [int(k) for k in spec.split(',')]
    with contextlib.redirect_stdout(sys.stderr):
        run = KGWAS(data, device='cuda:0', seed=1)
        run.initialize_model(gnn_num_layers=len(nn))
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-4, weight_decay=5e-4, num_neighbors=nn, sample_seed=1)
    for i in range(args.warmup):
        gs.step(i)
    gs.check()
    gs.stats.zero_()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(args.steps):
        gs.step(args.warmup + i)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    st = gs.check()                               # raises if a batch outgrew the static capacities
    L = len(nn)
    ov = gs.measure_overlap(min(args.steps, 20))
    line = {'num_neighbors': nn, 'ms_per_step': round(ms, 4), 'steps': args.steps, 'batch_size': bs,
            'edges_per_layer_per_step': [round(int(st[l]) / args.steps, 1) for l in range(L)],
            'edges_sampled_per_step': round(int(st[L]) / args.steps, 1),
            'sampler_alone_ms': round(ov.get('sampler_alone_ms', float('nan')), 4),
            'step_without_sampler_ms': round(ov.get('step_alone_ms', float('nan')), 4),
            'caps_edges': [int(e) for e in gs.caps.edges], 'loss_last': float(gs.loss[(args.warmup + args.steps - 1) % 2])}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del gs, run
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    for line in lines:
        f.write(json.dumps(line) + '\n')
