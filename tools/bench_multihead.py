#!/usr/bin/env python
"""The benchmark workload's captured training step at gat_num_head = 1, 2, 4 (KGWAS.initialize_model(gat_num_head=H)):
one JSON line per H -- ms per step (HIP events around ``steps`` replayed steps, side-stream sampler beside them).  H = 1 is the
default step (the fused route: FC_output fold, parameter riders, fused optimiser launch); H > 1 takes the head kernels of
kgw_aggregate_heads.h in both layers and the unfused route around them (no fold, no riders, masked H x R-stacked transform, Adam as
a launch of its own).  Each H runs in a child process of its own (in one process the position of a model, not its configuration,
was measured to set its number: tools/bench_multitrait.py).  Recorded, not promised: no target goes with these numbers.
A single H with ``--out ''`` writes no file: the body of a `rocprofv3 --kernel-trace --stats` run of its own.
usage: python tools/bench_multihead.py [--steps 200] [--warmup 10] [--heads 1,2,4]
                                       [--out profiles/multihead/bench_multihead.jsonl]"""
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
ap.add_argument('--heads', default='1,2,4')
ap.add_argument('--out', default=os.path.join('profiles', 'multihead', 'bench_multihead.jsonl'))
args = ap.parse_args()

bs = args.batch_size
lines = []
hs = [int(h) for h in args.heads.split(',')]
if len(hs) > 1:
    for h in hs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--warmup', str(args.warmup),
                            '--scale', str(args.scale), '--batch-size', str(bs), '--heads', str(h), '--out', ''],
                           stdout=subprocess.PIPE, text=True, check=True)
        print(r.stdout.strip(), flush=True)
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    hs = []
for h in hs:
    with contextlib.redirect_stdout(sys.stderr):
        data = KGWAS_Data.from_synthetic(scale=args.scale, seed=1, mode='fast', gwas_kind='causal', data_path='/tmp/kgwas_bench_0')
        ids = np.asarray(data.train_input_nodes[1])[:bs * (args.steps + args.warmup)]
        run = KGWAS(data, device='cuda:0', seed=1)
        run.initialize_model(gat_num_head=h)
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-4, weight_decay=5e-4, sample_seed=1)
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
    line = {'gat_num_head': h, 'ms_per_step': round(ms, 4), 'steps': args.steps, 'batch_size': bs,
            'route': 'fused (fold, riders, single-head kernels)' if h == 1 else 'unfused (head kernels, masked stacked transform)',
            'fused_adam': bool(gs.fused_adam), 'loss_last': float(gs.loss[(args.warmup + args.steps - 1) % 2])}
    print(json.dumps(line), flush=True)
    lines.append(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')
