#!/usr/bin/env python
"""The benchmark workload's captured training step under the three epoch orders (KGWAS.train(shuffle=False | True | 'batches'),
DESIGN.md section 8): one JSON line per order -- ms per step (HIP events around ``steps`` replayed steps of epoch 0, side-stream
sampler beside them), edges aggregated per layer and step, the static capacities, the sampler replayed alone, the seconds the
dry pass over one epoch's batches took, and kgw_epoch_order alone.  The seeds are ALL training SNPs (an order over a genome-
contiguous prefix would not show what a shuffle does to a batch's subgraph).  Each order runs in a child process of its own (in
one process the position of a model, not its configuration, was measured to set its number: tools/bench_multitrait.py).
Recorded, not promised: no target goes with these numbers.
usage: python tools/bench_shuffle.py [--steps 200] [--warmup 10] [--orders fixed,batches,seeds]
                                     [--out profiles/shuffle/bench_shuffle.jsonl]"""
import argparse
import contextlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--scale', type=float, default=1.0)
ap.add_argument('--batch-size', type=int, default=512)
ap.add_argument('--orders', default='fixed,batches,seeds')
ap.add_argument('--out', default=os.path.join('profiles', 'shuffle', 'bench_shuffle.jsonl'))
args = ap.parse_args()

bs = args.batch_size
lines = []
names = args.orders.split(',')
for n in names:
    if n not in ('fixed', 'batches', 'seeds'):
        raise SystemExit(f'unknown order {n!r}: fixed, batches or seeds')
if len(names) > 1:
    for n in names:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--warmup', str(args.warmup),
                            '--scale', str(args.scale), '--batch-size', str(bs), '--orders', n, '--out', ''],
                           stdout=subprocess.PIPE, text=True, check=True)
        print(r.stdout.strip(), flush=True)
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    names = []

for order in names:
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.kgwas_data import KGWAS_Data
    from kgwas_amd.sampler import NeighborLoader, epoch_order, order_word
    with contextlib.redirect_stdout(sys.stderr):
        data = KGWAS_Data.from_synthetic(scale=args.scale, seed=1, mode='fast', gwas_kind='causal', data_path='/tmp/kgwas_bench_0')
        ids = np.asarray(data.train_input_nodes[1])
        if len(ids) // bs < args.steps + args.warmup:
            raise SystemExit(f'{len(ids) // bs} batches in an epoch: fewer than --steps + --warmup')
        run = KGWAS(data, device='cuda:0', seed=1)
        run.initialize_model()
        run.model.train()
        # the dry pass alone (the trainer below makes it again for itself)
        probe = NeighborLoader(data.data, [-1, -1], ('SNP', ids), batch_size=bs, drop_last=True, device='cuda:0', prefetch=False, seed=1,
                               epoch_order=order)
        torch.cuda.synchronize()
        t = time.perf_counter()
        probe.measure_caps(epochs=1)
        dry = time.perf_counter() - t
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-4, weight_decay=5e-4, sample_seed=1, epoch_order=order, epochs=1)
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
    loss_last = float(gs.loss[(args.warmup + args.steps - 1) % 2])
    gs.set_epoch(0)
    ov = gs.measure_overlap(min(args.steps, 20))
    order_ms = None
    if order != 'fixed':
        d_ids = probe.ids
        out = epoch_order(d_ids, bs, order, order_word(1, 0))
        torch.cuda.synchronize()
        e0.record()
        for ep in range(20):
            epoch_order(d_ids, bs, order, order_word(1, ep), out=out)
        e1.record()
        torch.cuda.synchronize()
        order_ms = round(e0.elapsed_time(e1) / 20, 4)
    line = {'epoch_order': order, 'ms_per_step': round(ms, 4), 'steps': args.steps, 'batch_size': bs, 'batches_per_epoch': gs.n_batches,
            'edges_per_layer_per_step': [round(int(st[l]) / args.steps, 1) for l in range(2)],
            'edges_sampled_per_step': round(int(st[2]) / args.steps, 1),
            'sampler_alone_ms': round(ov.get('sampler_alone_ms', float('nan')), 4),
            'step_without_sampler_ms': round(ov.get('step_alone_ms', float('nan')), 4),
            'caps_edges': [int(e) for e in gs.caps.edges], 'caps_chunks': [int(c) for c in gs.caps.chunks],
            'caps_nodes': {t: int(gs.caps.node_off[i][-1]) for i, t in enumerate(gs.dg.schema.node_types)},
            'dry_pass_s_per_epoch': round(dry, 3), 'kgw_epoch_order_ms': order_ms, 'loss_last': loss_last}
    print(json.dumps(line), flush=True)
    lines.append(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')
