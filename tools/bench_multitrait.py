#!/usr/bin/env python
"""The benchmark workload's captured training step with T label columns read out of one shared trunk (multi-trait training,
DESIGN.md section 8): one JSON line per T -- ms per step (HIP events around ``steps`` replayed steps, side-stream sampler beside
them) and the launches that make up the read-out node.  Each T runs in a child process of its own: in one process the third
model built was measured 25 % slower whatever its T (T = 16 in the order 1, 4, 16, 32; T = 4 in the reverse order), so the
position, not the read-out, set that number.  Recorded, not
promised: no target goes with these numbers.
``--trait-weights on``: the same graph with per-trait LD weights and per-trait SNP lists (from_synthetic(trait_sample_sizes=,
trait_coverage=): sample sizes 5000 / 20000 / 387113 and coverages 1.0 / 0.6 / 0.3 in turn) -- the weight matrix form of the
read-out, kgw_readout_wmse_mtw_train; ``both``: every T without and with it.
usage: python tools/bench_multitrait.py [--steps 200] [--warmup 10] [--trait-weights off|on|both]
                                        [--out profiles/multitrait/bench_multitrait.jsonl]"""
import argparse
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kgwas_amd import ops
from kgwas_amd.graph_step import GraphTrainStep
from kgwas_amd.kgwas import KGWAS
from kgwas_amd.kgwas_data import KGWAS_Data

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--scale', type=float, default=1.0)
ap.add_argument('--batch-size', type=int, default=512)
ap.add_argument('--traits', default='1,4,16,32')
ap.add_argument('--trait-weights', choices=('off', 'on', 'both'), default='off')
ap.add_argument('--out', default=os.path.join('profiles', 'multitrait', 'bench_multitrait.jsonl'))
args = ap.parse_args()

bs = args.batch_size
lines = []
traits = [int(t) for t in args.traits.split(',')]
modes = ['off', 'on'] if args.trait_weights == 'both' else [args.trait_weights]
if len(traits) * len(modes) > 1:
    for T, mode in [(T, m) for T in traits for m in modes]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--warmup', str(args.warmup),
                            '--scale', str(args.scale), '--batch-size', str(bs), '--traits', str(T), '--trait-weights', mode,
                            '--out', ''], stdout=subprocess.PIPE, text=True, check=True)
        print(r.stdout.strip(), flush=True)
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    traits = []
for T in traits:
    with contextlib.redirect_stdout(sys.stderr):
        per_trait = {}
        if modes[0] == 'on':
            per_trait = {'trait_sample_sizes': [(5000, 20000, 387113)[t % 3] for t in range(T)],
                         'trait_coverage': [(1.0, 0.6, 0.3)[t % 3] for t in range(T)]}
        data = KGWAS_Data.from_synthetic(scale=args.scale, seed=1, mode='fast', gwas_kind='causal', data_path='/tmp/kgwas_bench_0',
                                         n_traits=T, **per_trait)
        ids = np.asarray(data.train_input_nodes[1])[:bs * (args.steps + args.warmup)]
        run = KGWAS(data, device='cuda:0', seed=1)
        run.initialize_model(out_channels=T)
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-4, weight_decay=5e-4)
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
    mtw = per_trait and T > 1
    assert bool(ops.ROUTES.get('kgw_readout_wmse_mtw_train')) == bool(mtw)
    line = {'traits': T, 'trait_weights': bool(per_trait), 'ms_per_step': round(ms, 4), 'steps': args.steps, 'batch_size': bs,
            'readout': ('kgw_readout_wmse_mtw_train' if mtw else 'kgw_readout_wmse_mt_train') if T > 1
            else 'kgw_readout_wmse_train_parts + fold riding',
            'fused_adam': bool(gs.fused_adam), 'library_gemm_calls': ops.LIBRARY_GEMM.calls,
            'loss_last': float(gs.loss[(args.warmup + args.steps - 1) % 2])}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del gs, run, data
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')
