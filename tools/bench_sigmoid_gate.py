#!/usr/bin/env python
"""The benchmark workload's captured training step under the softmax, the softmax without the FC_output fold, the sigmoid gate
(HeteroGNN(gat_sigmoid=True)) and the softmax at T = 2: one JSON line per configuration -- ms per step (HIP
events around ``steps`` replayed steps, side-stream sampler beside them).  The gated step takes the GATE instantiations of
k_agg_fwd and k_agg_bwd_dst in both layers and runs layer 1 unfolded (the gates do not sum to 1), so its yardstick is the
softmax step with KGW_FOLD_FC=0, not the default one.  Each configuration runs in a child process of its own (in one process
the position of a model, not its configuration, was measured to set its number: tools/bench_multitrait.py).  Recorded, not
promised: no target goes with these numbers.
usage: python tools/bench_sigmoid_gate.py [--steps 200] [--warmup 10] [--configs softmax,softmax_nofold,sigmoid,softmax_T2]
                                          [--out profiles/sigmoid_gate/bench_sigmoid_gate.jsonl]"""
import argparse
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name -> (initialize_model keywords, KGW_FOLD_FC of the child process)
CONFIGS = {'softmax': ({}, '1'), 'softmax_nofold': ({}, '0'), 'sigmoid': ({'gat_sigmoid': True}, '1'),
           'softmax_T2': ({'gat_temperature': 2.0}, '1')}

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--scale', type=float, default=1.0)
ap.add_argument('--batch-size', type=int, default=512)
ap.add_argument('--configs', default='softmax,softmax_nofold,sigmoid,softmax_T2')
ap.add_argument('--out', default=os.path.join('profiles', 'sigmoid_gate', 'bench_sigmoid_gate.jsonl'))
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
                           stdout=subprocess.PIPE, text=True, check=True, env=dict(os.environ, KGW_FOLD_FC=CONFIGS[n][1]))
        print(r.stdout.strip(), flush=True)
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    names = []
for n in names:
    kw, fold_env = CONFIGS[n]
    os.environ['KGW_FOLD_FC'] = fold_env                   # (read by HeteroGNN.__init__)
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.kgwas_data import KGWAS_Data
    with contextlib.redirect_stdout(sys.stderr):
        data = KGWAS_Data.from_synthetic(scale=args.scale, seed=1, mode='fast', gwas_kind='causal', data_path='/tmp/kgwas_bench_0')
        ids = np.asarray(data.train_input_nodes[1])[:bs * (args.steps + args.warmup)]
        run = KGWAS(data, device='cuda:0', seed=1)
        run.initialize_model(**kw)
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-4, weight_decay=5e-4, sample_seed=1)
    assert run.model.gat_sigmoid == bool(kw.get('gat_sigmoid')) and run.model.temperature == kw.get('gat_temperature', 1.0)
    assert run.model.fold_fc == (fold_env == '1' and not run.model.gat_sigmoid)
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
    line = {'config': n, 'gat_sigmoid': run.model.gat_sigmoid, 'gat_temperature': run.model.temperature, 'fold_fc': bool(run.model.fold_fc),
            'ms_per_step': round(ms, 4), 'steps': args.steps, 'batch_size': bs,
            'aggregate': 'k_agg_fwd<RAW, GATE> + k_agg_bwd_dst<GATE>' if run.model.gat_sigmoid else 'plain kernels',
            'fused_adam': bool(gs.fused_adam), 'loss_last': float(gs.loss[(args.warmup + args.steps - 1) % 2])}
    print(json.dumps(line), flush=True)
    lines.append(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')
