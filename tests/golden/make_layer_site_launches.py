#!/usr/bin/env python
"""Record tests/golden/layer_site_launches.json: for every configuration of CONFIGS, the kernels one training pass of HeteroGNN
launches -- forward_loss(unit_grad=True) and its backward on a NeighborLoader batch of the tiny synthetic graph (32 seeds, fan-out
[-1] * L, training mode, a fixed dropout word): the ORDERED names of the package's own kernels (k_*, template arguments kept,
whitespace stripped) and the NUMBER of all other launches (the framework's).  tests/test_gpu_layer_site_launches.py replays the
same passes and compares.

The fixture pins WHICH launches Python issues, in what order: it is recorded on the commit BEFORE a change that must not alter
them (a refactor of the layer routes), and the changed tree has to reproduce it.  Only the public model API and
tests/helpers.kernel_launches are used, so the file runs on either tree.  Needs a GPU.

    python tests/golden/make_layer_site_launches.py [--out FILE]    # writes the fixture (or FILE in its place)
    python tests/golden/make_layer_site_launches.py --bits FILE     # also: FILE gets SHA-256 digests of the loss, the predictions
        # and every parameter gradient of every configuration, and of the losses and all parameters after two captured
        # GraphTrainStep steps of the default model and of root + norm + dropout: to compare two trees on ONE machine (no digest is
        # committed: bit equality across machines has not been measured)
"""
import hashlib
import json
import os
import re
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

FIXTURE = os.path.join(HERE, 'layer_site_launches.json')
BS = 32
P = 0.3
WORD = 0x5DEECE66D1234567                 # any fixed 64-bit word: the kernels read it, the launches do not depend on it
ALL = dict(root=True, norm='layer', p=P)
CONFIGS = OrderedDict([
    ('default', {}),
    ('root', dict(root=True)),
    ('norm', dict(norm='layer')),
    ('drop', dict(p=P)),
    ('root+norm', dict(root=True, norm='layer')),
    ('root+drop', dict(root=True, p=P)),
    ('norm+drop', dict(norm='layer', p=P)),
    ('root+norm+drop', dict(ALL)),
    ('heads2', dict(heads=2)),
    ('heads2+root+norm+drop', dict(ALL, heads=2)),
    ('mean', dict(aggr='mean')),
    ('mean+root+norm+drop', dict(ALL, aggr='mean')),
    ('min+root+norm+drop', dict(ALL, aggr='min')),
    ('sage+norm+drop', dict(backbone='SAGE', norm='layer', p=P)),
    ('3layers+root+norm+drop', dict(ALL, layers=3)),
])
CAPTURED = OrderedDict([('default', {}), ('root+norm+drop', dict(gnn_root_weight=True, gnn_norm='layer', gnn_dropout=P))])


def tiny_kg(data_path='/tmp/kgwas_synth_tiny'):
    """The ``tiny_kg`` fixture of tests/conftest.py."""
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=data_path)


def own_kernel(name):
    """``name`` cut down to the package's kernel it names -- 'k_root_linear<false>' -- or None for anybody else's."""
    m = re.search(r'\bk_[a-z]\w*', name)
    if m is None:
        return None
    s, depth = name[m.start():], 0
    for i, ch in enumerate(s):
        depth += (ch == '<') - (ch == '>')
        if ch == '(' and depth == 0:                      # the parameter list: not part of the name
            s = s[:i]
            break
    return re.sub(r'\s', '', s)


def make_model(kg, cfg):
    from kgwas_amd.model import HeteroGNN
    torch.manual_seed(3)
    dims = (kg.snp_init_dim_size, kg.gene_init_dim_size, kg.go_init_dim_size)
    aggr = cfg.get('aggr', 'sum')
    model = HeteroGNN(kg.data, 128, 1, cfg.get('layers', 2), cfg.get('backbone', 'GAT'), aggr, *dims, cfg.get('heads', 1),
                      gat_split_heads=True, gnn_dropout=cfg.get('p', 0.0), gnn_norm=cfg.get('norm'),
                      gnn_root_weight=cfg.get('root', False)).cuda()
    with torch.no_grad():
        if aggr == 'min':                 # (the minimum over a gene's relations is negative nearly everywhere: keep the ReLU open)
            for pack in model.live_packs:
                pack.bias.add_(1.0)
        model.lin.bias.fill_(0.5)         # an open read-out ReLU: every parameter gets a gradient
    model.train()
    model.set_dropout_word(WORD)
    return model


def make_batch(kg, layers):
    """As tests/test_gpu_root_weight.py::_batch, at 32 seeds."""
    from kgwas_amd.sampler import NeighborLoader
    ids = np.random.default_rng(0).choice(kg.data['SNP'].x.shape[0], size=BS, replace=False)
    return next(iter(NeighborLoader(kg.data, [-1] * layers, ('SNP', ids), batch_size=BS, device='cuda:0', seed=5)))


def labels(kg):
    g = torch.Generator().manual_seed(9)
    n = kg.data['SNP'].x.shape[0]
    return kg.data['SNP'].y.cuda(), (torch.rand(n, generator=g, dtype=torch.float64) + 0.5).cuda()


def layout(batch, layers, nt):
    """(destination types with rows per layer, (layer, type) pairs whose destination rows are a proper prefix of the type's input
    rows): layer 1 reads the feature MLPs' output (lay_src[0]), layer l > 1 the previous layer's output (lay_rows[l - 2])."""
    m = batch.meta
    rows = [[int(m.lay_rows[l][t]) for t in range(nt)] for l in range(layers)]
    rows_in = [[int(m.lay_src[0][t]) for t in range(nt)]] + rows[:-1]
    dst = [sum(1 for r in rows[l] if r) for l in range(layers)]
    prefix = [(l + 1, t) for l in range(layers) for t in range(nt) if 0 < rows[l][t] < rows_in[l][t]]
    return dst, prefix


def one_pass(model, batch, y_all, w_all):
    from kgwas_amd import ops
    model.zero_grad(set_to_none=True)
    loss, pred = model.forward_loss(batch.x_dict, batch.edge_index_dict, BS, batch.n_id('SNP'), y_all, w_all, unit_grad=True)
    loss.backward(gradient=ops.unit_gradient(loss.device))
    return loss, pred


def record(kg, name):
    """One configuration: ({'own': [...], 'other': n}, layout, (loss, pred, model) of the profiled pass).  A first pass runs
    unprofiled: whatever a process launches once (library set-up) stays out."""
    from tests.helpers import kernel_launches
    cfg = CONFIGS[name]
    model = make_model(kg, cfg)
    batch = make_batch(kg, model.num_layers)
    y_all, w_all = labels(kg)
    one_pass(model, batch, y_all, w_all)
    res = []
    names = kernel_launches(lambda: res.append(one_pass(model, batch, y_all, w_all)))
    own = [k for k in map(own_kernel, names) if k is not None]
    loss, pred = res[0]
    return {'own': own, 'other': len(names) - len(own)}, layout(batch, model.num_layers, len(model.node_types)), (loss, pred, model)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def pass_digests(loss, pred, model):
    from tests.helpers import grads_by_name
    d = OrderedDict([('loss', digest(loss)), ('pred', digest(pred))])
    for n, g in sorted(grads_by_name(model).items()):
        d['grad ' + n] = digest(g) if g is not None else None
    return d


def captured_digests(kg, kw):
    """Two captured GraphTrainStep steps: the losses and every parameter afterwards."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from tests.helpers import params_by_name
    ids = np.asarray(kg.train_input_nodes[1][:BS * 2])
    run = KGWAS(kg, device='cuda:0', seed=7)
    run.initialize_model(**kw)
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)
    run.model.train()
    gs = GraphTrainStep(run, ('SNP', ids), BS, lr=1e-3, weight_decay=5e-4, sample_seed=7)
    losses = [gs.step(i).detach().clone() for i in range(2)]
    gs.check()
    d = OrderedDict((f'loss {i}', digest(l)) for i, l in enumerate(losses))
    for n, p in sorted(params_by_name(run.model).items()):
        d['param ' + n] = digest(p)
    return d


def main(argv):
    bits = argv[argv.index('--bits') + 1] if '--bits' in argv else None
    out = argv[argv.index('--out') + 1] if '--out' in argv else FIXTURE
    kg = tiny_kg()
    launches, digests = OrderedDict(), OrderedDict()
    for name in CONFIGS:
        launches[name], (dst, prefix), last = record(kg, name)
        print(f'{name}: {len(launches[name]["own"])} own launches, {launches[name]["other"]} others; destination types per layer '
              f'{dst}, proper-prefix (layer, type) pairs {prefix}', flush=True)
        assert max(dst) >= 2 and prefix, (name, dst, prefix)
        if bits:
            digests['pass ' + name] = pass_digests(*last)
    if bits:
        for name, kw in CAPTURED.items():
            digests['captured ' + name] = captured_digests(kg, kw)
            print(f'captured {name}: loss digests', [digests['captured ' + name][f'loss {i}'][:12] for i in range(2)], flush=True)
        with open(bits, 'w') as f:
            json.dump(digests, f, indent=1)
        print('wrote', bits)
    with open(out, 'w') as f:
        json.dump(launches, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main(sys.argv[1:])
