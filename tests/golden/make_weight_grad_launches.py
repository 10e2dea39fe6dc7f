#!/usr/bin/env python
"""Record tests/golden/weight_grad_launches.json: the kernels launched by every route that issues a weight / bias-gradient product
(dW = dY^T X, db = colsum(dY)) -- the ORDERED names of the package's own kernels and the NUMBER of all other launches, as
tests/golden/make_layer_site_launches.py records them for the layer routes.  tests/test_gpu_weight_grad_launches.py replays the
same cases and compares.

STEPS: one training step of the tiny synthetic graph (32 seeds) issued eagerly through the body GraphTrainStep captures
(tests/helpers.launches_of_one_step) -- the default model, the root-weight model, and the default model with each switch of the
GradSink machinery off.  OPS: the autograd nodes and products the tiny graph does not reach, at the smallest shapes that take
each route, forward + backward + optimiser step, once the eager way (every product finishes its own sums, FusedAdam.step) and
once inside a ``grad_sink_scope`` (FusedAdam.step_fused finishes them).

The fixture pins WHICH launches Python issues, in what order: it is recorded on the commit BEFORE a change that must not alter them
(a refactor of kgwas_amd/ops.py), and the changed tree has to reproduce it.  Only public entry points, the module switches the
tests patch and tests/helpers are used, so the file runs on either tree.  Needs a GPU.

    python tests/golden/make_weight_grad_launches.py [--out FILE]    # writes the fixture (or FILE in its place)
    python tests/golden/make_weight_grad_launches.py --bits FILE     # also: FILE gets SHA-256 digests of every output, gradient and
        # updated parameter of the OPS cases, and of the losses and all parameters after two captured steps of the STEPS cases: to
        # compare two trees on ONE machine (no digest is committed: bit equality across machines has not been measured)
"""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.make_layer_site_launches import BS, digest, own_kernel, tiny_kg      # noqa: E402

FIXTURE = os.path.join(HERE, 'weight_grad_launches.json')
DEV = 'cuda:0'
SWITCHES = ('_FUSED_ADAM', '_DEFER_PRODUCTS', '_PARAM_TAIL', '_DEFER_REDUCE', '_DEFER_READOUT_FOLD', '_PACK_FUSED')
# name -> (initialize_model keywords, ops switch set to False or None)
STEPS = OrderedDict([('default', ({}, None)), ('root', (dict(gnn_root_weight=True), None))] +
                    [(f'default {s}=False', ({}, s)) for s in SWITCHES])


def _split(names):
    own = [k for k in map(own_kernel, names) if k is not None]
    return {'own': own, 'other': len(names) - len(own)}


# ---- one training step --------------------------------------------------------------------------------------------------------
def trainer(kg, kw):
    """As tests/test_gpu_root_weight.py::_trainer, at 32 seeds and two batches."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    ids = np.asarray(kg.train_input_nodes[1][:BS * 2])
    run = KGWAS(kg, device=DEV, seed=7)
    run.initialize_model(**kw)
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)
    run.model.train()
    return run, GraphTrainStep(run, ('SNP', ids), BS, lr=1e-3, weight_decay=5e-4, sample_seed=7)


def record_step(kg, name, patch):
    """``patch(module, attribute, value)``: pytest's monkeypatch.setattr, or ``patched`` below.  The second eager step is the one
    recorded: whatever a process launches once (library set-up) stays out."""
    from kgwas_amd import ops
    from tests.helpers import launches_of_one_step
    kw, switch = STEPS[name]
    if switch is not None:
        patch(ops, switch, False)
    run, gs = trainer(kg, kw)
    launches_of_one_step(gs)
    return _split(launches_of_one_step(gs))


def step_digests(kg, name, patch):
    """Two captured steps: the losses and every parameter afterwards."""
    from kgwas_amd import ops
    from tests.helpers import params_by_name
    kw, switch = STEPS[name]
    if switch is not None:
        patch(ops, switch, False)
    run, gs = trainer(kg, kw)
    losses = [gs.step(i).detach().clone() for i in range(2)]
    gs.check()
    d = OrderedDict((f'loss {i}', digest(l)) for i, l in enumerate(losses))
    for n, p in sorted(params_by_name(run.model).items()):
        d['param ' + n] = digest(p)
    return d


class patched:
    """``monkeypatch.setattr`` for the command line: ``with patched() as patch: patch(ops, '_PARAM_TAIL', False)``."""

    def __enter__(self):
        self.undo = []
        return self.set

    def set(self, mod, attr, value):
        self.undo.append((mod, attr, getattr(mod, attr)))
        setattr(mod, attr, value)

    def __exit__(self, *exc):
        for mod, attr, value in reversed(self.undo):
            setattr(mod, attr, value)
        return False


# ---- op-level cases -----------------------------------------------------------------------------------------------------------
def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _mlp_params(g, k1):
    return [_rand(g, 128, k1, scale=0.3), _rand(g, 128, scale=0.1), _rand(g, 128, 128, scale=0.1), _rand(g, 128, scale=0.1)]


def _masked(g, rows):
    """An incoming gradient that is already multiplied by (h2 > 0) somewhere: the contract of the _MLP2 family."""
    return (torch.randn(rows, 128, generator=g) * (torch.rand(rows, 128, generator=g) > 0.5)).to(DEV)


def _mlp2(rows):
    def build(g):
        from kgwas_amd import ops
        x, params, dh2 = torch.rand(rows, 20, generator=g).to(DEV), _mlp_params(g, 20), _masked(g, rows)
        return params, lambda ps: ops.mlp2(x, *ps), dh2
    return build


def _mlp2_gathered(g):
    from kgwas_amd import ops
    feats = [_rand(g, 200, 128), _rand(g, 150, 128)]
    ids = [torch.randperm(200, generator=g)[:64].to(torch.int32).to(DEV), torch.randperm(150, generator=g)[:33].to(torch.int32).to(DEV)]
    params, dh2 = _mlp_params(g, 128), _masked(g, 97)
    assert ops.mlp2_gathered_ok(list(zip(feats, ids)), params[0], params[2])
    return params, lambda ps: ops.mlp2_gathered(list(zip(feats, ids)), *ps), dh2


RESIDENT = {}


def _resident(g):
    """The resident matrix [4096, 1024] and 96 of its rows: the smallest sizes resident_mlp2_ok and gemm3_ok accept.  ONE tensor for
    all cases (its operand images are built once per matrix)."""
    if not RESIDENT:
        X = _rand(torch.Generator().manual_seed(11), 4096, 1024)
        ids = torch.randperm(4096, generator=torch.Generator().manual_seed(12))[:96].to(torch.int32).to(DEV)
        g2l = torch.full((4096,), -1, dtype=torch.int32, device=DEV)
        g2l[ids.long()] = torch.arange(96, dtype=torch.int32, device=DEV)
        RESIDENT.update(X=X, ids=ids, g2l=g2l)
    return RESIDENT['X'], RESIDENT['ids'], RESIDENT['g2l']


def _resident_mlp2(g):
    from kgwas_amd import ops
    X, ids, g2l = _resident(g)
    params, dh2 = _mlp_params(g, 1024), _masked(g, 96)
    with torch.no_grad():
        params[0].mul_(0.1)
    assert ops.resident_mlp2_ok(X, params[0], params[2], 96) and ops.gemm3_ok(*X.shape) and ops._resident_ok(X, params[0])
    return params, lambda ps: ops.resident_mlp2(X, *ps, ids, g2l), dh2


def _resident_rows(g):
    from kgwas_amd import ops
    X, ids, g2l = _resident(g)
    params, dh = [_rand(g, 128, 1024, scale=0.03), _rand(g, 128, scale=0.1)], _rand(g, 96, 128)
    return params, lambda ps: ops.resident_linear_relu_rows(X, *ps, ids, g2l), dh


def _weight_grads(n_pairs):
    def build(g):
        pairs = [(_rand(g, 1024, 128), _rand(g, 1024, 128)) for _ in range(n_pairs)]
        params = [_rand(g, *s) for _ in range(n_pairs) for s in ((128, 128), (128,))]
        return params, pairs, None
    return build


# name -> (builder, ops switch set to False or None)
OPS = OrderedDict([
    ('mlp2 16384x20', (_mlp2(16384), None)),                 # kgw_mlp2_fwd / kgw_mlp2_bwd_first: the fused route's threshold
    ('mlp2 16383x20', (_mlp2(16383), None)),                 # one row under it: the general two-layer path
    ('mlp2_gathered 64+33', (_mlp2_gathered, None)),
    ('resident_mlp2', (_resident_mlp2, None)),               # kgw_mlp2_bwd_first_packed
    ('resident_mlp2 _PACK_FUSED=False', (_resident_mlp2, '_PACK_FUSED')),
    ('resident_linear_relu_rows', (_resident_rows, None)),
    ('weight_grads 2x1024x128', (_weight_grads(2), None)),   # the grouped route
    ('weight_grads 5x1024x128', (_weight_grads(5), None)),   # more products than one grouped launch takes
])


def _op_pass(build, with_sink, seed):
    """Forward, backward and the optimiser's step of one case on fresh tensors: (output or None, gradients, updated parameters)."""
    from kgwas_amd import ops
    from kgwas_amd.optim import FusedAdam
    params, fn, dout = build(torch.Generator().manual_seed(seed))
    params = [p.requires_grad_() for p in params]
    opt = FusedAdam(params, lr=1e-2, weight_decay=5e-4)
    sink = ops.GradSink() if with_sink else None
    out = None
    if callable(fn):
        out = fn(params)
        with ops.grad_sink_scope(sink):
            out.backward(dout)
    else:                                   # (ops.weight_grads called directly: its results ARE the parameters' gradients)
        with ops.grad_sink_scope(sink):
            got = ops.weight_grads(fn)
        for k, (dW, db) in enumerate(got):
            params[2 * k].grad, params[2 * k + 1].grad = dW, db
    if with_sink:
        opt.step_fused(sink)
        assert not sink.records
    else:
        opt.step()
    torch.cuda.synchronize()
    return out, [p.grad for p in params], params


def record_op(name, with_sink, patch, bits=False):
    """({'own': [...], 'other': n}, digests or None) of the second pass of one case (the first runs unprofiled)."""
    from kgwas_amd import ops
    from tests.helpers import kernel_launches
    build, switch = OPS[name]
    if switch is not None:
        patch(ops, switch, False)
    _op_pass(build, with_sink, 1)
    res = []
    names = kernel_launches(lambda: res.append(_op_pass(build, with_sink, 2)))
    d = None
    if bits:
        out, grads, params = res[0]
        d = OrderedDict([('out', digest(out) if out is not None else None)] + [(f'grad {k}', digest(t)) for k, t in enumerate(grads)] +
                        [(f'param {k}', digest(t)) for k, t in enumerate(params)])
    return _split(names), d


def op_key(name, with_sink):
    return name + (' | sink' if with_sink else ' | eager')


def main(argv):
    bits = argv[argv.index('--bits') + 1] if '--bits' in argv else None
    out = argv[argv.index('--out') + 1] if '--out' in argv else FIXTURE
    kg = tiny_kg()
    launches, digests = OrderedDict(steps=OrderedDict(), ops=OrderedDict()), OrderedDict()
    for name in STEPS:
        with patched() as patch:
            r = launches['steps'][name] = record_step(kg, name, patch)
            if bits:
                digests['step ' + name] = step_digests(kg, name, patch)
        print(f'step {name}: {len(r["own"])} own launches, {r["other"]} others', flush=True)
    for name in OPS:
        for with_sink in (False, True):
            with patched() as patch:
                r, d = record_op(name, with_sink, patch, bits=bool(bits))
            launches['ops'][op_key(name, with_sink)] = r
            if bits:
                digests['op ' + op_key(name, with_sink)] = d
            print(f'op {op_key(name, with_sink)}: {r["own"]} + {r["other"]} others', flush=True)
    if bits:
        with open(bits, 'w') as f:
            json.dump(digests, f, indent=1)
        print('wrote', bits)
    with open(out, 'w') as f:
        json.dump(launches, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main(sys.argv[1:])
