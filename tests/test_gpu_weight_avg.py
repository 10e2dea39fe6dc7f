"""-m gpu: weight averaging (kgw_weight_avg_update, optim.WeightAverage) up to GraphTrainStep and KGWAS.train(weight_average=).

The kernel against the float64 restatement of tests/weight_avg_ref.py at the project's fp32 kernel tolerance
(1e-5 + 1e-4 |b| + 1e-5 max|b|, tests/helpers.assert_close), and to the bit where the arithmetic is exact: alpha 1/2 and 1/4 on small
integers, the copy at alpha == 1, the untouched shadow on a non-event.  The trainer: the captured step against eager launches of
the same kernels to the bit, and against the float64 replay of the eager run's own parameter snapshots."""
import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest
import torch

from tests import weight_avg_ref as R
from tests.helpers import assert_close, launches_of_one_step

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
UNIT = 1024
SIZES = [1, 3, 4, 5, 7, UNIT - 1, UNIT, UNIT + 1, 3 * UNIT + 5]
OK, E_NULL, E_RANGE = 0, -1, -2
LR, WD = 1e-3, 5e-4
RTOL, ATOL = 1e-4, 1e-5                                   # (+ assert_close's 1e-5 max|b|)


def _cfg(kind, start_step=1, every=1, warmup=True, decay=0.999):
    from kgwas_amd import _lib
    return _lib.KgwWeightAvg(R.KINDS[kind], start_step, every, int(warmup), decay)


def _rand(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _tensors(sizes, seed, offset_at=None):
    """Device tensors of ``sizes``; tensor ``offset_at`` starts one float past a 16-byte boundary (the element-wise path)."""
    out, keep = [], []
    for k, n in enumerate(sizes):
        if k == offset_at:
            base = torch.zeros(n + 1, device=DEV)
            keep.append(base)
            t = base[1:]
            t.copy_(_rand(n, seed + k))
        else:
            t = _rand(n, seed + k).to(DEV)
        out.append(t)
    return out, keep


def _update(shadow, params, step, cfg, n_tensors=None, numel=None):
    """kgw_weight_avg_update over every 64 tensors; returns the status codes."""
    from kgwas_amd import _lib
    L = _lib.lib()
    rcs = []
    for i in range(0, len(shadow), 64):
        s, p = shadow[i:i + 64], params[i:i + 64]
        S = (C.c_void_p * len(s))(*[t.data_ptr() if t is not None else None for t in s])
        P = (C.c_void_p * len(p))(*[t.data_ptr() if t is not None else None for t in p])
        N = (C.c_int64 * len(s))(*(numel[i:i + 64] if numel is not None else [(a if a is not None else b).numel() for a, b in zip(s, p)]))
        rcs.append(L.kgw_weight_avg_update(len(s) if n_tensors is None else n_tensors, S, P, N, step.data_ptr() if step is not None else None,
                                           C.byref(cfg) if cfg is not None else None, _lib.stream_ptr()))
    return rcs


def _step_tensor(n=0):
    return torch.full((1,), n, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------------------------------------
# (a) the kernel against float64
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('count', [1, 64, 65])
@pytest.mark.parametrize('kind,kw', [('ema', dict(start_step=3, every=2, warmup=True, decay=0.9)),
                                     ('ema', dict(start_step=1, every=1, warmup=False, decay=0.999)),
                                     ('swa', dict(start_step=2, every=3))], ids=['ema_warm', 'ema', 'swa'])
def test_update_equals_float64(kind, kw, count):
    """Twelve consecutive counter values; tensors of 1, 3, 4, 5, 7 elements, one work unit - 1 / exactly / + 1 and three units + 5;
    1, 64 and 65 tensors (two launches); one tensor off the 16-byte boundary.  The parameters move between the updates."""
    sizes = SIZES[-1:] if count == 1 else [SIZES[k % len(SIZES)] for k in range(count)]
    params, keep_p = _tensors(sizes, 100, offset_at=7 if count > 1 else None)
    shadow, keep_s = _tensors(sizes, 900, offset_at=5 if count > 1 else None)
    drift = [_rand(n, 500 + k, 0.1).to(DEV) for k, n in enumerate(sizes)]
    ref = [s.cpu().double().numpy() for s in shadow]
    step = _step_tensor()
    cfg = _cfg(kind, **kw)
    events = 0
    for n in range(1, 13):
        for p, d in zip(params, drift):
            p.add_(d)
        step.fill_(n)
        assert _update(shadow, params, step, cfg) == [OK] * ((count + 63) // 64)
        ref = R.update(ref, [p.cpu().numpy() for p in params], kind, n, **kw)
        events += R.alpha_at(kind, n, **kw)[0]
        for k, (s, r) in enumerate(zip(shadow, ref)):
            assert_close(s, torch.from_numpy(r), RTOL, ATOL, f'{kind} n = {n} tensor {k} ({sizes[k]} elements)')
    assert events >= 4 and int(step) == 12                       # (the kernel never ticks the counter)
    for base in keep_p + keep_s:
        assert float(base[0]) == 0.0                             # (nothing written ahead of an offset tensor)


# ------------------------------------------------------------------------------------------------------------------------------
# (b) exact cases
# ------------------------------------------------------------------------------------------------------------------------------
def _ints(n, seed, unit=16.0):
    return (torch.randint(-64, 65, (n,), generator=torch.Generator().manual_seed(seed)).float() * unit)


def test_exact_ema_half_and_swa():
    """EMA at decay 1/2 without warm-up, four events on multiples of 16 in [-1024, 1024]: every value is a multiple of 2 after three
    halvings -- no rounding anywhere, float32 equals float64.  SWA at k = 0, 1, 3: alpha 1, 1/2, 1/4."""
    sizes = [5, UNIT + 1, 3 * UNIT + 5]
    shadow = [_rand(n, 7 + k).to(DEV) for k, n in enumerate(sizes)]
    ref = [s.cpu().double().numpy() for s in shadow]
    step = _step_tensor()
    kw = dict(start_step=2, every=1, warmup=False, decay=0.5)
    for n in range(2, 6):
        params = [_ints(m, 10 * n + k).to(DEV) for k, m in enumerate(sizes)]
        step.fill_(n)
        assert _update(shadow, params, step, _cfg('ema', **kw)) == [OK]
        ref = R.update(ref, [p.cpu().numpy() for p in params], 'ema', n, **kw)
        for s, r in zip(shadow, ref):
            assert np.array_equal(s.cpu().numpy().astype(np.float64), r), n
    kw = dict(start_step=3, every=2)
    shadow = [_rand(n, 70 + k).to(DEV) for k, n in enumerate(sizes)]
    ref = [s.cpu().double().numpy() for s in shadow]
    for k_ev in (0, 1, 3):
        n = 3 + 2 * k_ev
        assert R.alpha_at('swa', n, **kw) == (True, np.float32([1.0, 0.5, 0.0, 0.25][k_ev]))
        params = [_ints(m, 100 * n + k).to(DEV) for k, m in enumerate(sizes)]
        step.fill_(n)
        assert _update(shadow, params, step, _cfg('swa', **kw)) == [OK]
        ref = R.update(ref, [p.cpu().numpy() for p in params], 'swa', n, **kw)
        for s, r in zip(shadow, ref):
            assert np.array_equal(s.cpu().numpy().astype(np.float64), r), n


# ------------------------------------------------------------------------------------------------------------------------------
# (c) non-events, (d) alpha == 1
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fill', ['random', 'nan'])
def test_non_event_leaves_every_bit(fill):
    sizes = [1, 7, UNIT + 1, 3 * UNIT + 5]
    params = [_rand(n, 3 + k).to(DEV) for k, n in enumerate(sizes)]
    shadow = [(_rand(n, 30 + k) if fill == 'random' else torch.full((n,), float('nan'))).to(DEV) for k, n in enumerate(sizes)]
    before = [s.clone() for s in shadow]
    step = _step_tensor()
    for kind, kw, ns in (('ema', dict(start_step=5, every=3), (1, 4, 6, 7, 9, 10)), ('swa', dict(start_step=2, every=2), (1, 3, 5, 101))):
        for n in ns:
            assert not R.alpha_at(kind, n, **kw)[0]
            step.fill_(n)
            assert _update(shadow, params, step, _cfg(kind, **kw)) == [OK]
    torch.cuda.synchronize()
    for s, b in zip(shadow, before):
        assert _same_bits(s, b)
        if fill == 'random':
            assert torch.equal(s, b)


@pytest.mark.parametrize('kind', ['ema', 'swa'])
def test_alpha_one_copies_the_bits_over_a_nan_shadow(kind):
    """The first event stores the parameter's bits whatever the shadow held: -0.0, a denormal, an infinity and a NaN among them."""
    sizes = [1, 5, UNIT, UNIT + 1, 3 * UNIT + 5]
    params, keep = _tensors(sizes, 41, offset_at=3)
    special = torch.tensor([-0.0, 1e-45, float('inf'), float('-inf'), float('nan')], device=DEV)
    params[1].copy_(special)
    params[4][UNIT - 2:UNIT + 3].copy_(special)
    shadow = [torch.full((n,), float('nan'), device=DEV) for n in sizes]
    kw = dict(start_step=4, every=2)
    assert R.alpha_at(kind, 4, **kw) == (True, np.float32(1.0))
    assert _update(shadow, params, _step_tensor(4), _cfg(kind, **kw)) == [OK]
    torch.cuda.synchronize()
    for s, p in zip(shadow, params):
        assert _same_bits(s, p)
    assert not any(bool(torch.isnan(s).any()) for k, s in enumerate(shadow) if k in (0, 2, 3))


# ------------------------------------------------------------------------------------------------------------------------------
# (e) refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_shadow_untouched():
    from kgwas_amd import _lib
    sizes = [5, UNIT + 1]
    params = [_rand(n, 3 + k).to(DEV) for k, n in enumerate(sizes)]
    shadow = [_rand(n, 30 + k).to(DEV) for k, n in enumerate(sizes)]
    before = [s.clone() for s in shadow]
    step, ok = _step_tensor(1), _cfg('ema')                       # (n = 1 would be an event: alpha == 1, a copy)
    assert _update([shadow[0], None], params, step, ok) == [E_NULL]
    assert _update(shadow, [None, params[1]], step, ok) == [E_NULL]
    assert _update(shadow, params, None, ok) == [E_NULL]
    assert _update(shadow, params, step, None) == [E_NULL]
    L = _lib.lib()
    N = (C.c_int64 * 2)(*sizes)
    S = (C.c_void_p * 2)(*[t.data_ptr() for t in shadow])
    P = (C.c_void_p * 2)(*[t.data_ptr() for t in params])
    for args in ((None, P, N), (S, None, N), (S, P, None)):
        assert L.kgw_weight_avg_update(2, *args, step.data_ptr(), C.byref(ok), _lib.stream_ptr()) == E_NULL
    assert _update(shadow, params, step, ok, n_tensors=65) == [E_RANGE]
    assert _update(shadow, params, step, ok, n_tensors=-1) == [E_RANGE]
    assert _update(shadow, params, step, ok, numel=[5, -1]) == [E_RANGE]
    A = _lib.KgwWeightAvg
    for bad in (A(2, 1, 1, 1, 0.9), A(0, 0, 1, 1, 0.9), A(1, 1, 0, 0, 0.0), A(0, 1, 1, 2, 0.9), A(0, 1, 1, 1, 1.0), A(0, 1, 1, 1, 0.0),
                A(0, 1, 1, 1, float('nan'))):
        assert _update(shadow, params, step, bad) == [E_RANGE]
    torch.cuda.synchronize()
    assert all(torch.equal(s, b) for s, b in zip(shadow, before)) and int(step) == 1
    assert _update(shadow, params, step, ok) == [OK]              # (and the call they all refused does run)
    torch.cuda.synchronize()
    assert all(torch.equal(s, p) for s, p in zip(shadow, params))


# ------------------------------------------------------------------------------------------------------------------------------
# (f) trainer: captured against eager
# ------------------------------------------------------------------------------------------------------------------------------
def _run(kg, seed, state=None, **model_kw):
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(kg, device=DEV, seed=seed)
    run.initialize_model(**model_kw)
    if state is not None:
        run.model.load_state_dict(state)
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)
    run.model.train()
    return run


def _params(model):
    return [p.detach().clone() for p in model.parameters()]


SPECS = {'ema': {'kind': 'ema', 'decay': 0.9, 'start_step': 2}, 'swa': {'kind': 'swa', 'start_step': 2, 'every': 2}}


@pytest.mark.parametrize('kind', ['ema', 'swa'])
def test_trainer_captured_equals_eager(tiny_kg, kind):
    """tiny_kg, six steps.  Two captured trainers replay their graphs; a third issues the body it captured launch by launch on the
    same batches (eager launches of the same kernels on the same static layout: KGWAS.train's own eager loop samples batches of
    their exact sizes, and its weight-gradient sums are then grouped differently -- tests/test_gpu_attn_dropout.py -- so no two
    loops over different layouts share bits, with or without averaging; that loop is compared below at the bar of
    tests/test_gpu_graph.py).  Shadow and parameters: equal bits among the three.  The shadow of the eager run against the float64
    replay of the parameter snapshots it took after every step.  'swa' has non-events between its events (a replayed early exit),
    'ema' one ahead of its first."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.optim import FusedAdam, WeightAverage, parse_weight_average
    from kgwas_amd.sampler import NeighborLoader
    bs, nsteps, seed, spec = 32, 6, 11, SPECS[kind]
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * nsteps])
    run_0 = _run(tiny_kg, seed)
    state = run_0.model.state_dict()
    runs = [_run(tiny_kg, seed, state) for _ in range(3)]
    p0 = _params(runs[0].model)
    gss = [GraphTrainStep(r, ('SNP', ids), bs, lr=LR, weight_decay=WD, sample_seed=seed, weight_average=spec) for r in runs]
    for r, gs in zip(runs, gss):
        assert gs.n_batches == nsteps and gs.fused_adam and gs.avg_model is not None and not gs.avg_model.training
        for p, s, q in zip(r.model.parameters(), gs.avg_model.parameters(), p0):      # (the capture's warm-up steps were undone)
            assert torch.equal(p, q) and torch.equal(s, q) and s.data_ptr() != p.data_ptr()
    ga, gb, ge = gss
    kw = dict(R.DEFAULTS, **{k: v for k, v in spec.items() if k != 'kind'})
    cfg = parse_weight_average(spec, nsteps)
    assert (cfg.kind, cfg.start_step, cfg.every, cfg.warmup) == (R.KINDS[kind], kw['start_step'], kw['every'], 1)
    ref = [q.cpu().double().numpy() for q in p0]
    for i in range(nsteps):
        ga.step(i)
        gb.step(i)
        ge._sample_now(i % 2, i)
        ge._step_body(i % 2)                                       # (not replayed: every launch issued now)
        torch.cuda.synchronize()
        assert int(ga.opt.step_dev) == int(ge.opt.step_dev) == i + 1
        ref = R.update(ref, [p.detach().cpu().numpy() for p in runs[2].model.parameters()], kind, i + 1, **kw)
        for k, (sa, sb, se) in enumerate(zip(ga.avg_model.parameters(), gb.avg_model.parameters(), ge.avg_model.parameters())):
            assert torch.equal(sa, se) and torch.equal(sa, sb), f'shadow tensor {k} after step {i}'
            assert_close(se, torch.from_numpy(ref[k]), RTOL, ATOL, f'shadow tensor {k} after step {i} against float64')
        for k, (pa, pb, pe) in enumerate(zip(runs[0].model.parameters(), runs[1].model.parameters(), runs[2].model.parameters())):
            assert torch.equal(pa, pe) and torch.equal(pa, pb), f'parameter tensor {k} after step {i}'
        if i == 0:                                                 # (start_step = 2: nothing has been averaged yet)
            assert all(torch.equal(s, q) for s, q in zip(ga.avg_model.parameters(), p0))
    for gs in gss:
        gs.check()
    moved = [not torch.equal(s, p) for s, p in zip(ga.avg_model.parameters(), runs[0].model.parameters())]
    assert any(moved) and any(not torch.equal(s, q) for s, q in zip(ga.avg_model.parameters(), p0))   # an average, neither end

    # KGWAS.train's eager loop (exact-size batches, FusedAdam + WeightAverage.update): its shadow against the float64 replay of its
    # own snapshots, and against the captured trainer's at test_graph_step_equals_eager's bar (relative difference of the updates)
    run_k = _run(tiny_kg, seed, state)
    opt = FusedAdam(run_k.model.parameters(), lr=LR, weight_decay=WD)
    wavg = WeightAverage(run_k.model, opt, cfg)
    ld_w = run_k._ld_weight_vector()
    ref = [q.cpu().double().numpy() for q in p0]
    for step, batch in enumerate(NeighborLoader(tiny_kg.data, [-1, -1], ('SNP', ids), batch_size=bs, drop_last=True, device=DEV)):
        run_k.train_step(batch, opt, ld_w)
        wavg.update()
        torch.cuda.synchronize()
        ref = R.update(ref, [p.detach().cpu().numpy() for p in run_k.model.parameters()], kind, step + 1, **kw)
    assert step == nsteps - 1 and int(opt.step_dev) == nsteps
    for k, (s, r) in enumerate(zip(wavg.avg_model.parameters(), ref)):
        assert_close(s, torch.from_numpy(r), RTOL, ATOL, f'eager loop: shadow tensor {k} against float64')
    for what, xs, ys in (('parameters', run_k.model.parameters(), runs[0].model.parameters()),
                         ('shadow', wavg.avg_model.parameters(), ga.avg_model.parameters())):
        xs, ys = [x.detach().double() for x in xs], [y.detach().double() for y in ys]
        num = sum(float((x - y).pow(2).sum()) for x, y in zip(xs, ys))
        den = sum(float((x - q.double()).pow(2).sum()) for x, q in zip(xs, p0))
        print(f'{kind}: eager loop against captured, {what}: relative update difference {(num / max(den, 1e-300)) ** 0.5:.3e}; '
              f'equal bits: {all(torch.equal(x, y) for x, y in zip(xs, ys))}')
        assert den > 0 and (num / den) ** 0.5 < 5e-3, what


# ------------------------------------------------------------------------------------------------------------------------------
# (g) routes
# ------------------------------------------------------------------------------------------------------------------------------
def _trainer(kg, seed=7, **kw):
    from kgwas_amd.graph_step import GraphTrainStep
    bs = 32
    ids = np.asarray(kg.train_input_nodes[1][:bs * 4])
    run = _run(kg, seed)
    return run, GraphTrainStep(run, ('SNP', ids), bs, lr=LR, weight_decay=WD, sample_seed=seed, **kw)


def test_routes(tiny_kg, monkeypatch):
    """None: the entry is never called (a counting wrapper) and the step's launches hold no averaging kernel.  Set: the default
    step's launches plus exactly one, the last; the fused optimiser launch still taken, as many deferred gradients.  On the unfused
    route the launch follows the statistics launch that advances the counter."""
    from kgwas_amd import _lib, ops
    from kgwas_amd.optim import FusedAdam
    L = _lib.lib()
    calls = []
    real = L.kgw_weight_avg_update

    def wrapper(*a):
        calls.append(len(calls))
        return real(*a)
    monkeypatch.setattr(L, 'kgw_weight_avg_update', wrapper)
    run_0, gs_0 = _trainer(tiny_kg)
    for i in range(2):
        gs_0.step(i)
    gs_0.check()
    ps = [_rand(100, 1).to(DEV).requires_grad_(True)]
    ps[0].grad = _rand(100, 2).to(DEV)
    FusedAdam(ps, lr=LR).step()
    n0 = launches_of_one_step(gs_0)
    assert calls == [] and gs_0.wavg is None and gs_0.avg_model is None and gs_0.weight_average is None
    assert not any('k_weight_avg' in n for n in n0) and sum('k_adam_fused' in n for n in n0) == 1

    run_w, gs_w = _trainer(tiny_kg, weight_average='ema')
    assert calls and gs_w.fused_adam and gs_0.fused_adam and gs_w.duv_pieces == gs_0.duv_pieces
    for i in range(2):
        gs_w.step(i)
    gs_w.check()
    before = len(calls)
    nw = launches_of_one_step(gs_w)
    assert len(calls) == before + 1                                  # (one call per step: the model's tensors fit one table)
    print(f'default {len(n0)} launches, averaged {len(nw)}')
    assert len(nw) == len(n0) + 1 and nw[:-1] == n0 and 'k_weight_avg' in nw[-1]
    assert Counter(nw) - Counter(n0) == Counter([nw[-1]]) and not (Counter(n0) - Counter(nw))
    assert sum('k_adam_fused' in n for n in nw) == 1 and 'k_adam_fused' in nw[-2]
    assert gs_w.deferred_gradients == gs_0.deferred_gradients > 0 and gs_w.riders_taken == gs_0.riders_taken
    # the raw trajectory is the default run's: averaging reads the parameters and writes only the shadow
    assert all(torch.equal(a, b) for a, b in zip(run_0.model.parameters(), run_w.model.parameters()))

    monkeypatch.setattr(ops, '_FUSED_ADAM', False)
    run_u, gs_u = _trainer(tiny_kg)
    run_v, gs_v = _trainer(tiny_kg, weight_average='swa')
    assert not gs_u.fused_adam and not gs_v.fused_adam
    nu, nv = launches_of_one_step(gs_u), launches_of_one_step(gs_v)
    assert len(nv) == len(nu) + 1 and nv[:-1] == nu and 'k_weight_avg' in nv[-1] and 'k_weight_avg' not in nv[-2]
    assert not any('k_adam_fused' in n for n in nv)
    torch.cuda.synchronize()
    assert int(gs_v.opt.step_dev) == 1
    assert all(torch.equal(s, p) for s, p in zip(gs_v.avg_model.parameters(), run_v.model.parameters()))   # (n = 1: the copy)


# ------------------------------------------------------------------------------------------------------------------------------
# (h) nothing cached from the shadow goes stale
# ------------------------------------------------------------------------------------------------------------------------------
def test_evaluation_of_the_shadow_follows_it(tiny_kg):
    """HIP launches do not move a tensor's version counter: whatever the captured evaluation of ``avg_model`` kept from its
    parameters outside the graph would go stale.  After 2 epochs, and after 2 more on the same objects (the same cached evaluation
    graph, replayed), its predictions are those of a fresh HeteroGNN loaded from avg_model.state_dict()."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    from kgwas_amd.utils import evaluate_minibatch_clean
    bs, seed = 32, 5
    run = _run(tiny_kg, seed)
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * 4])
    gs = GraphTrainStep(run, ('SNP', ids), bs, lr=LR, weight_decay=WD, sample_seed=seed, cache_batches=True,
                        weight_average={'kind': 'ema', 'decay': 0.5, 'every': 2})
    val = [NeighborLoader(tiny_kg.data, [-1, -1], tiny_kg.val_input_nodes, batch_size=bs, drop_last=True, device=DEV) for _ in range(2)]
    assert len(val[0]) >= 1
    seen, preds = [], []
    for rnd in range(2):
        for ep in range(2):
            for i in range(gs.n_batches):
                gs.step(i)
        gs.check()
        res = evaluate_minibatch_clean(val[0], gs.avg_model, DEV)
        seen.append(val[0].__dict__['_graph_eval'][id(gs.avg_model)])
        fresh = KGWAS(tiny_kg, device=DEV, seed=seed + 1)
        fresh.initialize_model()
        fresh.model.load_state_dict(gs.avg_model.state_dict())
        for a, b in zip(fresh.model.parameters(), gs.avg_model.parameters()):
            assert torch.equal(a, b)
        ref = evaluate_minibatch_clean(val[1], fresh.model, DEV)
        assert torch.equal(torch.from_numpy(res['pred']), torch.from_numpy(ref['pred'])), f'round {rnd}'
        assert np.array_equal(res['truth'], ref['truth']) and np.isfinite(res['pred']).all()
        preds.append(res['pred'].copy())
    assert seen[0] is seen[1] and seen[0]                          # captured once, replayed (not the eager fallback)
    assert not np.array_equal(preds[0], preds[1])                  # the shadow moved between the two evaluations
    raw = evaluate_minibatch_clean(val[1], run.model, DEV)
    assert not np.array_equal(raw['pred'], preds[1])               # and it is not the raw model


# ------------------------------------------------------------------------------------------------------------------------------
# (i) KGWAS.train
# ------------------------------------------------------------------------------------------------------------------------------
def _record_validations(run, monkeypatch):
    """Every evaluate_minibatch_clean of KGWAS.train on the validation loader: (the model evaluated, a copy of its parameters,
    the result)."""
    from kgwas_amd import kgwas as K
    real, log = K.evaluate_minibatch_clean, []

    def wrapper(loader, model, device):
        res = real(loader, model, device)
        if loader is run.val_loader:
            log.append((model, _params(model), res))
        return res
    monkeypatch.setattr(K, 'evaluate_minibatch_clean', wrapper)
    return log


@pytest.mark.parametrize('use_graph', [True, False], ids=['captured', 'eager'])
def test_train_end_to_end(tiny_kg, use_graph, monkeypatch):
    """train(epoch=3) with the first averaging event in the second epoch: epoch 1 validates the raw model, epochs 2 and 3 the shadow;
    best_model is a copy of what was validated at the epoch that won, model.pt loads to exactly that, val_metrics are the last
    epoch's -- the shadow's -- and nothing enters the configuration."""
    from kgwas_amd.kgwas import KGWAS
    bs = 32
    nb = len(tiny_kg.train_input_nodes[1]) // bs
    run = KGWAS(tiny_kg, device=DEV, seed=3)
    run.initialize_model()
    cfg = dict(run.config)
    log = _record_validations(run, monkeypatch)
    name = f'weight_avg_e2e_{int(use_graph)}'
    run.train(batch_size=bs, epoch=3, save_best_model=True, save_name=name, use_graph=use_graph, lr=LR,
              weight_average={'kind': 'ema', 'decay': 0.9, 'start_step': nb + 2, 'every': 2})
    assert len(run.train_loader) == nb >= 2 and run.config == cfg and len(log) == 3
    assert log[0][0] is run.model and log[1][0] is run.avg_model and log[2][0] is run.avg_model
    assert run.avg_model is not run.model and not run.avg_model.training
    pears = [run._metrics(res)['pearsonr'] for _, _, res in log]
    won = max(range(3), key=lambda e: (pears[e], -e))               # (the first of equal maxima: a strict > moves the best)
    print(f'{nb} batches per epoch; validation Pearson per epoch {pears}; epoch {won + 1} won')
    best = list(run.best_model.parameters())
    assert len(best) == len(log[won][1]) and all(torch.equal(a, b) for a, b in zip(best, log[won][1]))
    assert run.val_metrics['pearsonr'] == pears[2] and run.val_metrics['mse'] == run._metrics(log[2][2])['mse']
    # the shadow is neither the raw model nor where it started; the last validation saw it as it is now
    assert any(not torch.equal(a, b) for a, b in zip(run.avg_model.parameters(), run.model.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(run.avg_model.parameters(), log[2][1]))
    path = os.path.join(tiny_kg.data_path, 'model', name)
    sd = torch.load(os.path.join(path, 'model.pt'), map_location='cpu', weights_only=False)
    want = run.best_model.state_dict()
    assert list(sd) == list(want)
    for k, v in sd.items():
        if not isinstance(v, torch.nn.parameter.UninitializedParameter):
            assert torch.equal(v, want[k].cpu()), k
    fresh = KGWAS(tiny_kg, device=DEV, seed=4)
    fresh.initialize_model()
    fresh.model.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(fresh.model.parameters(), log[won][1]))
    assert np.isfinite(run.test_metrics['mse']) and all(bool(torch.isfinite(p).all()) for p in run.avg_model.parameters())


def test_train_narrow_model_keeps_the_padding_zero_and_shard_refuses(tiny_kg, monkeypatch):
    """gnn_hidden_dim = 64: parameter and shadow are both 0 outside the model's own block and fmaf(alpha, 0 - 0, 0) keeps them
    there; every epoch validates the shadow (start_step = 1).  parallelism='shard' refuses, a bad specification is a ValueError,
    both before anything moves."""
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(tiny_kg, device=DEV, seed=3)
    run.initialize_model(gnn_hidden_dim=64)
    p0 = _params(run.model)
    with pytest.raises(NotImplementedError, match='weight_average'):
        run.train(batch_size=32, epoch=1, parallelism='shard', weight_average='ema')
    for bad in ('emma', 1.0, 0, {'kind': 'swa', 'decay': 0.5}, {'kind': 'ema', 'every': 'batch'}, {'kind': 'ema', 'start_step': 0}):
        with pytest.raises(ValueError, match='weight_average'):
            run.train(batch_size=32, epoch=1, weight_average=bad)
    assert all(torch.equal(a, b) for a, b in zip(run.model.parameters(), p0)) and getattr(run, 'avg_model', None) is None
    log = _record_validations(run, monkeypatch)
    run.train(batch_size=32, epoch=2, save_best_model=False, save_name='weight_avg_narrow', lr=LR,
              weight_average={'kind': 'swa', 'every': 'epoch', 'start_step': 2})
    nb = len(run.train_loader)
    assert [m is run.avg_model for m, _, _ in log] == [True, True] and nb >= 3
    hc, m = 64, run.avg_model
    assert m.hidden == 128 and m.hidden_logical == hc
    for model in (run.avg_model, run.best_model):
        for p in model.parameters():
            p = p.detach()
            if p.dim() == 3 and p.shape[-1] == 128:
                assert float(p[:, hc:, :].abs().sum()) == 0.0 and float(p[:, :, hc:].abs().sum()) == 0.0
        lin, fc = model.lin.weight.detach(), model.snp_feat_mlp.FC_hidden.weight.detach()
        assert float(lin[:, hc:].abs().sum()) == 0.0 and float(fc[hc:].abs().sum()) == 0.0 and float(lin[:, :hc].abs().sum()) > 0.0
    # 'every': 'epoch' from update 2: events at 2 and 2 + nb, so the second epoch's shadow is the mean of two snapshots
    assert any(not torch.equal(a, b) for a, b in zip(log[0][1], log[1][1]))
    assert any(not torch.equal(a, b) for a, b in zip(run.avg_model.parameters(), run.model.parameters()))
