"""-m gpu: learning-rate schedules and gradient-norm clipping (kgw_adam_ctl, kgw_adam_fused_ctl, kgw_grad_norm_partial / _fold,
optim.FusedAdam(lr_schedule=, grad_clip_norm=)) up to GraphTrainStep and KGWAS.train().

The rate and the update against the numpy float64 twin of tests/lr_schedule_ref.py: lr_t to 1 float32 ulp, parameters at the bar of
tests/test_gpu_dense.py::test_fused_adam_matches_torch_adam (rtol 2e-6, atol 1e-7, no rel-to-max).  The calls without controls and the
constant schedule leave the bits of kgw_adam / kgw_adam_notick.  The norm is a float64 sum rounded once: 1 float32 ulp, its
coefficient 2.  The trainer: captured against eager at tests/test_gpu_attn_dropout.py::test_captured_step_equals_eager_loop's bars,
and the optimiser alone against torch.optim.Adam + LambdaLR + clip_grad_norm_ fed the product's own gradients."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import lr_schedule_ref as R
from tests.helpers import assert_close, launches_of_one_step, params_by_name

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
UNIT = 1024
SIZES = [1, 255, 256, 257, 4099]
LR, WD = 1e-3, 5e-4
HYPER = (0.9, 0.999, 1e-8)
OK, E_NULL, E_RANGE, E_UNSUPPORTED = 0, -1, -2, -3
SHAPE = dict(W=3, N=8, r=0.1, step_size=2, gamma=0.5)


def _schedule(kind, W=3, N=8, r=0.1, step_size=2, gamma=0.5):
    from kgwas_amd import _lib
    return _lib.KgwLrSchedule(R.KINDS[kind], W, N, step_size, r, gamma)


def _rand(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class _State:
    """Parameters, gradients, both moments and the counter of a bare kgw_adam* call; ``offset``: tensor 1 starts one float past a
    16-byte boundary (the scalar path)."""

    def __init__(self, sizes, seed, offset=False):
        self.p, self._keep = [], []
        for k, n in enumerate(sizes):
            if offset and k == 1:
                base = torch.zeros(n + 1, device=DEV)
                self._keep.append(base)
                t = base[1:]
                t.copy_(_rand(n, seed + k))
            else:
                t = _rand(n, seed + k).to(DEV)
            self.p.append(t)
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.step = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.n = (C.c_int64 * len(sizes))(*sizes)

    def call(self, name, grads, tick=None, ctl=None, lr=LR):
        from kgwas_amd import _lib
        L = _lib.lib()
        args = [len(self.p), _ptrs(self.p), _ptrs(grads), _ptrs(self.m), _ptrs(self.v), self.n, self.step.data_ptr(), lr, *HYPER, WD]
        if name == 'kgw_adam_ctl':
            args += [int(tick), C.byref(ctl) if ctl is not None else None]
        return getattr(L, name)(*args, _lib.stream_ptr())

    def equal(self, other):
        return (all(torch.equal(a, b) for a, b in zip(self.p + self.m + self.v, other.p + other.m + other.v)) and
                torch.equal(self.step, other.step))


# ------------------------------------------------------------------------------------------------------------------------------
# (a) the scheduled update on bare tensors
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', list(R.KINDS))
def test_scheduled_adam_equals_float64(kind):
    """1, 255, 256, 257 and 4099 elements and one tensor that never gets a gradient; 12 updates with W = 3, N = 8, step_size = 2:
    through the warm-up's end, a decay, the run's end and beyond.  ``last_lr`` to 1 ulp of the twin, the parameters against the
    float64 Adam driven by the twin's rate."""
    from kgwas_amd.optim import FusedAdam
    ps = [_rand(n, 10 + k).to(DEV).requires_grad_(True) for k, n in enumerate(SIZES)]
    dead = _rand(77, 99).to(DEV).requires_grad_(True)
    dead0 = dead.detach().clone()
    opt = FusedAdam(ps[:2] + [dead] + ps[2:], lr=LR, weight_decay=WD, lr_schedule=_schedule(kind))
    ref = R.Adam64([p.detach().cpu().numpy() for p in ps], weight_decay=WD)
    seen = []
    for it in range(12):
        gs = [_rand(n, 1000 + 10 * it + k, 10.0 if it == 2 else 1.0) for k, n in enumerate(SIZES)]
        for p, g in zip(ps, gs):
            p.grad = g.to(DEV)
        opt.step()
        lr_ref = R.lr_at(kind, LR, it + 1, **SHAPE)
        lr_dev = float(opt.last_lr)
        seen.append(lr_dev)
        assert abs(lr_dev - float(lr_ref)) <= R.ulp32(lr_ref), (kind, it, lr_dev, float(lr_ref))
        ref.step([g.numpy() for g in gs], lr_ref)
        for k, p in enumerate(ps):
            assert_close(p, torch.from_numpy(ref.p[k]), 2e-6, 1e-7, f'{kind} update {it + 1} tensor {k}', rel_to_max=0)
    print(f'{kind}: lr_t of updates 1..12 = {[f"{v:.3e}" for v in seen]}')
    assert int(opt.step_dev) == 12 and torch.equal(dead, dead0) and dead not in opt.state
    assert seen[0] < seen[1] < seen[2] == R.f32(LR)                   # the warm-up
    if kind != 'constant':
        assert seen[-1] < seen[3] and (kind == 'step' or seen[-1] == seen[-2])      # decayed, and flat beyond the end ('step' goes on)


# ------------------------------------------------------------------------------------------------------------------------------
# (b) the calls without controls keep their bits
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tick', [True, False], ids=['kgw_adam', 'kgw_adam_notick'])
def test_default_bits(tick):
    """ctl = NULL and the constant schedule without warm-up against kgw_adam / kgw_adam_notick: parameters, both moments and the
    counter, torch.equal, three updates; tensor 1 off the 16-byte boundary."""
    from kgwas_amd import _lib
    const = _lib.KgwOptimCtl(_lib.KgwLrSchedule(_lib.KGW_LR_CONSTANT, 0, 1, 1, 0.0, 1.0), None, None)
    lr_out = torch.zeros(1, device=DEV)
    const_out = _lib.KgwOptimCtl(const.sched, None, lr_out.data_ptr())
    base, null, con, con_out = (_State(SIZES, 5, offset=True) for _ in range(4))
    for it in range(3):
        gs = [_rand(n, 200 + 10 * it + k).to(DEV) for k, n in enumerate(SIZES)]
        gs[1] = torch.cat([torch.zeros(3, device=DEV), gs[1]])[3:]              # (gradient off the boundary too)
        assert base.call('kgw_adam' if tick else 'kgw_adam_notick', gs) == OK
        assert null.call('kgw_adam_ctl', gs, tick=tick, ctl=None) == OK
        assert con.call('kgw_adam_ctl', gs, tick=tick, ctl=const) == OK
        assert con_out.call('kgw_adam_ctl', gs, tick=tick, ctl=const_out) == OK
        torch.cuda.synchronize()
        assert int(base.step) == (it + 1 if tick else it)
        assert base.equal(null) and base.equal(con) and base.equal(con_out), it
        assert float(lr_out) == R.f32(LR)
        if not tick:                                                              # (what the caller's statistics launch does)
            for s in (base, null, con, con_out):
                s.step += 1
    assert float((base.p[4] - _rand(4099, 5 + 4).to(DEV)).abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# (c) the fused launch with a schedule
# ------------------------------------------------------------------------------------------------------------------------------
def _same_state(pa, pb, oa, ob):
    for k, (x, y) in enumerate(zip(pa, pb)):
        assert torch.equal(x.grad, y.grad), k
        assert torch.equal(x, y), (k, float((x - y).abs().max()))
        assert torch.equal(oa.state[x]['exp_avg'], ob.state[y]['exp_avg'])
        assert torch.equal(oa.state[x]['exp_avg_sq'], ob.state[y]['exp_avg_sq'])
    assert int(oa.step_dev) == int(ob.step_dev)


@pytest.mark.parametrize('kind', ['cosine', 'step'])
def test_fused_launch_with_a_schedule_equals_the_unfused_one(kind):
    """Deferred KgwGradSrc records (a TN product and its column sums, as tests/test_gpu_fused_adam.py builds them) finished and
    updated by kgw_adam_fused_ctl == kgw_adam_ctl on the finished gradients, bit for bit, over 5 updates of a W = 2, N = 4 schedule;
    both report the same rate."""
    from kgwas_amd import ops
    from kgwas_amd.optim import FusedAdam
    rows, M, N = 9000, 128, 20
    g = torch.Generator().manual_seed(3)
    A, B = torch.randn(rows, M, generator=g).to(DEV), torch.randn(rows, N, generator=g).to(DEV)
    pa = [torch.randn(M, N, generator=g).to(DEV).requires_grad_(), torch.randn(M, generator=g).to(DEV).requires_grad_(),
          torch.randn(33, 7, generator=g).to(DEV).requires_grad_()]
    pb = [p.detach().clone().requires_grad_() for p in pa]
    sched = _schedule(kind, W=2, N=4)
    oa = FusedAdam(pa, lr=1e-2, weight_decay=WD, lr_schedule=sched)
    ob = FusedAdam(pb, lr=1e-2, weight_decay=WD, lr_schedule=sched)
    for it in range(5):
        ref, ref_cs = ops.tn_gemm(A, B, colsum=True)
        sink = ops.GradSink()
        with ops.grad_sink_scope(sink):
            out, cs = ops.tn_gemm(A, B, colsum=True, defer=True)
        assert len(sink.records) == 2                          # both gradients wait for the optimiser
        extra = torch.randn(33, 7, generator=g).to(DEV)
        pa[0].grad, pa[1].grad, pa[2].grad = out, cs, extra.clone()
        pb[0].grad, pb[1].grad, pb[2].grad = ref, ref_cs, extra.clone()
        oa.step_fused(sink)
        ob.step()
        _same_state(pa, pb, oa, ob)
        lr_ref = R.lr_at(kind, 1e-2, it + 1, W=2, N=4, r=0.1, step_size=2, gamma=0.5)
        assert torch.equal(oa.last_lr, ob.last_lr) and abs(float(oa.last_lr) - float(lr_ref)) <= R.ulp32(lr_ref)
        A = A * 0.5 + 0.1
    assert int(oa.step_dev) == 5 and int(oa.done_dev.abs().sum()) == 0


def _bad_schedules():
    from kgwas_amd import _lib
    S = _lib.KgwLrSchedule
    return [S(4, 0, 8, 1, 0.0, 0.1), S(-1, 0, 8, 1, 0.0, 0.1), S(1, -1, 8, 1, 0.0, 0.1), S(1, 0, 0, 1, 0.0, 0.1), S(3, 0, 8, 0, 0.0, 0.1),
            S(2, 0, 8, 1, -0.1, 0.1), S(2, 0, 8, 1, 1.5, 0.1), S(2, 0, 8, 1, float('nan'), 0.1), S(3, 0, 8, 1, 0.0, 0.0),
            S(3, 0, 8, 1, 0.0, -1.0), S(3, 0, 8, 1, 0.0, float('inf')), S(0, 0, 8, 1, 0.0, float('nan'))]


def test_refusals_leave_everything_untouched():
    """A scale pointer at the fused entry: KGW_E_UNSUPPORTED; every schedule outside the rule's ranges at both entries:
    KGW_E_RANGE; parameters, moments, the counter and lr_out as they were.  FusedAdam.step_fused with clipping raises before
    anything is claimed or launched."""
    from kgwas_amd import _lib, ops
    from kgwas_amd.optim import FusedAdam
    L = _lib.lib()
    st = _State(SIZES, 31)
    gs = [_rand(n, 300 + k).to(DEV) for k, n in enumerate(SIZES)]
    p0 = [t.clone() for t in st.p]
    lr_out = torch.full((1,), -1.0, device=DEV)
    scale = torch.full((1,), 0.5, device=DEV)
    done = torch.zeros(_lib.ADAM_FUSED_COUNTERS, dtype=torch.int32, device=DEV)

    def fused(ctl):
        return L.kgw_adam_fused_ctl(len(st.p), _ptrs(st.p), _ptrs(gs), _ptrs(st.m), _ptrs(st.v), st.n, None, st.step.data_ptr(), LR, *HYPER,
                                    WD, None, 0, 0, None, done.data_ptr(), C.byref(ctl), _lib.stream_ptr())

    good = _schedule('cosine')
    assert fused(_lib.KgwOptimCtl(good, scale.data_ptr(), lr_out.data_ptr())) == E_UNSUPPORTED
    for s in _bad_schedules():
        ctl = _lib.KgwOptimCtl(s, None, lr_out.data_ptr())
        assert fused(ctl) == E_RANGE and st.call('kgw_adam_ctl', gs, tick=1, ctl=ctl) == E_RANGE
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(st.p, p0)) and int(st.step) == 0 and float(lr_out) == -1.0
    assert all(float(t.abs().sum()) == 0.0 for t in st.m + st.v) and int(done.abs().sum()) == 0
    # the accepted calls, for contrast, write
    assert fused(_lib.KgwOptimCtl(good, None, lr_out.data_ptr())) == OK
    torch.cuda.synchronize()
    lr1 = R.lr_at('cosine', LR, 1, **SHAPE)
    assert int(st.step) == 1 and not torch.equal(st.p[4], p0[4]) and abs(float(lr_out) - float(lr1)) <= R.ulp32(lr1)
    # step_fused with clipping
    ps = [_rand(50, 1).to(DEV).requires_grad_(True)]
    ps[0].grad = _rand(50, 2).to(DEV)
    q0 = ps[0].detach().clone()
    opt = FusedAdam(ps, lr=LR, grad_clip_norm=1.0)
    with pytest.raises(ops.GradSinkMismatch, match='grad_clip_norm'):
        opt.step_fused(ops.GradSink())
    torch.cuda.synchronize()
    assert torch.equal(ps[0].detach(), q0) and int(opt.step_dev) == 0 and not opt.state
    with pytest.raises(ValueError):
        FusedAdam(ps, lr=LR, grad_clip_norm=0.0)
    with pytest.raises(ValueError):
        FusedAdam(ps, lr=LR, lr_schedule='cosine')                     # nobody named total_steps


# ------------------------------------------------------------------------------------------------------------------------------
# (d) the norm kernels
# ------------------------------------------------------------------------------------------------------------------------------
def _norm(ts, max_norm, ws=None):
    """kgw_grad_norm_partial + _fold over ``ts`` (device tensors): (norm, scale, the partial sums), on the CPU."""
    from kgwas_amd import _lib
    L = _lib.lib()
    n = (C.c_int64 * len(ts))(*[t.numel() for t in ts])
    units = int(L.kgw_grad_norm_workspace_doubles(len(ts), n))
    assert units == sum((t.numel() + UNIT - 1) // UNIT for t in ts)
    pad = 3
    ws = torch.full((units + 2 * pad,), -7.0, dtype=torch.float64, device=DEV)
    norm, scale = torch.full((1,), -1.0, device=DEV), torch.full((1,), -1.0, device=DEV)
    assert L.kgw_grad_norm_partial(len(ts), _ptrs(ts), n, ws.data_ptr(), pad, _lib.stream_ptr()) == OK
    assert L.kgw_grad_norm_fold(ws[pad:].data_ptr(), units, float(max_norm), norm.data_ptr(), scale.data_ptr(), _lib.stream_ptr()) == OK
    torch.cuda.synchronize()
    assert bool((ws[:pad] == -7.0).all()) and bool((ws[pad + units:] == -7.0).all())      # nothing beside the units' slots
    return norm.cpu(), scale.cpu(), ws[pad:pad + units].cpu()


NORM_SIZES = [UNIT - 1, UNIT, UNIT + 1, 3 * UNIT + 7]


@pytest.mark.parametrize('count', [1, 64])
def test_norm_and_coefficient_equal_float64(count):
    """Tensors of unit - 1, unit, unit + 1 and 3 units + 7 elements (and, among 64, of 1, 5 and no elements; every fourth one off
    the 16-byte boundary): the per-unit sums, the norm to 1 float32 ulp and the coefficient to 2, for a norm below, at and above
    max_norm; zeros give norm 0 and the coefficient exactly 1; two runs give equal bits."""
    sizes = NORM_SIZES if count == 1 else [(NORM_SIZES + [1, 5, 0, 700])[k % 8] for k in range(64)]
    cases = [[n] for n in sizes] if count == 1 else [sizes]
    for sizes in cases:
        ts, keep = [], []
        for k, n in enumerate(sizes):
            if k % 4 == 3:
                base = torch.zeros(n + 1, device=DEV)
                base[1:] = _rand(n, 40 + k, 0.3)
                keep.append(base)
                ts.append(base[1:])
            else:
                ts.append(_rand(n, 40 + k, 0.3).to(DEV))
        ref = R.grad_norm([t.cpu().numpy() for t in ts])
        assert ref > 0
        for max_norm in (2.0 * ref, ref, 0.5 * ref, 1e-3 * ref):
            norm, scale, part = _norm(ts, max_norm)
            norm2, scale2, part2 = _norm(ts, max_norm)
            assert torch.equal(norm, norm2) and torch.equal(scale, scale2) and torch.equal(part, part2)
            want = R.clip_scale(ref, max_norm)
            print(f'{count} tensor(s) {sizes[:4]}: norm {float(norm):.9g} (float64 {ref:.12g}), max_norm {max_norm:.6g}: scale '
                  f'{float(scale):.9g} (float64 {want:.12g})')
            assert abs(float(norm) - ref) <= R.ulp32(ref)
            assert abs(float(scale) - want) <= 2 * R.ulp32(want)
            if max_norm >= 2.0 * ref:
                assert float(scale) == 1.0
            if max_norm < ref:
                assert float(scale) < 1.0                              # (at max_norm: 1 - 1e-6 / norm, which may round to 1)
        # the units' own values: float64 sums of exact squares, any order agrees to a few float64 ulps
        flat, k = [], 0
        for t in ts:
            x = t.cpu().double().numpy()
            flat += [float(np.sum(x[i:i + UNIT] ** 2)) for i in range(0, len(x), UNIT)]
        assert len(flat) == part.numel()
        np.testing.assert_allclose(part.numpy(), np.asarray(flat), rtol=1e-14, atol=0)
        zeros = [torch.zeros_like(t) for t in ts]
        norm, scale, part = _norm(zeros, 1.0)
        assert float(norm) == 0.0 and float(scale) == 1.0 and float(part.abs().sum()) == 0.0


def test_non_finite_norms():
    """A NaN among the gradients: a NaN coefficient; an infinity: the coefficient 0 (what torch's default computes)."""
    t = _rand(UNIT + 5, 3).to(DEV)
    t[7] = float('nan')
    norm, scale, _ = _norm([t], 1.0)
    assert bool(torch.isnan(norm)) and bool(torch.isnan(scale))
    t[7] = float('inf')
    norm, scale, _ = _norm([t], 1.0)
    assert bool(torch.isinf(norm)) and float(scale) == 0.0


def test_clipped_adam_equals_float64():
    """FusedAdam(grad_clip_norm, lr_schedule='linear') on bare tensors, 8 updates whose gradients grow: the coefficient binds on
    some and not on others; against the float64 Adam fed g * scale.  The gradient tensors stay unscaled."""
    from kgwas_amd.optim import FusedAdam
    ps = [_rand(n, 60 + k).to(DEV).requires_grad_(True) for k, n in enumerate(SIZES)]
    max_norm = 40.0
    opt = FusedAdam(ps, lr=LR, weight_decay=WD, lr_schedule=_schedule('linear'), grad_clip_norm=max_norm)
    ref = R.Adam64([p.detach().cpu().numpy() for p in ps], weight_decay=WD)
    scales = []
    for it in range(8):
        gs = [_rand(n, 700 + 10 * it + k, 0.2 * (it + 1)) for k, n in enumerate(SIZES)]
        for p, g in zip(ps, gs):
            p.grad = g.to(DEV)
        opt.step()
        norm = R.grad_norm([g.numpy() for g in gs])
        want = R.clip_scale(norm, max_norm)
        scales.append(float(opt.last_clip_scale))
        assert abs(float(opt.last_grad_norm) - norm) <= R.ulp32(norm) and abs(scales[-1] - want) <= 2 * R.ulp32(want)
        ref.step([g.numpy() for g in gs], R.lr_at('linear', LR, it + 1, **SHAPE), want)
        for k, p in enumerate(ps):
            assert torch.equal(p.grad.cpu(), gs[k])                    # unscaled
            assert_close(p, torch.from_numpy(ref.p[k]), 2e-6, 1e-7, f'clipped update {it + 1} tensor {k}', rel_to_max=0)
    print('clip coefficients:', [f'{s:.4f}' for s in scales])
    assert scales[0] == 1.0 and scales[-1] < 0.9 and int(opt.step_dev) == 8


def test_clipping_over_more_than_64_tensors():
    """70 tensors: two tables, one norm over all of them (the second table's units behind the first's), one coefficient."""
    from kgwas_amd.optim import FusedAdam
    sizes = [(7 * k) % 300 + 1 for k in range(70)]
    ps = [_rand(n, 800 + k).to(DEV).requires_grad_(True) for k, n in enumerate(sizes)]
    gs = [_rand(n, 900 + k) for k, n in enumerate(sizes)]
    for p, g in zip(ps, gs):
        p.grad = g.to(DEV)
    norm = R.grad_norm([g.numpy() for g in gs])
    opt = FusedAdam(ps, lr=LR, weight_decay=WD, grad_clip_norm=0.25 * norm)
    ref = R.Adam64([p.detach().cpu().numpy() for p in ps], weight_decay=WD)
    opt.step()
    want = R.clip_scale(norm, 0.25 * norm)
    assert abs(float(opt.last_grad_norm) - norm) <= R.ulp32(norm) and abs(float(opt.last_clip_scale) - want) <= 2 * R.ulp32(want)
    assert float(opt.last_lr) == R.f32(LR) and int(opt.step_dev) == 1
    ref.step([g.numpy() for g in gs], R.f32(LR), want)
    for k, p in enumerate(ps):
        assert_close(p, torch.from_numpy(ref.p[k]), 2e-6, 1e-7, f'tensor {k}', rel_to_max=0)


# ------------------------------------------------------------------------------------------------------------------------------
# (e) the trainer
# ------------------------------------------------------------------------------------------------------------------------------
COSINE = {'kind': 'cosine', 'warmup_steps': 2, 'min_lr': 1e-4}


def _run(kg, seed, state=None):
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(kg, device=DEV, seed=seed)
    run.initialize_model()
    if state is not None:
        run.model.load_state_dict(state)
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)
    run.model.train()
    return run


def test_trainer_captured_equals_eager_and_torch(small_kg):
    """small_kg, six steps, cosine with W = 2 and a grad_clip_norm between the norms a dry pass saw: the coefficient binds on some
    steps and not on others.  Captured against eager at test_captured_step_equals_eager_loop's bars; the rate against the twin;
    and torch.optim.Adam + LambdaLR(twin) + clip_grad_norm_, fed the eager product's gradients step by step, against its
    parameters at the bare-tensor bar."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.optim import FusedAdam
    from kgwas_amd.sampler import NeighborLoader
    bs, nsteps, seed = 64, 6, 11
    ids = np.asarray(small_kg.train_input_nodes[1][:bs * nsteps])
    run_e = _run(small_kg, seed)
    run_d, run_g = _run(small_kg, seed, run_e.model.state_dict()), _run(small_kg, seed, run_e.model.state_dict())
    dry = GraphTrainStep(run_d, ('SNP', ids), bs, lr=LR, weight_decay=WD, sample_seed=seed, lr_schedule=COSINE, grad_clip_norm=1e30)
    norms = []
    for i in range(nsteps):
        dry.step(i)
        norms.append(float(dry.opt.last_grad_norm))
        assert float(dry.opt.last_clip_scale) == 1.0
    dry.check()
    srt = sorted(norms)
    clip = float(np.sqrt(srt[nsteps // 2 - 1] * srt[nsteps // 2]))
    print('gradient norms of the dry pass:', [f'{v:.4f}' for v in norms], 'grad_clip_norm', clip)
    assert srt[0] > 0 and srt[nsteps // 2 - 1] < clip < srt[nsteps // 2]
    del dry

    p0 = params_by_name(run_e.model)
    gs = GraphTrainStep(run_g, ('SNP', ids), bs, lr=LR, weight_decay=WD, sample_seed=seed, lr_schedule=COSINE, grad_clip_norm=clip)
    assert not gs.fused_adam and not gs.duv_pieces and gs.n_batches == nsteps
    assert (gs.lr_schedule.kind, gs.lr_schedule.warmup_steps, gs.lr_schedule.total_steps) == (2, 2, nsteps)
    for n, p in params_by_name(run_g.model).items():
        assert torch.equal(p, p0[n]), n                       # (the capture's warm-up steps were undone)
    opt_e = FusedAdam(run_e.model.parameters(), lr=LR, weight_decay=WD, lr_schedule=gs.lr_schedule, grad_clip_norm=clip)
    ld_w = run_e._ld_weight_vector()
    # torch's loop on a copy of the parameters
    names = [n for n, _ in run_e.model.named_parameters()]
    qs = [p.detach().clone().requires_grad_(True) for _, p in run_e.model.named_parameters()]
    opt_t = torch.optim.Adam(qs, lr=LR, weight_decay=WD)
    kw = dict(W=2, N=nsteps, r=R.f32(1e-4 / LR))

    def lam(ep):
        warm, decay = R.factor('cosine', ep + 1, **kw)
        return warm * decay
    sched_t = torch.optim.lr_scheduler.LambdaLR(opt_t, lam)
    scales_g, scales_e = [], []
    loader = NeighborLoader(small_kg.data, [-1, -1], ('SNP', ids), batch_size=bs, drop_last=True, device=DEV)
    for step, batch in enumerate(loader):
        le = run_e.train_step(batch, opt_e, ld_w)
        lg = gs.step(step)
        torch.cuda.synchronize()
        lr_ref = R.lr_at('cosine', LR, step + 1, **kw)
        for opt in (gs.opt, opt_e):
            assert abs(float(opt.last_lr) - float(lr_ref)) <= R.ulp32(lr_ref), (step, float(opt.last_lr), float(lr_ref))
        scales_g.append(float(gs.opt.last_clip_scale))
        scales_e.append(float(opt_e.last_clip_scale))
        print(f'step {step}: eager {float(le.detach()):.9f} captured {float(lg.detach()):.9f}; lr {float(opt_e.last_lr):.6e}; norm '
              f'{float(opt_e.last_grad_norm):.5f} / {float(gs.opt.last_grad_norm):.5f}; scale {scales_e[-1]:.5f} / {scales_g[-1]:.5f}')
        assert_close(lg.detach().clone(), le.detach(), 1e-5, 1e-7, f'loss step {step}')
        # the optimiser alone: torch on the eager product's own gradients
        for q, (_, p) in zip(qs, run_e.model.named_parameters()):
            q.grad = p.grad.detach().clone() if p.grad is not None else None
        torch.nn.utils.clip_grad_norm_([q for q in qs if q.grad is not None], clip)
        opt_t.step()
        sched_t.step()
        for n, q, (_, p) in zip(names, qs, run_e.model.named_parameters()):
            assert_close(p, q.detach(), 2e-6, 1e-7, f'{n} after step {step}', rel_to_max=0)
    gs.check()
    assert step == nsteps - 1 and int(gs.opt.step_dev) == int(opt_e.step_dev) == nsteps
    for scales in (scales_g, scales_e):
        assert any(s == 1.0 for s in scales) and any(s < 1.0 for s in scales), scales       # binds on some steps, not on others
    pe, pg = params_by_name(run_e.model), params_by_name(run_g.model)
    num = sum(float((pe[n] - pg[n]).pow(2).sum()) for n in pe)
    den = sum(float((pe[n] - p0[n]).pow(2).sum()) for n in pe)
    assert den > 0 and (num / den) ** 0.5 < 5e-3, f'relative update difference {(num / den) ** 0.5:.3e}'


# ------------------------------------------------------------------------------------------------------------------------------
# (f) routes
# ------------------------------------------------------------------------------------------------------------------------------
def _trainer(kg, seed=7, **kw):
    from kgwas_amd.graph_step import GraphTrainStep
    bs = 32
    ids = np.asarray(kg.train_input_nodes[1][:bs * 4])
    run = _run(kg, seed)
    return run, GraphTrainStep(run, ('SNP', ids), bs, lr=LR, weight_decay=WD, sample_seed=seed, **kw)


def _plain(names):
    """Kernel names with the optimiser's kernels reduced to which launch they are (the fused one or the plain one): with and
    without the controls they are kernels of their own names and argument lists."""
    out = []
    for n in names:
        if 'k_adam_fused' in n:
            n = 'k_adam_fused'
        elif 'k_adam' in n and 'k_adam_tick' not in n:
            n = 'k_adam'
        out.append(n)
    return sorted(out)


def test_routes(tiny_kg, monkeypatch):
    """A schedule alone keeps the default step's route: the fused optimiser launch, as many deferred gradients, the same launches
    (the optimiser's instantiation aside), and the rate moves under replay.  Clipping takes the unfused route -- the default step
    with the fused launch switched off -- plus exactly the two norm launches."""
    from kgwas_amd import ops
    run_0, gs_0 = _trainer(tiny_kg)
    run_s, gs_s = _trainer(tiny_kg, lr_schedule=COSINE)
    assert gs_0.fused_adam and gs_s.fused_adam and gs_0.duv_pieces == gs_s.duv_pieces
    assert gs_s.lr_schedule.total_steps == 4 and gs_0.lr_schedule is None and not hasattr(gs_0.opt, 'last_lr')
    for i in range(3):
        l0, ls = gs_0.step(i).detach().clone(), gs_s.step(i).detach().clone()
        if i == 0:
            assert torch.equal(l0, ls)                               # (the same model and batch; the rates differ from here on)
    gs_s.check()
    kw = dict(W=2, N=4, r=R.f32(1e-4 / LR))
    assert int(gs_s.opt.step_dev) == 3 and abs(float(gs_s.opt.last_lr) - float(R.lr_at('cosine', LR, 3, **kw))) <= R.ulp32(LR)
    assert gs_0.deferred_gradients == gs_s.deferred_gradients
    n0, ns = launches_of_one_step(gs_0), launches_of_one_step(gs_s)
    assert gs_0.deferred_gradients == gs_s.deferred_gradients and gs_0.riders_taken == gs_s.riders_taken
    assert len(n0) == len(ns) and _plain(n0) == _plain(ns)
    assert sum('k_adam_fused' in n for n in ns) == 1 and not any('k_grad_norm' in n for n in ns)
    pa, pb = params_by_name(run_0.model), params_by_name(run_s.model)
    assert any(not torch.equal(pa[n], pb[n]) for n in pa)            # another rate: another trajectory

    monkeypatch.setattr(ops, '_FUSED_ADAM', False)
    run_u, gs_u = _trainer(tiny_kg)
    monkeypatch.undo()
    run_c, gs_c = _trainer(tiny_kg, grad_clip_norm=1.0)
    assert not gs_u.fused_adam and not gs_c.fused_adam and not gs_c.duv_pieces and ops._FUSED_ADAM
    nu, nc = launches_of_one_step(gs_u), launches_of_one_step(gs_c)
    print(f'default {len(n0)} launches, schedule {len(ns)}, unfused {len(nu)}, clipped {len(nc)}')
    assert len(nc) == len(nu) + 2
    extra = sorted(set(_plain(nc)) - set(_plain(nu)))
    assert len(extra) == 2 and 'k_grad_norm_fold' in extra[0] and 'k_grad_norm_partial' in extra[1], extra
    from collections import Counter
    diff = Counter(_plain(nc)) - Counter(_plain(nu))
    assert sorted(diff.values()) == [1, 1] and not (Counter(_plain(nu)) - Counter(_plain(nc)))
    order = [n for n in nc if 'k_grad_norm' in n or 'k_adam' in n]
    assert 'k_grad_norm_partial' in order[0] and 'k_grad_norm_fold' in order[1] and 'k_adam' in order[2]


def test_without_the_knobs_no_new_entry_is_called(tiny_kg, monkeypatch):
    """Both None: the trainer, its capture and FusedAdam.step call none of the ``_ctl`` / kgw_grad_norm_* symbols (a counting wrapper
    around each); with a schedule the wrapper counts."""
    from kgwas_amd import _lib
    from kgwas_amd.optim import FusedAdam
    L = _lib.lib()
    calls = []
    for name in ('kgw_adam_ctl', 'kgw_adam_fused_ctl', 'kgw_grad_norm_partial', 'kgw_grad_norm_fold', 'kgw_grad_norm_workspace_doubles'):
        real = getattr(L, name)

        def wrapper(*a, _real=real, _name=name):
            calls.append(_name)
            return _real(*a)
        monkeypatch.setattr(L, name, wrapper)
    run, gs = _trainer(tiny_kg)
    for i in range(2):
        gs.step(i)
    gs.check()
    ps = [_rand(100, 1).to(DEV).requires_grad_(True)]
    ps[0].grad = _rand(100, 2).to(DEV)
    FusedAdam(ps, lr=LR).step()
    torch.cuda.synchronize()
    assert calls == []
    run, gs = _trainer(tiny_kg, lr_schedule='linear')
    gs.step(0)
    gs.check()
    assert calls and set(calls) == {'kgw_adam_fused_ctl'}


# ------------------------------------------------------------------------------------------------------------------------------
# train() and (g) refusals
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_graph', [True, False], ids=['captured', 'eager'])
def test_train_end_to_end(tiny_kg, use_graph):
    """KGWAS.train(epoch=2) with both knobs: total_steps defaults to epochs x batches, the rate read at the validation point is
    the twin's for the last update, nothing enters the configuration, and the eager loop runs FusedAdam."""
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(tiny_kg, device=DEV, seed=3)
    run.initialize_model()
    cfg = dict(run.config)
    run.train(batch_size=32, epoch=2, save_best_model=False, save_name='lr_schedule_e2e', use_graph=use_graph,
              lr_schedule={'kind': 'linear', 'warmup_steps': 3, 'min_lr': 1e-5}, grad_clip_norm=5.0, lr=LR)
    nb = len(run.train_loader)
    assert nb >= 2 and run.config == cfg and np.isfinite(run.val_metrics['mse'])
    want = R.lr_at('linear', LR, 2 * nb, W=3, N=2 * nb, r=R.f32(1e-5 / LR))
    print(f'{nb} batches per epoch; last_lr {run.last_lr:.6e} (twin {float(want):.6e})')
    assert abs(run.last_lr - float(want)) <= R.ulp32(want)
    assert all(bool(torch.isfinite(p).all()) for p in run.model.parameters())


def test_refusals_of_train(tiny_kg):
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(tiny_kg, device=DEV, seed=3)
    run.initialize_model()
    p0 = params_by_name(run.model)
    for kw in (dict(lr_schedule='cosine'), dict(grad_clip_norm=1.0)):
        with pytest.raises(NotImplementedError, match='lr_schedule / grad_clip_norm'):
            run.train(batch_size=32, epoch=1, parallelism='shard', **kw)
    for bad in (0, -1.0, float('nan'), float('inf'), 'big'):
        with pytest.raises(ValueError, match='grad_clip_norm'):
            run.train(batch_size=32, epoch=1, grad_clip_norm=bad)
    for bad in ('cosin', {'kind': 'step'}, {'kind': 'cosine', 'min_lr': 1.0}, {'kind': 'linear', 'warmup_steps': 1.5}):
        with pytest.raises(ValueError, match='lr_schedule'):
            run.train(batch_size=32, epoch=1, lr_schedule=bad)
    p1 = params_by_name(run.model)
    assert all(torch.equal(p0[n], p1[n]) for n in p0)
