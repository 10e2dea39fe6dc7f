"""CPU: the learning-rate rule (include/kgwas_hip.h: KgwLrSchedule, kgwlr_at; the host export kgw_lr_at), its ctypes mirrors and
optim.parse_lr_schedule, against the numpy float64 twin of tests/lr_schedule_ref.py.  No kernel is launched."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import lr_schedule_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['kgw_adam_ctl', 'kgw_adam_fused_ctl', 'kgw_lr_at', 'kgw_grad_norm_partial', 'kgw_grad_norm_fold',
       'kgw_grad_norm_workspace_doubles']


def _sched(kind, W=0, N=1, r=0.0, step_size=1, gamma=0.1):
    from kgwas_amd import _lib
    return _lib.KgwLrSchedule(R.KINDS[kind], W, N, step_size, r, gamma)


def _at(s, lr, t):
    from kgwas_amd import _lib
    return _lib.lib().kgw_lr_at(C.byref(s), lr, t)


def test_header_names_the_rule_and_the_mirrors_match():
    from kgwas_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, 'include', 'kgwas_hip.h')).read()
    for word in ('typedef struct KgwLrSchedule', 'typedef struct KgwOptimCtl', 'kgwlr_at', 'kgwlr_valid', 'KGW_LR_CONSTANT = 0',
                 'KGW_LR_LINEAR = 1', 'KGW_LR_COSINE = 2', 'KGW_LR_STEP = 3', 'warm(s)', 'decay(s)', 'lr_t',
                 '#define KGW_GRAD_NORM_UNIT 1024'):
        assert word in hdr, word
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS and re.search(r'\b' + name + r'\s*\(', hdr), name
    assert _lib.has_optim_ctl()
    assert L.kgw_version() == 125 and re.search(r'#define KGW_VERSION\s+125\b', hdr)
    s10 = (C.c_int64 * 10)(*([-1] * 10))
    assert L.kgw_struct_sizes(s10, 10) == 0
    assert [s10[8], s10[9]] == [C.sizeof(_lib.KgwLrSchedule), C.sizeof(_lib.KgwOptimCtl)] == [24, 40]
    s8 = (C.c_int64 * 10)(*([-1] * 10))
    assert L.kgw_struct_sizes(s8, 8) == 0 and list(s8)[:8] == list(s10)[:8] and s8[8] == s8[9] == -1
    assert [f[0] for f in _lib.KgwLrSchedule._fields_] == ['kind', 'warmup_steps', 'total_steps', 'step_size', 'min_ratio', 'gamma']
    assert [f[0] for f in _lib.KgwOptimCtl._fields_] == ['sched', 'grad_scale_dev', 'lr_out_dev']
    assert _lib.KgwOptimCtl.grad_scale_dev.offset == 24 and _lib.KgwOptimCtl.lr_out_dev.offset == 32
    assert _lib.LR_KINDS == R.KINDS and _lib.GRAD_NORM_UNIT == 1024


SHAPES = [dict(W=3, N=8), dict(W=0, N=8), dict(W=5, N=40), dict(W=8, N=8), dict(W=12, N=8), dict(W=1, N=2), dict(W=0, N=1),
          dict(W=100, N=1000)]


@pytest.mark.parametrize('kind', list(R.KINDS))
def test_host_rule_equals_the_twin(kind):
    """Every kind at t = 1, W-1, W, W+1, W+2, N-1, N, N+1, 10 N and at each step_size boundary +- 1; W = 0, W >= N, r = 0 and 1
    among the shapes: to 1 float32 ulp of lr."""
    n = 0
    for lr in (1e-4, 1e-3, 0.37):
        for shape in SHAPES:
            W, N = shape['W'], shape['N']
            for r in (0.0, 0.1, 1.0):
                for step_size, gamma in ((2, 0.5), (7, 0.1), (1, 0.9)):
                    if kind != 'step' and (step_size, gamma) != (2, 0.5):
                        continue
                    if kind in ('constant', 'step') and r != 0.0:
                        continue
                    ts = {1, W - 1, W, W + 1, W + 2, N - 1, N, N + 1, 10 * N}
                    if kind == 'step':
                        for k in range(1, 5):
                            ts |= {W + k * step_size + d for d in (0, 1, 2)}           # t = s + 1: s = boundary - 1, boundary, + 1
                    kw = dict(W=W, N=N, r=r, step_size=step_size, gamma=gamma)
                    s = _sched(kind, **kw)
                    for t in sorted(t for t in ts if t >= 1):
                        got, ref = _at(s, lr, t), float(R.lr_at(kind, lr, t, **kw))
                        assert got == float(np.float32(got))                            # a float32 value
                        assert abs(got - ref) <= R.ulp32(R.f32(lr)), (kind, lr, kw, t, got, ref)
                        n += 1
    assert n > 100


def test_constant_without_warmup_is_lr_to_the_bit():
    for lr in (1e-4, 1e-3, 0.1, 3.0):
        s = _sched('constant', 0, 5)
        for t in (1, 2, 5, 6, 1000, 2 ** 31 - 1):
            assert _at(s, lr, t) == R.f32(lr)
    # t < 1 is taken as t = 1
    assert _at(_sched('linear', 4, 10), 1e-3, 0) == _at(_sched('linear', 4, 10), 1e-3, 1) == float(np.float32(R.f32(1e-3) / 4))


@pytest.mark.parametrize('kind', list(R.KINDS))
def test_warmup_reaches_lr_and_decay_never_rises(kind):
    lr = 1e-3
    for W, N in ((3, 8), (1, 8), (5, 40), (8, 8), (12, 8)):
        for r in (0.0, 0.25, 1.0):
            s = _sched(kind, W, N, r, 3, 0.5)
            assert _at(s, lr, W) == R.f32(lr)                                           # s = W - 1: (s + 1) / W == 1
            warm = [_at(s, lr, t) for t in range(1, W + 1)]
            assert all(a < b for a, b in zip(warm, warm[1:]))
            tail = [_at(s, lr, t) for t in range(W, 3 * max(N, W) + 2)]
            assert all(a >= b for a, b in zip(tail, tail[1:])), (kind, W, N, r)
            if kind in ('linear', 'cosine'):
                floor = float(np.float32(R.f32(lr) * R.f32(r)))
                assert abs(tail[-1] - floor) <= R.ulp32(lr) and _at(s, lr, max(N, W + 1) + 1) == tail[-1]   # (u = 1 from there on)
            if kind == 'constant':
                assert set(tail) == {R.f32(lr)}


def test_refused_schedules():
    """kgw_lr_at of a schedule kgwlr_valid refuses is NaN; the same table as the entry points' KGW_E_RANGE."""
    from kgwas_amd import _lib
    L = _lib.lib()
    bad = [_lib.KgwLrSchedule(4, 0, 8, 1, 0.0, 0.1), _lib.KgwLrSchedule(-1, 0, 8, 1, 0.0, 0.1), _lib.KgwLrSchedule(1, -1, 8, 1, 0.0, 0.1),
           _lib.KgwLrSchedule(1, 0, 0, 1, 0.0, 0.1), _lib.KgwLrSchedule(3, 0, 8, 0, 0.0, 0.1), _lib.KgwLrSchedule(2, 0, 8, 1, -0.1, 0.1),
           _lib.KgwLrSchedule(2, 0, 8, 1, 1.5, 0.1), _lib.KgwLrSchedule(2, 0, 8, 1, float('nan'), 0.1),
           _lib.KgwLrSchedule(3, 0, 8, 1, 0.0, 0.0), _lib.KgwLrSchedule(3, 0, 8, 1, 0.0, -1.0),
           _lib.KgwLrSchedule(3, 0, 8, 1, 0.0, float('inf')), _lib.KgwLrSchedule(0, 0, 8, 1, 0.0, float('nan'))]
    for s in bad:
        assert math.isnan(L.kgw_lr_at(C.byref(s), 1e-3, 1)), (s.kind, s.warmup_steps, s.total_steps, s.step_size, s.min_ratio, s.gamma)
    assert math.isnan(L.kgw_lr_at(None, 1e-3, 1))
    assert L.kgw_lr_at(C.byref(_lib.KgwLrSchedule(1, 0, 8, 0, 0.0, 0.1)), 1e-3, 1) == R.f32(1e-3)   # step_size is STEP's alone
    # the argument checks of the device entry points come before any launch (no GPU here)
    ok = _lib.KgwOptimCtl(_lib.KgwLrSchedule(0, 0, 1, 1, 0.0, 1.0), None, None)
    for s in bad:
        ctl = _lib.KgwOptimCtl(s, None, None)
        assert L.kgw_adam_ctl(0, None, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, C.byref(ctl), None) == -2
        assert L.kgw_adam_fused_ctl(0, None, None, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, 0, 0, None, None,
                                    C.byref(ctl), None) == -2
    assert L.kgw_adam_ctl(0, None, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, C.byref(ok), None) == 0
    one = C.c_float(1.0)
    scaled = _lib.KgwOptimCtl(ok.sched, C.cast(C.pointer(one), C.c_void_p), None)
    assert L.kgw_adam_fused_ctl(0, None, None, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, 0, 0, None, None,
                                C.byref(scaled), None) == -3
    # the norm calls
    n1 = (C.c_int64 * 3)(1023, 1024, 1025)
    assert L.kgw_grad_norm_workspace_doubles(3, n1) == 1 + 1 + 2
    assert L.kgw_grad_norm_workspace_doubles(2, (C.c_int64 * 2)(0, 3 * 1024 + 7)) == 4
    assert L.kgw_grad_norm_partial(65, None, None, None, 0, None) == -2 and L.kgw_grad_norm_partial(1, None, None, None, 0, None) == -1
    assert L.kgw_grad_norm_partial(0, None, None, None, 0, None) == 0 and L.kgw_grad_norm_partial(1, None, None, None, -1, None) == -2
    assert L.kgw_grad_norm_fold(None, 1, 1.0, None, None, None) == -1
    buf = (C.c_double * 1)()
    out = C.c_float()
    for count, mx in ((0, 1.0), (1, 0.0), (1, -1.0), (1, float('inf')), (1, float('nan'))):
        assert L.kgw_grad_norm_fold(buf, count, mx, None, C.byref(out), None) == -2


def test_parse_lr_schedule():
    from kgwas_amd import _lib
    from kgwas_amd.optim import check_grad_clip_norm, parse_lr_schedule
    assert parse_lr_schedule(None, 1e-3, 100) is None
    s = parse_lr_schedule('cosine', 1e-3, 100)
    assert (s.kind, s.warmup_steps, s.total_steps, s.min_ratio) == (2, 0, 100, 0.0)
    s = parse_lr_schedule({'kind': 'linear', 'warmup_steps': 10, 'min_lr': 1e-4, 'total_steps': 50}, 1e-3, 100)
    assert (s.kind, s.warmup_steps, s.total_steps) == (1, 10, 50) and s.min_ratio == R.f32(1e-4 / 1e-3)
    s = parse_lr_schedule({'kind': 'step', 'step_size': np.int64(30), 'gamma': 0.5, 'warmup_steps': 2.0}, 1e-3, 100)
    assert (s.kind, s.step_size, s.gamma, s.warmup_steps) == (3, 30, 0.5, 2)
    assert parse_lr_schedule({'kind': 'step', 'step_size': 3}, 1e-3, 9).gamma == R.f32(0.1)
    assert parse_lr_schedule('constant', 1e-3, 1).kind == 0
    assert parse_lr_schedule(s, 1e-3, None) is s
    assert parse_lr_schedule({'kind': 'cosine', 'min_lr': 1e-3}, 1e-3, 5).min_ratio == 1.0
    bad = ['cosin', 7, ['cosine'], {'warmup_steps': 3}, {'kind': 'cosine', 'warmup': 3}, {'kind': 'cosine', 'min_lr': 2e-3},
           {'kind': 'cosine', 'min_lr': -1e-5}, {'kind': 'cosine', 'min_lr': float('nan')}, {'kind': 'linear', 'warmup_steps': -1},
           {'kind': 'linear', 'warmup_steps': 2.5}, {'kind': 'linear', 'warmup_steps': True}, {'kind': 'linear', 'total_steps': 0},
           {'kind': 'linear', 'total_steps': 7.5}, {'kind': 'linear', 'total_steps': 2 ** 31}, 'step', {'kind': 'step'},
           {'kind': 'step', 'step_size': 0}, {'kind': 'step', 'step_size': 1.5}, {'kind': 'step', 'step_size': 3, 'gamma': 0.0},
           {'kind': 'step', 'step_size': 3, 'gamma': float('inf')}, {'kind': 'step', 'step_size': 3, 'gamma': -0.5},
           _lib.KgwLrSchedule(7, 0, 1, 1, 0.0, 1.0)]
    for spec in bad:
        with pytest.raises(ValueError):
            parse_lr_schedule(spec, 1e-3, 100)
    with pytest.raises(ValueError):
        parse_lr_schedule('cosine', 1e-3, None)                       # nobody named total_steps
    with pytest.raises(ValueError):
        parse_lr_schedule('cosine', 1e-3, 0)
    with pytest.raises(ValueError):
        parse_lr_schedule('cosine', float('nan'), 10)
    assert check_grad_clip_norm(None) is None and check_grad_clip_norm(2) == 2.0
    for v in (0, -1.0, float('nan'), float('inf'), 'x', True):
        with pytest.raises(ValueError):
            check_grad_clip_norm(v)
    # what the parser builds evaluates like the twin
    s = parse_lr_schedule({'kind': 'cosine', 'warmup_steps': 3, 'min_lr': 1e-5}, 1e-3, 8)
    for t in range(1, 14):
        ref = float(R.lr_at('cosine', 1e-3, t, W=3, N=8, r=R.f32(1e-5 / 1e-3)))
        assert abs(_at(s, 1e-3, t) - ref) <= R.ulp32(1e-3)


def test_the_arguments_exist_at_every_level_and_default_to_off():
    import inspect
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.optim import FusedAdam
    for fn in (KGWAS.train, GraphTrainStep.__init__, FusedAdam.__init__):
        sig = inspect.signature(fn).parameters
        assert sig['lr_schedule'].default is None and sig['grad_clip_norm'].default is None
    assert {'lr_schedule', 'grad_clip_norm'} <= set(inspect.signature(KGWAS._train_sharded).parameters)
