"""The Huber loss of the read-out node without a GPU: the float64 twin (tests/robust_loss_ref.py) against torch's huber_loss with
autograd and against the MSE statement at delta = +inf, optim.parse_loss, the header / bindings / INTEGRATION.md, and the run
argument's refusals."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.multitrait_w_ref import readout_wmse_w_np
from tests.robust_loss_ref import make_case, make_case_w, readout_loss_np, residuals_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kgw_readout_loss_fwd', 'kgw_readout_loss_bwd', 'kgw_readout_loss_train')
INF = float('inf')


def _torch_statement(case, n, relu, gloss, delta):
    """loss and d loss / d pred of the rule from torch.nn.functional.huber_loss, column by column, weighted and averaged by hand;
    the unobserved pairs' labels are replaced by a finite number first (their weight is 0)."""
    H, W, b, n_id, y, w = case
    T = W.shape[0]
    ids = torch.from_numpy(np.asarray(n_id[:n], np.int64))
    wi = torch.from_numpy(np.asarray(w, np.float64))[ids]
    wi = wi[:, None].repeat(1, T) if wi.dim() == 1 else wi
    yi = torch.from_numpy(np.asarray(y, np.float64).reshape(-1, T))[ids]
    yi = torch.where(wi != 0, yi, torch.zeros_like(yi))
    z = torch.from_numpy(H[:n].astype(np.float64)) @ torch.from_numpy(W.astype(np.float64)).T + torch.from_numpy(b.astype(np.float64))
    pred = (torch.relu(z) if relu & 1 else z).detach().requires_grad_(True)
    loss = 0
    for t in range(T):
        rho = 2 * torch.nn.functional.huber_loss(pred[:, t], yi[:, t], reduction='none', delta=float(delta[t]))
        loss = loss + (wi[:, t] * rho).sum()
    loss = loss / (n * T)
    (loss * gloss).backward()
    return float(loss.detach()), pred.grad.numpy()


@pytest.mark.parametrize('T', (1, 3, 32))
def test_twin_equals_torch_huber_loss(T):
    """1a. Loss and d loss / d pred (recovered from db and dW of a case whose ReLU is off) to 1e-12 relative, one delta per column,
    both weight forms."""
    for n, rows, seed in ((5, 6, 1), (9, 16, 2), (64, 64, 3)):
        for case in (make_case(n, T, rows, seed), make_case_w(n, T, rows, seed)):
            _, _, r, wi, seen = residuals_np(*case, n, 0)
            delta = np.array([np.median(np.abs(r[seen[:, t], t])) if seen[:, t].any() else 1.0 for t in range(T)])
            delta[0] = max(delta[0], 1e-3)
            for gloss in (1.0, 0.7):
                pred, loss, dH, dW, db = readout_loss_np(*case, n, 0, gloss, rows, delta)
                loss_t, dpred_t = _torch_statement(case, n, 0, gloss, delta)
                assert abs(loss - loss_t) <= 1e-12 * abs(loss_t)
                Hn, Wl = case[0][:n].astype(np.float64), case[1].astype(np.float64)
                for got, ref in ((db, dpred_t.sum(0)), (dW, dpred_t.T @ Hn), (dH[:n], dpred_t @ Wl)):
                    assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300)
                assert not dH[n:].any()
                both = [(np.abs(r[seen[:, t], t]) < delta[t]).any() and (np.abs(r[seen[:, t], t]) > delta[t]).any() for t in range(T)]
                assert any(both)                            # (the cases exercise both branches)


@pytest.mark.parametrize('T', (1, 2, 31))
def test_twin_at_infinite_delta_is_the_mse_statement(T):
    """1b. delta = +inf: readout_wmse_w_np's outputs, exactly, at every relu word; a mixed delta leaves the +inf columns' dW / db."""
    for n, rows in ((1, 1), (4, 5), (9, 16)):
        case = make_case_w(n, T, rows, seed=n + T)
        for relu in (0, 1, 2, 3):
            a = readout_loss_np(*case, n, relu, 0.7, rows, INF)
            m = readout_wmse_w_np(*case, n, relu, 0.7, rows)
            for x, y in zip(a, m):
                assert np.array_equal(np.asarray(x), np.asarray(y))
            if T > 1:
                mixed = np.full(T, INF)
                mixed[1] = 0.05
                c = readout_loss_np(*case, n, relu, 0.7, rows, mixed)
                keep = np.arange(T) != 1
                assert np.array_equal(c[3][keep], m[3][keep]) and np.array_equal(c[4][keep], m[4][keep])


def test_the_gradient_is_bounded_by_the_knee():
    """|d loss / d pred| <= 2 delta w / N, whatever the label: one planted label of 1e6."""
    n, T, rows = 9, 3, 9
    H, W, b, n_id, y, w = make_case_w(n, T, rows, seed=4, p_zero=0.0, poison=False)
    y = y.copy()
    y[n_id[3], 1] = 1e6
    delta = np.array([0.5, 1.0, 2.0])
    _, loss, _, _, db = readout_loss_np(H, W, b, n_id, y, w, n, 0, 1.0, rows, delta)
    _, _, _, _, db_mse = readout_loss_np(H, W, b, n_id, y, w, n, 0, 1.0, rows, INF)
    assert math.isfinite(loss) and abs(db_mse[1]) > 1e4
    assert (np.abs(db) <= n * 2 * delta * w.max() / (n * T) * (1 + 1e-15)).all()


def test_parse_loss():
    """2. Every accepted form resolves as stated; every refusal is a ValueError."""
    from kgwas_amd.optim import LossRule, parse_loss
    f32 = lambda v: float(np.float32(v))
    for T in (1, 3):
        assert parse_loss(None, T) is None and parse_loss('mse', T) is None and parse_loss({'kind': 'mse'}, T) is None
        assert parse_loss('huber', T) == LossRule('huber', (1.0,) * T) == parse_loss({'kind': 'huber'}, T)
        assert parse_loss(0.25, T) == ('huber', (0.25,) * T)
        assert parse_loss(2, T) == ('huber', (2.0,) * T)
        assert parse_loss(0.1, T).delta == (f32(0.1),) * T                      # the float32 the kernels compare against
        assert parse_loss(np.float32(0.5), T).delta == (0.5,) * T
        assert parse_loss({'kind': 'huber', 'delta': INF}, T).delta == (INF,) * T
        assert parse_loss({'kind': 'huber', 'delta': [1.5] * T}, T).delta == (1.5,) * T
        rule = parse_loss({'kind': 'huber', 'delta': np.arange(1, T + 1, dtype=np.float64)}, T)
        assert rule.delta == tuple(float(t) for t in range(1, T + 1)) and parse_loss(rule, T) == rule
        assert isinstance(rule, tuple) and isinstance(rule.delta, tuple)        # immutable
        with pytest.raises(AttributeError):
            rule.kind = 'mse'
    assert parse_loss({'kind': 'huber', 'delta': (0.5, INF, 3.0)}, 3).delta == (0.5, INF, 3.0)
    bad = ['l1', 'Huber', '', True, False, 0, 0.0, -1.0, float('nan'), -INF, 1e-60, [1.0], (1.0, 2.0), object(),
           {'delta': 1.0}, {'kind': 'l1'}, {'kind': 'huber', 'delta': 0.0}, {'kind': 'huber', 'delta': -2.0},
           {'kind': 'huber', 'delta': float('nan')}, {'kind': 'huber', 'delta': -INF}, {'kind': 'huber', 'delta': [1.0, 2.0]},
           {'kind': 'huber', 'delta': [1.0, 1.0, float('nan')]}, {'kind': 'huber', 'delta': [1.0, 0.0, 1.0]},
           {'kind': 'huber', 'delta': 'big'}, {'kind': 'huber', 'delta': None}, {'kind': 'huber', 'delta': True},
           {'kind': 'huber', 'knee': 1.0}, {'kind': 'mse', 'delta': 1.0}, {'kind': 1}]
    for spec in bad:
        with pytest.raises(ValueError, match='loss'):
            parse_loss(spec, 3)
    with pytest.raises(ValueError, match='loss'):
        parse_loss({'kind': 'huber', 'delta': [1.0, 2.0, 3.0]}, 1)
    with pytest.raises(ValueError, match='loss'):
        parse_loss('huber', 0)


def test_header_bindings_and_integration_name_the_feature():
    """3. The header states the rule; the ctypes mirror has the header's layout; the three entry points are exported, bound and
    listed; the version stays."""
    from kgwas_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, 'include', 'kgwas_hip.h')).read()
    for word in ('#define KGW_LOSS_MSE   0', '#define KGW_LOSS_HUBER 1', 'typedef struct KgwReadoutLossArgs', 'float delta[32];',
                 'KgwReadoutFold* fold_out;', 'delta (2 |r| - delta)', '2 clamp(r, -delta, delta)',
                 '#define KGW_READOUT_LOSS_ARGS_BYTES 288'):
        assert word in hdr, word
    integ = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS and name in integ, name
        assert re.search(r'\bint ' + name + r'\(const KgwReadoutLossArgs\* args, kgw_stream_t stream\);', hdr), name
        assert getattr(L, name).argtypes == [C.POINTER(_lib.KgwReadoutLossArgs), C.c_void_p]
    assert _lib.has_readout_loss()
    assert L.kgw_version() == 125 and re.search(r'#define KGW_VERSION\s+125\b', hdr)           # detected by symbol: the version stays
    assert (_lib.KGW_LOSS_MSE, _lib.KGW_LOSS_HUBER) == (0, 1) and _lib.LOSS_KINDS == {'mse': 0, 'huber': 1}
    A = _lib.KgwReadoutLossArgs
    names = [f[0] for f in A._fields_]
    body = re.search(r'typedef struct KgwReadoutLossArgs \{(.*?)\} KgwReadoutLossArgs;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    declared = [re.sub(r'\[\d+\]', '', d.strip().split()[-1].lstrip('*')) for stmt in body.split(';') if stmt.strip()
                for d in stmt.split(',')]
    assert declared == names                                                    # the header's fields, in its order
    assert [getattr(A, f).offset for f in names[:17]] == [8 * i for i in range(17)]
    assert [getattr(A, f).offset for f in names[17:]] == [136, 140, 144, 148, 152, 156, 160]
    assert C.sizeof(A) == _lib.READOUT_LOSS_ARGS_BYTES == 288 and A.delta.size == 128
    # kgw_struct_sizes keeps its eleven entries
    s = (C.c_int64 * 13)(*([-1] * 13))
    assert L.kgw_struct_sizes(s, 13) == 0 and s[10] == C.sizeof(_lib.KgwWeightAvg) and s[11] == s[12] == -1


def test_argument_checks_refuse_before_the_device_is_needed():
    """The C calls' refusals need no GPU: they return before any launch."""
    from kgwas_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 64)()
    ptr = C.addressof(buf)

    def record(**kw):
        a = _lib.KgwReadoutLossArgs()
        for f in ('H', 'W', 'b', 'n_id', 'y', 'w', 'pred_in', 'grad_loss', 'pred', 'loss', 'dH', 'dW', 'db', 'terms', 'scratch'):
            setattr(a, f, ptr)
        a.rows, a.n, a.T, a.relu, a.loss_kind = 8, 5, 2, 1, _lib.KGW_LOSS_HUBER
        for t in range(32):
            a.delta[t] = 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    calls = [getattr(L, n) for n in NEW]
    for fn in calls:
        assert fn(None, None) == -1
        for bad in (dict(n=0), dict(T=0), dict(T=33), dict(loss_kind=2), dict(loss_kind=-1)):
            assert fn(C.byref(record(**bad)), None) == -2, bad
        for v in (float('nan'), 0.0, -0.0, -1.0, -INF):
            a = record()
            a.delta[1] = v
            assert fn(C.byref(a), None) == -2, v
            a = record(loss_kind=_lib.KGW_LOSS_MSE, n=0)
            a.delta[1] = v
            assert fn(C.byref(a), None) == -2                                   # (MSE does not read delta: refused for n alone)
        for f in ('H', 'W', 'n_id', 'y', 'w'):
            assert fn(C.byref(record(**{f: None})), None) == -1, f
    fwd, bwd, train = calls
    assert bwd(C.byref(record(rows=4)), None) == -2 and train(C.byref(record(rows=4)), None) == -2       # rows < n
    for f in ('b', 'pred', 'loss', 'terms'):
        assert fwd(C.byref(record(**{f: None})), None) == -1 and train(C.byref(record(**{f: None})), None) == -1, f
    for f in ('pred_in', 'grad_loss', 'dH', 'dW', 'db', 'scratch'):
        assert bwd(C.byref(record(**{f: None})), None) == -1, f
    for f in ('dH', 'dW', 'db', 'scratch'):
        assert train(C.byref(record(**{f: None})), None) == -1, f
    fold = _lib.KgwReadoutFold()
    assert train(C.byref(record(fold_out=C.pointer(fold))), None) == _lib.KGW_E_UNSUPPORTED
    assert fold.nb == 0 and fold.n == 0 and not fold.scratch


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path_factory.mktemp('robust')))


def test_the_argument_exists_at_every_level_and_the_run_refuses(tiny):
    """4. loss / loss_rule default to None everywhere; parallelism='shard' refuses a Huber loss (and takes 'mse' for what it is: the
    default); a bad specification is a ValueError before anything is built; config keeps its keys."""
    from kgwas_amd import ops
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.model import HeteroGNN
    for fn, name in ((KGWAS.train, 'loss'), (KGWAS._train_sharded, 'loss'), (GraphTrainStep.__init__, 'loss'),
                     (KGWAS.train_step, 'loss_rule'), (HeteroGNN.forward_loss, 'loss_rule'), (ops.readout_weighted_mse, 'loss_rule')):
        assert inspect.signature(fn).parameters[name].default is None, fn
    run = KGWAS(tiny, device='cpu', seed=1)
    run.initialize_model()
    before = dict(run.config)
    for spec in ('huber', 0.5, {'kind': 'huber', 'delta': 2.0}):
        with pytest.raises(NotImplementedError, match='loss'):
            run.train(epoch=1, parallelism='shard', loss=spec)
    for spec in ('l1', -1.0, {'kind': 'huber', 'delta': [1.0, 2.0]}):
        with pytest.raises(ValueError, match='loss'):
            run.train(epoch=1, loss=spec)
    assert run.config == before and 'loss' not in run.config
