"""-m gpu: the read-out node with a loss kind at the C ABI -- kgw_readout_loss_fwd / _bwd / _train against the existing entry points
(KGW_LOSS_MSE and Huber at delta = +inf: bit for bit) and against the float64 twin of tests/robust_loss_ref.py (both branches of the
Huber loss, exact integer cases, mixed columns, the gradient bound, refusals).  Shapes: tests/test_gpu_multitrait_w.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import assert_close
from tests.robust_loss_ref import make_case, make_case_w, readout_loss_np, residuals_np

pytestmark = pytest.mark.gpu

RT, AT = 1e-4, 1e-5            # the project's fp32 rule: |a - b| <= 1e-5 + 1e-4 |b| + 1e-5 max|b| (helpers.assert_close)
KGW_E_RANGE, KGW_E_UNSUPPORTED = -2, -3
NS, TS = (1, 3, 4, 5, 9), (1, 2, 3, 31, 32)
NAMES = ('pred', 'loss', 'dH', 'dW', 'db')
MSE, HUBER = 0, 1
INF = float('inf')
FORMS = ('n', 'nt')            # w [N] (kgw_readout_wmse_* / _mt_*), w [N, T] (kgw_readout_wmse_* / _mtw_*)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _dev(case):
    return [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in case]


def _shapes(T):
    """tests/test_gpu_multitrait_w.py::_shapes: n at 1, below / at / above one block of four seeds, three blocks; rows = n, n + 1 and
    n + 7 (blocks without seeds); at T = 32 also 129 blocks (the fold's groups of 7 and 28 blocks crossed, with a tail)."""
    out = [(n, n + extra) for n in NS for extra in (0, 1, 7)]
    return out + [(513, 520)] if T == 32 else out


def _case(form, n, T, rows, seed):
    """One case of a weight form.  T = 1 and the shared weight have no unobserved pairs: their zero weights keep finite labels."""
    if form == 'n':
        return make_case(n, T, rows, seed)
    return make_case_w(n, T, rows, seed, poison=T > 1)


def _outputs(n, rows, T, fill):
    pred = torch.full((n, T), fill, device='cuda')
    loss = torch.full((), fill, dtype=torch.float64, device='cuda')
    dH = torch.full((rows, 128), fill, device='cuda')
    dW, db = torch.full((T, 128), fill, device='cuda'), torch.full((T,), fill, device='cuda')
    return pred, loss, dH, dW, db


def _record(dv, n, rows, T, relu, kind, delta, out, work, **extra):
    from kgwas_amd import _lib
    H, W, b, n_id, y, w = dv
    a = _lib.KgwReadoutLossArgs()
    a.H, a.W, a.b, a.n_id, a.y, a.w = H.data_ptr(), W.data_ptr(), b.data_ptr(), n_id.data_ptr(), y.data_ptr(), w.data_ptr()
    pred, loss, dH, dW, db = out
    a.pred, a.loss, a.dH, a.dW, a.db = pred.data_ptr(), loss.data_ptr(), dH.data_ptr(), dW.data_ptr(), db.data_ptr()
    a.terms, a.scratch = work[0].data_ptr(), work[1].data_ptr()
    a.rows, a.n, a.T, a.relu, a.w_cols, a.loss_kind = rows, n, T, relu, int(w.dim() == 2), kind
    if delta is not None:
        for t, d in enumerate(np.broadcast_to(np.asarray(delta, np.float32), (T,)) if 1 <= T <= 32 else delta):
            a.delta[t] = float(d)
    for k, v in extra.items():
        setattr(a, k, v)
    return a


def _work(n, rows, T, fill=None):
    size = ((rows + 3) // 4) * max(T, 1) * 129
    if fill is None:
        return torch.empty(n, dtype=torch.float64, device='cuda'), torch.empty(size, device='cuda')
    return torch.full((n,), fill, dtype=torch.float64, device='cuda'), torch.full((size,), fill, device='cuda')


def _new_train(dv, n, rows, T, relu, kind, delta, fold=False):
    """kgw_readout_loss_train; ``fold``: the fold_out form followed by kgw_readout_train_fold.  Outputs start as NaN so that an
    unwritten element shows."""
    from kgwas_amd import _lib
    L = _lib.lib()
    out, work = _outputs(n, rows, T, float('nan')), _work(n, rows, T)
    f = _lib.KgwReadoutFold()
    a = _record(dv, n, rows, T, relu, kind, delta, out, work, **({'fold_out': C.pointer(f)} if fold else {}))
    assert L.kgw_readout_loss_train(C.byref(a), _lib.stream_ptr()) == 0
    if fold:
        assert (f.nb, f.n) == ((n + 3) // 4, n)
        assert L.kgw_readout_train_fold(C.byref(f), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    return out


def _new_fwd_bwd(dv, n, rows, T, relu, kind, delta, gloss):
    from kgwas_amd import _lib
    L = _lib.lib()
    out, work = _outputs(n, rows, T, float('nan')), _work(n, rows, T)
    assert L.kgw_readout_loss_fwd(C.byref(_record(dv, n, rows, T, relu, kind, delta, out, work)), _lib.stream_ptr()) == 0
    g = torch.tensor(gloss, dtype=torch.float64, device='cuda')
    a = _record(dv, n, rows, T, relu, kind, delta, out, work, pred_in=out[0].data_ptr(), grad_loss=g.data_ptr())
    assert L.kgw_readout_loss_bwd(C.byref(a), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    return out


def _old(dv, n, rows, T, relu, form, how, gloss=1.0):
    """The existing entry points: kgw_readout_wmse_* (T = 1), _mt_ (w [N]), _mtw_ (w [N, T]).  ``how``: 'train', 'fold' (T = 1:
    kgw_readout_wmse_train_parts + kgw_readout_train_fold) or 'fwd_bwd'."""
    from kgwas_amd import _lib
    L = _lib.lib()
    H, W, b, n_id, y, w = dv
    pred, loss, dH, dW, db = out = _outputs(n, rows, T, float('nan'))
    terms, part = _work(n, rows, T)
    st = _lib.stream_ptr()
    g = torch.tensor(gloss, dtype=torch.float64, device='cuda')
    if T == 1:
        if how == 'train':
            rc = L.kgw_readout_wmse_train(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, rows, relu, _p(pred), _p(loss), _p(dH), _p(dW),
                                          _p(db), _p(terms), _p(part), st)
        elif how == 'fold':
            f = _lib.KgwReadoutFold()
            rc = L.kgw_readout_wmse_train_parts(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, rows, relu, _p(pred), _p(loss), _p(dH),
                                                _p(dW), _p(db), _p(terms), _p(part), C.byref(f), st)
            assert rc == 0
            rc = L.kgw_readout_train_fold(C.byref(f), st)
        else:
            rc = L.kgw_readout_wmse_fwd(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, relu & 1, _p(pred), _p(loss), _p(terms), st)
            assert rc == 0
            rc = L.kgw_readout_wmse_bwd(_p(H), _p(W), _p(pred), _p(n_id), _p(y), _p(w), n, rows, relu, _p(g), _p(dH), _p(dW), _p(db),
                                        _p(part), st)
    else:
        fam = 'kgw_readout_wmse_mtw_' if form == 'nt' else 'kgw_readout_wmse_mt_'
        if how == 'train':
            rc = getattr(L, fam + 'train')(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, rows, T, relu, _p(pred), _p(loss), _p(dH),
                                           _p(dW), _p(db), _p(terms), _p(part), st)
        else:
            rc = getattr(L, fam + 'fwd')(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, T, relu & 1, _p(pred), _p(loss), _p(terms), st)
            assert rc == 0
            rc = getattr(L, fam + 'bwd')(_p(H), _p(W), _p(pred), _p(n_id), _p(y), _p(w), n, rows, T, relu, _p(g), _p(dH), _p(dW), _p(db),
                                         _p(part), st)
    assert rc == 0
    torch.cuda.synchronize()
    return out


def _same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), f'{what} {name}'


@pytest.mark.parametrize('T', TS)
def test_mse_and_infinite_delta_are_the_existing_entries(T):
    """5. Anchor.  loss_kind = MSE and HUBER with every delta = +inf: pred, loss, dH, dW, db of train, of fwd + bwd at grad_loss = 0.7
    and (T = 1) of the fold_out form + kgw_readout_train_fold are torch.equal to the existing entry's, at every shape, relu word and
    weight form."""
    for form in FORMS:
        for n, rows in _shapes(T):
            dv = _dev(_case(form, n, T, rows, seed=7 * n + T))
            for relu in (0, 1, 2, 3):
                what = f'T={T} form={form} n={n} rows={rows} relu={relu}'
                old_train, old_fb = _old(dv, n, rows, T, relu, form, 'train'), _old(dv, n, rows, T, relu, form, 'fwd_bwd', 0.7)
                for f in old_train + old_fb:
                    assert not torch.isnan(f).any(), what         # (NaN never equals NaN: the comparison below would be void)
                for kind, delta in ((MSE, None), (HUBER, INF)):
                    _same(_new_train(dv, n, rows, T, relu, kind, delta), old_train, f'{what} kind={kind} train')
                    _same(_new_fwd_bwd(dv, n, rows, T, relu, kind, delta, 0.7), old_fb, f'{what} kind={kind} fwd+bwd')
                    if T == 1:
                        old_fold = _old(dv, n, rows, T, relu, form, 'fold')
                        _same(old_fold, old_train, what + ' the existing fold form')
                        _same(_new_train(dv, n, rows, T, relu, kind, delta, fold=True), old_fold, f'{what} kind={kind} fold_out')


def _tolerance(ref):
    return AT + RT * np.abs(ref) + 1e-5 * np.abs(ref).max()


def _median_case(form, n, T, rows, relu, base):
    """The first seed from ``base`` on whose case, on the reference alone, has: delta[t] = the median observed |r| of column t (float32;
    1.0 for a column nothing observes) > 0; residuals strictly on both sides of delta[t] in every column with >= 2 observed pairs
    whose median is not a tied value; from n = 3 on at least one such column; and, with one, a Huber dH (at grad_loss = n T) further
    than 100 tolerances from the MSE dH.  (A tied median: make_case repeats SNPs among the seeds, and where the read-out ReLU is off
    two seeds of one SNP have the same residual -y; with 31 columns some column of every seed's case has that, and a median that
    sits on tied values can have nothing strictly on one side.  A column with ONE observed pair has delta = |r|: the knee itself,
    where the two losses agree -- with n = 1 that is every column, so the last condition cannot be asked there.)"""
    for seed in range(base, base + 64):
        case = _case(form, n, T, rows, seed)
        _, _, r, _, seen = residuals_np(*case, n, relu)
        delta = np.ones(T, np.float32)
        ok, two = True, False
        for t in range(T):
            a = np.abs(r[seen[:, t], t])
            if len(a):
                delta[t] = np.float32(np.median(a))
            if not delta[t] > 0:
                ok = False
            if len(a) >= 2 and (a == np.median(a)).sum() < 2:
                two = True
                ok = ok and bool((a < float(delta[t])).any() and (a > float(delta[t])).any())
        if not ok or (n >= 3 and not two):
            continue
        d64 = delta.astype(np.float64)
        if two:
            hub = readout_loss_np(*case, n, relu, float(n * T), rows, d64)[2]
            mse = readout_loss_np(*case, n, relu, float(n * T), rows, INF)[2]
            if not (np.abs(hub - mse) / _tolerance(hub)).max() > 100:
                continue
        return case, delta, two
    raise AssertionError(f'no case in 64 seeds: form={form} n={n} T={T} rows={rows} relu={relu}')


def _check(got, ref, n, T, what):
    pred, loss, dH, dW, db = got
    pred_r, loss_r, dH_r, dW_r, db_r = ref
    for t, name in zip(got, NAMES):
        assert bool(torch.isfinite(t).all()), f'{what}: {name} is not finite'
    assert_close(pred, torch.from_numpy(pred_r), RT, AT, what + ' pred')
    lv = float(loss)
    if T > 1:
        assert abs(lv - loss_r) <= 1e-6 * abs(loss_r), (what, lv, loss_r)       # float64 throughout
    else:
        assert abs(lv - loss_r) <= 1e-9 + 2e-6 * abs(loss_r), (what, lv, loss_r)  # tests/test_gpu_dense.py: a float32 residual
    assert_close(dH, torch.from_numpy(dH_r), RT, AT, what + ' dH')
    assert not dH[n:].ne(0).any(), what + ': dH beyond the seeds must be exactly zero'
    assert_close(dW, torch.from_numpy(dW_r), RT, AT, what + ' dW')
    assert_close(db, torch.from_numpy(db_r), RT, AT, what + ' db')


@pytest.mark.parametrize('T', TS)
def test_both_branches_match_the_twin(T):
    """6. delta[t] = the median observed |r| of the column (see _median_case for what the reference guarantees about every case):
    finite outputs, the twin's under the fp32 rule, the loss to 1e-6 relative (T = 1: 1e-9 + 2e-6, a float32 residual), dH[n:]
    exactly zero -- in the train form and in forward + backward at grad_loss = n T.  The unit gradient of the train form makes
    gradients of 1 / (n T): against the rule's absolute 1e-5 they could not tell Huber from MSE at the larger shapes, so the condition
    '100 tolerances from the MSE' is asked (and met) at grad_loss = n T, where d pred is of the residuals' order."""
    for form in FORMS:
        for n, rows in _shapes(T):
            for relu in (0, 1, 2, 3):
                what = f'T={T} form={form} n={n} rows={rows} relu={relu}'
                case, delta, two = _median_case(form, n, T, rows, relu, base=11 * n + T)
                d64 = delta.astype(np.float64)
                dv = _dev(case)
                ref = readout_loss_np(*case, n, relu, 1.0, rows, d64)
                _check(_new_train(dv, n, rows, T, relu, HUBER, delta), ref, n, T, what + ' train')
                k = float(n * T)
                _check(_new_fwd_bwd(dv, n, rows, T, relu, HUBER, delta, k), readout_loss_np(*case, n, relu, k, rows, d64), n, T,
                       what + ' fwd+bwd')


def _integer_case(n, T, rows, seed, delta):
    """One-hot H rows, integer W, b, y, dyadic weights, n T a power of two: every residual is a small integer, some equal +-delta[t]
    exactly (planted), and every product and sum of the node is exact in float32 / float64."""
    rng = np.random.default_rng(seed)
    H = np.zeros((rows, 128), np.float32)
    cols = rng.integers(0, 128, rows)
    H[np.arange(rows), cols] = 1.0
    W = rng.integers(-3, 4, (T, 128)).astype(np.float32)
    b = rng.integers(-2, 3, T).astype(np.float32)
    n_id = rng.permutation(n + 3)[:n].astype(np.int32)
    y = rng.integers(-4, 5, (n + 3, T)).astype(np.float32)
    w = np.ascontiguousarray(rng.choice([0.25, 0.5, 1.0, 2.0], (n + 3, T)))
    z = W[:, cols[:n]].T + b                                                     # [n, T], exact
    for t in range(T):                                                           # pred - y = +delta at seed 0, -delta at seed 1
        y[n_id[0], t] = z[0, t] - delta[t]
        y[n_id[1 % n], t] = z[1 % n, t] + delta[t] if n > 1 else y[n_id[0], t]
    return H, W, b, n_id, y, w


@pytest.mark.parametrize('T', (1, 2, 4, 32))
def test_exact_values_and_the_knee(T):
    """7. Integer residuals, some exactly +-delta: loss and gradients equal the twin's bit for bit after its one rounding to float32
    (the loss: float64, none).  Then one seed whose column t has residual +delta, -delta, 3 delta, 0, ...: db[t] is d pred itself,
    +-2 delta scale at the knee, and the knee's loss term is delta^2."""
    delta = np.array([1.0, 2.0, 3.0, 2.0] * 8, np.float32)[:T]
    n, rows = 8, 9
    for form in FORMS:
        H, W, b, n_id, y, w = _integer_case(n, T, rows, seed=T, delta=delta)
        case = (H, W, b, n_id, y, w if form == 'nt' else np.ascontiguousarray(w[:, 0]))
        _, _, r, _, _ = residuals_np(*case, n, 0)
        assert (r[0] == delta).all() and (r[1] == -delta).all() and (np.abs(r) > delta).any() and (np.abs(r) < delta).any()
        assert (r == np.round(r)).all()
        dv = _dev(case)
        for relu in (0, 1, 2, 3):
            for gloss, got in ((1.0, _new_train(dv, n, rows, T, relu, HUBER, delta)),
                               (0.5, _new_fwd_bwd(dv, n, rows, T, relu, HUBER, delta, 0.5))):
                ref = readout_loss_np(*case, n, relu, gloss, rows, delta.astype(np.float64))
                what = f'T={T} form={form} relu={relu} gloss={gloss}'
                assert float(got[1]) == ref[1], what + ' loss'
                for name, g, x in zip(NAMES, got, ref):
                    if name != 'loss':
                        assert torch.equal(g.cpu(), torch.from_numpy(np.asarray(x).astype(np.float32)).reshape(g.shape)), f'{what} {name}'
    # one seed: column t's residual is mult[t] * delta[t]
    mult = np.array([1.0, -1.0, 3.0, 0.0] * 8)[:T]
    H = np.zeros((1, 128), np.float32)
    H[0, 5] = 1.0
    W = np.zeros((T, 128), np.float32)
    W[:, 5] = 4.0
    b = np.ones(T, np.float32)
    y = (5.0 - mult * delta).astype(np.float32)[None, :]
    w = np.full((1, T), 0.5)
    case = (H, W, b, np.zeros(1, np.int32), y, w)
    got = _new_train(_dev(case), 1, 1, T, 0, HUBER, delta)
    scale = np.float32(0.5 / T)
    want = np.float32(2.0) * np.clip(mult, -1, 1).astype(np.float32) * delta * scale
    assert torch.equal(got[4].cpu(), torch.from_numpy(want.astype(np.float32)))
    rho = np.where(np.abs(mult) <= 1, (mult * delta) ** 2, delta.astype(np.float64) * (2 * np.abs(mult * delta) - delta))
    assert float(got[1]) == float((0.5 * rho).sum() / T)
    assert rho[0] == float(delta[0]) ** 2


@pytest.mark.parametrize('T', (2, 3, 32))
def test_mixed_columns_keep_the_mse_columns_bits(T):
    """8. delta = (+inf, small, +inf, ...): the +inf columns' dW[t] and db[t] carry the bits of the MSE run, column 1's do not; the
    NaN / +-Inf labels under the zero weights reach nothing."""
    delta = np.full(T, INF, np.float32)
    delta[1] = 0.05
    keep = torch.arange(T) != 1
    for n, rows in ((5, 6), (9, 16)) + (((513, 520),) if T == 32 else ()):
        for seed in range(13 * n + T, 13 * n + T + 16):     # (the first case whose column 1 has an observed residual past the knee)
            case = make_case_w(n, T, rows, seed=seed)
            z, _, r, _, _ = residuals_np(*case, n, 1)
            if ((np.abs(r[:, 1]) > 0.05) & (z[:, 1] > 0)).any():
                break
        assert ((np.abs(r[:, 1]) > 0.05) & (z[:, 1] > 0)).any()
        assert not np.isfinite(case[4][case[5] == 0]).any()
        dv = _dev(case)
        for relu in (1, 3):
            for gloss, run, anchor in (
                    (1.0, _new_train(dv, n, rows, T, relu, HUBER, delta), _old(dv, n, rows, T, relu, 'nt', 'train')),
                    (0.7, _new_fwd_bwd(dv, n, rows, T, relu, HUBER, delta, 0.7), _old(dv, n, rows, T, relu, 'nt', 'fwd_bwd', 0.7))):
                for t in run:
                    assert bool(torch.isfinite(t).all())
                assert torch.equal(run[0], anchor[0])
                assert torch.equal(run[3].cpu()[keep], anchor[3].cpu()[keep]) and torch.equal(run[4].cpu()[keep], anchor[4].cpu()[keep])
                assert not torch.equal(run[3][1], anchor[3][1]) and float(run[1]) < float(anchor[1])
                _check(run, readout_loss_np(*case, n, relu, gloss, rows, delta.astype(np.float64)), n, T,
                       f'T={T} n={n} relu={relu} gloss={gloss} mixed')


@pytest.mark.parametrize('T', (1, 3))
def test_one_huge_label_cannot_move_a_gradient_past_the_bound(T):
    """9. One planted label of 1e6.  H is one-hot with a column per seed, so dW[t][column of seed i] IS d pred[i][t]:
    max |d pred| <= 2 delta max(w) / N up to one ulp (two roundings of half an ulp: the scale, the product), every output finite;
    the MSE on the same batch moves it by thousands of times more."""
    n, rows = 9, 12
    delta = np.array([0.5, 1.0, 2.0], np.float32)[:T]
    for form in FORMS:
        H, W, b, n_id, y, w = _case(form, n, T, rows, seed=5)
        H = np.zeros_like(H)
        H[np.arange(rows), np.arange(rows) * 3] = 1.0
        w = np.where(w == 0, 0.75, w)
        y = np.where(np.isfinite(y), y, 1.0).astype(np.float32)
        y[n_id[3], T - 1] = 1e6
        dv = _dev((H, W, b, n_id, y, w))
        N = n * T
        bound = 2.0 * delta.astype(np.float64) * float(w.max()) / N * (1 + 2.0 ** -23)
        for got in (_new_train(dv, n, rows, T, 0, HUBER, delta), _new_fwd_bwd(dv, n, rows, T, 0, HUBER, delta, 1.0)):
            for t in got:
                assert bool(torch.isfinite(t).all())
            dpred = got[3].cpu().double().numpy()[:, np.arange(n) * 3]                      # [T, n]
            assert (np.abs(dpred) <= bound[:, None]).all() and np.abs(dpred).max() > 0
            assert abs(dpred[T - 1, 3]) >= 2.0 * float(delta[T - 1]) * float(w.min()) / N * (1 - 2.0 ** -22)   # (the outlier sits AT the bound)
        mse = _new_train(dv, n, rows, T, 0, MSE, None)
        assert float(mse[3].abs().max()) > 1e3 * bound.max()


def test_two_runs_are_bit_identical_and_train_is_forward_plus_backward_at_one():
    """10. No float atomics, a fixed fold order: T = 32 at n = 513 and T = 1, twice.  Forward + backward at grad_loss = 1 equals train
    where the existing entries have that property: the single-column node (its backward starts from the very float32 prediction the
    train form holds; the multi-trait backward starts from the ROUNDED float64 prediction, so there the property does not exist)."""
    for T, n, rows, form in ((32, 513, 520, 'nt'), (32, 513, 520, 'n'), (1, 9, 16, 'n'), (3, 9, 10, 'nt')):
        case = _case(form, n, T, rows, seed=3)
        delta = np.linspace(0.3, 1.7, T).astype(np.float32)
        dv = _dev(case)
        _same(_new_train(dv, n, rows, T, 3, HUBER, delta), _new_train(dv, n, rows, T, 3, HUBER, delta), f'T={T} train twice')
        _same(_new_fwd_bwd(dv, n, rows, T, 3, HUBER, delta, 0.7), _new_fwd_bwd(dv, n, rows, T, 3, HUBER, delta, 0.7), f'T={T} fwd+bwd twice')
    for n, rows in _shapes(1):
        dv = _dev(_case('n', n, 1, rows, seed=n))
        for relu in (0, 1, 2, 3):
            _same(_old(dv, n, rows, 1, relu, 'n', 'fwd_bwd', 1.0), _old(dv, n, rows, 1, relu, 'n', 'train'), 'the existing entries')
            d = np.array([0.6], np.float32)
            _same(_new_fwd_bwd(dv, n, rows, 1, relu, HUBER, d, 1.0), _new_train(dv, n, rows, 1, relu, HUBER, d), f'n={n} relu={relu}')


def test_bad_records_are_refused_before_any_launch():
    """11. A NaN, zero, negative or -inf delta, T = 0 / 33, an unknown kind: KGW_E_RANGE; fold_out with T > 1: KGW_E_UNSUPPORTED --
    from all three entry points where they apply, the outputs and workspaces, pre-filled with zeros, still all zero."""
    from kgwas_amd import _lib
    L = _lib.lib()
    n, rows = 5, 8
    dv = _dev(make_case_w(n, 32, rows, seed=1, poison=False))                   # (sized for 32 columns)
    calls = (L.kgw_readout_loss_fwd, L.kgw_readout_loss_bwd, L.kgw_readout_loss_train)
    g = torch.ones((), dtype=torch.float64, device='cuda')

    def refused(expect, T, kind, delta, fns=calls, **extra):
        out, work = _outputs(n, rows, 33, 0.0), _work(n, rows, 33, 0.0)
        a = _record(dv, n, rows, T, 1, kind, None, out, work, pred_in=out[0].data_ptr(), grad_loss=g.data_ptr(), **extra)
        for t in range(32):
            a.delta[t] = float(delta[t])
        for fn in fns:
            assert fn(C.byref(a), _lib.stream_ptr()) == expect, (fn.__name__, T, kind, list(delta[:4]))
        torch.cuda.synchronize()
        for t in out + work:
            assert not t.ne(0).any(), (T, kind, 'an output was written')

    ones = np.ones(32, np.float32)
    for T in (1, 2, 32):
        for v in (float('nan'), 0.0, -1.0, -INF):
            for t in {0, T - 1}:
                bad = ones.copy()
                bad[t] = v
                refused(KGW_E_RANGE, T, HUBER, bad)
    for T in (0, 33):
        refused(KGW_E_RANGE, T, HUBER, ones)
        refused(KGW_E_RANGE, T, MSE, ones)
    for kind in (2, -1, 7):
        refused(KGW_E_RANGE, 3, kind, ones)
    f = _lib.KgwReadoutFold()
    for kind in (MSE, HUBER):
        refused(KGW_E_UNSUPPORTED, 2, kind, ones, fns=(L.kgw_readout_loss_train,), fold_out=C.pointer(f))
    assert f.nb == 0 and f.n == 0
    # (a bad delta beyond the first T is not read)
    bad = ones.copy()
    bad[3:] = float('nan')
    out, work = _outputs(n, rows, 3, float('nan')), _work(n, rows, 3)
    a = _record([dv[0], dv[1][:3].contiguous(), dv[2][:3].contiguous(), dv[3], dv[4][:, :3].contiguous(), dv[5][:, :3].contiguous()],
                n, rows, 3, 1, HUBER, None, out, work)
    for t in range(32):
        a.delta[t] = float(bad[t])
    assert L.kgw_readout_loss_train(C.byref(a), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in out)
