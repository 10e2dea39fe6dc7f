"""-m gpu: per-trait LD weights and unobserved (SNP, trait) pairs in the multi-trait read-out -- kgw_readout_wmse_mtw_* against the
shared-weight kernels (equal columns: bit for bit) and against the float64 twin of tests/multitrait_w_ref.py (random weights, NaN /
+-Inf under every zero weight), up to KGWAS.train."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.helpers import assert_close, batch_cpu, grads_by_name, oracle_from_product
from tests.multitrait_ref import make_case
from tests.multitrait_w_ref import make_case_w, readout_wmse_w_np

pytestmark = pytest.mark.gpu

RT, AT = 1e-4, 1e-5            # the project's fp32 rule: |a - b| <= 1e-5 + 1e-4 |b| + 1e-5 max|b| (helpers.assert_close)
KGW_E_RANGE = -2
NS, TS = (1, 3, 4, 5, 9), (1, 2, 3, 31, 32)
NAMES = ('pred', 'loss', 'dH', 'dW', 'db')
SIZES, COVER = [5000, 20000, 387113], [1.0, 0.6, 0.3]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _dev(case):
    return [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in case]


def _shapes(T):
    """(n, rows) of one column count: n at 1, below / at / above one block of four seeds, three blocks; rows = n, n + 1 and n + 7
    (blocks without seeds); at T = 32 also 129 blocks (the fold's groups of 7 and 28 blocks crossed, with a tail)."""
    out = [(n, n + extra) for n in NS for extra in (0, 1, 7)]
    return out + [(513, 520)] if T == 32 else out


def _train(lib, fam, dv, n, rows, T, relu):
    """The unit-gradient form of family ``fam`` ('mt': w [N]; 'mtw': w [N, T]); outputs start as NaN so that an unwritten element
    shows."""
    from kgwas_amd import _lib
    H, W, b, n_id, y, w = dv
    nan = float('nan')
    pred = torch.full((n, T), nan, device='cuda')
    loss = torch.full((), nan, dtype=torch.float64, device='cuda')
    dH = torch.full((rows, 128), nan, device='cuda')
    dW, db = torch.full((T, 128), nan, device='cuda'), torch.full((T,), nan, device='cuda')
    terms = torch.empty(n, dtype=torch.float64, device='cuda')
    part = torch.empty(((rows + 3) // 4) * T * 129, device='cuda')
    rc = getattr(lib, f'kgw_readout_wmse_{fam}_train')(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, rows, T, relu, _p(pred),
                                                         _p(loss), _p(dH), _p(dW), _p(db), _p(terms), _p(part), _lib.stream_ptr())
    assert rc == 0
    return pred, loss, dH, dW, db


def _fwd_bwd(lib, fam, dv, n, rows, T, relu, gloss):
    from kgwas_amd import _lib
    H, W, b, n_id, y, w = dv
    nan = float('nan')
    pred = torch.full((n, T), nan, device='cuda')
    loss = torch.full((), nan, dtype=torch.float64, device='cuda')
    terms = torch.empty(n, dtype=torch.float64, device='cuda')
    rc = getattr(lib, f'kgw_readout_wmse_{fam}_fwd')(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, T, relu & 1, _p(pred), _p(loss),
                                                       _p(terms), _lib.stream_ptr())
    assert rc == 0
    g = torch.tensor(gloss, dtype=torch.float64, device='cuda')
    dH = torch.full((rows, 128), nan, device='cuda')
    dW, db = torch.full((T, 128), nan, device='cuda'), torch.full((T,), nan, device='cuda')
    part = torch.empty(((rows + 3) // 4) * T * 129, device='cuda')
    rc = getattr(lib, f'kgw_readout_wmse_{fam}_bwd')(_p(H), _p(W), _p(pred), _p(n_id), _p(y), _p(w), n, rows, T, relu, _p(g), _p(dH),
                                                       _p(dW), _p(db), _p(part), _lib.stream_ptr())
    assert rc == 0
    return pred, loss, dH, dW, db


def _check(got, ref, n, what):
    pred, loss, dH, dW, db = got
    pred_r, loss_r, dH_r, dW_r, db_r = ref
    for t, name in zip(got, NAMES):
        assert bool(torch.isfinite(t).all()), f'{what}: {name} is not finite'
    assert_close(pred, torch.from_numpy(pred_r), RT, AT, what + ' pred')
    lv = float(loss)
    assert abs(lv - loss_r) <= 1e-6 * abs(loss_r), (what, lv, loss_r)           # float64-accumulated
    assert_close(dH, torch.from_numpy(dH_r), RT, AT, what + ' dH')
    assert not dH[n:].ne(0).any(), what + ': dH beyond the seeds must be exactly zero'
    assert_close(dW, torch.from_numpy(dW_r), RT, AT, what + ' dW')
    assert_close(db, torch.from_numpy(db_r), RT, AT, what + ' db')


@pytest.mark.parametrize('T', TS)
def test_equal_columns_equal_the_shared_weight_kernels(T):
    """1. w[g][t] = w0[g], finite labels: all three entry points give the bits of kgw_readout_wmse_mt_* (one node of every case
    weighs 0 -- there the shared-weight kernel multiplies a finite residual by 0, this one never forms it: both exact zeros)."""
    from kgwas_amd import _lib
    lib = _lib.lib()
    for n, rows in _shapes(T):
        H, Wl, b, n_id, y, w0 = make_case(n, T, rows, seed=7 * n + T)
        dv = _dev((H, Wl, b, n_id, y, w0))
        dvw = dv[:5] + [dv[5][:, None].repeat(1, T).contiguous()]
        for relu in (0, 1, 2, 3):
            what = f'T={T} n={n} rows={rows} relu={relu}'
            for name, a, c in zip(NAMES, _train(lib, 'mtw', dvw, n, rows, T, relu), _train(lib, 'mt', dv, n, rows, T, relu)):
                assert torch.equal(a, c), f'{what} train {name}'
            for name, a, c in zip(NAMES, _fwd_bwd(lib, 'mtw', dvw, n, rows, T, relu, 0.7), _fwd_bwd(lib, 'mt', dv, n, rows, T, relu, 0.7)):
                assert torch.equal(a, c), f'{what} fwd+bwd {name}'


@pytest.mark.parametrize('T', TS)
def test_random_weights_with_unobserved_entries_match_the_twin(T):
    """2. Every weight 0 with probability 1/2, the label NaN / +Inf / -Inf at exactly those entries: every output finite and the
    twin's, in the two-launch train form and in forward + backward with grad_loss = 0.7."""
    from kgwas_amd import _lib
    lib = _lib.lib()
    for n, rows in _shapes(T):
        case = make_case_w(n, T, rows, seed=11 * n + T)
        y, w = case[4], case[5]
        assert not np.isfinite(y[w == 0]).any() and np.isfinite(y[w != 0]).all()
        dv = _dev(case)
        for relu in (0, 1, 2, 3):
            what = f'T={T} n={n} rows={rows} relu={relu}'
            _check(_train(lib, 'mtw', dv, n, rows, T, relu), readout_wmse_w_np(*case, n, relu, 1.0, rows), n, what + ' train')
            _check(_fwd_bwd(lib, 'mtw', dv, n, rows, T, relu, 0.7), readout_wmse_w_np(*case, n, relu, 0.7, rows), n, what + ' fwd+bwd')


def _poison(y, w):
    y = y.copy()
    y[w == 0] = np.nan
    return y


def test_zero_column_zero_row_and_all_zero():
    """3. - 5. A column of zeros: dW[t], db[t] exactly 0.  A row of zeros: dH[i] exactly 0 for every seed of that node.  All zeros:
    loss exactly 0.0, every gradient exactly 0, pred still written and finite (the twin's)."""
    from kgwas_amd import _lib
    lib = _lib.lib()
    for T, n, rows in ((3, 9, 10), (32, 9, 16), (31, 5, 5)):
        H, Wl, b, n_id, y, w = make_case_w(n, T, rows, seed=5 * T + n, p_zero=0.0, poison=False)
        assert w.all()
        t0, g0 = T - 1, int(n_id[1])
        wc, wr = w.copy(), w.copy()
        wc[:, t0] = 0.0
        wr[g0, :] = 0.0
        for relu in (1, 3):
            case = (H, Wl, b, n_id, _poison(y, wc), wc)
            got = _train(lib, 'mtw', _dev(case), n, rows, T, relu)
            _check(got, readout_wmse_w_np(*case, n, relu, 1.0, rows), n, f'T={T} zero column')
            assert not got[3][t0].ne(0).any() and float(got[4][t0]) == 0.0 and bool(got[3][:t0].ne(0).any())
            got = _fwd_bwd(lib, 'mtw', _dev(case), n, rows, T, relu, 0.7)
            assert not got[3][t0].ne(0).any() and float(got[4][t0]) == 0.0
            case = (H, Wl, b, n_id, _poison(y, wr), wr)
            seeds = torch.from_numpy(np.nonzero(n_id[:n] == g0)[0]).cuda()
            assert len(seeds) >= 2                               # (make_case repeats the id of seed 1 at seed 2)
            for got in (_train(lib, 'mtw', _dev(case), n, rows, T, relu), _fwd_bwd(lib, 'mtw', _dev(case), n, rows, T, relu, 0.7)):
                assert not got[2][seeds].ne(0).any() and bool(torch.isfinite(got[2]).all()) and bool(got[2][:n].ne(0).any())
            w0 = np.zeros_like(w)
            case = (H, Wl, b, n_id, _poison(y, w0), w0)
            ref = readout_wmse_w_np(*case, n, relu, 1.0, rows)
            for got in (_train(lib, 'mtw', _dev(case), n, rows, T, relu), _fwd_bwd(lib, 'mtw', _dev(case), n, rows, T, relu, 0.7)):
                assert float(got[1]) == 0.0 and not np.signbit(float(got[1]))
                assert bool(torch.isfinite(got[0]).all())
                assert_close(got[0], torch.from_numpy(ref[0]), RT, AT, 'pred with nothing observed')
                assert bool(got[0].ne(0).any())
                for t in got[2:]:
                    assert not t.ne(0).any()


def test_two_runs_are_bit_identical():
    """6. T = 32, n = 513: no float atomics, a fixed fold order."""
    from kgwas_amd import _lib
    lib = _lib.lib()
    dv = _dev(make_case_w(513, 32, 520, seed=3))
    a, b = _train(lib, 'mtw', dv, 513, 520, 32, 3), _train(lib, 'mtw', dv, 513, 520, 32, 3)
    for x, y, what in zip(a, b, NAMES):
        assert torch.equal(x, y), what


def test_column_counts_out_of_range_are_refused_before_any_launch():
    """7. T = 0 and T = 33: KGW_E_RANGE from the three entry points, outputs untouched."""
    from kgwas_amd import _lib
    lib = _lib.lib()
    n, rows = 5, 8
    H, W, b, n_id, y, w = _dev(make_case_w(n, 32, rows, seed=1, poison=False))               # (sized for 32 columns)
    for T in (0, 33):
        pred, dH = torch.zeros(n, 33, device='cuda'), torch.zeros(rows, 128, device='cuda')
        dW, db = torch.zeros(33, 128, device='cuda'), torch.zeros(33, device='cuda')
        loss = torch.zeros((), dtype=torch.float64, device='cuda')
        terms = torch.zeros(n, dtype=torch.float64, device='cuda')
        part = torch.zeros(2 * 33 * 129, device='cuda')
        g = torch.ones((), dtype=torch.float64, device='cuda')
        assert lib.kgw_readout_wmse_mtw_train(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, rows, T, 1, _p(pred), _p(loss), _p(dH),
                                              _p(dW), _p(db), _p(terms), _p(part), _lib.stream_ptr()) == KGW_E_RANGE
        assert lib.kgw_readout_wmse_mtw_fwd(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, T, 1, _p(pred), _p(loss), _p(terms),
                                            _lib.stream_ptr()) == KGW_E_RANGE
        assert lib.kgw_readout_wmse_mtw_bwd(_p(H), _p(W), _p(pred), _p(n_id), _p(y), _p(w), n, rows, T, 1, _p(g), _p(dH), _p(dW),
                                            _p(db), _p(part), _lib.stream_ptr()) == KGW_E_RANGE
        torch.cuda.synchronize()
        for t in (pred, loss, dH, dW, db, terms, part):
            assert not t.ne(0).any(), f'T={T}: an output was written'


@pytest.fixture(scope='module')
def small_kg3w(tmp_path_factory):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.01, seed=1, feat_dims={'Gene': 96}, data_path=str(tmp_path_factory.mktemp('mtw_small')),
                                     n_traits=3, trait_sample_sizes=SIZES, trait_coverage=COVER)


def test_model_parity_with_per_trait_weights(small_kg3w):
    """8. forward_loss with the [N, 3] weight against oracle/gat_oracle.py: its float64 predictions pushed through
    (w * (pred - y)^2).mean(), autograd for its gradients; tolerances of test_model_parity_with_three_traits."""
    from kgwas_amd import ops
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    data = small_kg3w
    run = KGWAS(data, device='cuda:0', seed=11)
    run.initialize_model(out_channels=3)
    with torch.no_grad():
        for pack in list(run.model.live_packs) + list(run.model.dead_packs):
            pack.bias.normal_(0, 0.1)
    model = run.model.train()
    ids = np.asarray(data.train_input_nodes[1][:64])
    batch = next(iter(NeighborLoader(data.data, [-1, -1], ('SNP', ids), batch_size=64, device='cuda:0')))
    ld_w = run._ld_weight_vector()
    assert tuple(ld_w.shape) == (data.data['SNP'].x.shape[0], 3)
    n_id = batch.n_id('SNP')
    seeds = n_id[:64].long().cpu()
    w_seeds = ld_w.cpu()[seeds]
    assert bool((w_seeds == 0).any()) and bool((w_seeds[:, 1:] != 0).any())        # the batch holds unobserved pairs
    before = dict(ops.ROUTES)
    loss, pred = model.forward_loss(batch.x_dict, batch.edge_index_dict, 64, n_id, batch.dg.y['SNP'], ld_w, unit_grad=True)
    assert ops.ROUTES.get('kgw_readout_wmse_mtw_train', 0) == before.get('kgw_readout_wmse_mtw_train', 0) + 1
    for name in ('kgw_readout_wmse_mt_train', 'kgw_readout_wmse_mt_fwd'):
        assert ops.ROUTES.get(name, 0) == before.get(name, 0), name
    assert pred.shape == (64, 3)
    loss.backward(gradient=ops.unit_gradient(loss.device))
    oracle = oracle_from_product(model)
    x, ei = batch_cpu(batch)
    out_o = oracle(x, ei, 64)
    y = data.data['SNP'].y.double()[seeds]
    loss_o = (w_seeds * (out_o - y) ** 2).mean()
    loss_o.backward()
    assert_close(pred, out_o.detach(), 1e-4, 1e-5, 'pred')
    assert_close(loss.detach(), loss_o.detach(), 1e-4, 1e-5, 'loss')
    go = grads_by_name(oracle)
    n_live = 0
    for name, g in grads_by_name(model).items():
        ref = go[name]
        if g is None:
            assert ref is None or float(ref.abs().max()) == 0.0, f'{name}: product has no grad, oracle has'
            continue
        n_live += 1
        assert_close(g, ref, 1e-4, max(1e-5, 1e-4 * float(ref.abs().max())), f'grad {name}')
    assert n_live > 10
    assert tuple(model.lin.weight.grad.shape) == (3, 128) and float(model.lin.weight.grad.abs().max()) > 0


class _Log:
    def __init__(self):
        self.losses = []

    def log(self, d):
        if 'training_loss' in d:
            self.losses.append(d['training_loss'])


def test_training_end_to_end_captured_and_eager(small_kg3w):
    """9. + 10. KGWAS.train(batch_size=64, epoch=1) with per-trait weights, captured and eager: the same loss at every step (the
    first three included; tolerance of the shared-weight test); per-trait validation metrics equal a recomputation over the pairs
    each trait observes; one prediction table per trait with that trait's rows; trait_pred keeps every pair."""
    import pandas as pd
    from kgwas_amd import ops
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.utils import compute_metrics, evaluate_minibatch_clean
    data = small_kg3w
    losses, sd0 = {}, None
    for use_graph in (True, False):
        run = KGWAS(data, device='cuda:0', seed=31)
        run.initialize_model(out_channels=3)
        if sd0 is None:
            sd0 = copy.deepcopy(run.model.state_dict())
        else:
            run.model.load_state_dict(sd0)
        run.wandb = _Log()
        name = 'mtw' + str(use_graph)
        before = dict(ops.ROUTES)
        run.train(batch_size=64, epoch=1, save_best_model=False, save_name=name, use_graph=use_graph)
        assert ops.ROUTES.get('kgw_readout_wmse_mtw_train', 0) > before.get('kgw_readout_wmse_mtw_train', 0)
        assert ops.ROUTES.get('kgw_readout_wmse_mt_train', 0) == before.get('kgw_readout_wmse_mt_train', 0)
        losses[use_graph] = run.wandb.losses
        assert all(np.isfinite(v) for v in run.wandb.losses)
        # the validation metrics are those of the model after the one epoch: evaluate it again and mask by hand
        res = evaluate_minibatch_clean(run.val_loader, run.model, run.device)
        val_ids = np.asarray(data.val_input_nodes[1])[:len(res['pred'])]
        row_of = np.full(data.data['SNP'].x.shape[0], -1)
        row_of[data.all_ids] = np.arange(len(data.all_ids))
        obs = data.trait_observed[row_of[val_ids]]
        truth = data.data['SNP'].y.numpy()[val_ids]
        per = run.val_metrics['per_trait']
        assert len(per) == 3
        for t in range(3):
            o = obs[:, t]
            assert 2 <= o.sum() and (t == 0) == bool(o.all())
            ref = compute_metrics({'pred': res['pred'][o, t], 'truth': truth[o, t]})
            assert np.isclose(per[t]['mse'], ref['mse'], rtol=1e-6, atol=0) and np.isclose(per[t]['pearsonr'], ref['pearsonr'], rtol=1e-6, atol=1e-9)
        assert np.isclose(run.val_metrics['pearsonr'], np.mean([m['pearsonr'] for m in per]))
        assert len(run.test_metrics['per_trait']) == 3 and all(np.isfinite(m['mse']) for m in run.test_metrics['per_trait'])
        out_dir = os.path.join(data.data_path, 'model_pred', 'new_experiments')
        assert run.trait_pred.shape == (len(data.all_ids), 3) and np.isfinite(run.trait_pred).all()
        for t in range(3):
            tab = pd.read_csv(os.path.join(out_dir, f'{name}_trait{t}_pred.csv'), sep='\t')
            assert len(tab) == int(data.trait_observed[:, t].sum()) == len(run.kgwas_res[t])
            assert np.allclose(tab['pred'].values, run.trait_pred[data.trait_observed[:, t], t], rtol=1e-5, atol=1e-6)
            assert 'KGWAS_P' in run.kgwas_res[t].columns
    n = len(losses[True])
    assert n == len(losses[False]) and n >= 3
    for i in range(n):
        assert_close(torch.tensor(losses[True][i]), torch.tensor(losses[False][i]), 1e-5, 1e-7, f'loss step {i}')
