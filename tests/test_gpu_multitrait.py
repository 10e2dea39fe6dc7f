"""-m gpu: multi-trait training -- T label columns read out of one shared trunk by kgw_readout_wmse_mt_* -- from the kernels
(against the float64 twin of tests/multitrait_ref.py) up to KGWAS.train."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.helpers import assert_close, batch_cpu, grads_by_name, oracle_from_product
from tests.multitrait_ref import make_case, readout_wmse_np

pytestmark = pytest.mark.gpu

RT, AT = 1e-4, 1e-5            # the project's fp32 rule: |a - b| <= 1e-5 + 1e-4 |b| + 1e-5 max|b| (helpers.assert_close)
KGW_E_RANGE = -2


def _p(t):
    return C.c_void_p(t.data_ptr())


def _dev(case):
    H, W, b, n_id, y, w = case
    return [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (H, W, b, n_id, y, w)]


def _train(lib, dv, n, rows, T, relu, entry='kgw_readout_wmse_mt_train', poison=True):
    """One call of the unit-gradient form; outputs start as NaN so that an unwritten element shows."""
    from kgwas_amd import _lib
    H, W, b, n_id, y, w = dv
    fill = float('nan') if poison else 0.0
    pred = torch.full((n, T), fill, device='cuda')
    loss = torch.full((), fill, dtype=torch.float64, device='cuda')
    dH = torch.full((rows, 128), fill, device='cuda')
    dW, db = torch.full((T, 128), fill, device='cuda'), torch.full((T,), fill, device='cuda')
    terms = torch.empty(n, dtype=torch.float64, device='cuda')
    part = torch.empty(((rows + 3) // 4) * T * 129, device='cuda')
    if entry == 'kgw_readout_wmse_mt_train':
        rc = lib.kgw_readout_wmse_mt_train(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, rows, T, relu, _p(pred), _p(loss), _p(dH),
                                           _p(dW), _p(db), _p(terms), _p(part), _lib.stream_ptr())
    else:               # the single-column call (T == 1)
        rc = lib.kgw_readout_wmse_train(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, rows, relu, _p(pred), _p(loss), _p(dH),
                                        _p(dW), _p(db), _p(terms), _p(part), _lib.stream_ptr())
    return rc, pred, loss, dH, dW, db


def _fwd_bwd(lib, dv, n, rows, T, relu, gloss):
    from kgwas_amd import _lib
    H, W, b, n_id, y, w = dv
    pred = torch.full((n, T), float('nan'), device='cuda')
    loss = torch.full((), float('nan'), dtype=torch.float64, device='cuda')
    terms = torch.empty(n, dtype=torch.float64, device='cuda')
    rc = lib.kgw_readout_wmse_mt_fwd(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, T, relu & 1, _p(pred), _p(loss), _p(terms),
                                     _lib.stream_ptr())
    assert rc == 0
    g = torch.tensor(gloss, dtype=torch.float64, device='cuda')
    dH = torch.full((rows, 128), float('nan'), device='cuda')
    dW, db = torch.full((T, 128), float('nan'), device='cuda'), torch.full((T,), float('nan'), device='cuda')
    part = torch.empty(((rows + 3) // 4) * T * 129, device='cuda')
    rc = lib.kgw_readout_wmse_mt_bwd(_p(H), _p(W), _p(pred), _p(n_id), _p(y), _p(w), n, rows, T, relu, _p(g), _p(dH), _p(dW), _p(db),
                                     _p(part), _lib.stream_ptr())
    assert rc == 0
    return pred, loss, dH, dW, db


def _check(got, ref, n, what):
    pred, loss, dH, dW, db = got
    pred_r, loss_r, dH_r, dW_r, db_r = ref
    assert_close(pred, torch.from_numpy(pred_r), RT, AT, what + ' pred')
    lv = float(loss)
    print(f'{what}: loss {lv:.12e} twin {loss_r:.12e} rel {abs(lv - loss_r) / max(abs(loss_r), 1e-300):.2e}')
    assert abs(lv - loss_r) <= 1e-6 * abs(loss_r), (what, lv, loss_r)           # float64-accumulated
    assert_close(dH, torch.from_numpy(dH_r), RT, AT, what + ' dH')
    assert not dH[n:].ne(0).any(), what + ': dH beyond the seeds must be exactly zero'
    assert_close(dW, torch.from_numpy(dW_r), RT, AT, what + ' dW')
    assert_close(db, torch.from_numpy(db_r), RT, AT, what + ' db')


@pytest.mark.parametrize('T', [1, 2, 3, 8, 31, 32])
def test_kernels_match_the_float64_twin(T):
    """1. Every form of the node (unit-gradient two-launch; forward + general backward with grad_loss = 0.7) against the twin:
    n at 1, below / at / above one block of four seeds, 16 blocks, 129 blocks (the fold's groups of 7 and 28 blocks crossed, with a
    tail); rows = n, n + 1 (same last block or one more) and n + 7 (blocks without seeds); all four relu values; repeated ids; a
    seed whose node weighs 0."""
    from kgwas_amd import _lib
    lib = _lib.lib()
    for n in (1, 3, 4, 5, 64, 513):
        for extra in (0, 1, 7):
            rows = n + extra
            case = make_case(n, T, rows, seed=7 * n + T)
            dv = _dev(case)
            for relu in (0, 1, 2, 3):
                what = f'T={T} n={n} rows={rows} relu={relu}'
                ref = readout_wmse_np(*case, n, relu, 1.0, rows)
                rc, *got = _train(lib, dv, n, rows, T, relu)
                assert rc == 0
                _check(got, ref, n, what + ' train')
                ref = readout_wmse_np(*case, n, relu, 0.7, rows)
                _check(_fwd_bwd(lib, dv, n, rows, T, relu, 0.7), ref, n, what + ' fwd+bwd')


def test_read_out_alone_matches_the_twin():
    """kgw_readout_mt_pred / _pred_bwd (HeteroGNN.forward's read-out): H W^T + b and the three products of its backward."""
    from kgwas_amd import ops
    for T, n in ((2, 1), (3, 5), (32, 130)):
        H, W, b, _, _, _ = make_case(n, T, n, seed=T + n)
        Ht, Wt, bt = [torch.from_numpy(v).cuda().requires_grad_() for v in (H, W, b)]
        out = ops.readout_linear(Ht, Wt, bt)
        G = torch.from_numpy(np.random.default_rng(n).standard_normal((n, T)).astype(np.float32)).cuda()
        out.backward(G)
        H6, W6, G6 = H.astype(np.float64), W.astype(np.float64), G.cpu().numpy().astype(np.float64)
        assert_close(out, torch.from_numpy(H6 @ W6.T + b), RT, AT, 'read-out')
        assert_close(Ht.grad, torch.from_numpy(G6 @ W6), RT, AT, 'read-out dH')
        assert_close(Wt.grad, torch.from_numpy(G6.T @ H6), RT, AT, 'read-out dW')
        assert_close(bt.grad, torch.from_numpy(G6.sum(0)), RT, AT, 'read-out db')


def test_one_column_through_the_new_entry_points_equals_the_single_column_call():
    """2. T = 1: kgw_readout_wmse_mt_train against kgw_readout_wmse_train on the same inputs (fp32 rule; whether the two are also
    bit-equal is printed, not required)."""
    from kgwas_amd import _lib
    lib = _lib.lib()
    for n, rows, relu in ((1, 1, 1), (5, 12, 3), (64, 65, 0), (513, 520, 3)):
        case = make_case(n, 1, rows, seed=n)
        dv = _dev(case)
        dv1 = list(dv)
        dv1[4] = dv[4].reshape(-1).contiguous()          # y [N]
        rc, *new = _train(lib, dv, n, rows, 1, relu)
        assert rc == 0
        rc, *old = _train(lib, dv1, n, rows, 1, relu, entry='kgw_readout_wmse_train')
        assert rc == 0
        bits = []
        for a, b, what in zip(new, old, ('pred', 'loss', 'dH', 'dW', 'db')):
            assert_close(a, b, RT, AT, f'n={n} {what}')
            bits.append(bool(torch.equal(a, b)))
        print(f'T=1 n={n} rows={rows} relu={relu}: bit-equal (pred, loss, dH, dW, db) = {bits}')


def test_two_runs_are_bit_identical():
    """3. T = 8, n = 513: no float atomics, a fixed fold order."""
    from kgwas_amd import _lib
    lib = _lib.lib()
    dv = _dev(make_case(513, 8, 520, seed=3))
    rc, *a = _train(lib, dv, 513, 520, 8, 3)
    rc2, *b = _train(lib, dv, 513, 520, 8, 3)
    assert rc == 0 and rc2 == 0
    for x, y, what in zip(a, b, ('pred', 'loss', 'dH', 'dW', 'db')):
        assert torch.equal(x, y), what


def test_column_counts_out_of_range_are_refused_before_any_launch():
    """4. T = 0 and T = 33: KGW_E_RANGE from every entry point, outputs untouched."""
    from kgwas_amd import _lib
    lib = _lib.lib()
    n, rows = 5, 8
    dv = _dev(make_case(n, 32, rows, seed=1))
    H, W, b, n_id, y, w = dv               # (sized for 32 columns)
    for T in (0, 33):
        pred, dH = torch.zeros(n, 33, device='cuda'), torch.zeros(rows, 128, device='cuda')
        dW, db = torch.zeros(33, 128, device='cuda'), torch.zeros(33, device='cuda')
        loss = torch.zeros((), dtype=torch.float64, device='cuda')
        terms = torch.zeros(n, dtype=torch.float64, device='cuda')
        part = torch.zeros(2 * 33 * 129, device='cuda')
        rc = lib.kgw_readout_wmse_mt_train(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, rows, T, 1, _p(pred), _p(loss), _p(dH),
                                           _p(dW), _p(db), _p(terms), _p(part), _lib.stream_ptr())
        assert rc == KGW_E_RANGE
        torch.cuda.synchronize()
        for t in (pred, loss, dH, dW, db, terms, part):
            assert not t.ne(0).any(), f'T={T}: an output was written'
        sc = torch.zeros(4096, device='cuda')
        scd = torch.zeros(64, dtype=torch.float64, device='cuda')
        g = torch.ones((), dtype=torch.float64, device='cuda')
        assert lib.kgw_readout_wmse_mt_fwd(_p(H), _p(W), _p(b), _p(n_id), _p(y), _p(w), n, T, 1, _p(sc), _p(scd), _p(scd),
                                           _lib.stream_ptr()) == KGW_E_RANGE
        assert lib.kgw_readout_wmse_mt_bwd(_p(H), _p(W), _p(sc), _p(n_id), _p(y), _p(w), n, rows, T, 1, _p(g), _p(sc), _p(sc), _p(sc),
                                           _p(sc), _lib.stream_ptr()) == KGW_E_RANGE
        assert lib.kgw_readout_mt_pred(_p(H), _p(W), _p(b), n, T, 0, _p(sc), _lib.stream_ptr()) == KGW_E_RANGE
        assert lib.kgw_readout_mt_pred_bwd(_p(H), _p(W), _p(sc), n, rows, T, 0, _p(sc), _p(sc), _p(sc), _p(sc),
                                           _lib.stream_ptr()) == KGW_E_RANGE
        torch.cuda.synchronize()
        assert not sc.ne(0).any() and not scd.ne(0).any()


@pytest.fixture(scope='module')
def small_kg3(tmp_path_factory):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.01, seed=1, feat_dims={'Gene': 96}, data_path=str(tmp_path_factory.mktemp('mt_small')),
                                     n_traits=3)


def _run3(data, seed=11):
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(data, device='cuda:0', seed=seed)
    run.initialize_model(out_channels=3)
    with torch.no_grad():
        for pack in list(run.model.live_packs) + list(run.model.dead_packs):
            pack.bias.normal_(0, 0.1)
    return run


def _first_batch(data, bs=64):
    from kgwas_amd.sampler import NeighborLoader
    ids = np.asarray(data.train_input_nodes[1][:bs])
    return next(iter(NeighborLoader(data.data, [-1, -1], ('SNP', ids), batch_size=bs, device='cuda:0')))


def test_model_parity_with_three_traits(small_kg3):
    """5. forward_loss and every parameter gradient at T = 3 against oracle/gat_oracle.py with out_channels = 3; the oracle's loss
    helper is single-column, so the twin's loss is applied to its [n, 3] predictions and autograd gives its gradients.
    Tolerances of tests/test_gpu_model.py."""
    run = _run3(small_kg3)
    model = run.model.train()
    batch = _first_batch(small_kg3)
    ld_w = run._ld_weight_vector()
    n_id = batch.n_id('SNP')
    loss, pred = model.forward_loss(batch.x_dict, batch.edge_index_dict, 64, n_id, batch.dg.y['SNP'], ld_w, unit_grad=True)
    assert pred.shape == (64, 3)
    from kgwas_amd import ops
    loss.backward(gradient=ops.unit_gradient(loss.device))
    oracle = oracle_from_product(model)
    x, ei = batch_cpu(batch)
    out_o = oracle(x, ei, 64)
    assert out_o.shape == (64, 3)
    ids = n_id[:64].long().cpu()
    y = small_kg3.data['SNP'].y.double()[ids]
    loss_o = (ld_w.cpu()[ids][:, None] * (out_o - y) ** 2).mean()
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


def test_captured_and_eager_training_agree_with_three_traits(small_kg3):
    """6. KGWAS.train(batch_size=64, epoch=2) at T = 3, captured and eager: the same loss at every step (tests/test_gpu_fanout.py's
    tolerance for that comparison), per-trait metrics, one prediction table per trait."""
    from kgwas_amd.kgwas import KGWAS
    losses, sd0 = {}, None
    for use_graph in (True, False):
        run = KGWAS(small_kg3, device='cuda:0', seed=31)
        run.initialize_model(out_channels=3)
        if sd0 is None:
            sd0 = copy.deepcopy(run.model.state_dict())
        else:
            run.model.load_state_dict(sd0)
        run.wandb = _Log()
        name = 'mt' + str(use_graph)
        run.train(batch_size=64, epoch=2, save_best_model=False, save_name=name, use_graph=use_graph)
        losses[use_graph] = run.wandb.losses
        for m in (run.val_metrics, run.test_metrics):
            assert len(m['per_trait']) == 3 and all(np.isfinite(t['mse']) for t in m['per_trait'])
            assert np.isclose(m['pearsonr'], np.mean([t['pearsonr'] for t in m['per_trait']]))
        out_dir = os.path.join(small_kg3.data_path, 'model_pred', 'new_experiments')
        for t in range(3):
            assert os.path.exists(os.path.join(out_dir, f'{name}_trait{t}_pred.csv'))
        assert len(run.kgwas_res) == 3 and 'KGWAS_P' in run.kgwas_res[2].columns
    n = len(losses[True])
    assert n == len(losses[False]) and n >= 4
    for i in range(n):
        assert_close(torch.tensor(losses[True][i]), torch.tensor(losses[False][i]), 1e-5, 1e-7, f'loss step {i}')


def test_forward_with_three_traits_calls_no_library(small_kg3):
    """7. forward() at T = 3: nothing recorded by ops.LIBRARY_GEMM, and nothing refused with the strict switch on."""
    from kgwas_amd import ops
    run = _run3(small_kg3)
    batch = _first_batch(small_kg3)
    was = ops.LIBRARY_GEMM.strict
    ops.LIBRARY_GEMM.reset()
    try:
        for strict in (False, True):
            ops.LIBRARY_GEMM.strict = strict
            before = ops.ROUTES.get('kgw_readout_mt_pred', 0)
            with torch.no_grad():
                out = run.model.eval()(batch.x_dict, batch.edge_index_dict, 64)
            assert out.shape == (64, 3) and ops.ROUTES.get('kgw_readout_mt_pred', 0) == before + 1
            assert ops.LIBRARY_GEMM.calls == 0, ops.LIBRARY_GEMM.by_site
    finally:
        ops.LIBRARY_GEMM.strict = was
    # the prediction of forward() is the prediction of forward_loss()
    _, pred = run.model.forward_loss(batch.x_dict, batch.edge_index_dict, 64, batch.n_id('SNP'), batch.dg.y['SNP'],
                                     run._ld_weight_vector())
    assert_close(out, pred.detach(), 1e-6, 1e-7, 'forward vs forward_loss')


def test_traits_are_independent_given_the_trunk(small_kg3):
    """8. Trunk frozen: d W[t] of the T = 3 node is a third of d W of a single-column node on column t (same trunk, row t of the
    weight, column t of the labels) -- a transposed y or W would not survive this."""
    from kgwas_amd import ops
    run = _run3(small_kg3, seed=5)
    model = run.model.train()
    for name, p in model.named_parameters():
        p.requires_grad_(name.startswith('lin.'))
    batch = _first_batch(small_kg3)
    ld_w = run._ld_weight_vector()
    y3 = batch.dg.y['SNP']
    loss, _ = model.forward_loss(batch.x_dict, batch.edge_index_dict, 64, batch.n_id('SNP'), y3, ld_w, unit_grad=True)
    loss.backward(gradient=ops.unit_gradient(loss.device))
    dW3, db3 = model.lin.weight.grad.clone(), model.lin.bias.grad.clone()
    lin3 = model.lin
    for t in range(3):
        lin1 = torch.nn.Linear(128, 1).cuda()
        with torch.no_grad():
            lin1.weight.copy_(lin3.weight[t:t + 1]); lin1.bias.copy_(lin3.bias[t:t + 1])
        model.lin = lin1
        loss1, _ = model.forward_loss(batch.x_dict, batch.edge_index_dict, 64, batch.n_id('SNP'), y3[:, t].contiguous(), ld_w,
                                      unit_grad=True)
        loss1.backward(gradient=ops.unit_gradient(loss1.device))
        assert_close(dW3[t], lin1.weight.grad[0] / 3.0, RT, AT, f'dW[{t}]')
        assert_close(db3[t], lin1.bias.grad[0] / 3.0, RT, AT, f'db[{t}]')
    model.lin = lin3
