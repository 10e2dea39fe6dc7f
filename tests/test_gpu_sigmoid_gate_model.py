"""-m gpu: HeteroGNN(gat_sigmoid=True, gat_temperature=T) and the temperature alone, up to KGWAS.train(): against the float64 oracle
(tests/helpers.py:oracle_from_product with every GATConvOracle's ``sigmoid_gat`` / ``temperature`` set: tests/sigmoid_gate_ref.py)
on the small synthetic KG of the other model tests -- the seeds' predictions, the loss and every gradient under the reference's
names; the captured training step against eager steps; KGWAS.train + load_pretrained; the attention queries and the export.

Tolerances of tests/test_gpu_multihead_model.py: predictions and loss rtol 1e-4 / atol 1e-5, gradients rtol 1e-4 / atol
max(1e-5, 1e-4 max|ref|), plus assert_close's rel_to_max; captured against eager: losses rtol 1e-5 / atol 1e-7, relative update
difference below 5e-3; the export: test_gpu_model.py::test_network_weight_export_matches_reference_procedure's rtol 2e-4 / atol 1e-5."""
import os

import numpy as np
import pytest
import torch

from tests import sigmoid_gate_ref as R
from tests.helpers import assert_close, batch_cpu, grads_by_name, params_by_name

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
BS = 48
ATT_SCALE = 4.0


def _model(kg, cl=128, aggr='sum', seed=3, **kw):
    from kgwas_amd.model import HeteroGNN
    torch.manual_seed(seed)
    dims = (kg.snp_init_dim_size, kg.gene_init_dim_size, kg.go_init_dim_size)
    model = HeteroGNN(kg.data, cl, 1, 2, 'GAT', aggr, *dims, 1, **kw).cuda()
    with torch.no_grad():
        for pack in list(model.live_packs) + list(model.dead_packs):
            pack.bias[:, :cl].normal_(0, 0.1)
            pack.att_src.mul_(ATT_SCALE)   # (glorot-sized attention vectors give logits near 0: every gate 1/2, every softmax flat, and
            pack.att_dst.mul_(ATT_SCALE)   #  neither the gate nor the temperature would be seen)
        model.lin.bias.fill_(0.5)
    return model


def _open_readout(model, batch, bs=BS):
    """The read-out's ReLU must be open for most seeds (a dead one passes no gradient at all): gated sums are not normalised by
    degree and can sit far below zero, so the read-out bias is raised until at most a fifth of the seeds are closed."""
    with torch.no_grad():
        model.eval()
        relu, model.no_relu = model.no_relu, True
        raw = model(batch.x_dict, batch.edge_index_dict, bs).reshape(-1)
        model.no_relu = relu
        model.train()
        model.lin.bias.add_(max(0.0, 0.1 - float(torch.quantile(raw, 0.2))))


def _batch(kg, bs=BS):
    from kgwas_amd.sampler import NeighborLoader
    ids = np.random.default_rng(0).choice(kg.data['SNP'].x.shape[0], size=bs, replace=False)
    return next(iter(NeighborLoader(kg.data, [-1, -1], ('SNP', ids), batch_size=bs, device='cuda:0', seed=5)))


def _labels(kg):
    g = torch.Generator().manual_seed(9)
    n = kg.data['SNP'].x.shape[0]
    return kg.data['SNP'].y.cuda(), (torch.rand(n, generator=g, dtype=torch.float64) + 0.5).cuda()


def _check_against_oracle(model, batch, y_all, w_all, bs=BS):
    """forward_loss + backward of the product against the oracle on the same batch: predictions, loss, all gradients."""
    from kgwas_amd import ops
    model.train()
    model.zero_grad(set_to_none=True)
    n_id = batch.n_id('SNP')
    loss, pred = model.forward_loss(batch.x_dict, batch.edge_index_dict, bs, n_id, y_all, w_all, unit_grad=True)
    loss.backward(gradient=ops.unit_gradient(loss.device))
    with torch.no_grad():
        model.eval()
        out = model(batch.x_dict, batch.edge_index_dict, bs)
        model.train()
    oracle = R.gated_oracle(model)
    x, ei = batch_cpu(batch)
    out_o = oracle(x, ei, bs).reshape(-1)
    ids = n_id[:bs].long().cpu()
    y, w = y_all.cpu().double()[ids], w_all.cpu().double()[ids]
    loss_o = torch.mean(w * (out_o - y) ** 2)
    loss_o.backward()
    print(f'pred: max abs err {float((pred.detach().cpu().double() - out_o.detach()).abs().max()):.3e}, max |ref| '
          f'{float(out_o.detach().abs().max()):.3e}; loss {float(loss.detach()):.9f} vs {float(loss_o.detach()):.9f}')
    assert float((out_o.detach() > 0).double().mean()) > 0.5, 'most seeds must sit on the open side of the read-out ReLU'
    assert_close(pred, out_o.detach(), RTOL, ATOL, 'pred (forward_loss)')
    assert_close(out.reshape(pred.shape), out_o.detach(), RTOL, ATOL, 'pred (forward)')
    assert_close(loss.detach(), loss_o.detach(), RTOL, ATOL, 'loss')
    go = grads_by_name(oracle)
    n_live = n_att = 0
    for name, g in grads_by_name(model).items():
        ref = go[name]
        if g is None:
            assert ref is None or float(ref.abs().max()) == 0.0, f'{name}: product has no grad, oracle has'
            continue
        n_live += 1
        n_att += name.endswith('att_src') and float(ref.abs().max()) > 0
        assert tuple(g.shape) == tuple(ref.shape), (name, g.shape, ref.shape)
        assert_close(g, ref, RTOL, max(ATOL, 1e-4 * float(ref.abs().max())), f'grad {name}')
    assert n_live > 10 and n_att > 3
    return oracle, x, ei, out_o


@pytest.mark.parametrize('aggr,temp,cl', [('sum', 1.0, 128), ('sum', 2.0, 128), ('max', 1.0, 128), ('max', 2.0, 128), ('sum', 2.0, 96)],
                         ids=['sum-T1', 'sum-T2', 'max-T1', 'max-T2', 'sum-T2-hidden96'])
def test_gated_model_matches_the_oracle(small_kg, aggr, temp, cl):
    model = _model(small_kg, cl, aggr, gat_sigmoid=True, gat_temperature=temp)
    assert model.gat_sigmoid and model.temperature == temp and not model.fold_fc
    batch = _batch(small_kg)
    _open_readout(model, batch)
    oracle, x, ei, out_o = _check_against_oracle(model, batch, *_labels(small_kg))
    # the gates are really computed: the same weights under the softmax are another function
    for hc in oracle.convs:
        for conv in hc.convs.values():
            conv.sigmoid_gat = False
    with torch.no_grad():
        assert float((oracle(x, ei, BS).reshape(-1) - out_o).abs().max()) > 1e-4


@pytest.mark.parametrize('aggr', ['sum', 'max'])
def test_temperature_alone(small_kg, aggr):
    """The softmax model at gat_temperature = 2: with gnn_aggr='sum' the folded, fused route."""
    model = _model(small_kg, 128, aggr, gat_temperature=2.0)
    assert not model.gat_sigmoid and model.temperature == 2.0 and model.fold_fc == (aggr == 'sum')
    oracle, x, ei, out_o = _check_against_oracle(model, _batch(small_kg), *_labels(small_kg))
    for hc in oracle.convs:
        for conv in hc.convs.values():
            conv.temperature = 1.0
    with torch.no_grad():
        assert float((oracle(x, ei, BS).reshape(-1) - out_o).abs().max()) > 1e-4


@pytest.mark.parametrize('kw', [dict(gat_sigmoid=True, gat_temperature=2.0), dict(gat_temperature=2.0)], ids=['gate-T2', 'softmax-T2'])
def test_captured_step_equals_eager_loop(tiny_kg, kw):
    """Eight steps of GraphTrainStep against eight eager steps from the same initial state; the bar of
    tests/test_gpu_multihead_model.py::test_captured_step_equals_eager_loop (the captured step orders some sums differently)."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    bs, nsteps, seed = 32, 8, 11
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * nsteps])
    assert len(ids) == bs * nsteps
    run_e = KGWAS(tiny_kg, device='cuda:0', seed=seed)
    run_e.initialize_model(**kw)
    run_g = KGWAS(tiny_kg, device='cuda:0', seed=seed)
    run_g.initialize_model(**kw)
    with torch.no_grad():
        run_e.model.lin.bias.fill_(0.5)    # (an open read-out ReLU: every parameter gets a gradient)
    run_g.model.load_state_dict(run_e.model.state_dict())
    p0 = params_by_name(run_e.model)
    gs = GraphTrainStep(run_g, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=seed)
    assert gs.n_batches == nsteps
    opt = torch.optim.Adam(run_e.model.parameters(), lr=1e-3, weight_decay=5e-4)
    ld_w = run_e._ld_weight_vector()
    run_e.model.train()
    run_g.model.train()
    for step, batch in enumerate(NeighborLoader(tiny_kg.data, [-1, -1], ('SNP', ids), batch_size=bs, drop_last=True, device='cuda:0')):
        le = run_e.train_step(batch, opt, ld_w)
        lg = gs.step(step)
        print(f'step {step}: eager {float(le.detach()):.9f} captured {float(lg.detach()):.9f}')
        assert_close(lg.detach().clone(), le.detach(), 1e-5, 1e-7, f'loss step {step}')
    gs.check()
    assert step == nsteps - 1
    pe, pg = params_by_name(run_e.model), params_by_name(run_g.model)
    num = sum(float((pe[n] - pg[n]).pow(2).sum()) for n in pe)
    den = sum(float((pe[n] - p0[n]).pow(2).sum()) for n in pe)
    print(f'relative update difference {(num / den) ** 0.5:.3e}')
    assert den > 0 and (num / den) ** 0.5 < 5e-3, f'relative update difference {(num / den) ** 0.5:.3e}'
    moved = [n for n in pe if n.endswith('att_src') and float((pg[n] - p0[n]).abs().max()) > 0]
    assert len(moved) > 3


def _tiny4(tmp_path_factory):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path_factory.mktemp('gate_tiny4')),
                                     n_traits=4)


@pytest.mark.parametrize('case', ['plain', 'fanout', 'traits4'])
def test_train_save_and_load_pretrained(tiny_kg, tmp_path_factory, case):
    """KGWAS.train(epoch=1) with gat_sigmoid=True runs through -- the captured step, evaluation, the result tables --, the
    validation metrics are finite, and load_pretrained of what it saved predicts the same values."""
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    kg = _tiny4(tmp_path_factory) if case == 'traits4' else tiny_kg
    T = 4 if case == 'traits4' else 1
    run = KGWAS(kg, device='cuda:0', seed=3)
    run.initialize_model(gat_sigmoid=True, gat_temperature=2.0, out_channels=T)
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)      # (an open read-out ReLU: predictions that are not all zero)
    name = 'sigmoid_gate_' + case
    run.train(batch_size=32, epoch=1, save_best_model=True, save_name=name, num_neighbors=[10, 5] if case == 'fanout' else None)
    assert np.isfinite(run.val_metrics['mse']) and np.isfinite(run.val_metrics['pearsonr'])
    assert run.config['gat_sigmoid'] is True and run.config['gat_temperature'] == 2.0
    run2 = KGWAS(kg, device='cuda:0', seed=4)
    run2.load_pretrained(os.path.join(kg.data_path, 'model', name))
    assert run2.config == run.config and run2.model.gat_sigmoid and run2.model.temperature == 2.0
    ids = np.asarray(kg.test_input_nodes[1][:32])
    batch = next(iter(NeighborLoader(kg.data, [-1, -1], ('SNP', ids), batch_size=32, device='cuda:0')))
    run.best_model.eval(); run2.model.eval()
    with torch.no_grad():
        a = run.best_model(batch.x_dict, batch.edge_index_dict, 32)
        b = run2.model(batch.x_dict, batch.edge_index_dict, 32)
    assert a.shape == (32, T) and torch.equal(a, b) and float(a.abs().sum()) > 0 and bool(torch.isfinite(a).all())


def test_attention_under_the_gate(small_kg):
    """get_network_weight of a gated model: every weight in (0, 1), and per relation and layer the float64 oracle's gates over the
    full graph -- layer 2 fed by the un-ReLU'd gated layer 1, as the reference's export does (kgwas/utils.py:452-460; conv.py:219-220
    takes the sigmoid branch whatever return_raw_attention_weights says).  forward(return_attention_weights=True): the mean gate per
    layer against the oracle's; hot_path_attention: sigmoid(e_edge / T) of the training path's edges.
    T = 10: layer 2 of the export reads un-ReLU'd, un-normalised sums over whole neighbourhoods, whose logits reach several tens, and
    in fp32 a gate is exactly 1 above e / T ~ 16.6 (at T = 2, 341 of the 214368 exported weights were); at T = 10 none is."""
    from kgwas_amd.kgwas import KGWAS
    from oracle.gat_oracle import GO_TYPES
    run = KGWAS(small_kg, device='cuda:0', seed=5)
    run.initialize_model(gat_sigmoid=True, gat_temperature=10.0)
    with torch.no_grad():                       # make bias / dead relations non-trivial
        for p in run.model.parameters():
            if p.dim() == 2 and p.shape[-1] == 128 and float(p.abs().sum()) == 0.0:
                p.uniform_(-0.1, 0.1)
    run.best_model = run.model
    df = run.get_network_weight()
    assert set(df.layer.unique()) == {'l1', 'l2'}
    print(f'gates: min {float(df.weight.min()):.3e}, 1 - max {1.0 - float(df.weight.max()):.3e}, exactly 1: {int((df.weight == 1.0).sum())}, '
          f'exactly 0: {int((df.weight == 0.0).sum())} of {len(df)}')
    assert float(df.weight.min()) > 0.0 and float(df.weight.max()) < 1.0
    g = small_kg.data
    o = R.gated_oracle(run.model)
    with torch.no_grad():
        x = {t: g[t].x.double() for t in g.node_types}
        x['SNP'] = o.snp_feat_mlp(x['SNP']); x['Gene'] = o.gene_feat_mlp(x['Gene'])
        for t in GO_TYPES:
            x[t] = o.go_feat_mlp(x[t])
        ei = {et: g[et].edge_index for et in g.edge_types}
        n_checked = 0
        for k, conv in enumerate(o.convs):
            x, att = conv(x, ei, return_attention_weights=True, raw=True)          # utils.py:452-460 (no relu)
            allg = torch.cat([a.reshape(-1) for a in att.values()])
            print(f'oracle layer {k + 1}: logit / T from {float(torch.logit(allg.clamp(1e-300, 1 - 1e-16)).min()):.2f} to '
                  f'{float(torch.logit(allg.clamp(1e-300, 1 - 1e-16)).max()):.2f}; exactly 1 in float64: {int((allg == 1.0).sum())}')
            for et, a in att.items():
                sub = df[(df.layer == f'l{k + 1}') & (df.h_type == et[0]) & (df.rel_type == et[1]) & (df.t_type == et[2])]
                e = ei[et].numpy()
                key_ref = e[0].astype(np.int64) * (1 << 32) + e[1]
                _, first = np.unique(key_ref, return_index=True)
                ref = dict(zip(key_ref[first].tolist(), a.reshape(-1).numpy()[first].tolist()))
                key_my = sub.h_idx.values.astype(np.int64) * (1 << 32) + sub.t_idx.values.astype(np.int64)
                assert len(key_my) == len(ref) and set(key_my.tolist()) == set(ref)
                mine = torch.tensor(sub.weight.values)
                want = torch.tensor([ref[q] for q in key_my.tolist()])
                assert_close(mine, want, 2e-4, 1e-5, f'gate l{k + 1} {et}', rel_to_max=1e-5)
                n_checked += len(ref)
    assert n_checked > 0
    # the mean gate per layer over all edge types of a batch (kgwas/model.py:65-72)
    model = run.model.eval()
    batch = _batch(small_kg, 32)
    xb, eb = batch_cpu(batch)
    with torch.no_grad():
        p, att = model(batch.x_dict, batch.edge_index_dict, 32, return_attention_weights=True)
        po, atto = o(xb, eb, 32, return_attention_weights=True)
        assert_close(p, po, RTOL, ATOL, 'pred(attention)')
        assert len(att) == len(atto) == 2
        for l, (a, ao) in enumerate(zip(att, atto)):
            assert 0.0 < float(a) < 1.0
            assert abs(float(a) - float(ao)) <= 1e-5 * abs(float(ao)) + 1e-7, (l, float(a), float(ao))       # (test_gpu_model.py's bar)
        hot = model.hot_path_attention(batch)
    assert len(hot) == 2
    for l, a in enumerate(hot):
        assert a.numel() == int(batch.meta.n_edges[l]) and float(a.min()) > 0.0 and float(a.max()) < 1.0
