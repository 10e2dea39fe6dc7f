"""-m gpu: HeteroGNN(gat_edge_dim=D) up to KGWAS.train(), against the float64 model oracle of tests/edge_attr_ref.py
(oracle/gat_oracle.py's model whose attributed relations carry lin_edge / att_edge, conv.py:207-215 op for op) on the small
synthetic KG of the other model tests, with attributes on some relations (and their mirrors) and none on the others.

Tolerances of tests/test_gpu_sigmoid_gate_model.py: predictions and loss rtol 1e-4 / atol 1e-5, gradients rtol 1e-4 / atol
max(1e-5, 1e-4 max|ref|), plus assert_close's rel_to_max; the export: rtol 2e-4 / atol 1e-5.  The captured step against the eager
step, and a cached epoch against a re-sampled one: bit for bit."""
import os

import numpy as np
import pytest
import torch

from tests import edge_attr_ref as R
from tests.helpers import assert_close, grads_by_name

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
BS = 48
D = 3
RELS = ['ABC', 'eQTL', 'PCHi-C', 'Gene-Signaling-Gene', 'Gene-Reaction-Gene', 'Gene-Associates-BiologicalProcess']


def _kg(tmp_path_factory, scale, gene, seed, name, edge_dim=D):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=scale, seed=seed, feat_dims={'Gene': gene}, data_path=str(tmp_path_factory.mktemp(name)),
                                     edge_dim=edge_dim, edge_attr_relations=RELS)


@pytest.fixture(scope='module')
def small_attr_kg(tmp_path_factory):
    """conftest's small_kg (1 % scale, hubs above KGW_CHUNK) with 3-wide attributes on RELS and their mirrors."""
    return _kg(tmp_path_factory, 0.01, 96, 1, 'eattr_small')


@pytest.fixture(scope='module')
def tiny_attr_kg(tmp_path_factory):
    return _kg(tmp_path_factory, 0.002, 40, 3, 'eattr_tiny')


def _model(kg, cl=128, aggr='sum', layers=2, seed=3, edge_dim=D, bias_shift=0.0):
    from kgwas_amd.model import HeteroGNN
    torch.manual_seed(seed)
    dims = (kg.snp_init_dim_size, kg.gene_init_dim_size, kg.go_init_dim_size)
    model = HeteroGNN(kg.data, cl, 1, layers, 'GAT', aggr, *dims, 1, gat_edge_dim=edge_dim).cuda()
    with torch.no_grad():
        for pack in list(model.live_packs) + list(model.dead_packs):
            pack.bias[:, :cl].normal_(0, 0.1).add_(bias_shift)
            pack.att_src.mul_(4.0)      # (glorot-sized attention vectors give logits near 0 and a flat softmax: nothing would be seen)
            pack.att_dst.mul_(4.0)
            pack.att_edge.mul_(4.0)
        model.lin.bias.fill_(0.5)
    return model


def _batch(kg, bs=BS, layers=2):
    from kgwas_amd.sampler import NeighborLoader
    ids = np.random.default_rng(0).choice(kg.data['SNP'].x.shape[0], size=bs, replace=False)
    return next(iter(NeighborLoader(kg.data, [-1] * layers, ('SNP', ids), batch_size=bs, device='cuda:0', seed=5)))


def _labels(kg):
    g = torch.Generator().manual_seed(9)
    n = kg.data['SNP'].x.shape[0]
    return kg.data['SNP'].y.cuda(), (torch.rand(n, generator=g, dtype=torch.float64) + 0.5).cuda()


def _check_against_oracle(model, batch, y_all, w_all, bs=BS):
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
    oracle = R.oracle_from_product(model)
    x, ei, ea = R.batch_cpu(batch)
    out_o = oracle(x, ei, ea, bs).reshape(-1)
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
    n_live = n_edge = 0
    for name, g in grads_by_name(model).items():
        ref = go[name]
        if g is None:
            assert ref is None or float(ref.abs().max()) == 0.0, f'{name}: product has no grad, oracle has'
            continue
        n_live += 1
        edge = name.endswith('lin_edge.weight') or name.endswith('att_edge')
        n_edge += edge and float(ref.abs().max()) > 0
        if edge:
            print(f'{name}: max abs err {float((g.double() - ref).abs().max()):.3e}, max |ref| {float(ref.abs().max()):.3e}')
        assert tuple(g.shape) == tuple(ref.shape), (name, g.shape, ref.shape)
        assert_close(g, ref, RTOL, max(ATOL, 1e-4 * float(ref.abs().max())), f'grad {name}')
    print(f'{n_live} gradients compared, {n_edge} of them non-zero edge parameters')
    assert n_live > 10 and n_edge > 3
    return oracle, x, ei, ea, out_o


@pytest.mark.parametrize('aggr,cl,layers', [('sum', 128, 2), ('mean', 128, 2), ('min', 128, 2), ('max', 128, 2), ('sum', 96, 2), ('sum', 128, 1)],
                         ids=['sum', 'mean', 'min', 'max', 'sum-hidden96', 'sum-1layer'])
def test_model_matches_the_oracle(small_attr_kg, aggr, cl, layers):
    # ('min': the minimum over a gene's ~17 relations is negative in nearly every channel and the ReLU after it would close -- every
    #  hidden state and every gradient exactly zero; the relation biases are raised by 1 to keep it open)
    model = _model(small_attr_kg, cl, aggr, layers, bias_shift=1.0 if aggr == 'min' else 0.0)
    assert model.edge_dim == D and model.fold_fc == (aggr in ('sum', 'mean'))      # the folded route stays
    batch = _batch(small_attr_kg, layers=layers)
    oracle, x, ei, ea, out_o = _check_against_oracle(model, batch, *_labels(small_attr_kg))
    # the attributes are really read: without them the same weights give other predictions
    with torch.no_grad():
        zero = {k: torch.zeros_like(v) for k, v in ea.items()}
        assert float((oracle(x, ei, zero, BS).reshape(-1) - out_o).abs().max()) > 1e-4


def test_seed_outputs_equal_the_full_graph_outputs(small_attr_kg):
    """The hop-pruned mini-batch and the plain COO route over the whole graph (edge_attr_dict) predict the same values for the seeds."""
    model = _model(small_attr_kg).eval()
    batch = _batch(small_attr_kg)
    g = small_attr_kg.data
    with torch.no_grad():
        a = model(batch.x_dict, batch.edge_index_dict, BS)
        x = {t: g[t].x.cuda() for t in g.node_types}
        ei = {et: g[et].edge_index.cuda() for et in g.edge_types}
        ea = {et: g[et].edge_attr.cuda() for et in g.edge_types if g[et].get('edge_attr') is not None}
        full = model(x, ei, int(g['SNP'].x.shape[0]), edge_attr_dict=ea)
    assert_close(a, full[batch.n_id('SNP')[:BS].long()], RTOL, ATOL, 'seeds: mini-batch against full graph')
    # batch.edge_attr_dict is what the oracle's own lookup finds
    _, _, ea_ref = R.batch_cpu(batch)
    mine = batch.edge_attr_dict
    assert set(mine) == set(ea_ref) and all(torch.equal(mine[k].cpu().double(), ea_ref[k]) for k in ea_ref)


def _runs(kg, seed, **kw):
    from kgwas_amd.kgwas import KGWAS
    run_e = KGWAS(kg, device='cuda:0', seed=seed)
    run_e.initialize_model(gat_edge_dim=D, **kw)
    run_g = KGWAS(kg, device='cuda:0', seed=seed)
    run_g.initialize_model(gat_edge_dim=D, **kw)
    with torch.no_grad():
        run_e.model.lin.bias.fill_(0.5)    # (an open read-out ReLU: every parameter gets a gradient)
        for pack in run_e.model.live_packs:
            pack.att_edge.mul_(4.0)
    run_g.model.load_state_dict(run_e.model.state_dict())
    return run_e, run_g


def test_captured_step_equals_eager_step_bit_for_bit(tiny_attr_kg):
    """One step of GraphTrainStep against one eager step of the same launches (a static layout, the fused optimiser launch, the
    d u_r / d v_r pieces) from the same state: the loss and every parameter afterwards, bit for bit; then eight steps against the
    plain eager loop at the sibling tests' bar.  fused_adam stays on and the edge parameters move."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.sampler import NeighborLoader
    from tests.helpers import params_by_name
    bs, nsteps, seed = 32, 8, 11
    ids = np.asarray(tiny_attr_kg.train_input_nodes[1][:bs * nsteps])
    run_e, run_g = _runs(tiny_attr_kg, seed)
    p0 = params_by_name(run_e.model)
    gs = GraphTrainStep(run_g, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=seed)
    assert gs.fused_adam and gs.n_batches == nsteps and run_g.model.fold_fc
    # a second trainer on its own copy of the model, stepped EAGERLY through the body the first one captured
    run_c, _ = _runs(tiny_attr_kg, seed)
    run_c.model.load_state_dict(run_e.model.state_dict())
    gc = GraphTrainStep(run_c, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=seed)
    run_c.model.train(); run_g.model.train()
    lg = gs.step(0).detach().clone()
    gc._sample_now(0, 0)
    torch.cuda.synchronize()
    lc = gc._step_body(0)
    lc = (lc[0] if isinstance(lc, tuple) else lc).detach().clone()
    torch.cuda.synchronize()
    assert torch.equal(lg, lc), (float(lg), float(lc))
    pg, pc = params_by_name(run_g.model), params_by_name(run_c.model)
    assert all(torch.equal(pg[n], pc[n]) for n in pg), [n for n in pg if not torch.equal(pg[n], pc[n])][:5]
    assert gc.fused_adam
    # the captured loop against the plain eager loop
    opt = torch.optim.Adam(run_e.model.parameters(), lr=1e-3, weight_decay=5e-4)
    ld_w = run_e._ld_weight_vector()
    run_e.model.train()
    for step, batch in enumerate(NeighborLoader(tiny_attr_kg.data, [-1, -1], ('SNP', ids), batch_size=bs, drop_last=True, device='cuda:0')):
        le = run_e.train_step(batch, opt, ld_w)
        lg = gs.step(step) if step else lg
        assert_close(lg.detach().clone(), le.detach(), 1e-5, 1e-7, f'loss step {step}')
    gs.check()
    pe, pg = params_by_name(run_e.model), params_by_name(run_g.model)
    num = sum(float((pe[n] - pg[n]).pow(2).sum()) for n in pe)
    den = sum(float((pe[n] - p0[n]).pow(2).sum()) for n in pe)
    print(f'relative update difference {(num / den) ** 0.5:.3e}')
    assert den > 0 and (num / den) ** 0.5 < 5e-3
    moved = [n for n in pe if n.endswith(('att_edge', 'lin_edge.weight')) and float((pg[n] - p0[n]).abs().max()) > 0]
    assert len(moved) > 3, moved


def test_cached_epoch_equals_resampled_epoch_bit_for_bit(tiny_attr_kg):
    """Epoch 2 served from BatchCache (the chunks' gpos travel with the batch) against epoch 2 re-sampled."""
    from kgwas_amd.graph_step import GraphTrainStep
    from tests.helpers import params_by_name
    bs, nsteps, seed = 32, 4, 7
    ids = np.asarray(tiny_attr_kg.train_input_nodes[1][:bs * nsteps])
    out = []
    for cache in (True, False):
        run, _ = _runs(tiny_attr_kg, seed)
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=seed, cache_batches=cache)
        run.model.train()
        losses = [gs.step(i).detach().clone() for _ in range(2) for i in range(nsteps)]
        gs.check()
        torch.cuda.synchronize()
        if cache:
            assert gs.cache is not None and gs.cache.restored >= nsteps - 1
        else:
            assert gs.cache is None
        out.append((torch.stack(losses), params_by_name(run.model)))
    assert torch.equal(out[0][0], out[1][0])
    assert all(torch.equal(out[0][1][n], out[1][1][n]) for n in out[0][1])


def test_evaluation_attention_queries_and_export(small_attr_kg):
    """evaluate_minibatch_clean's captured evaluation; forward(return_attention_weights=True) and hot_path_attention (rows sum to
    1, the oracle's alpha); get_network_weight against the oracle's raw logits over the whole graph."""
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    from kgwas_amd.utils import evaluate_minibatch_clean
    from tests.helpers import segment_alpha_sums
    kg = small_attr_kg
    run = KGWAS(kg, device='cuda:0', seed=5)
    run.initialize_model(gat_edge_dim=D)
    with torch.no_grad():
        for p in run.model.parameters():
            if p.dim() == 2 and p.shape[-1] == 128 and float(p.abs().sum()) == 0.0:
                p.uniform_(-0.1, 0.1)
        for pack in list(run.model.live_packs) + list(run.model.dead_packs):
            pack.att_edge.mul_(4.0)
        run.model.lin.bias.fill_(0.5)
    model = run.model.eval()
    o = R.oracle_from_product(model)
    batch = _batch(kg, 32)
    x, ei, ea = R.batch_cpu(batch)
    with torch.no_grad():
        # evaluation
        ids = np.asarray(kg.test_input_nodes[1][:96])
        res = evaluate_minibatch_clean(NeighborLoader(kg.data, [-1, -1], ('SNP', ids), batch_size=32, device='cuda:0'), model, 'cuda:0')
        eager = torch.cat([model(b.x_dict, b.edge_index_dict, 32).reshape(-1)
                           for b in NeighborLoader(kg.data, [-1, -1], ('SNP', ids), batch_size=32, device='cuda:0')])
        assert_close(torch.as_tensor(res['pred']).reshape(-1), eager, 1e-6, 1e-7, 'evaluation against eager forwards')
        # the mean attention per layer over all edge types of a batch (kgwas/model.py:65-72)
        p, att = model(batch.x_dict, batch.edge_index_dict, 32, return_attention_weights=True)
        po, atto = o(x, ei, ea, 32, return_attention_weights=True)
        assert_close(p, po, RTOL, ATOL, 'pred(attention)')
        for l, (a, ad) in enumerate(zip(att, atto)):
            ao = torch.cat([v.reshape(-1) for v in ad.values()]).mean()
            assert abs(float(a) - float(ao)) <= 1e-5 * abs(float(ao)) + 1e-7, (l, float(a), float(ao))
        hot = model.hot_path_attention(batch)
        for l, a in enumerate(hot):
            sums = segment_alpha_sums(batch, l + 1, a)
            assert a.numel() == int(batch.meta.n_edges[l]) and float((sums - 1.0).abs().max()) <= 1e-5
        # ... and they are the oracle's alpha on the live relations' edges of the top layer (every row of it is a seed row)
        lay2 = atto[1]
        sc = batch.dg.schema
        from tests.test_gpu_aggregate_parity import layer_edges
        for r, (eid, src, dst) in layer_edges(batch, 2).items():
            et = sc.edge_types[r]
            e_all = ei[et]
            keep = e_all[1] < 32                      # the oracle computes every row of the batch; layer 2 of the hot path, the seeds
            assert torch.equal(e_all[0][keep], src) and torch.equal(e_all[1][keep], dst)
            assert_close(hot[1][eid.cuda()], lay2[et].reshape(-1)[keep], RTOL, ATOL, f'alpha layer 2 {et}')
    # the attention query is inference only, as ever: nothing it returns is attached to an autograd graph
    p2, att2 = model(batch.x_dict, batch.edge_index_dict, 32, return_attention_weights=True)
    assert not p2.requires_grad and not any(a.requires_grad for a in att2) and torch.equal(p2, p)
    # the export
    run.best_model = run.model
    df = run.get_network_weight()
    assert set(df.layer.unique()) == {'l1', 'l2'}
    g = kg.data
    with torch.no_grad():
        xg = o.embed({t: g[t].x.double() for t in g.node_types})
        eig = {et: g[et].edge_index for et in g.edge_types}
        eag = {et: g[et].edge_attr.double() for et in g.edge_types if g[et].get('edge_attr') is not None}
        n_checked = 0
        for k, conv in enumerate(o.convs):
            xg, att = conv(xg, eig, eag, return_attention_weights=True, raw=True)          # utils.py:452-460 (no relu)
            for et, a in att.items():
                sub = df[(df.layer == f'l{k + 1}') & (df.h_type == et[0]) & (df.rel_type == et[1]) & (df.t_type == et[2])]
                e = eig[et].numpy()
                key_ref = e[0].astype(np.int64) * (1 << 32) + e[1]
                _, first = np.unique(key_ref, return_index=True)
                # (parallel edges carry different attributes; the table keeps the first of them in CSR order = in edge_index order)
                ref = dict(zip(key_ref[first].tolist(), a.reshape(-1).numpy()[first].tolist()))
                key_my = sub.h_idx.values.astype(np.int64) * (1 << 32) + sub.t_idx.values.astype(np.int64)
                assert len(key_my) == len(ref) and set(key_my.tolist()) == set(ref)
                assert_close(torch.tensor(sub.weight.values), torch.tensor([ref[q] for q in key_my.tolist()]), 2e-4, 1e-5,
                             f'raw attention l{k + 1} {et}', rel_to_max=1e-5)
                n_checked += len(ref)
    assert n_checked > 1000


def test_train_two_epochs_save_and_load_pretrained(tiny_attr_kg):
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    kg = tiny_attr_kg
    run = KGWAS(kg, device='cuda:0', seed=3)
    run.initialize_model(gat_edge_dim=D)
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)
    run.train(batch_size=32, epoch=2, save_best_model=True, save_name='edge_attr')
    assert np.isfinite(run.val_metrics['mse']) and np.isfinite(run.val_metrics['pearsonr'])
    assert run.config['gat_edge_dim'] == D
    run2 = KGWAS(kg, device='cuda:0', seed=4)
    run2.load_pretrained(os.path.join(kg.data_path, 'model', 'edge_attr'))
    assert run2.config == run.config and run2.model.edge_dim == D
    ids = np.asarray(kg.test_input_nodes[1][:32])
    batch = next(iter(NeighborLoader(kg.data, [-1, -1], ('SNP', ids), batch_size=32, device='cuda:0')))
    run.best_model.eval(); run2.model.eval()
    with torch.no_grad():
        a = run.best_model(batch.x_dict, batch.edge_index_dict, 32)
        b = run2.model(batch.x_dict, batch.edge_index_dict, 32)
    assert a.shape == (32, 1) and torch.equal(a, b) and float(a.abs().sum()) > 0 and bool(torch.isfinite(a).all())
    with pytest.raises(NotImplementedError, match='num_neighbors'):
        run.train(batch_size=32, epoch=1, num_neighbors=[10, 5])
