"""-m gpu: HeteroGNN(gat_num_head = 2 / 4, gat_split_heads=True) -- the unfused multi-head route (ops.gat_aggregate(heads=H) + ops.layer_transform_heads)
against the float64 oracle with heads (tests/multihead_ref.py:oracle_with_heads: GATConvOracle(cl, cl or None, cl / H, heads=H) per
relation), on the small synthetic KG of the other model tests: the seeds' predictions, the loss and every gradient under the
reference's names; the captured training step against eager steps; the captured evaluation against forward; KGWAS.train +
load_pretrained.

Tolerances of tests/test_gpu_model.py / tests/test_gpu_attn_dropout.py: predictions and loss rtol 1e-4 / atol 1e-5, gradients rtol
1e-4 / atol max(1e-5, 1e-4 max|ref|), plus assert_close's rel_to_max; captured against eager: losses rtol 1e-5 / atol 1e-7, relative
update difference below 5e-3."""
import os

import numpy as np
import pytest
import torch

from tests import multihead_ref as R
from tests.helpers import assert_close, batch_cpu, grads_by_name, params_by_name

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
BS = 48


def _model(kg, H, cl=128, aggr='sum', out_channels=1, seed=3):
    from kgwas_amd.model import HeteroGNN
    torch.manual_seed(seed)
    dims = (kg.snp_init_dim_size, kg.gene_init_dim_size, kg.go_init_dim_size)
    model = HeteroGNN(kg.data, cl, out_channels, 2, 'GAT', aggr, *dims, H, gat_split_heads=True).cuda()
    with torch.no_grad():
        for pack in list(model.live_packs) + list(model.dead_packs):
            pack.bias[:, :cl].normal_(0, 0.1)
        model.lin.bias.fill_(0.5)          # (the read-out's ReLU must be open for most seeds: a dead one passes no gradient at all)
    return model


def _batch(kg, num_neighbors=(-1, -1), bs=BS):
    from kgwas_amd.sampler import NeighborLoader
    ids = np.random.default_rng(0).choice(kg.data['SNP'].x.shape[0], size=bs, replace=False)
    return next(iter(NeighborLoader(kg.data, list(num_neighbors), ('SNP', ids), batch_size=bs, device='cuda:0', seed=5)))


def _check_against_oracle(model, batch, y_all, w_all, bs=BS):
    """forward_loss + backward of the product against the oracle with heads on the same batch: predictions, loss, all gradients."""
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
    oracle = R.oracle_with_heads(model)
    x, ei = batch_cpu(batch)
    out_o = oracle(x, ei, bs)
    ids = n_id[:bs].long().cpu()
    y, w = y_all.cpu().double()[ids], w_all.cpu().double()[ids]
    T = model.lin.out_features
    if T == 1:
        loss_o = torch.mean(w * (out_o.reshape(-1) - y) ** 2)
        out_o = out_o.reshape(-1)
    else:
        loss_o = (w[:, None] * (out_o - y) ** 2).mean()
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


def _labels(kg):
    g = torch.Generator().manual_seed(9)
    n = kg.data['SNP'].x.shape[0]
    return kg.data['SNP'].y.cuda(), (torch.rand(n, generator=g, dtype=torch.float64) + 0.5).cuda()


@pytest.mark.parametrize('cl', [128, 64])
@pytest.mark.parametrize('H', [2, 4])
def test_model_matches_the_oracle_with_heads(small_kg, H, cl):
    model = _model(small_kg, H, cl)
    batch = _batch(small_kg)
    y_all, w_all = _labels(small_kg)
    oracle, x, ei, out_o = _check_against_oracle(model, batch, y_all, w_all)
    # the same weights read as ONE head are another function: the heads are really computed
    from tests.helpers import oracle_from_product
    twin = _model(small_kg, 1, cl)
    twin.load_state_dict({k: (v.reshape(1, 1, -1) if k.endswith(('att_src', 'att_dst')) else v)
                          for k, v in model.state_dict().items()})
    one = oracle_from_product(twin)
    with torch.no_grad():
        assert float((one(x, ei, BS).reshape(-1) - out_o).abs().max()) > 1e-4


def test_relation_mean(small_kg):
    model = _model(small_kg, 2, aggr='mean')
    _check_against_oracle(model, _batch(small_kg), *_labels(small_kg))


def test_finite_fanout(small_kg):
    model = _model(small_kg, 4, cl=64)
    batch = _batch(small_kg, num_neighbors=(3, 2))
    full = _batch(small_kg)
    assert batch.n_edges_sampled < full.n_edges_sampled
    _check_against_oracle(model, batch, *_labels(small_kg))


def test_four_label_columns(tmp_path_factory):
    from kgwas_amd.kgwas_data import KGWAS_Data
    kg = KGWAS_Data.from_synthetic(scale=0.01, seed=1, feat_dims={'Gene': 96}, data_path=str(tmp_path_factory.mktemp('mh_small4')),
                                   n_traits=4)
    model = _model(kg, 2, out_channels=4)
    y_all, w_all = _labels(kg)
    assert y_all.shape[1] == 4
    _check_against_oracle(model, _batch(kg), y_all, w_all)


def test_captured_step_equals_eager_loop(tiny_kg):
    """Three steps of GraphTrainStep at gat_num_head = 2 against three eager steps from the same initial state; the bar of
    tests/test_gpu_attn_dropout.py::test_captured_step_equals_eager_loop."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    bs, nsteps, seed = 32, 3, 11
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * 3])
    run_e = KGWAS(tiny_kg, device='cuda:0', seed=seed)
    run_e.initialize_model(gat_num_head=2)
    run_g = KGWAS(tiny_kg, device='cuda:0', seed=seed)
    run_g.initialize_model(gat_num_head=2)
    with torch.no_grad():
        run_e.model.lin.bias.fill_(0.5)    # (an open read-out ReLU: every parameter gets a gradient)
    run_g.model.load_state_dict(run_e.model.state_dict())
    p0 = params_by_name(run_e.model)
    gs = GraphTrainStep(run_g, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=seed)
    assert gs.n_batches == 3 and not gs.fused_adam
    for n, p in params_by_name(run_g.model).items():
        assert torch.equal(p, p0[n]), n
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
    assert den > 0 and (num / den) ** 0.5 < 5e-3, f'relative update difference {(num / den) ** 0.5:.3e}'
    # every attention vector moved: the heads' gradients reach their parameters through the captured step too
    moved = [n for n in pe if n.endswith('att_src') and float((pg[n] - p0[n]).abs().max()) > 0]
    assert len(moved) > 3


def test_captured_evaluation_equals_forward(small_kg):
    from kgwas_amd.graph_step import GraphEvalStep
    model = _model(small_kg, 4).eval()
    ids = np.asarray(small_kg.test_input_nodes[1])[:64 * 2 + 9]
    ge = GraphEvalStep(model, small_kg.data, 2, ('SNP', ids), 64, 'cuda:0', eval_batch=64)
    got = ge.run().cpu()
    from kgwas_amd.sampler import NeighborLoader
    ref = []
    with torch.no_grad():
        for batch in NeighborLoader(small_kg.data, [-1, -1], ('SNP', ids), batch_size=64, drop_last=False, device='cuda:0'):
            bs = batch['SNP'].batch_size
            ref.append(model(batch.x_dict, batch.edge_index_dict, bs).reshape(-1).cpu())
    ref = torch.cat(ref)
    assert got.shape == ref.shape == (len(ids),) and float(ref.abs().max()) > 0
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-5, atol=1e-6)       # (tests/test_gpu_graph.py's bar for this comparison)


def test_train_save_and_load_pretrained(tiny_kg):
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    run = KGWAS(tiny_kg, device='cuda:0', seed=3)
    run.initialize_model(gat_num_head=2, gnn_hidden_dim=64)
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)      # (an open read-out ReLU: predictions that are not all zero)
    run.train(batch_size=32, epoch=1, save_best_model=True, save_name='multihead_h2')
    assert np.isfinite(run.val_metrics['mse']) and run.config['gat_num_head'] == 2
    path = os.path.join(tiny_kg.data_path, 'model', 'multihead_h2')
    run2 = KGWAS(tiny_kg, device='cuda:0', seed=4)
    run2.load_pretrained(path)
    assert run2.config['gat_num_head'] == 2 and run2.model.heads == 2 and run2.model.hidden_logical == 64
    ids = np.asarray(tiny_kg.test_input_nodes[1][:32])
    batch = next(iter(NeighborLoader(tiny_kg.data, [-1, -1], ('SNP', ids), batch_size=32, device='cuda:0')))
    run.best_model.eval(); run2.model.eval()
    with torch.no_grad():
        a = run.best_model(batch.x_dict, batch.edge_index_dict, 32)
        b = run2.model(batch.x_dict, batch.edge_index_dict, 32)
    assert torch.equal(a, b) and float(a.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# parallelism='seed': the multi-rank step (split backward, RCCL all-reduce of the gradient buckets, Adam on the bucket views)
# ------------------------------------------------------------------------------------------------------------------------------
DBS, DSTEPS = 32, 3


def _dist_run(kg):
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(kg, device='cuda:0', seed=11)
    run.initialize_model(gat_num_head=2)
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)
    return run


def _tiny():
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path='/tmp/kgwas_synth_tiny')


def _rccl_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['KGW_FORCE_MULTIRANK_PATH'] = '1'
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda:0'))
    try:
        from kgwas_amd.graph_step import GraphTrainStep
        kg = _tiny()
        run = _dist_run(kg)
        ids = np.asarray(kg.train_input_nodes[1])[:DBS * DSTEPS]
        gs = GraphTrainStep(run, ('SNP', ids), DBS, lr=1e-3, weight_decay=5e-4)
        assert gs.split_backward and not gs.capture_optimizer
        losses = [float(gs.step(i).detach()) for i in range(DSTEPS)]
        gs.check()
        torch.save({'params': {k: v.detach().cpu() for k, v in run.model.named_reference_tensors().items()}, 'losses': losses},
                   os.path.join(out_dir, 'rccl.pt'))
    finally:
        dist.destroy_process_group()


def test_seed_parallel_step_with_one_rank_tracks_the_single_gpu_step(tiny_kg, tmp_path):
    """The multi-rank step as a node runs it, with ONE rank (all a 1-GPU box can host; averaging over one rank is the identity),
    at gat_num_head = 2 against the single-GPU captured step from the same initial state: the same losses (rtol 1e-5 / atol 1e-7)
    and the same updates (relative difference below 5e-3), the bar of the captured-against-eager comparison above."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.start_processes(_rccl_worker, args=(1, port, str(tmp_path)), nprocs=1, join=True, start_method='spawn')
    got = torch.load(os.path.join(tmp_path, 'rccl.pt'), weights_only=False)
    from kgwas_amd.graph_step import GraphTrainStep
    run = _dist_run(tiny_kg)
    p0 = params_by_name(run.model)
    ids = np.asarray(tiny_kg.train_input_nodes[1])[:DBS * DSTEPS]
    gs = GraphTrainStep(run, ('SNP', ids), DBS, lr=1e-3, weight_decay=5e-4)
    assert gs.capture_optimizer and not gs.split_backward
    for i in range(DSTEPS):
        l = gs.step(i)
        assert_close(torch.tensor(got['losses'][i]), l.detach().cpu(), 1e-5, 1e-7, f'loss step {i}')
    gs.check()
    pe = params_by_name(run.model)
    num = sum(float((pe[n] - got['params'][n].double()).pow(2).sum()) for n in pe)
    den = sum(float((pe[n] - p0[n]).pow(2).sum()) for n in pe)
    assert den > 0 and (num / den) ** 0.5 < 5e-3, f'relative update difference {(num / den) ** 0.5:.3e}'
