"""-m gpu: hidden-state dropout (kgw_hidden_dropout, ops.hidden_dropout, HeteroGNN(gnn_dropout=p)) up to KGWAS.train().

The kernel against the numpy twin of the rule (tests/hidden_dropout_ref.py) with torch.equal: a kept element is one float32
multiply by float32(1 / (1 - p)), which numpy reproduces exactly, and a dropped one is exactly 0.0.
The model against the float64 oracle with the twin's masks multiplied into its hidden state, at the tolerances of
tests/test_gpu_attn_dropout.py::test_model_training_forward_backward_matches_the_masked_oracle (RTOL, ATOL, max(ATOL, 1e-4 max|ref|)
for gradients, plus assert_close's rel_to_max).
The trainer at the bars of test_gpu_attn_dropout.py::test_captured_step_equals_eager_loop (losses rtol 1e-5 / atol 1e-7, relative
update difference below 5e-3) and ::test_second_epoch_draws_other_masks_on_the_same_cached_batch (torch.equal on naming epoch 0
again)."""
import os

import numpy as np
import pytest
import torch

from tests import hidden_dropout_ref as R
from tests.helpers import assert_close, batch_cpu, grads_by_name, launches_of_one_step, oracle_from_product, params_by_name

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5                  # tests/test_gpu_aggregate_parity.py's, as test_gpu_attn_dropout.py imports them
WORDS = [R.dropout_word(0, 0, 0), R.dropout_word(42, 3, 17)]
PASS_ROWS = 2048 * 8                     # rows one pass of the largest launch grid covers (KGW_GRID blocks x 8 rows)
BS = 48


def _word_tensor(word):
    return torch.tensor([word - (1 << 64) if word >> 63 else word], dtype=torch.int64, device='cuda:0')


def _input(rows, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, R.C, generator=g)


def _launch(jobs, layer, p, word_t):
    """kgw_hidden_dropout on ``jobs`` = [(src tensor, dst tensor, type)]; the status."""
    from kgwas_amd import _lib
    from kgwas_amd.sampler import dropout_params
    arr = (_lib.KgwHDropJob * len(jobs))()
    for j, (x, y, t) in zip(arr, jobs):
        j.src, j.lds, j.dst, j.ldd, j.rows, j.type = x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), x.shape[0], t
    thresh, scale = dropout_params(p)
    assert (thresh, scale) == (R.thresh(p), float(R.scale(p)))
    return _lib.lib().kgw_hidden_dropout(len(jobs), arr, layer, word_t.data_ptr(), thresh, scale, _lib.stream_ptr())


@pytest.mark.parametrize('inplace', [False, True], ids=['out-of-place', 'in-place'])
@pytest.mark.parametrize('rows', [0, 1, 3, 4, 5, 257, PASS_ROWS + 9])
def test_kernel_equals_the_twin(rows, inplace):
    """One job at every row count where the half-wavefront / block / grid-stride mapping changes: none, one, an odd count, a full
    and an overfull half block, more than one block, and more rows than one pass of the largest grid takes."""
    word, layer, t, p = WORDS[1], 2, 3, 0.3
    x = _input(rows, 7 + rows)
    ref = torch.from_numpy(R.apply(x.numpy(), word, layer, t, p))
    src = x.cuda()
    dst = src if inplace else torch.full_like(src, 7.0)
    assert _launch([(src, dst, t)], layer, p, _word_tensor(word)) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), ref)
    if rows:
        dropped = int((ref == 0).sum())
        assert 0.2 * ref.numel() - 30 < dropped < 0.4 * ref.numel() + 30
        if not inplace:
            assert torch.equal(src.cpu(), x)                             # the source is only read


@pytest.mark.parametrize('n_jobs', [1, 5, 8])
def test_several_jobs_in_one_launch(n_jobs):
    """Distinct node types and row counts per job (one of them empty when there are several), two words, both kinds of destination."""
    counts = [37, 1, 0, 300, 8, 129, 5, 64][:n_jobs] if n_jobs > 1 else [37]
    types = [5, 0, 7, 2, 1, 6, 3, 4][:n_jobs]
    layer, p = 1, 0.5
    for word in WORDS:
        xs = [_input(n, 100 + k) for k, n in enumerate(counts)]
        jobs = []
        for k, x in enumerate(xs):
            src = x.cuda()
            jobs.append((src, src if k % 2 else torch.empty_like(src), types[k]))
        assert _launch(jobs, layer, p, _word_tensor(word)) == 0
        torch.cuda.synchronize()
        for (src, dst, t), x in zip(jobs, xs):
            assert torch.equal(dst.cpu(), torch.from_numpy(R.apply(x.numpy(), word, layer, t, p))), (t, x.shape[0])
        if n_jobs > 1:                                                   # the type enters the mask: equal rows, other elements
            a, b = R.keep(word, layer, types[0], 37, p), R.keep(word, layer, types[3], 37, p)
            assert not np.array_equal(a, b)


def test_strided_destination_and_source():
    """A destination that is a view of a wider buffer (ldd = 256) and a source with lds = 132: the other columns are untouched."""
    word, layer, t, p = WORDS[0], 1, 1, 0.25
    x = _input(70, 5)
    wide = torch.full((70, 256), -3.0, device='cuda:0')
    srcw = torch.zeros(70, 132, device='cuda:0')
    srcw[:, :128] = x.cuda()
    dst = wide[:, 128:]
    assert dst.stride(0) == 256 and dst.data_ptr() % 16 == 0
    assert _launch([(srcw[:, :128], dst, t)], layer, p, _word_tensor(word)) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), torch.from_numpy(R.apply(x.numpy(), word, layer, t, p)))
    assert bool((wide[:, :128] == -3.0).all())


def test_p_zero_returns_the_input_bits():
    x = _input(300, 9)
    x[0, 0], x[1, 5], x[2, 127], x[3, 3] = float('nan'), float('inf'), -float('inf'), -0.0
    src = x.cuda()
    dst = torch.empty_like(src)
    assert _launch([(src, dst, 2)], 1, 0.0, _word_tensor(WORDS[1])) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu().view(torch.int32), x.view(torch.int32))


def test_non_finite_values_are_dropped_to_zero_and_kept_otherwise():
    """NaN and +-Inf on positions the twin drops come out 0.0 (a select, not a product); on kept positions they stay non-finite."""
    word, layer, t, p = WORDS[1], 1, 0, 0.5
    k = R.keep(word, layer, t, 64, p)
    x = _input(64, 3)
    drop_pos, keep_pos = np.argwhere(~k)[:9], np.argwhere(k)[:9]
    vals = [float('nan'), float('inf'), -float('inf')] * 3
    for (i, c), v in zip(drop_pos, vals):
        x[i, c] = v
    for (i, c), v in zip(keep_pos, vals):
        x[i, c] = v
    src = x.cuda()
    dst = torch.empty_like(src)
    assert _launch([(src, dst, t)], layer, p, _word_tensor(word)) == 0
    out = dst.cpu()
    for i, c in drop_pos:
        assert float(out[i, c]) == 0.0 and not np.signbit(out[i, c].numpy())
    for (i, c), v in zip(keep_pos, vals):
        assert not np.isfinite(float(out[i, c])) and (np.isnan(v) == np.isnan(float(out[i, c])))
    assert torch.equal(torch.nan_to_num(out, 0.0, 1.0, -1.0), torch.nan_to_num(torch.from_numpy(R.apply(x.numpy(), word, layer, t, p)), 0.0, 1.0, -1.0))
    assert bool(torch.isfinite(out[torch.from_numpy(~k)]).all())


def test_two_runs_give_equal_bits_and_the_word_is_read_on_the_device():
    x = _input(1000, 11).cuda()
    w = _word_tensor(WORDS[0])
    a, b, c = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    assert _launch([(x, a, 1)], 1, 0.4, w) == 0 and _launch([(x, b, 1)], 1, 0.4, w) == 0
    w.copy_(_word_tensor(WORDS[1]))                                     # the same pointer, another word
    assert _launch([(x, c, 1)], 1, 0.4, w) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(c.cpu(), torch.from_numpy(R.apply(x.cpu().numpy(), WORDS[1], 1, 1, 0.4)))


def test_ops_forward_and_backward_equal_the_twin():
    """ops.hidden_dropout over three types: y' and dx = m' * dy' exactly, one block written in place of the next layer's input, the
    inputs left alone (the producer may have saved them), a None gradient passed through."""
    from kgwas_amd import ops
    word, layer, p = WORDS[1], 1, 0.25
    types, counts = [4, 0, 2], [33, 260, 5]
    xs = [_input(n, 40 + k) for k, n in enumerate(counts)]
    gs_ = [_input(n, 50 + k) for k, n in enumerate(counts)]
    leaves = [x.cuda().requires_grad_(True) for x in xs]
    buf = torch.zeros(300, R.C, device='cuda:0')
    blocks = [None, ops.RowBlock(buf, 16, 260), ops.RowBlock(buf, 0, 7)]           # (the last one does not fit: a temporary)
    outs = ops.hidden_dropout(leaves, types, layer, p, _word_tensor(word), blocks)
    assert outs[1].data_ptr() == buf[16:].data_ptr() and outs[2].data_ptr() != buf.data_ptr()
    facs = [torch.from_numpy(R.factor(word, layer, t, n, p)) for t, n in zip(types, counts)]
    for x, leaf, o, t in zip(xs, leaves, outs, types):
        assert torch.equal(o.detach().cpu(), torch.from_numpy(R.apply(x.numpy(), word, layer, t, p)))
        assert torch.equal(leaf.detach().cpu(), x)
    assert torch.equal(buf[16:276].cpu(), outs[1].detach().cpu()) and float(buf[:16].abs().sum()) == 0.0
    torch.autograd.backward([outs[0], outs[1]], [gs_[0].cuda(), gs_[1].cuda()])     # (the third output has no gradient)
    torch.cuda.synchronize()
    for k in (0, 1):
        assert torch.equal(leaves[k].grad.cpu(), facs[k] * gs_[k])                  # one float32 multiply, or exactly 0
    assert leaves[2].grad is None
    with pytest.raises(ValueError):
        ops.hidden_dropout(leaves, types, layer, 1.0, _word_tensor(word))


# ------------------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------------------
ROUTES = {
    'gat-sum': dict(backbone='GAT', aggr='sum'),
    'gat-mean': dict(backbone='GAT', aggr='mean'),        # (dropped after the 1 / R scale)
    'gat-max': dict(backbone='GAT', aggr='max'),
    'gat-heads2': dict(backbone='GAT', aggr='sum', heads=2),
    'gat-sigmoid': dict(backbone='GAT', aggr='sum', kw=dict(gat_sigmoid=True)),
    'sage-sum': dict(backbone='SAGE', aggr='sum'),
    'gat-3layers': dict(backbone='GAT', aggr='sum', layers=3),
}


def _model(kg, route, p, seed=3):
    from kgwas_amd.model import HeteroGNN
    r = ROUTES[route]
    torch.manual_seed(seed)
    dims = (kg.snp_init_dim_size, kg.gene_init_dim_size, kg.go_init_dim_size)
    model = HeteroGNN(kg.data, 128, 1, r.get('layers', 2), r['backbone'], r['aggr'], *dims, r.get('heads', 1), gat_split_heads=True,
                      gnn_dropout=p, **r.get('kw', {})).cuda()
    with torch.no_grad():
        for pack in list(model.live_packs) + list(model.dead_packs):
            pack.bias.normal_(0, 0.1)
        model.lin.bias.fill_(0.5)            # (an open read-out ReLU for most seeds: every parameter gets a gradient)
    return model


def _oracle(model):
    if model.heads > 1:
        from tests.multihead_ref import oracle_with_heads
        return oracle_with_heads(model)
    if model.gat_sigmoid:
        from tests.sigmoid_gate_ref import gated_oracle
        return gated_oracle(model)
    return oracle_from_product(model)


def _batch(kg, layers=2):
    from kgwas_amd.sampler import NeighborLoader
    ids = np.random.default_rng(0).choice(kg.data['SNP'].x.shape[0], size=BS, replace=False)
    return next(iter(NeighborLoader(kg.data, [-1] * layers, ('SNP', ids), batch_size=BS, device='cuda:0', seed=5)))


def _labels(kg):
    g = torch.Generator().manual_seed(9)
    n = kg.data['SNP'].x.shape[0]
    return kg.data['SNP'].y.cuda(), (torch.rand(n, generator=g, dtype=torch.float64) + 0.5).cuda()


@pytest.mark.parametrize('route', list(ROUTES))
def test_model_training_forward_backward_matches_the_masked_oracle(small_kg, route):
    """forward_loss + backward (the trainer's path) and forward (the reference-shaped one) in training mode with a set word,
    against the float64 oracle whose hidden state carries the twin's masks."""
    from kgwas_amd import ops
    p, word = 0.25, R.dropout_word(5, 1, 2)
    model = _model(small_kg, route, p)
    L = model.num_layers
    if route == 'gat-sum':
        assert model.fold_fc
    batch = _batch(small_kg, L)
    if model.gat_sigmoid:                    # (gated sums are not normalised by degree: keep most read-outs open)
        from tests.test_gpu_sigmoid_gate_model import _open_readout
        _open_readout(model, batch, BS)
    y_all, w_all = _labels(small_kg)
    model.train()
    model.set_dropout_word(word)
    model.zero_grad(set_to_none=True)
    n_id = batch.n_id('SNP')
    loss, pred = model.forward_loss(batch.x_dict, batch.edge_index_dict, BS, n_id, y_all, w_all, unit_grad=True)
    loss.backward(gradient=ops.unit_gradient(loss.device))
    with torch.no_grad():
        out = model(batch.x_dict, batch.edge_index_dict, BS)                      # training mode: it drops too, the same masks

    oracle = _oracle(model)
    fac, n_dropped = R.state_factors(model, batch, word, p)
    assert sorted(fac) == list(range(1, L)) and n_dropped > 100
    if L == 3:                               # two sites, other masks: the same rows of a type are not dropped alike
        name = next(n for n in fac[1] if n in fac[2])
        k = min(int((fac[1][name] != 1).any(1).sum()), int((fac[2][name] != 1).any(1).sum()))
        assert k > 0 and not torch.equal(fac[1][name][:k], fac[2][name][:k])
    R.DroppedStateOracle.adopt(oracle, fac)
    x, ei = batch_cpu(batch)
    out_o = oracle(x, ei, BS).reshape(-1)
    ids = n_id[:BS].long().cpu()
    yy, ww = y_all.cpu().double()[ids], w_all.cpu().double()[ids]
    loss_o = torch.mean(ww * (out_o - yy) ** 2)
    loss_o.backward()
    print(f'{route}: {n_dropped} dropped elements; pred max abs err '
          f'{float((pred.detach().cpu().double().reshape(-1) - out_o.detach()).abs().max()):.3e}, max |ref| {float(out_o.detach().abs().max()):.3e}; '
          f'loss {float(loss.detach()):.9f} vs {float(loss_o.detach()):.9f}')
    assert float((out_o.detach() > 0).double().mean()) > 0.5, 'most seeds must sit on the open side of the read-out ReLU'
    assert_close(pred.reshape(-1), out_o.detach(), RTOL, ATOL, 'pred (forward_loss)')
    assert_close(out.reshape(-1), out_o.detach(), RTOL, ATOL, 'pred (forward)')
    assert_close(loss.detach(), loss_o.detach(), RTOL, ATOL, 'loss')
    go = grads_by_name(oracle)
    n_live = 0
    for name, g in grads_by_name(model).items():
        ref = go[name]
        if g is None:
            assert ref is None or float(ref.abs().max()) == 0.0, f'{name}: product has no grad, oracle has'
            continue
        n_live += 1
        assert tuple(g.shape) == tuple(ref.shape), (name, g.shape, ref.shape)
        assert_close(g, ref, RTOL, max(ATOL, 1e-4 * float(ref.abs().max())), f'grad {name}')
    assert n_live > 10
    # the unmasked oracle is a different function: the masks are really applied
    oracle.state_factor = None
    with torch.no_grad():
        diff = float((oracle(x, ei, BS).reshape(-1) - out_o).abs().max())
    print(f'{route}: the unmasked oracle differs by {diff:.3e}')
    assert diff > 1e-3

    # eval mode never drops: the bits of a gnn_dropout = 0 model holding the same weights
    twin = _model(small_kg, route, 0.0)
    twin.load_state_dict(model.state_dict())
    model.eval(); twin.eval()
    with torch.no_grad():
        a, ha = model(batch.x_dict, batch.edge_index_dict, BS, return_h=True)
        b, hb = twin(batch.x_dict, batch.edge_index_dict, BS, return_h=True)
    assert torch.equal(a, b) and torch.equal(ha, hb) and float(ha.abs().sum()) > 0
    # ... and neither do the attention queries of a model left in training mode
    if model.backbone == 'GAT' and model.heads == 1:
        model.train(); twin.train()
        qs = list(zip(model.hot_path_attention(batch), twin.hot_path_attention(batch)))
        assert len(qs) == L
        for qa, qb in qs:
            assert torch.equal(qa, qb)


def _train_pass(model, batch, y_all, w_all):
    from kgwas_amd import ops
    model.train()
    model.zero_grad(set_to_none=True)
    loss, pred = model.forward_loss(batch.x_dict, batch.edge_index_dict, BS, batch.n_id('SNP'), y_all, w_all, unit_grad=True)
    loss.backward(gradient=ops.unit_gradient(loss.device))
    torch.cuda.synchronize()
    return loss.detach().clone(), pred.detach().clone(), {n: g.clone() for n, g in grads_by_name(model).items() if g is not None}


def test_the_default_model_is_unchanged(small_kg):
    """gnn_dropout = 0 (given or left out) in training mode: loss, predictions and every gradient bit for bit those of the same
    pass again and of a model built without the keyword."""
    from kgwas_amd.model import HeteroGNN
    batch = _batch(small_kg)
    y_all, w_all = _labels(small_kg)
    a = _model(small_kg, 'gat-sum', 0.0)
    dims = (small_kg.snp_init_dim_size, small_kg.gene_init_dim_size, small_kg.go_init_dim_size)
    b = HeteroGNN(small_kg.data, 128, 1, 2, 'GAT', 'sum', *dims, 1).cuda()
    b.load_state_dict(a.state_dict())
    assert a.gnn_dropout == 0.0 == b.gnn_dropout and a._hidden_dropout() is None
    a.set_dropout_word(WORDS[1])                                        # (nobody reads it)
    ra, ra2, rb = _train_pass(a, batch, y_all, w_all), _train_pass(a, batch, y_all, w_all), _train_pass(b, batch, y_all, w_all)
    for other in (ra2, rb):
        assert torch.equal(ra[0], other[0]) and torch.equal(ra[1], other[1]) and sorted(ra[2]) == sorted(other[2])
        for n in ra[2]:
            assert torch.equal(ra[2][n], other[2][n]), n
    assert len(ra[2]) > 10 and float(ra[0]) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# trainer: the captured step and the eager loop draw the same masks
# ------------------------------------------------------------------------------------------------------------------------------
def _launches_of_one_step(gs):
    """Kernel launches of one training step issued eagerly through the body the trainer captured (tests/helpers.py):
    (all, the k_hidden_dropout among them)."""
    names = launches_of_one_step(gs)
    return len(names), sum(1 for n in names if 'k_hidden_dropout' in n)


def test_captured_step_equals_eager_loop(tiny_kg):
    """KGWAS.train's two loops, three steps each at gnn_dropout = 0.25: the eager one sets model.drop_word from
    dropout_word(seed, epoch, step) before every train_step, the captured one copies the same word in ahead of the replay.  The
    step keeps the FC_output fold and the fused optimiser launch."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader, dropout_word
    bs, nsteps, seed = 32, 3, 11
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * 3])
    run_e = KGWAS(tiny_kg, device='cuda:0', seed=seed)
    run_e.initialize_model(gnn_dropout=0.25)
    run_g = KGWAS(tiny_kg, device='cuda:0', seed=seed)
    run_g.initialize_model(gnn_dropout=0.25)
    with torch.no_grad():
        run_e.model.lin.bias.fill_(0.5)      # (an open read-out ReLU: every parameter gets a gradient)
    run_g.model.load_state_dict(run_e.model.state_dict())
    p0 = params_by_name(run_e.model)
    run_g.model.eval()                                    # (the trainer captures a TRAINING step whatever the mode, and restores it)
    gs = GraphTrainStep(run_g, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=seed)
    assert gs.hidden_dropout and not gs.dropout and gs.fused_adam and run_g.model.fold_fc
    assert gs.n_batches == 3 and not run_g.model.training
    for n, p in params_by_name(run_g.model).items():
        assert torch.equal(p, p0[n]), n
    opt = torch.optim.Adam(run_e.model.parameters(), lr=1e-3, weight_decay=5e-4)
    ld_w = run_e._ld_weight_vector()
    run_e.model.train()
    run_g.model.train()
    plain = []
    for step, batch in enumerate(NeighborLoader(tiny_kg.data, [-1, -1], ('SNP', ids), batch_size=bs, drop_last=True, device='cuda:0')):
        if step == 0:                                     # what the step's loss would be without dropout: the masks matter
            run_e.model.eval()
            with torch.no_grad():
                plain.append(run_e.model.forward_loss(batch.x_dict, batch.edge_index_dict, bs, batch.n_id('SNP'), batch.dg.y['SNP'],
                                                      ld_w)[0].clone())
            run_e.model.train()
        run_e.model.set_dropout_word(dropout_word(seed, 0, step))
        le = run_e.train_step(batch, opt, ld_w)
        lg = gs.step(step)
        print(f'step {step}: eager {float(le.detach()):.9f} captured {float(lg.detach()):.9f}')
        if step == 0:
            print(f'step 0 without dropout: {float(plain[0]):.9f}')
            assert abs(float(le.detach()) - float(plain[0])) > 1e-6 * abs(float(plain[0]))
        assert_close(lg.detach().clone(), le.detach(), 1e-5, 1e-7, f'loss step {step}')
    gs.check()
    assert step == nsteps - 1 and gs.epoch == 1          # (the wrap after the last batch moved on to the next epoch's words)
    assert gs.fused_adam                                 # (the warm-up did not switch the fused optimiser launch off)
    pe, pg = params_by_name(run_e.model), params_by_name(run_g.model)
    num = sum(float((pe[n] - pg[n]).pow(2).sum()) for n in pe)
    den = sum(float((pe[n] - p0[n]).pow(2).sum()) for n in pe)
    print(f'relative update difference {(num / den) ** 0.5:.3e}')
    assert den > 0 and (num / den) ** 0.5 < 5e-3, f'relative update difference {(num / den) ** 0.5:.3e}'


def test_the_feature_adds_two_launches_and_the_default_step_has_none(tiny_kg):
    """Kernel launches of one eager step (the profiler's count, as tools/bench_edge_attr.py takes it): a gnn_dropout = 0 model
    issues no k_hidden_dropout, and p > 0 adds exactly the two k_hidden_dropout launches of the one site of a two-layer model and
    nothing else.  (The 26 launches of the default step are a property of the benchmark graph, which is too large for a test:
    tools/bench_hidden_dropout.py records them, profiles/hidden_dropout/bench_hidden_dropout.jsonl.)"""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    bs = 32
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * 2])
    counts = {}
    for what in ('p = 0', 'p = 0.25'):
        run = KGWAS(tiny_kg, device='cuda:0', seed=7)
        run.initialize_model(gnn_dropout=0.0 if what == 'p = 0' else 0.25)
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=7)
        assert gs.fused_adam and run.model.fold_fc and gs.hidden_dropout == (what == 'p = 0.25')
        counts[what] = _launches_of_one_step(gs)
        print(f'{what}: {counts[what][0]} kernel launches, {counts[what][1]} of them k_hidden_dropout')
    assert counts['p = 0'][1] == 0 and counts['p = 0'][0] > 10
    assert counts['p = 0.25'] == (counts['p = 0'][0] + 2, 2)


def test_second_epoch_draws_other_masks_on_the_same_cached_batch(tiny_kg):
    """lr = 0: the parameters stand still, so whatever changes the loss of step 0 between two epochs is the masks; naming epoch 0
    again gives epoch 0's bits back.  BatchCache stays on: the batches are the same, only the words change."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    bs = 32
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * 3])
    run = KGWAS(tiny_kg, device='cuda:0', seed=5)
    run.initialize_model(gnn_dropout=0.25)
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)
    sd0 = params_by_name(run.model)
    gs = GraphTrainStep(run, ('SNP', ids), bs, lr=0.0, weight_decay=0.0, cache_batches=True, sample_seed=5)
    assert gs.cache is not None and gs.hidden_dropout and not gs.dropout
    run.model.train()
    first = [gs.step(i).detach().clone() for i in range(3)]
    assert gs.epoch == 1
    second = [gs.step(i).detach().clone() for i in range(3)]
    gs.set_epoch(0)
    again = gs.step(0).detach().clone()
    gs.check()
    for k, v in params_by_name(run.model).items():
        assert torch.equal(v, sd0[k]), k
    assert all(gs.cache.filled) and gs.cache.restored >= 3
    for a, b in zip(first, second):
        assert float(a) > 0 and abs(float(a) - float(b)) > 1e-6 * abs(float(a)), (float(a), float(b))
    assert torch.equal(again, first[0])


@pytest.mark.parametrize('case', ['plain', 'fanout-shuffle', 'eager-sage-mean'])
def test_train_two_epochs_end_to_end(tiny_kg, case):
    """KGWAS.train(epoch=2) with a gnn_dropout model: the captured step with its word copies (or the eager loop), evaluation (which
    never drops), the saved model and the result table -- alone, beside a finite fan-out and a shuffled order, and on SAGE / mean."""
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(tiny_kg, device='cuda:0', seed=3)
    run.initialize_model(gnn_dropout=0.2, **(dict(gnn_backbone='SAGE', gnn_aggr='mean') if case == 'eager-sage-mean' else {}))
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)
    name = 'hidden_dropout_e2e_' + case
    kw = {'plain': {}, 'fanout-shuffle': dict(num_neighbors=[10, 5], shuffle=True), 'eager-sage-mean': dict(use_graph=False)}[case]
    run.train(batch_size=32, epoch=2, save_best_model=True, save_name=name, **kw)
    assert np.isfinite(run.val_metrics['mse']) and np.isfinite(run.val_metrics['pearsonr'])
    assert run.config['gnn_dropout'] == 0.2 and run.kgwas_res is not None and len(run.kgwas_res) > 0
    assert os.path.exists(os.path.join(tiny_kg.data_path, 'model_pred', 'new_experiments', name + '_pred.csv'))
    assert os.path.exists(os.path.join(tiny_kg.data_path, 'model', name, 'config.pkl'))
    run2 = KGWAS(tiny_kg, device='cuda:0', seed=4)
    run2.load_pretrained(os.path.join(tiny_kg.data_path, 'model', name))
    assert run2.config == run.config and run2.model.gnn_dropout == 0.2
