"""-m gpu: attention dropout (gat_aggregate(dropout=(p, word)), HeteroGNN(gat_dropout=p)) -- the DROP instantiations of k_agg_fwd
and k_agg_bwd_dst against a float64 masked restatement whose mask comes from the numpy twin of the rule
(tests/attn_dropout_ref.py), on the degree ladder of tests/test_gpu_aggregate_parity.py: 64-edge blocks, groups of 8 with tails of
4 and 2 in both halves, 128-edge chunks, the two-chunk hub and the 8-chunk row.

Tolerances as tests/test_gpu_aggregate_parity.py (rtol 1e-4, atol 1e-5 -- dH 2e-5, dU / dV / d logit_bias 1e-4 -- and
assert_close's rel_to_max).  dV and d logit_bias hang on d a_dst alone, a cancellation residue wherever a row's logits sit on one
branch of the leaky ReLU: where they miss the element-wise bound they must lie within 2 x the error of the same restatement run in
float32."""
import numpy as np
import pytest
import torch

from oracle.gat_oracle import edge_key, weighted_mse
from tests import attn_dropout_ref as R
from tests.helpers import assert_close, batch_cpu, grads_by_name, oracle_from_product, params_by_name
from tests.test_gpu_aggregate_parity import (ATOL, RTOL, _check_residue, _inputs, batches, ladder, layer_edges,  # noqa: F401
                                             realised_structure)

pytestmark = pytest.mark.gpu

WORDS = [R.dropout_word(0, 0, 0), R.dropout_word(42, 3, 17)]
GRAPHS = [('ladder_full', 1), ('ladder_full', 2), ('ladder_mini', 1), ('ladder_mini', 2)]
GRAPH_IDS = [f'{g}-L{l}' for g, l in GRAPHS]


def _word_tensor(word):
    return torch.tensor([word - (1 << 64) if word >> 63 else word], dtype=torch.int64, device='cuda:0')


def _run_gpu(batch, layer, H, U, V, kap, G, relu_input=False, dropout=None):
    """Forward and backward of ops.gat_aggregate; ``dropout`` = (p, 64-bit word) or None."""
    from kgwas_amd import ops
    m, sc = batch.meta, batch.dg.schema
    z_rows = int(m.z_base[layer - 1][sc.NT])
    n_edges = int(m.n_edges[layer - 1])
    Hd, Ud, Vd = (t.cuda().requires_grad_(True) for t in (H, U, V))
    kd = kap.cuda().requires_grad_(True) if kap is not None else None
    drop = (dropout[0], _word_tensor(dropout[1])) if dropout is not None else None
    Z, stat, e_edge = ops.gat_aggregate(batch, layer, Hd, Ud, Vd, relu_input=relu_input, logit_bias=kd, dropout=drop)
    alpha = ops.edge_alpha(batch, layer, stat, e_edge)
    (Z * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    return dict(Z=Z.detach().cpu(), stat=stat[:z_rows].cpu(), e=e_edge[:n_edges].cpu(), alpha=alpha.cpu(),
                dH=Hd.grad.cpu(), dU=Ud.grad.cpu(), dV=Vd.grad.cpu(), dlb=kd.grad.cpu() if kd is not None else None)


def _factor(batch, layer, word, p):
    return R.factor(word, layer, int(batch.meta.n_edges[layer - 1]), p)


@pytest.mark.parametrize('opts', [(0, 0), (1, 1)], ids=['plain', 'relu-lb'])
@pytest.mark.parametrize('wi', [0, 1], ids=['word0', 'word1'])
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('graph,layer', GRAPHS, ids=GRAPH_IDS)
def test_float64_parity(batches, graph, layer, p, wi, opts):
    batch = batches(graph)
    sc, dg = batch.dg.schema, batch.dg
    relu_input, lbias = map(bool, opts)
    word = WORDS[wi]
    H, U, V, kap, G = _inputs(batch, layer, seed=500 + 10 * layer + wi, relu_input=relu_input, lbias=lbias)
    edges = layer_edges(batch, layer)
    mf = _factor(batch, layer, word, p)
    got = _run_gpu(batch, layer, H, U, V, kap, G, relu_input, (p, word))
    ref = R.masked_grads(batch, layer, H, U, V, kap, G, edges, mf, torch.float64, relu_input=relu_input)
    cache = {}

    def lazy32():
        if not cache:
            cache.update(R.masked_grads(batch, layer, H, U, V, kap, G, edges, mf, torch.float32, relu_input=relu_input))
        return cache

    live = [r for r in range(sc.NR) if dg.kg.rel_live[layer - 1][r]]
    dead = [r for r in range(sc.NR) if not dg.kg.rel_live[layer - 1][r]]
    eid = torch.cat([edges[r][0] for r in edges])
    kept = float((mf[eid] > 0).double().mean())
    print(f'{graph} L{layer} p {p}: {eid.numel()} edges, kept {kept:.4f}, rows with every edge dropped {int(ref["all_dropped"].sum())}')
    for k, atol in (('Z', ATOL), ('dH', 2e-5), ('dU', 1e-4)):
        a, b = (got[k][live], ref[k][live]) if k == 'dU' else (got[k], ref[k])
        print(f'{k}: max abs err {float((a.double() - b).abs().max()):.3e}, max |ref| {float(b.abs().max()):.3e}')
    assert_close(got['Z'], ref['Z'], RTOL, ATOL, 'Z')
    # rows without an edge are never written, rows whose edges are all dropped sum zeros: exactly zero, as in PyG
    assert float(got['Z'][~ref['has']].abs().sum()) == 0.0
    if p == 0.5:
        assert bool(ref['all_dropped'].any()), 'the ladder has degree-1 and degree-2 rows: some lose every edge at p = 0.5'
    assert float(got['Z'][ref['all_dropped']].abs().sum()) == 0.0
    assert_close(got['dU'][live], ref['dU'][live], RTOL, 1e-4, 'dU')
    assert_close(got['dH'], ref['dH'], RTOL, 2e-5, 'dH')
    if relu_input:
        assert bool((H == 0).any()) and float(got['dH'][H == 0].abs().max()) == 0.0
    _check_residue('dV', got['dV'][live], ref['dV'][live], lambda: {'dV': lazy32()['dV'][live]}, 1e-4)
    assert float(got['dU'][dead].abs().sum()) == 0.0 and float(got['dV'][dead].abs().sum()) == 0.0
    if lbias:
        _check_residue('dlb', got['dlb'][live], ref['dlb'][live], lambda: {'dlb': lazy32()['dlb'][live]}, 1e-4)
        assert float(got['dlb'][dead].abs().sum()) == 0.0


@pytest.mark.parametrize('graph,layer', GRAPHS, ids=GRAPH_IDS)
def test_softmax_statistics_are_untouched(batches, graph, layer):
    """stat (row max, denominator), e_edge and ops.edge_alpha describe the undropped softmax: the bits of the dropout=None run."""
    batch = batches(graph)
    H, U, V, kap, G = _inputs(batch, layer, seed=61, lbias=True)
    a = _run_gpu(batch, layer, H, U, V, kap, G)
    b = _run_gpu(batch, layer, H, U, V, kap, G, dropout=(0.5, WORDS[0]))
    for k in ('stat', 'e', 'alpha'):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a['Z'], b['Z'])


@pytest.mark.parametrize('graph,layer', GRAPHS, ids=GRAPH_IDS)
def test_p_zero_takes_the_dropout_kernels_and_gives_the_plain_bits(batches, graph, layer):
    """dropout=(0.0, word) selects the DROP instantiations with thresh 0 and scale 1.0f: every output bit for bit the plain one's."""
    batch = batches(graph)
    H, U, V, kap, G = _inputs(batch, layer, seed=62, relu_input=True, lbias=True)
    a = _run_gpu(batch, layer, H, U, V, kap, G, relu_input=True)
    b = _run_gpu(batch, layer, H, U, V, kap, G, relu_input=True, dropout=(0.0, WORDS[1]))
    for k in ('Z', 'stat', 'e', 'dH', 'dU', 'dV', 'dlb'):
        assert torch.equal(a[k], b[k]), k
    assert float(a['Z'].abs().sum()) > 0 and float(a['dV'].abs().sum()) > 0


def test_deterministic_in_the_word_and_different_across_words_and_layers(batches):
    batch = batches('ladder_mini')
    H, U, V, kap, G = _inputs(batch, 1, seed=63, lbias=True)
    a = _run_gpu(batch, 1, H, U, V, kap, G, dropout=(0.25, WORDS[0]))
    b = _run_gpu(batch, 1, H, U, V, kap, G, dropout=(0.25, WORDS[0]))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    c = _run_gpu(batch, 1, H, U, V, kap, G, dropout=(0.25, WORDS[1]))
    assert not torch.equal(a['Z'], c['Z'])
    # layers 1 and 2 drop different edge sets (the twin's masks over the edges both layers have), and the kernels follow the
    # twin in each: layer 2 run with layer 1's mask as reference must NOT match
    n2 = int(batch.meta.n_edges[1])
    k1, k2 = R.keep(WORDS[0], 1, np.arange(n2), 0.25), R.keep(WORDS[0], 2, np.arange(n2), 0.25)
    assert not np.array_equal(k1, k2) and 0.3 < float((k1 == k2).mean()) < 0.95
    H2, U2, V2, kap2, G2 = _inputs(batch, 2, seed=64)
    edges = layer_edges(batch, 2)
    got = _run_gpu(batch, 2, H2, U2, V2, kap2, G2, dropout=(0.25, WORDS[0]))
    right = R.masked_grads(batch, 2, H2, U2, V2, kap2, G2, edges, _factor(batch, 2, WORDS[0], 0.25), torch.float64)
    wrong = R.masked_grads(batch, 2, H2, U2, V2, kap2, G2, edges, _factor(batch, 1, WORDS[0], 0.25)[:n2], torch.float64)
    assert_close(got['Z'], right['Z'], RTOL, ATOL, 'Z (layer 2, layer 2 mask)')
    assert float((got['Z'].double() - wrong['Z']).abs().max()) > 1e-2


def test_refused_combinations(batches):
    from kgwas_amd import _lib, ops
    batch = batches('ladder_mini')
    H, U, V, _, _ = _inputs(batch, 1, seed=65)
    w = _word_tensor(WORDS[0])
    with pytest.raises(ValueError):
        ops.gat_aggregate(batch, 1, H.cuda(), U.cuda(), V.cuda(), raw_weights=True, dropout=(0.1, w))
    with pytest.raises(ValueError):
        ops.gat_aggregate(batch, 1, H.cuda(), U.cuda(), V.cuda(), dropout=(1.0, w))
    # the C ABI refuses before any launch: raw-logit weights, partial softmax states, a scale below 1
    a = ops._layer_args(batch, 1, 0.2, 1.0)
    a.drop_word_dev, a.drop_thresh, a.drop_scale = w.data_ptr(), 1 << 31, 2.0
    L = _lib.lib()
    import ctypes as C
    a.flags = 1
    assert L.kgw_gat_aggregate_fwd(C.byref(a), _lib.stream_ptr()) == _lib.KGW_E_UNSUPPORTED
    a.flags, a.partial_rels = 0, 1
    assert L.kgw_gat_aggregate_fwd(C.byref(a), _lib.stream_ptr()) == _lib.KGW_E_UNSUPPORTED
    assert L.kgw_gat_aggregate_bwd_dst(C.byref(a), _lib.stream_ptr()) == _lib.KGW_E_UNSUPPORTED
    a.partial_rels = 0
    for bad in (0.5, float('inf'), float('nan')):
        a.drop_scale = bad
        assert L.kgw_gat_aggregate_fwd(C.byref(a), _lib.stream_ptr()) == -2        # KGW_E_RANGE
        assert L.kgw_gat_aggregate_bwd_dst(C.byref(a), _lib.stream_ptr()) == -2


# ------------------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------------------
def test_model_training_forward_backward_matches_the_masked_oracle(small_kg):
    from kgwas_amd.model import HeteroGNN
    from kgwas_amd.sampler import NeighborLoader
    data = small_kg.data
    dims = (small_kg.snp_init_dim_size, small_kg.gene_init_dim_size, small_kg.go_init_dim_size)
    p, word = 0.25, R.dropout_word(5, 1, 2)
    torch.manual_seed(3)
    model = HeteroGNN(data, 128, 1, 2, 'GAT', 'sum', *dims, 1, gat_dropout=p).cuda()
    with torch.no_grad():
        for pack in list(model.live_packs) + list(model.dead_packs):
            pack.bias.normal_(0, 0.1)
    ids = np.random.default_rng(0).choice(data['SNP'].x.shape[0], size=48, replace=False)
    batch = next(iter(NeighborLoader(data, [-1, -1], ('SNP', ids), batch_size=48, device='cuda:0')))
    model.train()
    model.set_dropout_word(word)
    out = model(batch.x_dict, batch.edge_index_dict, 48)
    y = torch.rand(48, dtype=torch.float64)
    w = torch.rand(48, dtype=torch.float64) + 0.5
    loss = weighted_mse(out, y.cuda(), w.cuda())
    loss.backward()

    oracle = oracle_from_product(model)
    x, ei = batch_cpu(batch)
    n_masked = 0
    for l in (1, 2):
        edges = layer_edges(batch, l)
        fac = _factor(batch, l, word, p)
        for r, et in enumerate(model.edge_types):
            conv = R.MaskedGATConvOracle.adopt(oracle.convs[l - 1].convs[edge_key(et)])
            f = torch.ones(ei[et].shape[1], dtype=torch.float64)       # (rows the product prunes by hop, dead relations: all kept --
            if r in edges:                                             #  they carry no gradient and reach no seed)
                eid, src, dst = edges[r]
                assert torch.equal(ei[et][:, :eid.numel()], torch.stack([src, dst]))
                f[:eid.numel()] = fac[eid]
                n_masked += int((fac[eid] == 0).sum())
            conv.edge_factor = f
    assert n_masked > 100
    out_o = oracle(x, ei, 48)
    loss_o = weighted_mse(out_o, y, w)
    loss_o.backward()
    assert_close(out, out_o.detach(), RTOL, ATOL, 'pred')
    assert_close(loss.detach(), loss_o.detach(), RTOL, ATOL, 'loss')
    go = grads_by_name(oracle)
    n_live = 0
    for name, g in grads_by_name(model).items():
        ref = go[name]
        if g is None:
            assert ref is None or float(ref.abs().max()) == 0.0, f'{name}: product has no grad, oracle has'
            continue
        n_live += 1
        assert_close(g, ref, RTOL, max(ATOL, 1e-4 * float(ref.abs().max())), f'grad {name}')
    assert n_live > 10
    # the unmasked oracle is a different function: the masks are really applied
    plain = oracle_from_product(model)
    with torch.no_grad():
        assert float((plain(x, ei, 48) - out_o).abs().max()) > 1e-3

    # eval mode never drops: the bits of a gat_dropout = 0 model holding the same weights
    twin = HeteroGNN(data, 128, 1, 2, 'GAT', 'sum', *dims, 1).cuda()
    twin.load_state_dict(model.state_dict())
    model.eval(); twin.eval()
    with torch.no_grad():
        a, ha = model(batch.x_dict, batch.edge_index_dict, 48, return_h=True)
        b, hb = twin(batch.x_dict, batch.edge_index_dict, 48, return_h=True)
    assert torch.equal(a, b) and torch.equal(ha, hb) and float(ha.abs().sum()) > 0
    # ... and neither do the attention queries of a model left in training mode
    model.train(); twin.train()
    for qa, qb in zip(model.hot_path_attention(batch), twin.hot_path_attention(batch)):
        assert torch.equal(qa, qb)


# ------------------------------------------------------------------------------------------------------------------------------
# trainer: the captured step and the eager loop draw the same masks
# ------------------------------------------------------------------------------------------------------------------------------
def test_captured_step_equals_eager_loop(tiny_kg):
    """KGWAS.train's two loops, three steps each at gat_dropout = 0.25: the eager one sets model.drop_word from
    dropout_word(seed, epoch, step) before every train_step, the captured one copies the same word in ahead of the replay.  The
    bar is test_gpu_graph.py::test_graph_step_equals_eager's (losses rtol 1e-5 / atol 1e-7, relative update difference 5e-3):
    captured and eager are not bit-equal at p = 0 either (padded GEMMs tile differently)."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader, dropout_word
    bs, nsteps, seed = 32, 3, 11
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * 3])
    run_e = KGWAS(tiny_kg, device='cuda:0', seed=seed)
    run_e.initialize_model(gat_dropout=0.25)
    run_g = KGWAS(tiny_kg, device='cuda:0', seed=seed)
    run_g.initialize_model(gat_dropout=0.25)
    run_g.model.load_state_dict(run_e.model.state_dict())
    p0 = params_by_name(run_e.model)
    run_g.model.eval()                                    # (the trainer captures a TRAINING step whatever the mode, and restores it)
    gs = GraphTrainStep(run_g, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=seed)
    assert gs.dropout and gs.n_batches == 3 and not run_g.model.training
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
            # (the float64 loss is dominated by the labels here: the masks move it by ~1e-4 of itself, float32 rounding of
            #  the predictions by ~1e-7)
            assert abs(float(le.detach()) - float(plain[0])) > 1e-6 * abs(float(plain[0]))
        assert_close(lg.detach().clone(), le.detach(), 1e-5, 1e-7, f'loss step {step}')
    gs.check()
    assert step == nsteps - 1 and gs.epoch == 1          # (the wrap after the last batch moved on to the next epoch's words)
    pe, pg = params_by_name(run_e.model), params_by_name(run_g.model)
    num = sum(float((pe[n] - pg[n]).pow(2).sum()) for n in pe)
    den = sum(float((pe[n] - p0[n]).pow(2).sum()) for n in pe)
    assert den > 0 and (num / den) ** 0.5 < 5e-3, f'relative update difference {(num / den) ** 0.5:.3e}'


def test_second_epoch_draws_other_masks_on_the_same_cached_batch(tiny_kg):
    """lr = 0: the parameters stand still, so whatever changes the loss of step 0 between two epochs is the masks; naming epoch 0
    again gives epoch 0's bits back.  BatchCache stays on: the batches are the same, only the words change."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    bs = 32
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * 3])
    run = KGWAS(tiny_kg, device='cuda:0', seed=5)
    run.initialize_model(gat_dropout=0.25)
    sd0 = params_by_name(run.model)
    gs = GraphTrainStep(run, ('SNP', ids), bs, lr=0.0, weight_decay=0.0, cache_batches=True, sample_seed=5)
    assert gs.cache is not None
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
