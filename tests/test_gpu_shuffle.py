"""-m gpu: the per-epoch order of the training seeds -- kgw_epoch_order, NeighborLoader(epoch_order=), measure_caps(epochs=),
GraphTrainStep(epoch_order=, epochs=), KGWAS.train(shuffle=) -- against the numpy twin of its rule (tests/shuffle_ref.py).
Integer work => exact comparisons; the captured step against the eager one at the bars of tests/test_gpu_graph.py."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import shuffle_ref as R
from tests.helpers import assert_close, params_by_name

pytestmark = pytest.mark.gpu

WORDS = [0, (1 << 64) - 1, R.order_word(0, 0), R.order_word(42, 3)]
MODES = {'seeds': 1, 'batches': 2}
RANKS = [(0, 1), (0, 2), (1, 2), (0, 4), (1, 4), (2, 4), (3, 4)]
PAD = 8


def _launch_edges():
    """One below, at and one above the launch's block size and its grid cap's worth of threads (kgw_epoch_order: blocks of
    EPOCH_ORDER_BLOCK threads, at most EPOCH_ORDER_GRID of them, grid-stride beyond)."""
    from kgwas_amd import _lib
    blk, cap = _lib.EPOCH_ORDER_BLOCK, _lib.EPOCH_ORDER_BLOCK * _lib.EPOCH_ORDER_GRID
    return [blk - 1, blk, blk + 1], [cap - 1, cap, cap + 1]


def _call(ids, n, B, mode, rank, world, word, out):
    from kgwas_amd import _lib
    return _lib.lib().kgw_epoch_order(C.c_void_p(ids.data_ptr()), n, B, mode, rank, world, word, C.c_void_p(out.data_ptr()),
                                      _lib.stream_ptr())


_perms = {}


def _expected(ids, B, mode, word, rank, world):
    """The twin's answer, its permutations computed once per (word, length)."""
    n = len(ids)
    m = n if mode == 'seeds' else n // B
    if m and (word, m) not in _perms:
        _perms[(word, m)] = R.permutation(word, m)
    if mode == 'seeds':
        pos = _perms[(word, n)]
    else:
        pos = np.arange(n, dtype=np.int64)
        if m:
            pos[:m * B] = (_perms[(word, m)][:, None] * B + np.arange(B)[None, :]).reshape(-1)
    return ids[pos[R.rank_positions(n, B, rank, world)]]


def _check_n(n, batches, rng):
    from kgwas_amd.sampler import epoch_order_len
    ids = rng.permutation(4 * n + 11)[:n].astype(np.int64) * 3 + (1 << 33)          # distinct, unordered, beyond 32 bits
    d_ids = torch.from_numpy(ids).cuda()
    n_cases = 0
    for B in batches:
        for rank, world in RANKS:
            if B % world:
                out = torch.full((n + PAD,), -1, dtype=torch.int64, device='cuda')
                assert _call(d_ids, n, B, 1, rank, world, 0, out) == -2            # KGW_E_RANGE, nothing launched
                assert bool((out == -1).all())
                continue
            total = epoch_order_len(n, B, world)
            for mode, code in MODES.items():
                for word in WORDS:
                    out = torch.full((total + PAD,), -1, dtype=torch.int64, device='cuda')
                    assert _call(d_ids, n, B, code, rank, world, word, out) == 0
                    got = out.cpu().numpy()
                    want = _expected(ids, B, mode, word, rank, world)
                    assert len(want) == total
                    assert np.array_equal(got[:total], want), (n, B, mode, hex(word), rank, world)
                    assert (got[total:] == -1).all(), 'wrote past its share'
                    n_cases += 1
            # a second call gives the same bits
            again = torch.full((total + PAD,), -1, dtype=torch.int64, device='cuda')
            assert _call(d_ids, n, B, code, rank, world, word, again) == 0 and torch.equal(again, out)
    return n_cases


SMALL_N = [1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 255, 257, 1023, 1025]


def test_epoch_order_equals_the_twin_small():
    """1. every small n and the launch's block size +- 1; B = 1, 7, 32, n and one that does not divide n; both modes; four words;
    every rank of 1, 2 and 4."""
    rng = np.random.default_rng(1)
    n_cases = 0
    for n in sorted(set(SMALL_N + _launch_edges()[0])):
        ragged = next(b for b in (3, 5, 6, 9, 2) if n % b) if n > 1 else 2
        n_cases += _check_n(n, [1, 7, 32, n, ragged, 4 * max(1, n // 9)], rng)
    assert n_cases > 2000


@pytest.mark.parametrize('which', [0, 1, 2])
def test_epoch_order_equals_the_twin_at_the_grid_cap(which):
    """1. one below, at and one above the number of threads of the largest grid: the grid-stride loop's second trip."""
    n = _launch_edges()[1][which]
    assert _check_n(n, [1, 32, 1000, n], np.random.default_rng(2)) >= 8 * (1 + 7 + 7 + 1)


def test_epoch_order_refusals():
    """1. KGW_E_RANGE before any launch: n < 1, n > 2^31, B < 1, B % world != 0, a bad mode, a bad rank."""
    ids = torch.arange(64, dtype=torch.int64, device='cuda')
    out = torch.full((64,), -1, dtype=torch.int64, device='cuda')
    bad = [(0, 8, 1, 0, 1), (-1, 8, 1, 0, 1), ((1 << 31) + 1, 8, 1, 0, 1), (64, 0, 1, 0, 1), (64, -8, 1, 0, 1), (64, 9, 1, 0, 2),
           (64, 8, 0, 0, 1), (64, 8, 3, 0, 1), (64, 8, 1, 1, 1), (64, 8, 1, -1, 1), (64, 8, 2, 4, 4), (64, 8, 1, 0, 0)]
    for n, B, mode, rank, world in bad:
        assert _call(ids, n, B, mode, rank, world, 5, out) == -2, (n, B, mode, rank, world)
    torch.cuda.synchronize()
    assert bool((out == -1).all())
    assert _call(ids, 64, 8, 1, 0, 1, 5, out) == 0 and sorted(out.tolist()) == list(range(64))
    from kgwas_amd.sampler import epoch_order
    assert np.array_equal(epoch_order(ids, 8, 'batches', WORDS[3], 1, 2).cpu().numpy(), R.epoch_order(np.arange(64), 8, 'batches', WORDS[3], 1, 2))


# ---- loader ------------------------------------------------------------------------------------------------------------------------
def _loader(data, ids, bs, **kw):
    from kgwas_amd.sampler import NeighborLoader
    nn = kw.pop('num_neighbors', [-1, -1])
    return NeighborLoader(data, num_neighbors=nn, input_nodes=('SNP', ids), batch_size=bs, device='cuda:0', **kw)


def _bits(batch):
    n = batch.n_edges_sampled
    return (batch.n_id('SNP')[:batch.batch_size].cpu().numpy().astype(np.int64), batch.n_id('Gene').cpu().clone(),
            batch.buf.col_local[:n].cpu().clone())


@pytest.mark.parametrize('mode', ['seeds', 'batches'])
def test_loader_draws_the_twins_order(small_kg, mode):
    """2. bs = 64 over 5 full batches and a partial one: the seeds of every batch of epochs 0 and 1 are the twin's; prefetch on and
    off give identical batches; set_epoch(0) after epoch 1 gives epoch 0's bits back."""
    data, bs, seed = small_kg.data, 64, 9
    ids = np.random.default_rng(4).choice(data['SNP'].x.shape[0], size=5 * bs + 17, replace=False)
    passes = {}
    for prefetch in (True, False):
        ld = _loader(data, ids, bs, epoch_order=mode, seed=seed, prefetch=prefetch)
        assert len(ld) == 6
        for ep in (0, 1):                                                # (the second pass is the next epoch by itself)
            passes[(prefetch, ep)] = [_bits(b) for b in ld]
            assert ld.epoch == ep
        ld.set_epoch(0)
        passes[(prefetch, 'again')] = [_bits(b) for b in ld]
    for ep in (0, 1):
        want = R.epoch_order(ids, bs, mode, R.order_word(seed, ep))
        for i, (seeds, genes, col) in enumerate(passes[(True, ep)]):
            assert np.array_equal(seeds, want[i * bs:(i + 1) * bs]), (ep, i)
            assert len(seeds) == (bs if i < 5 else 17)
            other = passes[(False, ep)][i]
            assert np.array_equal(seeds, other[0]) and torch.equal(genes, other[1]) and torch.equal(col, other[2]), (ep, i)
    for prefetch in (True, False):
        for a, b in zip(passes[(prefetch, 0)], passes[(prefetch, 'again')]):
            assert np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(passes[(True, 0)], passes[(True, 1)]))
    if mode == 'batches':                                                # whole batches of the fixed order, the partial one in place
        fixed = {tuple(ids[i * bs:(i + 1) * bs]) for i in range(5)}
        for ep in (0, 1):
            assert {tuple(s) for s, _, _ in passes[(True, ep)][:5]} == fixed
            assert np.array_equal(passes[(True, ep)][5][0], ids[5 * bs:])


def test_fixed_order_is_the_loader_without_the_keyword(small_kg):
    """2. epoch_order='fixed' is the loader built without the keyword, pass after pass."""
    data, bs = small_kg.data, 64
    ids = np.random.default_rng(5).choice(data['SNP'].x.shape[0], size=3 * bs + 5, replace=False)
    a, b = _loader(data, ids, bs, epoch_order='fixed', seed=3), _loader(data, ids, bs, seed=3)
    for _ in range(2):
        for x, y in zip(a, b):
            bx, by = _bits(x), _bits(y)
            assert np.array_equal(bx[0], by[0]) and torch.equal(bx[1], by[1]) and torch.equal(bx[2], by[2])
    assert np.array_equal(np.concatenate([_bits(x)[0] for x in a]), ids)
    # several ranks: a shuffled loader takes the global ids and slices the epoch's order itself
    for r in range(2):
        ld = _loader(data, ids, bs // 2, epoch_order='seeds', seed=3, rank=r, world=2, drop_last=True)
        ld.set_epoch(1)
        got = np.concatenate([_bits(x)[0] for x in ld])
        assert len(ld) == 3 and np.array_equal(got, R.epoch_order(ids, bs, 'seeds', R.order_word(3, 1), r, 2))
    with pytest.raises(ValueError):
        _loader(data, ids, bs // 2, epoch_order='seeds', rank=0, world=2)                  # (several ranks: full batches only)


# ---- capacities ---------------------------------------------------------------------------------------------------------------------
def _maxima(batches, dg, bs):
    sc, L = dg.schema, dg.num_layers
    node_off = np.zeros((sc.NT, L + 2), dtype=np.int64)
    edges, chunks = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    for m in batches:
        for t in range(sc.NT):
            for k in range(L + 2):
                node_off[t, k] = max(node_off[t, k], int(m.node_off[t][min(k, dg.n_hops + 1)]))
        for l in range(L):
            edges[l], chunks[l] = max(edges[l], int(m.n_edges[l])), max(chunks[l], int(m.n_chunks[l]))
    return node_off, edges, chunks


def test_capacities_cover_exactly_the_batches_of_the_run(small_kg, tiny_kg):
    """3. 'seeds': measure_caps(margin=1.0, round_to=1, epochs=2) is the element-wise maximum of the batches' counts over epochs 0
    and 1 and batch 0 of epoch 2; no batch of those exceeds the default-margin capacities; 'batches' has the fixed order's
    capacities; a captured trainer built with epochs=2 refuses epoch 3 (and 2)."""
    data, bs, seed = small_kg.data, 64, 6
    ids = np.asarray(small_kg.train_input_nodes[1][:bs * 6 + 9])
    ld = _loader(data, ids, bs, epoch_order='seeds', seed=seed, drop_last=True, prefetch=False)
    ld.set_epoch(7)
    exact = ld.measure_caps(margin=1.0, round_to=1, epochs=2)
    caps = ld.measure_caps(epochs=2)
    assert ld.epoch == 7 and ld._epoch_set                               # (the dry pass leaves the loader's epoch alone)
    metas = []
    for ep in (0, 1, 2):
        ld.set_epoch(ep)
        for i, b in enumerate(ld):
            if ep < 2 or i == 0:
                metas.append(b.meta)
    assert len(metas) == 13
    node_off, edges, chunks = _maxima(metas, ld.dg, bs)
    assert np.array_equal(np.asarray(exact.node_off), node_off), (exact.node_off, node_off.tolist())
    assert list(exact.edges) == edges.tolist() and list(exact.chunks) == chunks.tolist()
    assert node_off[ld.seed_type, 1] == bs
    # what epoch 0 alone needs never exceeds what the two epochs need
    one = ld.measure_caps(margin=1.0, round_to=1, epochs=1)
    assert (np.asarray(one.node_off) <= node_off).all() and one.edges[0] <= edges[0]
    for m in metas:
        n1, e1, c1 = _maxima([m], ld.dg, bs)
        assert (n1 <= np.asarray(caps.node_off)).all() and (e1 <= np.asarray(caps.edges)).all() and (c1 <= np.asarray(caps.chunks)).all()
    # whole batches in another order: the capacities of the fixed order
    fixed = _loader(data, ids, bs, drop_last=True, prefetch=False).measure_caps()
    shuf = _loader(data, ids, bs, epoch_order='batches', seed=seed, drop_last=True, prefetch=False).measure_caps(epochs=2)
    assert (shuf.node_off, shuf.edges, shuf.chunks) == (fixed.node_off, fixed.edges, fixed.chunks)
    # a finite fan-out composes: never above the full-neighbourhood capacities of the same shuffled seeds
    fan = _loader(data, ids, bs, num_neighbors=[4, 3], epoch_order='seeds', seed=seed, drop_last=True, prefetch=False).measure_caps(epochs=2)
    assert all(a <= b for a, b in zip(fan.edges, caps.edges)) and fan.edges[0] < caps.edges[0]

    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(tiny_kg, device='cuda:0', seed=1)
    run.initialize_model()
    tids = np.asarray(tiny_kg.train_input_nodes[1][:100])
    gs = GraphTrainStep(run, ('SNP', tids), 32, epoch_order='seeds', epochs=2, sample_seed=seed)
    assert gs.n_batches == 3 and gs.epochs == 2 and gs.cache is None
    for bad in (3, 2, -1):
        with pytest.raises(ValueError):
            gs.set_epoch(bad)
    run.model.train()
    gs.set_epoch(1)
    for i in range(3):
        gs.step(i)
    gs.check()
    assert gs.epoch == 2                                                 # (moved on by itself: batch 0 of epoch 2 is sampled ahead ...)
    with pytest.raises(ValueError):
        gs.step(0)                                                       # (... and never trained on)


# ---- captured trainer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['plain', 'fanout', 'dropout'])
def test_captured_shuffled_step_equals_eager(tiny_kg, case):
    """4. bs = 32, 3 batches, 2 epochs, 'seeds': GraphTrainStep against the eager loop over NeighborLoader(epoch_order='seeds') at
    the bars of test_gpu_graph.py::test_graph_step_equals_eager (loss rtol 1e-5 / atol 1e-7, relative update difference 5e-3)."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import dropout_word
    bs, seed = 32, 13
    ids = np.asarray(tiny_kg.train_input_nodes[1][:100])                 # 3 full batches; the 4 left over differ per epoch
    nn = [4, 3] if case == 'fanout' else None
    kw = {'gat_dropout': 0.25} if case == 'dropout' else {}
    run_e = KGWAS(tiny_kg, device='cuda:0', seed=11)
    run_e.initialize_model(**kw)
    run_g = KGWAS(tiny_kg, device='cuda:0', seed=12)
    run_g.initialize_model(**kw)
    run_g.model.load_state_dict(run_e.model.state_dict())
    p0 = params_by_name(run_e.model)
    gs = GraphTrainStep(run_g, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, num_neighbors=nn, sample_seed=seed,
                        epoch_order='seeds', epochs=2, cache_batches=True)
    assert gs.n_batches == 3 and gs.cache is None
    for n, p in params_by_name(run_g.model).items():
        assert torch.equal(p, p0[n]), n
    opt = torch.optim.Adam(run_e.model.parameters(), lr=1e-3, weight_decay=5e-4)
    ld_w = run_e._ld_weight_vector()
    run_e.model.train()
    run_g.model.train()
    ld = _loader(tiny_kg.data, ids, bs, num_neighbors=nn or [-1, -1], epoch_order='seeds', seed=seed, drop_last=True)
    seen = []
    for ep in range(2):
        ld.set_epoch(ep)
        gs.set_epoch(ep)
        want = R.epoch_order(ids, bs, 'seeds', R.order_word(seed, ep))
        for i, batch in enumerate(ld):
            seeds = batch.n_id('SNP')[:bs].cpu().numpy()
            assert np.array_equal(seeds, want[i * bs:(i + 1) * bs])
            seen.append(seeds)
            if case == 'dropout':
                run_e.model.set_dropout_word(dropout_word(seed, ep, i))
            le = run_e.train_step(batch, opt, ld_w)
            lg = gs.step(i)
            print(f'epoch {ep} step {i}: eager {float(le.detach()):.9f} captured {float(lg.detach()):.9f}')
            assert_close(lg.detach().clone(), le.detach(), 1e-5, 1e-7, f'loss epoch {ep} step {i}')
    gs.check()
    assert not np.array_equal(np.concatenate(seen[:3]), np.concatenate(seen[3:]))
    pe, pg = params_by_name(run_e.model), params_by_name(run_g.model)
    num = den = 0.0
    for n in pe:
        num += float((pe[n] - pg[n]).pow(2).sum())
        den += float((pe[n] - p0[n]).pow(2).sum())
    assert den > 0 and (num / den) ** 0.5 < 5e-3, f'relative update difference {(num / den) ** 0.5:.3e}'


def test_shuffled_batches_keep_the_cache(tiny_kg):
    """5. 'batches', lr = 0, cache_batches=True: the loss of step i of epoch 1 is bit for bit the loss of the epoch-0 step that
    trained on the same batch of the fixed order -- put back from that batch's slot, not sampled again."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import epoch_order_index, order_word
    bs, nb, seed = 32, 5, 4
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * nb + 7])
    src = [[epoch_order_index(order_word(seed, ep), nb, i) for i in range(nb)] for ep in (0, 1, 2)]
    assert src[0] != src[1] and sorted(src[0]) == sorted(src[1]) == list(range(nb))
    assert [R.permutation(R.order_word(seed, ep), nb).tolist() for ep in (0, 1, 2)] == src
    run = KGWAS(tiny_kg, device='cuda:0', seed=5)
    run.initialize_model()
    gs = GraphTrainStep(run, ('SNP', ids), bs, lr=0.0, weight_decay=0.0, cache_batches=True, sample_seed=seed, epoch_order='batches')
    assert gs.cache is not None and gs.n_batches == nb and gs.epochs is None
    run.model.train()
    losses = [[gs.step(i).detach().clone() for i in range(nb)] for _ in range(3)]
    gs.check()
    assert gs.epoch == 3
    by_src = {src[0][i]: losses[0][i] for i in range(nb)}
    assert len({float(v) for v in by_src.values()}) == nb                # (the batches really differ)
    for ep in (1, 2):
        for i in range(nb):
            assert torch.equal(losses[ep][i], by_src[src[ep][i]]), (ep, i)
    assert gs.cache.saved == nb and all(gs.cache.filled) and gs.cache.restored >= 2 * nb - 1, (gs.cache.saved, gs.cache.restored)
    # the same steps with every batch sampled when it is due: the same bits
    run2 = KGWAS(tiny_kg, device='cuda:0', seed=5)
    run2.initialize_model()
    run2.model.load_state_dict(run.model.state_dict())
    gs2 = GraphTrainStep(run2, ('SNP', ids), bs, lr=0.0, weight_decay=0.0, cache_batches=False, sample_seed=seed, epoch_order='batches')
    run2.model.train()
    assert gs2.cache is None
    for ep in range(2):
        for i in range(nb):
            assert torch.equal(gs2.step(i).detach(), losses[ep][i]), (ep, i)
    gs2.check()


# ---- KGWAS.train --------------------------------------------------------------------------------------------------------------------
class _Log:
    def __init__(self):
        self.losses = []

    def log(self, d):
        if 'training_loss' in d:
            self.losses.append(d['training_loss'])


@pytest.mark.parametrize('shuffle', [True, 'batches'])
def test_train_with_a_shuffle(tiny_kg, monkeypatch, shuffle):
    """6. KGWAS.train(batch_size=32, epoch=2, shuffle=...): finite metrics, kgwas_res written; the captured trainer and the eager
    loop (use_graph=False) draw the same order, the twin's, and give the same losses."""
    from kgwas_amd import graph_step
    from kgwas_amd.kgwas import KGWAS
    mode, bs = ('seeds' if shuffle is True else 'batches'), 32
    fed, trained = {}, []
    real_feed = graph_step.GraphTrainStep._feed

    def feed(self, i, epoch):
        real_feed(self, i, epoch)
        fed[(epoch, i)] = self.seeds.clone()
    monkeypatch.setattr(graph_step.GraphTrainStep, '_feed', feed)
    real_step = KGWAS.train_step

    def train_step(self, batch, *a, **k):
        trained.append(batch.n_id('SNP')[:bs].cpu().numpy().astype(np.int64))
        return real_step(self, batch, *a, **k)
    monkeypatch.setattr(KGWAS, 'train_step', train_step)
    losses, sd0 = {}, None
    for use_graph in (True, False):
        run = KGWAS(tiny_kg, device='cuda:0', seed=21)
        run.initialize_model()
        if sd0 is None:
            sd0 = copy.deepcopy(run.model.state_dict())
        else:
            run.model.load_state_dict(sd0)
        run.wandb = _Log()
        run.train(batch_size=bs, epoch=2, save_best_model=False, save_name='shuf' + str(use_graph), use_graph=use_graph, shuffle=shuffle)
        losses[use_graph] = run.wandb.losses
        assert np.isfinite(run.val_metrics['mse']) and np.isfinite(run.val_metrics['pearsonr']) and np.isfinite(run.test_metrics['mse'])
        assert len(run.kgwas_res) > 0 and np.isfinite(np.asarray(run.kgwas_res['pred'].values)).all()
        assert run.train_loader.epoch_order == mode and run.val_loader.epoch_order == 'fixed'
        assert 'shuffle' not in run.config and 'epoch_order' not in run.config
    ids = np.asarray(tiny_kg.train_input_nodes[1], dtype=np.int64)
    per = len(ids) // bs
    assert per >= 3 and len(trained) == 2 * per == len(losses[True]) == len(losses[False])
    for ep in (0, 1):
        want = R.epoch_order(ids, bs, mode, R.order_word(21, ep))
        for i in range(per):
            assert np.array_equal(trained[ep * per + i], want[i * bs:(i + 1) * bs]), (ep, i)
            if (ep, i) in fed:
                assert np.array_equal(fed[(ep, i)].cpu().numpy(), want[i * bs:(i + 1) * bs]), (ep, i)
    if mode == 'seeds':
        assert {(e, i) for e in (0, 1) for i in range(per)} <= set(fed)
    else:
        assert {(0, i) for i in range(per)} <= set(fed) and not any(e == 1 for e, _ in fed)     # (epoch 2: every batch from its slot)
    for i in range(2 * per):
        assert_close(torch.tensor(losses[True][i]), torch.tensor(losses[False][i]), 1e-5, 1e-7, f'loss step {i}')


def test_train_without_a_shuffle_is_the_run_without_the_keyword(tiny_kg):
    """6. shuffle=False: the parameters of a run without the keyword, bit for bit."""
    from kgwas_amd.kgwas import KGWAS
    outs, sd0 = [], None
    for kw in ({}, {'shuffle': False}):
        run = KGWAS(tiny_kg, device='cuda:0', seed=22)
        run.initialize_model()
        if sd0 is None:
            sd0 = copy.deepcopy(run.model.state_dict())
        else:
            run.model.load_state_dict(sd0)
        run.train(batch_size=32, epoch=2, save_best_model=False, save_name='noshuf' + str(len(outs)), **kw)
        outs.append(({k: v.detach().clone() for k, v in run.best_model.named_reference_tensors().items()},
                     np.asarray(run.kgwas_res['pred'].values).copy()))
    for k in outs[0][0]:
        assert torch.equal(outs[0][0][k], outs[1][0][k]), k
    assert np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize('ext', ['heads', 'sigmoid', 'traits', 'edge_attr'])
def test_train_with_a_shuffle_and_the_other_extensions(tiny_kg, tmp_path, ext):
    """6. shuffle=True beside gat_num_head, gat_sigmoid, out_channels > 1 and gat_edge_dim: one epoch, the captured trainer; finite
    metrics, predictions written."""
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.kgwas_data import KGWAS_Data
    data, model_kw = tiny_kg, {'heads': {'gat_num_head': 2}, 'sigmoid': {'gat_sigmoid': True, 'gat_temperature': 2.0}}.get(ext, {})
    if ext == 'traits':
        data, model_kw = KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path), n_traits=2), {'out_channels': 2}
    elif ext == 'edge_attr':
        data, model_kw = KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path), edge_dim=2), {'gat_edge_dim': 2}
    run = KGWAS(data, device='cuda:0', seed=3)
    run.initialize_model(**model_kw)
    run.wandb = _Log()
    run.train(batch_size=32, epoch=1, save_best_model=False, save_name='shuf_' + ext, shuffle=True)
    assert run.train_loader.epoch_order == 'seeds' and len(run.wandb.losses) == len(run.train_loader) >= 3
    assert np.isfinite(run.wandb.losses).all() and np.isfinite(run.val_metrics['mse']) and np.isfinite(run.test_metrics['mse'])
    if ext == 'traits':
        assert len(run.trait_pred) > 0 and np.isfinite(np.asarray(run.trait_pred)).all()
    else:
        assert len(run.kgwas_res) > 0 and np.isfinite(np.asarray(run.kgwas_res['pred'].values)).all()
