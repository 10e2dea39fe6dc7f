"""-m gpu: finite fan-out sampling (kgw_sample_batch_fanout, NeighborLoader(num_neighbors=[k_1, ..., k_L]), up to
KGWAS.train) against the numpy twin of its rule (tests/fanout_ref.py).  Integer work => exact comparisons."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fanout_ref as R
from tests.helpers import assert_close, batch_cpu, grads_by_name, oracle_from_product

pytestmark = pytest.mark.gpu

BIG = 1 << 30


def _loader(data, ids, bs, nn, **kw):
    from kgwas_amd.sampler import NeighborLoader
    return NeighborLoader(data, num_neighbors=list(nn), input_nodes=('SNP', ids), batch_size=bs, device='cuda:0', **kw)


@pytest.fixture(scope='module')
def graphs(small_kg):
    from tests.test_gpu_aggregate_parity import _ladder_seeds, make_degree_ladder_graph
    from tests.test_gpu_hub import HUB, make_hub_graph
    hub = make_hub_graph()[0]
    rng = np.random.default_rng(3)
    small = small_kg.data
    return {'small': (small, rng.choice(small['SNP'].x.shape[0], size=96, replace=False)),
            'ladder': (make_degree_ladder_graph(), _ladder_seeds()),
            # seeds below HUB hang on gene 0 (75 000 in-edges), the next 10 000 SNPs on gene 1
            'hub': (hub, np.concatenate([rng.choice(HUB, size=20, replace=False), [HUB + 3, HUB + 12_000, 89_999]]))}


def _csr(batch):
    dg = batch.dg
    sc = dg.schema
    rp_all, col_all = dg.g_rowptr.cpu().numpy(), dg.g_col.cpu().numpy()
    out = []
    for r in range(sc.NR):
        n_dst = dg.n_nodes[int(sc.dst_type[r])]
        ro, co = int(dg.kg.rowptr_off[r]), int(dg.kg.col_off[r])
        rp = rp_all[ro:ro + n_dst + 1].astype(np.int64)
        out.append((rp, col_all[co:co + int(rp[-1])]))
    return out


def _segments(batch):
    """{(h, r): [global source ids of every segment]} and the hops' node lists, read back from the batch's buffers."""
    dg, m, buf = batch.dg, batch.meta, batch.buf
    sc = dg.schema
    n_edges = int(m.edge_end[dg.n_hops - 1])
    seg_ptr = buf.seg_ptr[:int(m.seg_end[dg.n_hops - 1]) + 1].cpu().numpy()
    col = buf.col_local[:n_edges].cpu().numpy()
    n_id = [batch.n_id(t).cpu().numpy().astype(np.int64) for t in sc.node_types]
    segs = {}
    for h in range(dg.n_hops):
        for r in range(sc.NR):
            a, b = int(m.seg_off[h][r]), int(m.seg_off[h][r + 1])
            src = n_id[int(sc.src_type[r])]
            segs[(h, r)] = [src[col[seg_ptr[s]:seg_ptr[s + 1]]] for s in range(a, b)]
    hops = [[n_id[t][int(m.node_off[t][k]):int(m.node_off[t][k + 1])] for t in range(sc.NT)] for k in range(dg.n_hops + 1)]
    return hops, segs


def _assert_equals_twin(batch, seeds, nn, word):
    sc = batch.dg.schema
    hops_o, segs_o = R.sample_batch(_csr(batch), [int(t) for t in sc.src_type], [int(t) for t in sc.dst_type], sc.NT,
                                    sc.type_id['SNP'], seeds, list(nn), word)
    hops, segs = _segments(batch)
    n_drawn = 0
    for h in range(len(nn) + 1):
        for t in range(sc.NT):
            assert np.array_equal(hops[h][t], hops_o[h][t]), f'nodes of type {t} new at hop {h} differ'
    for (h, r), mine in segs.items():
        ref = segs_o[(h, r)]
        assert len(mine) == len(ref), (h, r)
        for j, (a, b) in enumerate(zip(mine, ref)):
            assert np.array_equal(a, b), f'hop {h} relation {r} segment {j}: {a[:8]} vs {b[:8]}'
            n_drawn += nn[h] >= 0 and len(b) == nn[h]
    # rows longer than their fan-out, counted from the CSR: each of them gave a segment of exactly k entries
    csr = _csr(batch)
    n_long = sum(int((np.diff(rp)[hops_o[h][int(sc.dst_type[r])]] > nn[h]).sum())
                 for h in range(len(nn)) if nn[h] >= 0 for r, (rp, _) in enumerate(csr))
    assert n_drawn >= n_long
    return n_long


FANOUTS = [(3, 3), (10, 5), (-1, 4), (4, -1), (3, 2, 2)]


@pytest.mark.parametrize('nn', FANOUTS, ids=lambda n: 'x'.join(map(str, n)))
@pytest.mark.parametrize('which', ['small', 'ladder', 'hub'])
def test_segments_equal_the_numpy_twin(graphs, which, nn):
    """3. Exact sets: every segment's source ids, hop by hop, on the small KG, the degree ladder (rows of 0 .. 1 000 entries: the
    one-wavefront select) and the hub graph (a row of 75 000 and one of 10 000: the block-wide select)."""
    data, ids = graphs[which]
    ld = _loader(data, ids, len(ids), nn, seed=5)
    ld.set_epoch(2)
    batch = next(iter(ld))
    assert np.array_equal(batch.n_id('SNP')[:len(ids)].cpu().numpy(), ids)
    n_drawn = _assert_equals_twin(batch, ids, nn, R.sample_word(5, 2, 0))
    # (the hub graph's seeds have two or three in-edges each: at (4, -1) nothing is drawn there and the case checks the pass-through)
    assert n_drawn > 0 or (which, tuple(nn)) == ('hub', (4, -1)), 'no row was longer than its fan-out: the case tests nothing'
    if which == 'hub':
        assert max(int(np.diff(rp).max()) for rp, _ in _csr(batch)) >= 75_000           # the hub row is there
        assert 0 in batch.n_id('Gene').cpu().numpy()                  # ... and was expanded (hop 1)


def _used_arrays(batch):
    dg, m, buf = batch.dg, batch.meta, batch.buf
    sc, L = dg.schema, dg.num_layers
    ns, ne, nc = int(m.seg_end[dg.n_hops - 1]), int(m.edge_end[dg.n_hops - 1]), int(m.chunk_end[dg.n_hops - 1])
    out = {'g2l': buf.g2l, 'seg_deg': buf.seg_deg[:ns], 'seg_nch': buf.seg_nch[:ns], 'seg_ptr': buf.seg_ptr[:ns + 1],
           'seg_chptr': buf.seg_chptr[:ns + 1], 'col_local': buf.col_local[:ne], 'chunks': buf.chunks[:nc * 8],
           'meta': buf.meta_host.clone()}
    for t, name in enumerate(sc.node_types):
        out['n_id ' + name] = batch.n_id(name)
    for h in range(dg.n_hops):
        k = int(m.multi_cnt[h])
        out[f'multi {h}'] = buf.multi[h * dg.multi_cap * 4:(h * dg.multi_cap + k) * 4].view(-1, 4).cpu().numpy()
        out[f'multi {h}'] = torch.from_numpy(out[f'multi {h}'][np.argsort(out[f'multi {h}'][:, 0], kind='stable')].copy())   # (listed in arrival order)
    for l in range(L):
        nt, trows, nsrc = int(m.t_entries[l]), int(m.t_base[l][sc.NT]), int(m.src_base[l][sc.NT])
        out[f't_ptr {l}'] = buf.t_ptr[l][:trows + 1]
        out[f't_edge {l}'] = buf.t_edge[l][:nt]
        out[f't_zrow {l}'] = buf.t_zrow[l][:nt]
        out[f't_rel {l}'] = buf.t_rel[l][:nt]
        out[f'oct {l}'] = buf.t_cnt[l][:(nsrc + 7) // 8]
    return {k: v.detach().cpu().clone() for k, v in out.items()}


@pytest.mark.parametrize('which', ['small', 'ladder', 'hub'])
def test_a_fanout_above_every_degree_is_the_full_neighbourhood_bit_for_bit(graphs, which):
    """4. k_h = 2^30: every array of the batch (and the whole meta block) equals the [-1] * L batch's."""
    data, ids = graphs[which]
    full = _used_arrays(next(iter(_loader(data, ids, len(ids), [-1, -1]))))
    for nn in ([BIG, BIG], [BIG, -1]):
        big = _used_arrays(next(iter(_loader(data, ids, len(ids), nn, seed=9))))
        assert full.keys() == big.keys()
        for k in full:
            assert torch.equal(full[k], big[k]), k


def _check_structure(batch):
    """The structural checks of tests/test_gpu_sampler.py::test_block_structures_are_consistent, restated."""
    from kgwas_amd._lib import KGW_CHUNK
    dg, m, buf = batch.dg, batch.meta, batch.buf
    sc = dg.schema
    L = dg.num_layers
    n_segs = int(m.seg_end[L - 1])
    n_chunks_all = int(m.chunk_end[L - 1])
    n_edges_all = int(m.edge_end[L - 1])
    ch = buf.chunks[:n_chunks_all * 8].view(-1, 8).cpu().numpy()
    col = buf.col_local[:n_edges_all].cpu().numpy()
    assert n_chunks_all > 0 and n_edges_all > 0
    # seg_off / seg_ptr / seg_chptr: prefixes of the segments' lengths and chunk counts, hop after hop
    seg_deg = buf.seg_deg[:n_segs].cpu().numpy()
    seg_ptr = buf.seg_ptr[:n_segs + 1].cpu().numpy()
    seg_chptr = buf.seg_chptr[:n_segs + 1].cpu().numpy()
    assert seg_ptr[0] == 0 and seg_ptr[-1] == n_edges_all and np.array_equal(np.diff(seg_ptr), seg_deg)
    assert seg_chptr[0] == 0 and seg_chptr[-1] == n_chunks_all
    assert np.array_equal(np.diff(seg_chptr), (seg_deg + KGW_CHUNK - 1) // KGW_CHUNK)
    for h in range(L):
        assert int(m.seg_off[h][0]) == (0 if h == 0 else int(m.seg_end[h - 1])) and int(m.seg_off[h][sc.NR]) == int(m.seg_end[h])
        for r in range(sc.NR):
            assert int(m.seg_off[h][r + 1]) - int(m.seg_off[h][r]) == int(m.hop_cnt[int(sc.dst_type[r])][h])
    # chunks tile [0, n_edges) in order, and belong to their segment
    assert ch[0, 0] == 0 and ch[-1, 1] == n_edges_all
    assert np.array_equal(ch[1:, 0], ch[:-1, 1])
    assert np.all(ch[:, 1] - ch[:, 0] <= KGW_CHUNK) and np.all(ch[:, 1] > ch[:, 0])
    seg_of_chunk = np.searchsorted(seg_chptr, np.arange(n_chunks_all), side='right') - 1
    assert np.array_equal(ch[:, 4], seg_chptr[seg_of_chunk]) and np.array_equal(ch[:, 5], np.diff(seg_chptr)[seg_of_chunk])
    n_multi = sum(int(m.multi_cnt[h]) for h in range(L))
    assert n_multi == len(np.unique(ch[ch[:, 5] > 1][:, 4]))
    for l in range(1, L + 1):
        nc, ne = int(m.n_chunks[l - 1]), int(m.n_edges[l - 1])
        live = np.array([dg.kg.rel_live[l - 1][r] for r in range(sc.NR)], dtype=bool)
        chl = ch[:nc]
        chl = chl[live[chl[:, 3]]]
        n_live_edges = int((chl[:, 1] - chl[:, 0]).sum())
        assert int(m.t_entries[l - 1]) == n_live_edges
        t_rows = int(m.t_base[l - 1][sc.NT])
        tptr = buf.t_ptr[l - 1][:t_rows + 1].cpu().numpy()
        tedge = buf.t_edge[l - 1][:n_live_edges].cpu().numpy()
        tz = buf.t_zrow[l - 1][:n_live_edges].cpu().numpy()
        assert tptr[0] == 0 and tptr[-1] == n_live_edges and np.all(np.diff(tptr) >= 0)
        expect = np.concatenate([np.arange(a, b) for a, b in chl[:, :2]]) if len(chl) else np.zeros(0, np.int64)
        assert np.array_equal(np.sort(tedge), np.sort(expect))
        e2chunk = np.searchsorted(ch[:, 1], tedge, side='right')
        rel = ch[e2chunk, 3]
        row = ch[e2chunk, 2]
        src_t = sc.src_type[rel]
        dst_t = sc.dst_type[rel]
        tb = np.array([m.t_base[l - 1][t] for t in range(sc.NT + 1)])
        zb = np.array([m.z_base[l - 1][t] for t in range(sc.NT + 1)])
        trow = tb[src_t] + col[tedge] * sc.R_src[src_t] + sc.slot_src[rel]
        pos = np.arange(n_live_edges)
        assert np.all(tptr[trow] <= pos) and np.all(pos < tptr[trow + 1])
        assert np.array_equal(tz, zb[dst_t] + row * sc.R_dst[dst_t] + sc.slot_dst[rel])
        assert np.array_equal(buf.t_rel[l - 1][:n_live_edges].cpu().numpy(), rel)
        n_src_rows = int(m.src_base[l - 1][sc.NT])
        flags = buf.t_cnt[l - 1][:(n_src_rows + 7) // 8].cpu().numpy()
        sb = np.array([m.src_base[l - 1][t] for t in range(sc.NT + 1)])
        for o in range(len(flags)):
            u0 = 8 * o
            ty = int(np.searchsorted(sb[1:], u0, side='right'))
            j0 = u0 - sb[ty]
            ok = bool((dg.short_type_mask >> ty) & 1) and j0 + 8 <= int(m.n_src[l - 1][ty]) and \
                not (sc.R_dst[ty] > 0 and j0 < int(m.n_rows[l - 1][ty]))
            if ok:
                Rs = int(sc.R_src[ty])
                t0 = tb[ty] + j0 * Rs
                ok = all(tptr[t0 + (q + 1) * Rs] - tptr[t0 + q * Rs] <= 8 for q in range(8))
            assert bool(flags[o]) == ok, (l, o)
        assert ne <= n_edges_all
        row_of = np.repeat(np.arange(t_rows), np.diff(tptr))
        same = row_of[1:] == row_of[:-1]
        assert np.all(tedge[1:][same] > tedge[:-1][same])


@pytest.mark.parametrize('nn', [(10, 5), (300, 200), (-1, 4)], ids=lambda n: 'x'.join(map(str, n)))
@pytest.mark.parametrize('which', ['small', 'ladder', 'hub'])
def test_block_structures_of_a_fanout_batch_are_consistent(graphs, which, nn):
    """5. seg_off / seg_ptr, chunk list, src-major transpose and octet flags of a fan-out batch ((300, 200): drawn segments of more
    than one chunk)."""
    data, ids = graphs[which]
    _check_structure(next(iter(_loader(data, ids, len(ids), nn, seed=1))))


def _draw_arrays(buf, n_hops):
    m = buf.read_meta()
    ns, ne = int(m.seg_end[n_hops - 1]), int(m.edge_end[n_hops - 1])
    return {'n_id': buf.n_id.cpu().clone(), 'seg_ptr': buf.seg_ptr[:ns + 1].cpu().clone(), 'col_local': buf.col_local[:ne].cpu().clone()}


def test_same_seed_epoch_batch_is_the_same_batch_and_another_epoch_is_another_draw(small_kg):
    """6. (seed, epoch, batch) fixes the batch -- prefetch on or off, eager or sampled by the captured side-stream graph of a
    training step; another epoch (or another loader seed) draws differently."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    data = small_kg.data
    ids = np.asarray(small_kg.train_input_nodes[1][:256])
    nn = [10, 5]
    a = _loader(data, ids, 64, nn, drop_last=True, seed=3)
    b = _loader(data, ids, 64, nn, drop_last=True, seed=3, prefetch=False)
    first = []
    for x, y in zip(a, b):
        ax, ay = _used_arrays(x), _used_arrays(y)
        for k in ax:
            assert torch.equal(ax[k], ay[k]), k
        first.append(ax)
    assert len(first) == 4
    # the next pass is the next epoch by itself; set_epoch(0) brings the first one back
    second = [_used_arrays(x) for x in a]
    assert a.epoch == 1
    for i in range(4):
        assert torch.equal(first[i]['n_id SNP'][:64], second[i]['n_id SNP'][:64])          # same seeds ...
        assert not torch.equal(first[i]['col_local'], second[i]['col_local']) or \
            not torch.equal(first[i]['n_id Gene'], second[i]['n_id Gene']), f'batch {i} was not redrawn'
    a.set_epoch(0)
    for i, x in enumerate(a):
        ax = _used_arrays(x)
        for k in ax:
            assert torch.equal(ax[k], first[i][k]), k
    other = _used_arrays(next(iter(_loader(data, ids, 64, nn, drop_last=True, seed=4))))
    assert not torch.equal(other['col_local'], first[0]['col_local']) or not torch.equal(other['n_id Gene'], first[0]['n_id Gene'])
    # a row with deg > k really differs between the epochs: the twin says which entries each epoch keeps
    b.set_epoch(1)
    _assert_equals_twin(next(iter(b)), ids[:64], nn, R.sample_word(3, 1, 0))

    # captured: after step(0) the side-stream graph has sampled batch 1 of epoch 0 into the other buffer
    run = KGWAS(small_kg, device='cuda:0', seed=3)
    run.initialize_model()
    gs = GraphTrainStep(run, ('SNP', ids), 64, num_neighbors=nn, sample_seed=3)
    assert gs.cache is None and not gs._want_cache
    gs.step(0)
    torch.cuda.synchronize()
    ld = _loader(data, ids, 64, nn, drop_last=True, seed=3, prefetch=False)
    it = iter(ld)
    next(it)
    e1 = next(it)
    torch.cuda.synchronize()
    want, got = _draw_arrays(e1.buf, 2), _draw_arrays(gs.bufs[1], 2)
    for k in ('seg_ptr', 'col_local'):
        assert torch.equal(want[k], got[k]), k
    for t in data.node_types:
        ti = e1.dg.schema.type_id[t]
        base, n = e1.dg.node_base[ti], e1.n_nodes[t]
        assert torch.equal(want['n_id'][base:base + n], got['n_id'][base:base + n]), t
    gs.check()


@pytest.mark.parametrize('nn', [(10, 5), (4, -1), (3, 2, 2)], ids=lambda n: 'x'.join(map(str, n)))
@pytest.mark.parametrize('which', ['small', 'hub'])
def test_model_on_a_fanout_batch_matches_the_float64_oracle(small_kg, graphs, which, nn):
    """7. HeteroGNN forward, loss and every gradient on a fan-out batch against the float64 oracle on THAT batch's exported
    edge_index_dict, at the standing tolerance |a - b| <= 1e-5 + 1e-4 |b| + 1e-5 max|b|."""
    from kgwas_amd.model import HeteroGNN
    from oracle.gat_oracle import weighted_mse
    if which == 'small':
        data, dims = small_kg.data, (small_kg.snp_init_dim_size, small_kg.gene_init_dim_size, small_kg.go_init_dim_size)
    else:
        data, dims = graphs['hub'][0], (20, 24, 16)
    ids = graphs[which][1][:23] if which == 'hub' else np.random.default_rng(2).choice(data['SNP'].x.shape[0], size=40, replace=False)
    L = len(nn)
    torch.manual_seed(0)
    model = HeteroGNN(data, 128, 1, L, 'GAT', 'sum', dims[0], dims[1], dims[2], 1).cuda()
    with torch.no_grad():
        for pack in list(model.live_packs) + list(model.dead_packs):
            pack.bias.normal_(0, 0.1)
    batch = next(iter(_loader(data, ids, len(ids), nn, seed=8)))
    n = len(ids)
    out = model(batch.x_dict, batch.edge_index_dict, n)
    y = torch.rand(n, dtype=torch.float64)
    w = torch.rand(n, dtype=torch.float64) + 0.5
    loss = weighted_mse(out, y.cuda(), w.cuda())
    loss.backward()
    oracle = oracle_from_product(model)
    x, ei = batch_cpu(batch)
    assert sum(int(e.shape[1]) for e in ei.values()) == batch.n_edges_sampled
    out_o = oracle(x, ei, n)
    loss_o = weighted_mse(out_o, y, w)
    loss_o.backward()
    RT, AT = 1e-4, 1e-5
    print(f'pred: max abs err {float((out.detach().cpu().double() - out_o.detach()).abs().max()):.3e}; loss {float(loss):.9f} vs {float(loss_o):.9f}')
    go = grads_by_name(oracle)
    mine = grads_by_name(model)
    for name, g in mine.items():
        if g is not None and go[name] is not None:
            print(f'grad {name}: max abs err {float((g.double() - go[name]).abs().max()):.3e}, max |ref| {float(go[name].abs().max()):.3e}')
    assert_close(out, out_o.detach(), RT, AT, 'pred')
    assert_close(loss.detach(), loss_o.detach(), RT, AT, 'loss')
    n_live = 0
    for name, g in mine.items():
        ref = go[name]
        if g is None:
            assert ref is None or float(ref.abs().max()) == 0.0, f'{name}: product has no grad, oracle has'
            continue
        n_live += 1
        assert ref is not None, name
        assert_close(g, ref, RT, AT, f'grad {name}')
    assert n_live > 10


class _Log:
    def __init__(self):
        self.losses = []

    def log(self, d):
        if 'training_loss' in d:
            self.losses.append(d['training_loss'])


def test_captured_training_with_a_fanout_equals_eager_and_redraws_every_epoch(small_kg, monkeypatch):
    """8. KGWAS.train(num_neighbors=[10, 5], epoch=2): the captured step (side-stream sampling graph reading the seed word) and
    eager launches give the same loss at every step (the criterion of tests/test_gpu_graph.py::test_graph_step_equals_eager);
    epoch 2's batches are not epoch 1's; the analytic capacities hold over both epochs (a batch that outgrew them raises)."""
    from kgwas_amd import graph_step
    from kgwas_amd.kgwas import KGWAS
    fed, sampled = [], []
    real_feed = graph_step.GraphTrainStep._feed

    def feed(self, i, epoch):
        real_feed(self, i, epoch)
        fed.append((epoch, i))
    monkeypatch.setattr(graph_step.GraphTrainStep, '_feed', feed)
    real_step = KGWAS.train_step

    def train_step(self, batch, *a, **k):
        sampled.append((batch.n_edges_sampled, batch.buf.col_local[:batch.n_edges_sampled].cpu().clone()))
        return real_step(self, batch, *a, **k)
    monkeypatch.setattr(KGWAS, 'train_step', train_step)
    losses, sd0 = {}, None
    for use_graph in (True, False):
        run = KGWAS(small_kg, device='cuda:0', seed=31)
        run.initialize_model()
        if sd0 is None:
            sd0 = copy.deepcopy(run.model.state_dict())
        else:
            run.model.load_state_dict(sd0)
        run.wandb = _Log()
        run.train(batch_size=64, epoch=2, save_best_model=False, save_name='fan' + str(use_graph), use_graph=use_graph,
                  num_neighbors=[10, 5])
        losses[use_graph] = run.wandb.losses
        assert np.isfinite(run.val_metrics['mse'])
    n = len(losses[True])
    assert n == len(losses[False]) and n % 2 == 0 and n >= 4
    for i in range(n):
        assert_close(torch.tensor(losses[True][i]), torch.tensor(losses[False][i]), 1e-5, 1e-7, f'loss step {i}')
    per = n // 2
    assert {e for e, _ in fed} >= {0, 1} and (1, per - 1) in fed
    assert len(sampled) == n
    differ = sum(1 for i in range(per) if sampled[i][0] != sampled[per + i][0] or not torch.equal(sampled[i][1], sampled[per + i][1]))
    assert differ == per, f'only {differ} of {per} batches were redrawn in epoch 2'


def test_what_is_not_built_is_refused(small_kg):
    """9. the dict form, k = 0, replacement, shuffle, and a finite fan-out in the SNP-sharded mode."""
    from kgwas_amd.kgwas import KGWAS
    data = small_kg.data
    ids = np.arange(64)
    with pytest.raises(NotImplementedError):
        _loader(data, ids, 64, [10, 5], replace=True)
    with pytest.raises(NotImplementedError):
        _loader(data, ids, 64, [10, 5], shuffle=True)
    from kgwas_amd.sampler import NeighborLoader
    with pytest.raises(NotImplementedError):
        NeighborLoader(data, num_neighbors={et: [10, 5] for et in data.edge_types}, input_nodes=('SNP', ids), batch_size=64,
                       device='cuda:0')
    for bad in ([0, 5], [10, 0], [-2, 5]):
        with pytest.raises(ValueError):
            _loader(data, ids, 64, bad)
    run = KGWAS(small_kg, device='cuda:0', seed=1)
    run.initialize_model()
    with pytest.raises(NotImplementedError):
        run.train(batch_size=64, epoch=1, save_best_model=False, parallelism='shard', num_neighbors=[10, 5])
    with pytest.raises(ValueError):
        run.train(batch_size=64, epoch=1, save_best_model=False, num_neighbors=[10, 0])
    with pytest.raises(ValueError):
        run.train(batch_size=64, epoch=1, save_best_model=False, num_neighbors=[10])


def test_capacities_of_a_fanout_loader_bound_every_epoch(small_kg):
    """measure_caps of a fan-out loader: never above the full-neighbourhood capacities, at most rows x k x relations where that
    is smaller, and no batch of three epochs exceeds them."""
    data = small_kg.data
    ids = np.asarray(small_kg.train_input_nodes[1][:512])
    full = _loader(data, ids, 64, [-1, -1], drop_last=True, prefetch=False).measure_caps()
    ld = _loader(data, ids, 64, [10, 5], drop_last=True, prefetch=False, seed=2)
    caps = ld.measure_caps()
    sc = ld.dg.schema
    assert all(c <= f for c, f in zip(caps.edges, full.edges)) and all(c <= f for c, f in zip(caps.chunks, full.chunks))
    assert caps.edges[0] < full.edges[0]
    seed_rels = sum(1 for r in range(sc.NR) if int(sc.dst_type[r]) == sc.type_id['SNP'])
    assert caps.edges[1] <= -(-64 * seed_rels * 10 // 64) * 64                 # layer 2 aggregates hop 0 only
    for t in range(sc.NT):
        assert all(c <= f for c, f in zip(caps.node_off[t], full.node_off[t]))
    for ep in range(3):
        for b in ld:
            m = b.meta
            for t in range(sc.NT):
                for k in range(4):
                    assert int(m.node_off[t][min(k, 3)]) <= caps.node_off[t][k]
            for l in range(2):
                assert int(m.n_edges[l]) <= caps.edges[l] and int(m.n_chunks[l]) <= caps.chunks[l]
