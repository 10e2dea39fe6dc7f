"""-m gpu: kgw_gat_aggregate_bwd (k_agg_bwd_dst + k_agg_bwd_combine, then the src-major pass) on ONE small graph whose destination
rows sit on every bound of the dst-major kernel at once, against the float64 oracle and with the tolerances of
tests/test_gpu_aggregate.py (its helpers are used as they are).

In one launch: rows of 0, 1, 7, 8, 9, 127, 128, 129 and 300 edges on one relation -- a row without edges, the half-waves' groups of
2 / 4 / 8 with their tails, exactly one 128-edge chunk, one chunk less and one more (two chunks: k_agg_bwd_combine), a hub row of
three chunks --, three relations into the Gene rows and two into the SNP rows, and, in the second batch, the padded static layout
of a captured step (row blocks of fixed capacity, fewer real rows).  About 1.5 k edges.

k_agg_bwd_dst keeps the per-lane offset of its d u_r record out of the prologue (it was the one value spilled to scratch at four
wavefronts per SIMD); the record of every chunk, short or long, single or part of a hub row, is compared here through dU."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests.helpers import assert_close, segment_alpha_sums
from tests.test_gpu_aggregate import ATOL, RTOL, _oracle_layer
from tests.test_gpu_aggregate_parity import realised_structure

pytestmark = pytest.mark.gpu

DEGREES = [0, 1, 7, 8, 9, 127, 128, 129, 300]      # in-degrees of genes 0..8 on ('SNP', 'LAD', 'Gene')
N_SNP, N_GENE = 400, 40                             # (genes 12..39: a few TSS edges each -- most stay outside a minibatch)
HUB_SNP = 0                                         # a TSS edge to genes 0..11: as a seed it pulls every ladder row into hop 1


def make_edge_graph():
    from kgwas_amd.graph import HeteroGraph, add_self_loops, to_undirected
    rng = np.random.default_rng(509)
    n = OrderedDict([('SNP', N_SNP), ('Gene', N_GENE)])
    src = [rng.choice(np.arange(1, N_SNP), size=d, replace=False) for d in DEGREES]
    dst = [np.full(d, g) for g, d in enumerate(DEGREES)]
    lad = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    tss_d = rng.integers(0, 4, N_GENE)
    tss = np.concatenate([np.stack([np.full(12, HUB_SNP), np.arange(12)]),
                          np.stack([rng.integers(1, N_SNP, int(tss_d.sum())), np.repeat(np.arange(N_GENE), tss_d)])],
                         axis=1).astype(np.int64)
    g2g = np.stack([rng.integers(0, N_GENE, 10), rng.integers(0, N_GENE, 10)]).astype(np.int64)
    e = OrderedDict([(('SNP', 'LAD', 'Gene'), lad), (('SNP', 'TSS', 'Gene'), tss), (('Gene', 'G2G', 'Gene'), g2g)])
    g = torch.Generator().manual_seed(17)
    data = HeteroGraph()
    for t, k in n.items():
        data[t].x = torch.rand(k, 16, generator=g)
    und = add_self_loops(to_undirected(e, n), n)
    for et, ei in und.items():
        data[et].edge_index = torch.from_numpy(np.ascontiguousarray(ei))
    data['SNP'].y = torch.rand(N_SNP, generator=g)
    return data


_STATE = {}


def _graph():
    if 'data' not in _STATE:
        _STATE['data'] = make_edge_graph()
    return _STATE['data']


def _batch(kind):
    """'full': every node a seed.  'static': a minibatch of 24 SNP seeds (the hub SNP among them) laid out in the row blocks of a
    static layout whose capacities are above the batch's own counts."""
    if kind not in _STATE:
        from kgwas_amd.sampler import BatchBuffers, NeighborLoader, finish_sample, sample_full_graph, sample_into
        data = _graph()
        if kind == 'full':
            _STATE[kind] = sample_full_graph(data, 2, 'cuda:0')
        else:
            seeds = np.concatenate([[HUB_SNP], np.random.default_rng(3).choice(np.arange(1, N_SNP), size=23, replace=False)])
            ld = NeighborLoader(data, [-1, -1], ('SNP', seeds.astype(np.int64)), batch_size=len(seeds), device='cuda:0', prefetch=False)
            dgs = ld.dg.with_static_caps(ld.measure_caps())                      # (3 % margin, rounded up to 64)
            buf = BatchBuffers(dgs)
            sample_into(dgs, buf, ld.ids, ld.seed_type)
            _STATE[kind] = finish_sample(dgs, buf, 'SNP', len(seeds))
    return _STATE[kind]


def test_graph_realises_every_edge():
    data = _graph()
    lad = data[('SNP', 'LAD', 'Gene')].edge_index
    assert torch.bincount(lad[1], minlength=N_GENE)[:len(DEGREES)].tolist() == DEGREES
    n_edges = sum(int(data[et].edge_index.shape[1]) for et in data.edge_types)
    assert n_edges <= 2200, n_edges
    into = {}
    for s, _, d in data.edge_types:
        into[d] = into.get(d, 0) + 1
    assert into['Gene'] >= 3 and into['SNP'] == 2, into
    for kind in ('full', 'static'):
        b = _batch(kind)
        s = realised_structure(b, 1)
        print(f'{kind} layer 1: chunk lengths {s["chunk_lens"]}, chunks per segment {sorted(s["nch"])}, hn mod 8 {sorted(s["hn_mod8"])}')
        assert {1, 7, 8, 9, 127, 128} <= set(s['chunk_lens']), s['chunk_lens']
        assert {1, 2, 3} <= s['nch'] and s['single_128'], s['nch']
    b = _batch('static')
    m, sc = b.meta, b.dg.schema
    gene = sc.type_id['Gene']
    block = int(m.z_base[0][gene + 1]) - int(m.z_base[0][gene])
    assert block > int(m.n_rows[0][gene]) * int(sc.R_dst[gene]) > 0, (block, int(m.n_rows[0][gene]))      # capacity above the real rows


@pytest.mark.parametrize('kind,layer', [('full', 1), ('full', 2), ('static', 1), ('static', 2)])
def test_backward_matches_float64(kind, layer):
    from kgwas_amd import ops
    batch = _batch(kind)
    dg, m = batch.dg, batch.meta
    sc = dg.schema
    g = torch.Generator().manual_seed(40 + layer)
    n_src = int(m.src_base[layer - 1][sc.NT])
    z_rows = int(m.z_base[layer - 1][sc.NT])
    assert n_src > 0 and z_rows > 0
    H = torch.randn(n_src, 128, generator=g)
    V = torch.randn(sc.NR, 128, generator=g) * 0.2
    U = torch.randn(sc.NR, 128, generator=g) * 0.2
    G = torch.randn(z_rows, 128, generator=g)

    Hd, Vd, Ud = (t.cuda().requires_grad_(True) for t in (H, V, U))
    Z, stat, e_edge = ops.gat_aggregate(batch, layer, Hd, Ud, Vd)
    (Z * G.cuda()).sum().backward()

    Ho, Vo, Uo = (t.double().requires_grad_(True) for t in (H, V, U))
    Zo = _oracle_layer(batch, layer, Ho, Vo, Uo)
    (Zo * G.double()).sum().backward()

    assert_close(Z, Zo.detach(), RTOL, ATOL, 'Z')
    assert_close(Hd.grad, Ho.grad, RTOL, 2e-5, 'dH')
    live = [r for r in range(sc.NR) if dg.kg.rel_live[layer - 1][r]]
    assert live
    assert_close(Ud.grad[live], Uo.grad[live], RTOL, 1e-4, 'dU')
    assert_close(Vd.grad[live], Vo.grad[live], RTOL, 1e-4, 'dV')
    dead = [r for r in range(sc.NR) if not dg.kg.rel_live[layer - 1][r]]
    assert float(Ud.grad[dead].abs().sum()) == 0.0 and float(Vd.grad[dead].abs().sum()) == 0.0
    alpha = ops.edge_alpha(batch, layer, stat, e_edge)
    assert torch.isfinite(alpha).all() and float(alpha.min()) >= 0.0
    if kind == 'full':
        sums = segment_alpha_sums(batch, layer, alpha)
        assert sums.numel() > 0 and float((sums - 1.0).abs().max()) <= 1e-5, float((sums - 1.0).abs().max())
    # the same launch again: no atomics anywhere, the same bits
    Hd2, Vd2, Ud2 = (t.cuda().requires_grad_(True) for t in (H, V, U))
    Z2, _, _ = ops.gat_aggregate(batch, layer, Hd2, Ud2, Vd2)
    (Z2 * G.cuda()).sum().backward()
    assert torch.equal(Hd2.grad, Hd.grad) and torch.equal(Ud2.grad, Ud.grad) and torch.equal(Vd2.grad, Vd.grad)
