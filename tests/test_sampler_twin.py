"""The sampler's numpy twin (tests/sampler_twin.py) against the PyG restatement and the structural invariants -- CPU only.
Also the home of the two graphs tests/test_gpu_sampler_exact.py pins the sampler's tile, grid and capacity edges with."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import pyg_semantics as P
from oracle.sampler_np import FullNeighborSamplerNP
from tests.sampler_twin import check_structures, global_edges, sample_twin

LADDER_N = OrderedDict([('SNP', 1025), ('Gene', 1024), ('CellularComponent', 1), ('BiologicalProcess', 1023),
                        ('MolecularFunction', 12400)])
LADDER_CLOSED_SNP, LADDER_LONE_SNP, LADDER_CLOSED_GENE = 1002, 1024, 1023
# MolecularFunction has ONE incoming relation: n seeds of it make a hop-0 segment range of exactly n
LADDER_TILE_EDGE_SEEDS = (4095, 4096, 4097, 8192, 3 * 4096 + 1)


def _graph(n, e, feat=4):
    from kgwas_amd.graph import HeteroGraph, add_self_loops, to_undirected
    data = HeteroGraph()
    for t, k in n.items():
        data[t].x = torch.zeros(k, feat)
    for et, ei in add_self_loops(to_undirected(e, n), n).items():
        data[et].edge_index = torch.from_numpy(np.ascontiguousarray(ei))
    return data


def make_ladder_graph():
    """Built like conftest.make_edge_case_graph (same type names, relations and corner cases), with node counts on the edges of
    the KGW_TILE = 1024 padding of the node space: SNP 1025 (one node into its second tile), Gene 1024 (a full tile),
    CellularComponent 1 (a single node right behind the full tile), BiologicalProcess 1023, MolecularFunction 12 400 (the
    seed type of the tile-edge segment ranges).  Kept: gene 0 with 600 in-edges of one relation (5 chunks), gene 1 with exactly
    128 and gene 2 with exactly 129, degree-0 rows, the EMPTY relation, duplicate edges, self-loops, SNP 1024 without any edge,
    and the closed pair SNP 1002 <-> gene 1023 (its expansion finds nothing new after hop 1)."""
    rng = np.random.default_rng(17)
    n = LADDER_N
    e = OrderedDict()
    hub = np.stack([np.arange(600), np.zeros(600, dtype=np.int64)])
    r128 = np.stack([np.arange(128), np.full(128, 1)])
    r129 = np.stack([np.arange(100, 229), np.full(129, 2)])
    few = np.stack([rng.integers(0, 1000, 300), rng.integers(10, 1000, 300)])
    dup = np.array([[5, 5, 5], [3, 3, 3]])
    closed = np.array([[LADDER_CLOSED_SNP], [LADDER_CLOSED_GENE]])
    e[('SNP', 'ABC', 'Gene')] = np.concatenate([hub, r128, r129, few, dup, closed], axis=1)
    tss = np.arange(0, 1025, 7)
    e[('SNP', 'TSS', 'Gene')] = np.stack([tss, 10 + (tss * 13) % 990])
    e[('SNP', 'EMPTY', 'Gene')] = np.zeros((2, 0), dtype=np.int64)
    g2g = np.stack([rng.integers(0, 1000, 400), rng.integers(0, 1000, 400)])
    e[('Gene', 'G2G', 'Gene')] = np.concatenate([g2g, np.array([[2, 3], [2, 3]])], axis=1)       # has self-loops 2, 3
    e[('Gene', 'G-CC', 'CellularComponent')] = np.stack([np.arange(3, 41), np.zeros(38, dtype=np.int64)])
    e[('Gene', 'G-BP', 'BiologicalProcess')] = np.stack([rng.integers(0, 1000, 1500), rng.integers(0, 1023, 1500)])
    mf = np.arange(12400)
    mf = mf[mf % 5 != 0]                                                                           # every fifth one: degree 0
    e[('Gene', 'G-MF', 'MolecularFunction')] = np.stack([mf % 1000, mf])
    return _graph(n, e)


def make_wide_graph(n_snp=262144 + 1024 + 32, n_gene=2000):
    """A wide sparse graph: the seed type spans more than 257 node tiles and two relations run into it, so a whole-graph call has
    more than 2 x 262 144 segments (the second and third trip of the 256-tiles-per-trip scans).  Degrees are 0 or 1 except
    SNP 5 (300 in-edges of one relation) and the genes' rows; the reduced size keeps the shape for the CPU tests."""
    from kgwas_amd.graph import HeteroGraph
    i = np.arange(n_snp)
    e = OrderedDict()
    a = i[i % 2 == 0]
    e[('Gene', 'A', 'SNP')] = np.concatenate([np.stack([a % n_gene, a]), np.stack([np.arange(300), np.full(300, 5)])], axis=1)
    b = i[i % 3 == 0]
    e[('Gene', 'B', 'SNP')] = np.stack([(b // 3) % n_gene, b])
    c = i[i % 4 == 1]
    e[('SNP', 'C', 'Gene')] = np.stack([c, (c // 4) % n_gene])
    data = HeteroGraph()
    data['SNP'].x = torch.zeros(n_snp, 4)
    data['Gene'].x = torch.zeros(n_gene, 4)
    for et, ei in e.items():
        data[et].edge_index = torch.from_numpy(np.ascontiguousarray(ei))
    return data


def wide_seeds(n_snp):
    """A few hundred seeds spread over the first, a middle and the last node tile."""
    mid = (n_snp // 2048) * 1024
    return np.concatenate([np.arange(0, 200, 2), mid + np.arange(0, 300, 3), np.arange(n_snp - 100, n_snp)])


def ladder_seeds(kind, n):
    if kind == 'SNP':
        fixed = {1: [LADDER_CLOSED_SNP], 2: [LADDER_CLOSED_SNP, LADDER_LONE_SNP]}
        if n in fixed:
            return np.array(fixed[n])
        # every larger batch holds the seed without any in-edge and SNP 5 (the triple edge into gene 3)
        pool = np.setdiff1d(np.arange(LADDER_N['SNP']), [LADDER_LONE_SNP, 5])
        return np.concatenate([[LADDER_LONE_SNP, 5], np.random.default_rng(n).choice(pool, size=n - 2, replace=False)])
    return np.random.default_rng(n).permutation(LADDER_N[kind])[:n]


@pytest.fixture(scope='module')
def ladder_graph():
    return make_ladder_graph()


@pytest.fixture(scope='module')
def wide_small():
    return make_wide_graph(6000 + 32, 400)


def _against_oracles(data, seed_type, seeds, L, all_live=False):
    v = sample_twin(data, L, seed_type, seeds, all_live=all_live)
    sc = v['schema']
    n_id_o, ei_o, hops_o = P.FullNeighborSampler(data.edge_index_dict, data.num_nodes_dict, L).sample(seed_type, seeds)
    n_id_n, ei_n = FullNeighborSamplerNP(data.edge_index_dict, data.num_nodes_dict, L).sample(seed_type, seeds)
    m = v['meta']
    for t, name in enumerate(sc.node_types):
        mine = v['n_id'][t]
        assert np.array_equal(np.sort(mine), np.sort(n_id_o[name].numpy()))
        assert np.array_equal(np.sort(mine), np.sort(n_id_n[name].numpy()))
        for k in range(L + 1):
            a, b = int(m['node_off'][t][k]), int(m['node_off'][t][k + 1])
            assert b - a == int(m['hop_cnt'][t][k])
            ref = n_id_o[name].numpy()[hops_o[name].numpy() == k]
            assert np.array_equal(mine[a:b], ref if k == 0 else np.sort(ref)), (name, k)       # seeds in seed order, then ascending
        base = int(v['node_base'][t])
        assert np.array_equal(v['g2l'][base + mine], np.arange(len(mine)))
        assert int((v['g2l'][base:int(v['node_base'][t + 1])] >= 0).sum()) == len(mine)
    mine_e = global_edges(v)
    for et in sc.edge_types:
        for n_id, ei in ((n_id_o, ei_o), (n_id_n, ei_n)):
            e = ei[et].numpy()
            p = np.stack([n_id[et[0]].numpy()[e[0]], n_id[et[2]].numpy()[e[1]]], axis=1)
            assert np.array_equal(mine_e[et], p[np.lexsort((p[:, 0], p[:, 1]))]), et
    return v


@pytest.mark.parametrize('L', [1, 2, 3])
@pytest.mark.parametrize('which', ['small', 'edge', 'ladder', 'wide'])
def test_twin_matches_pyg_semantics(small_kg, edge_case_graph, ladder_graph, wide_small, which, L):
    data = {'small': small_kg.data, 'edge': edge_case_graph[0], 'ladder': ladder_graph, 'wide': wide_small}[which]
    n_snp = data['SNP'].x.shape[0]
    if which == 'wide':
        cases = [('SNP', wide_seeds(n_snp))]
    elif which == 'ladder':
        cases = [('SNP', ladder_seeds('SNP', n)) for n in (1, 2, 32)] + [('MolecularFunction', ladder_seeds('MolecularFunction', 40))]
    else:
        cases = [('SNP', np.random.default_rng(5).choice(n_snp, size=n, replace=False)) for n in (1, 32)]
    for seed_type, seeds in cases:
        v = _against_oracles(data, seed_type, seeds, L)
        v['expect_multi'] = False                      # (a lone seed's batch need not hold a row above KGW_CHUNK edges)
        if int(v['meta']['edge_end'][L - 1]):
            check_structures(v)


@pytest.mark.parametrize('which', ['small', 'edge', 'ladder'])
@pytest.mark.parametrize('all_live', [False, True])
def test_twin_block_structures(small_kg, edge_case_graph, ladder_graph, which, all_live):
    """The invariants tests/test_gpu_sampler.py holds the HIP sampler to (hub rows included: multi-chunk segments must exist)."""
    if which == 'small':
        data = small_kg.data
        ids = np.random.default_rng(0).choice(data['SNP'].x.shape[0], size=512, replace=False)
    elif which == 'edge':
        data = edge_case_graph[0]
        ids = np.random.default_rng(0).choice(1500, size=64, replace=False)
    else:
        data, ids = ladder_graph, ladder_seeds('SNP', 512)
    for L in (2, 3):
        check_structures(sample_twin(data, L, 'SNP', ids, all_live=all_live))


@pytest.mark.parametrize('which', ['edge', 'ladder', 'wide'])
def test_twin_full_graph(edge_case_graph, ladder_graph, wide_small, which):
    """full_graph: identity node maps, every edge of every relation exactly once, one hop whatever the depth."""
    data = {'edge': edge_case_graph[0], 'ladder': ladder_graph, 'wide': wide_small}[which]
    v = sample_twin(data, 2, 'SNP', None, full_graph=True)
    m = v['meta']
    for t, name in enumerate(v['schema'].node_types):
        n = data[name].x.shape[0]
        assert np.array_equal(v['n_id'][t], np.arange(n))
        assert np.array_equal(v['g2l'][int(v['node_base'][t]):int(v['node_base'][t]) + n], np.arange(n))
        assert list(m['node_off'][t][:4]) == [0, n, n, 0] and list(m['hop_cnt'][t][:2]) == [n, 0]
    mine = global_edges(v)
    for et in data.edge_types:
        ei = data[et].edge_index.numpy()
        assert np.array_equal(mine[et], ei.T[np.lexsort((ei[0], ei[1]))])
    assert int(m['edge_end'][0]) == sum(int(data[et].edge_index.shape[1]) for et in data.edge_types)
    assert list(m['n_edges'][:2]) == [int(m['edge_end'][0])] * 2          # hd = min(L - l, n_hops - 1) = 0 for both layers
    check_structures(v)


def test_twin_static_layout(ladder_graph):
    """lay_* and the bases come from the capacities, n_rows / n_src from the batch; one row short is error bit 5."""
    from kgwas_amd.sampler import BatchCaps
    ids = ladder_seeds('SNP', 32)
    free = sample_twin(ladder_graph, 2, 'SNP', ids)
    m = free['meta']
    NT = free['schema'].NT
    exact = BatchCaps([[int(x) for x in m['node_off'][t][:4]] for t in range(NT)], [0, 0], [0, 0])
    roomy = BatchCaps([[0] + [int(x) + 37 for x in m['node_off'][t][1:4]] for t in range(NT)], [0, 0], [0, 0])
    a = sample_twin(ladder_graph, 2, 'SNP', ids, caps=exact)
    for k in ('n_rows', 'n_src', 'lay_rows', 'lay_src', 'z_base', 'src_base', 't_base', 'error'):
        assert np.array_equal(a['meta'][k], m[k]), k
    b = sample_twin(ladder_graph, 2, 'SNP', ids, caps=roomy)
    bm = b['meta']
    assert bm['error'] == 0 and np.array_equal(bm['n_rows'], m['n_rows']) and np.array_equal(bm['n_src'], m['n_src'])
    assert np.all(bm['lay_src'][:2, :NT][m['lay_src'][:2, :NT] > 0] > m['lay_src'][:2, :NT][m['lay_src'][:2, :NT] > 0])
    assert int(bm['t_base'][0][NT]) > int(m['t_base'][0][NT])
    assert len(b['t_ptr'][0]) == int(bm['t_base'][0][NT]) + 1
    check_structures(b)
    short = [list(r) for r in exact.node_off]
    short[free['schema'].type_id['Gene']][2] -= 1
    assert sample_twin(ladder_graph, 2, 'SNP', ids, caps=BatchCaps(short, [0, 0], [0, 0]))['meta']['error'] == 32
