"""-m gpu: the kernels of the SNP-sharded mode (kgwas_amd/shard.py) against float64, all ranks in one process on one device
(tests/shard_ranks.py): kgw_sample_batch_parts, the PARTIAL branches of k_agg_fwd / k_agg_fwd_combine / k_agg_bwd_dst /
k_agg_bwd_combine (KgwLayerArgs.partial_rels), kgw_softmax_pack, kgw_softmax_merge, kgw_gather_rows / kgw_scatter_rows.

The reference is always the float64 oracle of tests/test_gpu_aggregate_parity.py on the UNSHARDED batch of the same seeds (never
the sharded code path), rows and edges matched through global node ids; node features are generated per global node, so every
rank and the unsharded batch see the same H.  Upstream gradient: a random G_p per rank on its own Z rows; the reference's G on a
row is the sum of the G_p of the ranks that hold it.

What is compared: the sampler's integer structures exactly; every rank's packed record (m, s, acc) of every exchanged segment
before the merge; Z, stat, e and alpha after it (and bit equality of the merged rows between the ranks); dH of every node, dU,
dV and d logit_bias summed over the ranks.  Tolerances: the project's (tests/test_gpu_aggregate_parity.py), unchanged -- RTOL
1e-4, ATOL 1e-5 (1e-4 for dU / dV / dlb, 2e-5 for dH), assert_close's rel_to_max, and for the quantities that hang on d a_dst
the _check_residue rule (norm error at most 2 x that of the float32 oracle of the unsharded layer).

Graphs: the degree ladder of the parity file (its 1000-edge row is 508/492, 329/341/330, 245/263/240/252 and 113..133 edges per
rank at P = 2, 3, 4, 8), the 1 % synthetic graph, the hand-made corner graph, and a RANK ladder (make_rank_ladder_graph) whose
LAD sources are placed by id range so that the rank-local degrees of its genes sit on both sides of 64, 128, 192 and 256 on
every rank, with rows that are multi-chunk on every rank, multi-chunk on some ranks and single-chunk on others, and empty on
some ranks; test_rank_ladder_realises_every_branch reads that back from the sampled rank batches."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests.helpers import assert_close, global_edge_set
from tests.shard_ranks import PS, W, make_ranks, run_layer, run_layer_on_ranks, sample_parts, sample_ranks
from tests.test_gpu_aggregate_parity import (ATOL, RTOL, _check_residue, _ladder_seeds, _minibatch, _run_oracle, layer_edges,
                                             make_degree_ladder_graph)
from tests.test_gpu_sampler import check_block_structures

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------------------
# graphs
# ------------------------------------------------------------------------------------------------------------------------------
RL_SNP, RL_GENE, RL_ANCHORS = 3200, 40, 8
RL_DEG = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257]


def rank_ladder_degrees(P):
    """[RL_GENE, P]: in-degree of every gene on relation ('SNP', 'LAD', 'Gene') from the SNPs of every rank's id range."""
    D = np.zeros((RL_GENE, P), dtype=np.int64)
    D[0] = 129                                # two chunks (128 + 1) on every rank
    D[1] = 129
    D[1, 0] = 128                             # one full chunk on rank 0, two chunks elsewhere
    D[2] = 127
    D[2, 0] = 0                               # no edge on rank 0
    D[3, P - 1] = 1                           # one edge in all, on the last rank
    D[4] = 300
    D[4, P - 1] = 0                           # three chunks everywhere but on the last rank, which has none
    for g in range(5, RL_GENE):
        for p in range(P):
            D[g, p] = RL_DEG[(3 * g + 5 * p) % len(RL_DEG)]
    return D


def rank_ladder_seeds():
    """One anchor SNP in every eighth of the id range (a seed on every rank for P = 1, 2, 3, 4, 8) and a few more."""
    anchors = [RL_SNP * k // RL_ANCHORS + 7 for k in range(RL_ANCHORS)]
    extra = np.random.default_rng(3).choice(RL_SNP, size=24, replace=False)
    return np.unique(np.concatenate([anchors, extra]))


def make_rank_ladder_graph(P):
    """SNP / Gene graph for P ranks: gene g has rank_ladder_degrees(P)[g, p] LAD in-edges from the SNP id range of rank p; every
    anchor SNP has a TSS edge to every gene, so with the anchors among the seeds every gene is a hop-1 node of the batch."""
    from kgwas_amd.graph import HeteroGraph, add_self_loops, to_undirected
    from kgwas_amd.shard import shard_range
    rng = np.random.default_rng(77 + P)
    n = OrderedDict([('SNP', RL_SNP), ('Gene', RL_GENE)])
    D = rank_ladder_degrees(P)
    src, dst = [], []
    for p in range(P):
        lo, hi = shard_range(RL_SNP, p, P)
        for g in range(RL_GENE):
            src.append(rng.choice(np.arange(lo, hi), size=int(D[g, p]), replace=False))
            dst.append(np.full(int(D[g, p]), g))
    lad = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    anchors = np.array([RL_SNP * k // RL_ANCHORS + 7 for k in range(RL_ANCHORS)])
    tss = np.stack([np.repeat(anchors, RL_GENE), np.tile(np.arange(RL_GENE), RL_ANCHORS)]).astype(np.int64)
    g2g = np.stack([rng.integers(0, RL_GENE, 30), rng.integers(0, RL_GENE, 30)]).astype(np.int64)
    e = OrderedDict([(('SNP', 'LAD', 'Gene'), lad), (('SNP', 'TSS', 'Gene'), tss), (('Gene', 'G2G', 'Gene'), g2g)])
    gen = torch.Generator().manual_seed(6)
    data = HeteroGraph()
    for t, k in n.items():
        data[t].x = torch.rand(k, 16, generator=gen)
    und = add_self_loops(to_undirected(e, n), n)
    for et, ei in und.items():
        data[et].edge_index = torch.from_numpy(np.ascontiguousarray(ei))
    data['SNP'].y = torch.rand(RL_SNP, generator=gen)
    return data


_GRAPHS, _RANKS, _UNSHARDED = {}, {}, {}


@pytest.fixture
def world(small_kg, edge_case_graph):
    """world(name, P) -> (graph, seeds, the unsharded batch, the P sampled ranks); cached for the module."""
    def graph(name, P):
        key = (name, P if name == 'rankladder' else 0)
        if key not in _GRAPHS:
            if name == 'ladder':
                _GRAPHS[key] = (make_degree_ladder_graph(), _ladder_seeds())
            elif name == 'rankladder':
                _GRAPHS[key] = (make_rank_ladder_graph(P), rank_ladder_seeds())
            elif name == 'small':
                data = small_kg.data
                _GRAPHS[key] = (data, np.random.default_rng(0).choice(int(data['SNP'].num_nodes), size=96, replace=False))
            else:
                data = edge_case_graph[0]
                _GRAPHS[key] = (data, np.random.default_rng(0).choice(int(data['SNP'].num_nodes), size=64, replace=False))
        return key, _GRAPHS[key]

    def get(name, P):
        key, (data, seeds) = graph(name, P)
        if key not in _UNSHARDED:
            _UNSHARDED[key] = _minibatch(data, seeds)
        if (key, P) not in _RANKS:
            _RANKS[(key, P)] = sample_ranks(make_ranks(data, seeds, P))
        return data, seeds, _UNSHARDED[key], _RANKS[(key, P)]
    return get


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the sampler in parts against the unsharded sampler
# ------------------------------------------------------------------------------------------------------------------------------
def _step_arrays(dg, buf, meta):
    """Every array of a sampled batch that a training step reads, cut to the lengths the batch uses."""
    sc, L, Hn = dg.schema, dg.num_layers, dg.n_hops
    ns, ne, nc = int(meta.seg_end[Hn - 1]), int(meta.edge_end[Hn - 1]), int(meta.chunk_end[Hn - 1])
    out = OrderedDict(g2l=buf.g2l, n_id=buf.n_id, meta=buf.meta, seg_ptr=buf.seg_ptr[:ns + 1], seg_chptr=buf.seg_chptr[:ns + 1],
                      col_local=buf.col_local[:ne], chunks=buf.chunks[:nc * 8])
    for h in range(Hn):
        # (the list of a hop's multi-chunk segments is filled in arrival order -- k_fill_chunks takes the slots with an atomic
        #  counter -- and every entry is combined by a wavefront of its own: its ORDER is not part of the structure, two runs of the
        #  same call differ in it.  Compared as the sorted set of its (first chunk, chunks, row, relation) records.)
        mm = buf.multi[h * dg.multi_cap * 4:(h * dg.multi_cap + int(meta.multi_cnt[h])) * 4].view(-1, 4).cpu().numpy()
        out[f'multi[{h}]'] = torch.from_numpy(mm[np.lexsort(mm.T[::-1])].copy())
    for l in range(L):
        nt, tr = int(meta.t_entries[l]), int(meta.t_base[l][sc.NT])
        out[f't_ptr[{l}]'] = buf.t_ptr[l][:tr + 1]
        out[f't_edge[{l}]'] = buf.t_edge[l][:nt]
        out[f't_zrow[{l}]'] = buf.t_zrow[l][:nt]
        out[f't_rel[{l}]'] = buf.t_rel[l][:nt]
        out[f'oct_flags[{l}]'] = buf.t_cnt[l][:(int(meta.src_base[l][sc.NT]) + 7) // 8]
    return out


SAMPLER_CASES = [(g, P) for g in ('ladder', 'small', 'edge', 'rankladder') for P in (1, 2, 3, 4, 8)]


@pytest.mark.parametrize('name,P', SAMPLER_CASES, ids=[f'{g}-P{P}' for g, P in SAMPLER_CASES])
def test_sampler_in_parts_equals_the_unsharded_sampler(world, name, P):
    """Integers: exact.  P = 1 in 2 n_hops + 1 separate parts writes the buffers of the plain kgw_sample_batch call bit for bit;
    on P ranks every replicated type has the unsharded batch's nodes, hop boundaries and local order, the ranks' edges with a
    sharded endpoint are disjoint and add up to the unsharded batch's, and no KGW_PENDING flag is left."""
    from kgwas_amd.sampler import BatchBuffers, sample_into
    from kgwas_amd.shard import KGW_PENDING
    data, seeds, ub, ranks = world(name, P)
    assert all(int(rk.seeds.numel()) > 0 for rk in ranks) and sum(int(rk.seeds.numel()) for rk in ranks) == len(seeds)
    if P == 1:
        rk = ranks[0]
        a, b = BatchBuffers(rk.dg), BatchBuffers(rk.dg)
        sample_into(rk.dg, a, rk.seeds, rk.seed_type)
        for part in range(2 * rk.dg.n_hops + 1):
            sample_parts(rk.dg, b, rk.seeds, rk.seed_type, part, part)
        torch.cuda.synchronize()
        ma, mb = a.read_meta(), b.read_meta()
        assert bytes(ma) == bytes(mb) and not ma.error
        xa, xb = _step_arrays(rk.dg, a, ma), _step_arrays(rk.dg, b, mb)
        for k in xa:
            assert torch.equal(xa[k], xb[k]), k
        xr = _step_arrays(rk.dg, rk.buf, rk.batch.meta)          # (the rank loop itself: parts 0, 1 .. 2 n_hops)
        for k in xa:
            assert torch.equal(xa[k], xr[k]), k
    sc = ub.dg.schema
    for rk in ranks:
        assert not bool((rk.buf.g2l == KGW_PENDING).any()), f'rank {rk.p}: a PENDING flag is left in g2l'
        for t in data.node_types:
            if t == 'SNP':
                own = rk.batch.n_id(t).long() + rk.lo
                assert bool(((own >= rk.lo) & (own < rk.hi)).all())
                continue
            ti = sc.type_id[t]
            assert torch.equal(rk.batch.n_id(t), ub.n_id(t)), f'rank {rk.p}: nodes / local order of {t}'
            assert [int(rk.batch.meta.node_off[ti][k]) for k in range(ub.dg.n_hops + 2)] == \
                [int(ub.meta.node_off[ti][k]) for k in range(ub.dg.n_hops + 2)], f'rank {rk.p}: hop boundaries of {t}'
    snp_u = np.sort(ub.n_id('SNP').cpu().numpy())
    snp_r = np.sort(np.concatenate([(rk.batch.n_id('SNP').long() + rk.lo).cpu().numpy() for rk in ranks]))
    assert np.array_equal(snp_u, snp_r), 'the ranks\' SNP nodes are not a partition of the unsharded batch\'s'
    for et in data.edge_types:
        want = global_edge_set(ub, et)
        s, _, d = et
        if 'SNP' not in (s, d):
            for rk in ranks:
                assert np.array_equal(global_edge_set(rk.batch, et), want), f'rank {rk.p}: replicated relation {et}'
            continue
        col = 0 if s == 'SNP' else 1
        parts = []
        for rk in ranks:
            pairs = global_edge_set(rk.batch, et).copy()
            pairs[:, col] += rk.lo
            assert np.all((pairs[:, col] >= rk.lo) & (pairs[:, col] < rk.hi)), f'rank {rk.p}: {et} holds an edge it does not own'
            parts.append(pairs)
        got = np.concatenate(parts)
        got = got[np.lexsort((got[:, 0], got[:, 1]))]
        assert np.array_equal(got, want), f'{et}: the union of the ranks\' edges is not the unsharded batch\'s'


STRUCT_CASES = [('ladder', 1), ('ladder', 2), ('ladder', 4), ('rankladder', 2), ('rankladder', 3), ('rankladder', 4), ('rankladder', 8)]


@pytest.mark.parametrize('name,P', STRUCT_CASES, ids=[f'{g}-P{P}' for g, P in STRUCT_CASES])
def test_block_structures_of_rank_local_batches(world, name, P):
    """tests/test_gpu_sampler.py's structure checks (chunks, multi-chunk list, src-major tables, octet flags) on every rank's
    batch -- the cases where every rank holds a row above KGW_CHUNK edges, which those checks require."""
    for rk in world(name, P)[3]:
        check_block_structures(rk.batch)


def _exchanged_segments(rk, layer=1):
    """{(relation, destination row): chunk lengths} of the exchanged relations' non-empty segments on one rank."""
    m = rk.batch.meta
    nc = int(m.n_chunks[layer - 1])
    ch = rk.buf.chunks[:nc * 8].view(-1, 8).cpu().numpy()
    out = {}
    for e0, e1, row, rel, first, nch, _, _ in ch:
        if (rk.xchg.mask[layer] >> int(rel)) & 1:
            out.setdefault((int(rel), int(row)), []).append(int(e1 - e0))
    return out


@pytest.mark.parametrize('P', [2, 3, 4, 8])
def test_rank_ladder_realises_every_branch(world, P):
    """Read back from the sampled rank batches: the rank-local degrees are the builder's, some exchanged segment is multi-chunk
    on every rank, some is multi-chunk on one rank and single-chunk on another, some has a rank without an edge, and the
    rank-local chunk lengths hit 0, 1 and 63 mod 64 and the degrees 127, 128 and 129."""
    data, seeds, ub, ranks = world('rankladder', P)
    sc = ub.dg.schema
    r = sc.edge_types.index(('SNP', 'LAD', 'Gene'))
    assert all((rk.xchg.mask[1] >> r) & 1 for rk in ranks)
    genes = ub.n_id('Gene').cpu().numpy()
    n_rows = int(ub.meta.n_rows[0][sc.type_id['Gene']])
    assert n_rows == RL_GENE, 'every gene is a hop-1 node of the batch'
    D = rank_ladder_degrees(P)
    segs = [_exchanged_segments(rk) for rk in ranks]
    nch = np.zeros((RL_GENE, P), dtype=np.int64)
    lens = set()
    for p, sg in enumerate(segs):
        for (rel, row), v in sg.items():
            if rel == r:
                assert sum(v) == D[genes[row], p], (p, row)
                nch[genes[row], p] = len(v)
                lens.update(v)
    assert np.array_equal(nch, (D + 127) // 128)
    print(f'rank ladder P={P}: chunks per (gene, rank) {sorted(set(nch.ravel().tolist()))}, chunk lengths {sorted(lens)}')
    assert bool((nch > 1).all(1).any()), 'no segment is multi-chunk on every rank'
    assert bool(((nch > 1).any(1) & (nch == 1).any(1)).any()), 'no segment is multi-chunk on one rank and single-chunk on another'
    assert bool(((nch == 0).any(1) & (nch > 0).any(1)).any()), 'no non-empty segment has a rank without an edge'
    assert {0, 1, 63} <= {k % 64 for k in lens}
    assert {127, 128, 129} <= set(D.ravel().tolist())


@pytest.mark.parametrize('P,hub,empty', [(2, [508, 492], 17), (3, [329, 341, 330], 46), (4, [245, 263, 240, 252], 73),
                                         (8, [132, 113, 130, 133, 125, 115, 131, 121], 181)])
def test_degree_ladder_per_rank(world, P, hub, empty):
    """The parity file's ladder, read back from the sampled rank batches: the 1000-edge LAD row's edges per rank and the number of
    non-empty LAD segments that have a rank without an edge (figures computed on the CPU from the graph builder)."""
    data, seeds, ub, ranks = world('ladder', P)
    sc = ub.dg.schema
    r = sc.edge_types.index(('SNP', 'LAD', 'Gene'))
    n_rows = int(ub.meta.n_rows[0][sc.type_id['Gene']])
    deg = np.zeros((n_rows, P), dtype=np.int64)
    nch = np.zeros((n_rows, P), dtype=np.int64)
    for p, rk in enumerate(ranks):
        for (rel, row), v in _exchanged_segments(rk).items():
            if rel == r:
                deg[row, p], nch[row, p] = sum(v), len(v)
    tot = deg.sum(1)
    assert int(tot.max()) == 1000 and deg[tot.argmax()].tolist() == hub
    assert nch[tot.argmax()].tolist() == [(k + 127) // 128 for k in hub]
    assert int(((tot > 0) & (deg.min(1) == 0)).sum()) == empty


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the layer: partial states, merge and backward against the float64 oracle of the unsharded batch
# ------------------------------------------------------------------------------------------------------------------------------
def _tables(data, sc, seed, relu_input=False, lbias=False, u_scale=0.2, v_scale=0.2):
    """Node features per GLOBAL node (one float32 table per node type) and the relation vectors."""
    g = torch.Generator().manual_seed(seed)
    T = OrderedDict()
    for t in sc.node_types:
        T[t] = torch.randn(int(data[t].num_nodes), W, generator=g)
        if relu_input:
            T[t] = torch.relu(T[t])
    U = torch.randn(sc.NR, W, generator=g) * u_scale
    V = torch.randn(sc.NR, W, generator=g) * v_scale
    kap = torch.randn(sc.NR, generator=g) * 0.5 if lbias else None
    return T, U, V, kap


def _layer_H(batch, layer, T, lo=0):
    m, sc = batch.meta, batch.dg.schema
    H = torch.zeros(int(m.src_base[layer - 1][sc.NT]), W)
    for ti, t in enumerate(sc.node_types):
        n = int(m.n_src[layer - 1][ti])
        ids = batch.n_id(t)[:n].long().cpu() + (lo if t == 'SNP' else 0)
        a = int(m.src_base[layer - 1][ti])
        H[a:a + n] = T[t][ids]
    return H


def _row_maps(data, rk, ub, layer):
    """(local node -> unsharded local node per type, H row -> unsharded H row, Z row -> unsharded Z row) of one rank."""
    mp, mu, sc = rk.batch.meta, ub.meta, ub.dg.schema
    lmap = {}
    hmap = torch.full((int(mp.src_base[layer - 1][sc.NT]),), -1, dtype=torch.long)
    zmap = torch.full((int(mp.z_base[layer - 1][sc.NT]),), -1, dtype=torch.long)
    for ti, t in enumerate(sc.node_types):
        loc = torch.full((int(data[t].num_nodes),), -1, dtype=torch.long)
        loc[ub.n_id(t).long().cpu()] = torch.arange(int(ub.n_nodes[t]))
        n = int(mp.n_src[layer - 1][ti])
        lm = loc[rk.batch.n_id(t)[:n].long().cpu() + (rk.lo if t == 'SNP' else 0)]
        assert bool(((lm >= 0) & (lm < int(mu.n_src[layer - 1][ti]))).all()), t
        lmap[ti] = lm
        a = int(mp.src_base[layer - 1][ti])
        hmap[a:a + n] = int(mu.src_base[layer - 1][ti]) + lm
        nr, R = int(mp.n_rows[layer - 1][ti]), int(sc.R_dst[ti])
        if nr and R:
            assert bool((lm[:nr] < int(mu.n_rows[layer - 1][ti])).all()), t
            zp = int(mp.z_base[layer - 1][ti]) + torch.arange(nr)[:, None] * R + torch.arange(R)[None, :]
            zmap[zp.reshape(-1)] = (int(mu.z_base[layer - 1][ti]) + lm[:nr, None] * R + torch.arange(R)[None, :]).reshape(-1)
    assert bool((hmap >= 0).all()) and bool((zmap >= 0).all())
    return lmap, hmap, zmap


def _match_edges(edges_p, lmap, edges_u, sc):
    """{relation: unsharded local edge id of every edge of the rank} (duplicate edges carry equal values: any twin will do)."""
    out = {}
    for r, (eid, src, dst) in edges_p.items():
        s, d = int(sc.src_type[r]), int(sc.dst_type[r])
        eu, su, du = edges_u[r]
        ku = su * (1 << 32) + du
        order = torch.argsort(ku)
        kp = lmap[s][src] * (1 << 32) + lmap[d][dst]
        pos = torch.searchsorted(ku[order], kp)
        assert bool((pos < ku.numel()).all()) and bool((ku[order][pos] == kp).all()), f'relation {r}: an edge the unsharded batch lacks'
        out[r] = eu[order][pos]
    return out


def _maxerr(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max()) if torch.as_tensor(a).numel() else 0.0


def check_sharded_case(data, ub, ranks, seed, layer=1, slope=0.2, temp=1.0, relu_input=False, lbias=False, u_scale=0.2,
                       v_scale=0.2, spike_rank=None, order=None, tag=''):
    sc, dg = ub.dg.schema, ub.dg
    P = len(ranks)
    T, U, V, kap = _tables(data, sc, seed, relu_input, lbias, u_scale, v_scale)
    edges_u = layer_edges(ub, layer)
    r_lad = None
    if spike_rank is not None:          # one SNP source of the widest exchanged row, owned by ``spike_rank``: logit 3 |u_r|^2
        r_lad = max((r for r in edges_u if (ranks[0].xchg.mask[layer] >> r) & 1), key=lambda r: int(torch.bincount(edges_u[r][2]).max()))
        eid, src, dst = edges_u[r_lad]
        hub = int(torch.bincount(dst).argmax())
        gids = ub.n_id('SNP').long().cpu()[src[dst == hub]]
        rk = ranks[spike_rank]
        spike_gid = int(gids[(gids >= rk.lo) & (gids < rk.hi)][0])
        T['SNP'][spike_gid] = 3.0 * U[r_lad]
    Hu = _layer_H(ub, layer, T)
    Hs = [_layer_H(rk.batch, layer, T, rk.lo) for rk in ranks]
    maps = [_row_maps(data, rk, ub, layer) for rk in ranks]
    Gs = []
    for rk in ranks:
        g = torch.Generator().manual_seed(1000 * seed + rk.p)
        Gs.append(torch.randn(int(rk.batch.meta.z_base[layer - 1][sc.NT]), W, generator=g))
    Gu = torch.zeros(int(ub.meta.z_base[layer - 1][sc.NT]), W, dtype=torch.float64)
    cover_h = torch.zeros(Hu.shape[0], dtype=torch.long)
    for (lmap, hmap, zmap), G in zip(maps, Gs):
        Gu.index_add_(0, zmap, G.double())
        cover_h.index_add_(0, hmap, torch.ones_like(hmap))
    snp = sc.type_id['SNP']
    for ti in range(sc.NT):               # a sharded node lives on exactly one rank, a replicated one on all
        a, n = int(ub.meta.src_base[layer - 1][ti]), int(ub.meta.n_src[layer - 1][ti])
        assert bool((cover_h[a:a + n] == (1 if ti == snp else P)).all()), sc.node_types[ti]

    outs, run = run_layer_on_ranks(ranks, layer, Hs, U, V, kap, Gs, slope, temp, relu_input, order=order)
    ref = _run_oracle(ub, layer, Hu, U, V, kap, Gu, torch.float64, slope, temp, relu_input, edges_u)
    cache = {}

    def lazy32():
        if not cache:
            cache.update(_run_oracle(ub, layer, Hu, U, V, kap, Gu, torch.float32, slope, temp, relu_input, edges_u))
        return cache

    live = [r for r in range(sc.NR) if dg.kg.rel_live[layer - 1][r]]
    dead = [r for r in range(sc.NR) if not dg.kg.rel_live[layer - 1][r]]
    mask = ranks[0].xchg.mask[layer]
    assert mask and all(rk.xchg.mask[layer] == mask for rk in ranks)
    Hu64 = Hu.double()
    alpha_sum = torch.zeros(Gu.shape[0], dtype=torch.float64)
    has_edge = torch.zeros(Gu.shape[0], dtype=torch.bool)
    err = OrderedDict((k, 0.0) for k in ('m', 's', 'acc', 'Z', 'stat', 'e', 'alpha'))
    merged = []
    n_absent = 0
    for rk, out, (lmap, hmap, zmap) in zip(ranks, outs, maps):
        mp = rk.batch.meta
        edges_p = layer_edges(rk.batch, layer)
        match = _match_edges(edges_p, lmap, edges_u, sc)
        z_rows = int(mp.z_base[layer - 1][sc.NT])
        # -- before the merge: the packed record of every exchanged segment against the float64 partial state over this rank's edges
        rm = torch.zeros(z_rows, dtype=torch.float64)
        rs = torch.zeros(z_rows, dtype=torch.float64)
        racc = torch.zeros(z_rows, W, dtype=torch.float64)
        for r, (eid, src, dst) in edges_p.items():
            d, s = int(sc.dst_type[r]), int(sc.src_type[r])
            zrow = int(mp.z_base[layer - 1][d]) + dst * int(sc.R_dst[d]) + int(sc.slot_dst[r])
            has_edge[zmap[zrow]] = True
            if not (mask >> r) & 1:
                continue
            t = ref['e'][match[r]] / temp
            nr = int(mp.n_rows[layer - 1][d])
            mx = torch.full((nr,), float('-inf'), dtype=torch.float64).scatter_reduce(0, dst, t, reduce='amax')
            w = (t - mx[dst]).exp()
            rows = torch.unique(dst)
            zr = int(mp.z_base[layer - 1][d]) + rows * int(sc.R_dst[d]) + int(sc.slot_dst[r])
            rm[zr] = mx[rows]
            rs[zr] = torch.zeros(nr, dtype=torch.float64).index_add(0, dst, w)[rows]
            hsrc = Hu64[int(ub.meta.src_base[layer - 1][s]) + lmap[s][src]]
            racc[zr] = torch.zeros(nr, W, dtype=torch.float64).index_add(0, dst, w[:, None] * hsrc)[rows]
        seg = rk.xchg.seg_rows(rk.batch, layer).long().cpu()
        rec = run.records[rk.p].view(-1, PS).cpu()
        assert rec.shape[0] == seg.numel() and not bool(torch.isnan(rec).any())
        assert float(rec[:, 2:4].abs().sum()) == 0.0, 'words 2 and 3 of a packed record are zero'
        present = rs[seg] > 0
        n_absent += int((~present).sum())
        assert float(rec[~present].abs().sum()) == 0.0, f'rank {rk.p}: a segment without an edge must pack exactly (0, 0, 0...)'
        assert_close(rec[present, 0], rm[seg][present], RTOL, ATOL, f'rank {rk.p} packed m')
        assert_close(rec[present, 1], rs[seg][present], RTOL, ATOL, f'rank {rk.p} packed s')
        assert_close(rec[present, 4:], racc[seg][present], RTOL, ATOL, f'rank {rk.p} packed acc')
        err['m'] = max(err['m'], _maxerr(rec[present, 0], rm[seg][present]))
        err['s'] = max(err['s'], _maxerr(rec[present, 1], rs[seg][present]))
        err['acc'] = max(err['acc'], _maxerr(rec[present, 4:], racc[seg][present]))
        # -- after the merge: every Z row and stat pair of the rank (exchanged or not) against the oracle's
        assert_close(out['Z'], ref['Z'][zmap], RTOL, ATOL, f'rank {rk.p} Z')
        assert_close(out['stat'], ref['stat'][zmap], RTOL, ATOL, f'rank {rk.p} stat')
        empty = ref['stat'][zmap][:, 1] == 0
        assert float(out['Z'][empty].abs().sum()) == 0.0 and float(out['stat'][empty].abs().sum()) == 0.0, \
            f'rank {rk.p}: a segment no rank has an edge of must be exactly zero with stat (0, 0)'
        merged.append((out['Z'][seg], out['stat'][seg]))
        eid = torch.cat([edges_p[r][0] for r in edges_p])
        mu = torch.cat([match[r] for r in edges_p])
        assert_close(out['e'][eid], ref['e'][mu], RTOL, ATOL, f'rank {rk.p} e_edge')
        assert_close(out['alpha'][eid], ref['alpha'][mu], RTOL, ATOL, f'rank {rk.p} alpha')
        for k, a, b in (('Z', out['Z'], ref['Z'][zmap]), ('stat', out['stat'], ref['stat'][zmap]), ('e', out['e'][eid], ref['e'][mu]),
                        ('alpha', out['alpha'][eid], ref['alpha'][mu])):
            err[k] = max(err[k], _maxerr(a, b))
        for r, (e_, src, dst) in edges_p.items():
            d = int(sc.dst_type[r])
            zrow = int(mp.z_base[layer - 1][d]) + dst * int(sc.R_dst[d]) + int(sc.slot_dst[r])
            # (a replicated relation's edges are on every rank: count them once)
            if (mask >> r) & 1 or int(sc.dst_type[r]) == snp or rk.p == 0:
                alpha_sum.index_add_(0, zmap[zrow], out['alpha'][e_].double())
        if relu_input:
            H = Hs[rk.p]
            assert bool((H == 0).any()) and float(out['dH'][H == 0].abs().max()) == 0.0
        assert float(out['dU'][dead].abs().sum()) == 0.0 and float(out['dV'][dead].abs().sum()) == 0.0
        if lbias:
            assert float(out['dlb'][dead].abs().sum()) == 0.0
    for p in range(1, P):
        assert torch.equal(merged[p][0], merged[0][0]) and torch.equal(merged[p][1], merged[0][1]), \
            f'the merged rows of rank {p} differ from rank 0\'s in bits'
    assert bool(has_edge.any()) and float((alpha_sum[has_edge] - 1.0).abs().max()) <= 1e-5, float((alpha_sum[has_edge] - 1.0).abs().max())
    assert float(alpha_sum[~has_edge].abs().sum()) == 0.0
    # -- backward: sums over the ranks
    dH = torch.zeros(Hu.shape[0], W, dtype=torch.float64)
    for out, (lmap, hmap, zmap) in zip(outs, maps):
        dH.index_add_(0, hmap, out['dH'].double())
    dU = sum(out['dU'].double() for out in outs)
    dV = sum(out['dV'].double() for out in outs)
    assert_close(dU[live], ref['dU'][live], RTOL, 1e-4, 'dU summed over the ranks')
    _check_residue('dH', dH, ref['dH'], lazy32, 2e-5)
    _check_residue('dV', dV[live], ref['dV'][live], lambda: {'dV': lazy32()['dV'][live]}, 1e-4)
    err.update(dH=_maxerr(dH, ref['dH']), dU=_maxerr(dU[live], ref['dU'][live]), dV=_maxerr(dV[live], ref['dV'][live]))
    if lbias:
        dlb = sum(out['dlb'].double() for out in outs)
        _check_residue('dlb', dlb[live], ref['dlb'][live], lambda: {'dlb': lazy32()['dlb'][live]}, 1e-4)
        err['dlb'] = _maxerr(dlb[live], ref['dlb'][live])
    print(f'shard-kernels {tag} P={P}: absent (segment, rank) pairs {n_absent}; max abs error ' +
          ', '.join(f'{k} {v:.2e}' for k, v in err.items()))
    return dict(ref=ref, outs=outs, run=run, maps=maps, r_spike=r_lad, edges_u=edges_u)


PLAIN = [('ladder', 2), ('ladder', 3), ('ladder', 4), ('ladder', 8), ('small', 2), ('small', 4), ('edge', 2),
         ('rankladder', 2), ('rankladder', 3), ('rankladder', 4), ('rankladder', 8)]


@pytest.mark.parametrize('name,P', PLAIN, ids=[f'{g}-P{P}' for g, P in PLAIN])
def test_sharded_layer_against_the_unsharded_oracle(world, name, P):
    data, seeds, ub, ranks = world(name, P)
    check_sharded_case(data, ub, ranks, seed=40 + P, lbias=(P % 2 == 1), tag=name)


# (relu_input, logit_bias, no riders, no short-row path): the pairwise cover of the parity file, without its all-default case
OPTIONS = [(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 1)]
OPTION_GRAPHS = [('ladder', 2), ('ladder', 3), ('ladder', 8), ('small', 4)]


@pytest.mark.parametrize('opts', OPTIONS, ids=lambda o: 'relu{}-lb{}-noriders{}-noshort{}'.format(*o))
@pytest.mark.parametrize('name,P', OPTION_GRAPHS, ids=[f'{g}-P{P}' for g, P in OPTION_GRAPHS])
def test_sharded_layer_option_matrix(world, monkeypatch, name, P, opts):
    from kgwas_amd import ops
    relu_input, lbias, no_riders, no_short = map(bool, opts)
    monkeypatch.setattr(ops, '_DUV_RIDERS', not no_riders)
    monkeypatch.setattr(ops, '_SHORT_ROWS', not no_short)
    data, seeds, ub, ranks = world(name, P)
    check_sharded_case(data, ub, ranks, seed=200 + sum(o << i for i, o in enumerate(opts)), relu_input=relu_input, lbias=lbias,
                       tag=f'{name} options {opts}')


@pytest.mark.parametrize('slope', [0.05, 0.5])
@pytest.mark.parametrize('temp', [0.5, 2.5])
def test_sharded_layer_at_other_slopes_and_temperatures(world, slope, temp):
    data, seeds, ub, ranks = world('ladder', 4)
    check_sharded_case(data, ub, ranks, seed=31, slope=slope, temp=temp, lbias=True, tag=f'ladder slope {slope} T {temp}')


@pytest.mark.parametrize('P,where', [(2, 'first'), (2, 'last'), (4, 'first'), (4, 'last')])
def test_spike_on_one_rank_underflows_the_other_ranks_factors(world, P, where):
    """One SNP source of the 1000-edge row gets a logit ~35 x the others': its rank's m_p exceeds every other rank's by more than
    fp32 exp can represent, the other ranks' factors exp(m_p - m*) are 0 in the merge, and the result must still match, forward
    and backward."""
    data, seeds, ub, ranks = world('ladder', P)
    spike_rank = 0 if where == 'first' else P - 1
    res = check_sharded_case(data, ub, ranks, seed=9, u_scale=1.0, v_scale=0.1, lbias=True, spike_rank=spike_rank,
                             tag=f'ladder spike on rank {spike_rank}')
    r = res['r_spike']
    eid, src, dst = res['edges_u'][r]
    hub = int(torch.bincount(dst).argmax())
    assert float(res['ref']['alpha'][eid[dst == hub]].max()) > 0.99
    sc = ub.dg.schema
    gene = sc.type_id['Gene']
    m = []
    for rk in ranks:             # the hub row's packed m on every rank (Gene rows are the same local rows on every rank)
        seg = rk.xchg.seg_rows(rk.batch, 1).long().cpu()
        z = int(rk.batch.meta.z_base[0][gene]) + hub * int(sc.R_dst[gene]) + int(sc.slot_dst[r])
        k = int(torch.nonzero(seg == z)[0])
        m.append(float(res['run'].records[rk.p].view(-1, PS)[k, 0]))
    others = [v for p, v in enumerate(m) if p != spike_rank]
    assert m[spike_rank] - max(others) > 104.0, m          # exp(-104) < the smallest fp32 denormal


def test_a_broken_exchange_is_noticed(world):
    """The harness can tell a broken exchange from a working one: a rank that misses the frontier merge samples other replicated
    nodes than its peers, and a rank that concatenates the records in another order than its peers merges other bits."""
    data, seeds, ub, ranks = world('ladder', 3)
    broken = sample_ranks(make_ranks(data, seeds, 3), no_merge=(1,))
    same = [torch.equal(rk.batch.n_id('Gene'), ub.n_id('Gene')) for rk in broken]
    assert same == [True, False, True], same
    with pytest.raises(AssertionError, match='differ from rank 0'):
        check_sharded_case(data, ub, ranks, seed=43, order={2: [2, 1, 0]}, tag='ladder, rank 2 merges in reverse order')


_KEYS = ('Z', 'stat', 'e', 'alpha', 'dH', 'dU', 'dV', 'dlb')


def test_one_rank_with_the_exchange_is_the_single_gpu_layer(world):
    """shard.py: "With P = 1 every collective is the identity and the step is the single-GPU step" -- per kernel: partial state,
    pack, merge of one record, gather / scatter of the dZ rows, against the plain call without an exchange object.

    Bit-identical: Z, stat, e, alpha, dU and the dH rows of the sharded type.  NOT bit-identical (measured on an MI355X): dV,
    d logit_bias and the dH rows of the replicated types.  Why: with partial_rels set, k_agg_bwd_dst / k_agg_bwd_combine leave
    d a_dst of an exchanged row as the plain sum over the rank's edges (`tot`), because the row-consistent correction
    `tot - (te / ts) * tb` of the plain call is a property of the WHOLE row, which a rank does not see; at P = 1 the two forms
    are the same number up to round-off but not the same bits.  d a_dst feeds dV, d logit_bias and the destination rows' dH, and
    nothing else.  Those three are held to the project's tolerances against the float64 oracle instead (check_sharded_case)."""
    data, seeds, ub, ranks = world('ladder', 1)
    rk = ranks[0]
    sc = rk.dg.schema
    T, U, V, kap = _tables(data, sc, 5, lbias=True)
    H = _layer_H(rk.batch, 1, T)
    G = torch.randn(int(rk.batch.meta.z_base[0][sc.NT]), W, generator=torch.Generator().manual_seed(6))
    assert rk.batch.exchange is None
    plain = run_layer(rk.batch, 1, H, U, V, kap, G)
    outs, run = run_layer_on_ranks(ranks, 1, [H], U, V, kap, [G])
    diff = [k for k in _KEYS if not torch.equal(outs[0][k], plain[k])]
    print('P = 1 with the exchange attached vs the plain call: not bit-identical:', diff or 'nothing')
    assert set(diff) <= {'dH', 'dV', 'dlb'}, diff
    snp = sc.type_id['SNP']
    a, n = int(rk.batch.meta.src_base[0][snp]), int(rk.batch.meta.n_src[0][snp])
    assert torch.equal(outs[0]['dH'][a:a + n], plain['dH'][a:a + n]), 'dH of the sharded type\'s rows'
    check_sharded_case(data, ub, ranks, seed=5, lbias=True, tag='ladder, one rank')


@pytest.mark.parametrize('P', [1, 2])
def test_layer_two_has_nothing_to_exchange(world, P):
    """No exchange relation reaches the seeds: the mask of layer 2 is 0 and the call with the exchange object attached equals the
    call without it bit for bit (the object's forward / backward must not be reached)."""
    data, seeds, ub, ranks = world('ladder', P)
    for rk in ranks:
        sc = rk.dg.schema
        assert rk.xchg.mask[2] == 0
        T, U, V, kap = _tables(data, sc, 8, lbias=True)
        H = _layer_H(rk.batch, 2, T, rk.lo)
        G = torch.randn(int(rk.batch.meta.z_base[1][sc.NT]), W, generator=torch.Generator().manual_seed(2))
        plain = run_layer(rk.batch, 2, H, U, V, kap, G)

        class Untouched:
            staged, mask = False, rk.xchg.mask

            def forward(self, *a):
                raise AssertionError('layer 2 reached the exchange')
            backward = forward
        rk.batch.exchange = Untouched()
        try:
            with_x = run_layer(rk.batch, 2, H, U, V, kap, G)
        finally:
            rk.batch.exchange = None
        for k in _KEYS:
            assert torch.equal(with_x[k], plain[k]), k


# ------------------------------------------------------------------------------------------------------------------------------
# 4. kgw_softmax_merge, kgw_softmax_pack, kgw_scatter_rows on synthetic data
# ------------------------------------------------------------------------------------------------------------------------------
def _lib_and_stream():
    from kgwas_amd import _lib
    return _lib.lib(), _lib.stream_ptr()


KINDS = ('all', 'one', 'none', 'far_below', 'spread', 'absent_big_m', 'negative')


def _states(n_ranks, n_seg, seed):
    """[n_ranks, n_seg, 132] float32 records; segment x is of kind KINDS[x % 7]."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(n_ranks, n_seg, generator=g) * 5
    s = 10.0 ** (torch.rand(n_ranks, n_seg, generator=g) * 6)                 # 1 .. 1e6
    acc = torch.randn(n_ranks, n_seg, W, generator=g) * s[..., None]
    kind = torch.arange(n_seg) % len(KINDS)
    who = torch.randint(0, n_ranks, (n_seg,), generator=g)
    rank = torch.arange(n_ranks)[:, None]
    present = torch.ones(n_ranks, n_seg, dtype=torch.bool)
    present[:, kind == 1] = (rank == who[None, :])[:, kind == 1]              # exactly one rank present
    present[:, kind == 2] = False                                             # no rank present
    far = (kind == 3)[None, :] & (rank == who[None, :]) & (n_ranks > 1)
    m = torch.where(far, m.max(0).values[None, :] - 200.0, m)                 # a present rank 200 below m*
    m = torch.where((kind == 4)[None, :], (torch.rand(n_ranks, n_seg, generator=g) - 0.5) * 160, m)      # spread over +-80
    absent_big = (kind == 5)[None, :] & (rank == who[None, :]) & (n_ranks > 1)
    present &= ~absent_big
    m = torch.where((kind == 6)[None, :], -m.abs() - 5, m)                    # negative-only maxima
    m = torch.where(present, m, torch.zeros(()))
    m = torch.where(absent_big, torch.full((), 1e3), m)                       # absent, yet a large positive m: must not lift m*
    s = torch.where(present, s, torch.zeros(()))
    acc = torch.where(present[..., None], acc, torch.zeros(()))
    parts = torch.zeros(n_ranks, n_seg, PS)
    parts[..., 0], parts[..., 1], parts[..., 4:] = m, s, acc
    return parts


def _merge_ref(parts):
    """The header's formula in float64: Z = sum_p acc_p e^(m_p - m*) / (sum_p s_p e^(m_p - m*) + 1e-16), m* over s_p > 0."""
    p = parts.double()
    m, s, acc = p[..., 0], p[..., 1], p[..., 4:]
    present = s > 0
    any_ = present.any(0)
    mstar = torch.where(present, m, torch.full((), float('-inf'), dtype=torch.float64)).max(0).values
    mstar = torch.where(any_, mstar, torch.zeros((), dtype=torch.float64))
    f = torch.where(present, (m - mstar[None, :]).exp(), torch.zeros((), dtype=torch.float64))
    den = (s * f).sum(0) + 1e-16
    Z = torch.where(any_[:, None], (acc * f[..., None]).sum(0) / den[:, None], torch.zeros((), dtype=torch.float64))
    stat = torch.stack([mstar, torch.where(any_, den, torch.zeros((), dtype=torch.float64))], 1)
    return Z, stat


def _merge(parts, seg, n_z):
    L, st = _lib_and_stream()
    n_ranks, n_seg = parts.shape[:2]
    Z = torch.full((n_z, W), float('nan'), device='cuda')
    stat = torch.full((n_z, 2), float('nan'), device='cuda')
    rc = L.kgw_softmax_merge(parts.data_ptr(), n_ranks, seg.data_ptr(), n_seg, Z.data_ptr(), stat.data_ptr(), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return Z.cpu(), stat.cpu()


@pytest.mark.parametrize('n_seg', [1, 7, 8, 9, 16385, 2 * 16384 + 1037])
@pytest.mark.parametrize('n_ranks', [1, 2, 3, 8])
def test_softmax_merge_against_float64(n_ranks, n_seg):
    """8 segments per 256-thread block, 2048-block grid cap: 16 385 and 33 805 segments take the grid-stride loop more than once."""
    parts = _states(n_ranks, n_seg, 13 * n_ranks + n_seg)
    n_z = 2 * n_seg + 5
    seg = torch.randperm(n_z, generator=torch.Generator().manual_seed(n_seg))[:n_seg].int()
    Z, stat = _merge(parts.cuda(), seg.cuda(), n_z)
    Zr, sr = _merge_ref(parts)
    idx = seg.long()
    assert_close(Z[idx], Zr, RTOL, ATOL, 'merged Z')
    assert_close(stat[idx], sr, RTOL, ATOL, 'merged stat')
    none = ~(parts[..., 1] > 0).any(0)
    assert bool(none.any()) or n_seg < 3
    assert float(Z[idx][none].abs().sum()) == 0.0 and float(stat[idx][none].abs().sum()) == 0.0, 'no rank present: Z = 0, stat = (0, 0)'
    rest = torch.ones(n_z, dtype=torch.bool)
    rest[idx] = False
    assert bool(torch.isnan(Z[rest]).all()) and bool(torch.isnan(stat[rest]).all()), 'a row that is not listed was written'
    Z2, stat2 = _merge(parts.cuda(), seg.cuda(), n_z)
    assert torch.equal(Z2[idx], Z[idx]) and torch.equal(stat2[idx], stat[idx]), 'merging the same records twice: same bits'


@pytest.mark.parametrize('n_ranks', [2, 3, 8])
def test_merging_copies_of_one_state_is_its_own_normalisation(n_ranks):
    one = _states(1, 999, 4)
    seg = torch.arange(999, dtype=torch.int32)
    Z, stat = _merge(one.expand(n_ranks, -1, -1).contiguous().cuda(), seg.cuda(), 999)
    s, acc = one[0, :, 1].double(), one[0, :, 4:].double()
    present = s > 0
    assert_close(Z[present], (acc / (s[:, None] + 1e-16))[present], RTOL, ATOL, 'Z of P copies')
    assert_close(stat[present][:, 0], one[0, :, 0][present], RTOL, ATOL, 'm* of P copies')
    assert_close(stat[present][:, 1], n_ranks * s[present] + 1e-16, RTOL, ATOL, 'denominator of P copies')


@pytest.mark.parametrize('n_seg', [1, 9, 16385])
def test_pack_then_merge_of_one_rank(n_seg):
    """pack copies (m, s, acc) of exactly the listed rows (words 2 and 3 zero); merging that one record gives acc / (s + 1e-16)."""
    L, st = _lib_and_stream()
    g = torch.Generator().manual_seed(n_seg)
    n_z = 2 * n_seg + 3
    Z0 = torch.randn(n_z, W, generator=g) * 50
    stat0 = torch.stack([torch.randn(n_z, generator=g) * 5, 10.0 ** (torch.rand(n_z, generator=g) * 6)], 1)
    seg = torch.randperm(n_z, generator=g)[:n_seg].int()
    parts = torch.full((n_seg, PS), float('nan'), device='cuda')
    Zd, sd, segd = Z0.cuda(), stat0.cuda(), seg.cuda()
    assert L.kgw_softmax_pack(Zd.data_ptr(), sd.data_ptr(), segd.data_ptr(), n_seg, parts.data_ptr(), st) == 0
    torch.cuda.synchronize()
    idx = seg.long()
    pc = parts.cpu()
    assert torch.equal(pc[:, :2], stat0[idx]) and float(pc[:, 2:4].abs().sum()) == 0.0 and torch.equal(pc[:, 4:], Z0[idx])
    Z1, stat1 = _merge(parts.view(1, n_seg, PS), segd, n_z)
    den = stat0[idx][:, 1].double() + 1e-16
    assert_close(Z1[idx], Z0[idx].double() / den[:, None], RTOL, ATOL, 'pack -> merge Z')
    assert_close(stat1[idx], torch.stack([stat0[idx][:, 0].double(), den], 1), RTOL, ATOL, 'pack -> merge stat')
    rest = torch.ones(n_z, dtype=torch.bool)
    rest[idx] = False
    assert bool(torch.isnan(Z1[rest]).all()) and bool(torch.isnan(stat1[rest]).all())


SCATTER = [(w, n, off) for w in (128, 4, 20, 1, 3, 130) for n in (0, 1, 8191) for off in (0,)] + \
          [(128, 8191, 1), (128, 140000, 0), (130, 40000, 0), (3, 1500000, 0)]


@pytest.mark.parametrize('width,n_rows,offset', SCATTER, ids=[f'w{w}-n{n}-off{o}' for w, n, o in SCATTER])
def test_scatter_rows(width, n_rows, offset):
    """dst[ids[i]] = src[i]: widths on the float4 path (128, 4, 20) and on the scalar path (1, 3, 130; a 128-wide source 4 bytes
    off 16-byte alignment), row counts up to past the 16 384-block grid cap; rows that are not listed stay untouched."""
    L, st = _lib_and_stream()
    g = torch.Generator().manual_seed(width * 7 + n_rows)
    n_dst = 2 * n_rows + 3
    buf = torch.randn(n_rows * width + offset + 1, generator=g).cuda()
    src = buf[offset:offset + n_rows * width]
    assert (src.data_ptr() % 16 != 0) == bool(offset)
    ids = torch.randperm(n_dst, generator=g)[:n_rows].int()
    dst = torch.full((n_dst, width), float('nan'), device='cuda')
    idd = ids.cuda()
    assert L.kgw_scatter_rows(src.data_ptr(), idd.data_ptr(), n_rows, width, dst.data_ptr(), st) == 0
    torch.cuda.synchronize()
    want = torch.full((n_dst, width), float('nan'))
    want[ids.long()] = src.cpu().view(n_rows, width)
    got = dst.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))


@pytest.mark.parametrize('width', [128, 3])
def test_scatter_rows_inverts_gather_rows_on_a_permutation(width):
    L, st = _lib_and_stream()
    n = 5000
    g = torch.Generator().manual_seed(width)
    src = torch.randn(n, width, generator=g).cuda()
    ids = torch.randperm(n, generator=g).int().cuda()
    mid = torch.full((n, width), float('nan'), device='cuda')
    back = torch.full((n, width), float('nan'), device='cuda')
    assert L.kgw_gather_rows(src.data_ptr(), ids.data_ptr(), n, width, mid.data_ptr(), st) == 0
    assert L.kgw_scatter_rows(mid.data_ptr(), ids.data_ptr(), n, width, back.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(mid, src[ids.long()]) and torch.equal(back, src)


def test_argument_errors_launch_nothing():
    """NULL pointers, n_ranks = 0 and negative counts return KGW_E_NULL (-1) / KGW_E_RANGE (-2); the outputs stay as they were."""
    L, st = _lib_and_stream()
    n = 16
    Z = torch.full((n, W), float('nan'), device='cuda')
    stat = torch.full((n, 2), float('nan'), device='cuda')
    parts = torch.full((2, n, PS), float('nan'), device='cuda')
    seg = torch.arange(n, dtype=torch.int32, device='cuda')
    rows = torch.full((n, W), float('nan'), device='cuda')
    z, s_, p, sg, rw = (t.data_ptr() for t in (Z, stat, parts, seg, rows))
    E_NULL, E_RANGE = -1, -2
    assert L.kgw_softmax_pack(None, s_, sg, n, p, st) == E_NULL
    assert L.kgw_softmax_pack(z, None, sg, n, p, st) == E_NULL
    assert L.kgw_softmax_pack(z, s_, None, n, p, st) == E_NULL
    assert L.kgw_softmax_pack(z, s_, sg, n, None, st) == E_NULL
    assert L.kgw_softmax_pack(z, s_, sg, -1, p, st) == E_RANGE
    assert L.kgw_softmax_merge(None, 2, sg, n, z, s_, st) == E_NULL
    assert L.kgw_softmax_merge(p, 2, None, n, z, s_, st) == E_NULL
    assert L.kgw_softmax_merge(p, 2, sg, n, None, s_, st) == E_NULL
    assert L.kgw_softmax_merge(p, 2, sg, n, z, None, st) == E_NULL
    assert L.kgw_softmax_merge(p, 0, sg, n, z, s_, st) == E_RANGE
    assert L.kgw_softmax_merge(p, -3, sg, n, z, s_, st) == E_RANGE
    assert L.kgw_softmax_merge(p, 2, sg, -1, z, s_, st) == E_RANGE
    assert L.kgw_scatter_rows(None, sg, n, W, rw, st) == E_NULL
    assert L.kgw_scatter_rows(z, None, n, W, rw, st) == E_NULL
    assert L.kgw_scatter_rows(z, sg, n, W, None, st) == E_NULL
    assert L.kgw_scatter_rows(z, sg, n, 0, rw, st) == E_RANGE
    assert L.kgw_scatter_rows(z, sg, n, -4, rw, st) == E_RANGE
    assert L.kgw_scatter_rows(z, sg, -1, W, rw, st) == E_RANGE
    assert L.kgw_softmax_pack(None, None, None, 0, None, st) == 0 and L.kgw_softmax_merge(None, 2, None, 0, None, None, st) == 0
    assert L.kgw_scatter_rows(None, None, 0, W, None, st) == 0
    torch.cuda.synchronize()
    for t in (Z, stat, parts, rows):
        assert bool(torch.isnan(t).all())
