"""-m gpu: the attention-aggregate kernels of kgw_aggregate.hip (k_agg_fwd / _combine, k_agg_bwd_dst / _combine, k_agg_bwd_src
with its rider blocks, k_duv_fold, k_edge_alpha) against a float64 restatement, output by output, at the degrees the kernels
branch on and with every option of gat_aggregate switched on and off.

What is compared, per case: Z, the per-row softmax statistics (row max of e / T, denominator S + 1e-16), the per-edge logit e and
alpha, and the gradients dH, dU, dV and d logit_bias.  Dead relations must get exactly zero gradients, Z rows without edges
exactly zero, and alpha must sum to one over every non-empty segment.

The degree ladder (make_degree_ladder_graph) pins the in-degrees around the kernels' bounds: 64-edge blocks, the two half-waves'
groups of 8 with tails of 4 and 2 (hn = (nb + 1) / 2 edges per half), KGW_CHUNK = 128-edge chunks and segments of 2, 3 and
more than 4 chunks; test_degree_ladder_realises_every_branch reads the realised structure back from the sampled batch.

Tolerances as tests/test_gpu_aggregate.py (rtol 1e-4, atol 1e-5, assert_close's rel_to_max).  Quantities that hang on d a_dst
alone are cancellation residues wherever a row's logits sit on one branch of the leaky ReLU (exact value 0): where they miss
the element-wise bound they must be within 2 x the error of the same oracle run in float32 (tests/test_gpu_hub.py)."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle.pyg_semantics import segment_softmax
from tests.helpers import assert_close, segment_alpha_sums

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
C = 128

# in-degrees of the first genes on relation ('SNP', 'LAD', 'Gene'): both sides of 8, 16, 32, 64, 128, 256, 384 (the 64-edge
# blocks and the half-waves' groups) and one row of 1000 edges (8 chunks)
LADDER = [0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 385, 1000]
N_SNP, N_GENE = 3000, 256
HUB_SNP = 0              # TSS edge to every gene: 256 in-edges on ('Gene', 'rev_TSS', 'SNP'), a segment of two chunks
HEAVY_SNPS = 40          # SNPs 1..40: 12 extra LAD edges each, source rows with more than 8 entries (octet flag 0)


def make_degree_ladder_graph():
    """SNP / Gene graph whose destination rows hit the chunk and half-wave bounds of the aggregate kernels (LADDER) and whose
    SNP source rows have 1 to ~20 out-edges; a second SNP -> Gene relation (its mirror is slot 1 of the SNP destination rows), a
    Gene -> Gene relation with self-loops, and a SNP hub row of 256 in-edges on the reverse of the second relation."""
    from kgwas_amd.graph import HeteroGraph, add_self_loops, to_undirected
    rng = np.random.default_rng(2024)
    n = OrderedDict([('SNP', N_SNP), ('Gene', N_GENE)])
    src, dst = [], []
    for g, d in enumerate(LADDER):
        src.append(rng.choice(np.arange(1, N_SNP), size=d, replace=False))
        dst.append(np.full(d, g))
    for g in range(len(LADDER), N_GENE):                 # filler genes: 0 .. 23 in-edges
        d = int(rng.integers(0, 24))
        src.append(rng.choice(np.arange(1, N_SNP), size=d, replace=False))
        dst.append(np.full(d, g))
    for s in range(1, HEAVY_SNPS + 1):
        src.append(np.full(12, s))
        dst.append(rng.choice(np.arange(len(LADDER), N_GENE), size=12, replace=False))
    lad = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    tss_d = rng.integers(0, 15, N_GENE)                   # plus the hub's edge: 1 .. 15 in-edges per gene
    tss = np.concatenate([np.stack([np.full(N_GENE, HUB_SNP), np.arange(N_GENE)]),
                          np.stack([rng.integers(1, N_SNP, int(tss_d.sum())), np.repeat(np.arange(N_GENE), tss_d)])],
                         axis=1).astype(np.int64)
    g2g = np.stack([rng.integers(0, N_GENE, 40), rng.integers(0, N_GENE, 40)]).astype(np.int64)
    e = OrderedDict([(('SNP', 'LAD', 'Gene'), lad), (('SNP', 'TSS', 'Gene'), tss), (('Gene', 'G2G', 'Gene'), g2g)])
    g = torch.Generator().manual_seed(5)
    data = HeteroGraph()
    for t, k in n.items():
        data[t].x = torch.rand(k, 16, generator=g)
    und = add_self_loops(to_undirected(e, n), n)
    for et, ei in und.items():
        data[et].edge_index = torch.from_numpy(np.ascontiguousarray(ei))
    data['SNP'].y = torch.rand(N_SNP, generator=g)
    return data


@pytest.fixture(scope='module')
def ladder():
    return make_degree_ladder_graph()


def _minibatch(data, seeds):
    from kgwas_amd.sampler import NeighborLoader
    seeds = np.asarray(seeds, dtype=np.int64)
    return next(iter(NeighborLoader(data, [-1, -1], ('SNP', seeds), batch_size=len(seeds), device='cuda:0')))


def _ladder_seeds():
    rng = np.random.default_rng(11)
    return np.concatenate([[HUB_SNP, 1], rng.choice(np.arange(HEAVY_SNPS + 1, N_SNP), size=46, replace=False)])


_BATCHES = {}


@pytest.fixture
def batches(ladder, small_kg, edge_case_graph):
    from kgwas_amd.sampler import sample_full_graph

    def get(name):
        if name not in _BATCHES:
            if name == 'ladder_full':
                _BATCHES[name] = sample_full_graph(ladder, 2, 'cuda:0')
            elif name == 'ladder_mini':
                _BATCHES[name] = _minibatch(ladder, _ladder_seeds())
            elif name == 'small_mini':
                ids = np.random.default_rng(0).choice(small_kg.data['SNP'].x.shape[0], size=48, replace=False)
                _BATCHES[name] = _minibatch(small_kg.data, ids)
            else:
                _BATCHES[name] = sample_full_graph(edge_case_graph[0], 2, 'cuda:0')
        return _BATCHES[name]
    return get


def _seeds_only(batch, layer):
    """The expression ops._layer_args decides by whether a layer may skip the combine launches."""
    dg = batch.dg
    n_multi_hops = min(dg.num_layers - layer, dg.n_hops - 1) + 1
    return (not dg.full_graph) and n_multi_hops == 1 and batch.input_type is not None and \
        dg.schema.type_id[batch.input_type] not in dg.multi_dst_types


# ------------------------------------------------------------------------------------------------------------------------------
# the float64 oracle
# ------------------------------------------------------------------------------------------------------------------------------
def layer_edges(batch, layer):
    """{relation id: (local edge ids, local source ids, destination rows)} of the layer's live relations, in the kernels' local
    edge order: the segments of every destination hop the layer aggregates, relation by relation (meta.seg_off, buf.seg_ptr,
    buf.col_local -- as tests/test_gpu_golden.py maps the attention export)."""
    dg, m = batch.dg, batch.meta
    sc = dg.schema
    n_hops = min(dg.num_layers - layer, dg.n_hops - 1) + 1
    seg_ptr = batch.buf.seg_ptr[:int(m.seg_end[dg.n_hops - 1]) + 1].cpu().long()
    col = batch.buf.col_local[:max(int(m.edge_end[dg.n_hops - 1]), 1)].cpu().long()
    out, total = {}, 0
    for r in range(sc.NR):
        d = int(sc.dst_type[r])
        es, ds = [], []
        for h in range(n_hops):
            a, b = int(m.seg_off[h][r]), int(m.seg_off[h][r + 1])
            if b <= a:
                continue
            deg = seg_ptr[a + 1:b + 1] - seg_ptr[a:b]
            es.append(torch.arange(int(seg_ptr[a]), int(seg_ptr[b])))
            ds.append(torch.repeat_interleave(torch.arange(b - a) + int(m.node_off[d][h]), deg))
            total += int(seg_ptr[b] - seg_ptr[a])
        e = torch.cat(es) if es else torch.zeros(0, dtype=torch.long)
        if not dg.kg.rel_live[layer - 1][r] or not e.numel():
            continue
        out[r] = (e, col[e], torch.cat(ds))
    assert total == int(m.n_edges[layer - 1]), (total, int(m.n_edges[layer - 1]))
    return out


def oracle_layer(batch, layer, H, U, V, slope=0.2, temp=1.0, lbias=None, raw=False, edges=None):
    """Z[zrow(i, r)] = sum_j w_ij H_src[j] with pre_ij = <H_src[j], u_r> + <H_dst[i], v_r> + kappa_r, e_ij = leaky_relu(pre_ij,
    slope), w = softmax_i(e / T) (PyG: max-subtracted, denominator + 1e-16) or, raw, w = e.  Also the per-row statistics as
    the kernels store them (max of e / T, denominator; raw: (0, 1)) and e / alpha per local edge.  Differentiable in H, U, V,
    lbias (their dtype)."""
    dg, m = batch.dg, batch.meta
    sc = dg.schema
    edges = layer_edges(batch, layer) if edges is None else edges
    dt = H.dtype
    z_rows = int(m.z_base[layer - 1][sc.NT])
    n_edges = int(m.n_edges[layer - 1])
    Z = torch.zeros(z_rows, C, dtype=dt)
    stat = torch.zeros(z_rows, 2, dtype=dt)
    e_all = torch.zeros(n_edges, dtype=dt)
    alpha_all = torch.zeros(n_edges, dtype=dt)
    for r, (eid, src, dst) in edges.items():
        s, d = int(sc.src_type[r]), int(sc.dst_type[r])
        nr = int(m.n_rows[layer - 1][d])
        assert int(dst.max()) < nr
        Hs = H[int(m.src_base[layer - 1][s]):int(m.src_base[layer - 1][s]) + int(m.n_src[layer - 1][s])]
        Hd = H[int(m.src_base[layer - 1][d]):int(m.src_base[layer - 1][d]) + nr]
        pre = (Hs @ U[r])[src] + (Hd @ V[r])[dst]
        if lbias is not None:
            pre = pre + lbias[r]
        e = torch.nn.functional.leaky_relu(pre, slope)
        zrow = int(m.z_base[layer - 1][d]) + dst * int(sc.R_dst[d]) + int(sc.slot_dst[r])
        with torch.no_grad():
            e_all[eid] = e.detach()
            if raw:
                stat[zrow] = torch.tensor([0.0, 1.0], dtype=dt)
            else:
                t = (e / temp).detach()
                mx = torch.full((nr,), float('-inf'), dtype=dt).scatter_reduce(0, dst, t, reduce='amax')
                den = torch.zeros(nr, dtype=dt).index_add(0, dst, (t - mx[dst]).exp()) + 1e-16
                has = torch.zeros(nr, dtype=torch.bool)
                has[dst] = True
                rows = torch.nonzero(has).squeeze(1)
                stat[int(m.z_base[layer - 1][d]) + rows * int(sc.R_dst[d]) + int(sc.slot_dst[r])] = \
                    torch.stack([mx[rows], den[rows]], 1)
        w = e if raw else segment_softmax(e / temp, dst, nr)
        if not raw:
            alpha_all[eid] = w.detach()
        Z = Z.index_add(0, zrow, w.unsqueeze(-1) * Hs[src])
    return Z, stat, e_all, alpha_all


# ------------------------------------------------------------------------------------------------------------------------------
# one case: kernels and oracle on the same inputs
# ------------------------------------------------------------------------------------------------------------------------------
def _inputs(batch, layer, seed, relu_input=False, lbias=False, u_scale=0.2, v_scale=0.2):
    m, sc = batch.meta, batch.dg.schema
    g = torch.Generator().manual_seed(seed)
    n_src = int(m.src_base[layer - 1][sc.NT])
    z_rows = int(m.z_base[layer - 1][sc.NT])
    H = torch.randn(n_src, C, generator=g)
    if relu_input:
        H = torch.relu(H)                    # a ReLU output: exact zeros, the mask of the backward is (H > 0)
    U = torch.randn(sc.NR, C, generator=g) * u_scale
    V = torch.randn(sc.NR, C, generator=g) * v_scale
    kap = torch.randn(sc.NR, generator=g) * 0.5 if lbias else None
    G = torch.randn(z_rows, C, generator=g)
    return H, U, V, kap, G


def _run_gpu(batch, layer, H, U, V, kap, G, slope=0.2, temp=1.0, relu_input=False):
    from kgwas_amd import ops
    m, sc = batch.meta, batch.dg.schema
    z_rows = int(m.z_base[layer - 1][sc.NT])
    n_edges = int(m.n_edges[layer - 1])
    Hd, Ud, Vd = (t.cuda().requires_grad_(True) for t in (H, U, V))
    kd = kap.cuda().requires_grad_(True) if kap is not None else None
    Z, stat, e_edge = ops.gat_aggregate(batch, layer, Hd, Ud, Vd, neg_slope=slope, temperature=temp, relu_input=relu_input,
                                        logit_bias=kd)
    alpha = ops.edge_alpha(batch, layer, stat, e_edge, temperature=temp)
    (Z * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    return dict(Z=Z.detach().cpu(), stat=stat[:z_rows].cpu(), e=e_edge[:n_edges].cpu(), alpha=alpha.cpu(),
                dH=Hd.grad.cpu(), dU=Ud.grad.cpu(), dV=Vd.grad.cpu(), dlb=kd.grad.cpu() if kd is not None else None)


def _run_oracle(batch, layer, H, U, V, kap, G, dtype, slope=0.2, temp=1.0, relu_input=False, edges=None):
    Ho, Uo, Vo = (t.to(dtype).requires_grad_(True) for t in (H, U, V))
    ko = kap.to(dtype).requires_grad_(True) if kap is not None else None
    Z, stat, e, alpha = oracle_layer(batch, layer, Ho, Uo, Vo, slope, temp, ko, edges=edges)
    (Z * G.to(dtype)).sum().backward()
    dH = Ho.grad * (H > 0) if relu_input else Ho.grad
    return dict(Z=Z.detach(), stat=stat, e=e, alpha=alpha, dH=dH, dU=Uo.grad, dV=Vo.grad,
                dlb=ko.grad if ko is not None else None)


def _check_residue(name, got, ref, lazy32, atol):
    """Element-wise bound, or -- a gradient that hangs on d a_dst, a cancellation residue wherever a row's logits sit on one
    branch of the leaky ReLU -- norm-wise within 2 x the error of the float32 oracle."""
    try:
        assert_close(got, ref, RTOL, atol, name)
    except AssertionError:
        r32 = lazy32()[name]
        e = float((got.double() - ref).norm())
        e32 = float((r32.double() - ref).norm())
        print(f'{name}: beyond the element-wise bound; norm error {e:.3e} vs float32 oracle {e32:.3e}')
        assert e <= 2.0 * e32, (name, e, e32)


def check_case(batch, layer, seed, slope=0.2, temp=1.0, relu_input=False, lbias=False, u_scale=0.2, v_scale=0.2, spike=None):
    sc = batch.dg.schema
    dg = batch.dg
    H, U, V, kap, G = _inputs(batch, layer, seed, relu_input, lbias, u_scale, v_scale)
    if spike is not None:          # (H row, relation r): its logit on r becomes 3 |u_r|^2, ~35 x a typical one
        j, r = spike
        H[j] = 3.0 * U[r]
    edges = layer_edges(batch, layer)
    got = _run_gpu(batch, layer, H, U, V, kap, G, slope, temp, relu_input)
    ref = _run_oracle(batch, layer, H, U, V, kap, G, torch.float64, slope, temp, relu_input, edges)
    cache = {}

    def lazy32():
        if not cache:
            cache.update(_run_oracle(batch, layer, H, U, V, kap, G, torch.float32, slope, temp, relu_input, edges))
        return cache

    live = [r for r in range(sc.NR) if dg.kg.rel_live[layer - 1][r]]
    dead = [r for r in range(sc.NR) if not dg.kg.rel_live[layer - 1][r]]
    eid = torch.cat([edges[r][0] for r in edges]) if edges else torch.zeros(0, dtype=torch.long)
    assert eid.numel() > 0
    assert_close(got['Z'], ref['Z'], RTOL, ATOL, 'Z')
    assert_close(got['stat'], ref['stat'], RTOL, ATOL, 'stat (row max, denominator)')
    assert_close(got['e'][eid], ref['e'][eid], RTOL, ATOL, 'e_edge')
    assert_close(got['alpha'][eid], ref['alpha'][eid], RTOL, ATOL, 'alpha')
    # rows without an edge (degree 0, dead relations) are never written: exactly zero
    empty = torch.ones(got['Z'].shape[0], dtype=torch.bool)
    for r, (_, _, dst) in edges.items():
        d = int(sc.dst_type[r])
        empty[int(batch.meta.z_base[layer - 1][d]) + dst * int(sc.R_dst[d]) + int(sc.slot_dst[r])] = False
    assert float(got['Z'][empty].abs().sum()) == 0.0 and float(got['stat'][empty].abs().sum()) == 0.0
    sums = segment_alpha_sums(batch, layer, got['alpha'])
    assert sums.numel() > 0 and float((sums - 1.0).abs().max()) <= 1e-5, float((sums - 1.0).abs().max())
    if relu_input:
        assert bool((H == 0).any()) and float(got['dH'][H == 0].abs().max()) == 0.0
    assert_close(got['dU'][live], ref['dU'][live], RTOL, 1e-4, 'dU')
    _check_residue('dH', got['dH'], ref['dH'], lazy32, 2e-5)
    _check_residue('dV', got['dV'][live], ref['dV'][live], lambda: {'dV': lazy32()['dV'][live]}, 1e-4)
    assert float(got['dU'][dead].abs().sum()) == 0.0 and float(got['dV'][dead].abs().sum()) == 0.0
    if lbias:
        _check_residue('dlb', got['dlb'][live], ref['dlb'][live], lambda: {'dlb': lazy32()['dlb'][live]}, 1e-4)
        assert float(got['dlb'][dead].abs().sum()) == 0.0
    return got, ref


# ------------------------------------------------------------------------------------------------------------------------------
# the realised structure of the ladder
# ------------------------------------------------------------------------------------------------------------------------------
def realised_structure(batch, layer):
    """Chunk lengths, chunks per segment, half-wave sizes hn of every 64-edge block and octet flags of the layer, as the
    sampler laid them out (live relations: what the kernels visit)."""
    m = batch.meta
    live = batch.dg.kg.rel_live[layer - 1]
    nc = int(m.n_chunks[layer - 1])
    ch = batch.buf.chunks[:nc * 8].view(-1, 8).cpu().numpy()
    keep = np.array([bool(live[r]) for r in ch[:, 3]], dtype=bool)
    ch, idx = ch[keep], np.arange(nc)[keep]
    n = ch[:, 1] - ch[:, 0]
    hn = set()
    for k in set(n.tolist()):
        for b in range(0, k, 64):
            hn.add(((min(64, k - b) + 1) // 2) % 8)
    seg_len = np.bincount(ch[:, 4], weights=n, minlength=nc)          # edges per segment, at its first chunk
    heads = ch[ch[:, 4] == idx]
    seg_nch = heads[:, 5]
    seg_len = seg_len[heads[:, 4]]
    n_src = int(m.src_base[layer - 1][batch.dg.schema.NT])
    flags = batch.buf.t_cnt[layer - 1][:(n_src + 7) // 8].cpu().numpy()
    return dict(len_mod64=set((n % 64).tolist()), hn_mod8=hn, nch=set(seg_nch.tolist()),
                single_128=bool(((seg_nch == 1) & (seg_len == 128)).any()), oct=set(flags.tolist()),
                chunk_lens=sorted(set(n.tolist())), max_nch=int(seg_nch.max()))


def test_degree_ladder_realises_every_branch(ladder, batches):
    lad = ladder[('SNP', 'LAD', 'Gene')].edge_index
    deg = torch.bincount(lad[1], minlength=N_GENE)[:len(LADDER)].tolist()
    assert deg == LADDER
    for name in ('ladder_full', 'ladder_mini'):
        b = batches(name)
        sc = b.dg.schema
        snp = sc.type_id['SNP']
        assert snp in b.dg.multi_dst_types and b.dg.short_type_mask & (1 << snp)
        assert int(sc.R_dst[snp]) == 2 and int(sc.slot_dst[sc.edge_types.index(('Gene', 'rev_TSS', 'SNP'))]) == 1
        s = realised_structure(b, 1)
        print(f'{name} layer 1: chunk lengths {s["chunk_lens"]}, chunks per segment {sorted(s["nch"])}, '
              f'hn mod 8 {sorted(s["hn_mod8"])}, octet flags {sorted(s["oct"])}')
        assert {0, 1, 63} <= s['len_mod64'], s['len_mod64']
        assert s['hn_mod8'] == set(range(8)), s['hn_mod8']
        assert s['single_128']
        assert {1, 2, 3} <= s['nch'] and s['max_nch'] > 4, s['nch']
    assert realised_structure(batches('ladder_mini'), 1)['oct'] == {0, 1}
    # the top layer of the minibatch: the hub SNP is a seed, its 256-edge row needs the combine launches
    mb = batches('ladder_mini')
    assert not _seeds_only(mb, 2) and int(mb.meta.multi_cnt[0]) > 0 and realised_structure(mb, 2)['max_nch'] >= 2


# ------------------------------------------------------------------------------------------------------------------------------
# the parity matrix
# ------------------------------------------------------------------------------------------------------------------------------
GRAPHS = [('ladder_full', 1), ('ladder_full', 2), ('ladder_mini', 1), ('ladder_mini', 2), ('small_mini', 2), ('edge_full', 1)]
# (relu_input, logit_bias, no riders, no short-row path): a pairwise cover of the four switches plus the all-non-default case
OPTIONS = [(0, 0, 0, 0), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 1)]


@pytest.mark.parametrize('opts', OPTIONS, ids=lambda o: 'relu{}-lb{}-noriders{}-noshort{}'.format(*o))
@pytest.mark.parametrize('graph,layer', GRAPHS, ids=[f'{g}-L{l}' for g, l in GRAPHS])
def test_parity_matrix(batches, monkeypatch, graph, layer, opts):
    from kgwas_amd import ops
    relu_input, lbias, no_riders, no_short = map(bool, opts)
    monkeypatch.setattr(ops, '_DUV_RIDERS', not no_riders)
    monkeypatch.setattr(ops, '_SHORT_ROWS', not no_short)
    batch = batches(graph)
    if graph == 'small_mini':
        assert _seeds_only(batch, layer), 'this case covers the top layer without combine launches'
    if graph == 'ladder_mini' and layer == 2:
        assert not _seeds_only(batch, layer)
    check_case(batch, layer, seed=100 * layer + sum(o << i for i, o in enumerate(opts)), relu_input=relu_input, lbias=lbias)


# ------------------------------------------------------------------------------------------------------------------------------
# focused cases
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graph', ['ladder_full', 'ladder_mini'])
def test_raw_weights(batches, graph):
    """Attention export: Z = sum e_ij H_j, no softmax (stat (0, 1)); the backward refuses."""
    from kgwas_amd import ops
    batch = batches(graph)
    layer = 1
    H, U, V, kap, _ = _inputs(batch, layer, seed=7, lbias=True)
    edges = layer_edges(batch, layer)
    Hd = H.cuda().requires_grad_(True)
    Z, stat, e = ops.gat_aggregate(batch, layer, Hd, U.cuda(), V.cuda(), raw_weights=True, logit_bias=kap.cuda())
    Zo, so, eo, _ = oracle_layer(batch, layer, H.double(), U.double(), V.double(), lbias=kap.double(), raw=True, edges=edges)
    eid = torch.cat([edges[r][0] for r in edges])
    z_rows = Zo.shape[0]
    assert_close(Z, Zo, RTOL, ATOL, 'Z (raw)')
    assert_close(e[eid.cuda()], eo[eid], RTOL, ATOL, 'e_edge (raw)')
    assert torch.equal(stat[:z_rows].cpu().double(), so), 'stat (raw): (0, 1) on rows with edges, zero elsewhere'
    with pytest.raises(RuntimeError):
        Z.sum().backward()


@pytest.mark.parametrize('slope', [0.05, 0.5])
@pytest.mark.parametrize('temp', [0.5, 2.5])
def test_backward_at_other_slopes_and_temperatures(batches, slope, temp):
    check_case(batches('ladder_full'), 1, seed=31, slope=slope, temp=temp, lbias=True)


def _hub_edge(batch, layer, chunk=4, offset=70):
    """(local edge, H row of its source, relation) of edge ``offset`` of chunk ``chunk`` of the 1000-edge LAD row: a later
    chunk, and its second 64-edge block."""
    sc = batch.dg.schema
    r = sc.edge_types.index(('SNP', 'LAD', 'Gene'))
    eid, src, dst = layer_edges(batch, layer)[r]
    deg = torch.bincount(dst)
    assert int(deg.max()) == 1000
    e = int(eid[dst == int(deg.argmax())][128 * chunk + offset])
    j = int(batch.buf.col_local[e])
    return e, int(batch.meta.src_base[layer - 1][sc.type_id['SNP']]) + j, r


@pytest.mark.parametrize('graph', ['ladder_full', 'ladder_mini'])
def test_spike_in_a_late_chunk_of_the_hub_row(batches, graph):
    """One source of the 1000-edge row gets a logit ~35 x the others' in its fifth chunk: the chunk's online softmax rescales
    mid-chunk and the combine rescales every other chunk's partial state by less than exp(-300); forward and backward."""
    batch = batches(graph)
    e, j, r = _hub_edge(batch, 1)
    got, ref = check_case(batch, 1, seed=9, u_scale=1.0, v_scale=0.1, spike=(j, r), lbias=True)
    assert float(ref['alpha'][e]) > 0.99 and float(got['alpha'][e]) > 0.99


def test_deterministic(batches):
    """No atomics: two runs of forward and backward give the same bits."""
    batch = batches('ladder_mini')
    H, U, V, kap, G = _inputs(batch, 1, seed=3, lbias=True)
    a = _run_gpu(batch, 1, H, U, V, kap, G)
    b = _run_gpu(batch, 1, H, U, V, kap, G)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_duv_pieces_add_up_to_du_dv(batches):
    """KGW_F_DUV_PIECES (inside ops.duv_pieces_scope): dU / dV are left as eight pieces per relation for their consumer to add;
    the pieces' sum is the oracle's dU / dV."""
    from kgwas_amd import ops
    batch = batches('ladder_full')
    layer = 1
    sc = batch.dg.schema
    H, U, V, kap, G = _inputs(batch, layer, seed=17)
    ref = _run_oracle(batch, layer, H, U, V, kap, G, torch.float64)
    Hd, Ud, Vd = (t.cuda().requires_grad_(True) for t in (H, U, V))
    table = {}
    with ops.duv_pieces_scope(table):
        Z, _, _ = ops.gat_aggregate(batch, layer, Hd, Ud, Vd)
        (Z * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert len(table) == 2
    ws = next(iter(table.values()))[1]
    pieces = ws[:2 * sc.NR * 8 * C].view(2, sc.NR, 8, C).sum(2).cpu()
    live = [r for r in range(sc.NR) if batch.dg.kg.rel_live[layer - 1][r]]
    assert_close(pieces[0][live], ref['dU'][live], RTOL, 1e-4, 'dU from pieces')
    assert_close(pieces[1][live], ref['dV'][live], RTOL, 1e-4, 'dV from pieces')
    assert_close(Hd.grad, ref['dH'], RTOL, 2e-5, 'dH')
