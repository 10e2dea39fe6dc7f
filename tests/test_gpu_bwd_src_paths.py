"""-m gpu: the src-major backward (k_agg_bwd_src: octet path, row-pair path, single-row path, riders) on ONE small graph whose
source rows sit on every bound of the three row paths at once, against the float64 oracle with the tolerances of
tests/test_gpu_aggregate.py.

Source rows of 0, 1, 2, 7, 8, 9 entries (the octet path takes rows of at most 8), 31, 32, 33 (the pair path's blocks of 32 per
half), 64, 65 (the single-row path's blocks of 64), 128, 129 (KGW_PAIR_MAX) and 300 entries; an octet of source-only SNP rows
that holds a 9-entry row (unflagged: its pairs go through the pair path); the seeds in front of the SNP block (rows with a
d a_dst term, octets the sampler never flags); 383 SNP rows, so that the Gene block starts at an odd row and a pair straddles
two types; and the same minibatch in the row blocks of a static layout, where the SNP block's last real row shares its pair with
a padding row and whole pairs are padding.  Layers 1 and 2, with and without the ReLU mask of the layer input.

Before anything is compared, every case counts on the host -- from t_ptr, the octet flags and the row counts, with the kernel's
own rule -- how many rows go down each path and how many octets are unflagged, and asserts that the paths named for the case
are not empty.

dH, d u_r / d v_r (from the riders' eight pieces, and, with the riders off, through the [d a_src | d a_dst] rows) and the
relation sums of a logit constant are compared; the same launch twice gives the same bits.  The float64 reference is
tests/test_gpu_aggregate.py's; with a logit constant, which that one does not take, tests/test_gpu_aggregate_parity.py's."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests.helpers import assert_close
from tests.test_gpu_aggregate import ATOL, RTOL, _oracle_layer
from tests.test_gpu_aggregate_parity import oracle_layer, realised_structure

pytestmark = pytest.mark.gpu

N_SEED = 320                                         # SNPs 0..319: the seeds; no out-edges (source rows of 0 entries)
# entries of the Gene rows (edges Gene -> seed SNP); consecutive rows share a pair.  The Gene block starts at an odd row in the
# minibatch's own layout -- (2,7) (8,9) (31,32) (33,64) (65,128) take the pair path, 1, (129,300) (64,200) (65,130) the single-row
# path -- and at an even one in the static layout: (1,2) .. (64,65) pair path, (128,129) (300,64) (200,65) single-row path
GENE_DEG = [1, 2, 7, 8, 9, 31, 32, 33, 64, 65, 128, 129, 300, 64, 200, 65, 130]
# entries of the source-only SNPs 320.. (edges SNP -> Gene): octets of short rows, two of them with a 9-entry row
SNP_DEG = [1, 2, 7, 8, 1, 2, 1, 1] + [1, 9, 1, 1, 2, 2, 1, 1] + [1, 2, 1, 3, 2, 1, 7, 8] * 2 + [2, 1, 1, 9, 1, 8, 1, 2] + \
          [1, 2, 1, 3, 2, 1, 7, 8] * 2 + [1, 2, 7, 1, 1, 2, 1]
N_SNP, N_GENE = N_SEED + len(SNP_DEG) + 5, len(GENE_DEG) + 2       # (a few nodes that no minibatch reaches)
REQUIRED = {0, 1, 2, 7, 8, 9, 31, 32, 33, 64, 65, 128, 129}
KGW_PAIR_MAX = 128


def make_graph():
    from kgwas_amd.graph import HeteroGraph
    assert len(SNP_DEG) == 63                        # 383 reachable SNPs: the Gene block starts at an odd row
    rng = np.random.default_rng(1138)
    g2s = np.concatenate([np.stack([np.full(d, k), rng.choice(N_SEED, size=d, replace=False)]) for k, d in enumerate(GENE_DEG)], axis=1)
    s2g = np.concatenate([np.stack([np.full(d, N_SEED + j), rng.choice(len(GENE_DEG), size=d, replace=False)])
                          for j, d in enumerate(SNP_DEG)], axis=1)
    g = torch.Generator().manual_seed(23)
    data = HeteroGraph()
    for t, k in OrderedDict([('SNP', N_SNP), ('Gene', N_GENE)]).items():
        data[t].x = torch.rand(k, 16, generator=g)
    data[('Gene', 'G2S', 'SNP')].edge_index = torch.from_numpy(np.ascontiguousarray(g2s.astype(np.int64)))
    data[('SNP', 'S2G', 'Gene')].edge_index = torch.from_numpy(np.ascontiguousarray(s2g.astype(np.int64)))
    data['SNP'].y = torch.rand(N_SNP, generator=g)
    return data


_STATE = {}


def _batch(kind):
    """The minibatch of all 320 seeds: 'loader' in the layout of its own counts, 'static' in the row blocks of a static layout
    whose capacities are above them (a captured step's)."""
    if kind not in _STATE:
        from kgwas_amd.sampler import BatchBuffers, NeighborLoader, finish_sample, sample_into
        if 'data' not in _STATE:
            _STATE['data'] = make_graph()
        data = _STATE['data']
        seeds = np.arange(N_SEED, dtype=np.int64)
        ld = NeighborLoader(data, [-1, -1], ('SNP', seeds), batch_size=N_SEED, device='cuda:0', prefetch=False)
        if kind == 'loader':
            _STATE[kind] = next(iter(ld))
        else:
            dgs = ld.dg.with_static_caps(ld.measure_caps())                      # (3 % margin, rounded up to 64)
            buf = BatchBuffers(dgs)
            sample_into(dgs, buf, ld.ids, ld.seed_type)
            _STATE[kind] = finish_sample(dgs, buf, 'SNP', N_SEED)
    return _STATE[kind]


def path_census(batch, layer):
    """Which path every source row of the layer takes, by the rule of k_agg_bwd_src, from what the sampler wrote: the entries of
    every row, the rows per path, the flagged and unflagged octets, and what the single-row path meets."""
    from kgwas_amd import ops
    dg, m = batch.dg, batch.meta
    sc = dg.schema
    l = layer - 1
    base = [int(m.src_base[l][t]) for t in range(sc.NT + 1)]
    n_rows_all = base[sc.NT]
    tp = batch.buf.t_ptr[l].cpu().numpy()
    ty_of, ent, real, is_dst = [], [], [], []
    for t in range(sc.NT):
        rs, tb, n_real, n_dst = int(sc.R_src[t]), int(m.t_base[l][t]), int(m.n_src[l][t]), int(m.n_rows[l][t])
        for j in range(base[t + 1] - base[t]):
            ty_of.append(t)
            real.append(j < n_real)
            is_dst.append(int(sc.R_dst[t]) > 0 and j < n_dst)
            ent.append(int(tp[tb + j * rs + rs] - tp[tb + j * rs]) if j < n_real else -1)
    t = 0
    while t < sc.NT and (dg.short_type_mask >> t) & 1:
        t += 1
    oct_rows = (base[t] & ~7) if ops._SHORT_ROWS else 0
    flags = batch.buf.t_cnt[l][:(n_rows_all + 7) // 8].cpu().numpy()
    c = dict(octet=0, pair=0, single=0, padding=0, flagged=0, unflagged=0, unflagged_by_length=0, cross_type=0, half_real=0,
             single_entries=set(), pair_entries=set(), octet_entries=set(), dst_rows_short=0, entries=set(e for e in ent if e >= 0))
    for o in range(oct_rows // 8):
        rows = range(8 * o, 8 * o + 8)
        if flags[o]:
            c['flagged'] += 1
            assert all(real[u] and not is_dst[u] and 0 <= ent[u] <= 8 for u in rows) and len({ty_of[u] for u in rows}) == 1, o
        else:
            c['unflagged'] += 1
            if all(real[u] and not is_dst[u] for u in rows) and max(ent[u] for u in rows) > 8:
                c['unflagged_by_length'] += 1
    for u in range(0, n_rows_all, 2):
        if u < oct_rows and flags[u >> 3]:
            c['octet'] += 2
            c['octet_entries'] |= {ent[u], ent[u + 1]}
            continue
        pair = u + 1 < n_rows_all and ty_of[u + 1] == ty_of[u] and real[u] and real[u + 1] and int(sc.R_src[ty_of[u]]) < 32 and \
            max(ent[u], ent[u + 1]) <= KGW_PAIR_MAX
        if pair:
            c['pair'] += 2
            c['pair_entries'] |= {ent[u], ent[u + 1]}
            continue
        if u + 1 < n_rows_all and ty_of[u + 1] != ty_of[u]:
            c['cross_type'] += 1
        if u + 1 < n_rows_all and real[u] != real[u + 1]:
            c['half_real'] += 1
        for v in (u, u + 1):
            if v < n_rows_all:
                c['single' if real[v] else 'padding'] += 1
                if real[v]:
                    c['single_entries'].add(ent[v])
    c['dst_rows_short'] = sum(1 for u in range(oct_rows) if is_dst[u])
    c['first_long_row'] = base[t]
    return c


# paths that a case must exercise (counted on the host before the launch)
NAMED = {
    ('loader', 1): ('octet', 'pair', 'single', 'unflagged', 'unflagged_by_length', 'dst_rows_short', 'cross_type'),
    ('loader', 2): ('pair', 'single', 'unflagged', 'dst_rows_short'),
    ('static', 1): ('octet', 'pair', 'single', 'unflagged', 'unflagged_by_length', 'dst_rows_short', 'padding', 'half_real'),
    ('static', 2): ('pair', 'single', 'unflagged', 'dst_rows_short', 'padding'),
}


def test_graph_realises_every_row_length_and_path():
    for kind in ('loader', 'static'):
        b = _batch(kind)
        for layer in (1, 2):
            c = path_census(b, layer)
            print(f'{kind} layer {layer}: ' + ', '.join(f'{k} {sorted(v) if isinstance(v, set) else v}' for k, v in c.items()))
            for name in NAMED[(kind, layer)]:
                assert c[name], (kind, layer, name)
    c = path_census(_batch('loader'), 1)
    assert REQUIRED <= c['entries'] and max(c['entries']) > 256, sorted(c['entries'])
    assert {0, 1, 2, 7, 8} <= c['octet_entries'] | c['pair_entries'] and 9 in c['pair_entries'], (c['octet_entries'], c['pair_entries'])
    assert {1, 2, 7, 8} <= c['octet_entries'], c['octet_entries']                   # the octet limit from below ...
    assert {31, 32, 33, 64, 65, 128} <= c['pair_entries'], c['pair_entries']        # ... the pair path's blocks of 32, KGW_PAIR_MAX
    assert {64, 65, 129} <= c['single_entries'] and max(c['single_entries']) > 256, c['single_entries']     # blocks of 64
    assert c['first_long_row'] % 2 == 1, c['first_long_row']                        # a pair of two types
    assert 1 in realised_structure(_batch('loader'), 1)['oct'] and 0 in realised_structure(_batch('loader'), 1)['oct']
    c = path_census(_batch('static'), 1)
    assert REQUIRED <= c['entries'] and c['padding'] >= 2 and c['half_real'] >= 1, c


def _inputs(batch, layer, relu_in, seed):
    m, sc = batch.meta, batch.dg.schema
    g = torch.Generator().manual_seed(seed)
    n_src = int(m.src_base[layer - 1][sc.NT])
    z_rows = int(m.z_base[layer - 1][sc.NT])
    assert n_src > 0 and z_rows > 0
    H = torch.randn(n_src, 128, generator=g)
    if relu_in:
        H = torch.relu(H)                             # a ReLU output: exact zeros, the backward's mask is (H > 0)
    V = torch.randn(sc.NR, 128, generator=g) * 0.2
    U = torch.randn(sc.NR, 128, generator=g) * 0.2
    kap = torch.randn(sc.NR, generator=g) * 0.5
    G = torch.randn(z_rows, 128, generator=g)
    return H, V, U, kap, G


def _gpu(batch, layer, H, V, U, kap, G, relu_in):
    from kgwas_amd import ops
    Hd, Vd, Ud = (t.cuda().requires_grad_(True) for t in (H, V, U))
    kd = kap.cuda().requires_grad_(True) if kap is not None else None
    Z, _, _ = ops.gat_aggregate(batch, layer, Hd, Ud, Vd, relu_input=relu_in, logit_bias=kd)
    (Z * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    return Z.detach(), Hd.grad, Ud.grad, Vd.grad, (kd.grad if kd is not None else None)


_REF = {}


def _reference(kind, layer, relu_in, lbias):
    """float64, once per (batch, layer, mask, constant): shared by the riders / da_src cases, never written to."""
    key = (kind, layer, relu_in, lbias)
    if key not in _REF:
        batch = _batch(kind)
        H, V, U, kap, G = _inputs(batch, layer, relu_in, 70 + layer)
        Ho, Vo, Uo = (t.double().requires_grad_(True) for t in (H, V, U))
        ko = kap.double().requires_grad_(True) if lbias else None
        Hin = torch.relu(Ho) if relu_in else Ho       # (H is a ReLU output already: relu(H) = H, its gradient carries the mask)
        Zo = oracle_layer(batch, layer, Hin, Uo, Vo, lbias=ko)[0] if lbias else _oracle_layer(batch, layer, Hin, Vo, Uo)
        (Zo * G.double()).sum().backward()
        dH = Ho.grad * (H > 0) if relu_in else Ho.grad
        _REF[key] = (Zo.detach(), dH, Uo.grad, Vo.grad, ko.grad if lbias else None)
    return _REF[key]


@pytest.mark.parametrize('kind,layer,relu_in,mode', [
    ('loader', 1, False, 'riders'), ('loader', 1, True, 'riders'), ('loader', 2, False, 'riders'), ('loader', 2, True, 'riders'),
    ('static', 1, False, 'riders'), ('static', 1, True, 'riders'), ('static', 2, False, 'riders'), ('static', 2, True, 'riders'),
    ('loader', 1, True, 'da_src'), ('static', 1, False, 'da_src'), ('static', 2, True, 'da_src'),
    ('loader', 1, True, 'rel_sums'), ('static', 1, False, 'rel_sums'), ('loader', 2, False, 'rel_sums'),
])
def test_bwd_src_matches_float64(monkeypatch, kind, layer, relu_in, mode):
    from kgwas_amd import ops
    batch = _batch(kind)
    dg = batch.dg
    sc = dg.schema
    census = path_census(batch, layer)
    for name in NAMED[(kind, layer)]:                  # a path may not silently drop out of the case
        assert census[name], (kind, layer, name, census)
    if mode == 'da_src':
        monkeypatch.setattr(ops, '_DUV_RIDERS', False)   # d u_r / d v_r through the [d a_src | d a_dst] row of every node
    lbias = mode == 'rel_sums'
    H, V, U, kap, G = _inputs(batch, layer, relu_in, 70 + layer)
    got = _gpu(batch, layer, H, V, U, kap if lbias else None, G, relu_in)
    ref = _reference(kind, layer, relu_in, lbias)
    live = [r for r in range(sc.NR) if dg.kg.rel_live[layer - 1][r]]
    dead = [r for r in range(sc.NR) if not dg.kg.rel_live[layer - 1][r]]
    assert live
    for name, a, b in (('Z', got[0], ref[0]), ('dH', got[1], ref[1]), ('dU', got[2][live], ref[2][live]),
                       ('dV', got[3][live], ref[3][live])) + ((('rel_sums', got[4][live], ref[4][live]),) if lbias else ()):
        err = (a.detach().double().cpu() - b).abs()
        print(f'{kind} layer {layer} relu_in {relu_in} {mode}: {name} max abs err {float(err.max()):.3e}, max |ref| {float(b.abs().max()):.3e}')
    assert_close(got[0], ref[0], RTOL, ATOL, 'Z')
    assert_close(got[1], ref[1], RTOL, ATOL, 'dH')
    assert_close(got[2][live], ref[2][live], RTOL, ATOL, 'dU')
    assert_close(got[3][live], ref[3][live], RTOL, ATOL, 'dV')
    assert float(got[2][dead].abs().sum()) == 0.0 and float(got[3][dead].abs().sum()) == 0.0
    if lbias:
        assert_close(got[4][live], ref[4][live], RTOL, ATOL, 'rel_sums')
        assert float(got[4][dead].abs().sum()) == 0.0
    if relu_in:
        assert bool((H == 0).any()) and float(got[1].cpu()[H == 0].abs().max()) == 0.0
    # the same launch again: no atomics anywhere, the same bits
    again = _gpu(batch, layer, H, V, U, kap if lbias else None, G, relu_in)
    for a, b in zip(got[1:], again[1:]):
        assert (a is None and b is None) or torch.equal(a, b)
