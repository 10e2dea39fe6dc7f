"""CPU: attention with H heads (gat_num_head = H).  (1) The re-associated form the kernels compute (tests/multihead_ref.py: per-head
vectors u^h / v^h, per-head softmax over the layer input, block transform) IS PyG's GATConv((-1,-1), cl / H, heads=H, concat=True)
-- oracle/gat_oracle.py:GATConvOracle -- output and every gradient, in float64 to 1e-10 relative; (2) at H = 1 it is the
single-head oracle; (3) the product's constructor, state-dict shapes, load_state_dict round trip, the glorot bound of att_* and
every refusal that needs no device."""
import math
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle.gat_oracle import GATConvOracle
from tests import multihead_ref as R

REL_TOL = 1e-10


def make_graph():
    """3 node types, 6 relations, a few dozen nodes: a bipartite relation (A -> B) and its mirror (B -> A), a second bipartite pair
    (B -> C, C -> B), a same-type relation with self-loops (B -> B) and one without (A -> A; 40 edges, so that its
    rows' logits sit on both branches of the leaky ReLU and d att_dst is not a pure cancellation residue).  B node 0 and A node 1 have no
    in-edge on any relation (zero-degree rows); B node 1 has 9 in-edges on A -> B."""
    rng = np.random.default_rng(12)
    n = OrderedDict([('A', 14), ('B', 9), ('C', 5)])
    ab = np.concatenate([np.stack([rng.integers(0, 14, 20), rng.integers(2, 9, 20)]), np.stack([np.arange(9), np.ones(9, dtype=np.int64)])], 1)
    ab = ab[:, ab[0] != 1]                                   # (A node 1 sends nothing, so its mirror row is empty)
    bc = np.stack([rng.integers(1, 9, 12), rng.integers(0, 5, 12)])
    bb = np.stack([np.concatenate([rng.integers(1, 9, 8), np.arange(1, 9)]), np.concatenate([rng.integers(1, 9, 8), np.arange(1, 9)])])
    aa = np.stack([rng.integers(0, 14, 40), rng.integers(2, 14, 40)])
    e = OrderedDict([(('A', 'ab', 'B'), ab), (('B', 'rev_ab', 'A'), ab[::-1].copy()), (('B', 'bc', 'C'), bc),
                     (('C', 'rev_bc', 'B'), bc[::-1].copy()), (('B', 'bb', 'B'), bb), (('A', 'aa', 'A'), aa)])
    e = OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v)).long()) for k, v in e.items())
    deg_b = sum(torch.bincount(ei[1], minlength=9) for et, ei in e.items() if et[2] == 'B')
    deg_a = sum(torch.bincount(ei[1], minlength=14) for et, ei in e.items() if et[2] == 'A')
    assert int(deg_b[0]) == 0 and int(deg_a[1]) == 0 and int((bb[0] == bb[1]).sum()) >= 8
    return n, e


def _conv_and_inputs(et, n, cl, H, seed):
    g = torch.Generator().manual_seed(seed)
    s, _, d = et
    conv = GATConvOracle(cl, None if s == d else cl, cl // H, heads=H, dtype=torch.float64, gen=g)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(cl, generator=g, dtype=torch.float64) * 0.1)
    xs = torch.randn(n[s], cl, generator=g, dtype=torch.float64)
    xd = None if s == d else torch.randn(n[d], cl, generator=g, dtype=torch.float64)
    G = torch.randn(n[d], cl, generator=g, dtype=torch.float64)
    return conv, xs, xd, G


def _both(et, ei, n, cl, H, seed):
    conv, xs, xd, G = _conv_and_inputs(et, n, cl, H, seed)
    # the oracle
    xs_o = xs.clone().requires_grad_(True)
    xd_o = None if xd is None else xd.clone().requires_grad_(True)
    out_o = conv(xs_o if xd is None else (xs_o, xd_o), ei)
    (out_o * G).sum().backward()
    ref = {'out': out_o.detach(), 'x_src': xs_o.grad, 'x_dst': None if xd is None else xd_o.grad}
    ref.update({k: p.grad.clone() for k, p in conv.named_parameters()})
    # the restatement, on its own leaves
    leaves = {k: p.detach().clone().requires_grad_(True) for k, p in conv.named_parameters()}
    xs_r = xs.clone().requires_grad_(True)
    xd_r = None if xd is None else xd.clone().requires_grad_(True)
    out_r = R.reassociated_conv(xs_r, xd_r, ei, leaves['lin_src.weight'], leaves.get('lin_dst.weight'), leaves['att_src'],
                                leaves['att_dst'], leaves['bias'], H)
    (out_r * G).sum().backward()
    got = {'out': out_r.detach(), 'x_src': xs_r.grad, 'x_dst': None if xd is None else xd_r.grad}
    got.update({k: p.grad for k, p in leaves.items()})
    return got, ref


def _check(got, ref, what):
    assert set(got) == set(ref)
    for k in ref:
        if ref[k] is None:
            assert got[k] is None
            continue
        scale = float(ref[k].abs().max())
        assert scale > 0, (what, k)
        err = float((got[k] - ref[k]).abs().max())
        assert err <= REL_TOL * scale, (what, k, err, scale)


@pytest.mark.parametrize('cl', [128, 64])
@pytest.mark.parametrize('H', [2, 4])
def test_reassociated_form_is_gatconv_with_heads(H, cl):
    n, e = make_graph()
    assert len(n) == 3 and len(e) == 6
    for k, (et, ei) in enumerate(e.items()):
        got, ref = _both(et, ei, n, cl, H, seed=100 * H + k)
        assert ref['att_src'].shape == (1, H, cl // H)
        _check(got, ref, (et, H, cl))
        # a destination row without in-edges is the bias alone
        deg = torch.bincount(ei[1], minlength=n[et[2]])
        if bool((deg == 0).any()):
            assert torch.equal(got['out'][deg == 0], ref['out'][deg == 0])


def test_one_head_is_the_single_head_oracle():
    n, e = make_graph()
    for k, (et, ei) in enumerate(e.items()):
        got, ref = _both(et, ei, n, 128, 1, seed=7 + k)
        _check(got, ref, (et, 1, 128))


def test_heads_are_not_one_head():
    """The same parameters read as one head give another function: the head structure is really there."""
    n, e = make_graph()
    et, ei = next(iter(e.items()))
    conv, xs, xd, _ = _conv_and_inputs(et, n, 64, 4, seed=3)
    p = dict(conv.named_parameters())
    a = R.reassociated_conv(xs, xd, ei, p['lin_src.weight'], p['lin_dst.weight'], p['att_src'], p['att_dst'], p['bias'], 4)
    b = R.reassociated_conv(xs, xd, ei, p['lin_src.weight'], p['lin_dst.weight'], p['att_src'], p['att_dst'], p['bias'], 1)
    assert float((a - b).detach().abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------------------------------------
# the product's host side
# ------------------------------------------------------------------------------------------------------------------------------
def _model(kg, H, cl=128, **kw):
    from kgwas_amd.model import HeteroGNN
    args = dict(gnn_backbone='GAT', gnn_aggr='sum')
    args.update(kw)
    backbone, aggr = args.pop('gnn_backbone'), args.pop('gnn_aggr')
    args.setdefault('gat_split_heads', True)
    return HeteroGNN(kg.data, cl, 1, 2, backbone, aggr, 20, 40, 128, H, **args)


@pytest.mark.parametrize('cl', [128, 64])
@pytest.mark.parametrize('H', [2, 4])
def test_constructor_state_dict_and_glorot_bound(tiny_kg, H, cl):
    torch.manual_seed(H + cl)
    m = _model(tiny_kg, H, cl)
    assert m.heads == H and not m.fold_fc
    c = cl // H
    assert m.head_mask.shape == (H, 128) and torch.equal(m.head_mask.sum(0), (torch.arange(128) < cl).float())
    assert all(torch.equal(m.head_mask[h, h * c:(h + 1) * c], torch.ones(c)) for h in range(H))
    sd = m.state_dict()
    bound = math.sqrt(6.0 / (H + c))
    n_att = 0
    for k, v in sd.items():
        if isinstance(v, torch.nn.parameter.UninitializedParameter):
            continue
        if k.endswith('.att_src') or k.endswith('.att_dst'):
            assert v.shape == (1, H, c), (k, v.shape)
            assert float(v.abs().max()) <= bound
            n_att += v.numel()
        elif k.endswith('lin_src.weight') or k.endswith('lin_dst.weight'):
            assert v.shape == (cl, cl), (k, v.shape)
        elif k.startswith('convs.') and k.endswith('.bias'):
            assert v.shape == (cl,)
    # the draw fills the bound: with thousands of values the largest sits within 1 % of it, and above one head's bound
    allv = torch.cat([v.reshape(-1) for k, v in sd.items() if k.endswith('.att_src') or k.endswith('.att_dst')])
    assert n_att > 2000 and float(allv.abs().max()) > 0.99 * bound > math.sqrt(6.0 / (1 + cl))
    # the flat storage: column c of the 128-wide row is element (c // c', c % c') of the view, zero beyond cl
    P = m.live_packs[0]
    assert torch.equal(P.get(0, 'att_src').reshape(-1), P.att_src[0, :cl].detach()) and float(P.att_src.detach()[:, cl:].abs().sum()) == 0.0
    # round trip
    m2 = _model(tiny_kg, H, cl)
    m2.load_state_dict(sd)
    a, b = m.named_reference_tensors(), m2.named_reference_tensors()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    # the oracle with heads takes the same state
    o = R.oracle_with_heads(m)
    conv = next(iter(o.convs[0].convs.values()))
    assert conv.heads == H and conv.out_channels == c and conv.att_src.shape == (1, H, c)


def test_one_head_model_is_unchanged(tiny_kg):
    torch.manual_seed(1)
    a = _model(tiny_kg, 1)
    torch.manual_seed(1)
    from kgwas_amd.model import HeteroGNN
    b = HeteroGNN(tiny_kg.data, 128, 1, 2, 'GAT', 'sum', 20, 40, 128, 1)
    assert a.heads == 1 and not hasattr(a, 'head_mask')
    sa, sb = a.named_reference_tensors(), b.named_reference_tensors()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert next(v for k, v in a.state_dict().items() if k.endswith('att_src')).shape == (1, 1, 128)


def test_refusals(tiny_kg):
    for H in (3, 8, 0, -2, 2.5):
        with pytest.raises(NotImplementedError, match='head'):
            _model(tiny_kg, H)
    # the constructor's reference signature alone keeps the reference's literal meaning of H heads: refused, and says how to ask
    with pytest.raises(NotImplementedError, match='gat_split_heads=True'):
        _model(tiny_kg, 2, gat_split_heads=False)
    assert _model(tiny_kg, 1, gat_split_heads=False).heads == 1
    with pytest.raises(NotImplementedError, match='divide'):
        _model(tiny_kg, 4, cl=90)
    with pytest.raises(ValueError, match='SAGE'):
        _model(tiny_kg, 2, gnn_backbone='SAGE')
    for aggr in ('min', 'max'):
        with pytest.raises(NotImplementedError, match='gnn_aggr'):
            _model(tiny_kg, 2, gnn_aggr=aggr)
    with pytest.raises(NotImplementedError, match='gat_dropout'):
        _model(tiny_kg, 2, gat_dropout=0.1)
    m = _model(tiny_kg, 2)
    with pytest.raises(NotImplementedError, match='return_attention_weights'):
        m({}, {}, 1, return_attention_weights=True)
    with pytest.raises(NotImplementedError, match='hot_path_attention'):
        m.hot_path_attention(None)
    with pytest.raises(NotImplementedError, match='raw_attention_full_graph'):
        m.raw_attention_full_graph(tiny_kg.data)
    # get_disease_critical_network starts with the attention export
    from kgwas_amd.utils import get_network_weight
    run = types.SimpleNamespace(model=m, best_model=None, device='cpu')
    with pytest.raises(NotImplementedError, match='get_disease_critical_network'):
        get_network_weight(run, tiny_kg)
    # the SNP-sharded trainer
    from kgwas_amd.kgwas import KGWAS
    k = KGWAS(tiny_kg, device='cpu', seed=1)
    k.initialize_model(gat_num_head=2)
    assert k.config['gat_num_head'] == 2 and k.model.heads == 2
    with pytest.raises(NotImplementedError, match="parallelism='shard'"):
        k.train(batch_size=32, epoch=1, parallelism='shard')


def test_abi_names_the_field():
    """KgwLayerArgs.n_heads sits in the former padding word: the struct keeps its size, and the library refuses values it does
    not know by VALUE, before it looks at anything else (no device needed)."""
    import ctypes as C
    from kgwas_amd import _lib
    f = _lib.KgwLayerArgs
    assert f.n_heads.offset == f.flags.offset + 4 and f.graph_host.offset == f.n_heads.offset + 4
    L = _lib.lib()
    for bad in (3, 5, 8, -1):
        a = f()
        a.n_heads = bad
        for fn in (L.kgw_gat_aggregate_fwd, L.kgw_gat_aggregate_bwd_dst, L.kgw_gat_aggregate_bwd_src):
            assert fn(C.byref(a), None) == -2, (bad, fn)
        out = C.c_float()
        assert L.kgw_edge_alpha(C.byref(a), C.byref(out), None) == -2
    assert _lib.has_heads()
    hdr = open(__import__('os').path.join(__import__('os').path.dirname(__file__), '..', 'include', 'kgwas_hip.h')).read()
    for s in ('int32_t n_heads;', '[NH][n_rels][128]', '[NH][z rows][128]', '[NH][n_edges][2]', '[NH][2][n_rels][8][128]'):
        assert s in hdr, s
