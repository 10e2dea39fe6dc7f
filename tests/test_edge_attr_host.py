"""CPU: edge attributes (gat_edge_dim; KgwEdgeAttr in include/kgwas_hip.h).  (1) A self-check of the test reference, not of
the product: the two float64 restatements in tests/edge_attr_ref.py -- the literal text of the reference's edge_update
(kgwas/conv.py:207-215) and the re-associated rule of the header -- are held against each other to 1e-10, for D = 1 (1-D
attributes), 3 and 8, and the model oracle's attributed convolution against the rule, output and every gradient (the kernels
themselves are held against these restatements in tests/test_gpu_edge_attr_kernels.py); (2) the attribute reorder is
build_csr's, duplicates and self-loops included; (3) state-dict keys and shapes, the save / load round trip and what enters
``config``; (4) every refusal that needs no device; (5) the new symbols, KGW_VERSION and sizeof(KgwLayerArgs)."""
import ctypes as C
import os
import pickle
import re
import types

import numpy as np
import pytest
import torch

from tests import edge_attr_ref as R

REL_TOL = 1e-10


@pytest.fixture(scope='module')
def attr_kg(tmp_path_factory):
    """The tiny synthetic KG with 3-wide attributes on two bipartite relations (and their mirrors) and one same-type relation."""
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path_factory.mktemp('eattr_host')),
                                     edge_dim=3, edge_attr_relations=['ABC', 'eQTL', 'Gene-Signaling-Gene'])


ATTR_TYPES = [('SNP', 'ABC', 'Gene'), ('SNP', 'eQTL', 'Gene'), ('Gene', 'Gene-Signaling-Gene', 'Gene'), ('Gene', 'rev_ABC', 'SNP'),
              ('Gene', 'rev_eQTL', 'SNP')]


# ------------------------------------------------------------------------------------------------------------------------------
# (1) the rule
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 3, 8])
@pytest.mark.parametrize('same_type', [False, True])
def test_reassociated_rule_is_the_literal_edge_update(D, same_type):
    g = torch.Generator().manual_seed(10 * D + same_type)
    cl, n_src, n_dst, E = 64, 23, 23 if same_type else 11, 140
    conv = R.EdgeGATConvOracle(cl, None if same_type else cl, cl, D, dtype=torch.float64, gen=g)
    xs = torch.randn(n_src, cl, generator=g, dtype=torch.float64)
    xd = xs if same_type else torch.randn(n_dst, cl, generator=g, dtype=torch.float64)
    ei = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    attr = torch.randn(E, D, generator=g, dtype=torch.float64)
    if D == 1:
        attr = attr.reshape(-1)                    # conv.py:208-209: the view(-1, 1) case
    w_dst = conv.lin_src.weight if same_type else conv.lin_dst.weight
    args = (xs, xd, ei, attr, conv.lin_src.weight, w_dst, conv.att_src, conv.att_dst, conv.lin_edge.weight, conv.att_edge)
    with torch.no_grad():
        lit, re_ = R.literal_pre_logit(*args), R.reassociated_pre_logit(*args)
        scale = float(lit.abs().max())
        assert scale > 0 and float((lit - re_).abs().max()) <= REL_TOL * scale
        # the edge term is really in there
        zero = torch.zeros_like(attr)
        assert float((R.literal_pre_logit(xs, xd, ei, zero, *args[4:]) - lit).abs().max()) > 1e-3 * scale
    # ... and the oracle's attributed convolution is that logit through the softmax: output and every gradient against the rule
    G = torch.randn(n_dst, cl, generator=g, dtype=torch.float64)
    out = conv(xs if same_type else (xs, xd), ei, attr)
    (out * G).sum().backward()
    ref = {n: p.grad.clone() for n, p in conv.named_parameters()}
    leaves = {n: p.detach().clone().requires_grad_(True) for n, p in conv.named_parameters()}
    wd = leaves['lin_src.weight'] if same_type else leaves['lin_dst.weight']
    pre = R.reassociated_pre_logit(xs, xd, ei, attr, leaves['lin_src.weight'], wd, leaves['att_src'], leaves['att_dst'],
                                   leaves['lin_edge.weight'], leaves['att_edge'])
    from oracle.pyg_semantics import segment_softmax
    alpha = segment_softmax(torch.nn.functional.leaky_relu(pre, 0.2), ei[1], n_dst)
    z = torch.zeros(n_dst, cl, dtype=torch.float64).index_add(0, ei[1], alpha.unsqueeze(1) * xs[ei[0]])
    out_r = z @ leaves['lin_src.weight'].t() + leaves['bias']
    (out_r * G).sum().backward()
    assert float((out_r - out).detach().abs().max()) <= REL_TOL * float(out.detach().abs().max())
    for n in ref:
        s = float(ref[n].abs().max())
        assert s > 0 and float((leaves[n].grad - ref[n]).abs().max()) <= REL_TOL * s, n
    assert {'lin_edge.weight', 'att_edge'} <= set(ref) and tuple(ref['lin_edge.weight'].shape) == (cl, D)


# ------------------------------------------------------------------------------------------------------------------------------
# (2) the reorder
# ------------------------------------------------------------------------------------------------------------------------------
def test_attribute_reorder_is_build_csrs():
    from kgwas_amd.graph import build_csr, csr_edge_attr, csr_order
    rng = np.random.default_rng(3)
    n_src, n_dst = 9, 7
    ei = np.stack([rng.integers(0, n_src, 60), rng.integers(0, n_dst, 60)])
    ei = np.concatenate([ei, ei[:, :10], np.array([[2, 2, 2, 5], [2, 2, 2, 5]])], axis=1)      # duplicates, self-loops (thrice)
    attr = np.arange(ei.shape[1] * 2, dtype=np.float32).reshape(-1, 2)                         # row e names column e
    rowptr, col = build_csr(ei, n_src, n_dst)
    order = csr_order(ei, n_src, n_dst)
    a = csr_edge_attr(attr, ei, n_src, n_dst)
    assert a.dtype == np.float32 and a.shape == attr.shape
    assert np.array_equal(col, ei[0][order]) and np.array_equal(a, attr[order])
    e_of = (a[:, 0] / 2).astype(np.int64)                  # the edge_index column every CSR entry came from
    for d in range(n_dst):
        seg = e_of[rowptr[d]:rowptr[d + 1]]
        assert np.all(ei[1][seg] == d) and np.array_equal(ei[0][seg], col[rowptr[d]:rowptr[d + 1]])
        for s in set(col[rowptr[d]:rowptr[d + 1]].tolist()):    # parallel edges keep their own rows, in edge_index order
            par = seg[ei[0][seg] == s]
            assert np.all(np.diff(par) > 0)
    assert sorted(e_of.tolist()) == list(range(ei.shape[1]))
    # 1-D attributes are a column; a cached CSR must be the same sort
    assert csr_edge_attr(attr[:, 0], ei, n_src, n_dst, col=col).shape == (ei.shape[1], 1)
    with pytest.raises(AssertionError):
        csr_edge_attr(attr, ei, n_src, n_dst, col=col[::-1])
    with pytest.raises(ValueError):
        csr_edge_attr(attr[:-1], ei, n_src, n_dst)


def test_set_edge_attr_checks(attr_kg):
    from kgwas_amd.kgwas_data import KGWAS_Data
    kg = attr_kg
    for et in kg.data.edge_types:
        a = kg.data[et].get('edge_attr')
        assert (a is not None) == (et in ATTR_TYPES), et
        if a is not None:
            assert a.dtype == torch.float32 and tuple(a.shape) == (kg.data[et].edge_index.shape[1], 3)
    # a mirror repeats its forward relation's values edge by edge
    assert torch.equal(kg.data[('SNP', 'ABC', 'Gene')].edge_attr, kg.data[('Gene', 'rev_ABC', 'SNP')].edge_attr)
    assert torch.equal(kg.data[('SNP', 'ABC', 'Gene')].edge_index.flip(0), kg.data[('Gene', 'rev_ABC', 'SNP')].edge_index)
    et = ('SNP', 'TSS', 'Gene')
    E = kg.data[et].edge_index.shape[1]
    with pytest.raises(ValueError, match='edges'):
        kg.set_edge_attr({et: np.zeros((E - 1, 3))})
    with pytest.raises(ValueError, match='finite'):
        kg.set_edge_attr({et: np.full((E, 3), np.nan)})
    with pytest.raises(ValueError, match='width'):
        kg.set_edge_attr({et: np.zeros((E, 2))})
    with pytest.raises(ValueError, match='not in the graph'):
        kg.set_edge_attr({('SNP', 'nope', 'Gene'): np.zeros((E, 3))})
    assert kg.data[et].get('edge_attr') is None                      # a refused call changes nothing
    with pytest.raises(ValueError):
        KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=kg.data_path, edge_dim=9)


# ------------------------------------------------------------------------------------------------------------------------------
# (3) parameters, state dict, config
# ------------------------------------------------------------------------------------------------------------------------------
def _model(kg, cl=128, **kw):
    from kgwas_amd.model import HeteroGNN
    args = dict(gnn_backbone='GAT', gnn_aggr='sum', gat_num_head=1)
    args.update(kw)
    backbone, aggr, heads = args.pop('gnn_backbone'), args.pop('gnn_aggr'), args.pop('gat_num_head')
    return HeteroGNN(kg.data, cl, 1, 2, backbone, aggr, 20, 40, 128, heads, **args)


@pytest.mark.parametrize('cl', [128, 96])
def test_state_dict_keys_shapes_and_round_trip(attr_kg, cl):
    from kgwas_amd.model import edge_key
    torch.manual_seed(4)
    plain = _model(attr_kg, cl)
    torch.manual_seed(4)
    m = _model(attr_kg, cl, gat_edge_dim=3)
    assert m.edge_dim == 3 and [m.edge_types[r] for r in m.attr_rels] == ATTR_TYPES and m.fold_fc
    sd, sd0 = m.state_dict(), plain.state_dict()
    extra = sorted(set(sd) - set(sd0))
    want = sorted(f'convs.{l}.convs.{edge_key(et)}.{f}' for l in range(2) for et in ATTR_TYPES for f in ('lin_edge.weight', 'att_edge'))
    assert extra == want and set(sd0) <= set(sd)
    for k in extra:
        assert tuple(sd[k].shape) == ((cl, 3) if k.endswith('lin_edge.weight') else (1, 1, cl)), k
        bound = (6.0 / (cl + 3)) ** 0.5 if k.endswith('lin_edge.weight') else (6.0 / (1 + cl)) ** 0.5
        assert 0.5 * bound < float(sd[k].abs().max()) <= bound, k
    # the other tensors are drawn as ever up to the first pack's edge parameters; the storage beyond the model's width stays zero
    for P in list(m.live_packs) + list(m.dead_packs):
        assert P.w_edge_t.shape[1:] == (3, 128) and float(P.w_edge_t.detach()[:, :, cl:].abs().sum()) == 0.0
        assert float(P.att_edge.detach()[:, cl:].abs().sum()) == 0.0
    # the float64 oracle takes the keys as they are
    o = R.oracle_from_product(m)
    assert isinstance(o.convs[0].convs[edge_key(ATTR_TYPES[0])], R.EdgeGATConvOracle)
    assert not isinstance(o.convs[0].convs[edge_key(('SNP', 'TSS', 'Gene'))], R.EdgeGATConvOracle)
    m2 = _model(attr_kg, cl, gat_edge_dim=3)
    m2.load_state_dict(sd)
    a, b = m.named_reference_tensors(), m2.named_reference_tensors()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(RuntimeError, match='missing'):
        m2.load_state_dict(sd0)                                  # a plain checkpoint lacks the edge tensors
    with pytest.raises(RuntimeError, match='unexpected'):
        plain.load_state_dict(sd)


def test_config_and_load_pretrained_round_trip(attr_kg, tmp_path):
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.utils import save_model
    base = {'gnn_num_layers': 2, 'gnn_hidden_dim': 128, 'gnn_backbone': 'GAT', 'gnn_aggr': 'sum', 'gat_num_head': 1}
    k = KGWAS(attr_kg, device='cpu', seed=1)
    k.initialize_model()
    assert k.config == base and k.model.edge_dim is None        # attributes on the graph alone change nothing
    k.initialize_model(gat_edge_dim=None)
    assert k.config == base
    k.initialize_model(gat_edge_dim=3, gnn_hidden_dim=96)
    assert k.config == dict(base, gnn_hidden_dim=96, gat_edge_dim=3) and k.model.edge_dim == 3
    path = os.path.join(str(tmp_path), 'eattr')
    save_model(k.model, k.config, path)
    with open(os.path.join(path, 'config.pkl'), 'rb') as f:
        assert pickle.load(f)['gat_edge_dim'] == 3
    k2 = KGWAS(attr_kg, device='cpu', seed=2)
    k2.load_pretrained(path)
    assert k2.config == k.config and k2.model.edge_dim == 3 and k2.model.hidden_logical == 96 and k2.model.fold_fc
    a, b = k.model.named_reference_tensors(), k2.model.named_reference_tensors()
    assert set(a) == set(b) and all(torch.equal(a[n], b[n]) for n in a)
    assert sum(n.endswith('att_edge') for n in a) == 2 * len(ATTR_TYPES)


# ------------------------------------------------------------------------------------------------------------------------------
# (4) refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_constructor_refusals(attr_kg, tiny_kg):
    from kgwas_amd.model import HeteroGNN
    with pytest.raises(TypeError):                               # keyword only
        HeteroGNN(attr_kg.data, 128, 1, 2, 'GAT', 'sum', 20, 40, 128, 1, False, 0.0, False, 3)
    with pytest.raises(ValueError, match='SAGE'):
        _model(attr_kg, gat_edge_dim=3, gnn_backbone='SAGE')
    for H in (2, 4):
        with pytest.raises(NotImplementedError, match='gat_num_head'):
            _model(attr_kg, gat_edge_dim=3, gat_num_head=H, gat_split_heads=True)
    with pytest.raises(NotImplementedError, match='gat_dropout'):
        _model(attr_kg, gat_edge_dim=3, gat_dropout=0.1)
    with pytest.raises(NotImplementedError, match='gat_sigmoid'):
        _model(attr_kg, gat_edge_dim=3, gat_sigmoid=True)
    with pytest.raises(ValueError, match='no relation'):
        _model(tiny_kg, gat_edge_dim=3)                          # a graph without attributes
    with pytest.raises(ValueError, match='width'):
        _model(attr_kg, gat_edge_dim=4)                          # the graph's attributes are 3 wide
    for bad in (0, 9, 2.5):
        with pytest.raises(ValueError, match='gat_edge_dim'):
            _model(attr_kg, gat_edge_dim=bad)
    for aggr in ('sum', 'mean', 'min', 'max'):
        assert _model(attr_kg, gat_edge_dim=3, gnn_aggr=aggr).aggr == aggr
    assert _model(attr_kg, gat_edge_dim=3, gat_temperature=2.0).temperature == 2.0


def test_trainer_refusals(attr_kg):
    from kgwas_amd.kgwas import KGWAS
    k = KGWAS(attr_kg, device='cpu', seed=1)
    k.initialize_model(gat_edge_dim=3)
    with pytest.raises(NotImplementedError, match="parallelism='shard'"):
        k.train(batch_size=32, epoch=1, parallelism='shard')
    with pytest.raises(NotImplementedError, match='num_neighbors'):
        k.train(batch_size=32, epoch=1, num_neighbors=[10, 5])


def test_coo_route_needs_every_attributed_relation(attr_kg):
    m = _model(attr_kg, gat_edge_dim=3)
    g = attr_kg.data
    x = {t: g[t].x for t in g.node_types}
    ei = {et: g[et].edge_index for et in g.edge_types}
    ea = {et: g[et].edge_attr for et in ATTR_TYPES[1:]}
    with pytest.raises(ValueError, match='edge_attr_dict'):
        m(x, ei, 8, edge_attr_dict=ea)
    with pytest.raises(ValueError, match='edge_attr_dict'):
        m(x, ei, 8)


def test_ops_refusals_that_need_no_device():
    from kgwas_amd import ops
    batch = types.SimpleNamespace()
    term = torch.zeros(4)
    word = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match='sigmoid_gate'):
        ops.gat_aggregate(batch, 1, None, None, None, edge_term=term, sigmoid_gate=True)
    for H in (2, 4):
        with pytest.raises(NotImplementedError, match='heads'):
            ops.gat_aggregate(batch, 1, None, None, None, edge_term=term, heads=H)
    with pytest.raises(NotImplementedError, match='dropout'):
        ops.gat_aggregate(batch, 1, None, None, None, edge_term=term, dropout=(0.1, word))
    sharded = types.SimpleNamespace(exchange=types.SimpleNamespace())
    with pytest.raises(NotImplementedError, match='SNP-sharded'):
        ops.gat_aggregate(sharded, 1, None, None, None, edge_term=term)
    with pytest.raises(ValueError, match='no edge attributes'):
        ops.edge_logit_term(types.SimpleNamespace(dg=types.SimpleNamespace(g_eattr=None)), 1, term)
    with pytest.raises(NotImplementedError, match='SNP-sharded'):
        ops.edge_logit_term(types.SimpleNamespace(dg=types.SimpleNamespace(g_eattr=term), exchange=object()), 1, term)


# ------------------------------------------------------------------------------------------------------------------------------
# (5) the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_sizes_and_refusals_by_value():
    from kgwas_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'kgwas_hip.h')).read()
    for name in ('kgw_edge_term_fwd', 'kgw_edge_term_bwd', 'kgw_edge_term_workspace_floats', 'kgw_gat_aggregate_fwd_eterm'):
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r'\b' + name + r'\s*\(', hdr), name
    assert _lib.has_edge_attr()
    assert L.kgw_version() == 125 and int(re.search(r'#define KGW_VERSION\s+(\d+)', hdr).group(1)) == 125
    # KgwLayerArgs is what it was: size, and the offsets of its last fields (tests/test_attn_dropout_rule.py pins them too)
    f = _lib.KgwLayerArgs
    assert C.sizeof(f) == 336 and f.drop_word_dev.offset == 320 and f.n_heads.offset == 28
    sizes = (C.c_int64 * 8)()
    assert L.kgw_struct_sizes(sizes, 8) == 0
    assert list(sizes)[:7] == [C.sizeof(_lib.KgwGraph), C.sizeof(_lib.KgwBatchMeta), C.sizeof(_lib.KgwChunk), C.sizeof(_lib.KgwBatchBuf),
                               C.sizeof(f), C.sizeof(_lib.KgwTnJob), C.sizeof(_lib.KgwGradSrc)]
    assert sizes[7] == C.sizeof(_lib.KgwEdgeAttr) == 8 + 8 * 64 + 8 + 6 * 8
    seven = (C.c_int64 * 8)(*([-1] * 8))
    assert L.kgw_struct_sizes(seven, 7) == 0 and seven[7] == -1 and list(seven)[:7] == list(sizes)[:7]
    # refused by value, before anything else is looked at (no launch, no device needed)
    term = C.c_float(0)
    tp = C.cast(C.pointer(term), C.c_void_p)
    word = C.c_uint64(0)
    for kw in (dict(flags=_lib.KGW_F_SIGMOID_GATE), dict(n_heads=2), dict(n_heads=4), dict(partial_rels=1),
               dict(drop_word_dev=C.cast(C.pointer(word), C.c_void_p).value, drop_scale=1.0)):
        a = f()
        for k, v in kw.items():
            setattr(a, k, v)
        assert L.kgw_gat_aggregate_fwd_eterm(C.byref(a), tp, None) == _lib.KGW_E_UNSUPPORTED, kw
    a = f()
    assert L.kgw_gat_aggregate_fwd_eterm(C.byref(a), tp, None) == 0           # an empty layer: nothing to do
    a.flags = 1
    assert L.kgw_gat_aggregate_fwd_eterm(C.byref(a), tp, None) == 0           # raw weights take the term
    for dim in (0, 9, -3):
        ea = _lib.KgwEdgeAttr()
        ea.dim = dim
        assert L.kgw_edge_term_fwd(C.byref(f()), C.byref(ea), None) == -2, dim
        assert L.kgw_edge_term_bwd(C.byref(f()), C.byref(ea), None) == -2, dim
    ea = _lib.KgwEdgeAttr()
    ea.dim = 4
    assert L.kgw_edge_term_fwd(C.byref(f()), C.byref(ea), None) == 0          # an empty layer
    assert L.kgw_edge_term_fwd(None, C.byref(ea), None) == -1 and L.kgw_edge_term_bwd(C.byref(f()), None, None) == -1
    assert L.kgw_edge_term_workspace_floats(C.byref(f())) == 8
