"""CPU: sigmoid-gated attention and the temperature (gat_sigmoid / gat_temperature).  (1) The re-associated form the kernels compute
(tests/sigmoid_gate_ref.py) IS the reference's GATConv(sigmoid_gat=True, temperature=T) -- oracle/gat_oracle.py:GATConvOracle --
output and every gradient, in float64 to 1e-10 relative; (2) what enters ``config`` and the load_pretrained round trip; (3) every
refusal that needs no device; (4) the flag of the C ABI and its refusals by value (no launch)."""
import ctypes as C
import math
import os
import re
import types

import pytest
import torch

from oracle.gat_oracle import GATConvOracle
from tests import sigmoid_gate_ref as R
from tests.test_multihead_host import make_graph

REL_TOL = 1e-10


@pytest.mark.parametrize('temp', [1.0, 0.5, 2.5])
@pytest.mark.parametrize('slope', [0.2, 0.05])
def test_reassociated_form_is_gatconv_with_sigmoid_gat(slope, temp):
    n, e = make_graph()
    cl = 64
    for k, (et, ei) in enumerate(e.items()):
        g = torch.Generator().manual_seed(50 + k)
        s, _, d = et
        conv = GATConvOracle(cl, None if s == d else cl, cl, negative_slope=slope, sigmoid_gat=True, temperature=temp,
                             dtype=torch.float64, gen=g)
        with torch.no_grad():
            conv.bias.copy_(torch.randn(cl, generator=g, dtype=torch.float64) * 0.1)
        xs = torch.randn(n[s], cl, generator=g, dtype=torch.float64)
        xd = None if s == d else torch.randn(n[d], cl, generator=g, dtype=torch.float64)
        G = torch.randn(n[d], cl, generator=g, dtype=torch.float64)
        xs_o = xs.clone().requires_grad_(True)
        xd_o = None if xd is None else xd.clone().requires_grad_(True)
        out_o = conv(xs_o if xd is None else (xs_o, xd_o), ei)
        (out_o * G).sum().backward()
        ref = {'out': out_o.detach(), 'x_src': xs_o.grad, 'x_dst': None if xd is None else xd_o.grad}
        ref.update({name: p.grad.clone() for name, p in conv.named_parameters()})
        leaves = {name: p.detach().clone().requires_grad_(True) for name, p in conv.named_parameters()}
        xs_r = xs.clone().requires_grad_(True)
        xd_r = None if xd is None else xd.clone().requires_grad_(True)
        out_r = R.reassociated_gated_conv(xs_r, xd_r, ei, leaves['lin_src.weight'], leaves.get('lin_dst.weight'), leaves['att_src'],
                                          leaves['att_dst'], leaves['bias'], slope, temp)
        (out_r * G).sum().backward()
        got = {'out': out_r.detach(), 'x_src': xs_r.grad, 'x_dst': None if xd is None else xd_r.grad}
        got.update({name: p.grad for name, p in leaves.items()})
        assert set(got) == set(ref)
        for name in ref:
            if ref[name] is None:
                assert got[name] is None
                continue
            scale = float(ref[name].abs().max())
            assert scale > 0, (et, name)
            err = float((got[name] - ref[name]).abs().max())
            assert err <= REL_TOL * scale, (et, name, err, scale)
        # a destination row without in-edges is the bias alone; the gates are not a softmax (a row's weights do not sum to 1)
        deg = torch.bincount(ei[1], minlength=n[d])
        if bool((deg == 0).any()):
            assert torch.equal(got['out'][deg == 0], ref['out'][deg == 0])
    conv.sigmoid_gat = False
    with torch.no_grad():
        assert float((conv(xs if xd is None else (xs, xd), ei) - out_o).abs().max()) > 1e-3


def _model(kg, **kw):
    from kgwas_amd.model import HeteroGNN
    args = dict(gnn_backbone='GAT', gnn_aggr='sum', gat_num_head=1)
    args.update(kw)
    backbone, aggr, heads = args.pop('gnn_backbone'), args.pop('gnn_aggr'), args.pop('gat_num_head')
    return HeteroGNN(kg.data, 128, 1, 2, backbone, aggr, 20, 40, 128, heads, **args)


def test_constructor(tiny_kg):
    m = _model(tiny_kg)
    assert m.gat_sigmoid is False and m.temperature == 1.0 and m.fold_fc
    m = _model(tiny_kg, gat_temperature=2)
    assert m.gat_sigmoid is False and m.temperature == 2.0 and m.fold_fc          # the temperature alone keeps the folded route
    m = _model(tiny_kg, gat_sigmoid=True, gat_temperature=0.5)
    assert m.gat_sigmoid is True and m.temperature == 0.5 and not m.fold_fc       # the gates do not sum to 1: no FC_output fold
    for aggr in ('sum', 'mean', 'min', 'max'):
        assert _model(tiny_kg, gat_sigmoid=True, gnn_aggr=aggr).aggr == aggr
    assert _model(tiny_kg, gnn_backbone='SAGE', gat_temperature=3.0).temperature == 3.0
    # keyword only, after gat_split_heads
    from kgwas_amd.model import HeteroGNN
    with pytest.raises(TypeError):
        HeteroGNN(tiny_kg.data, 128, 1, 2, 'GAT', 'sum', 20, 40, 128, 1, False, 0.0, False, True)
    # the same parameters whatever the switches: they change no tensor of the state_dict
    torch.manual_seed(4)
    a = _model(tiny_kg).named_reference_tensors()
    torch.manual_seed(4)
    b = _model(tiny_kg, gat_sigmoid=True, gat_temperature=2.0).named_reference_tensors()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_refusals(tiny_kg):
    for bad in (0.0, -1.0, math.inf, -math.inf, math.nan):
        with pytest.raises(ValueError, match='gat_temperature'):
            _model(tiny_kg, gat_temperature=bad)
        with pytest.raises(ValueError, match='gat_temperature'):
            _model(tiny_kg, gat_sigmoid=True, gat_temperature=bad)
    with pytest.raises(ValueError, match='SAGE'):
        _model(tiny_kg, gat_sigmoid=True, gnn_backbone='SAGE')
    for H in (2, 4):
        with pytest.raises(NotImplementedError, match='gat_num_head'):
            _model(tiny_kg, gat_sigmoid=True, gat_num_head=H, gat_split_heads=True)
    with pytest.raises(NotImplementedError, match='gat_dropout'):
        _model(tiny_kg, gat_sigmoid=True, gat_dropout=0.1)
    # the temperature alone goes with heads and with dropout: both routes already read it
    assert _model(tiny_kg, gat_temperature=2.0, gat_num_head=2, gat_split_heads=True).temperature == 2.0
    assert _model(tiny_kg, gat_temperature=2.0, gat_dropout=0.1).temperature == 2.0
    # the SNP-sharded trainer
    from kgwas_amd.kgwas import KGWAS
    for kw in (dict(gat_sigmoid=True), dict(gat_temperature=2.0), dict(gat_sigmoid=True, gat_temperature=0.5)):
        k = KGWAS(tiny_kg, device='cpu', seed=1)
        k.initialize_model(**kw)
        with pytest.raises(NotImplementedError, match="parallelism='shard'"):
            k.train(batch_size=32, epoch=1, parallelism='shard')


def test_ops_refusals_that_need_no_device():
    """ops.gat_aggregate(sigmoid_gate=True) refuses before it looks at a tensor."""
    from kgwas_amd import ops
    batch = types.SimpleNamespace()
    word = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match='raw_weights'):
        ops.gat_aggregate(batch, 1, None, None, None, sigmoid_gate=True, raw_weights=True)
    for H in (2, 4, 3):
        with pytest.raises(NotImplementedError, match='heads'):
            ops.gat_aggregate(batch, 1, None, None, None, sigmoid_gate=True, heads=H)
    with pytest.raises(NotImplementedError, match='dropout'):
        ops.gat_aggregate(batch, 1, None, None, None, sigmoid_gate=True, dropout=(0.1, word))
    sharded = types.SimpleNamespace(exchange=types.SimpleNamespace())
    with pytest.raises(NotImplementedError, match='SNP-sharded'):
        ops.gat_aggregate(sharded, 1, None, None, None, sigmoid_gate=True)


def test_config_and_load_pretrained_round_trip(tiny_kg, tmp_path):
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.utils import save_model
    base = {'gnn_num_layers': 2, 'gnn_hidden_dim': 128, 'gnn_backbone': 'GAT', 'gnn_aggr': 'sum', 'gat_num_head': 1}
    k = KGWAS(tiny_kg, device='cpu', seed=1)
    k.initialize_model()
    assert k.config == base                                                     # the config.pkl of a default run is what it was
    k.initialize_model(gat_sigmoid=False, gat_temperature=1)
    assert k.config == base
    k.initialize_model(gat_temperature=2.5)
    assert k.config == dict(base, gat_temperature=2.5) and k.model.temperature == 2.5 and not k.model.gat_sigmoid
    k.initialize_model(gat_sigmoid=True)
    assert k.config == dict(base, gat_sigmoid=True) and k.model.gat_sigmoid and k.model.temperature == 1.0
    k.initialize_model(gat_sigmoid=True, gat_temperature=0.5, gnn_hidden_dim=96)
    assert k.config == dict(base, gnn_hidden_dim=96, gat_sigmoid=True, gat_temperature=0.5)
    path = os.path.join(str(tmp_path), 'gated')
    save_model(k.model, k.config, path)
    k2 = KGWAS(tiny_kg, device='cpu', seed=2)
    k2.load_pretrained(path)
    assert k2.config == k.config
    assert k2.model.gat_sigmoid and k2.model.temperature == 0.5 and k2.model.hidden_logical == 96 and not k2.model.fold_fc
    a, b = k.model.named_reference_tensors(), k2.model.named_reference_tensors()
    assert set(a) == set(b) and all(torch.equal(a[n], b[n]) for n in a)


def test_abi_flag_and_refusals_by_value():
    """KGW_F_SIGMOID_GATE: the header's value is the binding's; every refused combination returns KGW_E_UNSUPPORTED on an
    otherwise empty KgwLayerArgs, from the forward and the dst-major backward, before anything else is looked at (no launch, no
    device needed); the src-major backward ignores the flag."""
    from kgwas_amd import _lib
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'kgwas_hip.h')).read()
    m = re.search(r'#define\s+KGW_F_SIGMOID_GATE\s+(\d+)', hdr)
    assert m and int(m.group(1)) == _lib.KGW_F_SIGMOID_GATE == 8
    flags = {name: int(v) for name, v in re.findall(r'#define\s+(KGW_F_\w+)\s+(\d+)', hdr)}
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 for v in flags.values()), flags
    assert 'kgwgate_weight' in hdr
    L = _lib.lib()
    f = _lib.KgwLayerArgs
    word = C.c_uint64(0)
    refused = [dict(flags=8 | flags['KGW_F_RAW_WEIGHTS']), dict(flags=8, n_heads=2), dict(flags=8, n_heads=4),
               dict(flags=8, partial_rels=1), dict(flags=8, partial_rels=1 << 40),
               dict(flags=8, drop_word_dev=C.cast(C.pointer(word), C.c_void_p).value, drop_scale=1.0),
               dict(flags=8 | flags['KGW_F_RELU_INPUT'], n_heads=2)]
    for kw in refused:
        a = f()
        for k, v in kw.items():
            setattr(a, k, v)
        assert L.kgw_gat_aggregate_fwd(C.byref(a), None) == _lib.KGW_E_UNSUPPORTED, kw
        assert L.kgw_gat_aggregate_bwd_dst(C.byref(a), None) == _lib.KGW_E_UNSUPPORTED, kw
    for kw in (dict(flags=8), dict(flags=8 | flags['KGW_F_RELU_INPUT']), dict(flags=8 | flags['KGW_F_DUV_PIECES'])):
        a = f()                                         # the flag alone on an empty layer: nothing to do, nothing refused
        for k, v in kw.items():
            setattr(a, k, v)
        for fn in (L.kgw_gat_aggregate_fwd, L.kgw_gat_aggregate_bwd_dst, L.kgw_gat_aggregate_bwd_src):
            assert fn(C.byref(a), None) == 0, (kw, fn)
    a = f()
    a.flags = 8 | flags['KGW_F_RAW_WEIGHTS']
    assert L.kgw_gat_aggregate_bwd_src(C.byref(a), None) == 0
    # the struct and the version are what they were
    sizes = (C.c_int64 * 7)()
    assert L.kgw_struct_sizes(sizes, 7) == 0 and sizes[4] == C.sizeof(f)
    assert _lib.has_sigmoid_gate() and _lib.has_heads()
