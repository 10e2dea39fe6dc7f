"""-m gpu: the edge-attribute kernels (k_edge_term, k_agg_fwd<.., ETERM>, k_edge_term_bwd and its fold; KgwEdgeAttr in
include/kgwas_hip.h) against the float64 restatement of tests/edge_attr_ref.py, on the batches of tests/test_gpu_aggregate_parity.py:
the degree ladder (rows of 0 to 9 edges for the 2 / 4 / 8 group forms, both sides of 32, 64 and 128, hub rows of 2, 3 and 8 chunks),
hop-pruned mini-batches, both layers.

Every third relation (id % 3 == 2) carries no attributes; the others get N(0, 1) rows [E_r, D] in CSR order, D in {1, 3, 4, 8}.
The reference finds the CSR position of a local edge from seg_ptr, n_id and the row pointers; the kernels read the chunks' gpos.

Bars: term, Z, e_edge, stat and alpha at the parity file's rtol 1e-4 / atol 1e-5; dH at 2e-5; dU, dV, d logit_bias and d w_r at
1e-4 (all through assert_close's rel_to_max); a gradient that misses the element-wise bound must be within 2 x the float32 oracle's
own error (that file's _check_residue), nothing wider."""
import copy
import ctypes as C

import pytest
import torch

from tests import edge_attr_ref as R
from tests.helpers import assert_close, segment_alpha_sums
from tests.test_gpu_aggregate_parity import ATOL, RTOL, _check_residue, _inputs, batches, ladder, layer_edges  # noqa: F401

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 4, 8)


def with_attrs(batch, D, seed=0, zero=False):
    """A view of ``batch`` whose graph carries attributes of width D on every relation with id % 3 != 2: (batch', {relation id:
    float32 [E_r, D] in CSR order}).  The batch's buffers and the resident CSR are shared; nothing of the original changes."""
    dg = copy.copy(batch.dg)
    sc = dg.schema
    g = torch.Generator().manual_seed(1000 + 17 * D + seed)
    rp = dg.g_rowptr.cpu().long()
    attrs, rows, off = {}, [], 0
    dg.eattr_off = [-1] * sc.NR
    for r in range(sc.NR):
        E = int(rp[int(dg.kg.rowptr_off[r]) + dg.n_nodes[int(sc.dst_type[r])]])
        if r % 3 == 2:
            continue
        a = torch.zeros(E, D) if zero else torch.randn(E, D, generator=g)
        attrs[r] = a
        dg.eattr_off[r] = off
        off += E
        rows.append(a)
    dg.eattr_dim, dg.eattr_rels = D, sorted(attrs)
    dg.g_eattr = torch.cat(rows).cuda()
    b = copy.copy(batch)
    b.dg = dg
    return b, attrs


def _w(batch, D, seed):
    return torch.randn(batch.dg.schema.NR, D, generator=torch.Generator().manual_seed(77 + seed)) * 0.5


def _run_gpu(batch, layer, H, U, V, kap, G, W, slope=0.2, temp=1.0, relu_input=False, plain=False):
    from kgwas_amd import ops
    m, sc = batch.meta, batch.dg.schema
    z_rows = int(m.z_base[layer - 1][sc.NT])
    n_edges = int(m.n_edges[layer - 1])
    Hd, Ud, Vd, Wd = (t.cuda().requires_grad_(True) for t in (H, U, V, W))
    kd = kap.cuda().requires_grad_(True) if kap is not None else None
    term = None if plain else ops.edge_logit_term(batch, layer, Wd)
    Z, stat, e_edge = ops.gat_aggregate(batch, layer, Hd, Ud, Vd, neg_slope=slope, temperature=temp, relu_input=relu_input,
                                        logit_bias=kd, edge_term=term)
    alpha = ops.edge_alpha(batch, layer, stat, e_edge, temperature=temp)
    (Z * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    return dict(Z=Z.detach().cpu(), stat=stat[:z_rows].cpu(), e=e_edge[:n_edges].cpu(), alpha=alpha.cpu(),
                term=None if plain else term.detach()[:n_edges].cpu(), dH=Hd.grad.cpu(), dU=Ud.grad.cpu(), dV=Vd.grad.cpu(),
                dW=None if plain else Wd.grad.cpu(), dlb=kd.grad.cpu() if kd is not None else None)


def check_case(batch0, layer, D, seed, relu_input=False, lbias=False, slope=0.2, temp=1.0):
    batch, attrs = with_attrs(batch0, D, seed)
    sc, dg = batch.dg.schema, batch.dg
    H, U, V, kap, G = _inputs(batch, layer, seed, relu_input, lbias)
    W = _w(batch, D, seed)
    edges = layer_edges(batch, layer)
    pos = R.layer_positions(batch, layer, edges)
    got = _run_gpu(batch, layer, H, U, V, kap, G, W, slope, temp, relu_input)
    ref = R.eattr_grads(batch, layer, H, U, V, W, kap, G, attrs, edges, pos, torch.float64, slope, temp, relu_input)
    cache = {}

    def lazy32():
        if not cache:
            cache.update(R.eattr_grads(batch, layer, H, U, V, W, kap, G, attrs, edges, pos, torch.float32, slope, temp, relu_input))
        return cache

    live = [r for r in range(sc.NR) if dg.kg.rel_live[layer - 1][r]]
    dead = [r for r in range(sc.NR) if not dg.kg.rel_live[layer - 1][r]]
    eid = torch.cat([edges[r][0] for r in edges])
    assert eid.numel() > 0 and any(r in attrs for r in edges)
    assert float(ref['term'].abs().max()) > 0.1, 'the term must matter'
    for name, bar in (('term', ATOL), ('Z', ATOL), ('stat', ATOL)):
        print(f'{name}: max abs err {float((got[name].double() - ref[name]).abs().max()):.3e}, max |ref| {float(ref[name].abs().max()):.3e}')
    assert_close(got['term'][eid], ref['term'][eid], RTOL, ATOL, 'term')
    for r in edges:                     # relations without attributes: exactly 0.0f
        if r not in attrs:
            assert float(got['term'][edges[r][0]].abs().sum()) == 0.0
    assert_close(got['Z'], ref['Z'], RTOL, ATOL, 'Z')
    assert_close(got['stat'], ref['stat'], RTOL, ATOL, 'stat (row max, denominator)')
    assert_close(got['e'][eid], ref['e'][eid], RTOL, ATOL, 'e_edge')
    assert_close(got['alpha'][eid], ref['alpha'][eid], RTOL, ATOL, 'alpha')
    sums = segment_alpha_sums(batch, layer, got['alpha'])
    assert sums.numel() > 0 and float((sums - 1.0).abs().max()) <= 1e-5, 'the softmax still sums to one'
    assert_close(got['dU'][live], ref['dU'][live], RTOL, 1e-4, 'dU')
    _check_residue('dH', got['dH'], ref['dH'], lazy32, 2e-5)
    _check_residue('dV', got['dV'][live], ref['dV'][live], lambda: {'dV': lazy32()['dV'][live]}, 1e-4)
    print(f'dW: max abs err {float((got["dW"].double() - ref["dW"]).abs().max()):.3e}, max |ref| {float(ref["dW"].abs().max()):.3e}')
    _check_residue('dW', got['dW'][live], ref['dW'][live], lambda: {'dW': lazy32()['dW'][live]}, 1e-4)
    assert float(ref['dW'].abs().max()) > 1e-3
    if lbias:
        _check_residue('dlb', got['dlb'][live], ref['dlb'][live], lambda: {'dlb': lazy32()['dlb'][live]}, 1e-4)
    # exact zeros: relations the layer does not compute, relations without attributes
    silent = dead + [r for r in range(sc.NR) if r not in attrs]
    assert float(got['dW'][silent].abs().sum()) == 0.0
    assert float(got['dU'][dead].abs().sum()) == 0.0 and float(got['dV'][dead].abs().sum()) == 0.0
    return got, ref


GRAPHS = [('ladder_full', 1), ('ladder_full', 2), ('ladder_mini', 1), ('ladder_mini', 2), ('small_mini', 2), ('edge_full', 1)]
# every graph and layer with one width, the switches of gat_aggregate alternating ...
CASES = [(g, l, DIMS[i % 4], bool(i & 1), bool(i & 2)) for i, (g, l) in enumerate(GRAPHS)]
# ... and every width on the degree ladder, both as a full graph and as a hop-pruned mini-batch
CASES += [('ladder_full', 1, D, True, True) for D in DIMS if D != 1] + [('ladder_mini', 1, D, False, True) for D in DIMS if D != 4]


@pytest.mark.parametrize('graph,layer,D,relu_input,lbias', CASES, ids=[f'{g}-L{l}-D{D}-relu{int(a)}-lb{int(b)}' for g, l, D, a, b in CASES])
def test_parity(batches, graph, layer, D, relu_input, lbias):
    check_case(batches(graph), layer, D, seed=10 * layer + D, relu_input=relu_input, lbias=lbias)


def test_other_slope_and_temperature(batches):
    check_case(batches('ladder_full'), 1, 3, seed=5, lbias=True, slope=0.05, temp=2.5)


@pytest.mark.parametrize('graph,layer', [('ladder_full', 1), ('ladder_mini', 2)])
def test_zero_attributes_give_the_plain_call_bit_for_bit(batches, graph, layer):
    batch, _ = with_attrs(batches(graph), 4, zero=True)
    H, U, V, kap, G = _inputs(batch, layer, seed=21, lbias=True)
    W = _w(batch, 4, 21)
    a = _run_gpu(batch, layer, H, U, V, kap, G, W)
    b = _run_gpu(batch, layer, H, U, V, kap, G, W, plain=True)
    assert float(a['term'].abs().sum()) == 0.0
    for k in ('Z', 'stat', 'e', 'alpha', 'dH', 'dU', 'dV', 'dlb'):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('graph', ['ladder_full', 'ladder_mini'])
def test_raw_weights_with_the_term(batches, graph):
    """The attention export's route: Z = sum e_ij H_j with the term inside e, stat (0, 1)."""
    from kgwas_amd import ops
    batch, attrs = with_attrs(batches(graph), 3)
    layer = 1
    H, U, V, kap, _ = _inputs(batch, layer, seed=7, lbias=True)
    W = _w(batch, 3, 7)
    edges = layer_edges(batch, layer)
    pos = R.layer_positions(batch, layer, edges)
    term = ops.edge_logit_term(batch, layer, W.cuda())
    Z, stat, e = ops.gat_aggregate(batch, layer, H.cuda(), U.cuda(), V.cuda(), raw_weights=True, logit_bias=kap.cuda(), edge_term=term)
    Zo, so, eo, _, _ = R.eattr_layer(batch, layer, H.double(), U.double(), V.double(), W.double(), attrs, edges, pos,
                                     lbias=kap.double(), raw=True)
    eid = torch.cat([edges[r][0] for r in edges])
    assert_close(Z, Zo, RTOL, ATOL, 'Z (raw)')
    assert_close(e[eid.cuda()], eo[eid], RTOL, ATOL, 'e_edge (raw)')
    assert torch.equal(stat[:Zo.shape[0]].cpu().double(), so)


def test_rerun_is_bit_identical(batches):
    """No atomics anywhere, a fixed two-level order in the gradient of w_r."""
    batch, _ = with_attrs(batches('ladder_mini'), 8)
    H, U, V, kap, G = _inputs(batch, 1, seed=3, lbias=True)
    W = _w(batch, 8, 3)
    a = _run_gpu(batch, 1, H, U, V, kap, G, W)
    b = _run_gpu(batch, 1, H, U, V, kap, G, W)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_strided_and_dense_gradient_of_the_term_agree(batches):
    """k_edge_term_bwd reads d_term through a pointer and a stride: the adp view (stride 2) and a dense copy give the same bits."""
    from kgwas_amd import ops
    batch, _ = with_attrs(batches('ladder_full'), 3)
    n = int(batch.meta.n_edges[0])
    g = torch.randn(max(n, 1), 2, generator=torch.Generator().manual_seed(4)).cuda()
    out = []
    for d_term in (g[:, 1], g[:, 1].contiguous()):
        W = _w(batch, 3, 1).cuda().requires_grad_(True)
        ops.edge_logit_term(batch, 1, W).backward(d_term)
        out.append(W.grad.clone())
    assert torch.equal(out[0], out[1]) and float(out[0].abs().max()) > 0


def test_refusals_at_the_c_abi(batches):
    from kgwas_amd import _lib, ops
    L = _lib.lib()
    batch, _ = with_attrs(batches('ladder_mini'), 3)
    a = ops._layer_args(batch, 1, 0.2, 1.0)
    term = torch.zeros(8, device='cuda')
    word = torch.zeros(1, dtype=torch.int64, device='cuda')

    def call(**kw):
        b = ops._layer_args(batch, 1, 0.2, 1.0)
        for k, v in kw.items():
            setattr(b, k, v)
        return L.kgw_gat_aggregate_fwd_eterm(C.byref(b), C.c_void_p(term.data_ptr()), None)
    assert call(flags=_lib.KGW_F_SIGMOID_GATE) == _lib.KGW_E_UNSUPPORTED
    assert call(n_heads=2) == _lib.KGW_E_UNSUPPORTED
    assert call(drop_word_dev=word.data_ptr(), drop_scale=1.0) == _lib.KGW_E_UNSUPPORTED
    assert call(partial_rels=1) == _lib.KGW_E_UNSUPPORTED
    assert call(n_heads=3) == -2
    for dim in (0, 9, -1):
        ea = ops._edge_attr_args(batch)
        ea.dim = dim
        assert L.kgw_edge_term_fwd(C.byref(a), C.byref(ea), None) == -2
        assert L.kgw_edge_term_bwd(C.byref(a), C.byref(ea), None) == -2
    assert L.kgw_edge_term_fwd(C.byref(a), None, None) == -1 and L.kgw_gat_aggregate_fwd_eterm(C.byref(a), None, None) == -1
    with pytest.raises(NotImplementedError):
        ops.gat_aggregate(batch, 1, torch.zeros(1, 128).cuda(), None, None, edge_term=term, sigmoid_gate=True)
    with pytest.raises(NotImplementedError):
        ops.gat_aggregate(batch, 1, torch.zeros(1, 128).cuda(), None, None, edge_term=term, heads=2)
    with pytest.raises(NotImplementedError):
        ops.gat_aggregate(batch, 1, torch.zeros(1, 128).cuda(), None, None, edge_term=term, dropout=(0.1, word))
    with pytest.raises(ValueError):
        ops.edge_logit_term(batches('ladder_mini'), 1, torch.zeros(batch.dg.schema.NR, 3).cuda())       # a graph without attributes
