"""-m gpu: the aggregate kernels with NH = 2 and 4 heads (KgwLayerArgs.n_heads; kgw_aggregate_heads.h: k_agg_fwd_heads / _combine,
k_agg_bwd_dst_heads / _combine, k_agg_bwd_src_heads with its rider blocks, k_duv_fold_heads) against the float64 restatement of the
planes contract (tests/multihead_ref.py), plane by plane, on the degree ladder of tests/test_gpu_aggregate_parity.py: 3000 SNPs,
256 genes, in-degrees on both sides of 8 ... 384, one 1000-edge row, a two-chunk hub, dead relations -- the smallest graph on which
every branch of these kernels runs (64-edge blocks, groups of 8 with tails of 4 and 2 in both halves, 128-edge chunks, segments of
2, 3 and more than 4 chunks, the combine launches, source rows of 1 to ~270 entries, padding-free and hop-pruned layouts).

Tolerances as tests/test_gpu_aggregate_parity.py, for fp32 kernels against float64: rtol 1e-4, atol 1e-5 (dH 2e-5, dU / dV 1e-4)
plus assert_close's rel_to_max 1e-5.  dH and dV carry d a_dst, a cancellation residue wherever a row's logits sit on one branch of
the leaky ReLU: where they miss the element-wise bound they must lie within 2 x the error of the same restatement run in float32."""
import ctypes as C

import pytest
import torch

from tests import multihead_ref as R
from tests.helpers import assert_close, segment_alpha_sums
from tests.test_gpu_aggregate_parity import (ATOL, RTOL, _check_residue, batches, ladder, layer_edges,  # noqa: F401
                                             realised_structure)

pytestmark = pytest.mark.gpu

CH = 128
GRAPHS = [('ladder_full', 1), ('ladder_mini', 1), ('ladder_mini', 2)]
GRAPH_IDS = [f'{g}-L{l}' for g, l in GRAPHS]


def _inputs(batch, layer, NH, seed, relu_input=False):
    m, sc = batch.meta, batch.dg.schema
    g = torch.Generator().manual_seed(seed)
    n_src = int(m.src_base[layer - 1][sc.NT])
    z_rows = int(m.z_base[layer - 1][sc.NT])
    H = torch.randn(n_src, CH, generator=g)
    if relu_input:
        H = torch.relu(H)
    U = torch.randn(NH, sc.NR, CH, generator=g) * 0.2
    V = torch.randn(NH, sc.NR, CH, generator=g) * 0.2
    G = torch.randn(NH, z_rows, CH, generator=g)
    return H, U, V, G


def _run_gpu(batch, layer, H, U, V, G, relu_input=False):
    from kgwas_amd import ops
    NH = U.shape[0]
    Hd, Ud, Vd = (t.cuda().requires_grad_(True) for t in (H, U, V))
    Z, stat, e_edge = ops.gat_aggregate(batch, layer, Hd, Ud, Vd, relu_input=relu_input, heads=NH)
    (Z * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    return dict(Z=Z.detach().cpu(), stat=stat.cpu(), e=e_edge.cpu(), dH=Hd.grad.cpu(), dU=Ud.grad.cpu(), dV=Vd.grad.cpu())


_REF = {}


def _reference(batches, graph, layer, NH, relu_input):
    """(inputs, edges, float64 restatement) of a case: computed once, shared by the tests that need it, never modified."""
    key = (graph, layer, NH, relu_input)
    if key not in _REF:
        batch = batches(graph)
        inp = _inputs(batch, layer, NH, seed=1000 * NH + 10 * layer + int(relu_input), relu_input=relu_input)
        edges = layer_edges(batch, layer)
        _REF[key] = (inp, edges, R.planes_grads(batch, layer, *inp, torch.float64, relu_input=relu_input, edges=edges))
    return _REF[key]


@pytest.mark.parametrize('relu_input', [False, True], ids=['plain', 'relu'])
@pytest.mark.parametrize('NH', [2, 4])
@pytest.mark.parametrize('graph,layer', GRAPHS, ids=GRAPH_IDS)
def test_every_plane_against_float64(batches, graph, layer, NH, relu_input):
    batch = batches(graph)
    sc, dg = batch.dg.schema, batch.dg
    if graph == 'ladder_full':          # every branch of the chunk loops and the combine launches is on this layer
        s = realised_structure(batch, layer)
        assert s['hn_mod8'] == set(range(8)) and {1, 2, 3} <= s['nch'] and s['max_nch'] > 4 and s['single_128']
    (H, U, V, G), edges, ref = _reference(batches, graph, layer, NH, relu_input)
    got = _run_gpu(batch, layer, H, U, V, G, relu_input)
    cache = {}

    def lazy32():
        if not cache:
            cache.update(R.planes_grads(batch, layer, H, U, V, G, torch.float32, relu_input=relu_input, edges=edges))
        return cache

    live = [r for r in range(sc.NR) if dg.kg.rel_live[layer - 1][r]]
    dead = [r for r in range(sc.NR) if not dg.kg.rel_live[layer - 1][r]]
    eid = torch.cat([edges[r][0] for r in edges])
    assert eid.numel() > 0
    empty = torch.ones(got['Z'].shape[1], dtype=torch.bool)
    for r, (_, _, dst) in edges.items():
        d = int(sc.dst_type[r])
        empty[int(batch.meta.z_base[layer - 1][d]) + dst * int(sc.R_dst[d]) + int(sc.slot_dst[r])] = False
    assert bool(empty.any())
    for h in range(NH):
        for k, atol in (('Z', ATOL), ('stat', ATOL)):
            print(f'head {h} {k}: max abs err {float((got[k][h].double() - ref[k][h]).abs().max()):.3e}, max |ref| {float(ref[k][h].abs().max()):.3e}')
            assert_close(got[k][h], ref[k][h], RTOL, atol, f'{k}[{h}]')
        assert_close(got['e'][h][eid], ref['e'][h][eid], RTOL, ATOL, f'e_edge[{h}]')
        # rows without an edge (degree 0, dead relations) are never written: exactly zero
        assert float(got['Z'][h][empty].abs().sum()) == 0.0 and float(got['stat'][h][empty].abs().sum()) == 0.0
        # alpha^h recomputed on the host from (stat, e_edge) sums to one over every non-empty segment
        zrow_of_edge = torch.zeros(got['e'].shape[1], dtype=torch.long)
        for r, (e_ids, _, dst) in edges.items():
            d = int(sc.dst_type[r])
            zrow_of_edge[e_ids] = int(batch.meta.z_base[layer - 1][d]) + dst * int(sc.R_dst[d]) + int(sc.slot_dst[r])
        st = got['stat'][h].double()
        alpha = torch.zeros(got['e'].shape[1], dtype=torch.float64)
        alpha[eid] = torch.exp(got['e'][h][eid].double() - st[zrow_of_edge[eid], 0]) / st[zrow_of_edge[eid], 1]
        sums = segment_alpha_sums(batch, layer, alpha)
        assert sums.numel() > 0 and float((sums - 1.0).abs().max()) <= 1e-5, float((sums - 1.0).abs().max())
        assert_close(alpha[eid], ref['alpha'][h][eid], RTOL, ATOL, f'alpha[{h}]')
        print(f'head {h} dU: max abs err {float((got["dU"][h][live].double() - ref["dU"][h][live]).abs().max()):.3e}')
        assert_close(got['dU'][h][live], ref['dU'][h][live], RTOL, 1e-4, f'dU[{h}]')
        _check_residue('dV', got['dV'][h][live], ref['dV'][h][live], lambda h=h: {'dV': lazy32()['dV'][h][live]}, 1e-4)
        # dead relations get exactly zero gradient
        assert float(got['dU'][h][dead].abs().sum()) == 0.0 and float(got['dV'][h][dead].abs().sum()) == 0.0
    # the heads are different functions (the planes are not copies of one another)
    assert float((ref['Z'][0] - ref['Z'][1]).abs().max()) > 1e-2
    if relu_input:
        assert bool((H == 0).any()) and float(got['dH'][H == 0].abs().max()) == 0.0
    print(f'dH: max abs err {float((got["dH"].double() - ref["dH"]).abs().max()):.3e}, max |ref| {float(ref["dH"].abs().max()):.3e}')
    _check_residue('dH', got['dH'], ref['dH'], lazy32, 2e-5)


def _call_abi(batch, layer, H, U, V, n_heads):
    """One forward through the C ABI with ``n_heads`` given as is and single-plane buffers (n_heads <= 1)."""
    from kgwas_amd import _lib, ops
    m, sc = batch.meta, batch.dg.schema
    z_rows, n_edges, n_chunks = int(m.z_base[layer - 1][sc.NT]), int(m.n_edges[layer - 1]), int(m.n_chunks[layer - 1])
    Z = torch.zeros(z_rows, CH, device='cuda')
    stat = torch.zeros(z_rows, 2, device='cuda')
    e = torch.zeros(n_edges, device='cuda')
    part = torch.zeros(n_chunks * _lib.PART_STRIDE, device='cuda')
    a = ops._layer_args(batch, layer, 0.2, 1.0)
    a.n_heads = n_heads
    Hd, Ud, Vd = H.cuda(), U.cuda().contiguous(), V.cuda().contiguous()
    a.H, a.U, a.V, a.Z, a.stat, a.e_edge, a.part = (t.data_ptr() for t in (Hd, Ud, Vd, Z, stat, e, part))
    _lib.check(_lib.lib().kgw_gat_aggregate_fwd(C.byref(a), _lib.stream_ptr()), 'kgw_gat_aggregate_fwd')
    torch.cuda.synchronize()
    return Z.cpu(), stat.cpu(), e.cpu()


def test_one_head_is_the_call_without_the_field(batches):
    """n_heads = 1 runs the kernels n_heads = 0 runs: the same bits, and a head plane of an NH = 2 call is that function too."""
    batch = batches('ladder_mini')
    H, U, V, G = _inputs(batch, 1, 2, seed=77)
    a = _call_abi(batch, 1, H, U[0], V[0], 0)
    b = _call_abi(batch, 1, H, U[0], V[0], 1)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[0].abs().sum()) > 0
    got = _run_gpu(batch, 1, H, U, V, G)
    assert_close(got['Z'][0], a[0], RTOL, ATOL, 'plane 0 of NH = 2 against the single-head kernels')


def test_reruns_are_bit_identical(batches):
    """No atomics: two runs of the same NH = 4 call, forward and backward, give the same bits."""
    batch = batches('ladder_full')
    H, U, V, G = _inputs(batch, 1, 4, seed=78, relu_input=True)
    a = _run_gpu(batch, 1, H, U, V, G, relu_input=True)
    b = _run_gpu(batch, 1, H, U, V, G, relu_input=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a['dV'].abs().sum()) > 0


def test_refused_combinations_leave_z_untouched(batches):
    """Every combination include/kgwas_hip.h refuses returns its code before any launch: a sentinel-filled Z stays as it is."""
    from kgwas_amd import _lib, ops
    batch = batches('ladder_mini')
    layer = 1
    m, sc = batch.meta, batch.dg.schema
    z_rows, n_edges, n_chunks = int(m.z_base[layer - 1][sc.NT]), int(m.n_edges[layer - 1]), int(m.n_chunks[layer - 1])
    n_src = int(m.src_base[layer - 1][sc.NT])
    NH = 2
    H, U, V, G = _inputs(batch, layer, NH, seed=79)
    dev = 'cuda'
    Hd, Ud, Vd, Gd = H.to(dev), U.to(dev), V.to(dev), G.to(dev)
    Z = torch.full((NH, z_rows, CH), 7.5, device=dev)
    bufs = dict(stat=torch.zeros(NH, z_rows, 2, device=dev), e_edge=torch.zeros(NH, n_edges, device=dev),
                part=torch.zeros(NH * n_chunks * _lib.PART_STRIDE, device=dev), adp=torch.zeros(NH, n_edges, 2, device=dev),
                da_dst=torch.zeros(NH, z_rows, device=dev), part_da=torch.zeros(NH * n_chunks * 4, device=dev),
                dH=torch.full((n_src, CH), 7.5, device=dev), part_du=torch.zeros(NH * n_chunks, CH, device=dev),
                duv_ws=torch.zeros(NH * 2 * sc.NR * 8 * CH, device=dev), dU=torch.zeros(NH, sc.NR, CH, device=dev),
                dV=torch.zeros(NH, sc.NR, CH, device=dev))
    spare = torch.zeros(max(z_rows, n_src) * 2 * ((sc.NR + 3) & ~3), device=dev)
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    L = _lib.lib()

    def args(n_heads=NH):
        a = ops._layer_args(batch, layer, 0.2, 1.0)
        a.n_heads = n_heads
        a.H, a.U, a.V, a.Z, a.dZ = Hd.data_ptr(), Ud.data_ptr(), Vd.data_ptr(), Z.data_ptr(), Gd.data_ptr()
        for k, t in bufs.items():
            setattr(a, k, t.data_ptr())
        a.seg_chptr = batch.buf.seg_chptr.data_ptr()
        return a

    calls = (L.kgw_gat_aggregate_fwd, L.kgw_gat_aggregate_bwd_dst, L.kgw_gat_aggregate_bwd_src)
    for bad in (3, 5, 8, -1):
        for fn in calls:
            assert fn(C.byref(args(bad)), _lib.stream_ptr()) == -2, bad                       # KGW_E_RANGE
    unsupported = []
    a = args(); a.flags = 1; unsupported.append(a)                                            # KGW_F_RAW_WEIGHTS
    a = args(); a.partial_rels = 1; unsupported.append(a)
    a = args(); a.drop_word_dev, a.drop_thresh, a.drop_scale = word.data_ptr(), 1 << 31, 2.0; unsupported.append(a)
    a = args(); a.logit_bias = spare.data_ptr(); unsupported.append(a)
    a = args(); a.V = None; a.a_dst = spare.data_ptr(); unsupported.append(a)                 # a_dst without V
    a = args(); a.da_src = spare.data_ptr(); a.dU = None; a.dV = None; unsupported.append(a)  # da_src without the dU / dV route
    for a in unsupported:
        for fn in calls:
            assert fn(C.byref(a), _lib.stream_ptr()) == _lib.KGW_E_UNSUPPORTED
    alpha = torch.zeros(n_edges, device=dev)
    assert L.kgw_edge_alpha(C.byref(args()), C.c_void_p(alpha.data_ptr()), _lib.stream_ptr()) == _lib.KGW_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((Z == 7.5).all()) and bool((bufs['dH'] == 7.5).all()) and float(bufs['stat'].abs().sum()) == 0.0
    with pytest.raises(NotImplementedError):
        ops.gat_aggregate(batch, layer, Hd, Ud, Vd, heads=3)
    with pytest.raises(NotImplementedError):
        ops.gat_aggregate(batch, layer, Hd, Ud, Vd, heads=2, raw_weights=True)
    with pytest.raises(NotImplementedError):
        ops.gat_aggregate(batch, layer, Hd, Ud, Vd, heads=2, logit_bias=spare[:sc.NR])
    # ... and the accepted call on the same buffers runs
    a = args()
    Z.zero_()
    assert L.kgw_gat_aggregate_fwd(C.byref(a), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert float(Z.abs().sum()) > 0
