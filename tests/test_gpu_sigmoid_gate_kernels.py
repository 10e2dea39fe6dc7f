"""-m gpu: the sigmoid-gate instantiations of the aggregate kernels (KGW_F_SIGMOID_GATE: k_agg_fwd<RAW, GATE>, k_agg_bwd_dst<GATE>,
with the unchanged combines, k_agg_bwd_src, riders and k_duv_fold behind them) through ops.gat_aggregate(sigmoid_gate=True), against
the float64 restatement of tests/sigmoid_gate_ref.py, output by output.

The graphs are the `batches` of tests/test_gpu_aggregate_parity.py: its degree ladder realises every branch of the dst-major kernels
(test_degree_ladder_realises_every_branch there: rows of 0 .. 9 in-edges, both sides of 32 / 64 / 128 -- the 2 / 4 / 8 group forms, the
64-edge block, the chunk --, hub rows of 2, 3 and 8 chunks for the combine kernels, and the mini-batch with hop-pruned rows).

What is compared, per case: Z, the per-edge logit e_edge, stat == (0, 1) on visited rows (zero elsewhere), dH, dU, dV and the
logit_bias gradient.  Tolerances: the project's fp32 bound (assert_close with the parity file's RTOL / ATOL; 2e-5 for dH and 1e-4
for dU / dV / d logit_bias, as there).  Every output holds that bound on every case, hub rows included, so the parity file's
other rule (within 2 x the float32 oracle's error, _check_residue) is used for none of them."""
import pytest
import torch

from tests import sigmoid_gate_ref as R
from tests.helpers import assert_close
from tests.test_gpu_aggregate_parity import ATOL, RTOL, _hub_edge, _inputs, batches, ladder, layer_edges  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


def _run_gpu(batch, layer, H, U, V, kap, G, slope=0.2, temp=1.0, relu_input=False):
    from kgwas_amd import ops
    m, sc = batch.meta, batch.dg.schema
    z_rows = int(m.z_base[layer - 1][sc.NT])
    n_edges = int(m.n_edges[layer - 1])
    Hd, Ud, Vd = (t.cuda().requires_grad_(True) for t in (H, U, V))
    kd = kap.cuda().requires_grad_(True) if kap is not None else None
    Z, stat, e_edge = ops.gat_aggregate(batch, layer, Hd, Ud, Vd, neg_slope=slope, temperature=temp, relu_input=relu_input,
                                        logit_bias=kd, sigmoid_gate=True)
    (Z * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    return dict(Z=Z.detach().cpu(), stat=stat[:z_rows].cpu(), e=e_edge[:n_edges].cpu(), dH=Hd.grad.cpu(), dU=Ud.grad.cpu(),
                dV=Vd.grad.cpu(), dlb=kd.grad.cpu() if kd is not None else None)


def check_case(batch, layer, seed, slope=0.2, temp=1.0, relu_input=False, lbias=False, u_scale=0.2, v_scale=0.2, spike=None):
    sc, dg = batch.dg.schema, batch.dg
    H, U, V, kap, G = _inputs(batch, layer, seed, relu_input, lbias, u_scale, v_scale)
    if spike is not None:          # (H row, relation r): its logit on r becomes 3 |u_r|^2
        j, r = spike
        H[j] = 3.0 * U[r]
    edges = layer_edges(batch, layer)
    got = _run_gpu(batch, layer, H, U, V, kap, G, slope, temp, relu_input)
    ref = R.gated_grads(batch, layer, H, U, V, kap, G, torch.float64, slope, temp, relu_input, edges)
    live = [r for r in range(sc.NR) if dg.kg.rel_live[layer - 1][r]]
    dead = [r for r in range(sc.NR) if not dg.kg.rel_live[layer - 1][r]]
    eid = torch.cat([edges[r][0] for r in edges])
    assert eid.numel() > 0
    for k, v in got.items():
        assert v is None or bool(torch.isfinite(v).all()), k
    assert_close(got['Z'], ref['Z'], RTOL, ATOL, 'Z')
    assert_close(got['e'][eid], ref['e'][eid], RTOL, ATOL, 'e_edge')
    # stat: exactly (0, 1) on every visited row, exactly zero on the others (never written), as are their Z rows
    assert torch.equal(got['stat'].double(), ref['stat']), 'stat: (0, 1) on rows with edges, zero elsewhere'
    empty = ref['stat'][:, 1] == 0
    assert bool(empty.any()) and float(got['Z'][empty].abs().sum()) == 0.0
    if relu_input:
        assert bool((H == 0).any()) and float(got['dH'][H == 0].abs().max()) == 0.0
    assert_close(got['dH'], ref['dH'], RTOL, 2e-5, 'dH')
    assert_close(got['dU'][live], ref['dU'][live], RTOL, 1e-4, 'dU')
    assert_close(got['dV'][live], ref['dV'][live], RTOL, 1e-4, 'dV')
    assert float(got['dU'][dead].abs().sum()) == 0.0 and float(got['dV'][dead].abs().sum()) == 0.0
    if lbias:
        assert_close(got['dlb'][live], ref['dlb'][live], RTOL, 1e-4, 'dlb')
        assert float(got['dlb'][dead].abs().sum()) == 0.0
    return got, ref


GRAPHS = [('ladder_full', 1), ('ladder_full', 2), ('ladder_mini', 1), ('ladder_mini', 2), ('small_mini', 1), ('small_mini', 2),
          ('edge_full', 1), ('edge_full', 2)]


@pytest.mark.parametrize('lbias', [False, True], ids=['lb0', 'lb1'])
@pytest.mark.parametrize('relu_input', [False, True], ids=['relu0', 'relu1'])
@pytest.mark.parametrize('graph,layer', GRAPHS, ids=[f'{g}-L{l}' for g, l in GRAPHS])
def test_parity_sweep(batches, graph, layer, relu_input, lbias):
    """Every graph, both layers, relu_input off / on, logit_bias off / on.  A gated hub row is a sum of hundreds of terms, not a
    convex combination: Z and the gradients are compared with assert_close's bound, whose rel_to_max term scales with the largest
    entry of the reference -- the sum's round-off scales the same way."""
    check_case(batches(graph), layer, seed=1000 + 100 * layer + 2 * relu_input + lbias, relu_input=relu_input, lbias=lbias)


def test_gates_are_not_a_softmax(batches):
    """A softmax row is a convex combination of rows of H, so its norm cannot exceed the largest row norm of H; the gated hub
    row (1000 terms with gates around 1/2: a norm of about sqrt(1000) / 2 row norms) does, several times over."""
    from kgwas_amd import ops
    batch = batches('ladder_full')
    H, U, V, _, _ = _inputs(batch, 1, seed=5)
    Zg, _, _ = ops.gat_aggregate(batch, 1, H.cuda(), U.cuda(), V.cuda(), sigmoid_gate=True)
    Zs, _, _ = ops.gat_aggregate(batch, 1, H.cuda(), U.cuda(), V.cuda())
    hmax = float(H.norm(dim=1).max())
    assert float(Zs.norm(dim=1).max()) <= hmax * (1 + 1e-5)
    assert float(Zg.norm(dim=1).max()) > 4.0 * hmax


@pytest.mark.parametrize('slope', [0.05, 0.5])
@pytest.mark.parametrize('temp', [0.5, 2.5])
def test_other_slopes_and_temperatures(batches, slope, temp):
    check_case(batches('ladder_full'), 1, seed=31, slope=slope, temp=temp, lbias=True)


def test_saturation(batches):
    """Logits beyond +-100: in fp32 the gate is exactly 1 above e / T ~ 16.7 and exactly 0 below ~ -88.7 (the exponential
    overflows to +inf and 1 / inf = 0).  Every output stays finite, Z is within tolerance, and the gradients -- g (1 - g) = 0 on
    the saturated edges, in float64 below 4e-44 -- are within tolerance of the float64 ones."""
    got, ref = check_case(batches('ladder_full'), 1, seed=41, u_scale=20.0, v_scale=20.0, lbias=True)
    assert float(ref['e'].min()) < -100.0 and float(ref['e'].max()) > 100.0
    sat = (ref['e'].abs() > 100.0)
    assert float(sat.double().mean()) > 0.2
    assert float(ref['g'][ref['e'] > 100.0].min()) == 1.0 and float(ref['g'][ref['e'] < -100.0].max()) < 1e-43


@pytest.mark.parametrize('graph', ['ladder_full', 'ladder_mini'])
def test_spike_in_a_late_chunk_of_the_hub_row(batches, graph):
    """The construction of the parity file's spike case: one source of the 1000-edge row gets a logit ~35 x the others' in its fifth
    chunk.  Under the gate nothing rescales: the edge saturates at 1 and the other chunks' partial sums are added as they are."""
    batch = batches(graph)
    e, j, r = _hub_edge(batch, 1)
    got, ref = check_case(batch, 1, seed=9, u_scale=1.0, v_scale=0.1, spike=(j, r), lbias=True)
    assert float(ref['g'][e]) > 0.999999 and float(ref['e'][e]) > 100.0


def test_deterministic(batches):
    """No atomics: two runs of forward and backward give the same bits."""
    batch = batches('ladder_mini')
    H, U, V, kap, G = _inputs(batch, 1, seed=3, lbias=True)
    a = _run_gpu(batch, 1, H, U, V, kap, G, relu_input=False)
    b = _run_gpu(batch, 1, H, U, V, kap, G, relu_input=False)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    batch = batches('ladder_full')
    H, U, V, kap, G = _inputs(batch, 2, seed=4, relu_input=True, lbias=True)
    a = _run_gpu(batch, 2, H, U, V, kap, G, relu_input=True)
    b = _run_gpu(batch, 2, H, U, V, kap, G, relu_input=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_zbuf_route(batches):
    """``zbuf``: a caller's zeroed workspace gives the bits of the call that allocates its own."""
    from kgwas_amd import ops
    batch = batches('ladder_mini')
    H, U, V, _, G = _inputs(batch, 1, seed=6)
    Hc, Uc, Vc = H.cuda(), U.cuda(), V.cuda()
    ws = ops.aggregate_workspace(batch, 1, 'cuda:0').zero_()
    Za, sa, ea = ops.gat_aggregate(batch, 1, Hc, Uc, Vc, sigmoid_gate=True)
    Zb, sb, eb = ops.gat_aggregate(batch, 1, Hc, Uc, Vc, sigmoid_gate=True, zbuf=ws)
    assert torch.equal(Za, Zb) and torch.equal(sa[:Za.shape[0]], sb[:Za.shape[0]]) and torch.equal(ea, eb)


def test_refusals(batches):
    from kgwas_amd import ops
    batch = batches('ladder_mini')
    H, U, V, _, _ = _inputs(batch, 1, seed=2)
    Hc, Uc, Vc = H.cuda(), U.cuda(), V.cuda()
    word = torch.zeros(1, dtype=torch.int64, device='cuda')
    with pytest.raises(ValueError, match='raw_weights'):
        ops.gat_aggregate(batch, 1, Hc, Uc, Vc, sigmoid_gate=True, raw_weights=True)
    for NH in (2, 4):
        with pytest.raises(NotImplementedError, match='heads'):
            ops.gat_aggregate(batch, 1, Hc, Uc.expand(NH, -1, -1).contiguous(), Vc.expand(NH, -1, -1).contiguous(), sigmoid_gate=True,
                              heads=NH)
    with pytest.raises(NotImplementedError, match='dropout'):
        ops.gat_aggregate(batch, 1, Hc, Uc, Vc, sigmoid_gate=True, dropout=(0.1, word))
    import copy
    import types
    sharded = copy.copy(batch)             # (the fixture's batch is shared: the exchange goes on a shallow copy)
    sharded.exchange = types.SimpleNamespace()
    with pytest.raises(NotImplementedError, match='SNP-sharded'):
        ops.gat_aggregate(sharded, 1, Hc, Uc, Vc, sigmoid_gate=True)
    assert batch.exchange is None
