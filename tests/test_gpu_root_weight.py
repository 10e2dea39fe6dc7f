"""-m gpu: the root weight of the message-passing layers (kgw_root_linear_fwd / _bwd, ops.root_linear,
HeteroGNN(gnn_root_weight=True)) up to KGWAS.train().

The kernels at the C ABI against float64 (tests/root_weight_ref.py).  Every error is taken relative to sum |x||w| + |y| of the
element's own dot product (sum |gm||w| for dx), as tests/test_gpu_mlp2_kernels.py does, and held to that file's bar for an fp32-pipe
product (the kernel is one fp32 MFMA chain over k, as kgw_linear): no worse than 1.25 x ORDER x the fp32 device product of the same
operands or 4 u, and never above max(16 u, its chain ceiling for the number of elements compared).  ops.linear -- the kgw_linear the
kernel imitates -- is measured on the same inputs against the same float64 and printed beside it
(profiles/root_weight/gputests.txt keeps the figures).  Masks are exact: (out > 0) of an ``out`` GIVEN at the C ABI and (x > 0).
The model against the float64 RootedOracle at tests/test_gpu_layer_norm.py's bars (RTOL, ATOL, max(ATOL, 1e-4 max|ref|) for
gradients, plus assert_close's rel_to_max); the trainer bit for bit against the body it captured issued eagerly."""
import os
import re

import numpy as np
import pytest
import torch

from tests import hidden_dropout_ref as HD
from tests import root_weight_ref as R
from tests.helpers import assert_close, batch_cpu, grads_by_name, launches_of_one_step, oracle_from_product, params_by_name
from tests.test_gpu_aggregate_parity import layer_edges
from tests.test_gpu_mlp2_kernels import ORDER, U, _chain_ceiling

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5                  # tests/test_gpu_layer_norm.py's
C = R.C
NT = 8
BS = 48
TILE = 32                                # rows of one MFMA tile; a block takes two tiles (64 rows) until the grid cap doubles that
CAP_ROWS = 2048 * 2 * TILE               # rows above which 2 tiles per block no longer fit 2048 blocks: the tile loop runs
OK, E_NULL, E_RANGE, E_UNSUPPORTED = 0, -1, -2, -3


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _weights(cl, seed):
    """[8, 128, 128], [out, in], the padding zero (the model keeps it zero)."""
    w = _rand((NT, C, C), seed, 0.2)
    w[:, cl:, :] = 0.0
    w[:, :, cl:] = 0.0
    return w


def _rows(n, cl, seed, scale=1.0):
    t = _rand((n, C), seed, scale)
    t[:, cl:] = 0.0
    return t


def _dev(t, strided, fill=None):
    """``t`` on the device -- ``strided``: as columns 128 .. 255 of a [rows, 256] matrix whose other half holds -3."""
    if not strided:
        return (t.cuda() if fill is None else torch.full(t.shape, fill, device='cuda:0')), None
    wide = torch.full((t.shape[0], 256), -3.0, device='cuda:0')
    wide[:, 128:] = t.cuda() if fill is None else fill
    return wide[:, 128:], wide


def _fwd(cases, W, relu, strided=False):
    """kgw_root_linear_fwd over ``cases`` = [(type, x, y)] (CPU): the destinations, on the CPU."""
    from kgwas_amd import _lib
    Wd = W.cuda()
    jobs = (_lib.KgwRootJob * len(cases))()
    keep = []
    for j, (t, x, y) in zip(jobs, cases):
        n = x.shape[0]
        (xd, xw), (yd, yw), (dd, dw) = _dev(x, strided), _dev(y, False), _dev(y, strided, float('nan'))
        j.x, j.ldx, j.y, j.ldy, j.dst, j.ldd = xd.data_ptr(), xd.stride(0) if n else 128, yd.data_ptr(), 128, dd.data_ptr(), dd.stride(0) if n else 128
        j.rows, j.type, j.W = n, t, Wd[t].data_ptr()
        keep.append((xd, yd, dd, xw, dw, xd.clone(), yd.clone()))
    assert _lib.lib().kgw_root_linear_fwd(len(cases), jobs, int(relu), _lib.stream_ptr()) == OK
    torch.cuda.synchronize()
    for xd, yd, dd, xw, dw, x0, y0 in keep:
        assert torch.equal(xd, x0) and torch.equal(yd, y0)                       # x and y are only read
        for wide in (xw, dw):
            assert wide is None or bool((wide[:, :128] == -3.0).all())           # the columns beside a strided operand too
    return [k[2].cpu() for k in keep]


def _bwd(cases, W, with_out, x_premasked, strided=False):
    """kgw_root_linear_bwd over ``cases`` = [(type, g, out, x)] (CPU): per case (dx, gm or None), on the CPU."""
    from kgwas_amd import _lib
    Wd = W.cuda()
    jobs = (_lib.KgwRootBwdJob * len(cases))()
    keep = []
    for j, (t, g, out, x) in zip(jobs, cases):
        n = g.shape[0]
        (gd, _), (od, _), (xd, _) = _dev(g, False), _dev(out, strided), _dev(x, False)
        (dxd, dxw), (gmd, gmw) = _dev(g, strided, float('nan')), _dev(g, False, float('nan'))
        j.g, j.ldg, j.dx, j.lddx = gd.data_ptr(), 128, dxd.data_ptr(), dxd.stride(0) if n else 128
        if with_out:
            j.out, j.ldo, j.gm, j.ldgm = od.data_ptr(), od.stride(0) if n else 128, gmd.data_ptr(), 128
        if x_premasked:
            j.x, j.ldx = xd.data_ptr(), 128
        j.rows, j.type, j.W, j.x_premasked = n, t, Wd[t].data_ptr(), int(x_premasked)
        keep.append((gd, od, xd, dxd, gmd, dxw, gd.clone()))
    assert _lib.lib().kgw_root_linear_bwd(len(cases), jobs, _lib.stream_ptr()) == OK
    torch.cuda.synchronize()
    res = []
    for gd, od, xd, dxd, gmd, dxw, g0 in keep:
        assert torch.equal(gd, g0)                                               # g is only read
        assert dxw is None or bool((dxw[:, :128] == -3.0).all())
        if not with_out:
            assert bool(torch.isnan(gmd).all())                                  # nothing to mask: gm is not written
        res.append((dxd.cpu(), gmd.cpu() if with_out else None))
    return res


def _errors(what, ours, a, Wop, add=None, post=None):
    """max |ours - float64| / (sum |a||w| + |add|) for ours = post(add + a @ Wop) -- beside it the same figure of the fp32 device
    product (torch) and of ops.linear (kgw_linear) on the same operands -- and the bar of tests/test_gpu_mlp2_kernels.py for an
    fp32-pipe product.  ``post``: an exact 1-Lipschitz map applied to all three and to the reference (the ReLU, a given mask)."""
    from kgwas_amd import ops
    if ours.numel() == 0:
        return
    post = post or (lambda t: t)
    a64, w64 = a.double(), Wop.double()
    ref = a64 @ w64
    scale = a64.abs() @ w64.abs()
    if add is not None:
        ref, scale = ref + add.double(), scale + add.double().abs()
    scale = scale.clamp_min(1e-30)
    ref = post(ref)
    ad, wd = a.cuda(), Wop.cuda().contiguous()
    t32 = ad @ wd
    k32 = ops.linear(ad, wd, w_kn=True)
    if add is not None:
        t32, k32 = t32 + add.cuda(), k32 + add.cuda()
    e = float(((ours.double() - ref).abs() / scale).max())
    e32 = float(((post(t32.cpu().double()) - ref).abs() / scale).max())
    ek = float(((post(k32.cpu().double()) - ref).abs() / scale).max())
    ceiling = max(16 * U, _chain_ceiling(ours.numel()))
    print(f'[root {what}] ours {e / U:.3f} u, fp32 device product {e32 / U:.3f} u, ops.linear {ek / U:.3f} u '
          f'(u = 2^-24, relative to sum |a||w|; ceiling {ceiling / U:.1f} u)')
    assert e <= max(1.25 * ORDER * e32, 4 * U), (what, e, e32)
    assert e <= ceiling, (what, e, ceiling)


def _check_case(t, x, y, g, W, cl, label, strided=False, others=()):
    """Forward with and without the ReLU and the four backward variants of one job (``others``: further jobs of the same launches,
    [(type, x, y, g)]), against float64; the pad columns exactly 0."""
    jobs = [(t, x, y, g)] + list(others)
    for relu in (True, False):
        outs = _fwd([(tt, xx, yy) for tt, xx, yy, _ in jobs], W, relu, strided)
        for (tt, xx, yy, gg), out in zip(jobs, outs):
            assert out.shape == yy.shape and bool(torch.isfinite(out).all())
            assert float(out[:, cl:].abs().sum()) == 0.0
            _errors(f'{label} type {tt} fwd relu={int(relu)}', out, xx, W[tt].t(), add=yy, post=torch.relu if relu else None)
            if relu and xx.shape[0] >= 8 and cl >= 4:
                assert 0.2 < float((out[:, :cl] > 0).float().mean()) < 0.8       # the ReLU both opens and closes
        if relu:
            saved = outs
    for with_out in (True, False):
        for xp in (False, True):
            res = _bwd([(tt, gg, oo, xx) for (tt, xx, yy, gg), oo in zip(jobs, saved)], W, with_out, xp, strided)
            for (tt, xx, yy, gg), oo, (dx, gm) in zip(jobs, saved, res):
                gm64, dx64, _ = R.backward(gg.double(), oo.double(), xx.double(), W[tt].double(), masked=not with_out, x_premasked=xp)
                assert bool(torch.isfinite(dx).all()) and float(dx[:, cl:].abs().sum()) == 0.0
                if with_out:
                    assert torch.equal(gm.double(), gm64)                        # a selection: exact
                xmask = (xx > 0).double()
                _errors(f'{label} type {tt} dx out={int(with_out)} x_premasked={int(xp)}', dx, gm64.float(), W[tt],
                        post=(lambda v, m=xmask: v * m) if xp else None)
                assert_close(dx, dx64, RTOL, ATOL, f'{label} dx')


SHAPES = [(rows, cl) for rows in (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 257) for cl in (128, 100, 4, 1)] + [(CAP_ROWS + 33, 128)]


@pytest.mark.parametrize('rows,cl', SHAPES)
def test_kernels_equal_float64(rows, cl):
    """One job at every row count where the mapping changes -- none, one row, a partial / full / overfull 32-row tile, a partial
    / full / overfull two-tile block, several blocks, and more than 2 tiles x 2048 blocks (the blocks walk their tiles in a loop)
    -- at every width class; forward with and without the ReLU, backward with ``out`` given and NULL, ``x_premasked`` on and off."""
    W = _weights(cl, 5)
    x, y, g = _rows(rows, cl, 7 + rows), _rows(rows, cl, 9 + rows), _rows(rows, cl, 11 + rows)
    if rows > CAP_ROWS:
        x = x.abs() * (torch.arange(rows).unsqueeze(1) % 2 * 2 - 1)              # (x > 0 opens and closes by row as well)
    _check_case(3, x, y, g, W, cl, f'rows {rows} cl {cl}')


@pytest.mark.parametrize('n_jobs', [1, 5, 8])
def test_several_jobs_in_one_launch(n_jobs):
    """Distinct node types, row counts and weights per job, one job empty when there are several; strided x, dst, out and dx
    (leading dimension 256) whose neighbouring columns stay untouched."""
    counts = [37, 1, 0, 300, 8, 129, 5, 64][:n_jobs] if n_jobs > 1 else [37]
    types = [5, 0, 7, 2, 1, 6, 3, 4][:n_jobs]
    for cl, strided in ((128, False), (100, True)):
        W = _weights(cl, 21)
        jobs = [(t, _rows(n, cl, 100 + k), _rows(n, cl, 200 + k), _rows(n, cl, 300 + k)) for k, (t, n) in enumerate(zip(types, counts))]
        _check_case(*jobs[0], W, cl, f'{n_jobs} jobs cl {cl}', strided=strided, others=jobs[1:])
        if n_jobs > 1:                                                           # the weights are the type's own
            a = _fwd([(types[0], jobs[0][1], jobs[0][2])], W, True)[0]
            b = _fwd([(types[3], jobs[0][1], jobs[0][2])], W, True)[0]
            assert not torch.equal(a, b)


def test_two_runs_give_equal_bits():
    """dst, dx and gm of two runs over five jobs (several blocks each, one of them past the grid cap's first doubling): equal
    bits -- and the bits of a job do not depend on what else is in the launch (the grid changes, the sums do not)."""
    counts, types, cl = [1000, 37, 0, 4500, 129], [5, 0, 7, 2, 1], 100
    W = _weights(cl, 51)
    jobs = [(t, _rows(n, cl, 400 + k), _rows(n, cl, 500 + k), _rows(n, cl, 600 + k)) for k, (t, n) in enumerate(zip(types, counts))]
    f1 = _fwd([(t, x, y) for t, x, y, _ in jobs], W, True)
    f2 = _fwd([(t, x, y) for t, x, y, _ in jobs], W, True)
    assert all(torch.equal(a, b) for a, b in zip(f1, f2)) and float(f1[0].abs().sum()) > 0
    b1 = _bwd([(t, g, o, x) for (t, x, y, g), o in zip(jobs, f1)], W, True, True)
    b2 = _bwd([(t, g, o, x) for (t, x, y, g), o in zip(jobs, f1)], W, True, True)
    for (d1, m1), (d2, m2) in zip(b1, b2):
        assert torch.equal(d1, d2) and torch.equal(m1, m2)
    alone = _fwd([(jobs[3][0], jobs[3][1], jobs[3][2])], W, True)[0]
    assert torch.equal(alone, f1[3])
    alone_b = _bwd([(jobs[3][0], jobs[3][3], f1[3], jobs[3][1])], W, True, True)[0]
    assert torch.equal(alone_b[0], b1[3][0])


def test_refusals_launch_nothing():
    """Every listed refusal with DEVICE pointers: the status, and the destination still holds what it held."""
    from kgwas_amd import _lib
    L = _lib.lib()
    dev = 'cuda:0'
    x, y, W = torch.randn(8, C, device=dev), torch.randn(8, C, device=dev), torch.randn(C, C, device=dev)
    dst = torch.full((8, C), 7.0, device=dev)
    wide = torch.zeros(8, 130, device=dev)

    def fjob(rows=8, x=x.data_ptr(), y=y.data_ptr(), dst=dst.data_ptr(), ldx=128, ldy=128, ldd=128, t=0, W=W.data_ptr()):
        j = _lib.KgwRootJob()
        j.x, j.ldx, j.y, j.ldy, j.dst, j.ldd, j.rows, j.type, j.W = x, ldx, y, ldy, dst, ldd, rows, t, W
        return j

    def fwd(jobs, n=None):
        arr = (_lib.KgwRootJob * max(1, len(jobs)))(*jobs)
        return L.kgw_root_linear_fwd(len(jobs) if n is None else n, arr, 1, _lib.stream_ptr())

    cases = [([fjob(x=None)], E_NULL), ([fjob(y=None)], E_NULL), ([fjob(dst=None)], E_NULL), ([fjob(W=None)], E_NULL),
             ([fjob()] * 8 + [fjob()], E_RANGE), ([fjob(rows=-1)], E_RANGE), ([fjob(rows=(1 << 25) + 1)], E_RANGE),
             ([fjob(ldx=124)], E_RANGE), ([fjob(ldy=64)], E_RANGE), ([fjob(ldd=127)], E_RANGE), ([fjob(t=8)], E_RANGE),
             ([fjob(t=-1)], E_RANGE), ([fjob(t=1), fjob(t=1)], E_RANGE),
             ([fjob(x=x.data_ptr() + 4)], E_UNSUPPORTED), ([fjob(dst=dst.data_ptr() + 8)], E_UNSUPPORTED),
             ([fjob(W=W.data_ptr() + 4)], E_UNSUPPORTED), ([fjob(x=wide.data_ptr(), ldx=130)], E_UNSUPPORTED),
             ([fjob(dst=y.data_ptr())], E_UNSUPPORTED), ([fjob(dst=x.data_ptr())], E_UNSUPPORTED),
             ([fjob(t=2), fjob(t=3, ldd=130)], E_UNSUPPORTED)]
    assert L.kgw_root_linear_fwd(1, None, 1, _lib.stream_ptr()) == E_NULL and fwd([fjob()], n=0) == E_RANGE
    x0, y0 = x.clone(), y.clone()
    for jobs, status in cases:
        assert fwd(jobs) == status, (status, [(j.rows, j.type, j.ldx, j.ldy, j.ldd) for j in jobs])
    g, out = torch.randn(8, C, device=dev), torch.randn(8, C, device=dev)
    dx, gm = torch.full((8, C), 7.0, device=dev), torch.full((8, C), 7.0, device=dev)

    def bjob(rows=8, g=g.data_ptr(), out=out.data_ptr(), x=x.data_ptr(), gm=gm.data_ptr(), dx=dx.data_ptr(), t=0, W=W.data_ptr(), ld=128,
             xp=1):
        j = _lib.KgwRootBwdJob()
        j.g, j.ldg, j.out, j.ldo, j.x, j.ldx, j.gm, j.ldgm, j.dx, j.lddx = g, ld, out, ld, x, ld, gm, ld, dx, ld
        j.rows, j.type, j.W, j.x_premasked = rows, t, W, xp
        return j

    def bwd(jobs, n=None):
        arr = (_lib.KgwRootBwdJob * max(1, len(jobs)))(*jobs)
        return L.kgw_root_linear_bwd(len(jobs) if n is None else n, arr, _lib.stream_ptr())

    bcases = [([bjob(g=None)], E_NULL), ([bjob(dx=None)], E_NULL), ([bjob(W=None)], E_NULL), ([bjob(x=None)], E_NULL),
              ([bjob()] * 9, E_RANGE), ([bjob(rows=-1)], E_RANGE), ([bjob(rows=(1 << 25) + 1)], E_RANGE), ([bjob(ld=124)], E_RANGE),
              ([bjob(t=8)], E_RANGE), ([bjob(t=4), bjob(t=4)], E_RANGE),
              ([bjob(g=g.data_ptr() + 4)], E_UNSUPPORTED), ([bjob(out=out.data_ptr() + 4)], E_UNSUPPORTED),
              ([bjob(dx=dx.data_ptr() + 8)], E_UNSUPPORTED), ([bjob(ld=130)], E_UNSUPPORTED), ([bjob(dx=g.data_ptr())], E_UNSUPPORTED),
              ([bjob(gm=g.data_ptr())], E_UNSUPPORTED), ([bjob(dx=out.data_ptr())], E_UNSUPPORTED),
              ([bjob(gm=out.data_ptr())], E_UNSUPPORTED), ([bjob(gm=dx.data_ptr())], E_UNSUPPORTED),
              ([bjob(dx=x.data_ptr())], E_UNSUPPORTED), ([bjob(gm=x.data_ptr())], E_UNSUPPORTED)]
    assert L.kgw_root_linear_bwd(1, None, _lib.stream_ptr()) == E_NULL and bwd([bjob()], n=0) == E_RANGE
    g0 = g.clone()
    for jobs, status in bcases:
        assert bwd(jobs) == status, status
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()) and bool((dx == 7.0).all()) and bool((gm == 7.0).all())
    assert torch.equal(x, x0) and torch.equal(y, y0) and torch.equal(g, g0) and bool((wide == 0).all())
    # ... and no rows at all is KGW_OK without a launch, whatever the pointers
    assert fwd([fjob(rows=0, x=None, y=None, dst=None, W=None)]) == OK and bwd([bjob(rows=0, g=None, dx=None, W=None, x=None)]) == OK
    # the accepted call, for contrast, writes
    assert fwd([fjob()]) == OK and bwd([bjob()]) == OK
    torch.cuda.synchronize()
    assert not bool((dst == 7.0).any()) and not bool((gm == 7.0).all())


@pytest.mark.parametrize('blocks', [False, True], ids=['temporaries', 'out_blocks'])
def test_ops_forward_and_backward(blocks):
    """ops.root_linear over three types: a block written in place of the next layer's input, the inputs left alone, a None
    gradient passed through, the packed gradient with zero slices for the types that got none; every masking mode against the
    float64 rule."""
    from kgwas_amd import ops
    cl, types, counts = 100, [4, 0, 2], [33, 260, 5]
    W = _weights(cl, 61)
    ys = [_rows(n, cl, 70 + k) for k, n in enumerate(counts)]
    xs = [_rows(n, cl, 75 + k).abs() * (1 - 2 * (torch.arange(C) % 3 == 0).float()) for k, n in enumerate(counts)]
    gs_ = [_rows(n, cl, 80 + k) for k, n in enumerate(counts)]
    for premasked, relu, xp in ((False, True, False), (True, True, True), (True, False, False), (False, True, True)):
        Wd = W.cuda().requires_grad_(True)
        ly = [y.cuda().requires_grad_(True) for y in ys]
        lx = [x.cuda().requires_grad_(True) for x in xs]
        buf = torch.zeros(300, C, device='cuda:0')
        ob = [None, ops.RowBlock(buf, 16, 260), ops.RowBlock(buf, 0, 7)] if blocks else None      # (the last one does not fit)
        outs = ops.root_linear(ly, types, lx, Wd, ob, premasked=premasked, relu=relu, x_premasked=xp)
        if blocks:
            assert outs[1].data_ptr() == buf[16:].data_ptr() and outs[2].data_ptr() != buf.data_ptr()
        masked = premasked or not relu
        ups = [g.cuda() * (o.detach() > 0) if (premasked and relu) else g.cuda() for g, o in zip(gs_, outs)]
        torch.autograd.backward([outs[0], outs[1]], [ups[0], ups[1]])               # (the third output has no gradient)
        torch.cuda.synchronize()
        assert ly[2].grad is None and lx[2].grad is None
        for t in range(NT):
            if t not in (4, 0):
                assert float(Wd.grad[t].abs().sum()) == 0.0                          # zero slices, not None
        for k in (0, 1):
            t = types[k]
            assert torch.equal(ly[k].detach().cpu(), ys[k]) and torch.equal(lx[k].detach().cpu(), xs[k])
            o64 = R.forward(ys[k].double(), xs[k].double(), W[t].double(), relu)
            assert_close(outs[k], o64, RTOL, ATOL, f'ops out {k}')
            dy64, dx64, dW64 = R.backward(ups[k].cpu().double(), outs[k].detach().cpu().double(), xs[k].double(), W[t].double(),
                                          masked=masked, x_premasked=xp)
            assert_close(ly[k].grad, dy64, RTOL, ATOL, f'ops dy {k}')
            assert_close(lx[k].grad, dx64, RTOL, ATOL, f'ops dx {k}')
            assert_close(Wd.grad[t], dW64, RTOL, max(ATOL, 1e-4 * float(dW64.abs().max())), f'ops dW type {t}')
            assert float(Wd.grad[t, cl:, :].abs().sum()) == 0.0 == float(Wd.grad[t, :, cl:].abs().sum())
    with pytest.raises(AssertionError):
        ops.root_linear(ly, [4, 4, 2], lx, Wd)
    with pytest.raises(AssertionError):
        ops.root_linear(ly, types, lx[:2], Wd)


# ------------------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------------------
ROUTES = {
    'gat-sum': dict(aggr='sum'),
    'gat-mean': dict(aggr='mean'),                 # (the 1 / R scales the relation part only)
    'gat-heads2': dict(aggr='sum', heads=2),
    'gat-min': dict(aggr='min'),                   # (the root term is added after the reduction)
    'gat-max': dict(aggr='max'),
    'gat-sum-width100': dict(aggr='sum', hidden=100),
    'gat-3layers': dict(aggr='sum', layers=3),
    'gat-1layer': dict(aggr='sum', layers=1),
    'gat-sigmoid': dict(aggr='sum', sigmoid=True),
    'gat-edge-dim': dict(aggr='sum', edge_dim=3),
}
ATTR_RELS = ['ABC', 'eQTL', 'PCHi-C', 'Gene-Signaling-Gene', 'Gene-Reaction-Gene', 'Gene-Associates-BiologicalProcess']


@pytest.fixture(scope='module')
def small_attr_kg(tmp_path_factory):
    """conftest's small_kg with 3-wide edge attributes on ATTR_RELS and their mirrors (tests/test_gpu_edge_attr_model.py's)."""
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.01, seed=1, feat_dims={'Gene': 96}, data_path=str(tmp_path_factory.mktemp('root_eattr')),
                                     edge_dim=3, edge_attr_relations=ATTR_RELS)


def _model(kg, route, root=True, norm=None, p=0.0, seed=3, lin_bias=0.5):
    from kgwas_amd.model import HeteroGNN
    r = ROUTES[route]
    torch.manual_seed(seed)
    dims = (kg.snp_init_dim_size, kg.gene_init_dim_size, kg.go_init_dim_size)
    cl = r.get('hidden', 128)
    model = HeteroGNN(kg.data, cl, 1, r.get('layers', 2), 'GAT', r['aggr'], *dims, r.get('heads', 1), gat_split_heads=True,
                      gat_sigmoid=r.get('sigmoid', False), gat_edge_dim=r.get('edge_dim'), gnn_dropout=p, gnn_norm=norm,
                      gnn_root_weight=root).cuda()
    with torch.no_grad():
        for pack in list(model.live_packs) + list(model.dead_packs):
            # ('min': the minimum over a gene's ~17 relations is negative in nearly every channel; the biases are raised to keep the
            #  ReLU behind it open, as tests/test_gpu_edge_attr_model.py does)
            pack.bias[:, :cl].normal_(0, 0.1).add_(1.0 if r['aggr'] == 'min' else 0.0)
        model.lin.bias.fill_(lin_bias)       # (an open read-out ReLU for most seeds: every parameter gets a gradient)
        for w, b in zip(model.norm_weight, model.norm_bias):
            live = (w != 0).float()
            w.add_(torch.randn_like(w) * 0.3 * live)
            b.add_(torch.randn_like(b) * 0.2 * live)
    return model


def _builder(model):
    if model.heads > 1:
        from tests.multihead_ref import oracle_with_heads
        return oracle_with_heads
    if model.gat_sigmoid:
        from tests.sigmoid_gate_ref import gated_oracle
        return gated_oracle
    if model.edge_dim is not None:
        from tests.edge_attr_ref import oracle_from_product as with_attrs
        return with_attrs
    return oracle_from_product


def _oracle(model, state_factor=None):
    return R.rooted_oracle(model, _builder(model), state_factor)


def _batch(kg, layers=2):
    from kgwas_amd.sampler import NeighborLoader
    ids = np.random.default_rng(0).choice(kg.data['SNP'].x.shape[0], size=BS, replace=False)
    return next(iter(NeighborLoader(kg.data, [-1] * layers, ('SNP', ids), batch_size=BS, device='cuda:0', seed=5)))


def _labels(kg):
    g = torch.Generator().manual_seed(9)
    n = kg.data['SNP'].x.shape[0]
    return kg.data['SNP'].y.cuda(), (torch.rand(n, generator=g, dtype=torch.float64) + 0.5).cuda()


def _cpu_inputs(model, batch):
    if model.edge_dim is not None:
        from tests.edge_attr_ref import batch_cpu as with_attrs
        return with_attrs(batch)
    return batch_cpu(batch) + (None,)


def _against_oracle(model, oracle, batch, y_all, w_all, route, word=None):
    """forward_loss + backward and forward in training mode against ``oracle``: predictions, loss and every gradient."""
    from kgwas_amd import ops
    model.train()
    if word is not None:
        model.set_dropout_word(word)
    model.zero_grad(set_to_none=True)
    n_id = batch.n_id('SNP')
    loss, pred = model.forward_loss(batch.x_dict, batch.edge_index_dict, BS, n_id, y_all, w_all, unit_grad=True)
    loss.backward(gradient=ops.unit_gradient(loss.device))
    with torch.no_grad():
        out = model(batch.x_dict, batch.edge_index_dict, BS)
    x, ei, ea = _cpu_inputs(model, batch)
    out_o = oracle(x, ei, BS, edge_attr_dict=ea).reshape(-1)
    ids = n_id[:BS].long().cpu()
    yy, ww = y_all.cpu().double()[ids], w_all.cpu().double()[ids]
    loss_o = torch.mean(ww * (out_o - yy) ** 2)
    loss_o.backward()
    print(f'{route}: pred max abs err {float((pred.detach().cpu().double().reshape(-1) - out_o.detach()).abs().max()):.3e}, '
          f'max |ref| {float(out_o.detach().abs().max()):.3e}; loss {float(loss.detach()):.9f} vs {float(loss_o.detach()):.9f}')
    assert float((out_o.detach() > 0).double().mean()) > 0.5, 'most seeds must sit on the open side of the read-out ReLU'
    assert_close(pred.reshape(-1), out_o.detach(), RTOL, ATOL, 'pred (forward_loss)')
    assert_close(out.reshape(-1), out_o.detach(), RTOL, ATOL, 'pred (forward)')
    assert_close(loss.detach(), loss_o.detach(), RTOL, ATOL, 'loss')
    go = grads_by_name(oracle)
    go.update(oracle.norm_grads())
    go.update(oracle.root_grads())
    n_live = n_root = 0
    for name, g in grads_by_name(model).items():
        ref = go[name]
        if g is None:
            assert ref is None or float(ref.abs().max()) == 0.0, f'{name}: product has no grad, oracle has'
            continue
        if ref is None:                       # (a slice of a type without rows in the layer: zeros, where the oracle has None)
            assert name.startswith(('norms.', 'roots.')) and float(g.abs().max()) == 0.0, name
            continue
        n_live += 1
        if name.startswith('roots.'):
            n_root += float(ref.abs().max()) > 0
            print(f'{name}: max abs err {float((g.double() - ref).abs().max()):.3e}, max |ref| {float(ref.abs().max()):.3e}')
        assert tuple(g.shape) == tuple(ref.shape), (name, g.shape, ref.shape)
        assert_close(g, ref, RTOL, max(ATOL, 1e-4 * float(ref.abs().max())), f'grad {name}')
    assert n_live > 10 and n_root >= model.num_layers, (n_live, n_root)
    return out_o.detach(), x, ei, ea


@pytest.mark.parametrize('route', list(ROUTES))
def test_model_matches_the_rooted_oracle(small_kg, small_attr_kg, route):
    """Per route: the training forward, the loss and every gradient (the roots' among them), the evaluation forward and
    return_h, against the float64 oracle; the oracle without its roots is another function; the attention queries see the root
    term; layer 1 runs unfolded."""
    kg = small_attr_kg if route == 'gat-edge-dim' else small_kg
    model = _model(kg, route)
    L = model.num_layers
    assert len(model.root_weight) == L and model.gnn_root_weight
    # FC_output would get gradient from the fold and from the root product of layer 1: the fused optimiser's records hold one
    # source per tensor, so a root model runs layer 1 unfolded (Open) -- the documented opposite of the fold
    assert not model.fold_fc
    batch = _batch(kg, L)
    y_all, w_all = _labels(kg)
    oracle = _oracle(model)
    out_o, x, ei, ea = _against_oracle(model, oracle, batch, y_all, w_all, route)
    model.eval()                             # the root term is live in evaluation: the same function
    with torch.no_grad():
        a = model(batch.x_dict, batch.edge_index_dict, BS)
        a2, h = model(batch.x_dict, batch.edge_index_dict, BS, return_h=True)
        _, h_o = oracle(x, ei, BS, return_h=True, edge_attr_dict=ea)
        diff = float((oracle.without_roots()(x, ei, BS, edge_attr_dict=ea).reshape(-1) - out_o).abs().max())
    assert_close(a.reshape(-1), out_o, RTOL, ATOL, 'pred (eval)')
    assert torch.equal(a, a2)
    assert_close(h, h_o, RTOL, ATOL, 'h (eval, return_h)')
    print(f'{route}: the oracle without roots differs by {diff:.3e}')
    assert diff > 1e-3
    if route in ('gat-sum', 'gat-sum-width100', 'gat-3layers'):                  # single-head sum: the attention queries
        with torch.no_grad():
            out_att, att = model(batch.x_dict, batch.edge_index_dict, BS, return_attention_weights=True)
            per_edge = [t.clone() for t in model.last_attention]
            hot = model.hot_path_attention(batch)
        assert len(att) == L == len(hot)
        assert_close(out_att.reshape(-1), out_o, RTOL, ATOL, 'pred (all-relations route)')
        twin = _model(kg, route, root=False)
        twin.load_state_dict({k: v for k, v in model.state_dict().items() if not k.startswith('roots.')})
        twin.eval()
        with torch.no_grad():
            twin(batch.x_dict, batch.edge_index_dict, BS, return_attention_weights=True)
            hot_t = twin.hot_path_attention(batch)
        # layer 1 reads the feature MLPs' output, root or not; layer 2 reads a state the root term is in.  (The twin's hot path runs
        # layer 1 folded, another summation order: close, not equal.)
        assert torch.equal(per_edge[0], twin.last_attention[0])
        assert_close(hot[0], hot_t[0], RTOL, ATOL, 'layer-1 attention of the twin')
        assert not torch.allclose(per_edge[1], twin.last_attention[1], rtol=1e-3, atol=1e-6)
        assert not torch.allclose(hot[1], hot_t[1], rtol=1e-3, atol=1e-6)
        with torch.no_grad():
            oa = oracle.attention_means(x, ei)
            o_att = oracle.attention(x, ei)
        for k in range(L):
            assert_close(att[k], oa[k], RTOL, ATOL, f'mean attention layer {k + 1}')
        # ... and per edge against the oracle's values (a mean of softmax weights is rows / edges whatever the state): every edge the
        # training path aggregates, by (local source, local destination) of its relation (the all-relations route's per-edge values
        # are pinned through the export: test_network_weight_export_of_a_root_model)
        n_hot = 0
        for k in range(L):
            hk = hot[k].cpu().double()
            for r, (e, src, dst) in layer_edges(batch, k + 1).items():
                et = model.edge_types[r]
                ref = dict(zip((ei[et][0] * (1 << 32) + ei[et][1]).tolist(), o_att[k][et].reshape(-1).tolist()))
                want = torch.tensor([ref[q] for q in (src * (1 << 32) + dst).tolist()], dtype=torch.float64)
                assert_close(hk[e], want, RTOL, ATOL, f'hot-path attention layer {k + 1} {et}')
                n_hot += e.numel()
        assert n_hot > 100, n_hot


@pytest.mark.parametrize('route', ['gat-sum', 'gat-heads2', 'gat-3layers', 'gat-min'])
def test_root_with_norm_and_hidden_dropout(small_kg, route):
    """conv + root -> norm -> ReLU -> dropout, p = 0.3: layer 2's root term reads the DROPPED state, and on the fused and
    multi-head routes its dx is multiplied by (x > 0) inside the kernel (``x_premasked``: the producers of x run premasked).
    Against the oracle with all three, gradients included -- a wrong flag shows in every gradient upstream of layer 2."""
    p, word = 0.3, HD.dropout_word(5, 1, 2)
    model = _model(small_kg, route, norm='layer', p=p, lin_bias=1.5)    # (normed states: a read-out bias of 0.5 leaves half the seeds closed)
    batch = _batch(small_kg, model.num_layers)
    y_all, w_all = _labels(small_kg)
    fac, n_dropped = HD.state_factors(model, batch, word, p)
    assert n_dropped > 100 and len(model.norm_weight) == model.num_layers - 1
    _against_oracle(model, _oracle(model, fac), batch, y_all, w_all, f'{route} + norm + dropout', word=word)


def test_root_with_hidden_dropout_alone(small_kg):
    """Without a norm the root launch applies the ReLU itself and is the premasked producer of the dropped state."""
    p, word = 0.3, HD.dropout_word(7, 0, 1)
    model = _model(small_kg, 'gat-sum', p=p)
    batch = _batch(small_kg)
    fac, n_dropped = HD.state_factors(model, batch, word, p)
    assert n_dropped > 100
    _against_oracle(model, _oracle(model, fac), batch, *_labels(small_kg), 'gat-sum + dropout', word=word)


# ------------------------------------------------------------------------------------------------------------------------------
# trainer
# ------------------------------------------------------------------------------------------------------------------------------
def _launches_of_one_step(gs):
    """Kernel launches of one training step issued eagerly through the body the trainer captured (tests/helpers.py):
    (all, sorted names of the k_root_linear* among them, number of k_tn_gemm* / k_tn_reduce*)."""
    names = launches_of_one_step(gs)
    root = sorted(re.search(r'k_root_linear<\w+>|k_root_linear\w*', n).group(0) for n in names if 'k_root_linear' in n)
    return len(names), root, sum(1 for n in names if 'k_tn_gemm' in n or 'k_tn_reduce' in n), names


def _trainer(kg, bs, n, seed=7, **kw):
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    ids = np.asarray(kg.train_input_nodes[1][:bs * n])
    run = KGWAS(kg, device='cuda:0', seed=seed)
    run.initialize_model(**kw)
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)
    run.model.train()
    return run, GraphTrainStep(run, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=seed)


def test_the_default_model_is_unchanged(tiny_kg):
    """gnn_root_weight left out or False: the same launches of the eager step (none of them k_root_linear), no ``roots.`` key,
    the folded route and the fused optimiser launch, and the same loss and parameter bits after two captured steps."""
    res = {}
    for what, kw in (('left out', {}), ('False', dict(gnn_root_weight=False))):
        run, gs = _trainer(tiny_kg, 32, 2, **kw)
        assert gs.fused_adam and run.model.fold_fc and not gs.root_weight
        assert not any(k.startswith('roots.') for k in run.model.state_dict()) and 'gnn_root_weight' not in run.config
        n, root, n_tn, names = _launches_of_one_step(gs)
        print(f'gnn_root_weight {what}: {n} kernel launches, k_root_linear: {root}')
        assert root == [] and n > 10
        run, gs = _trainer(tiny_kg, 32, 2, **kw)                                  # (a fresh trainer: the count above took a step)
        losses = [gs.step(i).detach().clone() for i in range(2)]
        gs.check()
        res[what] = (n, sorted(names), losses, params_by_name(run.model))
    a, b = res['left out'], res['False']
    assert a[0] == b[0] and a[1] == b[1]
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and sorted(a[3]) == sorted(b[3])
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3])


# What DESIGN.md section 8 says the feature adds to one eager step of a two-layer model: per layer k_root_linear<false> in the
# forward and k_root_linear<true> in the backward (4); per layer the weight-gradient products' launch (kgw_tn_gemm_multi: k_tn_gemm,
# and k_tn_reduce behind it only when a product has more than one 256-row block -- none has on the tiny graph: 2, the benchmark
# step: 4); and the framework's launches: one zero fill of the packed d W_root per layer, and per layer and destination type the
# addition of dx to the dH of the same state (an add; before it, where the destination rows are a proper prefix of the type's
# rows, a zero fill and a device-to-device memcpy, which is no kernel) -- 2 + #prefixes fills and #pairs adds, asserted exactly.  Nothing else: the rest of the difference to the DEFAULT step is the unfolded layer 1 -- the route a
# gat_sigmoid model takes, which is what the root step is compared with here.
ROOT_LAUNCHES = ['k_root_linear<false>', 'k_root_linear<false>', 'k_root_linear<true>', 'k_root_linear<true>']
ROOT_TN_LAUNCHES = 2


def test_the_feature_adds_its_launches_and_nothing_of_its_own_elsewhere(tiny_kg):
    """The root model's eager step against the step of a model on the same (unfolded) route without it -- a gated model with and
    without the root weight: exactly the two forward and two backward root launches and the weight-gradient launches of a
    two-layer model, plus the framework's zero fills and additions of dx to dH, counted exactly from the batch's layout; the default step holds
    none of the new kernels."""
    counts = {}
    for what, kw in (('default', {}), ('gated', dict(gat_sigmoid=True)), ('gated + root', dict(gat_sigmoid=True, gnn_root_weight=True)),
                     ('root', dict(gnn_root_weight=True))):
        run, gs = _trainer(tiny_kg, 32, 2, **kw)
        assert gs.fused_adam and gs.root_weight == ('root' in what) and run.model.fold_fc == (what == 'default')
        n, root, n_tn, names = _launches_of_one_step(gs)
        counts[what] = (n, root, n_tn, names)
        m = gs.meta
        nt = len(run.model.node_types)
        pairs = sum(1 for l in range(2) for t in range(nt) if int(m.lay_rows[l][t]))
        # a type's layer input: every row of it the layer reads (layer 1: the feature MLP's output), later the previous layer's output
        rows_in = [[int(m.lay_src[0][t]) for t in range(nt)], [int(m.lay_rows[0][t]) for t in range(nt)]]
        prefix = sum(1 for l in range(2) for t in range(nt) if 0 < int(m.lay_rows[l][t]) < rows_in[l][t])
        print('lay_rows', [[int(m.lay_rows[l][t]) for t in range(nt)] for l in range(2)], 'input rows', rows_in)
        print(f'{what}: {n} kernel launches, k_root_linear: {root}, k_tn_*: {n_tn}; (layer, destination type) pairs: {pairs}')
    assert counts['default'][1] == [] and counts['gated'][1] == []
    for what in ('gated + root', 'root'):
        assert [re.sub(r'\s', '', n) for n in counts[what][1]] == ROOT_LAUNCHES, counts[what][1]
    extra = sorted(set(counts['gated + root'][3]) - set(counts['gated'][3]))
    print('kernels of the root step that the same route without it does not have:', extra)
    own = [n for n in extra if re.search(r'\bk_[a-z]', n)]
    assert all('k_root_linear' in n for n in own), own                          # nothing else of the package's own
    assert counts['gated + root'][2] == counts['gated'][2] + ROOT_TN_LAUNCHES
    from collections import Counter
    diff = Counter(counts['gated + root'][3]) - Counter(counts['gated'][3])
    fills = sum(v for k, v in diff.items() if 'FillFunctor' in k)
    adds = sum(v for k, v in diff.items() if 'CUDAFunctor_add' in k)
    print(f'(layer, type) pairs {pairs}, of them proper prefixes {prefix}; framework launches added: {fills} zero fills, {adds} adds')
    # exactly: one zero fill of the packed d W_root per layer and one per proper-prefix pair (autograd's slice backward; its copy of
    # dx into the zeros is a device-to-device memcpy, not a kernel), one add of dx to dH per pair -- and nothing else
    assert fills == 2 + prefix and adds == pairs and prefix >= 1
    assert counts['gated + root'][0] == counts['gated'][0] + len(ROOT_LAUNCHES) + ROOT_TN_LAUNCHES + fills + adds
    assert counts['root'][0] == counts['gated + root'][0]                        # (the gate itself costs no launch)


def test_captured_step_equals_eager_step_bit_for_bit(tiny_kg):
    """Three steps of GraphTrainStep against three eager steps of the same launches (a second trainer on its own copy of the model,
    stepped through the body the first one captured): every loss, every parameter and both moments of every parameter afterwards
    -- the roots' too -- bit for bit.  The step keeps the fused optimiser launch, and the root weights move while their padding and
    the slices of types without relations stay zero."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    bs, nsteps, seed = 32, 3, 11
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * nsteps])
    runs = []
    for _ in range(2):
        run = KGWAS(tiny_kg, device='cuda:0', seed=seed)
        run.initialize_model(gnn_root_weight=True, gnn_hidden_dim=100)
        runs.append(run)
    run_g, run_c = runs
    with torch.no_grad():
        run_g.model.lin.bias.fill_(0.5)
    run_c.model.load_state_dict(run_g.model.state_dict())
    p0 = params_by_name(run_g.model)
    for m in (run_g.model, run_c.model):
        m.train()
    gs = GraphTrainStep(run_g, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=seed)
    gc = GraphTrainStep(run_c, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=seed)
    assert gs.root_weight and gs.fused_adam and not run_g.model.fold_fc and gs.n_batches == nsteps
    for n, p in params_by_name(run_g.model).items():
        assert torch.equal(p, p0[n]), n                       # (the capture's warm-up steps were undone)
    for step in range(nsteps):
        lg = gs.step(step).detach().clone()
        gc._sample_now(step % 2, step)
        torch.cuda.synchronize()
        lc = gc._step_body(step % 2).detach().clone()
        torch.cuda.synchronize()
        print(f'step {step}: captured {float(lg):.9f} same launches eagerly {float(lc):.9f}')
        assert torch.equal(lg, lc) and bool(torch.isfinite(lg)), (step, float(lg), float(lc))
        pg, pc = params_by_name(run_g.model), params_by_name(run_c.model)
        assert all(torch.equal(pg[n], pc[n]) for n in pg), [n for n in pg if not torch.equal(pg[n], pc[n])][:5]
    gs.check()
    assert gs.fused_adam and gc.fused_adam
    n_state = 0
    for (ng, a), (nc, b) in zip(run_g.model.named_parameters(), run_c.model.named_parameters()):
        sa, sb = gs.opt.state.get(a), gc.opt.state.get(b)
        assert ng == nc and (sa is None) == (sb is None), ng
        if sa is not None:
            n_state += 1
            assert torch.equal(sa['exp_avg'], sb['exp_avg']) and torch.equal(sa['exp_avg_sq'], sb['exp_avg_sq']), ng
    assert n_state >= 20
    moved = [n for n in pg if n.startswith('roots.') and float((pg[n] - p0[n]).abs().max()) > 0]
    assert len(moved) >= 2 * 2, moved
    for p in run_g.model.root_weight:
        w, m1 = p.detach(), gs.opt.state[p]['exp_avg']
        dead = [t for t in range(w.shape[0]) if t not in run_g.model.root_types]
        assert float(w[dead].abs().sum()) == 0.0 and float(w[:, 100:, :].abs().sum()) == 0.0 == float(w[:, :, 100:].abs().sum())
        assert float(m1[dead].abs().sum()) == 0.0 and float(m1[:, 100:, :].abs().sum()) == 0.0 == float(m1[:, :, 100:].abs().sum())


@pytest.mark.parametrize('case', ['plain', 'fanout-shuffle-dropouts-norm', 'eager-mean'])
def test_train_two_epochs_end_to_end(tiny_kg, case, monkeypatch):
    """KGWAS.train(epoch=2) with a root model -- the captured step (alone; beside a finite fan-out, a shuffled order, both
    dropouts and the norm) or the eager loop on the relation mean: finite losses, a saved checkpoint, a reload that predicts the
    same bits, and evaluate_minibatch_clean through the captured evaluation graph equal to the eager forward."""
    from kgwas_amd.utils import evaluate_minibatch_clean
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    run = KGWAS(tiny_kg, device='cuda:0', seed=3)
    kw = {'plain': {}, 'fanout-shuffle-dropouts-norm': dict(gnn_dropout=0.2, gat_dropout=0.1, gnn_norm='layer'),
          'eager-mean': dict(gnn_aggr='mean')}[case]
    run.initialize_model(gnn_root_weight=True, **kw)
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)
    w0 = [w.detach().clone() for w in run.model.root_weight]
    name = 'root_weight_e2e_' + case
    tkw = {'plain': {}, 'fanout-shuffle-dropouts-norm': dict(num_neighbors=[10, 5], shuffle=True), 'eager-mean': dict(use_graph=False)}[case]
    run.train(batch_size=32, epoch=2, save_best_model=True, save_name=name, **tkw)
    assert np.isfinite(run.val_metrics['mse']) and np.isfinite(run.val_metrics['pearsonr'])
    assert run.config['gnn_root_weight'] is True and run.kgwas_res is not None and len(run.kgwas_res) > 0
    assert all(not torch.equal(w.detach(), a) for w, a in zip(run.model.root_weight, w0))       # the roots were trained
    assert all(bool(torch.isfinite(w).all()) for w in run.model.root_weight)
    assert os.path.exists(os.path.join(tiny_kg.data_path, 'model', name, 'config.pkl'))
    run2 = KGWAS(tiny_kg, device='cuda:0', seed=4)
    run2.load_pretrained(os.path.join(tiny_kg.data_path, 'model', name))
    assert run2.config == run.config and run2.model.gnn_root_weight
    sa, sb = run.best_model.state_dict(), run2.model.state_dict()
    assert list(sa) == list(sb) and any(k.startswith('roots.') for k in sa)
    ids = np.asarray(tiny_kg.val_input_nodes[1][:64])
    batch = next(iter(NeighborLoader(tiny_kg.data, [-1, -1], ('SNP', ids), batch_size=64, device='cuda:0')))
    run.best_model.eval(); run2.model.eval()
    with torch.no_grad():
        a = run.best_model(batch.x_dict, batch.edge_index_dict, 64)
        b = run2.model(batch.x_dict, batch.edge_index_dict, 64)
    assert torch.equal(a, b) and float(a.abs().sum()) > 0
    # the captured evaluation graph computes the root model's function (tests/test_gpu_graph.py's bars: the graph runs all
    # nodes as one batch, the eager loop the loader's batches)
    ids = np.asarray(tiny_kg.val_input_nodes[1])[:64 * 2 + 17]
    mk = lambda: NeighborLoader(tiny_kg.data, [-1, -1], ('SNP', ids), batch_size=64, drop_last=False, device='cuda:0')
    loader = mk()
    res = evaluate_minibatch_clean(loader, run2.model, 'cuda:0')
    assert loader.__dict__.get('_graph_eval', {}).get(id(run2.model)), 'the captured evaluation graph was not used'
    monkeypatch.setenv('KGW_EVAL_EAGER', '1')
    eager = evaluate_minibatch_clean(mk(), run2.model, 'cuda:0')
    assert res['pred'].shape == eager['pred'].shape == (len(ids),) and float(np.abs(eager['pred']).sum()) > 0
    np.testing.assert_allclose(res['pred'], eager['pred'], rtol=1e-5, atol=1e-6)


def test_network_weight_export_of_a_root_model(small_kg):
    """KGWAS.get_network_weight() of a root model: per edge the all-relations route's raw weights with the root term in the state
    between the layers (no ReLU there, like the reference's export), against the float64 oracle's export procedure; layer 2's
    table differs from the same weights without the roots."""
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(small_kg, device='cuda:0', seed=5)
    run.initialize_model(gnn_root_weight=True)
    m = run.model
    with torch.no_grad():
        for pack in list(m.live_packs) + list(m.dead_packs):
            pack.bias.uniform_(-0.1, 0.1)
    run.best_model = m
    df = run.get_network_weight()
    assert set(df.layer.unique()) == {'l1', 'l2'}
    g = small_kg.data
    o = R.rooted_oracle(m, oracle_from_product)
    with torch.no_grad():
        x = {t: g[t].x.double() for t in g.node_types}
        ei = {et: g[et].edge_index for et in g.edge_types}
        atts = o.export_attention(x, ei)
    n_checked = 0
    for k, att in enumerate(atts):
        for et, a in att.items():
            sub = df[(df.layer == f'l{k + 1}') & (df.h_type == et[0]) & (df.rel_type == et[1]) & (df.t_type == et[2])]
            e = ei[et].numpy()
            key_ref = e[0].astype(np.int64) * (1 << 32) + e[1]               # (duplicate pairs are dropped: compare on unique ones)
            _, first = np.unique(key_ref, return_index=True)
            ref = dict(zip(key_ref[first].tolist(), a.reshape(-1).numpy()[first].tolist()))
            key_my = sub.h_idx.values.astype(np.int64) * (1 << 32) + sub.t_idx.values.astype(np.int64)
            assert len(key_my) == len(ref) and set(key_my.tolist()) == set(ref)
            assert_close(torch.tensor(sub.weight.values), torch.tensor([ref[q] for q in key_my.tolist()]), 2e-4, 1e-5,
                         f'raw attention l{k + 1} {et}', rel_to_max=1e-5)
            n_checked += len(ref)
    assert n_checked > 0
    run0 = KGWAS(small_kg, device='cuda:0', seed=5)
    run0.initialize_model()
    run0.model.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith('roots.')})
    run0.best_model = run0.model
    df0 = run0.get_network_weight()
    assert np.array_equal(df[df.layer == 'l1'].weight.values, df0[df0.layer == 'l1'].weight.values)
    assert not np.allclose(df[df.layer == 'l2'].weight.values, df0[df0.layer == 'l2'].weight.values, rtol=1e-3, atol=1e-6)


def test_the_sharded_step_refuses(tiny_kg):
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(tiny_kg, device='cuda:0', seed=3)
    run.initialize_model(gnn_root_weight=True)
    with pytest.raises(NotImplementedError, match='gnn_root_weight'):
        run.train(batch_size=32, epoch=1, parallelism='shard')
