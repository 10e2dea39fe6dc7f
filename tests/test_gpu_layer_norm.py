"""-m gpu: layer normalisation between the message-passing layers (kgw_layer_norm_relu_fwd / _bwd / _fold, ops.layer_norm_relu,
HeteroGNN(gnn_norm='layer')) up to KGWAS.train().

The kernels at the C ABI against float64 relu(F.layer_norm) and its autograd (tests/layer_norm_ref.py).  Well-conditioned rows
(standard normal): the project's fp32 bar, helpers.assert_close(rtol 1e-4, atol 1e-5, rel_to_max 1e-5), for out and dy.
Ill-conditioned rows (constant, mean 1e4) and the column sums dw / db, for which no fixed bar can be derived: at most twice the
maximum error float32 F.layer_norm on the CPU (forward and autograd) makes on the same inputs against the same float64, plus one
fp32 ulp of the tensor's largest magnitude -- the project's convention for cancellation-prone gradients.  Both references are sent
the gradient masked by the kernel's own (out > 0), so that one mask serves all three.  Every figure is printed before it is
asserted (profiles/layer_norm/gputests.txt keeps them).
The model against the float64 oracle with F.layer_norm before the ReLU of layers 1 .. L - 1 (NormedStateOracle), at the bars
tests/test_gpu_hidden_dropout.py uses for the same routes (RTOL, ATOL, max(ATOL, 1e-4 max|ref|) for gradients, plus assert_close's
rel_to_max); the trainer bit for bit against the body it captured issued eagerly, and at test_gpu_hidden_dropout.py's bars
against the plain eager loop."""
import os
import re

import numpy as np
import pytest
import torch

from tests import hidden_dropout_ref as HD
from tests import layer_norm_ref as R
from tests.helpers import assert_close, batch_cpu, grads_by_name, launches_of_one_step, oracle_from_product, params_by_name

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5                  # tests/test_gpu_aggregate_parity.py's, as test_gpu_hidden_dropout.py uses them
PASS_ROWS = 2048 * 8                     # rows one pass of the forward's largest grid covers (KGW_GRID blocks x KGW_BLK / 32 rows)
CAP_ROWS = 2048 * 64                     # rows above which the backward's 64 rows per block no longer fit 2048 blocks
NT = 8
BS = 48


def _rand(shape, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + offset


def _params(cl, seed):
    """weight / bias [8, 128]; the columns past cl hold values a kernel that read them would show."""
    w, b = _rand((NT, R.C), seed, 0.5, 1.0), _rand((NT, R.C), seed + 1, 0.5)
    w[:, cl:], b[:, cl:] = 7.0, -3.0
    return w, b


def _pipeline(cases, w, b, cl, kernel_masks, strided=False):
    """Forward, backward and fold at the C ABI.  ``cases`` = [(type, y [rows, 128], g [rows, 128])] on the CPU.  Returns per case
    (out, stat, dy, the gradient as masked by the kernel's own out) and (dw, db) [8, 128], all on the CPU."""
    from kgwas_amd import _lib
    L = _lib.lib()
    dev = 'cuda:0'
    W, B = w.to(dev), b.to(dev)
    total = sum(y.shape[0] for _, y, _ in cases)
    stat = torch.full((max(total, 1), 2), float('nan'), device=dev)
    fj = (_lib.KgwLNormJob * len(cases))()
    keep, r0 = [], 0
    for j, (t, y, g) in zip(fj, cases):
        rows = y.shape[0]
        if strided:
            srcw = torch.zeros(rows, 132, device=dev)
            srcw[:, :128] = y.to(dev)
            src = srcw[:, :128]
            wide = torch.full((rows, 256), -3.0, device=dev)
            dst = wide[:, 128:]
        else:
            src, wide = y.to(dev), None
            dst = torch.full((rows, R.C), float('nan'), device=dev)
        j.src, j.lds, j.dst, j.ldd, j.rows, j.type = src.data_ptr(), src.stride(0) if rows else 128, dst.data_ptr(), dst.stride(0) if rows else 128, rows, t
        j.weight, j.bias, j.stat = W[t].data_ptr(), B[t].data_ptr(), stat[r0:].data_ptr()
        keep.append((src, dst, wide, stat[r0:r0 + rows], src.clone()))
        r0 += rows
    assert L.kgw_layer_norm_relu_fwd(len(cases), fj, cl, 1e-5, _lib.stream_ptr()) == 0
    bj = (_lib.KgwLNormBwdJob * len(cases))()
    res = []
    for j, (t, y, g), (src, dst, wide, st, src0) in zip(bj, cases, keep):
        rows = y.shape[0]
        gm = g.to(dev) * (dst > 0)
        gin = g.to(dev) if kernel_masks else gm.clone()
        dyw = torch.full((rows, 256 if strided else R.C), float('nan'), device=dev)
        dy = dyw[:, 128:] if strided else dyw
        j.g, j.ldg, j.y, j.ldy, j.dy, j.lddy = gin.data_ptr(), 128, src.data_ptr(), src.stride(0) if rows else 128, dy.data_ptr(), dy.stride(0) if rows else 128
        j.out, j.ldo = (dst.data_ptr(), dst.stride(0) if rows else 128) if kernel_masks else (None, 0)
        j.rows, j.type, j.weight, j.stat = rows, t, W[t].data_ptr(), st.data_ptr()
        res.append((dst, st, dy, gm, gin, src, src0, wide))
    nf = int(L.kgw_layer_norm_partial_floats(len(cases), bj))
    assert nf >= 0
    partial = torch.full((max(nf, 1),), float('nan'), device=dev)
    dw, db = torch.full((NT, R.C), float('nan'), device=dev), torch.full((NT, R.C), float('nan'), device=dev)
    assert L.kgw_layer_norm_bwd(len(cases), bj, cl, partial.data_ptr(), nf, _lib.stream_ptr()) == 0
    assert L.kgw_layer_norm_fold(len(cases), bj, partial.data_ptr(), nf, NT, dw.data_ptr(), db.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    for dst, st, dy, gm, gin, src, src0, wide in res:
        assert torch.equal(src, src0)                                            # the source is only read
        if wide is not None:
            assert bool((wide[:, :128] == -3.0).all())                           # the columns beside a strided destination too
    return [(dst.cpu(), st.cpu(), dy.cpu(), gm.cpu()) for dst, st, dy, gm, *_ in res], dw.cpu(), db.cpu()


def _float32_bar(what, ours, ref64, ref32):
    """|ours - float64| <= 2 max|float32 CPU - float64| + one fp32 ulp of max|float64|; the figures are printed first."""
    ours, ref64, ref32 = ours.double(), ref64.double(), ref32.double()
    if ours.numel() == 0:
        return
    err, err32, big = float((ours - ref64).abs().max()), float((ref32 - ref64).abs().max()), float(ref64.abs().max())
    floor = float(np.spacing(np.float32(big)))
    print(f'{what}: max abs err ours {err:.3e}, float32 CPU {err32:.3e}, max |ref| {big:.3e}, bar {2 * err32 + floor:.3e}')
    assert err <= 2 * err32 + floor, what


def _check(cases, results, dw, db, w, b, cl, label, ill=False):
    seen = set()
    for (t, y, g), (out, st, dy, gm) in zip(cases, results):
        seen.add(t)
        rows = y.shape[0]
        assert float(out[:, cl:].abs().sum()) == 0.0 and float(dy[:, cl:].abs().sum()) == 0.0        # pad columns: exactly 0
        assert float(dw[t, cl:].abs().sum()) == 0.0 and float(db[t, cl:].abs().sum()) == 0.0
        if rows == 0:
            assert float(dw[t].abs().sum()) == 0.0 and float(db[t].abs().sum()) == 0.0                # an empty job: zero rows
            continue
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dy).all()) and bool(torch.isfinite(st).all())
        o64, dy64, dw64, db64 = R.torch_reference(y, w[t], b[t], gm, cl, masked=True)
        o32, dy32, dw32, db32 = R.torch_reference(y, w[t], b[t], gm, cl, dtype=torch.float32, masked=True)
        _, mean64, rstd64, _ = R.forward(y.double(), w[t].double(), b[t].double(), cl)
        if ill:
            _float32_bar(f'{label} type {t} out', out, o64, o32)
            _float32_bar(f'{label} type {t} dy', dy, dy64, dy32)
        else:
            assert_close(out, o64, RTOL, ATOL, f'{label} type {t} out')
            assert_close(dy, dy64, RTOL, ATOL, f'{label} type {t} dy')
            assert_close(st[:, 0], mean64, RTOL, ATOL, f'{label} type {t} mean')
            assert_close(st[:, 1], rstd64, RTOL, ATOL, f'{label} type {t} rstd')
        _float32_bar(f'{label} type {t} dw', dw[t], dw64, dw32)
        _float32_bar(f'{label} type {t} db', db[t], db64, db32)
    for t in range(NT):                                                          # a type without a job: zero rows
        if t not in seen:
            assert float(dw[t].abs().sum()) == 0.0 and float(db[t].abs().sum()) == 0.0


SHAPES = [(rows, cl) for rows in (0, 1, 2, 3, 8, 9, 257) for cl in (128, 100, 64, 4, 1)] + \
    [(PASS_ROWS + 9, 128), (PASS_ROWS + 9, 100), (CAP_ROWS + 1, 128)]


@pytest.mark.parametrize('kernel_masks', [False, True], ids=['premasked', 'kernel-masks'])
@pytest.mark.parametrize('rows,cl', SHAPES)
def test_kernels_equal_float64(rows, cl, kernel_masks):
    """One job at every row count where the half-wavefront / block / grid-stride mapping changes -- none, one, both halves of a
    wavefront, an odd count, a full and an overfull block, several blocks, more rows than one pass of the forward's grid (so its
    stride wraps and the fold adds 257 blocks) and more than 64 rows x 2048 blocks (the backward doubles its rows per block) --
    at every width class, in both masking modes of the backward."""
    w, b = _params(cl, 5)
    y, g = _rand((rows, R.C), 7 + rows), _rand((rows, R.C), 11 + rows)
    y[:, cl:] = 5.0                                                              # (columns past cl are not read either)
    cases = [(3, y, g)]
    results, dw, db = _pipeline(cases, w, b, cl, kernel_masks)
    _check(cases, results, dw, db, w, b, cl, f'rows {rows} cl {cl}', ill=(cl == 1))          # (one column: constant rows, var = 0)
    if rows:
        out = results[0][0]
        assert cl < 64 or rows < 8 or 0.2 < float((out[:, :cl] > 0).float().mean()) < 0.8     # (the ReLU both opens and closes)


@pytest.mark.parametrize('n_jobs', [1, 5, 8])
def test_several_jobs_in_one_launch(n_jobs):
    """Distinct node types, row counts and parameters per job, one job empty when there are several; strided sources and
    destinations (lds = 132, ldd = 256) whose neighbouring columns stay untouched."""
    counts = [37, 1, 0, 300, 8, 129, 5, 64][:n_jobs] if n_jobs > 1 else [37]
    types = [5, 0, 7, 2, 1, 6, 3, 4][:n_jobs]
    for cl, strided in ((128, False), (100, True)):
        w, b = _params(cl, 21)
        cases = [(t, _rand((n, R.C), 100 + k), _rand((n, R.C), 200 + k)) for k, (t, n) in enumerate(zip(types, counts))]
        for kernel_masks in (False, True):
            results, dw, db = _pipeline(cases, w, b, cl, kernel_masks, strided=strided)
            _check(cases, results, dw, db, w, b, cl, f'{n_jobs} jobs cl {cl}')
        if n_jobs > 1:                                                           # the parameters are the type's own
            other = _pipeline([(types[3], cases[0][1], cases[0][2])], w, b, cl, True)[0][0][0]
            assert not torch.equal(results[0][0], other)


@pytest.mark.parametrize('cl', [128, 100])
def test_constant_rows(cl):
    """Rows of one exactly summable value each: mean = the value, var = 0, rstd = 1 / sqrt(eps) and out = relu(b), bit for bit;
    dy and the column sums at the float32 bar (xh = 0: dy = rstd (gh - mean(gh)), dw = 0, db = sum g)."""
    rows = 40
    w, b = _params(cl, 31)
    vals = torch.arange(rows, dtype=torch.float32) * 0.25 - 3.0
    y = vals.unsqueeze(1).expand(rows, R.C).contiguous()
    g = _rand((rows, R.C), 32)
    cases = [(2, y, g)]
    for kernel_masks in (False, True):
        results, dw, db = _pipeline(cases, w, b, cl, kernel_masks)
        out, st, dy, gm = results[0]
        assert torch.equal(st[:, 0], vals)
        assert torch.equal(st[:, 1], torch.full((rows,), float(np.float32(1.0) / np.sqrt(np.float32(1e-5)))))
        assert torch.equal(out[:, :cl], torch.relu(b[2, :cl]).expand(rows, cl))
        assert float(dw[2].abs().sum()) == 0.0
        _check(cases, results, dw, db, w, b, cl, f'constant rows cl {cl}', ill=True)


@pytest.mark.parametrize('cl', [128, 100])
def test_rows_with_a_large_offset(cl):
    """Mean 1e4, unit spread: what the two-pass variance and the refined mean are for (E[y^2] - mean^2 would keep no bit of the
    spread, and a float32 mean alone is good to 5e-4 here)."""
    rows = 257
    w, b = _params(cl, 41)
    y, g = _rand((rows, R.C), 42, offset=1e4), _rand((rows, R.C), 43)
    cases = [(6, y, g)]
    for kernel_masks in (False, True):
        results, dw, db = _pipeline(cases, w, b, cl, kernel_masks)
        out, st, dy, gm = results[0]
        _, mean64, rstd64, _ = R.forward(y.double(), w[6].double(), b[6].double(), cl)
        assert float((st[:, 0].double() - mean64).abs().max()) <= float(np.spacing(np.float32(1e4)))   # the mean as float32 holds it
        assert float((st[:, 1].double() / rstd64 - 1).abs().max()) < 1e-4                               # ... and a spread not lost
        _check(cases, results, dw, db, w, b, cl, f'offset 1e4 cl {cl}', ill=True)


def test_two_runs_give_equal_bits():
    """out, stat, dy, dw and db of two runs over five jobs (several blocks each, one pass of the grid exceeded): equal bits."""
    counts, types = [1000, 37, 0, PASS_ROWS + 100, 129], [5, 0, 7, 2, 1]
    w, b = _params(100, 51)
    cases = [(t, _rand((n, R.C), 300 + k), _rand((n, R.C), 400 + k)) for k, (t, n) in enumerate(zip(types, counts))]
    a = _pipeline(cases, w, b, 100, True)
    c = _pipeline(cases, w, b, 100, True)
    for (o1, s1, d1, _), (o2, s2, d2, _) in zip(a[0], c[0]):
        assert torch.equal(o1, o2) and torch.equal(s1, s2) and torch.equal(d1, d2)
    assert torch.equal(a[1], c[1]) and torch.equal(a[2], c[2]) and float(a[1].abs().sum()) > 0


def test_ops_forward_and_backward():
    """ops.layer_norm_relu over three types: one block written in place of the next layer's input, the inputs left alone (the
    producer saved them), a None gradient passed through, packed gradients with zero rows for the types that got none; both
    masking modes against float64 autograd."""
    from kgwas_amd import ops
    cl, types, counts = 100, [4, 0, 2], [33, 260, 5]
    w, b = _params(cl, 61)
    w[:, cl:], b[:, cl:] = 0.0, 0.0
    ys = [_rand((n, R.C), 70 + k) for k, n in enumerate(counts)]
    gs_ = [_rand((n, R.C), 80 + k) for k, n in enumerate(counts)]
    for premasked in (False, True):
        W, B = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        leaves = [y.cuda().requires_grad_(True) for y in ys]
        buf = torch.zeros(300, R.C, device='cuda:0')
        blocks = [None, ops.RowBlock(buf, 16, 260), ops.RowBlock(buf, 0, 7)]       # (the last one does not fit: a temporary)
        outs = ops.layer_norm_relu(leaves, types, W, B, cl, blocks, premasked=premasked)
        assert outs[1].data_ptr() == buf[16:].data_ptr() and outs[2].data_ptr() != buf.data_ptr()
        ups = [g.cuda() * (o.detach() > 0) if premasked else g.cuda() for g, o in zip(gs_, outs)]
        torch.autograd.backward([outs[0], outs[1]], [ups[0], ups[1]])               # (the third output has no gradient)
        torch.cuda.synchronize()
        assert leaves[2].grad is None and float(W.grad[2].abs().sum()) == 0.0 == float(B.grad[2].abs().sum())
        for t in range(NT):
            if t not in (4, 0):
                assert float(W.grad[t].abs().sum()) == 0.0 == float(B.grad[t].abs().sum())
        for k in (0, 1):
            t = types[k]
            assert torch.equal(leaves[k].detach().cpu(), ys[k])
            gm = gs_[k] * (outs[k].detach().cpu() > 0)
            o64, dy64, dw64, db64 = R.torch_reference(ys[k], w[t], b[t], gm, cl, masked=True)
            _, _, dw32, db32 = R.torch_reference(ys[k], w[t], b[t], gm, cl, dtype=torch.float32, masked=True)
            assert_close(outs[k], o64, RTOL, ATOL, f'ops out {k}')
            assert_close(leaves[k].grad, dy64, RTOL, ATOL, f'ops dy {k}')
            _float32_bar(f'ops dw type {t}', W.grad[t].cpu(), dw64, dw32)
            _float32_bar(f'ops db type {t}', B.grad[t].cpu(), db64, db32)
    with pytest.raises(ValueError):
        ops.layer_norm_relu(leaves, types, W, B, 129)
    with pytest.raises(AssertionError):
        ops.layer_norm_relu(leaves, [4, 4, 2], W, B, cl)


# ------------------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------------------
ROUTES = {
    'gat-sum': dict(backbone='GAT', aggr='sum'),
    'gat-mean': dict(backbone='GAT', aggr='mean'),        # (the 1 / R goes in before the norm)
    'gat-heads2': dict(backbone='GAT', aggr='sum', heads=2),
    'sage-sum': dict(backbone='SAGE', aggr='sum'),
    'gat-min': dict(backbone='GAT', aggr='min'),
    'gat-sum-width100': dict(backbone='GAT', aggr='sum', hidden=100),
    'gat-3layers': dict(backbone='GAT', aggr='sum', layers=3),
}


def _model(kg, route, norm='layer', p=0.0, seed=3):
    from kgwas_amd.model import HeteroGNN
    r = ROUTES[route]
    torch.manual_seed(seed)
    dims = (kg.snp_init_dim_size, kg.gene_init_dim_size, kg.go_init_dim_size)
    model = HeteroGNN(kg.data, r.get('hidden', 128), 1, r.get('layers', 2), r['backbone'], r['aggr'], *dims, r.get('heads', 1),
                      gat_split_heads=True, gnn_dropout=p, gnn_norm=norm).cuda()
    with torch.no_grad():
        for pack in list(model.live_packs) + list(model.dead_packs):
            pack.bias.normal_(0, 0.1)
        model.lin.bias.fill_(0.5)            # (an open read-out ReLU for most seeds: every parameter gets a gradient)
        for w, b in zip(model.norm_weight, model.norm_bias):
            live = (w != 0).float()          # (the rows of the destination types at the model's own width; the rest stays 0)
            w.add_(torch.randn_like(w) * 0.3 * live)
            b.add_(torch.randn_like(b) * 0.2 * live)
    return model


def _oracle(model, state_factor=None):
    build = oracle_from_product
    if model.heads > 1:
        from tests.multihead_ref import oracle_with_heads as build
    return R.normed_oracle(model, build, state_factor)


def _batch(kg, layers=2):
    from kgwas_amd.sampler import NeighborLoader
    ids = np.random.default_rng(0).choice(kg.data['SNP'].x.shape[0], size=BS, replace=False)
    return next(iter(NeighborLoader(kg.data, [-1] * layers, ('SNP', ids), batch_size=BS, device='cuda:0', seed=5)))


def _labels(kg):
    g = torch.Generator().manual_seed(9)
    n = kg.data['SNP'].x.shape[0]
    return kg.data['SNP'].y.cuda(), (torch.rand(n, generator=g, dtype=torch.float64) + 0.5).cuda()


def _against_oracle(model, oracle, batch, y_all, w_all, route, word=None):
    """forward_loss + backward and forward in training mode, model.eval() and return_h, against ``oracle``."""
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
    x, ei = batch_cpu(batch)
    out_o = oracle(x, ei, BS).reshape(-1)
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
    n_live = n_norm = 0
    for name, g in grads_by_name(model).items():
        ref = go[name]
        if g is None:
            assert ref is None or float(ref.abs().max()) == 0.0, f'{name}: product has no grad, oracle has'
            continue
        if ref is None:                       # (a norm row of a type without rows in the layer: zeros, where the oracle has None)
            assert name.startswith('norms.') and float(g.abs().max()) == 0.0, name
            continue
        n_live += 1
        n_norm += name.startswith('norms.') and float(ref.abs().max()) > 0
        assert tuple(g.shape) == tuple(ref.shape), (name, g.shape, ref.shape)
        assert_close(g, ref, RTOL, max(ATOL, 1e-4 * float(ref.abs().max())), f'grad {name}')
    assert n_live > 10 and n_norm >= 2, (n_live, n_norm)
    return out_o.detach(), x, ei


@pytest.mark.parametrize('route', list(ROUTES))
def test_model_matches_the_normed_oracle(small_kg, route):
    """Per route: the training forward, the loss and every gradient (the norms' among them), the evaluation forward and
    return_h, against the float64 oracle; the oracle without its norms is another function."""
    model = _model(small_kg, route)
    L = model.num_layers
    assert len(model.norm_weight) == L - 1
    if route == 'gat-sum':
        assert model.fold_fc
    batch = _batch(small_kg, L)
    y_all, w_all = _labels(small_kg)
    oracle = _oracle(model)
    out_o, x, ei = _against_oracle(model, oracle, batch, y_all, w_all, route)
    # the norm is live in evaluation: the same function
    model.eval()
    with torch.no_grad():
        a = model(batch.x_dict, batch.edge_index_dict, BS)
        a2, h = model(batch.x_dict, batch.edge_index_dict, BS, return_h=True)
        _, h_o = oracle(x, ei, BS, return_h=True)
    assert_close(a.reshape(-1), out_o, RTOL, ATOL, 'pred (eval)')
    assert torch.equal(a, a2)
    assert_close(h, h_o, RTOL, ATOL, 'h (eval, return_h)')
    # ... and really applied: the oracle with the plain ReLU differs
    plain = oracle_from_product(R._WithoutNorms(model)) if model.heads == 1 else None
    if plain is not None:
        with torch.no_grad():
            diff = float((plain(x, ei, BS).reshape(-1) - out_o).abs().max())
        print(f'{route}: the oracle without norms differs by {diff:.3e}')
        assert diff > 1e-3
    # the attention queries apply it too: layer 2's weights are those of a normed layer-1 state
    if model.backbone == 'GAT' and model.heads == 1 and model.aggr == 'sum':
        with torch.no_grad():
            out_att, att = model(batch.x_dict, batch.edge_index_dict, BS, return_attention_weights=True)
            per_edge = [a.clone() for a in model.last_attention]
            hot = model.hot_path_attention(batch)
        assert len(att) == L == len(hot)
        assert_close(out_att.reshape(-1), out_o, RTOL, ATOL, 'pred (all-relations route)')
        twin = _model(small_kg, route, norm=None)
        twin.load_state_dict({k: v for k, v in model.state_dict().items() if not k.startswith('norms.')})
        twin.eval()
        with torch.no_grad():
            twin(batch.x_dict, batch.edge_index_dict, BS, return_attention_weights=True)
            hot_t = twin.hot_path_attention(batch)
        # (per edge: the MEAN of softmax weights is rows / edges whatever the state)
        assert torch.equal(per_edge[0], twin.last_attention[0]) and torch.equal(hot[0], hot_t[0])     # layer 1 reads no normed state
        assert not torch.equal(per_edge[1], twin.last_attention[1]) and not torch.equal(hot[1], hot_t[1])
        with torch.no_grad():
            oa = oracle.attention_means(x, ei)
        for k in range(L):
            assert_close(att[k], oa[k], RTOL, ATOL, f'mean attention layer {k + 1}')


def test_norm_together_with_hidden_dropout(small_kg):
    """conv -> norm -> ReLU -> dropout: the dropout launch reads the norm's output.  Against the oracle with both."""
    p, word = 0.25, HD.dropout_word(5, 1, 2)
    model = _model(small_kg, 'gat-sum', p=p)
    batch = _batch(small_kg)
    y_all, w_all = _labels(small_kg)
    fac, n_dropped = HD.state_factors(model, batch, word, p)
    assert n_dropped > 100
    _against_oracle(model, _oracle(model, fac), batch, y_all, w_all, 'gat-sum + dropout', word=word)


def _train_pass(model, batch, y_all, w_all):
    from kgwas_amd import ops
    model.train()
    model.zero_grad(set_to_none=True)
    loss, pred = model.forward_loss(batch.x_dict, batch.edge_index_dict, BS, batch.n_id('SNP'), y_all, w_all, unit_grad=True)
    loss.backward(gradient=ops.unit_gradient(loss.device))
    torch.cuda.synchronize()
    return loss.detach().clone(), pred.detach().clone(), {n: g.clone() for n, g in grads_by_name(model).items() if g is not None}


def test_the_default_model_is_unchanged(small_kg):
    """gnn_norm=None (given or left out): loss, predictions and every gradient bit for bit those of the same pass again and of a
    model built without the keyword; and an identity norm (weight 1, bias 0) is NOT the default model: it normalises."""
    from kgwas_amd.model import HeteroGNN
    batch = _batch(small_kg)
    y_all, w_all = _labels(small_kg)
    a = _model(small_kg, 'gat-sum', norm=None)
    dims = (small_kg.snp_init_dim_size, small_kg.gene_init_dim_size, small_kg.go_init_dim_size)
    b = HeteroGNN(small_kg.data, 128, 1, 2, 'GAT', 'sum', *dims, 1).cuda()
    b.load_state_dict(a.state_dict())
    assert a.gnn_norm is None and b.gnn_norm is None and a._norm_site(1) is None and list(a.state_dict()) == list(b.state_dict())
    ra, ra2, rb = _train_pass(a, batch, y_all, w_all), _train_pass(a, batch, y_all, w_all), _train_pass(b, batch, y_all, w_all)
    for other in (ra2, rb):
        assert torch.equal(ra[0], other[0]) and torch.equal(ra[1], other[1]) and sorted(ra[2]) == sorted(other[2])
        for n in ra[2]:
            assert torch.equal(ra[2][n], other[2][n]), n
    assert len(ra[2]) > 10 and float(ra[0]) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# trainer
# ------------------------------------------------------------------------------------------------------------------------------
def _launches_of_one_step(gs):
    """Kernel launches of one training step issued eagerly through the body the trainer captured (tests/helpers.py):
    (all, [names of the k_layer_norm_* among them])."""
    names = launches_of_one_step(gs)
    return len(names), sorted(re.search(r'k_layer_norm\w*', n).group(0) for n in names if 'k_layer_norm' in n)


def test_the_feature_adds_three_launches_and_the_default_step_has_none(tiny_kg):
    """Kernel launches of one eager step (the profiler's count): a default model issues no k_layer_norm_* launch -- with the
    keyword left out and with gnn_norm=None alike, the same count -- and gnn_norm='layer' adds exactly the forward, the backward
    and the fold of the one site of a two-layer model, and nothing else.  (The launch count of the benchmark's default step is a
    property of its graph, too large for a test: tools/bench_layer_norm.py records it, profiles/layer_norm/.)"""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    bs = 32
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * 2])
    counts = {}
    for what, kw in (('left out', {}), ('None', dict(gnn_norm=None)), ('layer', dict(gnn_norm='layer'))):
        run = KGWAS(tiny_kg, device='cuda:0', seed=7)
        run.initialize_model(**kw)
        run.model.train()
        gs = GraphTrainStep(run, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=7)
        assert gs.fused_adam and run.model.fold_fc and gs.layer_norm == (what == 'layer')
        counts[what] = _launches_of_one_step(gs)
        print(f'gnn_norm {what}: {counts[what][0]} kernel launches, k_layer_norm_*: {counts[what][1]}')
    assert counts['left out'] == counts['None'] and counts['None'][1] == [] and counts['None'][0] > 10
    assert counts['layer'][0] == counts['None'][0] + 3
    assert [n for n in counts['layer'][1]] == ['k_layer_norm_bwd', 'k_layer_norm_fold', 'k_layer_norm_relu_fwd']


def test_captured_step_equals_eager_step_bit_for_bit(tiny_kg):
    """Three steps of GraphTrainStep against three eager steps of the same launches (a second trainer on its own copy of the model,
    stepped through the body the first one captured): every loss and every parameter afterwards -- the norms' too -- bit for
    bit; then the captured loop against the plain eager loop (KGWAS.train_step, torch's Adam) at test_gpu_hidden_dropout.py's bars.
    The step keeps the FC_output fold and the fused optimiser launch, and the norm parameters move."""
    from kgwas_amd.graph_step import GraphTrainStep
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    bs, nsteps, seed = 32, 3, 11
    ids = np.asarray(tiny_kg.train_input_nodes[1][:bs * nsteps])
    runs = []
    for _ in range(3):
        run = KGWAS(tiny_kg, device='cuda:0', seed=seed)
        run.initialize_model(gnn_norm='layer')
        runs.append(run)
    run_e, run_g, run_c = runs
    with torch.no_grad():
        run_e.model.lin.bias.fill_(0.5)      # (an open read-out ReLU: every parameter gets a gradient)
    run_g.model.load_state_dict(run_e.model.state_dict())
    run_c.model.load_state_dict(run_e.model.state_dict())
    p0 = params_by_name(run_e.model)
    gs = GraphTrainStep(run_g, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=seed)
    gc = GraphTrainStep(run_c, ('SNP', ids), bs, lr=1e-3, weight_decay=5e-4, sample_seed=seed)
    assert gs.layer_norm and gs.fused_adam and run_g.model.fold_fc and gs.n_batches == nsteps
    for n, p in params_by_name(run_g.model).items():
        assert torch.equal(p, p0[n]), n                       # (the capture's warm-up steps were undone)
    for m in (run_e.model, run_g.model, run_c.model):
        m.train()
    opt = torch.optim.Adam(run_e.model.parameters(), lr=1e-3, weight_decay=5e-4)
    ld_w = run_e._ld_weight_vector()
    for step, batch in enumerate(NeighborLoader(tiny_kg.data, [-1, -1], ('SNP', ids), batch_size=bs, drop_last=True, device='cuda:0')):
        lg = gs.step(step).detach().clone()
        gc._sample_now(step % 2, step)
        torch.cuda.synchronize()
        lc = gc._step_body(step % 2).detach().clone()
        torch.cuda.synchronize()
        le = run_e.train_step(batch, opt, ld_w)
        print(f'step {step}: captured {float(lg):.9f} same launches eagerly {float(lc):.9f} plain eager loop {float(le.detach()):.9f}')
        assert torch.equal(lg, lc), (step, float(lg), float(lc))
        pg, pc = params_by_name(run_g.model), params_by_name(run_c.model)
        assert all(torch.equal(pg[n], pc[n]) for n in pg), [n for n in pg if not torch.equal(pg[n], pc[n])][:5]
        assert_close(lg, le.detach(), 1e-5, 1e-7, f'loss step {step}')
    gs.check()
    assert step == nsteps - 1 and gs.fused_adam and gc.fused_adam
    pe, pg = params_by_name(run_e.model), params_by_name(run_g.model)
    num = sum(float((pe[n] - pg[n]).pow(2).sum()) for n in pe)
    den = sum(float((pe[n] - p0[n]).pow(2).sum()) for n in pe)
    print(f'relative update difference {(num / den) ** 0.5:.3e}')
    assert den > 0 and (num / den) ** 0.5 < 5e-3, f'relative update difference {(num / den) ** 0.5:.3e}'
    moved = [n for n in pg if n.startswith('norms.') and float((pg[n] - p0[n]).abs().max()) > 0]
    assert len(moved) >= 4, moved
    # pad columns and the rows of other types stay zero under Adam with weight decay
    for w, b in zip(run_g.model.norm_weight, run_g.model.norm_bias):
        dead = [t for t in range(w.shape[0]) if t not in run_g.model.norm_types]
        assert float(w.detach()[dead].abs().sum()) == 0.0 == float(b.detach()[dead].abs().sum())


@pytest.mark.parametrize('case', ['plain', 'fanout-shuffle-dropout', 'eager-sage-mean'])
def test_train_two_epochs_end_to_end(tiny_kg, case):
    """KGWAS.train(epoch=2) with a gnn_norm model -- the captured step (alone; beside a finite fan-out, a shuffled order and
    gnn_dropout) or the eager loop on SAGE / mean -- evaluation, the saved model and the result table; then save_model ->
    load_pretrained -> identical predictions."""
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    run = KGWAS(tiny_kg, device='cuda:0', seed=3)
    kw = {'plain': {}, 'fanout-shuffle-dropout': dict(gnn_dropout=0.2), 'eager-sage-mean': dict(gnn_backbone='SAGE', gnn_aggr='mean')}[case]
    run.initialize_model(gnn_norm='layer', **kw)
    with torch.no_grad():
        run.model.lin.bias.fill_(0.5)
    w0 = run.model.norm_weight[0].detach().clone()
    name = 'layer_norm_e2e_' + case
    tkw = {'plain': {}, 'fanout-shuffle-dropout': dict(num_neighbors=[10, 5], shuffle=True), 'eager-sage-mean': dict(use_graph=False)}[case]
    run.train(batch_size=32, epoch=2, save_best_model=True, save_name=name, **tkw)
    assert np.isfinite(run.val_metrics['mse']) and np.isfinite(run.val_metrics['pearsonr'])
    assert run.config['gnn_norm'] == 'layer' and run.kgwas_res is not None and len(run.kgwas_res) > 0
    assert not torch.equal(run.model.norm_weight[0].detach(), w0)                    # the norm was trained
    assert os.path.exists(os.path.join(tiny_kg.data_path, 'model_pred', 'new_experiments', name + '_pred.csv'))
    assert os.path.exists(os.path.join(tiny_kg.data_path, 'model', name, 'config.pkl'))
    run2 = KGWAS(tiny_kg, device='cuda:0', seed=4)
    run2.load_pretrained(os.path.join(tiny_kg.data_path, 'model', name))
    assert run2.config == run.config and run2.model.gnn_norm == 'layer'
    sa, sb = run.best_model.state_dict(), run2.model.state_dict()
    assert list(sa) == list(sb) and any(k.startswith('norms.') for k in sa)
    ids = np.asarray(tiny_kg.val_input_nodes[1][:64])
    batch = next(iter(NeighborLoader(tiny_kg.data, [-1, -1], ('SNP', ids), batch_size=64, device='cuda:0')))
    run.best_model.eval(); run2.model.eval()
    with torch.no_grad():
        a = run.best_model(batch.x_dict, batch.edge_index_dict, 64)
        b = run2.model(batch.x_dict, batch.edge_index_dict, 64)
    assert torch.equal(a, b) and float(a.abs().sum()) > 0


def test_network_weight_export_of_a_normed_model(small_kg):
    """KGWAS.get_network_weight() of a normed model against the export's procedure on the float64 oracle: raw attention returned
    and propagated, the state between the layers normalised and -- like the reference's -- not passed through a ReLU."""
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(small_kg, device='cuda:0', seed=5)
    run.initialize_model(gnn_norm='layer')
    m = run.model
    with torch.no_grad():
        for pack in list(m.live_packs) + list(m.dead_packs):
            pack.bias.uniform_(-0.1, 0.1)
        for w, b in zip(m.norm_weight, m.norm_bias):
            live = (w != 0).float()
            w.add_(torch.randn_like(w) * 0.3 * live)
            b.add_(torch.randn_like(b) * 0.2 * live)
    run.best_model = m
    df = run.get_network_weight()
    assert set(df.layer.unique()) == {'l1', 'l2'}
    g = small_kg.data
    o = R.normed_oracle(m, oracle_from_product)
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
    # the norm is applied: layer 2's attention of the same weights without it is another table
    run0 = KGWAS(small_kg, device='cuda:0', seed=5)
    run0.initialize_model()
    run0.model.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith('norms.')})
    run0.best_model = run0.model
    df0 = run0.get_network_weight()
    assert np.array_equal(df[df.layer == 'l1'].weight.values, df0[df0.layer == 'l1'].weight.values)
    assert not np.allclose(df[df.layer == 'l2'].weight.values, df0[df0.layer == 'l2'].weight.values, rtol=1e-3, atol=1e-6)
