"""CPU: the layer-normalisation rule (tests/layer_norm_ref.py) against float64 autograd, the header and the bindings, the
refusals of the C entry points before any launch, and how KGWAS / HeteroGNN carry ``gnn_norm`` through config and state_dict."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

from tests import layer_norm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(rows, cl, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(rows, R.C, generator=g, dtype=torch.float64) + offset
    w = torch.randn(R.C, generator=g, dtype=torch.float64)
    b = torch.randn(R.C, generator=g, dtype=torch.float64) * 0.5
    up = torch.randn(rows, R.C, generator=g, dtype=torch.float64)
    y[:, cl:] = 0
    w[cl:] = 0
    b[cl:] = 0
    return y, w, b, up


@pytest.mark.parametrize('cl', [128, 100, 64, 4, 1])
@pytest.mark.parametrize('rows', [1, 9, 257])
def test_closed_form_equals_float64_autograd(rows, cl):
    """forward / backward of the ref (the header's formulas) against relu(F.layer_norm) and its autograd, both float64: they differ
    by rounding only.  cl = 1: var = 0, xh = 0, out = relu(b) and dy = 0."""
    y, w, b, up = _case(rows, cl, 10 * rows + cl)
    out, mean, rstd, xh = R.forward(y, w, b, cl)
    o_t, dy_t, dw_t, db_t = R.torch_reference(y, w, b, up, cl)
    dy, dw, db = R.backward(up, y, w, b, cl)
    for name, a, ref in (('out', out, o_t), ('dy', dy, dy_t), ('dw', dw, dw_t), ('db', db, db_t)):
        assert float((a - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), name
        assert float(a[..., cl:].abs().sum()) == 0.0, name
    # the masked form: handing in g * (out > 0) gives the same
    dy2, dw2, db2 = R.backward(up * (out > 0), y, w, b, cl, masked=True)
    assert torch.equal(dy, dy2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    if cl == 1:
        assert float(xh.abs().sum()) == 0.0 and torch.equal(out[:, 0], torch.relu(b[0]).expand(rows)) and float(dy.abs().sum()) == 0.0


def test_constant_rows_and_large_offsets():
    """A constant row: var = 0, rstd = 1 / sqrt(eps), out = relu(b).  Mean 1e4 with unit spread: in float32 the two-pass variance
    keeps what E[y^2] - mean^2 loses (1e8 against a spread of 1 leaves no bit of it)."""
    cl = 100
    y, w, b, _ = _case(5, cl, 3)
    y[:, :cl] = 7.25
    out, mean, rstd, xh = R.forward(y, w, b, cl)
    assert torch.equal(mean, torch.full((5,), 7.25, dtype=torch.float64)) and float(xh.abs().sum()) == 0.0
    assert torch.allclose(rstd, torch.full((5,), R.EPS ** -0.5, dtype=torch.float64), rtol=1e-15)
    assert torch.equal(out[:, :cl], torch.relu(b[:cl]).expand(5, cl))
    y, w, b, _ = _case(64, 128, 4, offset=1e4)
    y32 = y.float()
    two_pass = ((y32 - y32.mean(1, keepdim=True)) ** 2).mean(1)
    one_pass = (y32 * y32).mean(1) - y32.mean(1) ** 2
    exact = y32.double().var(1, unbiased=False)
    assert float(((two_pass.double() - exact) / exact).abs().max()) < 1e-3
    assert float(((one_pass.double() - exact) / exact).abs().max()) > 1.0


def test_header_names_the_rule():
    hdr = open(os.path.join(ROOT, 'include', 'kgwas_hip.h')).read()
    for name in ('KGW_LNORM_EPS 1e-5f', 'kgwlnorm_out', 'kgwlnorm_dy', 'KgwLNormJob', 'KgwLNormBwdJob',
                 'int kgw_layer_norm_relu_fwd(', 'int kgw_layer_norm_bwd(', 'int kgw_layer_norm_fold(',
                 'int64_t kgw_layer_norm_partial_floats(', 'mean = m0 + sum(y - m0) / Cl', 'return rstd * (gh - mean_gh - xh * mean_ghxh);'):
        assert name in hdr, name
    assert hdr.index('int kgwhdrop_keep(') < hdr.index('#define KGW_LNORM_EPS') < hdr.index('int kgw_gat_aggregate_fwd')
    assert '#define KGW_VERSION      125' in hdr


def test_symbol_binding_and_struct_sizes():
    from kgwas_amd import _lib
    L = _lib.lib()
    assert _lib.has_layer_norm() and L.kgw_version() == 125
    for name in ('kgw_layer_norm_relu_fwd', 'kgw_layer_norm_partial_floats', 'kgw_layer_norm_bwd', 'kgw_layer_norm_fold'):
        assert hasattr(L, name) and name in _lib.EXPORTS
    j, k = _lib.KgwLNormJob, _lib.KgwLNormBwdJob
    assert C.sizeof(j) == 64 and (j.src.offset, j.lds.offset, j.dst.offset, j.ldd.offset, j.rows.offset, j.type.offset,
                                  j.weight.offset, j.bias.offset, j.stat.offset) == (0, 8, 16, 24, 32, 36, 40, 48, 56)
    assert C.sizeof(k) == 88 and (k.g.offset, k.y.offset, k.out.offset, k.dy.offset, k.rows.offset, k.type.offset, k.weight.offset,
                                  k.stat.offset) == (0, 16, 32, 48, 64, 68, 72, 80)
    # no struct of the existing ABI changed
    s8 = (C.c_int64 * 8)()
    assert L.kgw_struct_sizes(s8, 8) == 0 and s8[4] == C.sizeof(_lib.KgwLayerArgs) and s8[7] == C.sizeof(_lib.KgwEdgeAttr)


def test_refusals_by_value_before_any_launch():
    """Every call here is refused (or has no rows) before a kernel could be launched: the pointers are host memory or NULL."""
    from kgwas_amd import _lib
    L = _lib.lib()
    E_NULL, E_RANGE, E_UNSUPPORTED = -1, -2, _lib.KGW_E_UNSUPPORTED
    buf = np.zeros(64 * 128 + 8, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16                     # a 16-byte aligned host address
    q = p + 16 * 128 * 4

    def fjob(rows=4, src=p, dst=q, lds=128, ldd=128, t=0, w=p, b=p, stat=p):
        j = _lib.KgwLNormJob()
        j.src, j.lds, j.dst, j.ldd, j.rows, j.type, j.weight, j.bias, j.stat = src, lds, dst, ldd, rows, t, w, b, stat
        return j

    def fwd(jobs, n=None, cl=128, eps=1e-5):
        arr = (_lib.KgwLNormJob * max(1, len(jobs)))(*jobs)
        return L.kgw_layer_norm_relu_fwd(len(jobs) if n is None else n, arr, cl, eps, None)

    assert L.kgw_layer_norm_relu_fwd(1, None, 128, 1e-5, None) == E_NULL
    for kw in (dict(src=None), dict(dst=None), dict(w=None), dict(b=None), dict(stat=None)):
        assert fwd([fjob(**kw)]) == E_NULL, kw
    assert fwd([fjob()], n=0) == E_RANGE and fwd([fjob()] * 8, n=9) == E_RANGE
    for cl in (0, -1, 129):
        assert fwd([fjob()], cl=cl) == E_RANGE
    for eps in (-1e-5, float('inf'), float('nan')):
        assert fwd([fjob()], eps=eps) == E_RANGE
    assert fwd([fjob(rows=-1)]) == E_RANGE and fwd([fjob(rows=(1 << 25) + 1)]) == E_RANGE
    assert fwd([fjob(lds=64)]) == E_RANGE and fwd([fjob(ldd=124)]) == E_RANGE
    for kw in (dict(src=p + 4), dict(dst=q + 8), dict(w=p + 4), dict(b=p + 8), dict(stat=p + 4), dict(lds=130), dict(ldd=258), dict(dst=p)):
        assert fwd([fjob(**kw)]) == E_UNSUPPORTED, kw
    assert fwd([fjob(), fjob(lds=130)]) == E_UNSUPPORTED                # any job of the list
    assert fwd([fjob(rows=0), fjob(rows=0, src=None, dst=None, w=None, b=None, stat=None)]) == 0

    def bjob(rows=4, g=p, y=p, out=None, dy=q, t=0, w=p, stat=p, ld=128):
        j = _lib.KgwLNormBwdJob()
        j.g, j.ldg, j.y, j.ldy, j.out, j.ldo, j.dy, j.lddy = g, ld, y, ld, out, ld, dy, ld
        j.rows, j.type, j.weight, j.stat = rows, t, w, stat
        return j

    def arr(jobs):
        return (_lib.KgwLNormBwdJob * max(1, len(jobs)))(*jobs)

    def bwd(jobs, n=None, cl=128, part=p, nf=1 << 20):
        return L.kgw_layer_norm_bwd(len(jobs) if n is None else n, arr(jobs), cl, part, nf, None)

    def fold(jobs, n=None, part=p, nf=1 << 20, nt=8, dw=p, db=p):
        return L.kgw_layer_norm_fold(len(jobs) if n is None else n, arr(jobs), part, nf, nt, dw, db, None)

    assert L.kgw_layer_norm_bwd(1, None, 128, p, 1 << 20, None) == E_NULL and bwd([bjob()], part=None) == E_NULL
    for kw in (dict(g=None), dict(y=None), dict(dy=None), dict(w=None), dict(stat=None)):
        assert bwd([bjob(**kw)]) == E_NULL, kw
    assert bwd([bjob()], n=0) == E_RANGE and bwd([bjob()], cl=0) == E_RANGE and bwd([bjob()], cl=129) == E_RANGE
    assert bwd([bjob(rows=-1)]) == E_RANGE and bwd([bjob(ld=64)]) == E_RANGE
    assert bwd([bjob(t=8)]) == E_RANGE and bwd([bjob(t=-1)]) == E_RANGE and bwd([bjob(t=2), bjob(t=2)]) == E_RANGE
    assert bwd([bjob()], nf=255) == E_RANGE                             # 4 rows: one block, 256 floats
    for kw in (dict(g=p + 4), dict(out=p + 4), dict(dy=q + 8), dict(stat=p + 4), dict(ld=130)):
        assert bwd([bjob(**kw)]) == E_UNSUPPORTED, kw
    assert bwd([bjob(rows=0), bjob(rows=0, t=1)]) == 0                  # no rows: no launch
    assert fold([bjob()], part=None) == E_NULL and fold([bjob()], dw=None) == E_NULL and fold([bjob()], db=None) == E_NULL
    assert fold([bjob()], nt=0) == E_RANGE and fold([bjob()], nt=9) == E_RANGE and fold([bjob(t=3)], nt=3) == E_RANGE
    assert fold([bjob()], nf=255) == E_RANGE

    # the partial sums' size is a function of the row counts alone: 64 rows per block until 2048 blocks are not enough
    def floats(rows):
        return int(L.kgw_layer_norm_partial_floats(len(rows), arr([bjob(rows=r, t=k) for k, r in enumerate(rows)])))
    assert floats([0]) == 0 and floats([1]) == 256 and floats([64]) == 256 and floats([65]) == 512
    assert floats([1, 0, 64, 129]) == (1 + 0 + 1 + 3) * 256
    assert floats([2048 * 64]) == 2048 * 256 and floats([2048 * 64 + 1]) == 1025 * 256
    assert floats([1 << 25] * 8) <= 2048 * 256
    assert L.kgw_layer_norm_partial_floats(0, arr([bjob()])) == E_RANGE and L.kgw_layer_norm_partial_floats(1, None) == E_NULL


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path_factory.mktemp('lnorm')))


def test_construction_and_refusals(tiny):
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.model import HeteroGNN
    run = KGWAS(tiny, device='cpu', seed=1)
    for bad in ('batch', 'Layer', True, 1):
        with pytest.raises(ValueError, match='gnn_norm'):
            run.initialize_model(gnn_norm=bad)
    with pytest.raises(ValueError, match='gnn_norm'):
        run.initialize_model(gnn_num_layers=1, gnn_norm='layer')
    dims = (tiny.snp_init_dim_size, tiny.gene_init_dim_size, tiny.go_init_dim_size)
    with pytest.raises(ValueError, match='gnn_norm'):
        HeteroGNN(tiny.data, 128, 1, 1, 'GAT', 'sum', *dims, 1, gnn_norm='layer')
    with pytest.raises(ValueError, match='gnn_norm'):
        HeteroGNN(tiny.data, 128, 1, 2, 'GAT', 'sum', *dims, 1, gnn_norm='graph')
    run.initialize_model(gnn_num_layers=1)                                   # (no norm: one layer as before)
    for kw in ({'gnn_backbone': 'SAGE'}, {'gnn_aggr': 'max'}, {'gat_num_head': 2}, {'gat_sigmoid': True}, {'gat_dropout': 0.1},
               {'gnn_dropout': 0.2}, {'gnn_num_layers': 3}, {'gnn_hidden_dim': 100}):
        run.initialize_model(gnn_norm='layer', **kw)                         # independent of the backbone and of every switch
        assert run.model.gnn_norm == 'layer' and len(run.model.norm_weight) == run.model.num_layers - 1
    run.initialize_model(gnn_norm='layer')
    m = run.model
    assert m.fold_fc and m._norm_site(1) is not None and m._norm_site(2) is None
    m.eval()
    assert m._norm_site(1) is not None                                       # live in evaluation
    with pytest.raises(NotImplementedError, match='gnn_norm'):
        run.train(epoch=1, parallelism='shard')
    run.initialize_model()
    assert run.model.gnn_norm is None and run.model._norm_site(1) is None and len(run.model.norm_weight) == 0


def test_config_carries_the_key_only_when_set(tiny, tmp_path):
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.utils import save_model
    run = KGWAS(tiny, device='cpu', seed=1)
    run.initialize_model()
    default = dict(run.config)
    assert sorted(default) == ['gat_num_head', 'gnn_aggr', 'gnn_backbone', 'gnn_hidden_dim', 'gnn_num_layers']
    run.initialize_model(gnn_norm=None)
    assert run.config == default
    run.initialize_model(gnn_norm='layer')
    assert run.config == dict(default, gnn_norm='layer')
    with torch.no_grad():
        run.model.norm_weight[0][:, :128].mul_(1.5)
        run.model.norm_bias[0].add_(0.25)
    path = os.path.join(str(tmp_path), 'ckpt')
    save_model(run.model, run.config, path)
    with open(os.path.join(path, 'config.pkl'), 'rb') as f:
        assert pickle.load(f)['gnn_norm'] == 'layer'
    run2 = KGWAS(tiny, device='cpu', seed=2)
    run2.load_pretrained(path)
    assert run2.config == run.config and run2.model.gnn_norm == 'layer'
    a, b = run.model.state_dict(), run2.model.state_dict()
    assert list(a) == list(b)
    for k in a:
        if not isinstance(a[k], torch.nn.parameter.UninitializedParameter):
            assert torch.equal(a[k], b[k]), k


def test_state_dict_keys(tiny):
    """A default model's keys are what they were; a normed one adds ``norms.<l>.<node type>.weight|bias`` at the model's own width,
    for every node type that is the destination of a relation, after the keys it had.  The packed tensors keep their pad columns
    and the rows of other types zero; loading refuses a wrong shape and reports a missing key."""
    from kgwas_amd.model import HeteroGNN
    dims = (tiny.snp_init_dim_size, tiny.gene_init_dim_size, tiny.go_init_dim_size)
    torch.manual_seed(0)
    plain = HeteroGNN(tiny.data, 100, 1, 3, 'GAT', 'sum', *dims, 1)
    torch.manual_seed(0)
    normed = HeteroGNN(tiny.data, 100, 1, 3, 'GAT', 'sum', *dims, 1, gnn_norm='layer')
    kp, kn = list(plain.state_dict()), list(normed.state_dict())
    assert not any(k.startswith('norms.') for k in kp) and kn[:len(kp)] == kp
    assert len(list(plain.parameters())) + 4 == len(list(normed.parameters()))
    dst_types = sorted({et[2] for et in normed.edge_types})
    extra = kn[len(kp):]
    assert sorted(extra) == sorted(f'norms.{l}.{t}.{f}' for l in (0, 1) for t in dst_types for f in ('weight', 'bias'))
    sd = normed.state_dict()
    for k in extra:
        assert tuple(sd[k].shape) == (100,) and float(sd[k][0]) == (1.0 if k.endswith('weight') else 0.0)
    # the other parameters are initialised as in the plain model: the norm draws nothing
    for k in kp:
        if not isinstance(sd[k], torch.nn.parameter.UninitializedParameter):
            assert torch.equal(sd[k], plain.state_dict()[k]), k
    for w, b in zip([p.detach() for p in normed.norm_weight], [p.detach() for p in normed.norm_bias]):
        assert tuple(w.shape) == (len(normed.node_types), 128) and float(w[:, 100:].abs().sum()) == 0.0 == float(b.abs().sum())
        for t, name in enumerate(normed.node_types):
            assert float(w[t, :100].sum()) == (100.0 if name in dst_types else 0.0)
    assert sorted(k for k in normed.named_reference_tensors() if k.startswith('norms.')) == sorted(extra)
    assert all(v is None for k, v in normed.named_reference_tensors(grad=True).items() if k.startswith('norms.'))
    # round trip, shape check, missing key
    sd[extra[0]] = sd[extra[0]] * 3.0
    normed.load_state_dict(sd)
    assert torch.equal(normed.state_dict()[extra[0]], sd[extra[0]])
    assert float(normed.norm_weight[0].detach()[:, 100:].abs().sum()) == 0.0
    bad = dict(sd)
    bad[extra[0]] = torch.zeros(128)
    with pytest.raises(RuntimeError, match='shape'):
        normed.load_state_dict(bad)
    del bad[extra[0]]
    with pytest.raises(RuntimeError, match='missing'):
        normed.load_state_dict(bad)
    assert extra[0] in normed.load_state_dict(bad, strict=False).missing_keys
    with pytest.raises(RuntimeError, match='unexpected'):
        plain.load_state_dict(sd)
