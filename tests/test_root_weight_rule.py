"""CPU: the root-weight rule (kgwroot_* in include/kgwas_hip.h, restated in float64 by tests/root_weight_ref.py), the C ABI's
refusals by value, and the host side of HeteroGNN(gnn_root_weight=True) / KGWAS.initialize_model(gnn_root_weight=True):
validation, config, checkpoints, state_dict keys and the order the parameters are drawn in.  No kernel is launched."""
import ctypes as C
import math
import os
import pickle

import numpy as np
import pytest
import torch

from tests import root_weight_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('x_premasked', [False, True])
def test_closed_form_backward_equals_autograd(masked, x_premasked):
    """(dy, dx, dW) of tests/root_weight_ref.backward against float64 autograd of its forward.  ``masked``: the gradient handed in
    already carries (out > 0) -- the consumer's half of the ReLU's backward -- so autograd goes through the pre-activation alone;
    ``x_premasked``: x is itself a ReLU output whose producer expects its gradient multiplied by (x > 0) by whoever consumes x, so
    the product of the rule with that mask is the gradient of the PRE-ReLU state x came from."""
    rows, n = 37, 24
    y, W, g = _rand((rows, n), 1), _rand((n, n), 2, 0.3), _rand((rows, n), 3)
    pre_x = _rand((rows, n), 4)
    yl, Wl, pl = (t.clone().requires_grad_(True) for t in (y, W, pre_x))
    x = torch.relu(pl) if x_premasked else pl
    out = R.forward(yl, x, Wl, relu=True)
    assert 0.2 < float((out > 0).double().mean()) < 0.8
    up = g * (out.detach() > 0) if masked else g
    pre = yl + x @ Wl.t()
    (pre if masked else out).backward(up)
    dy, dx, dW = R.backward(up, out.detach(), x.detach(), W, masked=masked, x_premasked=x_premasked)
    assert torch.allclose(dy, yl.grad, rtol=1e-12, atol=1e-14)
    assert torch.allclose(dx, pl.grad, rtol=1e-12, atol=1e-14)
    assert torch.allclose(dW, Wl.grad, rtol=1e-12, atol=1e-14)
    # without a ReLU the rule is the plain Linear's
    out2 = R.forward(y, pre_x, W, relu=False)
    assert torch.equal(out2, y + pre_x @ W.t())
    dy2, dx2, dW2 = R.backward(g, out2, pre_x, W, masked=True)
    assert torch.equal(dy2, g) and torch.allclose(dx2, g @ W) and torch.allclose(dW2, g.t() @ pre_x)


def test_header_names_the_rule():
    hdr = open(os.path.join(ROOT, 'include', 'kgwas_hip.h')).read()
    for name in ('kgwroot_out', 'kgwroot_mask', 'KgwRootJob', 'KgwRootBwdJob', 'int kgw_root_linear_fwd(', 'int kgw_root_linear_bwd(',
                 'dst_n = act(y_n + sum_k x_k W[n][k])', 'x_premasked'):
        assert name in hdr, name
    assert hdr.index('int kgw_layer_norm_fold(') < hdr.index('KgwRootJob') < hdr.index('int kgw_gat_aggregate_fwd')
    assert '#define KGW_VERSION      125' in hdr
    integ = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert '`kgw_root_linear_fwd`' in integ and '`kgw_root_linear_bwd`' in integ


def test_symbol_binding_and_struct_sizes():
    from kgwas_amd import _lib
    L = _lib.lib()
    assert _lib.has_root_weight() and L.kgw_version() == 125
    for name in ('kgw_root_linear_fwd', 'kgw_root_linear_bwd'):
        assert hasattr(L, name) and name in _lib.EXPORTS
    j, k = _lib.KgwRootJob, _lib.KgwRootBwdJob
    assert C.sizeof(j) == 64 and (j.x.offset, j.ldx.offset, j.y.offset, j.ldy.offset, j.dst.offset, j.ldd.offset, j.rows.offset,
                                  j.type.offset, j.W.offset) == (0, 8, 16, 24, 32, 40, 48, 52, 56)
    assert C.sizeof(k) == 104 and (k.g.offset, k.out.offset, k.x.offset, k.gm.offset, k.dx.offset, k.rows.offset, k.type.offset,
                                   k.W.offset, k.x_premasked.offset) == (0, 16, 32, 48, 64, 80, 84, 88, 96)
    # no struct of the existing ABI changed
    s8 = (C.c_int64 * 8)()
    assert L.kgw_struct_sizes(s8, 8) == 0 and s8[4] == C.sizeof(_lib.KgwLayerArgs) and s8[7] == C.sizeof(_lib.KgwEdgeAttr)
    assert C.sizeof(_lib.KgwLNormJob) == 64 and C.sizeof(_lib.KgwLNormBwdJob) == 88


def test_refusals_by_value_before_any_launch():
    """Every call here is refused (or has no rows) before a kernel could be launched: the pointers are host memory or NULL."""
    from kgwas_amd import _lib
    L = _lib.lib()
    E_NULL, E_RANGE, E_UNSUPPORTED = -1, -2, _lib.KGW_E_UNSUPPORTED
    buf = np.zeros(3 * 16 * 128 + 128 * 128 + 8, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16                     # 16-byte aligned host addresses
    q, r, w = p + 16 * 128 * 4, p + 2 * 16 * 128 * 4, p + 3 * 16 * 128 * 4

    def fjob(rows=4, x=p, y=q, dst=r, ldx=128, ldy=128, ldd=128, t=0, W=w):
        j = _lib.KgwRootJob()
        j.x, j.ldx, j.y, j.ldy, j.dst, j.ldd, j.rows, j.type, j.W = x, ldx, y, ldy, dst, ldd, rows, t, W
        return j

    def fwd(jobs, n=None, relu=1):
        arr = (_lib.KgwRootJob * max(1, len(jobs)))(*jobs)
        return L.kgw_root_linear_fwd(len(jobs) if n is None else n, arr, relu, None)

    assert L.kgw_root_linear_fwd(1, None, 1, None) == E_NULL
    for kw in (dict(x=None), dict(y=None), dict(dst=None), dict(W=None)):
        assert fwd([fjob(**kw)]) == E_NULL, kw
    assert fwd([fjob()], n=0) == E_RANGE and fwd([fjob()] * 8, n=9) == E_RANGE and fwd([fjob()], n=-1) == E_RANGE
    assert fwd([fjob(rows=-1)]) == E_RANGE and fwd([fjob(rows=(1 << 25) + 1)]) == E_RANGE
    for kw in (dict(ldx=64), dict(ldy=124), dict(ldd=0), dict(t=8), dict(t=-1)):
        assert fwd([fjob(**kw)]) == E_RANGE, kw
    assert fwd([fjob(t=2), fjob(t=2)]) == E_RANGE                       # a type named twice
    for kw in (dict(x=p + 4), dict(y=q + 8), dict(dst=r + 4), dict(W=w + 8), dict(ldx=130), dict(ldy=258), dict(ldd=129), dict(dst=q),
               dict(dst=p)):
        assert fwd([fjob(**kw)]) == E_UNSUPPORTED, kw
    assert fwd([fjob(), fjob(t=1, ldx=130)]) == E_UNSUPPORTED           # any job of the list
    assert fwd([fjob(rows=0), fjob(rows=0, t=1, x=None, y=None, dst=None, W=None)]) == 0       # no rows: KGW_OK, no launch

    def bjob(rows=4, g=p, out=None, x=None, gm=None, dx=r, t=0, W=w, ld=128, xp=0):
        j = _lib.KgwRootBwdJob()
        j.g, j.ldg, j.out, j.ldo, j.x, j.ldx, j.gm, j.ldgm, j.dx, j.lddx = g, ld, out, ld, x, ld, gm, ld, dx, ld
        j.rows, j.type, j.W, j.x_premasked = rows, t, W, xp
        return j

    def bwd(jobs, n=None):
        arr = (_lib.KgwRootBwdJob * max(1, len(jobs)))(*jobs)
        return L.kgw_root_linear_bwd(len(jobs) if n is None else n, arr, None)

    assert L.kgw_root_linear_bwd(1, None, None) == E_NULL
    for kw in (dict(g=None), dict(dx=None), dict(W=None), dict(xp=1, x=None)):
        assert bwd([bjob(**kw)]) == E_NULL, kw
    assert bwd([bjob()], n=0) == E_RANGE and bwd([bjob()] * 8, n=9) == E_RANGE
    assert bwd([bjob(rows=-1)]) == E_RANGE and bwd([bjob(rows=(1 << 25) + 1)]) == E_RANGE and bwd([bjob(ld=64)]) == E_RANGE
    assert bwd([bjob(t=8)]) == E_RANGE and bwd([bjob(t=-1)]) == E_RANGE and bwd([bjob(t=2), bjob(t=2)]) == E_RANGE
    for kw in (dict(g=p + 4), dict(out=q + 4), dict(dx=r + 8), dict(W=w + 4), dict(gm=q + 4, out=q), dict(xp=1, x=q + 4), dict(ld=130),
               dict(dx=p), dict(out=q, gm=p), dict(out=q, dx=q), dict(out=q, gm=q), dict(out=q, gm=r), dict(xp=1, x=q, dx=q),
               dict(xp=1, x=q, out=w, gm=q)):
        assert bwd([bjob(**kw)]) == E_UNSUPPORTED, kw
    assert bwd([bjob(rows=0), bjob(rows=0, t=1, g=None, dx=None, W=None)]) == 0


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path_factory.mktemp('root')))


def test_construction_and_refusals(tiny):
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.model import HeteroGNN
    run = KGWAS(tiny, device='cpu', seed=1)
    with pytest.raises(ValueError, match='gnn_root_weight'):
        run.initialize_model(gnn_backbone='SAGE', gnn_root_weight=True)
    dims = (tiny.snp_init_dim_size, tiny.gene_init_dim_size, tiny.go_init_dim_size)
    with pytest.raises(ValueError, match='gnn_root_weight'):
        HeteroGNN(tiny.data, 128, 1, 2, 'SAGE', 'sum', *dims, 1, gnn_root_weight=True)
    with pytest.raises(TypeError):                                           # keyword only
        HeteroGNN(tiny.data, 128, 1, 2, 'GAT', 'sum', *dims, 1, False, 0.0, False, True)
    run.initialize_model(gnn_backbone='SAGE')                                # (SAGE without it: as before)
    for kw in ({'gnn_aggr': 'mean'}, {'gnn_aggr': 'min'}, {'gnn_aggr': 'max'}, {'gat_num_head': 2}, {'gat_num_head': 4}, {'gat_sigmoid': True},
               {'gat_temperature': 2.0}, {'gat_dropout': 0.1}, {'gnn_dropout': 0.2}, {'gnn_norm': 'layer'}, {'gnn_num_layers': 1},
               {'gnn_num_layers': 3}, {'gnn_hidden_dim': 100}, {'out_channels': 3}):
        run.initialize_model(gnn_root_weight=True, **kw)
        m = run.model
        assert m.gnn_root_weight and len(m.root_weight) == m.num_layers and not m.fold_fc
        assert all(tuple(w.shape) == (len(m.node_types), 128, 128) for w in m.root_weight)
    m.eval()
    assert m._root_site(1) is not None                                       # live in evaluation
    with pytest.raises(NotImplementedError, match='gnn_root_weight'):
        run.train(epoch=1, parallelism='shard')
    run.initialize_model()
    assert not run.model.gnn_root_weight and run.model._root_site(1) is None and len(run.model.root_weight) == 0 and run.model.fold_fc
    # the step stays under the fused optimiser launch's limit: L more trainable tensors
    from kgwas_amd import _lib
    run.initialize_model(gnn_root_weight=True, gnn_norm='layer')
    assert sum(1 for p in run.model.parameters() if p.requires_grad) <= _lib.ADAM_FUSED_MAX


def test_config_carries_the_key_only_when_on_and_a_checkpoint_round_trips(tiny, tmp_path):
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.utils import save_model
    run = KGWAS(tiny, device='cpu', seed=1)
    run.initialize_model()
    default = dict(run.config)
    assert sorted(default) == ['gat_num_head', 'gnn_aggr', 'gnn_backbone', 'gnn_hidden_dim', 'gnn_num_layers']
    run.initialize_model(gnn_root_weight=False)
    assert run.config == default
    run.initialize_model(gnn_root_weight=True, gnn_hidden_dim=100)
    assert run.config == dict(default, gnn_hidden_dim=100, gnn_root_weight=True)
    with torch.no_grad():
        run.model.root_weight[1].mul_(1.5)
    path = os.path.join(str(tmp_path), 'ckpt')
    save_model(run.model, run.config, path)
    with open(os.path.join(path, 'config.pkl'), 'rb') as f:
        assert pickle.load(f)['gnn_root_weight'] is True
    run2 = KGWAS(tiny, device='cpu', seed=2)
    run2.load_pretrained(path)
    assert run2.config == run.config and run2.model.gnn_root_weight
    a, b = run.model.state_dict(), run2.model.state_dict()
    assert list(a) == list(b) and any(k.startswith('roots.') for k in a)
    for k in a:
        if not isinstance(a[k], torch.nn.parameter.UninitializedParameter):
            assert torch.equal(a[k], b[k]), k
    for wa, wb in zip(run.model.root_weight, run2.model.root_weight):
        assert torch.equal(wa.detach(), wb.detach())


def test_state_dict_keys_and_the_order_of_the_draws(tiny):
    """A default model's keys are what they were and it draws nothing new; a root model adds ``roots.<l>.<node type>.weight``
    [hidden, hidden] at the model's own width for every layer and every node type that is the destination of a relation, after the
    keys it had, and its other parameters are those of a default model at the same seed (the roots are drawn last).  The packed
    tensors keep the padding and the slices of other types zero; loading refuses a wrong shape and reports a missing key."""
    from kgwas_amd.model import HeteroGNN
    dims = (tiny.snp_init_dim_size, tiny.gene_init_dim_size, tiny.go_init_dim_size)
    cl = 100
    torch.manual_seed(0)
    plain = HeteroGNN(tiny.data, cl, 1, 3, 'GAT', 'sum', *dims, 1)
    after_plain = torch.rand(1)
    torch.manual_seed(0)
    off = HeteroGNN(tiny.data, cl, 1, 3, 'GAT', 'sum', *dims, 1, gnn_root_weight=False)
    assert torch.equal(torch.rand(1), after_plain)                           # a default model draws nothing new
    torch.manual_seed(0)
    rooted = HeteroGNN(tiny.data, cl, 1, 3, 'GAT', 'sum', *dims, 1, gnn_root_weight=True)
    kp, kr = list(plain.state_dict()), list(rooted.state_dict())
    assert kp == list(off.state_dict()) and not any(k.startswith('roots.') for k in kp) and kr[:len(kp)] == kp
    assert len(list(plain.parameters())) + 3 == len(list(rooted.parameters()))
    dst_types = sorted({et[2] for et in rooted.edge_types})
    extra = kr[len(kp):]
    assert sorted(extra) == sorted(f'roots.{l}.{t}.weight' for l in (0, 1, 2) for t in dst_types)
    sd, sp = rooted.state_dict(), plain.state_dict()
    bound = math.sqrt(6.0 / (cl + cl))                                       # RelationPack's rule for lin_src
    for k in extra:
        assert tuple(sd[k].shape) == (cl, cl)
        assert 0.5 * bound < float(sd[k].abs().max()) <= bound and abs(float(sd[k].mean())) < 0.1 * bound
    for k in kp:
        if not isinstance(sd[k], torch.nn.parameter.UninitializedParameter):
            assert torch.equal(sd[k], sp[k]), k
    for w in (p.detach() for p in rooted.root_weight):
        assert tuple(w.shape) == (len(rooted.node_types), 128, 128)
        assert float(w[:, cl:, :].abs().sum()) == 0.0 == float(w[:, :, cl:].abs().sum())
        for t, name in enumerate(rooted.node_types):
            assert (float(w[t].abs().sum()) > 0) == (name in dst_types)
    assert sorted(k for k in rooted.named_reference_tensors() if k.startswith('roots.')) == sorted(extra)
    assert all(v is None for k, v in rooted.named_reference_tensors(grad=True).items() if k.startswith('roots.'))
    # round trip, shape check, missing key, unexpected key
    sd[extra[0]] = sd[extra[0]] * 3.0
    rooted.load_state_dict(sd)
    assert torch.equal(rooted.state_dict()[extra[0]], sd[extra[0]])
    assert float(rooted.root_weight[0].detach()[:, cl:, :].abs().sum()) == 0.0
    bad = dict(sd)
    bad[extra[0]] = torch.zeros(128, 128)
    with pytest.raises(RuntimeError, match='shape'):
        rooted.load_state_dict(bad)
    del bad[extra[0]]
    with pytest.raises(RuntimeError, match='missing'):
        rooted.load_state_dict(bad)
    assert extra[0] in rooted.load_state_dict(bad, strict=False).missing_keys
    with pytest.raises(RuntimeError, match='unexpected'):
        plain.load_state_dict(sd)


def test_documents_name_the_feature():
    readme = open(os.path.join(ROOT, 'README.md')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'gnn_root_weight=True' in readme and 'tools/bench_root_weight.py' in readme
    assert '**Root weight**' in design and 'kgw_root_linear_fwd' in design and 'profiles/root_weight/' in design
