"""The float64 references tests/test_gpu_param_kernels.py compares the relation-vector, fold and param-tail kernels with
(tests/param_kernels_ref.py), checked on the CPU against what they restate: an unpacked, relation-by-relation statement of
kgwas/conv.py:138-151 and kgwas/model.py:15,21 with the reference model's own names (W[c][k] = Linear.weight, att) under float64
autograd; and the properties of the magnitude pass the derived bar rests on."""
import pytest
import torch

from tests import param_kernels_ref as R

C = R.C
NAMES_FOLD = ('Up', 'Vp', 'kappa', 'Wp', 'gamma')


def _case(lay, seed):
    g = torch.Generator().manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)
    P = dict(w_src_t=rn(lay.n, C, C), w_dst_t=rn(lay.n_bip, C, C), att_src=rn(lay.n, C), att_dst=rn(lay.n, C),
             fcw=rn(lay.n_mlp, C, C), fcb=rn(lay.n_mlp, C))
    up = dict(Up=rn(lay.n_rels, C), Vp=rn(lay.n_rels, C), kappa=rn(lay.n_rels), Wp=rn(lay.n, C, C), gamma=rn(lay.n, C))
    return P, up, rn(lay.n, C, C)


def _unpacked(lay, P, up, signs=True):
    """Relation by relation, Linear weights as the reference model keeps them ([out c][in k]): the gradients of
    sum <output, upstream> over U', V', kappa, W', gamma (and, with up_uv, over u_r, v_r themselves), returned in the packed layout."""
    f = (lambda t: t) if signs else (lambda t: t.abs())
    lin_src = [f(P['w_src_t'][i]).t().clone().requires_grad_(True) for i in range(lay.n)]               # lin_src.weight [c][k]
    lin_dst = [f(P['w_dst_t'][j]).t().clone().requires_grad_(True) for j in range(lay.n_bip)]           # lin_dst.weight
    att_src = [f(P['att_src'][i]).clone().requires_grad_(True) for i in range(lay.n)]
    att_dst = [f(P['att_dst'][i]).clone().requires_grad_(True) for i in range(lay.n)]
    fc_w = [f(P['fcw'][m]).clone().requires_grad_(True) for m in range(lay.n_mlp)]                      # FC_output.weight [out][in]
    fc_b = [f(P['fcb'][m]).clone().requires_grad_(True) for m in range(lay.n_mlp)]
    loss = torch.zeros((), dtype=torch.float64)
    for i, r in enumerate(lay.rel_ids):
        Ws = lin_src[i]
        Wd = lin_dst[lay.bip_pos[i]] if lay.bip_pos[i] >= 0 else Ws
        # alpha_src = (lin_src(x) * att_src).sum(-1) = <x, u>,  u = W^T att   (conv.py:138-151)
        u, v = att_src[i] @ Ws, att_dst[i] @ Wd
        ms, md = lay.src_m[i], lay.dst_m[i]
        # x = h2 FC_output.weight^T + FC_output.bias   (model.py:15,21):  <x, u> = <h2, weight^T u> + <bias, u>
        Up, Vp = fc_w[ms].t() @ u, fc_w[md].t() @ v
        kappa = fc_b[ms] @ u + fc_b[md] @ v
        # lin_src(x) = h2 (weight^T W^T) + bias W^T
        Wp, gamma = fc_w[ms].t() @ Ws.t(), fc_b[ms] @ Ws.t()
        for val, name, idx in ((Up, 'Up', r), (Vp, 'Vp', r), (kappa, 'kappa', r), (Wp, 'Wp', i), (gamma, 'gamma', i)):
            loss = loss + (val * f(up[name][idx])).sum()
    loss.backward()

    def grad(t):
        return torch.zeros_like(t) if t.grad is None else t.grad
    return dict(w_src_t=torch.stack([grad(w).t() for w in lin_src]),
                w_dst_t=torch.stack([grad(w).t() for w in lin_dst]) if lay.n_bip else torch.zeros(0, C, C, dtype=torch.float64),
                att_src=torch.stack([grad(a) for a in att_src]), att_dst=torch.stack([grad(a) for a in att_dst]),
                fcw=torch.stack([grad(w) for w in fc_w]), fcb=torch.stack([grad(b) for b in fc_b]))


def _two_stage(lay, P, up, acc=None):
    """The way the GPU module composes the references: the fold's backward, then the relation vectors' backward on its dU, dV
    with its dws (+ acc) as the gradient that arrived by another path.  Values and scales."""
    (Uf, Vf, _), _ = R.relvec_fwd_ref(lay, P['w_src_t'], P['w_dst_t'], P['att_src'], P['att_dst'])
    ups = [up[k] for k in NAMES_FOLD]
    (dws, dU, dV, dfcw, dfcb), (s_dws, s_dU, s_dV, s_fcw, s_fcb) = R.fold_bwd_ref(lay, P['w_src_t'], Uf, Vf, P['fcw'], P['fcb'], *ups)
    a = dws if acc is None else dws + acc
    g, _ = R.relvec_bwd_ref(lay, P['w_src_t'], P['w_dst_t'], P['att_src'], P['att_dst'], dU, dV, 1, a)
    # scales: the magnitude pass of the second stage on the magnitude pass of the first
    absP = {k: v.abs() for k, v in P.items()}
    (sUf, sVf, _) = R.relvec_fwd_ref(lay, P['w_src_t'], P['w_dst_t'], P['att_src'], P['att_dst'])[1]
    (_, _, _, _, _), (s_dws, s_dU, s_dV, s_fcw, s_fcb) = R.fold_bwd_ref(lay, absP['w_src_t'], sUf, sVf, absP['fcw'], absP['fcb'],
                                                                       *[u.abs() for u in ups])
    sa = s_dws if acc is None else s_dws + acc.abs()
    _, s = R.relvec_bwd_ref(lay, P['w_src_t'], P['w_dst_t'], P['att_src'], P['att_dst'], s_dU, s_dV, 1, sa)
    vals = dict(w_src_t=g[0], w_dst_t=g[1], att_src=g[2], att_dst=g[3], fcw=dfcw, fcb=dfcb)
    scales = dict(w_src_t=s[0], w_dst_t=s[1], att_src=s[2], att_dst=s[3], fcw=s_fcw, fcb=s_fcb)
    return vals, scales


@pytest.mark.parametrize('name', ['L1', 'L2', 'L3', 'L4', 'L5'])
def test_reference_backward_is_autograd_of_the_unpacked_statement(name):
    lay = R.LAYOUTS[name]
    P, up, acc = _case(lay, 10 + lay.n)
    vals, scales = _two_stage(lay, P, up, acc)
    want = _unpacked(lay, P, up)
    want['w_src_t'] = want['w_src_t'] + acc
    mag = _unpacked(lay, P, up, signs=False)                     # sum |terms| of the same statement
    mag['w_src_t'] = mag['w_src_t'] + acc.abs()
    for k in vals:
        S = scales[k]
        assert vals[k].shape == want[k].shape == S.shape, k
        if S.numel() == 0:
            continue
        assert bool(((vals[k] - want[k]).abs() <= 1e-12 * S).all()), (k, float((vals[k] - want[k]).abs().max()))
        assert bool(((S - mag[k]).abs() <= 1e-12 * mag[k]).all()), k          # the magnitude pass IS sum |terms|
        assert bool((S >= vals[k].abs()).all()), k                               # S >= |ref| everywhere
    # an MLP that no relation touches has no gradient and no scale: exactly zero
    for m in range(lay.n_mlp):
        if lay.n_src(m) + lay.n_dst(m) == 0:
            assert float(scales['fcw'][m].abs().max()) == 0.0 and float(scales['fcb'][m].abs().max()) == 0.0
            assert float(vals['fcw'][m].abs().max()) == 0.0 and float(vals['fcb'][m].abs().max()) == 0.0
        else:
            assert float(scales['fcw'][m].min()) > 0.0
    assert name != 'L4' or (lay.n_src(2) + lay.n_dst(2) == 0)


@pytest.mark.parametrize('name', ['L1', 'L2', 'L3', 'L4', 'L5'])
def test_forward_references_scales_and_dead_rows(name):
    lay = R.LAYOUTS[name]
    P, up, _ = _case(lay, 20 + lay.n)
    (Uf, Vr, Vs), (sU, sVr, sVs) = R.relvec_fwd_ref(lay, P['w_src_t'], P['w_dst_t'], P['att_src'], P['att_dst'])
    for i, r in enumerate(lay.rel_ids):                          # the unpacked statement, relation by relation
        W = P['w_src_t'][i].t()
        Wd = P['w_dst_t'][lay.bip_pos[i]].t() if lay.bip_pos[i] >= 0 else W
        assert torch.allclose(Uf[r], P['att_src'][i] @ W, rtol=0, atol=1e-12 * float(sU[r].max()))
        assert torch.allclose(Vr[r], P['att_dst'][i] @ Wd, rtol=0, atol=1e-12 * float(sVr[r].max()))
        assert torch.equal(Vs[i], Vr[r]) and torch.equal(sVs[i], sVr[r])
    fo, fs = R.fold_fwd_ref(lay, P['w_src_t'], Uf, Vr, P['fcw'], P['fcb'])
    for val, S in list(zip((Uf, Vr, Vs), (sU, sVr, sVs))) + list(zip(fo, fs)):
        assert bool((S >= val.abs()).all())
    for r in lay.dead:                                           # S == 0 exactly on dead rows
        for S in (sU, sVr, fs[0], fs[1]):
            assert float(S[r].abs().max()) == 0.0
        assert float(fs[2][r]) == 0.0
    live = torch.as_tensor(lay.rel_ids)
    assert float(sU[live].min()) > 0.0 and float(fs[2][live].min()) > 0.0
    # the backward of a dead row: no gradient reaches anything
    dU = torch.zeros(lay.n_rels, C, dtype=torch.float64)
    if lay.dead:
        dU[lay.dead] = 1.0
    g, s = R.relvec_bwd_ref(lay, P['w_src_t'], P['w_dst_t'], P['att_src'], P['att_dst'], dU, dU, 1)
    assert all(float(t.abs().sum()) == 0.0 for t in g + s)


def test_magnitude_pass_of_a_sum_of_graphs_is_the_sum_of_the_passes():
    """dw_src_acc: the gradient of w_src_t is (relvec's share) + (what arrived by another path); its scale is the sum of the two
    scales.  And the whole chain relvec -> fold in ONE graph has the scales of the two stages composed."""
    lay = R.LAYOUTS['L2']
    P, up, acc = _case(lay, 7)
    g = torch.Generator().manual_seed(8)
    dU, dV = torch.randn(lay.n_rels, C, generator=g, dtype=torch.float64), torch.randn(lay.n_rels, C, generator=g, dtype=torch.float64)
    a = (P['w_src_t'], P['w_dst_t'], P['att_src'], P['att_dst'])
    g0, s0 = R.relvec_bwd_ref(lay, *a, dU, dV, 1)
    g1, s1 = R.relvec_bwd_ref(lay, *a, dU, dV, 1, acc)
    assert torch.allclose(g1[0], g0[0] + acc, rtol=0, atol=1e-13 * float(s1[0].max()))
    assert torch.allclose(s1[0], s0[0] + acc.abs(), rtol=1e-14, atol=0)
    for k in (1, 2, 3):
        assert torch.equal(g1[k], g0[k]) and torch.equal(s1[k], s0[k])
    # by slot and by relation id are the same gradient
    g2, s2 = R.relvec_bwd_ref(lay, *a, dU, dV[lay.rel_ids], 0)
    assert all(torch.equal(x, y) for x, y in zip(g0 + s0, g2 + s2))
    # one graph for the chain against the two stages
    vals, scales = _two_stage(lay, P, up)
    ups = [up[k] for k in NAMES_FOLD]
    fn = lambda *x: R.chain(lay, *x)
    gc, sc = R.backward_with_scale(fn, a + (P['fcw'], P['fcb']), ups)
    for k, x, s in zip(('w_src_t', 'w_dst_t', 'att_src', 'att_dst', 'fcw', 'fcb'), gc, sc):
        assert torch.allclose(vals[k], x, rtol=0, atol=1e-12 * float(s.max())), k
        assert torch.allclose(scales[k], s, rtol=1e-12, atol=0), k


def test_bias_sums_and_err_in_u():
    g = torch.Generator().manual_seed(3)
    bias = torch.randn(5, C, generator=g)
    out, s = R.bias_sums(bias, [2, -1, 0, 2, 7], 3)
    assert torch.equal(out[2], (bias[0].double() + bias[3].double())) and torch.equal(out[0], bias[2].double())
    assert float(out[1].abs().max()) == 0.0 and float(s[1].abs().max()) == 0.0 and bool((s >= out.abs()).all())
    ref, S = torch.tensor([1.0, 0.0, 2.0]), torch.tensor([2.0, 0.0, 4.0])
    assert R.err_in_u(ref + torch.tensor([2 * R.U, 0.0, 0.0]), ref, S) == pytest.approx(1.0)
    assert R.err_in_u(torch.tensor([1.0, float('nan'), 2.0]), ref, S) == float('inf')
    with pytest.raises(AssertionError):
        R.err_in_u(torch.tensor([1.0, 1e-30, 2.0]), ref, S)       # no scale: exactly zero or nothing
    assert R.n_terms_fc(R.LAYOUTS['L3'], 0) == 128 * 17 + 17 + 16 and R.n_terms_fc(R.LAYOUTS['L4'], 2) == 0
