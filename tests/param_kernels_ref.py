"""Plain float64 references of the parameter-only kernels of a step (kgwas_amd/csrc/kgw_dense_relvec.h: k_relvec_fwd, k_relvec_bwd,
k_param_tail; kgw_fold.hip: k_fold_fwd, k_fold_bwd; kgw_riders.h) and the error measure tests/test_gpu_param_kernels.py holds them
to.  No GPU code: torch float64 on the CPU, on the packed layout w_t[i][k][c] = W_i[c][k].

  relvec   U[r][k] = sum_c w_src_t[i][k][c] att_src[i][c], i = the packed slot of relation id r          (kgwas/conv.py:138-151)
           V[r | i][k] = sum_c wv_i[k][c] att_dst[i][c], wv_i = w_dst_t[bip_pos[i]] if bip_pos[i] >= 0 else w_src_t[i]
           rows of relations outside the pack are zero; bias_sum[b] = sum of bias[i] over blk_of_live[i] == b
  fold     tests.helpers.fold_fc_output_reference (kgwas/model.py:15,21 folded into layer 1), any number of MLPs

The backward passes are float64 AUTOGRAD of those two forwards (no second hand-written formula), a gradient that arrived by
another path (dw_src_acc) added to the result.

The scale S of every element is the MAGNITUDE PASS: the same float64 graph run on the absolute values of every input and every
upstream gradient.  Every operation here is a sum of products with plus signs only, so the pass returns exactly sum |terms| of
each forward value and its autograd exactly sum |terms| of each gradient -- what every rounding-error bound of a sum is relative
to.  An element whose scale is zero (a dead relation's row, an MLP no relation touches) has no rounding to forgive and must be
exactly 0.0."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.helpers import fold_fc_output_reference

C = 128
U = 2.0 ** -24                                          # unit round-off of fp32


class Layout:
    """n packed relations of n_rels: slot i is relation id rel_ids[i], bipartite with its destination weights at w_dst_t[bip_pos[i]]
    (bip_pos[i] >= 0) or same-type (-1), source / destination node type served by MLP src_m[i] / dst_m[i] of n_mlp."""

    def __init__(self, name, n_rels, rel_ids, bip_pos, src_m, dst_m, n_mlp):
        self.name, self.n_rels, self.n, self.n_mlp = name, n_rels, len(rel_ids), n_mlp
        self.rel_ids, self.bip_pos, self.src_m, self.dst_m = list(rel_ids), list(bip_pos), list(src_m), list(dst_m)
        assert len(set(self.rel_ids)) == self.n and all(0 <= r < n_rels for r in self.rel_ids)
        assert len(self.bip_pos) == len(self.src_m) == len(self.dst_m) == self.n
        pos = sorted(j for j in self.bip_pos if j >= 0)
        self.n_bip = len(pos)
        assert pos == list(range(self.n_bip))
        assert all(0 <= m < n_mlp for m in self.src_m + self.dst_m)
        self.live_of_rel = [-1] * n_rels
        for i, r in enumerate(self.rel_ids):
            self.live_of_rel[r] = i
        self.dead = [r for r in range(n_rels) if self.live_of_rel[r] < 0]

    def n_src(self, m):
        return sum(1 for x in self.src_m if x == m)

    def n_dst(self, m):
        return sum(1 for x in self.dst_m if x == m)

    def __repr__(self):
        return self.name


def _positions(flags, order=None):
    """bip_pos of the slots whose flag is set: 0, 1, ... in slot order, or in the given order of the bipartite slots."""
    k = sum(1 for f in flags if f)
    order = list(range(k)) if order is None else list(order)
    it = iter(order)
    return [next(it) if f else -1 for f in flags]


def _layouts():
    out = {}
    out['L1'] = Layout('L1', 1, [0], [-1], [0], [0], 1)
    ids = [3, 4, 5, 9, 10, 11, 12, 0, 1, 2, 20, 21, 28]                        # tests/test_gpu_fold.py
    sm, dm = [r % 3 for r in ids], [(r * 2) % 3 for r in ids]
    out['L2'] = Layout('L2', 29, ids, _positions([s != d for s, d in zip(sm, dm)]), sm, dm, 3)
    # 64 of 64: relation ids a fixed permutation of the slots; MLPs 0..3 the source of 17, 8, 39 and 0 relations, scattered over
    # the slots; MLP 3 a destination only; bipartite where the two MLPs differ, their w_dst_t positions shuffled
    ids = [(27 * i + 5) % 64 for i in range(64)]
    pool = [0] * 17 + [1] * 8 + [2] * 39
    sm = [pool[(37 * i + 11) % 64] for i in range(64)]
    dm = [i % 4 for i in range(64)]
    flags = [s != d for s, d in zip(sm, dm)]
    order = np.random.RandomState(3).permutation(sum(flags)).tolist()
    out['L3'] = Layout('L3', 64, ids, _positions(flags, order), sm, dm, 4)
    assert [out['L3'].n_src(m) for m in range(4)] == [17, 8, 39, 0] and out['L3'].n_dst(3) == 16
    assert 0 < out['L3'].n_bip < 64 and order != sorted(order)                 # (bip_pos not monotone in the slot)
    ids = [39 - 4 * i for i in range(9)]                                        # descending; all bipartite; MLP 2 untouched
    out['L4'] = Layout('L4', 40, ids, list(range(9)), [i % 2 for i in range(9)], [(i + 1) % 2 for i in range(9)], 3)
    out['L5'] = Layout('L5', 8, list(range(8)), [-1] * 8, [i % 2 for i in range(8)], [i % 2 for i in range(8)], 2)
    return out


LAYOUTS = _layouts()


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().double().cpu()


# ---- the two forwards (differentiable) ------------------------------------------------------------------------------------------

def relvec(lay, w_src_t, w_dst_t, att_src, att_dst):
    """(U_full [n_rels, C] by relation id, V [n_rels, C] by relation id, V [n, C] by packed slot)."""
    u = torch.einsum('ikc,ic->ik', w_src_t, att_src)
    wv = torch.stack([w_dst_t[j] if j >= 0 else w_src_t[i] for i, j in enumerate(lay.bip_pos)])
    v = torch.einsum('ikc,ic->ik', wv, att_dst)
    ids = torch.as_tensor(lay.rel_ids, dtype=torch.long)
    z = torch.zeros(lay.n_rels, C, dtype=u.dtype)
    return z.index_copy(0, ids, u), z.index_copy(0, ids, v), v


def bias_sums(bias, blk_of_live, n_blk):
    """(bias_sum [n_blk, C], its scale): entries -1 of blk_of_live belong to no block."""
    bias = _d(bias)
    out, s = torch.zeros(n_blk, C, dtype=torch.float64), torch.zeros(n_blk, C, dtype=torch.float64)
    for i, b in enumerate(blk_of_live):
        if 0 <= b < n_blk:
            out[b] += bias[i]
            s[b] += bias[i].abs()
    return out, s


def fold(lay, w_src_t, Uf, Vf, fcw, fcb):
    """(U', V', kappa by relation id; W', gamma by packed slot) from U, V [n_rels, C] by relation id, FC_output.weight
    fcw [n_mlp, C out, C in] and .bias fcb [n_mlp, C]."""
    pack = SimpleNamespace(rel_ids_t=torch.as_tensor(lay.rel_ids, dtype=torch.long), w_src_t=w_src_t)
    sm, dm = torch.as_tensor(lay.src_m, dtype=torch.long), torch.as_tensor(lay.dst_m, dtype=torch.long)
    return fold_fc_output_reference(pack, Uf, Vf, fcw.transpose(1, 2), fcb, sm, dm)


# ---- value + scale, forward and backward ----------------------------------------------------------------------------------------

def forward_with_scale(fn, inputs):
    """fn(*inputs) -> tuple of tensors, in float64; returns (values, scales): scales = fn on the absolute values."""
    x = [_d(t) for t in inputs]
    with torch.no_grad():
        return tuple(fn(*x)), tuple(fn(*[t.abs() for t in x]))


def backward_with_scale(fn, inputs, upstream, add=None):
    """Gradients of sum_o <fn(*inputs)[o], upstream[o]> with respect to every input by float64 autograd, plus add[k] (a gradient
    of input k that arrived by another path; None = none), and their scales: the same on absolute values.  upstream[o] None:
    that output has no gradient."""
    add = [None] * len(inputs) if add is None else list(add)

    def once(absolute):
        f = (lambda t: t.abs()) if absolute else (lambda t: t)
        x = [f(_d(t)).clone().requires_grad_(True) for t in inputs]
        outs = fn(*x)
        assert len(outs) == len(upstream)
        loss = sum((o * f(_d(g))).sum() for o, g in zip(outs, upstream) if g is not None)
        if not torch.is_tensor(loss):
            return [torch.zeros_like(t) if a is None else f(_d(a)) for t, a in zip(x, add)]
        gr = torch.autograd.grad(loss, x, allow_unused=True)
        gr = [torch.zeros_like(t) if g is None else g for t, g in zip(x, gr)]
        return [g if a is None else g + f(_d(a)) for g, a in zip(gr, add)]
    return once(False), once(True)


def relvec_fwd_ref(lay, w_src_t, w_dst_t, att_src, att_dst):
    """((U_full, V by relation id, V by slot), their scales)."""
    return forward_with_scale(lambda a, b, c, d: relvec(lay, a, b, c, d), (w_src_t, w_dst_t, att_src, att_dst))


def relvec_bwd_ref(lay, w_src_t, w_dst_t, att_src, att_dst, dU_full, dV, v_by_rel, dw_src_acc=None):
    """((d w_src_t, d w_dst_t, d att_src, d att_dst), their scales) from dU_full [n_rels, C] and dV ([n_rels, C] by relation id
    when v_by_rel else [n, C] by slot); either may be None (zero)."""
    up = (dU_full, dV if v_by_rel else None, None if v_by_rel else dV)
    return backward_with_scale(lambda a, b, c, d: relvec(lay, a, b, c, d), (w_src_t, w_dst_t, att_src, att_dst), up,
                               add=(dw_src_acc, None, None, None))


def fold_fwd_ref(lay, w_src_t, Uf, Vf, fcw, fcb):
    """((U', V', kappa, W', gamma), their scales)."""
    return forward_with_scale(lambda a, b, c, d, e: fold(lay, a, b, c, d, e), (w_src_t, Uf, Vf, fcw, fcb))


def fold_bwd_ref(lay, w_src_t, Uf, Vf, fcw, fcb, dUp, dVp, dkappa, dWp, dgamma):
    """((dws, dU, dV, d fcw [n_mlp, C, C], d fcb [n_mlp, C]), their scales)."""
    return backward_with_scale(lambda a, b, c, d, e: fold(lay, a, b, c, d, e), (w_src_t, Uf, Vf, fcw, fcb),
                               (dUp, dVp, dkappa, dWp, dgamma))


def chain(lay, w_src_t, w_dst_t, att_src, att_dst, fcw, fcb):
    """relvec then fold on its vectors: (U', V', kappa, W', gamma) as functions of the parameters alone."""
    Uf, Vf, _ = relvec(lay, w_src_t, w_dst_t, att_src, att_dst)
    return fold(lay, w_src_t, Uf, Vf, fcw, fcb)


# ---- number of products in one element's sum (the derived bar is (n_terms + 2) 2^-24 S) ---------------------------------------

N_TERMS = dict(U=128, V=128, Up=128, Vp=128, Wp=128, gamma=128, datt_src=128, datt_dst=128, kappa=256, fold_dU=129, fold_dV=129,
               dw_src_t=3, dw_dst_t=1, fold_dws=129)


def n_terms_fc(lay, m):
    """d FC_output.weight_m and d FC_output.bias_m: a 128-term product per source relation and a rank-1 term per source and per
    destination relation."""
    return 128 * lay.n_src(m) + lay.n_src(m) + lay.n_dst(m)


def err_in_u(got, ref, scale):
    """max |got - ref| / (2^-24 scale) over every element.  Where scale == 0 the element must be exactly 0.0 (AssertionError
    otherwise: no division, no tolerance).  A non-finite `got` gives inf."""
    got, ref, scale = _d(got), _d(ref), _d(scale)
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    zero = scale == 0
    if bool(zero.any()):
        bad = zero & ((got != 0) | (ref != 0))
        assert not bool(bad.any()), f'{int(bad.sum())} elements of scale 0 are not exactly 0.0'
    err = (got - ref).abs() / torch.where(zero, torch.ones_like(scale), scale)
    return float(torch.where(zero, torch.zeros_like(err), err).max()) / U
