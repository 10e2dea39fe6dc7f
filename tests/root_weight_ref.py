"""float64 statement of the root-weight rule of kgw_root_linear_fwd / kgw_root_linear_bwd (HeteroGNN(gnn_root_weight=True)),
restated from include/kgwas_hip.h:

    dst = act(y + x W^T)                       W [out, in], act = max(0, .) iff relu
    gm  = g * (out > 0)  unless ``masked``     (g arrives masked, or no ReLU was applied)
    dx  = gm W           times (x > 0) under ``x_premasked``
    dy  = gm             dW = gm^T x

and the float64 oracle of a model with root weights: y_i = combine_r(conv_r(...)_i) + W_root[l][t] x_i for every layer l and every
destination type t, x_i the node's own layer-l input; then the norm (tests/layer_norm_ref.py), the ReLU and the dropout factor
(tests/hidden_dropout_ref.py) as before.  Nothing here calls the package."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.layer_norm_ref import NormedStateOracle

C = 128


def forward(y, x, W, relu=True):
    """dst [rows, n] for y [rows, n], x [rows, k], W [n, k], in the arguments' dtype."""
    v = y + x @ W.t()
    return torch.relu(v) if relu else v


def backward(g, out, x, W, masked=False, x_premasked=False):
    """The closed form: (dy, dx, dW) for the upstream gradient ``g`` of dst.  ``masked``: g is used as it is (it already carries
    (out > 0), or the forward applied no ReLU); ``x_premasked``: dx is multiplied by (x > 0)."""
    gm = g if masked else g * (out > 0).to(g.dtype)
    dx = gm @ W
    if x_premasked:
        dx = dx * (x > 0).to(g.dtype)
    return gm, dx, gm.t() @ x


class RootedOracle(NormedStateOracle):
    """HeteroGNNOracle (through NormedStateOracle, whose norms may be absent) with  y[t] += x[t] W_root[l][t]^T  on the
    pre-activation of EVERY layer: ``roots[l - 1][node type]`` = float64 [hidden, hidden] in nn.Linear layout for l = 1 .. L, x the
    layer's own input of that type (the oracle computes every row of every type, so x[t] and y[t] have the same rows).  The order
    is conv + root -> norm -> ReLU -> dropout factor.  ``edge_attr_dict`` is handed to a HeteroConv oracle that takes one
    (tests/edge_attr_ref.py)."""

    @classmethod
    def adopt(cls, oracle, root_tensors, norm_tensors=None, state_factor=None):
        """``root_tensors``: {'roots.<l>.<type>.weight': tensor}, ``norm_tensors``: {'norms.<l>.<type>.weight|bias': tensor} (the
        product's state_dict entries)."""
        NormedStateOracle.adopt(oracle, norm_tensors or {}, state_factor)
        oracle.__class__ = cls
        oracle.roots = nn.ModuleList([nn.ParameterDict() for _ in range(len(oracle.convs))])
        for k, v in root_tensors.items():
            _, l, t, _ = k.split('.')
            oracle.roots[int(l)][t] = nn.Parameter(v.detach().cpu().double().clone())
        return oracle

    def root_grads(self):
        return {f'roots.{l}.{t}.weight': p.grad for l, d in enumerate(self.roots) for t, p in d.items()}

    def without_roots(self):
        """The same oracle with the root term removed (its other parameters shared)."""
        import copy
        o = copy.copy(self)
        o._modules = dict(self._modules)
        o.roots = nn.ModuleList([nn.ParameterDict() for _ in range(len(self.convs))])
        return o

    def _conv(self, conv, x, ei, ea, **kw):
        return conv(x, ei, ea, **kw) if ea is not None else conv(x, ei, **kw)

    def _root(self, l, x, y):
        d = self.roots[l - 1]
        return {k: (v + x[k] @ d[k].t() if k in d else v) for k, v in y.items()}

    def _drop(self, l, x):
        if l < len(self.convs) and self.state_factor is not None:
            fac = self.state_factor.get(l, {})
            x = {k: (v * fac[k].to(v.dtype) if k in fac else v) for k, v in x.items()}
        return x

    def forward(self, x_dict, edge_index_dict, batch_size, return_h=False, edge_attr_dict=None):
        x = self._embed(x_dict)
        for l, conv in enumerate(self.convs, start=1):
            y = self._root(l, x, self._conv(conv, x, edge_index_dict, edge_attr_dict))
            x = self._drop(l, self._norm(l, y))
        if return_h:
            return F.relu(self.lin(x['SNP']))[:batch_size], x['SNP'][:batch_size]
        if self.no_relu:
            return self.lin(x['SNP'])[:batch_size]
        return F.relu(self.lin(x['SNP']))[:batch_size]

    def attention(self, x_dict, edge_index_dict, edge_attr_dict=None, raw=False):
        """Per layer {edge type: per-edge attention} with the root term in the state between the layers: ``raw`` is the export's
        procedure (kgwas/utils.py:446-461: raw weights returned and propagated, no ReLU between the layers), otherwise
        forward(return_attention_weights=True)'s (kgwas/model.py:65-72)."""
        x, atts = self._embed(x_dict), []
        for l, conv in enumerate(self.convs, start=1):
            y, att = self._conv(conv, x, edge_index_dict, edge_attr_dict, return_attention_weights=True, raw=raw)
            x = self._norm(l, self._root(l, x, y), relu=not raw)
            atts.append(att)
        return atts

    def attention_means(self, x_dict, edge_index_dict, edge_attr_dict=None):
        return [torch.mean(torch.vstack([a for a in att.values()])) for att in self.attention(x_dict, edge_index_dict, edge_attr_dict)]

    def export_attention(self, x_dict, edge_index_dict, edge_attr_dict=None):
        return self.attention(x_dict, edge_index_dict, edge_attr_dict, raw=True)


class _WithoutExtras:
    """The product model as the oracle builders of tests/helpers.py see it: everything but the ``roots.*`` / ``norms.*`` entries
    of its state_dict (their strict load knows the reference's keys only)."""

    def __init__(self, model):
        self._model = model

    def __getattr__(self, name):
        return getattr(self._model, name)

    def state_dict(self):
        sd = self._model.state_dict()
        return type(sd)((k, v) for k, v in sd.items() if not k.startswith(('roots.', 'norms.')))


def rooted_oracle(model, build, state_factor=None):
    """``build`` (tests.helpers.oracle_from_product, tests.multihead_ref.oracle_with_heads, tests.sigmoid_gate_ref.gated_oracle,
    tests.edge_attr_ref.oracle_from_product) on the model without its roots and norms, then both adopted from its state_dict."""
    oracle = build(_WithoutExtras(model))
    sd = model.state_dict()
    return RootedOracle.adopt(oracle, {k: v for k, v in sd.items() if k.startswith('roots.')},
                              {k: v for k, v in sd.items() if k.startswith('norms.')}, state_factor)
