"""float64 statement of the layer-normalisation rule of kgw_layer_norm_relu_fwd / kgw_layer_norm_bwd (HeteroGNN(gnn_norm='layer')),
restated from include/kgwas_hip.h:

    mean = (1 / Cl) sum_{c < Cl} y_c      var = (1 / Cl) sum_{c < Cl} (y_c - mean)^2      rstd = 1 / sqrt(var + eps)
    xh_c = (y_c - mean) rstd              out_c = max(0, xh_c w_c + b_c) for c < Cl,      out_c = 0 for Cl <= c < 128
    gh_c = g_c w_c      dy_c = rstd (gh_c - mean_c(gh) - xh_c mean_c(gh xh))      dw_c = sum_rows g xh      db_c = sum_rows g
    (g: the upstream gradient masked by out > 0; dy_c = dw_c = db_c = 0 for c >= Cl)

and the float64 oracle of a normed model.  Nothing here calls the package."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.gat_oracle import GO_TYPES, HeteroGNNOracle

C = 128
EPS = 1e-5


def forward(y, w, b, cl, eps=EPS):
    """(out, mean, rstd, xh) of rows ``y`` [rows, 128] in y's dtype (float64 for the rule, float32 for the CPU yardstick); w, b [128]."""
    yl = y[:, :cl]
    mean = yl.mean(1, keepdim=True)
    var = ((yl - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = torch.zeros_like(y)
    xh[:, :cl] = (yl - mean) * rstd
    out = torch.zeros_like(y)
    out[:, :cl] = torch.relu(xh[:, :cl] * w[:cl] + b[:cl])
    return out, mean.reshape(-1), rstd.reshape(-1), xh


def backward(g, y, w, b, cl, eps=EPS, masked=False):
    """The closed form: (dy, dw, db) for the upstream gradient ``g`` of out; ``masked``: g already carries (out > 0)."""
    out, _, rstd, xh = forward(y, w, b, cl, eps)
    g = g.clone()
    g[:, cl:] = 0
    if not masked:
        g = g * (out > 0).to(g.dtype)
    gh = g[:, :cl] * w[:cl]
    x = xh[:, :cl]
    dy = torch.zeros_like(y)
    dy[:, :cl] = rstd.unsqueeze(1) * (gh - gh.mean(1, keepdim=True) - x * (gh * x).mean(1, keepdim=True))
    dw, db = torch.zeros_like(w), torch.zeros_like(w)
    dw[:cl] = (g[:, :cl] * x).sum(0)
    db[:cl] = g[:, :cl].sum(0)
    return dy, dw, db


def torch_reference(y, w, b, g, cl, eps=EPS, dtype=torch.float64, masked=False):
    """relu(F.layer_norm) on the logical columns and its autograd in ``dtype`` on the CPU: (out, dy, dw, db), each padded to 128
    columns with zeros.  float64: the reference of the kernel tests; float32: the yardstick of the ill-conditioned cases.
    ``masked``: g already carries (out > 0) -- it is sent back through the norm alone, so that both precisions use ONE mask."""
    yl = y[:, :cl].to(dtype).clone().requires_grad_(True)
    wl = w[:cl].to(dtype).clone().requires_grad_(True)
    bl = b[:cl].to(dtype).clone().requires_grad_(True)
    pre = F.layer_norm(yl, (cl,), wl, bl, eps)
    o = torch.relu(pre)
    (pre if masked else o).backward(g[:, :cl].to(dtype))

    def pad(t):
        return F.pad(t.detach(), (0, C - cl))
    return pad(o), pad(yl.grad), pad(wl.grad), pad(bl.grad)


class NormedStateOracle(HeteroGNNOracle):
    """HeteroGNNOracle with relu(F.layer_norm(y, (Cl,), w, b, 1e-5)) in place of the ReLU of every layer but the last:
    ``norms[l - 1][node type]`` = (weight, bias) float64 parameters for l = 1 .. L - 1 (a type without an entry keeps the plain
    ReLU).  ``state_factor`` (tests/hidden_dropout_ref.py's) multiplies the state after the ReLU: norm -> ReLU -> dropout."""

    state_factor = None

    @classmethod
    def adopt(cls, oracle: HeteroGNNOracle, norm_tensors, state_factor=None):
        """``norm_tensors``: {'norms.<l>.<type>.weight' | '.bias': tensor} (the product's state_dict entries)."""
        oracle.__class__ = cls
        L = len(oracle.convs)
        oracle.norms = nn.ModuleList([nn.ParameterDict() for _ in range(L - 1)])
        for k, v in norm_tensors.items():
            _, l, t, f = k.split('.')
            oracle.norms[int(l)][f'{t}__{f}'] = nn.Parameter(v.detach().cpu().double().clone())
        oracle.state_factor = state_factor
        return oracle

    def norm_grads(self):
        return {f'norms.{l}.{k.replace("__", ".")}': p.grad for l, d in enumerate(self.norms) for k, p in d.items()}

    def _norm(self, l, x_dict, relu=True):
        d = self.norms[l - 1] if l < len(self.convs) else {}
        out = {}
        for k, v in x_dict.items():
            if f'{k}__weight' in d:
                v = F.layer_norm(v, (v.shape[1],), d[f'{k}__weight'], d[f'{k}__bias'], EPS)
            out[k] = v.relu() if relu else v
        return out

    def forward(self, x_dict, edge_index_dict, batch_size, return_h=False):
        x_dict = self._embed(x_dict)
        L = len(self.convs)
        for l, conv in enumerate(self.convs, start=1):
            x_dict = self._norm(l, conv(x_dict, edge_index_dict))
            if l < L and self.state_factor is not None:
                fac = self.state_factor.get(l, {})
                x_dict = {k: (v * fac[k].to(v.dtype) if k in fac else v) for k, v in x_dict.items()}
        if return_h:
            return F.relu(self.lin(x_dict['SNP']))[:batch_size], x_dict['SNP'][:batch_size]
        if self.no_relu:
            return self.lin(x_dict['SNP'])[:batch_size]
        return F.relu(self.lin(x_dict['SNP']))[:batch_size]

    def _embed(self, x_dict):
        x = dict(x_dict)
        x['SNP'] = self.snp_feat_mlp(x['SNP'])
        x['Gene'] = self.gene_feat_mlp(x['Gene'])
        for t in GO_TYPES:
            if t in x:
                x[t] = self.go_feat_mlp(x[t])
        return x

    def attention_means(self, x_dict, edge_index_dict):
        """forward(return_attention_weights=True)'s second result (kgwas/model.py:65-72): per layer the mean softmax attention over
        all relations, the state between the layers normalised."""
        x, means = self._embed(x_dict), []
        for l, conv in enumerate(self.convs, start=1):
            x, att = conv(x, edge_index_dict, return_attention_weights=True)
            means.append(torch.mean(torch.vstack([a for a in att.values()])))
            x = self._norm(l, x)
        return means

    def export_attention(self, x_dict, edge_index_dict):
        """The export's procedure (kgwas/utils.py:446-461) on a normed model: per layer the raw attention of every relation, the
        state between the layers normalised but -- like the reference's -- not passed through a ReLU."""
        x, atts = self._embed(x_dict), []
        for l, conv in enumerate(self.convs, start=1):
            x, att = conv(x, edge_index_dict, return_attention_weights=True, raw=True)
            x = self._norm(l, x, relu=False)
            atts.append(att)
        return atts


class _WithoutNorms:
    """The product model as the oracle builders of tests/helpers.py see it: everything but the ``norms.*`` entries of its
    state_dict (their strict load knows the reference's keys only)."""

    def __init__(self, model):
        self._model = model

    def __getattr__(self, name):
        return getattr(self._model, name)

    def state_dict(self):
        return type(self._model.state_dict())((k, v) for k, v in self._model.state_dict().items() if not k.startswith('norms.'))


def normed_oracle(model, build, state_factor=None):
    """``build`` (tests.helpers.oracle_from_product, tests.multihead_ref.oracle_with_heads, ...) on the model without its norms,
    then the norms adopted from the model's state_dict."""
    oracle = build(_WithoutNorms(model))
    norms = {k: v for k, v in model.state_dict().items() if k.startswith('norms.')}
    return NormedStateOracle.adopt(oracle, norms, state_factor)
