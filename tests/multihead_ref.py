"""Float64 restatements of attention with H heads (gat_num_head = H, KgwLayerArgs.n_heads), in torch on the CPU.

The model: per relation exactly PyG's GATConv((-1,-1), c', heads=H, concat=True, add_self_loops=False) with c' = cl / H --
oracle/gat_oracle.py:GATConvOracle(in_src, in_dst, out_channels=c', heads=H) as it stands.  Column c < cl of the cl-wide state
belongs to head c // c'.

What the kernels compute is that model re-associated (the aggregate gathers the layer INPUT and W_src is applied after the sum),
per head h, relation r, destination i:
    u_r^h[k] = sum_{c in head h} W_src^T[k, c] att_src[c]           (v_r^h likewise; W_src for same-type relations)
    e^h_ij   = leaky_relu(<x_j, u_r^h> + <x_i, v_r^h>, 0.2)
    alpha^h  = softmax_j(e^h_ij / T)                                 (max-subtracted, denominator + 1e-16, per head)
    z^h_i    = sum_j alpha^h_ij x_j                                  (full width, per head)
    out_i[c] = sum_k z^{head(c)}_i[k] W_src^T[k, c] + bias[c]

``head_vectors`` + ``reassociated_conv`` restate that on a plain edge list (tests/test_multihead_host.py holds it against
GATConvOracle); ``planes_layer`` / ``planes_grads`` restate the PLANES contract of the C ABI on a sampled batch -- plane h of every
head-carrying array is what a single-head call with (U[h], V[h]) produces, dH sums over the heads -- on top of the single-head
float64 oracle of tests/test_gpu_aggregate_parity.py; ``oracle_with_heads`` builds the whole-model oracle."""
from collections import OrderedDict

import torch

from oracle.gat_oracle import GATConvOracle, HeteroGNNOracle, edge_key
from oracle.pyg_semantics import segment_softmax


def head_of_column(cl: int, H: int) -> torch.Tensor:
    return torch.arange(cl) // (cl // H)


def head_vectors(w_src, w_dst, att_src, att_dst, H: int):
    """(u [H, in], v [H, in]) of one relation from the reference-shaped parameters: lin_src.weight [cl, in], lin_dst.weight
    [cl, in] (None: a same-type relation, whose destination side goes through lin_src), att_* [1, H, c']."""
    cl = w_src.shape[0]
    hc = head_of_column(cl, H)
    wd = w_src if w_dst is None else w_dst
    a_s, a_d = att_src.reshape(-1), att_dst.reshape(-1)
    u = torch.stack([(w_src * (a_s * (hc == h)).unsqueeze(1)).sum(0) for h in range(H)])
    v = torch.stack([(wd * (a_d * (hc == h)).unsqueeze(1)).sum(0) for h in range(H)])
    return u, v


def reassociated_conv(x_src, x_dst, edge_index, w_src, w_dst, att_src, att_dst, bias, H: int, slope=0.2, temp=1.0):
    """One relation in the re-associated form (the docstring above), ending in the block transform
    out[:, head h] = z^h @ W_src^T[:, head h] + bias.  x_dst None: a same-type relation (x_dst = x_src)."""
    cl = w_src.shape[0]
    xd = x_src if x_dst is None else x_dst
    u, v = head_vectors(w_src, w_dst, att_src, att_dst, H)
    src, dst = edge_index[0], edge_index[1]
    hc = head_of_column(cl, H)
    out = torch.zeros(xd.shape[0], cl, dtype=x_src.dtype)
    for h in range(H):
        e = torch.nn.functional.leaky_relu((x_src @ u[h])[src] + (xd @ v[h])[dst], slope)
        alpha = segment_softmax(e / temp, dst, xd.shape[0])
        z = torch.zeros(xd.shape[0], x_src.shape[1], dtype=x_src.dtype).index_add(0, dst, alpha.unsqueeze(1) * x_src[src])
        cols = hc == h
        out[:, cols] = z @ w_src.t()[:, cols]
    return out + bias


# ------------------------------------------------------------------------------------------------------------------------------
# the planes contract on a sampled batch
# ------------------------------------------------------------------------------------------------------------------------------
def planes_layer(batch, layer, H, U, V, slope=0.2, temp=1.0, edges=None):
    """U, V [NH, n_rels, 128] -> (Z [NH, z rows, 128], stat [NH, z rows, 2], e_edge [NH, n_edges], alpha [NH, n_edges]); plane h
    = the single-head oracle with (U[h], V[h]).  Differentiable in H, U, V (their dtype)."""
    from tests.test_gpu_aggregate_parity import oracle_layer
    outs = [oracle_layer(batch, layer, H, U[h], V[h], slope, temp, edges=edges) for h in range(U.shape[0])]
    return tuple(torch.stack([o[k] for o in outs]) for k in range(4))


def planes_grads(batch, layer, H, U, V, G, dtype, slope=0.2, temp=1.0, relu_input=False, edges=None):
    """Forward and backward of sum(Z * G), G [NH, z rows, 128]: dict(Z, stat, e, alpha, dH, dU, dV) in ``dtype``."""
    Ho, Uo, Vo = (t.to(dtype).requires_grad_(True) for t in (H, U, V))
    Z, stat, e, alpha = planes_layer(batch, layer, Ho, Uo, Vo, slope, temp, edges)
    (Z * G.to(dtype)).sum().backward()
    dH = Ho.grad * (H > 0) if relu_input else Ho.grad
    return dict(Z=Z.detach(), stat=stat, e=e, alpha=alpha, dH=dH, dU=Uo.grad, dV=Vo.grad)


# ------------------------------------------------------------------------------------------------------------------------------
# the whole model
# ------------------------------------------------------------------------------------------------------------------------------
def oracle_with_heads(model, dtype=torch.float64):
    """HeteroGNNOracle of the product ``model`` (gat_num_head = H): built with one head, its convs replaced by
    GATConvOracle(cl, cl or None, cl // H, heads=H), loaded from the product's state_dict."""
    from tests.helpers import product_dims
    H = model.heads
    cl = model.hidden_logical
    snp, gene, go = product_dims(model)
    o = HeteroGNNOracle(model.edge_types, cl, model.lin.out_features, model.num_layers, 'GAT', model.aggr, snp, gene, go, 1,
                        no_relu=model.no_relu, dtype=dtype)
    for hc in o.convs:
        for et in hc.edge_types:
            s, _, d = et
            hc.convs[edge_key(et)] = GATConvOracle(cl, None if s == d else cl, cl // H, heads=H, dtype=dtype)
    sd = OrderedDict()
    for k, v in model.state_dict().items():
        if isinstance(v, torch.nn.parameter.UninitializedParameter):
            continue
        sd[k] = v.detach().cpu().to(dtype)
    o.load_state_dict(sd, strict=True)
    return o
