"""Float64 restatements of edge attributes (GATConv's ``edge_dim``; KgwEdgeAttr in include/kgwas_hip.h), in torch on the CPU.

The model: per attributed relation the reference's GATConv with ``edge_dim=D`` (kgwas/conv.py:46,95-101,207-215): a bias-free
``lin_edge`` [C, D] maps the edge's attribute row to the hidden width and <lin_edge(attr_e), att_edge> is added to a_j + a_i before
the LeakyReLU; the messages do not change.  ``literal_pre_logit`` is that text, op for op.

What the kernels compute is the same thing re-associated, the way u_r and v_r are:
    w_r   = lin_edge.weight^T att_edge                         in R^D
    t_e   = sum_d A_r[p(e)][d] w_r[d]
    pre_e = <x_j, u_r> + <x_i, v_r> (+ kappa_r) + t_e
with A_r's rows in the order of the relation's dst-major CSR (``reassociated_pre_logit``; tests/test_edge_attr_host.py holds the two
against each other).  ``layer_positions`` finds the CSR position of every local edge of a sampled batch from seg_ptr, n_id and the
resident row pointers -- not from the chunks' gpos, which is what the kernels read --, ``eattr_layer`` / ``eattr_grads`` restate one
layer in the kernels' layout, and ``EdgeAttrGNNOracle`` is oracle/gat_oracle.py's model with the edge term on its attributed
relations, under the reference's parameter names."""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.gat_oracle import GATConvOracle, HeteroConvOracle, HeteroGNNOracle, _group, edge_key, glorot_
from oracle.pyg_semantics import segment_softmax

C = 128


# ------------------------------------------------------------------------------------------------------------------------------
# one relation on a plain edge list
# ------------------------------------------------------------------------------------------------------------------------------
def literal_pre_logit(x_src, x_dst, edge_index, edge_attr, w_src, w_dst, att_src, att_dst, w_edge, att_edge):
    """conv.py:142-151,205-215 with heads = 1: the logit before the LeakyReLU.  w_* are reference-shaped (lin_*.weight [C, in],
    lin_edge.weight [C, D], att_* [1, 1, C]); ``edge_attr`` [E] or [E, D]."""
    Cc = w_src.shape[0]
    xs = (x_src @ w_src.t()).view(-1, 1, Cc)
    xd = (x_dst @ w_dst.t()).view(-1, 1, Cc)
    alpha_src = (xs * att_src).sum(dim=-1)
    alpha_dst = (xd * att_dst).sum(dim=-1)
    alpha = alpha_src[edge_index[0]] + alpha_dst[edge_index[1]]
    if edge_attr.dim() == 1:
        edge_attr = edge_attr.view(-1, 1)
    ea = (edge_attr @ w_edge.t()).view(-1, 1, Cc)
    return (alpha + (ea * att_edge).sum(dim=-1)).reshape(-1)


def reassociated_pre_logit(x_src, x_dst, edge_index, edge_attr, w_src, w_dst, att_src, att_dst, w_edge, att_edge):
    """The rule of include/kgwas_hip.h: u_r, v_r, w_r formed from the parameters, one dot product per node and per edge."""
    u = w_src.t() @ att_src.reshape(-1)
    v = w_dst.t() @ att_dst.reshape(-1)
    w = w_edge.t() @ att_edge.reshape(-1)
    A = edge_attr.view(-1, 1) if edge_attr.dim() == 1 else edge_attr
    return (x_src @ u)[edge_index[0]] + (x_dst @ v)[edge_index[1]] + A @ w


# ------------------------------------------------------------------------------------------------------------------------------
# one layer of a sampled batch, in the kernels' layout
# ------------------------------------------------------------------------------------------------------------------------------
def layer_positions(batch, layer, edges):
    """{relation id: CSR position (relative to the relation's first entry) of every local edge in ``edges[r][0]``'s order}:
    the segments of a batch hold whole rows in CSR order, so edge k of the segment of local row i sits at rowptr[n_id[i]] + k."""
    dg, m = batch.dg, batch.meta
    sc = dg.schema
    n_hops = min(dg.num_layers - layer, dg.n_hops - 1) + 1
    seg_ptr = batch.buf.seg_ptr[:int(m.seg_end[dg.n_hops - 1]) + 1].cpu().long()
    rowptr = dg.g_rowptr.cpu().long()
    out = {}
    for r in edges:
        d = int(sc.dst_type[r])
        rp = rowptr[int(dg.kg.rowptr_off[r]):int(dg.kg.rowptr_off[r]) + dg.n_nodes[d] + 1]
        gid = batch.n_id(sc.node_types[d]).cpu().long()
        pos = []
        for h in range(n_hops):
            a, b = int(m.seg_off[h][r]), int(m.seg_off[h][r + 1])
            if b <= a:
                continue
            deg = seg_ptr[a + 1:b + 1] - seg_ptr[a:b]
            g = gid[int(m.node_off[d][h]):int(m.node_off[d][h]) + (b - a)]
            assert torch.equal(deg, rp[g + 1] - rp[g]), 'a segment that does not hold its whole row'
            within = torch.arange(int(deg.sum())) - torch.repeat_interleave(torch.cumsum(deg, 0) - deg, deg)
            pos.append(torch.repeat_interleave(rp[g], deg) + within)
        out[r] = torch.cat(pos)
        assert out[r].numel() == edges[r][0].numel()
    return out


def eattr_layer(batch, layer, H, U, V, W, attrs, edges, pos, slope=0.2, temp=1.0, lbias=None, raw=False):
    """(Z, stat, e, alpha, term) of one layer over its live relations (tests/test_gpu_aggregate_parity.py:oracle_layer with
    pre_e += t_e).  ``attrs`` {relation id: [E_r, D] in CSR order} (a relation that is not in it has t_e = 0), ``W`` [n_rels, D].
    Differentiable in H, U, V, W, lbias (their dtype)."""
    dg, m = batch.dg, batch.meta
    sc = dg.schema
    dt = H.dtype
    z_rows = int(m.z_base[layer - 1][sc.NT])
    n_edges = int(m.n_edges[layer - 1])
    Z = torch.zeros(z_rows, C, dtype=dt)
    stat = torch.zeros(z_rows, 2, dtype=dt)
    e_all = torch.zeros(n_edges, dtype=dt)
    alpha_all = torch.zeros(n_edges, dtype=dt)
    term_all = torch.zeros(n_edges, dtype=dt)
    for r, (eid, src, dst) in edges.items():
        s, d = int(sc.src_type[r]), int(sc.dst_type[r])
        nr = int(m.n_rows[layer - 1][d])
        Hs = H[int(m.src_base[layer - 1][s]):int(m.src_base[layer - 1][s]) + int(m.n_src[layer - 1][s])]
        Hd = H[int(m.src_base[layer - 1][d]):int(m.src_base[layer - 1][d]) + nr]
        pre = (Hs @ U[r])[src] + (Hd @ V[r])[dst]
        if lbias is not None:
            pre = pre + lbias[r]
        if r in attrs:
            t = attrs[r].to(dt)[pos[r]] @ W[r]
            pre = pre + t
            with torch.no_grad():
                term_all[eid] = t.detach()
        e = F.leaky_relu(pre, slope)
        zrow = int(m.z_base[layer - 1][d]) + dst * int(sc.R_dst[d]) + int(sc.slot_dst[r])
        with torch.no_grad():
            e_all[eid] = e.detach()
            if raw:
                stat[zrow] = torch.tensor([0.0, 1.0], dtype=dt)
            else:
                tt = (e / temp).detach()
                mx = torch.full((nr,), float('-inf'), dtype=dt).scatter_reduce(0, dst, tt, reduce='amax')
                den = torch.zeros(nr, dtype=dt).index_add(0, dst, (tt - mx[dst]).exp()) + 1e-16
                rows = torch.unique(dst)
                stat[int(m.z_base[layer - 1][d]) + rows * int(sc.R_dst[d]) + int(sc.slot_dst[r])] = torch.stack([mx[rows], den[rows]], 1)
        w = e if raw else segment_softmax(e / temp, dst, nr)
        if not raw:
            alpha_all[eid] = w.detach()
        Z = Z.index_add(0, zrow, w.unsqueeze(-1) * Hs[src])
    return Z, stat, e_all, alpha_all, term_all


def eattr_grads(batch, layer, H, U, V, W, kap, G, attrs, edges, pos, dtype, slope=0.2, temp=1.0, relu_input=False):
    """Forward and backward of sum(Z * G): dict(Z, stat, e, alpha, term, dH, dU, dV, dW, dlb) in ``dtype``."""
    Ho, Uo, Vo, Wo = (t.to(dtype).requires_grad_(True) for t in (H, U, V, W))
    ko = kap.to(dtype).requires_grad_(True) if kap is not None else None
    Z, stat, e, alpha, term = eattr_layer(batch, layer, Ho, Uo, Vo, Wo, attrs, edges, pos, slope, temp, ko)
    (Z * G.to(dtype)).sum().backward()
    dH = Ho.grad * (H > 0) if relu_input else Ho.grad
    dW = Wo.grad if Wo.grad is not None else torch.zeros_like(Wo)
    return dict(Z=Z.detach(), stat=stat, e=e, alpha=alpha, term=term, dH=dH, dU=Uo.grad, dV=Vo.grad, dW=dW,
                dlb=ko.grad if ko is not None else None)


# ------------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------------
class EdgeGATConvOracle(GATConvOracle):
    """GATConvOracle with ``edge_dim`` (conv.py:95-101: lin_edge bias-free, glorot; att_edge [1, H, C], glorot)."""

    def __init__(self, in_src, in_dst, out_channels, edge_dim, dtype=torch.float32, gen=None):
        super().__init__(in_src, in_dst, out_channels, dtype=dtype, gen=gen)
        self.lin_edge = nn.Linear(edge_dim, out_channels, bias=False, dtype=dtype)
        glorot_(self.lin_edge.weight, gen)
        self.att_edge = nn.Parameter(glorot_(torch.empty(1, 1, out_channels, dtype=dtype), gen))

    def forward(self, x, edge_index, edge_attr, return_attention_weights=None, return_raw_attention_weights=None):
        Hh, Cc = self.heads, self.out_channels
        if isinstance(x, torch.Tensor):
            x_src = x_dst = self.lin_src(x).view(-1, Hh, Cc)
        else:
            x_src = self.lin_src(x[0]).view(-1, Hh, Cc)
            x_dst = self.lin_dst(x[1]).view(-1, Hh, Cc)
        alpha_src = (x_src * self.att_src).sum(dim=-1)
        alpha_dst = (x_dst * self.att_dst).sum(dim=-1)
        n_dst = x_dst.size(0)
        src, dst = edge_index[0], edge_index[1]
        alpha = alpha_src.index_select(0, src) + alpha_dst.index_select(0, dst)        # :205
        if edge_attr.dim() == 1:                                                        # :208-209
            edge_attr = edge_attr.view(-1, 1)
        ea = self.lin_edge(edge_attr).view(-1, Hh, Cc)                                  # :212-213
        alpha = alpha + (ea * self.att_edge).sum(dim=-1)                                # :214-215
        alpha = F.leaky_relu(alpha, self.negative_slope)                                # :217
        if not return_raw_attention_weights:
            alpha = segment_softmax(alpha / self.temperature, dst, n_dst)               # :223
        msg = alpha.unsqueeze(-1) * x_src.index_select(0, src)
        out = torch.zeros(n_dst, Hh, Cc, dtype=msg.dtype).index_add(0, dst, msg).view(-1, Hh * Cc) + self.bias
        if isinstance(return_attention_weights, bool):
            return out, (edge_index, alpha)
        return out


class EdgeHeteroConvOracle(HeteroConvOracle):
    """HeteroConvOracle that hands an attributed relation its ``edge_attr`` (PyG HeteroConv passes ``edge_attr_dict[et]``)."""

    def forward(self, x_dict, edge_index_dict, edge_attr_dict, return_attention_weights=False, raw=False):
        out_dict, att = {}, {}
        for et, edge_index in edge_index_dict.items():
            key = edge_key(et)
            if key not in self.convs:
                continue
            s, _, d = et
            x = x_dict[s] if s == d else (x_dict[s], x_dict[d])
            conv = self.convs[key]
            args = (x, edge_index, edge_attr_dict[et]) if isinstance(conv, EdgeGATConvOracle) else (x, edge_index)
            if return_attention_weights:
                out, (_, a) = conv(*args, return_attention_weights=True, return_raw_attention_weights=raw)
                att[et] = a
            else:
                out = conv(*args)
            out_dict.setdefault(d, []).append(out)
        res = {k: _group(v, self.aggr) for k, v in out_dict.items()}
        return (res, att) if return_attention_weights else res


class EdgeAttrGNNOracle(HeteroGNNOracle):
    """HeteroGNNOracle whose attributed relations (``attr_types``) are EdgeGATConvOracle in every layer."""

    def __init__(self, edge_types, hidden, out_channels, num_layers, aggr, snp, gene, go, edge_dim, attr_types, no_relu=False,
                 dtype=torch.float64):
        super().__init__(edge_types, hidden, out_channels, num_layers, 'GAT', aggr, snp, gene, go, 1, no_relu=no_relu, dtype=dtype)
        attr_types = {tuple(e) for e in attr_types}
        convs = nn.ModuleList()
        for _ in range(num_layers):
            layer = OrderedDict()
            for et in self.edge_types:
                s, _, d = et
                in_dst = None if s == d else hidden
                layer[et] = EdgeGATConvOracle(hidden, in_dst, hidden, edge_dim, dtype=dtype) if tuple(et) in attr_types else \
                    GATConvOracle(hidden, in_dst, hidden, dtype=dtype)
            convs.append(EdgeHeteroConvOracle(layer, aggr=aggr))
        self.convs = convs

    def embed(self, x_dict):
        from oracle.gat_oracle import GO_TYPES
        x_dict = dict(x_dict)
        x_dict['SNP'] = self.snp_feat_mlp(x_dict['SNP'])
        x_dict['Gene'] = self.gene_feat_mlp(x_dict['Gene'])
        for t in GO_TYPES:
            if t in x_dict:
                x_dict[t] = self.go_feat_mlp(x_dict[t])
        return x_dict

    def forward(self, x_dict, edge_index_dict, edge_attr_dict, batch_size, return_attention_weights=False):
        x_dict = self.embed(x_dict)
        att_all = []
        for conv in self.convs:
            if return_attention_weights:
                x_dict, att = conv(x_dict, edge_index_dict, edge_attr_dict, return_attention_weights=True)
                att_all.append(att)
            else:
                x_dict = conv(x_dict, edge_index_dict, edge_attr_dict)
            x_dict = {k: v.relu() for k, v in x_dict.items()}
        out = self.lin(x_dict['SNP'])[:batch_size]
        out = out if self.no_relu else F.relu(out)
        return (out, att_all) if return_attention_weights else out


def oracle_from_product(model, dtype=torch.float64):
    """The float64 oracle with the product's parameters, exchanged by the reference's names (lin_edge.weight / att_edge included)."""
    from tests.helpers import product_dims
    snp, gene, go = product_dims(model)
    o = EdgeAttrGNNOracle(model.edge_types, model.hidden_logical, model.lin.out_features, model.num_layers, model.aggr, snp, gene, go,
                          model.edge_dim, [model.edge_types[r] for r in model.attr_rels], no_relu=model.no_relu, dtype=dtype)
    sd = OrderedDict()
    for k, v in model.state_dict().items():
        if isinstance(v, torch.nn.parameter.UninitializedParameter):
            continue
        sd[k] = v.detach().cpu().to(dtype)
    o.load_state_dict(sd, strict=True)
    return o


def batch_cpu(batch, dtype=torch.float64):
    """(x_dict, edge_index_dict, edge_attr_dict) of a sampled batch on the CPU; the attributes found by CSR position from seg_ptr,
    n_id and the row pointers (``layer_positions``' rule over all hops), independently of the product's own lookup."""
    dg, m = batch.dg, batch.meta
    sc = dg.schema
    x = {t: v.detach().cpu().to(dtype) for t, v in batch.x_dict.items()}
    ei = OrderedDict((k, v.cpu()) for k, v in batch.edge_index_dict.items())
    seg_ptr = batch.buf.seg_ptr[:int(m.seg_end[dg.n_hops - 1]) + 1].cpu().long()
    rowptr = dg.g_rowptr.cpu().long()
    ea = OrderedDict()
    for r, et in enumerate(sc.edge_types):
        a = dg.data[et].get('edge_attr')
        if a is None:
            continue
        a = a.view(-1, 1) if a.dim() == 1 else a
        d = int(sc.dst_type[r])
        rp = rowptr[int(dg.kg.rowptr_off[r]):int(dg.kg.rowptr_off[r]) + dg.n_nodes[d] + 1]
        full = dg.data[et].edge_index.cpu().long()
        order = torch.argsort(full[1] * dg.n_nodes[int(sc.src_type[r])] + full[0], stable=True)      # CSR entry p = column order[p]
        gid = batch.n_id(sc.node_types[d]).cpu().long()
        pos = []
        for h in range(dg.n_hops):
            s0, s1 = int(m.seg_off[h][r]), int(m.seg_off[h][r + 1])
            if s1 <= s0:
                continue
            deg = seg_ptr[s0 + 1:s1 + 1] - seg_ptr[s0:s1]
            g = gid[int(m.node_off[d][h]):int(m.node_off[d][h]) + (s1 - s0)]
            within = torch.arange(int(deg.sum())) - torch.repeat_interleave(torch.cumsum(deg, 0) - deg, deg)
            pos.append(torch.repeat_interleave(rp[g], deg) + within)
        p = torch.cat(pos) if pos else torch.zeros(0, dtype=torch.long)
        ea[et] = a.cpu().to(dtype)[order[p]]
        assert ea[et].shape[0] == ei[et].shape[1]
    return x, ei, ea
