"""Float64 restatements of sigmoid-gated attention (gat_sigmoid, KGW_F_SIGMOID_GATE), in torch on the CPU.

The model: per relation the reference's GATConv with ``sigmoid_gat=True`` and ``temperature=T`` (kgwas/conv.py:49-50,217-224) --
oracle/gat_oracle.py:GATConvOracle(sigmoid_gat=True, temperature=T) as it stands: every edge's message is weighted by
sigmoid(leaky_relu(a_j + a_i) / T), independently of the other edges of its row.

What the kernels compute is that model re-associated (the aggregate gathers the layer INPUT and W_src is applied after the sum),
per relation r and destination i:
    u_r     = W_src^T att_src,  v_r = W_dst^T att_dst            (W_src for same-type relations)
    e_ij    = leaky_relu(<x_j, u_r> + <x_i, v_r> (+ kappa_r), slope)
    g_ij    = 1 / (1 + exp(-e_ij / T))
    z_i     = sum_j g_ij x_j                                       (no max, no denominator; a row without in-edges stays 0)
    out_i   = z_i W_src^T + bias

``reassociated_gated_conv`` restates that on a plain edge list (tests/test_sigmoid_gate_host.py holds it against GATConvOracle);
``gated_layer`` / ``gated_grads`` restate one layer of a sampled batch in the kernels' layout (Z rows by (row, relation slot), stat
(0, 1) on visited rows, e_edge and the gate per local edge), with the gradients by autograd."""
import torch

C = 128


def reassociated_gated_conv(x_src, x_dst, edge_index, w_src, w_dst, att_src, att_dst, bias, slope=0.2, temp=1.0):
    """One relation in the re-associated form.  x_dst None: a same-type relation (x_dst = x_src, W_dst = W_src).  w_* are the
    reference-shaped lin_*.weight [out, in], att_* [1, 1, out]."""
    xd = x_src if x_dst is None else x_dst
    wd = w_src if w_dst is None else w_dst
    u = w_src.t() @ att_src.reshape(-1)
    v = wd.t() @ att_dst.reshape(-1)
    src, dst = edge_index[0], edge_index[1]
    e = torch.nn.functional.leaky_relu((x_src @ u)[src] + (xd @ v)[dst], slope)
    g = 1.0 / (1.0 + torch.exp(-e / temp))
    z = torch.zeros(xd.shape[0], x_src.shape[1], dtype=x_src.dtype).index_add(0, dst, g.unsqueeze(1) * x_src[src])
    return z @ w_src.t() + bias


def gated_layer(batch, layer, H, U, V, slope=0.2, temp=1.0, lbias=None, edges=None):
    """(Z [z rows, 128], stat [z rows, 2], e [n_edges], g [n_edges]) of one layer of ``batch`` over its live relations, in the
    kernels' layout (see tests/test_gpu_aggregate_parity.py:oracle_layer, whose edge lists this takes).  Differentiable in H, U, V,
    lbias (their dtype)."""
    from tests.test_gpu_aggregate_parity import layer_edges
    dg, m = batch.dg, batch.meta
    sc = dg.schema
    edges = layer_edges(batch, layer) if edges is None else edges
    dt = H.dtype
    z_rows = int(m.z_base[layer - 1][sc.NT])
    n_edges = int(m.n_edges[layer - 1])
    Z = torch.zeros(z_rows, C, dtype=dt)
    stat = torch.zeros(z_rows, 2, dtype=dt)
    e_all = torch.zeros(n_edges, dtype=dt)
    g_all = torch.zeros(n_edges, dtype=dt)
    for r, (eid, src, dst) in edges.items():
        s, d = int(sc.src_type[r]), int(sc.dst_type[r])
        nr = int(m.n_rows[layer - 1][d])
        Hs = H[int(m.src_base[layer - 1][s]):int(m.src_base[layer - 1][s]) + int(m.n_src[layer - 1][s])]
        Hd = H[int(m.src_base[layer - 1][d]):int(m.src_base[layer - 1][d]) + nr]
        pre = (Hs @ U[r])[src] + (Hd @ V[r])[dst]
        if lbias is not None:
            pre = pre + lbias[r]
        e = torch.nn.functional.leaky_relu(pre, slope)
        g = 1.0 / (1.0 + torch.exp(-e / temp))
        zrow = int(m.z_base[layer - 1][d]) + dst * int(sc.R_dst[d]) + int(sc.slot_dst[r])
        with torch.no_grad():
            e_all[eid] = e.detach()
            g_all[eid] = g.detach()
            stat[zrow] = torch.tensor([0.0, 1.0], dtype=dt)
        Z = Z.index_add(0, zrow, g.unsqueeze(-1) * Hs[src])
    return Z, stat, e_all, g_all


def gated_grads(batch, layer, H, U, V, kap, G, dtype, slope=0.2, temp=1.0, relu_input=False, edges=None):
    """Forward and backward of sum(Z * G): dict(Z, stat, e, g, dH, dU, dV, dlb) in ``dtype``; ``relu_input``: dH is masked by
    (H > 0), as the source-side kernel does for a layer input that is a ReLU output."""
    Ho, Uo, Vo = (t.to(dtype).requires_grad_(True) for t in (H, U, V))
    ko = kap.to(dtype).requires_grad_(True) if kap is not None else None
    Z, stat, e, g = gated_layer(batch, layer, Ho, Uo, Vo, slope, temp, ko, edges)
    (Z * G.to(dtype)).sum().backward()
    dH = Ho.grad * (H > 0) if relu_input else Ho.grad
    return dict(Z=Z.detach(), stat=stat, e=e, g=g, dH=dH, dU=Uo.grad, dV=Vo.grad, dlb=ko.grad if ko is not None else None)


def gated_oracle(model, dtype=torch.float64):
    """tests.helpers.oracle_from_product(model) with the product's two switches set on every GATConvOracle."""
    from tests.helpers import oracle_from_product
    o = oracle_from_product(model, dtype)
    for hc in o.convs:
        for conv in hc.convs.values():
            conv.sigmoid_gat = bool(getattr(model, 'gat_sigmoid', False))
            conv.temperature = float(model.temperature)
    return o
