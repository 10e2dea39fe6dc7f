"""numpy / float64 twin of the attention-dropout rule of kgw_gat_aggregate_fwd / _bwd_dst, restated from include/kgwas_hip.h:

    base(word, l) = step(step(step(0, lo32(word)), hi32(word)), l)         step(h, x) = mix32((h ^ x) + 0x9e3779b9)
    keep(e)       = mix32(base ^ e) >= floor(p * 2^32)                      e = LOCAL edge index of the batch
    m'(e)         = keep(e) ? float32(1 / (1 - p)) : 0
    Z[i, r]       = sum_j m'(e_ij) alpha_ij H_src[j]                        alpha = the undropped softmax

and of the host's word, dropout_word(seed, epoch, batch).  Nothing here calls the package's rule: the tests hand it the
batch's edge lists (tests/test_gpu_aggregate_parity.py::layer_edges)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.gat_oracle import GATConvOracle
from oracle.pyg_semantics import segment_softmax
from tests.fanout_ref import M32, M64, _splitmix64, _step, mix32

DROPOUT_TAG = int.from_bytes(b'dropout!', 'big')


def dropout_word(seed, epoch, batch):
    """The trainer's 64-bit word of (seed, epoch, batch index): the sampler's splitmix64 rounds behind one constant tag."""
    z = _splitmix64(DROPOUT_TAG)
    z = _splitmix64(z ^ (int(seed) & M64))
    z = _splitmix64(z ^ (int(epoch) & M64))
    return _splitmix64(z ^ (int(batch) & M64))


def base(word, layer):
    word = int(word) & M64
    h = _step(0, word & M32)
    h = _step(h, word >> 32)
    return _step(h, int(layer))


def thresh(p):
    return int(float(p) * 4294967296.0)


def keep(word, layer, e, p):
    """bool array: local edges ``e`` (array of indices) kept in layer ``layer`` under ``word`` at drop probability ``p``."""
    e = np.asarray(e, dtype=np.uint64)
    return mix32(np.uint64(base(word, layer)) ^ e) >= np.uint64(thresh(p))


def factor(word, layer, n_edges, p):
    """float64 tensor [n_edges]: m'(e) of every local edge -- float32(1 / (1 - p)) where kept, 0 where dropped."""
    k = keep(word, layer, np.arange(n_edges), p)
    return torch.from_numpy(np.where(k, float(np.float32(1.0 / (1.0 - p))), 0.0))


def masked_layer(batch, layer, H, U, V, edges, mfac, slope=0.2, temp=1.0, lbias=None):
    """Z[zrow(i, r)] = sum_j m'(e_ij) alpha_ij H_src[j] (alpha: PyG's softmax of leaky_relu(<H_src[j], u_r> + <H_dst[i], v_r> +
    kappa_r) / T), in the dtype of H; differentiable in H, U, V, lbias.  ``edges``: layer_edges(batch, layer); ``mfac`` [n_edges]
    by local edge id.  Also returns the set of Z rows that have an edge and the set whose edges are all dropped."""
    m, sc = batch.meta, batch.dg.schema
    dt = H.dtype
    z_rows = int(m.z_base[layer - 1][sc.NT])
    Z = torch.zeros(z_rows, H.shape[1], dtype=dt)
    has = torch.zeros(z_rows, dtype=torch.bool)
    kept = torch.zeros(z_rows, dtype=torch.bool)
    mf = mfac.to(dt)
    for r, (eid, src, dst) in edges.items():
        s, d = int(sc.src_type[r]), int(sc.dst_type[r])
        nr = int(m.n_rows[layer - 1][d])
        Hs = H[int(m.src_base[layer - 1][s]):int(m.src_base[layer - 1][s]) + int(m.n_src[layer - 1][s])]
        Hd = H[int(m.src_base[layer - 1][d]):int(m.src_base[layer - 1][d]) + nr]
        pre = (Hs @ U[r])[src] + (Hd @ V[r])[dst]
        if lbias is not None:
            pre = pre + lbias[r]
        alpha = segment_softmax(F.leaky_relu(pre, slope) / temp, dst, nr)
        zrow = int(m.z_base[layer - 1][d]) + dst * int(sc.R_dst[d]) + int(sc.slot_dst[r])
        has[zrow] = True
        kept[zrow[mf[eid] > 0]] = True
        Z = Z.index_add(0, zrow, (alpha * mf[eid]).unsqueeze(-1) * Hs[src])
    return Z, has, has & ~kept


def masked_grads(batch, layer, H, U, V, kap, G, edges, mfac, dtype, slope=0.2, temp=1.0, relu_input=False):
    """{Z, dH, dU, dV, dlb, has, all_dropped} of sum(Z * G) through ``masked_layer`` in ``dtype`` (torch autograd)."""
    Ho, Uo, Vo = (t.to(dtype).requires_grad_(True) for t in (H, U, V))
    ko = kap.to(dtype).requires_grad_(True) if kap is not None else None
    Z, has, gone = masked_layer(batch, layer, Ho, Uo, Vo, edges, mfac, slope, temp, ko)
    (Z * G.to(dtype)).sum().backward()
    dH = Ho.grad * (H > 0) if relu_input else Ho.grad
    return dict(Z=Z.detach(), dH=dH, dU=Uo.grad, dV=Vo.grad, dlb=ko.grad if ko is not None else None, has=has, all_dropped=gone)


class MaskedGATConvOracle(GATConvOracle):
    """GATConvOracle whose softmax weights are multiplied by a supplied per-edge m' (``edge_factor``, in the order of the
    ``edge_index`` it is called with; None = no dropout) -- alpha = F.dropout(alpha, p, training) of kgwas/conv.py:224 with the
    mask given instead of drawn."""

    edge_factor = None

    @classmethod
    def adopt(cls, conv: GATConvOracle):
        conv.__class__ = cls
        return conv

    def forward(self, x, edge_index, return_attention_weights=None, return_raw_attention_weights=None):
        assert return_attention_weights is None and return_raw_attention_weights is None and not self.sigmoid_gat
        H, C = self.heads, self.out_channels
        if isinstance(x, torch.Tensor):
            x_src = x_dst = self.lin_src(x).view(-1, H, C)
        else:
            xs, xd = x
            x_src = self.lin_src(xs).view(-1, H, C)
            x_dst = self.lin_dst(xd).view(-1, H, C) if xd is not None else None
        alpha_src = (x_src * self.att_src).sum(dim=-1)
        alpha_dst = None if x_dst is None else (x_dst * self.att_dst).sum(-1)
        n_dst = x_dst.size(0) if x_dst is not None else x_src.size(0)
        src, dst = edge_index[0], edge_index[1]
        alpha = alpha_src.index_select(0, src)
        if alpha_dst is not None:
            alpha = alpha + alpha_dst.index_select(0, dst)
        alpha = segment_softmax(F.leaky_relu(alpha, self.negative_slope) / self.temperature, dst, n_dst)
        if self.edge_factor is not None:
            assert self.edge_factor.shape[0] == alpha.shape[0]
            alpha = alpha * self.edge_factor.to(alpha.dtype).view(-1, 1)
        msg = alpha.unsqueeze(-1) * x_src.index_select(0, src)
        out = torch.zeros(n_dst, H, C, dtype=msg.dtype).index_add(0, dst, msg)
        return out.view(-1, H * C) + self.bias
