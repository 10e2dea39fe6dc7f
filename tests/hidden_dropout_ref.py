"""numpy / float64 twin of the hidden-state dropout rule of kgw_hidden_dropout (HeteroGNN(gnn_dropout=p)), restated from
include/kgwas_hip.h:

    base(word, l, t) = step(step(attn_base(word, l), TAG), t)          TAG = the bytes of 'hdrp', big-endian
    keep(row, c)     = mix32(base ^ (row * 128 + c)) >= floor(p * 2^32)  row = LOCAL index of the node within its type, c < 128
    y'(row, c)       = keep ? float32(y * float32(1 / (1 - p))) : 0.0

attn_base is the attention-dropout rule's base (tests/attn_dropout_ref.py), step / mix32 the fan-out rule's (tests/fanout_ref.py).
Nothing here calls the package."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.gat_oracle import GO_TYPES, HeteroGNNOracle
from tests import attn_dropout_ref as A
from tests.fanout_ref import M32, _step, mix32

HDROP_TAG = int.from_bytes(b'hdrp', 'big')
C = 128
dropout_word = A.dropout_word
thresh = A.thresh


def base(word, layer, t):
    return _step(_step(A.base(word, layer), HDROP_TAG), int(t) & M32)


def scale(p):
    return np.float32(1.0 / (1.0 - float(p)))


def keep(word, layer, t, rows, p, row0=0):
    """bool [rows, 128]: the kept elements of local rows row0 .. row0 + rows - 1 of node type ``t`` in layer ``layer``."""
    idx = (np.arange(row0, row0 + rows, dtype=np.uint64)[:, None] * np.uint64(C)) + np.arange(C, dtype=np.uint64)[None, :]
    return mix32(np.uint64(base(word, layer, t)) ^ idx) >= np.uint64(thresh(p))


def factor(word, layer, t, rows, p):
    """float32 [rows, 128]: m' -- float32(1 / (1 - p)) where kept, 0 where dropped."""
    return np.where(keep(word, layer, t, rows, p), scale(p), np.float32(0.0)).astype(np.float32)


def apply(y, word, layer, t, p):
    """The kernel's output for float32 ``y`` [rows, 128] (numpy): one float32 multiply where kept, exactly 0.0 elsewhere --
    whatever the dropped element held (NaN * 0 would be NaN: the rule selects)."""
    y = np.asarray(y, dtype=np.float32)
    k = keep(word, layer, t, y.shape[0], p)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.where(k, y * scale(p), np.float32(0.0)).astype(np.float32)


class DroppedStateOracle(HeteroGNNOracle):
    """HeteroGNNOracle whose hidden state is multiplied by a supplied factor after the ReLU of every layer but the last:
    ``state_factor[l][node type]`` = [rows of the type in the batch, C] for l = 1 .. L - 1 (a missing entry: no dropout) --
    x = F.dropout(x, p, training) between the layers with the mask given instead of drawn."""

    state_factor = None

    @classmethod
    def adopt(cls, oracle: HeteroGNNOracle, state_factor):
        oracle.__class__ = cls
        oracle.state_factor = state_factor
        return oracle

    def forward(self, x_dict, edge_index_dict, batch_size, return_h=False):
        x_dict = dict(x_dict)
        x_dict['SNP'] = self.snp_feat_mlp(x_dict['SNP'])
        x_dict['Gene'] = self.gene_feat_mlp(x_dict['Gene'])
        for t in GO_TYPES:
            if t in x_dict:
                x_dict[t] = self.go_feat_mlp(x_dict[t])
        L = len(self.convs)
        for l, conv in enumerate(self.convs, start=1):
            x_dict = conv(x_dict, edge_index_dict)
            x_dict = {k: v.relu() for k, v in x_dict.items()}
            if l < L and self.state_factor is not None:
                fac = self.state_factor.get(l, {})
                x_dict = {k: (v * fac[k].to(v.dtype) if k in fac else v) for k, v in x_dict.items()}
        if return_h:
            return F.relu(self.lin(x_dict['SNP']))[:batch_size], x_dict['SNP'][:batch_size]
        if self.no_relu:
            return self.lin(x_dict['SNP'])[:batch_size]
        return F.relu(self.lin(x_dict['SNP']))[:batch_size]


def state_factors(model, batch, word, p):
    """``state_factor`` of DroppedStateOracle for the product's ``batch``: the twin's m' on the rows layer l computes (the
    hop-pruned prefix ``meta.n_rows[l - 1][t]`` of the type's local nodes), 1 on the rows the product prunes by hop -- they reach no
    seed.  Also returns the number of dropped elements among the model's own columns."""
    m, sc = batch.meta, model.schema
    cl = model.hidden_logical
    out, n_dropped = {}, 0
    for l in range(1, model.num_layers):
        out[l] = {}
        for t, name in enumerate(sc.node_types):
            rows = int(m.n_rows[l - 1][t])
            if not rows:
                continue
            n_all = int(batch.n_nodes[name])
            f = torch.ones(n_all, cl, dtype=torch.float64)
            f[:rows] = torch.from_numpy(factor(word, l, t, rows, p)[:, :cl].astype(np.float64))
            n_dropped += int((f == 0).sum())
            out[l][name] = f
    return out, n_dropped
