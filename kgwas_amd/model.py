"""HeteroGNN for KGWAS on MI355X -- same constructor, forward signature, outputs and ``state_dict`` keys
as the reference model (kgwas/model.py:24-86, kgwas/conv.py:36-232), executed by the fused HIP
kernels in kgwas_amd/csrc.

Execution plan of one HeteroConv layer (all relations at once):
  1. u_r = W_src^T att_src, v_r = W_dst^T att_dst (or W_src^T att_dst for same-type relations,
     conv.py:138) -- the destination-side linear map is only ever used through a_d = <x_d, v_r>
     (conv.py:144,151), so it is never materialised;
  2. a_d = H_d @ V_d^T for the destination rows the layer needs (pruned to hops <= L-l);
  3. kgw_gat_aggregate: Z[i, r] = sum_j softmax_j(leaky_relu(<H_s[j],u_r> + a_d[i,r])) H_s[j];
  4. out_d = relu( [Z[:,r0] | Z[:,r1] | ...] @ [W_r0^T ; W_r1^T ; ...] + sum_r bias_r )  -- the
     per-relation linear maps of conv.py:138/142, the bias of :190, the relation sum of PyG HeteroConv
     (model.py:74) and the ReLU of model.py:75 as ONE GEMM per destination type.
Only what the seeds' prediction depends on is computed (layer l on rows of hop <= L-l); rows the
reference computes and then discards (model.py:86 keeps [:batch_size]) carry zero gradient, so
parameter gradients are identical.

Parameter storage is MI355X-first: the ~30 relations x 5 tensors of a layer live in a handful of packed
tensors (``RelationPack``), laid out so that step 4's concatenated weight is a free view and steps 1-2
are three batched mat-vecs -- a step issues ~100 launches instead of ~1000.  ``state_dict()`` /
``load_state_dict()`` translate to and from the reference's per-relation keys
(``convs.<l>.convs.<src__rel__dst>.{lin_src.weight,lin_dst.weight,att_src,att_dst,bias}``), so a
checkpoint written by either implementation loads in the other (kgwas/utils.py:203-222).
Relations that are structurally disconnected from the read-out (e.g. every layer-2 relation whose
destination is not SNP) are kept in a separate pack that never enters the autograd graph: like in the
reference their gradient is None and Adam (incl. its weight decay) never touches them.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from .graph import GraphSchema, HeteroGraph
from .sampler import SampledBatch, dropout_word, gather_rows_multi, sample_full_graph

_RELVEC_ALL = os.environ.get('KGW_RELVEC_ALL', '1') != '0'      # (A/B: one relation-vector launch per layer as before)

EdgeType = Tuple[str, str, str]
GO_TYPES = ('CellularComponent', 'BiologicalProcess', 'MolecularFunction')
REL_FIELDS = ('att_src', 'att_dst', 'bias', 'lin_src.weight', 'lin_dst.weight')
EDGE_FIELDS = ('lin_edge.weight', 'att_edge')        # relations that carry edge attributes only (gat_edge_dim)


def _signed64(word: int) -> int:
    """Two's-complement int64 view of a 64-bit word (what an int64 tensor holds)."""
    word = int(word) & ((1 << 64) - 1)
    return word - (1 << 64) if word >> 63 else word


def edge_key(et: EdgeType) -> str:
    """ModuleDict key of PyG <= 2.3 HeteroConv."""
    return '__'.join(et)


def _uniform_(t: torch.Tensor, a: float):
    with torch.no_grad():
        t.uniform_(-a, a)
    return t


def _padded_linear(in_l: int, out_l: int, in_p: int, out_p: int) -> nn.Linear:
    """nn.Linear(in_l, out_l) with its default initialisation, stored zero-padded as [out_p, in_p] (see HeteroGNN: a hidden width
    below 128 runs on the 128-wide kernels; the padding stays exactly zero through training)."""
    if (in_l, out_l) == (in_p, out_p):
        return nn.Linear(in_p, out_p)
    src = nn.Linear(in_l, out_l)
    lin = nn.Linear(in_p, out_p)
    with torch.no_grad():
        lin.weight.zero_(); lin.bias.zero_()
        lin.weight[:out_l, :in_l].copy_(src.weight)
        lin.bias[:out_l].copy_(src.bias)
    return lin


class SimpleMLP(nn.Module):
    """kgwas/model.py:10-22.  ``c_logical``: the model's hidden width when it is below the kernels' 128 (zero-padded storage)."""

    def __init__(self, input_dim, hidden_dim, output_dim, c_logical=None):
        super().__init__()
        cl = hidden_dim if c_logical is None else c_logical
        self.FC_hidden = _padded_linear(input_dim, cl, input_dim, hidden_dim)
        self.FC_hidden2 = _padded_linear(cl, cl, hidden_dim, hidden_dim)
        self.FC_output = _padded_linear(cl, cl, hidden_dim, output_dim)
        self.ReLU = nn.ReLU()

    def first(self, x, fixed_shape=False):
        """relu(FC_hidden(x)) -- one autograd node; weight gradient on the split-K MFMA kernel."""
        return ops.linear_relu(x, self.FC_hidden.weight, self.FC_hidden.bias, fixed_shape)

    def tail(self, h1, out=None):
        """FC_output(relu(FC_hidden2(h1))) -- one autograd node."""
        return ops.mlp_tail(h1, self.FC_hidden2.weight, self.FC_hidden2.bias, self.FC_output.weight, self.FC_output.bias,
                            out)

    def tail2(self, h1, out=None):
        """relu(FC_hidden2(h1)): the MLP without FC_output (folded into layer 1, ops.fold_fc_output_hip)."""
        return ops.mlp_tail2(h1, self.FC_hidden2.weight, self.FC_hidden2.bias, out)

    def hidden(self, x, out=None, rows_dev=None, ids=None):
        """h2 = relu(FC_hidden2(relu(FC_hidden(x)))): the MLP without FC_output (folded into layer 1).  ``ids`` (int32): the
        input rows are ``x[ids]`` of a resident feature matrix."""
        if x.requires_grad:
            if ids is not None:
                x = x[ids.long()]
            return self.tail2(self.first(x), out)
        return ops.mlp2(x, self.FC_hidden.weight, self.FC_hidden.bias, self.FC_hidden2.weight, self.FC_hidden2.bias, out, rows_dev,
                        ids)

    def forward(self, x, out=None, rows_dev=None):
        if x.requires_grad:
            return self.tail(self.first(x), out)
        return ops.mlp3(x, self.FC_hidden.weight, self.FC_hidden.bias, self.FC_hidden2.weight, self.FC_hidden2.bias,
                        self.FC_output.weight, self.FC_output.bias, out, rows_dev)




class RelationPack(nn.Module):
    """Parameters of a list of relations of one layer, packed (kgwas/conv.py:81-120 per relation):
    ``w_src_t[i]`` = lin_src.weight^T  ([in k, out c], glorot), ``w_dst_t[j]`` = lin_dst.weight^T of the
    j-th bipartite relation (same-type relations never materialise lin_dst in the reference),
    ``att_src`` / ``att_dst`` (glorot on [1,heads,C/heads], kept flat: column c belongs to head c // (C/heads)), ``bias`` (zeros).
    ``edge_dim`` = D with ``attr_rels`` (relation ids that carry edge attributes; conv.py:95-101): for the j-th attributed relation
    of the pack ``w_edge_t[j]`` = lin_edge.weight^T ([D, out c], glorot on [C, D]) and ``att_edge[j]`` (glorot on [1, 1, C])."""

    def __init__(self, edge_types: List[EdgeType], rel_ids: List[int], C: int, c_logical: int = None, heads: int = 1,
                 edge_dim: int = None, attr_rels=()):
        super().__init__()
        self.n_rels_total = len(edge_types)
        self.rel_ids = list(rel_ids)
        self.rel_types = [edge_types[r] for r in rel_ids]
        n = len(rel_ids)
        bip = [i for i, et in enumerate(self.rel_types) if et[0] != et[2]]
        self.bip = bip
        self.bip_pos = {i: j for j, i in enumerate(bip)}
        cl = self.cl = C if c_logical is None else c_logical      # the model's width; storage is C (= 128) wide, zero beyond cl
        a_w = math.sqrt(6.0 / (cl + cl))        # glorot on [C_out, C_in]
        self.heads = heads
        a_a = math.sqrt(6.0 / (heads + cl // heads))         # glorot on [1, heads, C / heads]: PyG's, over the last two dimensions

        def block(shape, a):
            if cl == C:
                return _uniform_(torch.empty(*shape), a)
            t = torch.zeros(*shape)
            with torch.no_grad():
                if len(shape) == 3:
                    t[:, :cl, :cl].uniform_(-a, a)
                else:
                    t[:, :cl].uniform_(-a, a)
            return t
        self.w_src_t = nn.Parameter(block((n, C, C), a_w))
        self.w_dst_t = nn.Parameter(block((len(bip), C, C), a_w))
        self.att_src = nn.Parameter(block((n, C), a_a))
        self.att_dst = nn.Parameter(block((n, C), a_a))
        self.bias = nn.Parameter(torch.zeros(n, C))
        self.register_buffer('rel_ids_t', torch.tensor(rel_ids, dtype=torch.long), persistent=False)
        self.register_buffer('bip_t', torch.tensor(bip, dtype=torch.long), persistent=False)
        # int32 tables of the HIP kernels: relation id of each packed slot, packed slot of each relation id (-1 =
        # not in this pack), index into w_dst_t of each packed slot (-1 = same-type relation)
        live_of = [-1] * len(edge_types)
        for i, r in enumerate(rel_ids):
            live_of[r] = i
        self._sel_cache = {}                       # relation-sum selectors of ops.layer_transform, by block layout
        self.register_buffer('rel_ids_i32', torch.tensor(rel_ids, dtype=torch.int32), persistent=False)
        self.register_buffer('live_of_rel_i32', torch.tensor(live_of, dtype=torch.int32), persistent=False)
        self.register_buffer('bip_pos_i32', torch.tensor([self.bip_pos.get(i, -1) for i in range(n)], dtype=torch.int32),
                             persistent=False)
        # edge attributes: created only when asked for, after everything else (a model without them draws what it always drew)
        self.edge_dim = edge_dim
        self.attr = [i for i, r in enumerate(rel_ids) if r in set(attr_rels)] if edge_dim else []
        self.attr_pos = {i: j for j, i in enumerate(self.attr)}
        if edge_dim:
            w = torch.zeros(len(self.attr), edge_dim, C)
            with torch.no_grad():
                w[:, :, :cl].uniform_(-math.sqrt(6.0 / (cl + edge_dim)), math.sqrt(6.0 / (cl + edge_dim)))
            self.w_edge_t = nn.Parameter(w)
            self.att_edge = nn.Parameter(block((len(self.attr), C), math.sqrt(6.0 / (1 + cl))))
            self.register_buffer('attr_rel_ids_t', torch.tensor([rel_ids[i] for i in self.attr], dtype=torch.long), persistent=False)

    # reference-named view of one tensor of relation slot i (value or gradient)
    def get(self, i: int, field: str, grad: bool = False):
        def pick(p):
            if grad:
                return None if p.grad is None else p.grad
            return p.detach()
        cl = self.cl
        if field in EDGE_FIELDS:
            j = self.attr_pos[i]
            t = pick(self.w_edge_t if field == 'lin_edge.weight' else self.att_edge)
            if t is None:
                return None
            return t[j, :, :cl].t() if field == 'lin_edge.weight' else t[j, :cl].reshape(1, 1, -1)
        if field == 'lin_src.weight':
            t = pick(self.w_src_t)
            return None if t is None else t[i, :cl, :cl].t()
        if field == 'lin_dst.weight':
            if i not in self.bip_pos:
                return 'lazy'
            t = pick(self.w_dst_t)
            return None if t is None else t[self.bip_pos[i], :cl, :cl].t()
        t = pick(getattr(self, field))
        if t is None:
            return None
        return t[i, :cl].reshape(1, self.heads, -1) if field.startswith('att') else t[i, :cl]

    def set(self, i: int, field: str, value: torch.Tensor):
        cl = self.cl
        with torch.no_grad():
            if field == 'lin_edge.weight':
                self.w_edge_t[self.attr_pos[i], :, :cl].copy_(value.t())
            elif field == 'att_edge':
                self.att_edge[self.attr_pos[i], :cl].copy_(value.reshape(-1))
            elif field == 'lin_src.weight':
                self.w_src_t[i, :cl, :cl].copy_(value.t())
            elif field == 'lin_dst.weight':
                if i in self.bip_pos:
                    self.w_dst_t[self.bip_pos[i], :cl, :cl].copy_(value.t())
            elif field.startswith('att'):
                getattr(self, field)[i, :cl].copy_(value.reshape(-1))
            else:
                getattr(self, field)[i, :cl].copy_(value)


class SagePack(nn.Module):
    """Parameters of a list of SAGEConv((-1,-1), C) relations of one layer, packed (kgwas/model.py:38; PyG SAGEConv:
    aggr='mean', root_weight=True): ``w_l_t[i]`` = lin_l.weight^T ([in, out]) and ``bias[i]`` = lin_l.bias act on the
    mean of the neighbours, ``w_r_t[i]`` = lin_r.weight^T (no bias) on the destination node itself.  Same field
    plumbing as RelationPack (``get`` / ``set`` by reference name)."""

    FIELDS = ('lin_l.weight', 'lin_l.bias', 'lin_r.weight')

    def __init__(self, edge_types: List[EdgeType], rel_ids: List[int], C: int, c_logical: int = None):
        super().__init__()
        self.n_rels_total = len(edge_types)
        self.rel_ids = list(rel_ids)
        n = len(rel_ids)
        cl = self.cl = C if c_logical is None else c_logical
        a = 1.0 / math.sqrt(cl)                    # nn.Linear's default (kaiming_uniform a=sqrt(5)) bound for fan_in = cl

        def block(shape):
            if cl == C:
                return _uniform_(torch.empty(*shape), a)
            t = torch.zeros(*shape)
            with torch.no_grad():
                (t[:, :cl, :cl] if len(shape) == 3 else t[:, :cl]).uniform_(-a, a)
            return t
        self.w_l_t = nn.Parameter(block((n, C, C)))
        self.bias = nn.Parameter(block((n, C)))
        self.w_r_t = nn.Parameter(block((n, C, C)))
        self._sel_cache = {}

    def get(self, i: int, field: str, grad: bool = False):
        p = {'lin_l.weight': self.w_l_t, 'lin_l.bias': self.bias, 'lin_r.weight': self.w_r_t}[field]
        t = p.grad if grad else p.detach()
        if t is None:
            return None
        cl = self.cl
        return t[i, :cl] if field == 'lin_l.bias' else t[i, :cl, :cl].t()

    def set(self, i: int, field: str, value: torch.Tensor):
        cl = self.cl
        with torch.no_grad():
            if field == 'lin_l.bias':
                self.bias[i, :cl].copy_(value)
            else:
                (self.w_l_t if field == 'lin_l.weight' else self.w_r_t)[i, :cl, :cl].copy_(value.t())


class LayerSite(NamedTuple):
    """What follows the transform of layer ``layer`` on the fused and the multi-head route (HeteroGNN._layer_site decides it,
    HeteroGNN._finish_layer runs it): up to three launches, the LAST of which (``writer``) writes the next layer's row blocks, so
    no join_blocks copy is added; the others write temporaries.  ``premasked``: the consumer masks the gradient by (out > 0).
    * root weight: the transform stops at the pre-activation as at a norm site; the root launch adds W_root x of the destination
      rows' own layer input and applies the ReLU (or leaves it to the norm).  From layer 2 on x is a ReLU output whose producer
      runs premasked: ``x_premasked``.
    * layer normalisation: the transform then stops at the pre-activation (its backward has no ReLU left: premasked), the norm's
      launch applies LN and the ReLU.  The next aggregate folds dH *= (H > 0) with H the norm's output: premasked for the norm too.
    * hidden-state dropout: the producer keeps its own (undropped) rows -- it saves them -- and the dropout launch writes the
      dropped state.  The next aggregate folds dH *= (H > 0) with H the DROPPED state (kept and positive); the dropout's backward
      supplies the scale."""
    layer: int
    root: Optional[torch.Tensor]        # the packed root weights (HeteroGNN._root_site) or None
    norm: Optional[tuple]               # the norm's (weight, bias) (HeteroGNN._norm_site) or None
    drop: Optional[tuple]               # the dropout's (p, word) or None
    writer: str                         # 'transform', 'root', 'norm' or 'drop'
    premasked: bool                     # of the transform
    relu: bool                          # of the transform
    root_premasked: bool
    root_relu: bool
    x_premasked: bool
    norm_premasked: bool

    def out_blocks(self, stage: str, nxt):
        return nxt if stage == self.writer else None

    def hbuf_after_mean(self, hbuf):
        """'mean' scales the transform's outputs: they are no longer its blocks, so only a later launch's writing keeps ``hbuf``."""
        return hbuf if self.writer != 'transform' else None


class HeteroGNN(nn.Module):
    """kgwas/model.py:24-86 (same ctor / forward signature).  ``pyg_data`` only needs ``.edge_types``
    and ``.node_types``.  ``gat_dropout`` = p (an extension: the reference's GATConv has the knob, conv.py:44,224, its HeteroGNN
    never passes it): in training mode the softmax weight of every edge is dropped with probability p and the kept ones scaled
    by 1 / (1 - p), inside the aggregate kernels; which edges is a pure function of (``drop_word``, layer, local edge index) --
    kgwdrop_keep in include/kgwas_hip.h.  0 (the default) runs exactly the launches the model ran without it.
    ``gat_split_heads`` (an extension too; KGWAS.initialize_model passes True): ``gat_num_head`` = H in (2, 4) means H heads of width
    hidden / H concatenated back to hidden (PyG's GATConv(hidden // H, heads=H)).  Without it H > 1 keeps the reference's literal
    meaning -- GATConv(hidden, heads=H), a state H * hidden wide that breaks the reference's own read-out -- and is refused.
    ``gat_sigmoid`` / ``gat_temperature`` (extensions, keyword only: the reference's GATConv has both switches, conv.py:49-50,
    217-224, its HeteroGNN never passes them): ``gat_temperature`` = T > 0 divides every attention logit, in the softmax and in the
    gate; ``gat_sigmoid=True`` weights every edge by sigmoid(e / T) instead of by the softmax over its row (independent gates, not
    normalised by degree: ops.gat_aggregate(sigmoid_gate=True)), in training, evaluation, the attention queries and the export.
    GAT only; not with gat_num_head > 1 or gat_dropout > 0.  A gated model does not fold FC_output into layer 1 (``fold_fc``).
    ``gat_edge_dim`` = D in 1..8 (an extension, keyword only: the reference's GATConv has ``edge_dim``, conv.py:46,95-101,207-215, its
    HeteroGNN never passes it): every relation whose ``pyg_data[edge_type].edge_attr`` ([E] or [E, D], aligned with the columns of
    its ``edge_index``) is set gets a bias-free ``lin_edge`` [hidden, D] and an ``att_edge``, and <lin_edge(attr_e), att_edge> joins
    the attention logit of its edges before the LeakyReLU, in every layer (state-dict keys ``convs.<l>.convs.<key>.lin_edge.weight``
    / ``.att_edge``).  The other relations are what they were.  The softmax still sums to one: the model keeps the FC_output fold
    and the fused optimiser launch.  GAT only; not with gat_num_head > 1, gat_dropout > 0 or gat_sigmoid; ``None`` (the default) is
    the model as ever, launch for launch.
    ``gnn_dropout`` = p (an extension, keyword only: the reference's HeteroGNN has no dropout on its hidden state): in training mode
    the output of every message-passing layer but the last -- after its ReLU, for ``gnn_aggr='mean'`` after the 1 / R scale -- goes
    through F.dropout(x, p): every element is dropped with probability p and the kept ones are scaled by 1 / (1 - p), by one
    element-wise launch per layer and pass (ops.hidden_dropout); which elements is a pure function of (``drop_word``, layer, node
    type, local row, column) -- kgwhdrop_keep in include/kgwas_hip.h.  Never on the feature MLPs' output, so the FC_output fold, the
    parameter riders and the fused optimiser launch stay; every backbone, aggregation and attention switch takes it.  Needs
    ``num_layers >= 2`` (there is no site otherwise).  Evaluation, the attention queries and the export never drop; 0 (the default)
    runs exactly the launches the model ran without it.
    ``gnn_norm`` = 'layer' (an extension, keyword only: PyG's BasicGNN runs conv -> norm -> act -> dropout, the reference's HeteroGNN
    has no norm): the pre-activation output y of every message-passing layer but the last -- the relation sum, or the relation
    mean (the 1 / R goes in BEFORE the norm) / min / max -- becomes relu(LN_{l,t}(y)), LN = torch.nn.LayerNorm(hidden, eps=1e-5)
    per node, one per site and per node type that is the destination of some relation (PyG's LayerNorm(mode='node') as to_hetero
    would duplicate it); ``gnn_dropout`` then reads the norm's output.  One forward launch per site, a backward and a fold launch
    (ops.layer_norm_relu, kgwlnorm_* in include/kgwas_hip.h).  Learned, and live in evaluation, the attention queries and the
    export alike (the export, which applies no ReLU between the layers, applies the norm without one).  The parameters of a site
    are ONE packed pair ``norm_weight[l - 1]`` / ``norm_bias[l - 1]`` [n_node_types, 128]: row t for node type t, the columns past
    the model's width and the rows of types that receive no relation zero and kept zero; under the reference's names
    ``norms.<l - 1>.<node type>.weight`` / ``.bias`` (the index of the ``convs.<l - 1>`` they follow) at the model's own width.  A
    type that has no rows in a batch's layer gets ZERO gradient rows, where one torch module per type would leave ``grad`` None:
    with weight decay such a row still decays.  The FC_output fold, the parameter riders and the fused optimiser launch stay (the
    norm sits after the layer-1 transform).  Needs ``num_layers >= 2``; ``None`` (the default) is the model as ever, launch for
    launch and bit for bit.
    ``gnn_root_weight`` = True (an extension, keyword only: PyG's SAGEConv.lin_r, RGCNConv.root, GATConv(residual=True); the
    reference builds GATConv(add_self_loops=False) for every relation and a SNP has no SNP-SNP relation, so a node's own state
    never enters its own update): for every layer l = 1 .. L and every node type t that is the destination of a relation the
    pre-activation of destination node i becomes  y_i = combine_r(conv_r(...)_i) + W_root[l][t] x_i  with x_i the node's OWN layer-l
    input -- at layer 1 its feature MLP's output, later the state the previous layer left (after its norm, ReLU and, in training,
    hidden dropout: what the relations of layer l read for that node as a source).  The 1 / R of 'mean' scales the relation part
    only, 'min' / 'max' add the root term after the reduction; everything after y (norm, ReLU, dropout, read-out) is as it was.  One
    forward and one backward launch per layer (ops.root_linear, kgwroot_* in include/kgwas_hip.h) plus the weight-gradient products;
    learned and live in evaluation, the attention queries and the export.  The destination rows of a type are the leading
    ``lay_rows[l - 1][t]`` rows of that type's layer input (the sampler's layout: seeds, then hop 1, ...; the SAGE root term and the
    read-out rely on the same).  Parameters: ONE packed tensor per layer ``root_weight[l - 1]`` [n_node_types, 128, 128], slice t
    a bias-free nn.Linear [out, in] for node type t (glorot, as lin_src), the padding and the slices of types that receive no
    relation zero and kept zero; drawn AFTER every other parameter, so the other parameters are those of a default model at the
    same seed; under the names ``roots.<l - 1>.<node type>.weight`` at the model's own width.  A type without rows in a batch's
    layer gets a ZERO gradient slice (the ``gnn_norm`` convention).  Layer 1 runs UNFOLDED (``fold_fc`` False, as a gated model's):
    FC_output would get gradient from the fold and from the root product, which the one-source-per-tensor records of the fused
    optimiser launch do not take.  GAT only (SAGE's lin_r IS a root weight per relation: ValueError); ``False`` (the default) is
    the model as ever, launch for launch and bit for bit."""

    def __init__(self, pyg_data, hidden_channels, out_channels, num_layers, gnn_backbone, gnn_aggr,
                 snp_init_dim_size, gene_init_dim_size, go_init_dim_size, gat_num_head, no_relu=False, gat_dropout=0.0,
                 gat_split_heads=False, *, gat_sigmoid=False, gat_temperature=1.0, gat_edge_dim=None, gnn_dropout=0.0,
                 gnn_norm=None, gnn_root_weight=False):
        super().__init__()
        if gnn_backbone not in ('GAT', 'SAGE'):
            raise NotImplementedError(f"backbone {gnn_backbone!r}: 'GAT' (the reference default, kgwas.py:52) and 'SAGE' "
                                      "run on the fused MI355X path; GCNConv / SGConv cannot take the bipartite "
                                      "relations HeteroConv hands them (kgwas/model.py:44-46)")
        self.backbone = gnn_backbone
        gat_dropout = float(gat_dropout)
        if not 0.0 <= gat_dropout < 1.0:
            raise ValueError(f'gat_dropout {gat_dropout}: 0 <= p < 1')
        if gat_dropout != 0.0 and gnn_backbone == 'SAGE':
            raise ValueError("gat_dropout needs gnn_backbone='GAT': SAGE has no attention weights to drop (its aggregate merely "
                             "reuses the kernels)")
        self.gat_dropout = gat_dropout
        gnn_dropout = float(gnn_dropout)
        if not 0.0 <= gnn_dropout < 1.0:
            raise ValueError(f'gnn_dropout {gnn_dropout}: 0 <= p < 1')
        if gnn_dropout != 0.0 and int(num_layers) < 2:
            raise ValueError(f'gnn_dropout > 0 with num_layers = {num_layers}: the hidden state is dropped BETWEEN message-passing '
                             'layers, and one layer has no such site')
        self.gnn_dropout = gnn_dropout
        if gnn_norm not in (None, 'layer'):
            raise ValueError(f"gnn_norm {gnn_norm!r}: None (the reference's model) or 'layer'")
        if gnn_norm is not None and int(num_layers) < 2:
            raise ValueError(f'gnn_norm with num_layers = {num_layers}: the hidden state is normalised BETWEEN message-passing '
                             'layers, and one layer has no such site')
        self.gnn_norm = gnn_norm
        self.gnn_root_weight = bool(gnn_root_weight)
        if self.gnn_root_weight and gnn_backbone == 'SAGE':
            raise ValueError("gnn_root_weight needs gnn_backbone='GAT': SAGE's lin_r already is a root weight per relation")
        # the 64-bit word of the step's masks (attention and hidden-state dropout alike: the rules keep them apart), resident on
        # the device: the kernels read it when they run, so a captured step replays with whatever the trainer copied here
        # (set_dropout_word / GraphTrainStep).  Not part of the state_dict.
        self.register_buffer('drop_word', torch.tensor([_signed64(dropout_word(0, 0, 0))], dtype=torch.int64), persistent=False)
        if gnn_aggr not in ('sum', 'mean', 'min', 'max'):
            raise NotImplementedError(f"gnn_aggr {gnn_aggr!r}: 'sum' (the reference default, fused), 'mean', 'min' and 'max' are "
                                      "built; 'cat' widens the hidden state to R*128 and breaks the reference's own "
                                      "read-out (kgwas/model.py:50), like the reference's literal gat_num_head > 1")
        self.aggr = gnn_aggr
        if not 1 <= hidden_channels <= 128:
            raise NotImplementedError('gnn_hidden_dim > 128: the fused kernels are 128 wide (narrower models run on them '
                                      'zero-padded; wider ones would need a second instantiation of every kernel -- DESIGN.md section 8)')
        # gat_num_head = H > 1 with this constructor's reference signature alone keeps the reference's literal meaning,
        # GATConv(hidden, heads=H), which widens the state to H * hidden and breaks the reference's own read-out (model.py:50 expects
        # hidden_channels inputs): refused, as ever.  ``gat_split_heads=True`` (an extension; KGWAS.initialize_model passes it) selects
        # what every GAT paper and PyG example means by H heads: GATConv((-1,-1), hidden // H, heads=H) -- H heads of width hidden / H,
        # concatenated back to hidden.
        if gat_num_head != int(gat_num_head) or int(gat_num_head) < 1:
            raise NotImplementedError(f'gat_num_head {gat_num_head!r}: 1, 2 or 4 heads')
        gat_num_head = int(gat_num_head)
        if gat_num_head != 1 and not gat_split_heads:
            raise NotImplementedError('gat_num_head > 1 as the reference builds it (GATConv(hidden, heads=H)) widens the hidden state '
                                      'to H * hidden and breaks the reference read-out (model.py:50 expects hidden_channels inputs); '
                                      'gat_split_heads=True builds H heads of width hidden / H concatenated back to hidden '
                                      '(KGWAS.initialize_model(gat_num_head=H) does)')
        if gat_num_head != 1:
            if gnn_backbone == 'SAGE':
                raise ValueError("gat_num_head > 1 needs gnn_backbone='GAT': SAGE has no attention heads")
            if gat_num_head not in (2, 4):
                raise NotImplementedError(f'gat_num_head {gat_num_head}: the aggregate kernels are built for 1, 2 and 4 heads')
            if hidden_channels % gat_num_head:
                raise NotImplementedError(f'gat_num_head {gat_num_head} does not divide gnn_hidden_dim {hidden_channels}: the heads '
                                          'are hidden / H wide and concatenated back to hidden')
            if gnn_aggr not in ('sum', 'mean'):
                raise NotImplementedError(f"gat_num_head > 1 with gnn_aggr {gnn_aggr!r}: the multi-head route is built for the relation "
                                          "'sum' and 'mean'")
            if gat_dropout != 0.0:
                raise NotImplementedError('gat_num_head > 1 with gat_dropout > 0: the dropout kernels are single-head')
        self.heads = gat_num_head
        gat_temperature = float(gat_temperature)
        if not (math.isfinite(gat_temperature) and gat_temperature > 0.0):
            raise ValueError(f'gat_temperature {gat_temperature}: a finite T > 0')
        self.gat_sigmoid = bool(gat_sigmoid)
        if self.gat_sigmoid:
            if gnn_backbone == 'SAGE':
                raise ValueError("gat_sigmoid needs gnn_backbone='GAT': SAGE has no attention logits to gate")
            if gat_num_head > 1:
                raise NotImplementedError('gat_sigmoid with gat_num_head > 1: the gate kernels are single-head')
            if gat_dropout != 0.0:
                raise NotImplementedError('gat_sigmoid with gat_dropout > 0: the dropout kernels weight by the softmax')
        self.node_types = list(pyg_data.node_types)
        self.edge_types = [tuple(e) for e in pyg_data.edge_types]
        self.schema = GraphSchema(self.node_types, self.edge_types)
        sc = self.schema
        self.edge_dim, self.attr_rels = None, []
        if gat_edge_dim is not None:
            if gnn_backbone == 'SAGE':
                raise ValueError("gat_edge_dim needs gnn_backbone='GAT': SAGE has no attention logits for the attributes to enter")
            what = [n for n, v in (('gat_num_head > 1', gat_num_head > 1), ('gat_dropout > 0', gat_dropout != 0.0),
                                   ('gat_sigmoid', self.gat_sigmoid)) if v]
            if what:
                raise NotImplementedError(f'gat_edge_dim with {", ".join(what)}: the edge-attribute forward is built for one head of '
                                          'undropped softmax weights')
            if gat_edge_dim != int(gat_edge_dim) or not 1 <= int(gat_edge_dim) <= 8:
                raise ValueError(f'gat_edge_dim {gat_edge_dim!r}: 1 to 8 attribute columns')
            self.edge_dim = int(gat_edge_dim)
            widths = {}
            for r, et in enumerate(self.edge_types):
                a = getattr(pyg_data[et], 'edge_attr', None)
                if a is not None:
                    widths[r] = 1 if a.dim() == 1 else int(a.shape[1])
            if not widths:
                raise ValueError('gat_edge_dim is set but no relation of the graph carries edge_attr (KGWAS_Data.set_edge_attr)')
            if set(widths.values()) != {self.edge_dim}:
                raise ValueError(f'gat_edge_dim {self.edge_dim} but the relations carry attributes of width '
                                 f'{sorted(set(widths.values()))}: one width for all relations')
            self.attr_rels = sorted(widths)
        self.num_layers = num_layers
        # gnn_hidden_dim < 128 (kgwas/kgwas.py:52): the model is embedded in the 128-wide kernels -- every hidden tensor and
        # parameter zero-padded to 128.  Exact: padded channels are 0 after every Linear / ReLU, padded parameters receive a
        # gradient of exactly 0 (their inputs or their output gradients are 0) and Adam with L2 leaves 0 at 0; checkpoints,
        # state_dict and gradients are exposed at the model's own width.  Costs what 128 costs.
        self.hidden_logical = cl = int(hidden_channels)
        hidden_channels = 128
        self.hidden = hidden_channels
        self.negative_slope, self.temperature = 0.2, gat_temperature      # conv.py:43,50 (model.py:40-42 passes neither: 0.2, 1)
        self.rel_fields = REL_FIELDS if gnn_backbone == 'GAT' else SagePack.FIELDS
        self.live_rel, self.live_types = sc.live_relations(num_layers, 'SNP')
        self.live_packs = nn.ModuleList()
        self.dead_packs = nn.ModuleList()
        self._slot: List[Dict[int, Tuple[str, int]]] = []        # per layer: relation id -> (pack, index)
        self._dst_range: List[Dict[int, Tuple[int, int]]] = []   # per layer: dst type -> [lo, hi) in live pack
        for l in range(1, num_layers + 1):
            live = set(self.live_rel[l])
            order = [r for t in range(sc.NT) for r in sc.rels_by_dst[t] if r in live]   # grouped by dst type
            dead = [r for r in range(sc.NR) if r not in live]
            Pack = RelationPack if gnn_backbone == 'GAT' else SagePack
            kw = {'heads': gat_num_head} if gnn_backbone == 'GAT' else {}
            if self.edge_dim is not None:
                kw.update(edge_dim=self.edge_dim, attr_rels=self.attr_rels)
            self.live_packs.append(Pack(self.edge_types, order, hidden_channels, cl, **kw))
            self.dead_packs.append(Pack(self.edge_types, dead, hidden_channels, cl, **kw))
            slot = {r: ('live', i) for i, r in enumerate(order)}
            slot.update({r: ('dead', i) for i, r in enumerate(dead)})
            self._slot.append(slot)
            rng, lo = {}, 0
            for t in range(sc.NT):
                k = sum(1 for r in sc.rels_by_dst[t] if r in live)
                if k:
                    assert k == len(sc.rels_by_dst[t])
                    rng[t] = (lo, lo + k)
                    lo += k
            self._dst_range.append(rng)
        self.snp_feat_mlp = SimpleMLP(snp_init_dim_size, hidden_channels, hidden_channels, cl)
        self.go_feat_mlp = SimpleMLP(go_init_dim_size, hidden_channels, hidden_channels, cl)
        self.gene_feat_mlp = SimpleMLP(gene_init_dim_size, hidden_channels, hidden_channels, cl)
        self.ReLU = nn.ReLU()
        self.lin = _padded_linear(cl, out_channels, hidden_channels, out_channels)
        self.no_relu = no_relu
        self.last_attention = None
        # FC_output of the feature MLPs folded into the layer-1 relation parameters (ops.fold_fc_output_hip): exact, removes a
        # 128 x 128 Linear (forward, dX, dW) over every sampled node.  GAT with a relation SUM only: SAGE has a root term and
        # min / max are not linear in the messages.
        import os
        self.fold_fc = gnn_backbone == 'GAT' and gnn_aggr in ('sum', 'mean') and os.environ.get('KGW_FOLD_FC', '1') == '1'
        if gat_num_head > 1:
            # several heads take the unfused route (_head_layers): no FC_output fold, no parameter riders.  head_mask[h, c] = 1 for
            # the columns of head h (c // (cl / H) == h), 0 elsewhere and on the zero-padded columns cl..127
            self.fold_fc = False
            hm = torch.zeros(gat_num_head, hidden_channels)
            for hd in range(gat_num_head):
                hm[hd, hd * (cl // gat_num_head):(hd + 1) * (cl // gat_num_head)] = 1.0
            self.register_buffer('head_mask', hm, persistent=False)
        if self.gat_sigmoid:
            # the fold moves FC_output's constant c out of the messages as c * sum_j alpha_ij = c, and the gates do not sum to 1: the
            # gated model takes the unfolded route, as a dropping step does (_dropout).  OPEN: keeping the fold by having the forward
            # emit sum_j g_e per row (gamma would be scaled by it in the transform) -- DESIGN.md section 8.
            self.fold_fc = False
        if self.fold_fc:
            mlp_of = {'SNP': 0, 'Gene': 1}
            order = self.live_packs[0].rel_ids
            try:
                sm = [mlp_of.get(self.edge_types[r][0], 2) for r in order]
                dm = [mlp_of.get(self.edge_types[r][2], 2) for r in order]
                for r in order:
                    for t in (self.edge_types[r][0], self.edge_types[r][2]):
                        self._mlp_for(t)
            except KeyError:
                self.fold_fc = False
            if self.fold_fc:
                self._fold_used = set(sm) | set(dm)
                import numpy as np
                self._fold_tab = (np.asarray(order, dtype=np.int32), np.asarray(sm, dtype=np.int32), np.asarray(dm, dtype=np.int32))
                self.register_buffer('_fold_src_m', torch.tensor(sm, dtype=torch.long), persistent=False)
                self.register_buffer('_fold_dst_m', torch.tensor(dm, dtype=torch.long), persistent=False)
        # layer normalisation: one packed (weight, bias) pair per site l = 1 .. L - 1, row t = node type t; none without gnn_norm, so
        # the default model's parameters are what they were
        self.norm_types = [t for t in range(sc.NT) if sc.rels_by_dst[t]] if gnn_norm is not None else []
        self.norm_weight, self.norm_bias = nn.ParameterList(), nn.ParameterList()
        for _ in range(num_layers - 1 if gnn_norm is not None else 0):
            w = torch.zeros(sc.NT, hidden_channels)
            w[self.norm_types, :cl] = 1.0
            self.norm_weight.append(nn.Parameter(w))
            self.norm_bias.append(nn.Parameter(torch.zeros(sc.NT, hidden_channels)))
        # dead packs never receive gradients; keep them out of autograd entirely
        for p in self.dead_packs.parameters():
            p.requires_grad_(False)
        # root weight: one packed tensor per layer, slice t = node type t's bias-free Linear [out, in]; none without gnn_root_weight,
        # and drawn LAST, so the default model's parameters -- and a root model's other parameters -- are what they were
        self.root_types = [t for t in range(sc.NT) if sc.rels_by_dst[t]] if self.gnn_root_weight else []
        self.root_weight = nn.ParameterList()
        if self.gnn_root_weight:
            # FC_output would get gradient from the fold AND from the root product of layer 1's destination rows; the fused
            # optimiser's records hold one source per tensor: layer 1 runs unfolded (OPEN)
            self.fold_fc = False
            a_w = math.sqrt(6.0 / (cl + cl))                  # glorot on [C_out, C_in]: RelationPack's rule for lin_src
            for _ in range(num_layers):
                w = torch.zeros(sc.NT, hidden_channels, hidden_channels)
                for t in self.root_types:
                    _uniform_(w[t, :cl, :cl], a_w)
                self.root_weight.append(nn.Parameter(w))

    # ------------------------------------------------------------------------------------------
    def _mlp_for(self, t: str) -> SimpleMLP:
        if t == 'SNP':
            return self.snp_feat_mlp
        if t == 'Gene':
            return self.gene_feat_mlp
        if t in GO_TYPES:
            return self.go_feat_mlp
        raise KeyError(f'no feature MLP for node type {t!r} (kgwas/model.py:56-60)')

    def _embed(self, batch: SampledBatch, x_dict, t: str, out=None, fold=False):
        """Feature MLP of the sampled nodes of type t (model.py:56-60).  When most of a type is in the batch
        and its features are wide (the 5120 / 57742-wide gene matrix), the first Linear runs on the RESIDENT
        matrix and the 128-wide result is sliced, instead of slicing 20 KB rows first: same values, the
        x[n_id] copy (kgwas.py:135 moves it over PCIe every step) disappears."""
        mlp = self._mlp_for(t)
        dg = batch.dg
        n = batch.n_nodes[t]
        if n == 0:
            return torch.zeros(0, self.hidden, device=self.lin.weight.device)
        if out is not None and out.n != n:
            out = None
        lazy = getattr(x_dict, 'kgw_batch', None) is batch and t in dg.x
        if lazy and not dg.full_graph:
            X = dg.x[t]
            if X.shape[1] >= 512 and 2 * n > X.shape[0]:
                i = dg.schema.type_id[t]
                g2l = batch.buf.g2l[dg.node_base[i]:dg.node_base[i] + X.shape[0]]
                if fold and ops.resident_mlp2_ok(X, mlp.FC_hidden.weight, mlp.FC_hidden2.weight, n):
                    # (static layout: the block is padded to its capacity; the count of real rows lives on the device)
                    real = batch.rows_dev(t) if n == batch.lay_src(1, i) else None
                    return ops.resident_mlp2(X, mlp.FC_hidden.weight, mlp.FC_hidden.bias, mlp.FC_hidden2.weight,
                                             mlp.FC_hidden2.bias, batch.n_id(t), g2l, out, rows_real=real)
                h1 = ops.resident_linear_relu_rows(X, mlp.FC_hidden.weight, mlp.FC_hidden.bias, batch.n_id(t), g2l)
                return mlp.tail2(h1, out) if fold else mlp.tail(h1, out)
        # static layout: the row block is padded to its capacity; the kernels skip the padding (count on the device)
        rd = batch.rows_dev(t) if n == batch.lay_src(1, dg.schema.type_id[t]) else None
        if fold and lazy and dict.get(x_dict, t) is None and dg.x[t].shape[1] <= 20:
            # narrow features (the 20-wide SNP rows): the x[n_id] slicing happens inside the fused two-layer kernel
            return mlp.hidden(dg.x[t], out, rd, ids=batch.n_id(t))
        return mlp.hidden(x_dict[t], out, rd) if fold else mlp(x_dict[t], out, rd)

    def _layer_input(self, batch: SampledBatch, l: int):
        """Preallocated type-major input matrix of layer l and one RowBlock per node type that has rows in it."""
        m, sc = batch.meta, self.schema
        total = int(m.src_base[l - 1][sc.NT])
        buf = torch.empty(max(total, 1), self.hidden, device=self.lin.weight.device)
        blocks = {name: ops.RowBlock(buf, int(m.src_base[l - 1][t]), int(m.lay_src[l - 1][t]))
                  for t, name in enumerate(sc.node_types) if int(m.lay_src[l - 1][t])}
        return buf, blocks

    def _layer_parts(self, batch: SampledBatch, l: int, h: Dict[str, torch.Tensor]):
        """The state of every node type that sends or receives messages in layer l (its leading ``lay_src`` rows), in type order, and
        their (row offset, rows) spans in the type-major layer input (src_base)."""
        m = batch.meta
        parts, spans = [], []
        for t, name in enumerate(self.schema.node_types):
            ns = int(m.lay_src[l - 1][t])
            if ns:
                if name not in h or h[name].shape[0] < ns:
                    raise RuntimeError(f'layer {l}: node type {name!r} takes part in the layer but has no '
                                       f'incoming relation to produce its layer-{l - 1} state')
                parts.append(h[name] if h[name].shape[0] == ns else h[name][:ns])
                spans.append((int(m.src_base[l - 1][t]), ns))
        return parts, spans

    def _join_layer_input(self, batch: SampledBatch, l: int, h: Dict[str, torch.Tensor], hbuf=None):
        """The type-major input matrix H of layer l from the per-type states ``h``, joined in ``hbuf`` (``_layer_input(batch, l)``,
        allocated here when the caller carries none), or the one part itself when it is the whole matrix."""
        parts, spans = self._layer_parts(batch, l, h)
        if hbuf is None:
            hbuf, _ = self._layer_input(batch, l)
        return ops.join_blocks(hbuf, spans, parts) if len(parts) != 1 or parts[0].shape[0] != hbuf.shape[0] else parts[0]

    def _dst_blocks(self, batch: SampledBatch, l: int):
        """The destination blocks of layer l, one per node type that receives messages: (``tys``, the type ids; ``blocks`` =
        [(lo, hi, z0, rows)]: the type's relation slots [lo, hi) in the layer's pack, its offset in the aggregate Z, its rows)."""
        m, rng = batch.meta, self._dst_range[l - 1]
        tys = [t for t in range(self.schema.NT) if int(m.lay_rows[l - 1][t])]
        return tys, [(rng[t][0], rng[t][1], int(m.z_base[l - 1][t]), int(m.lay_rows[l - 1][t])) for t in tys]

    def _embed_all(self, batch: SampledBatch, x_dict, blocks=None, fold=False):
        """All feature MLPs (model.py:56-60).  The three GO types share ``go_feat_mlp`` (model.py:58-60): their
        rows go through it as ONE matrix.  ``blocks``: RowBlocks of the first layer's input to write into."""
        h = {}
        blocks = blocks or {}
        # (n_nodes first: touching a lazy x_dict entry would gather that type's rows a second time)
        go = [t for t in self.node_types if t in GO_TYPES and t in x_dict and
              (batch.n_nodes[t] if t in batch.n_nodes else x_dict[t].shape[0]) > 0]
        if len(go) > 1:
            lazy = getattr(x_dict, 'kgw_batch', None) is batch and all(t in batch.dg.x for t in go) and \
                len({batch.dg.x[t].shape[1] for t in go}) == 1
            fused_jobs = None
            if lazy and fold:
                mlp = self.go_feat_mlp
                fj = [(batch.dg.x[t], batch.n_id(t)) for t in go]
                if ops.mlp2_gathered_ok(fj, mlp.FC_hidden.weight, mlp.FC_hidden2.weight):
                    fused_jobs = fj         # gather + both hidden layers in one launch (kgw_mlp2w_fwd)
            if fused_jobs is not None:
                ns = [batch.n_nodes[t] for t in go]
                xg = xs = None
            elif lazy:            # gather the three types' rows straight into one matrix (no concatenation copy)
                ns = [batch.n_nodes[t] for t in go]
                xg = torch.empty(sum(ns), batch.dg.x[go[0]].shape[1], device=self.lin.weight.device)
                off, jobs = 0, []
                for t, n in zip(go, ns):
                    jobs.append((batch.dg.x[t], batch.n_id(t), xg[off:off + n]))
                    off += n
                gather_rows_multi(jobs)                       # one launch for the three types
                xs = None
            else:
                xs = [x_dict[t] for t in go]
                ns = [x.shape[0] for x in xs]
                xg = torch.cat(xs, 0)
            out = None
            bl = [blocks.get(t) for t in go]
            if all(b is not None and b.n == n for b, n in zip(bl, ns)) and \
                    all(bl[k + 1].lo == bl[k].lo + bl[k].n for k in range(len(bl) - 1)):
                out = ops.RowBlock(bl[0].buf, bl[0].lo, sum(ns))          # the GO blocks are adjacent: one output
            if fused_jobs is not None:
                mlp = self.go_feat_mlp
                y = ops.mlp2_gathered(fused_jobs, mlp.FC_hidden.weight, mlp.FC_hidden.bias, mlp.FC_hidden2.weight,
                                      mlp.FC_hidden2.bias, out)
            else:
                y = self.go_feat_mlp.hidden(xg, out) if fold else self.go_feat_mlp(xg, out)
            for t, piece in zip(go, ops.split_rows(y, ns)):
                h[t] = piece
        for t in self.node_types:
            if t in x_dict and t not in h:
                h[t] = self._embed(batch, x_dict, t, blocks.get(t), fold)
        return h

    def _combine_relations(self, o: torch.Tensor) -> torch.Tensor:
        """HeteroConv(aggr) over the relation axis of per-relation outputs o [R, rows, C] (PyG hetero_conv.group:
        stack + reduce; kgwas/model.py:47): used for 'min' / 'max', which cannot be folded into one GEMM."""
        if o.shape[0] == 1:
            return o[0]
        return getattr(torch, self.aggr)(o, dim=0).values

    def _relation_products(self, zr: torch.Tensor, w_t: torch.Tensor, bias: torch.Tensor, lo: int, hi: int, what: str):
        """'min' / 'max': the per-relation outputs o[r] = zr[r] @ w_t[lo + r] + bias[lo + r] of one destination type, [R, rows, C]: one
        own-kernel product per relation (the library-free form) or, where the library is allowed, one batched product, noted."""
        if ops.LIBRARY_GEMM.own_first:
            return torch.stack([ops.linear_act(zr[r].contiguous(), w_t[lo + r], bias[lo + r], relu=False) for r in range(hi - lo)])
        ops.LIBRARY_GEMM.note(what, hi - lo, zr.shape[1], self.hidden)
        return torch.baddbmm(bias[lo:hi].unsqueeze(1), zr, w_t[lo:hi])

    def _sage_layers(self, batch: SampledBatch, h: Dict[str, torch.Tensor], hbuf=None, hdrop=None):
        """SAGE backbone (kgwas/model.py:38,74-75): out_d = relu(sum_r [lin_l^r(mean_{j->i} h_s[j]) + lin_r^r(h_d[i])]).
        The neighbour mean IS the attention aggregate with all logits equal: the same kernels run with zero attention
        vectors (alpha = 1/deg; rows without in-edges stay zero like PyG's mean), forward and backward; the root
        term is one more product per destination type with the relation-summed lin_r."""
        sc, C = self.schema, self.hidden
        dev = self.lin.weight.device
        zeros = torch.zeros(sc.NR, C, device=dev)
        for l in range(1, self.num_layers + 1):
            P: SagePack = self.live_packs[l - 1]
            H = self._join_layer_input(batch, l, h, hbuf)
            hbuf = None
            Z, _, _ = ops.gat_aggregate(batch, l, H, zeros, zeros, self.negative_slope, self.temperature)
            h_next = {}
            for t, (lo, hi, z0, rows) in zip(*self._dst_blocks(batch, l)):
                name, R = sc.node_types[t], hi - lo
                if self.aggr in ('min', 'max'):
                    zr = Z[z0:z0 + rows * R].view(rows, R, C).transpose(0, 1)                    # [R, rows, C]
                    o = self._relation_products(zr, P.w_l_t, P.bias, lo, hi, 'sage min/max per-relation outputs')
                    if ops.LIBRARY_GEMM.own_first:          # (library-free form: one own-kernel product per relation and term)
                        hr = h[name][:rows].contiguous()
                        zero = torch.zeros(C, device=dev)
                        o = o + torch.stack([ops.linear_act(hr, P.w_r_t[lo + r], zero, relu=False) for r in range(R)])
                    else:
                        o = o + torch.matmul(h[name][:rows].unsqueeze(0), P.w_r_t[lo:hi])
                    h_next[name] = self._combine_relations(o)
                    continue
                x = Z[z0:z0 + rows * R].view(rows, R * C)
                y = ops.linear_act(x, P.w_l_t[lo:hi].reshape(R * C, C), P.bias[lo:hi].sum(0), relu=False)
                if ops.LIBRARY_GEMM.own_first:
                    y = y + ops.linear_act(h[name][:rows].contiguous(), P.w_r_t[lo:hi].sum(0), torch.zeros(C, device=dev), relu=False)
                else:
                    ops.LIBRARY_GEMM.note('sage root term', rows, C, C)
                    y = y + h[name][:rows] @ P.w_r_t[lo:hi].sum(0)        # root term: sum_r lin_r^r(h_d[i])
                if self.aggr == 'mean':
                    y = y * (1.0 / R)
                h_next[name] = y
            h = self._drop_hidden(l, self._activate(l, h_next), hdrop)
        return h, []

    def _all_layer_params(self, batch: SampledBatch, folded: bool):
        """_layer_params for every layer with the relation vectors of ALL layers from one launch (ops.rel_vectors_all): they
        depend on the parameters only.  Their backward then is one launch too, after the first layer's."""
        dev = self.lin.weight.device
        blocks_all = [self._dst_blocks(batch, l)[1] for l in range(1, self.num_layers + 1)]
        zeros = [ops.aggregate_workspace(batch, l, dev) for l in range(1, self.num_layers + 1)]
        rv =ops.rel_vectors_all([self.live_packs[l] for l in range(self.num_layers)], blocks_all, zeros)
        return [self._layer_params(batch, l, folded, relvec=rv[l - 1], zbuf=zeros[l - 1]) for l in range(1, self.num_layers + 1)]

    def _layer_params(self, batch: SampledBatch, l: int, folded: bool, relvec=None, zbuf=None):
        """Everything layer l needs that depends on the PARAMETERS only (and on the batch's static row counts): the destination
        blocks, the zeroed aggregate workspace, u_r / v_r / summed biases (ops.rel_vectors) and, for a folded layer 1, the
        fold of FC_output into them.  No activation enters."""
        P: RelationPack = self.live_packs[l - 1]
        tys, blocks = self._dst_blocks(batch, l)
        # u_r = W_src^T att_src ; v_r = W_dst^T att_dst (W_src^T att_dst for same-type relations) and the summed
        # bias of every destination block: one launch
        # ... and the zero fill of the aggregate's workspace rides in the same launch
        zws = ops.aggregate_workspace(batch, l, self.lin.weight.device)
        # (the weights reach the transform / the fold THROUGH that node: their gradient is added inside its backward kernel)
        if relvec is not None:                          # (all layers' vectors came out of ONE launch: _all_layer_params)
            U, V, bsum, Wv = relvec
            zws = zbuf
        else:
            U, V, bsum, Wv = ops.rel_vectors(P, blocks, zero=zws, pass_weights=True)
        Wp = gam = kap = None
        if folded and l == 1:
            # (an MLP no live layer-1 relation touches -- the GO one of a 1-layer model -- stays out of the graph: like
            # in the reference its parameters get no gradient and Adam skips them)
            mlps = (self.snp_feat_mlp, self.gene_feat_mlp, self.go_feat_mlp)
            fc = []
            for k, mm in enumerate(mlps):
                used = k in self._fold_used
                fc += [mm.FC_output.weight if used else mm.FC_output.weight.detach(),
                       mm.FC_output.bias if used else mm.FC_output.bias.detach()]
            U, V, kap, Wp, gam = ops.fold_fc_output_hip(P, U, V, fc, self._fold_tab, weight=Wv)
        return tys, blocks, zws, U, V, bsum, Wv, kap, Wp, gam, self._edge_term(batch, l, (P,))

    def _edge_term(self, batch: SampledBatch, l: int, packs):
        """The per-edge logit term of layer l's attributed relations (ops.edge_logit_term), or None for a model without edge
        attributes / a layer that computes no attributed relation.  w_r = lin_edge.weight^T att_edge [n_rels, 8] by relation id is
        formed by element-wise framework ops (as ``_head_vectors`` forms u^h, v^h): a product, a sum, the padding to 8 columns and the
        scatter to relation ids."""
        if self.edge_dim is None:
            return None
        dg = batch.dg
        if dg.eattr_rels != self.attr_rels or dg.eattr_dim != self.edge_dim:      # (both fixed when the graph / the model was built)
            have = dg.eattr_rels
            missing = [self.edge_types[r] for r in self.attr_rels if r not in have]
            raise ValueError(f'the model was built with edge attributes of width {self.edge_dim} on {len(self.attr_rels)} relations; the '
                             f'batch\'s graph carries width {dg.eattr_dim} on {len(have)}' +
                             (f' (no edge_attr for {missing[:3]})' if missing else ''))
        W = None
        for P in packs:
            if not len(P.attr):
                continue
            w = (P.w_edge_t * P.att_edge.unsqueeze(1)).sum(2)                  # [n_attr, D]
            if self.edge_dim < 8:
                w = torch.nn.functional.pad(w, (0, 8 - self.edge_dim))
            w = w.new_zeros(self.schema.NR, 8).index_copy(0, P.attr_rel_ids_t, w)
            W = w if W is None else W + w
        return None if W is None else ops.edge_logit_term(batch, l, W)

    def _head_vectors(self, P: RelationPack):
        """u_r^h[k] = sum_{c in head h} W_src^T[k, c] att_src[c] and v_r^h likewise (W_dst of a bipartite relation, W_src of a
        same-type one) for the pack's relations, [H, n_rels_total, 128] by relation id (zero rows for relations outside the pack):
        element-wise products and sums over a [H, n, 128, 128] tensor -- no library GEMM."""
        hm = self.head_mask
        a_s = P.att_src.unsqueeze(0) * hm.unsqueeze(1)                       # [H, n, C]: att_src restricted to the head's columns
        a_d = P.att_dst.unsqueeze(0) * hm.unsqueeze(1)
        w_dst = P.w_src_t.index_copy(0, P.bip_t, P.w_dst_t) if len(P.bip) else P.w_src_t
        u = (P.w_src_t.unsqueeze(0) * a_s.unsqueeze(2)).sum(3)               # [H, n, C(k)]
        v = (w_dst.unsqueeze(0) * a_d.unsqueeze(2)).sum(3)
        U = u.new_zeros(self.heads, self.schema.NR, self.hidden).index_copy(1, P.rel_ids_t, u)
        V = v.new_zeros(self.heads, self.schema.NR, self.hidden).index_copy(1, P.rel_ids_t, v)
        return U, V

    def _head_layers(self, batch: SampledBatch, h: Dict[str, torch.Tensor], hbuf=None, last_premasked=False, hdrop=None):
        """The layers with gat_num_head = H > 1: per relation exactly GATConv((-1,-1), cl / H, heads=H, concat=True), re-associated
        as the single-head route is -- the aggregate gathers the layer input once per edge for all heads (ops.gat_aggregate(heads=H):
        Z[h] = sum_j alpha^h_ij x_j, full width per head), and column c of the output takes head(c)'s aggregate:
            out_i[c] = sum_k Z[head(c)]_i[k] W_src^T[k, c] + bias[c].
        That column-block product runs on the layer-transform kernels with the heads as H x R stacked "relations" of column-masked
        weights W_r^T * mask_h (H times the transform's FLOPs: DESIGN.md section 8).  Unfused: no FC_output fold, no parameter
        riders; u^h, v^h and the summed bias come from element-wise framework ops."""
        for l in range(1, self.num_layers + 1):
            P: RelationPack = self.live_packs[l - 1]
            tys, blocks = self._dst_blocks(batch, l)
            U, V = self._head_vectors(P)
            H = self._join_layer_input(batch, l, h, hbuf)
            # (from layer 2 on, H is the previous layer's ReLU output and its backward is folded into this node's)
            Z, _, _ = ops.gat_aggregate(batch, l, H, U, V, self.negative_slope, self.temperature, relu_input=(l > 1), heads=self.heads)
            hbuf, nxt = self._next_blocks(batch, l, tys)
            site = self._layer_site(l, hdrop, last_premasked)
            outs = ops.layer_transform_heads(P, Z, blocks, self.head_mask, site.out_blocks('transform', nxt),
                                             premasked=site.premasked, relu=site.relu)
            # (a root Linear behind it is full width, as PyG's ``res`` is H * C wide)
            h, hbuf = self._finish_layer(site, h, tys, blocks, outs, nxt, hbuf)
        return h, []

    def _edge_weights(self, batch: SampledBatch, l: int, stat, e_edge):
        """The weight every edge's message carried, from what the aggregate saved: the softmax's alpha (kgw_edge_alpha) or, gated,
        sigmoid(e / T) element-wise from the stored logits."""
        if self.gat_sigmoid:
            return torch.sigmoid(e_edge[:int(batch.meta.n_edges[l - 1])] * (1.0 / self.temperature))
        return ops.edge_alpha(batch, l, stat, e_edge, self.temperature)

    def set_dropout_word(self, word: int):
        """The word of the NEXT steps' attention-dropout masks (``dropout_word(seed, epoch, batch)``): one fill of the resident
        tensor, no synchronisation."""
        self.drop_word.fill_(_signed64(word))

    def _dropout(self):
        """``dropout=`` of the training forward's aggregates: (p, word) in training mode with gat_dropout > 0, else None.
        A forward that drops does NOT fold FC_output into layer 1 (``fold_fc``): the fold moves the Linear's constant c out of the
        messages as c * sum_j alpha_ij = c, and with dropout that sum is sum_j m'_j alpha_ij, which no kernel writes down -- so
        the step runs the unfolded route (the one KGW_FOLD_FC=0 takes) and pays FC_output's 128 x 128 Linear over the sampled
        nodes.  Evaluation and the attention queries never drop and keep the fold."""
        return (self.gat_dropout, self.drop_word) if (self.training and self.gat_dropout > 0.0) else None

    def _hidden_dropout(self):
        """``hdrop=`` of the training forward's layers: (p, word) in training mode with gnn_dropout > 0, else None.  Unlike the
        attention dropout it leaves the softmax rows alone (they still sum to 1), so the FC_output fold stays."""
        return (self.gnn_dropout, self.drop_word) if (self.training and self.gnn_dropout > 0.0) else None

    def _drop_hidden(self, l: int, h: Dict[str, torch.Tensor], hdrop):
        """Hidden-state dropout on the per-type outputs ``h`` of layer l (the routes whose outputs are framework tensors: SAGE, the
        relation min / max): one launch over all types, nothing for the last layer or with ``hdrop`` None."""
        if hdrop is None or l >= self.num_layers or not h:
            return h
        names = list(h)
        outs = ops.hidden_dropout([h[n] for n in names], [self.schema.type_id[n] for n in names], l, hdrop[0], hdrop[1])
        return dict(zip(names, outs))

    def _norm_site(self, l: int):
        """(weight, bias) [n_node_types, 128] of the normalisation after layer l, or None: a model without ``gnn_norm``, or the
        last layer.  In every mode: the norm is part of the function the model computes, not of its training."""
        return (self.norm_weight[l - 1], self.norm_bias[l - 1]) if self.gnn_norm is not None and l < self.num_layers else None

    def _root_site(self, l: int):
        """The packed root weights [n_node_types, 128, 128] of layer l, or None for a model without ``gnn_root_weight``.  In every
        mode: the root term is part of the function the model computes."""
        return self.root_weight[l - 1] if self.gnn_root_weight else None

    def _root_inputs(self, h: Dict[str, torch.Tensor], tys, rows):
        """The destination rows' own layer input: the leading ``rows`` rows of each type's state (the sampler's layout)."""
        xs = []
        for t, n in zip(tys, rows):
            name = self.schema.node_types[t]
            if name not in h or h[name].shape[0] < n:
                raise RuntimeError(f'root weight: node type {name!r} has {n} destination rows but no layer input of its own for them')
            xs.append(h[name] if h[name].shape[0] == n else h[name][:n])
        return xs

    def _add_root(self, l: int, h: Dict[str, torch.Tensor], pre: Dict[str, torch.Tensor]):
        """``pre`` + W_root x on per-type PRE-ACTIVATIONS that are framework tensors (the relation min / max, the all-relations
        routes), ahead of ``_activate``: one launch, no ReLU in it, and x an ordinary autograd tensor (not premasked)."""
        root = self._root_site(l)
        if root is None or not pre:
            return pre
        names = list(pre)
        tys = [self.schema.type_id[n] for n in names]
        ys = [pre[n] for n in names]
        outs = ops.root_linear(ys, tys, self._root_inputs(h, tys, [y.shape[0] for y in ys]), root, relu=False)
        return dict(zip(names, outs))

    def _activate(self, l: int, pre: Dict[str, torch.Tensor], relu: bool = True):
        """The activation of layer l on per-type PRE-ACTIVATIONS that are framework tensors (SAGE, the relation min / max, the
        all-relations routes): the ReLU of model.py:75, or at a norm site relu(LN(y)) for all types in one launch, whose backward
        masks by the saved output.  ``relu=False`` (the export: utils.py:460 applies no ReLU) leaves the plain state, or LN(y) =
        relu(LN(y)) - relu(-LN(y)) exactly: the kernel twice, the second time with the negated parameters."""
        site = self._norm_site(l)
        if site is None or not pre:
            return {n: torch.relu(y) for n, y in pre.items()} if relu else pre
        names = list(pre)
        ys, tys = [pre[n] for n in names], [self.schema.type_id[n] for n in names]
        outs = ops.layer_norm_relu(ys, tys, site[0], site[1], self.hidden_logical)
        if not relu:
            neg = ops.layer_norm_relu(ys, tys, -site[0].detach(), -site[1].detach(), self.hidden_logical)
            outs = [a - b for a, b in zip(outs, neg)]
        return dict(zip(names, outs))

    def _next_blocks(self, batch: SampledBatch, l: int, tys):
        """(``_layer_input(batch, l + 1)``'s matrix, its RowBlock or None for each type of ``tys``); (None, Nones) after the last layer."""
        hbuf, nxt = self._layer_input(batch, l + 1) if l < self.num_layers else (None, {})
        return hbuf, [nxt.get(self.schema.node_types[t]) for t in tys]

    def _layer_site(self, l: int, hdrop=None, last_premasked=False) -> LayerSite:
        """``hdrop``: see ``_hidden_dropout``; ``last_premasked``: the consumer of the LAST layer's output masks its gradient by
        (out > 0) itself (the fused read-out + loss node), as the next layer's aggregate does for every other layer."""
        last = l == self.num_layers
        root, norm = self._root_site(l), self._norm_site(l)
        drop = None if (hdrop is None or last) else (hdrop[0], hdrop[1])
        writer = 'drop' if drop is not None else 'norm' if norm is not None else 'root' if root is not None else 'transform'
        consumer_masks = (not last) or bool(last_premasked)
        return LayerSite(layer=l, root=root, norm=norm, drop=drop, writer=writer,
                         premasked=consumer_masks or root is not None, relu=norm is None and root is None,
                         root_premasked=consumer_masks, root_relu=norm is None, x_premasked=l > 1, norm_premasked=True)

    def _finish_layer(self, site: LayerSite, h: Dict[str, torch.Tensor], tys, blocks, outs, nxt, hbuf):
        """The stages of ``site`` on the transform's per-type outputs ``outs``: the 1 / R of 'mean', the root term (x from the layer's
        input ``h``), the norm, the dropout.  ``nxt`` / ``hbuf``: see ``_next_blocks``.  Returns (the new h, the hbuf to carry)."""
        if self.aggr == 'mean':
            # mean over the relations of a destination type = the sum scaled by 1/R; relu(s/R) = relu(s)/R, and the
            # positive scale commutes with the folded ReLU masks.  At a norm site the scale goes in BEFORE the norm: LN(y / R);
            # the root term is added to the scaled relation part
            hbuf = site.hbuf_after_mean(hbuf)
            outs = [o * (1.0 / (hi - lo)) for o, (lo, hi, _, _) in zip(outs, blocks)]
        if site.root is not None:
            outs = ops.root_linear(outs, tys, self._root_inputs(h, tys, [b[3] for b in blocks]), site.root, site.out_blocks('root', nxt),
                                   premasked=site.root_premasked, relu=site.root_relu, x_premasked=site.x_premasked)
        if site.norm is not None:
            outs = ops.layer_norm_relu(outs, tys, site.norm[0], site.norm[1], self.hidden_logical, site.out_blocks('norm', nxt),
                                       premasked=site.norm_premasked)
        if site.drop is not None:
            outs = ops.hidden_dropout(outs, tys, site.layer, site.drop[0], site.drop[1], site.out_blocks('drop', nxt))
        return {self.schema.node_types[t]: o for t, o in zip(tys, outs)}, hbuf

    def _fused_layers(self, batch: SampledBatch, h: Dict[str, torch.Tensor], want_attention=False, hbuf=None,
                      last_premasked=False, folded=False, prep=None, dropout=None, hdrop=None):
        """``folded``: h holds the feature MLPs' hidden state h2 (``_embed_all(fold=True)``), not their output: layer 1 runs
        with FC_output folded into its relation parameters (ops.fold_fc_output_hip).  ``prep``: per layer, what
        ``_layer_params`` returns, computed ahead by the caller.  ``dropout``: see ``_dropout``, ``hdrop``: see ``_hidden_dropout``
        (only ``forward`` and ``forward_loss`` pass them: the attention queries never drop)."""
        if self.backbone == 'SAGE':
            if want_attention:
                raise NotImplementedError('attention weights exist for the GAT backbone only (kgwas/model.py:65-72)')
            return self._sage_layers(batch, h, hbuf, hdrop)
        if self.heads > 1:
            if want_attention:
                raise NotImplementedError('gat_num_head > 1: the attention queries are single-head (kgw_edge_alpha)')
            return self._head_layers(batch, h, hbuf, last_premasked, hdrop)
        sc, C = self.schema, self.hidden
        attn = []
        if prep is None and self.num_layers > 1 and _RELVEC_ALL:
            prep = self._all_layer_params(batch, folded)
        for l in range(1, self.num_layers + 1):
            P: RelationPack = self.live_packs[l - 1]
            tys, blocks, zws, U, V, bsum, Wv, kap, Wp, gam, term = prep[l - 1] if prep is not None else self._layer_params(batch, l, folded)
            H = self._join_layer_input(batch, l, h, hbuf)
            # (from layer 2 on, H is the previous layer's ReLU output: with the fused transform its backward is folded
            # into this node's)
            fused = self.aggr in ('sum', 'mean')
            Z, stat, e_edge = ops.gat_aggregate(batch, l, H, U, V, self.negative_slope, self.temperature,
                                                relu_input=((l > 1 or folded) and fused), zbuf=zws, logit_bias=kap,
                                                dropout=dropout, sigmoid_gate=self.gat_sigmoid, edge_term=term)
            if want_attention:
                attn.append(self._edge_weights(batch, l, stat, e_edge))
            if not fused:
                # 'min' / 'max' over relations: per-relation outputs (lin_src + bias, conv.py:138-190) as one batched
                # product per destination type, then the reduction over the relation axis and the ReLU (model.py:74-75)
                hbuf = None
                outs = []
                for (lo, hi, z0, rows) in blocks:
                    R = hi - lo
                    zr = Z[z0:z0 + rows * R].view(rows, R, C).transpose(0, 1)
                    o = self._relation_products(zr, Wv, P.bias, lo, hi, 'gat min/max per-relation outputs')
                    outs.append(self._combine_relations(o))
                pre = self._add_root(l, h, {sc.node_types[t]: o for t, o in zip(tys, outs)})
                h = self._drop_hidden(l, self._activate(l, pre), hdrop)
                continue
            # per-relation linear maps + bias + relation sum + ReLU: one GEMM per destination type, one autograd node
            hbuf, nxt = self._next_blocks(batch, l, tys)
            site = self._layer_site(l, hdrop, last_premasked)
            outs = ops.layer_transform(P, Z, blocks, site.out_blocks('transform', nxt), premasked=site.premasked, bias_sum=bsum,
                                       weight=Wp if Wp is not None else Wv, gamma=gam, stat=stat if gam is not None else None,
                                       relu=site.relu)
            h, hbuf = self._finish_layer(site, h, tys, blocks, outs, nxt, hbuf)
        return h, attn

    def forward(self, x_dict, edge_index_dict, batch_size, genotype=None, return_h=False,
                return_attention_weights=False, edge_attr_dict=None):
        """``edge_attr_dict`` (a model with ``gat_edge_dim``, plain COO inputs): {edge type: [E] or [E, D]} aligned with the columns
        of ``edge_index_dict``; every attributed relation needs its entry.  The dicts of a sampled batch bring their own
        (``batch.edge_attr_dict``)."""
        if return_attention_weights and not return_h:           # model.py:65-72,80-81 (mean attention per layer)
            if self.heads > 1:
                raise NotImplementedError('gat_num_head > 1: forward(return_attention_weights=True) is single-head')
            if edge_attr_dict is None and self.edge_dim is not None and getattr(edge_index_dict, 'kgw_batch', None) is not None:
                edge_attr_dict = edge_index_dict.kgw_batch.edge_attr_dict
            return self._forward_with_attention(x_dict, edge_index_dict, batch_size, edge_attr_dict)
        batch: Optional[SampledBatch] = getattr(x_dict, 'kgw_batch', None) or getattr(edge_index_dict, 'kgw_batch', None)
        if batch is None:
            batch = self._block_from_coo(x_dict, edge_index_dict, edge_attr_dict)
        hbuf, blocks = self._layer_input(batch, 1)
        drop = self._dropout()
        fold = self.fold_fc and drop is None                    # (see _dropout: a step that drops runs layer 1 unfolded)
        h = self._embed_all(batch, x_dict, blocks, fold=fold)
        h, attn = self._fused_layers(batch, h, hbuf=hbuf, folded=fold, dropout=drop, hdrop=self._hidden_dropout())
        snp = h['SNP']
        out = self._readout(snp[:batch_size])
        if return_h:                                            # model.py:78-79
            return self.ReLU(out), snp[:batch_size, :self.hidden_logical]
        if self.no_relu:                                        # model.py:83-84
            return out
        return self.ReLU(out)                                   # model.py:86

    def _readout(self, h):
        """self.lin(h) (kgwas/model.py:50,83-86).  For the reference's out_channels == 1 (kgwas.py:52) the Linear(128 -> 1) is a
        row-wise dot product: elementwise multiply + row sum, not a library GEMV; out_channels = T > 1 (a shared trunk read out into
        T label columns) runs the read-out kernel of the multi-trait loss node without the loss."""
        if self.lin.out_features == 1:
            return (h * self.lin.weight.view(1, -1)).sum(1, keepdim=True) + self.lin.bias
        return ops.readout_linear(h, self.lin.weight, self.lin.bias)      # out_channels = T <= 32: kgw_readout_mt_pred

    @torch.no_grad()
    def hot_path_attention(self, batch: SampledBatch):
        """Per layer, the softmax attention weight of every edge the TRAINING path aggregates (live relations, hop-pruned
        destination rows; local edge order of ``batch``) -- what the fused kernels actually use, as opposed to the
        reference-shaped ``forward(return_attention_weights=True)`` which runs all relations over all rows."""
        if self.heads > 1:
            raise NotImplementedError('gat_num_head > 1: hot_path_attention is single-head (one alpha per edge)')
        hbuf, blocks = self._layer_input(batch, 1)
        h = self._embed_all(batch, batch.x_dict, blocks, fold=self.fold_fc)
        _, attn = self._fused_layers(batch, h, want_attention=True, hbuf=hbuf, folded=self.fold_fc)
        return attn

    def forward_loss(self, x_dict, edge_index_dict, batch_size, n_id, y_all, w_all, mlp_out=None, unit_grad=False,
                     edge_attr_dict=None, loss_rule=None):
        """The training step's forward (kgwas/kgwas.py:137-145): HeteroGNN.forward followed by
        mean(w_all[n_id] * (pred - y_all[n_id])**2), with the read-out Linear + ReLU (model.py:86) and the loss fused
        into one node.  Returns (loss [float64 scalar], pred [batch_size]) -- with ``out_channels = T > 1`` (a shared trunk read out
        into T label columns, ``y_all`` [N,T]) the mean runs over seeds and columns and pred is [batch_size, T]; ``w_all`` is then [N]
        (one weight per SNP) or [N,T] (per-trait weights, 0 = unobserved pair: ops.readout_weighted_mse).  ``mlp_out`` (list): receives the feature MLPs'
        output tensors -- the cut between the two halves of a backward pass whose first half's gradients are all-reduced
        while the second half runs (multi-GPU GraphTrainStep).  ``unit_grad``: the caller will backpropagate exactly
        ``loss.backward()`` (gradient 1): the read-out node then does its forward and backward in two launches.  ``loss_rule``
        (optim.parse_loss; None = the MSE above): a weighted Huber loss in the place of the square, in the same node
        (ops.readout_weighted_mse)."""
        batch: Optional[SampledBatch] = getattr(x_dict, 'kgw_batch', None) or getattr(edge_index_dict, 'kgw_batch', None)
        if batch is None:
            batch = self._block_from_coo(x_dict, edge_index_dict, edge_attr_dict)
        if not 1 <= self.lin.out_features <= 32:
            raise NotImplementedError('the fused read-out + loss takes out_channels from 1 (kgwas/kgwas.py:52) to 32')
        hbuf, blocks = self._layer_input(batch, 1)
        gat = self.backbone == 'GAT' and self.aggr in ('sum', 'mean')
        prep = None
        # what depends on the parameters only -- the relation vectors of all layers, the FC_output fold -- is prepared FIRST and
        # handed to the first gene Linear's kgw_gemm3 launch as rider blocks (ops.ParamRiders); whatever no launch took is
        # launched the ordinary way when the scope closes, before the layers read it
        drop = self._dropout()
        fold = self.fold_fc and drop is None                    # (see _dropout: a step that drops runs layer 1 unfolded)
        riders = ops.ParamRiders() if (ops._G3_RIDERS and self.backbone == 'GAT' and self.num_layers > 1 and _RELVEC_ALL and
                                       self.heads == 1) else None
        with ops.param_riders_scope(riders):
            if riders is not None:
                prep = self._all_layer_params(batch, fold)
            h = self._embed_all(batch, x_dict, blocks, fold=fold)
        self.last_riders_taken = riders.taken if riders is not None else 0
        if mlp_out is not None:
            mlp_out.extend(h.values())
        h, _ = self._fused_layers(batch, h, hbuf=hbuf, last_premasked=gat, folded=fold, prep=prep, dropout=drop,
                                  hdrop=self._hidden_dropout())
        return ops.readout_weighted_mse(h['SNP'], self.lin.weight, self.lin.bias, n_id, y_all, w_all, batch_size,
                                        relu=not self.no_relu, h_is_relu=gat, unit_grad=unit_grad, loss_rule=loss_rule)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _forward_all_relations(self, batch: SampledBatch, raw: bool):
        """Both layers over EVERY relation and every row of a full-graph block (no structural pruning), the way the
        reference runs a batch (kgwas/model.py:64-75): returns (final x_dict, [per layer: per-edge attention of the whole
        block, local edge order]).  ``raw``: the export's variant (kgwas/utils.py:446-461) -- raw leaky_relu logits as
        message weights (conv.py:221-228) and no ReLU between the layers (utils.py:460).  A gated model (``gat_sigmoid``) weights
        by its gates there too and returns them: conv.py:219-220 takes the sigmoid branch whatever return_raw_attention_weights says."""
        sc, m, C = self.schema, batch.meta, self.hidden
        dev = self.lin.weight.device
        h = self._embed_all(batch, batch.x_dict)
        per_layer = []
        for l in range(1, self.num_layers + 1):
            U = torch.zeros(sc.NR, C, device=dev)
            V = torch.zeros(sc.NR, C, device=dev)
            for pack in (self.live_packs[l - 1], self.dead_packs[l - 1]):
                if len(pack.rel_ids):
                    u, v = ops.rel_vectors(pack)           # rows of the pack's relations, zeros elsewhere
                    U += u; V += v
            H = torch.cat(self._layer_parts(batch, l, h)[0], 0)       # (no preallocated layer input on this route)
            gate = self.gat_sigmoid
            Z, stat, e_edge = ops.gat_aggregate(batch, l, H, U, V, self.negative_slope, self.temperature, raw_weights=raw and not gate,
                                                sigmoid_gate=gate,
                                                edge_term=self._edge_term(batch, l, (self.live_packs[l - 1], self.dead_packs[l - 1])))
            per_layer.append(e_edge if (raw and not gate) else self._edge_weights(batch, l, stat, e_edge))
            h_next = {}
            for t, name in enumerate(sc.node_types):
                n, R = int(m.lay_rows[l - 1][t]), int(sc.R_dst[t])
                if n == 0 or R == 0:
                    continue
                z0 = int(m.z_base[l - 1][t])
                x = Z[z0:z0 + n * R].view(n, R * C)
                ws, bs = [], 0
                for r in sc.rels_by_dst[t]:                # slot order of the Z columns
                    which, i = self._slot[l - 1][r]
                    pack = self.live_packs[l - 1] if which == 'live' else self.dead_packs[l - 1]
                    ws.append(pack.w_src_t[i])
                    bs = bs + pack.bias[i]
                h_next[name] = ops.linear(x, torch.cat(ws, 0), bs, w_kn=True)
            h = self._activate(l, self._add_root(l, h, h_next), relu=not raw)        # model.py:75 / no ReLU at utils.py:460

        return h, per_layer

    @torch.no_grad()
    def raw_attention_full_graph(self, graph: HeteroGraph, device=None):
        """Per layer, per relation: (edge_index [2,E] global ids, raw attention [E]) over the WHOLE graph, the way
        the reference's export computes them (kgwas/utils.py:437-461): every relation of every layer takes part,
        the attention is leaky_relu(alpha_j + alpha_i) without softmax (conv.py:217-223 under
        return_raw_attention_weights), the layer output fed to the next layer is the sum of messages weighted by
        those raw values (conv.py:227-228) plus bias, summed over relations, and -- unlike HeteroGNN.forward -- NO
        ReLU is applied between the layers (utils.py:460)."""
        from .sampler import BatchBuffers, DeviceGraph, finish_sample, sample_into
        if self.heads > 1:
            raise NotImplementedError('gat_num_head > 1: the attention export (raw_attention_full_graph / '
                                      'get_disease_critical_network) is single-head')
        if self.backbone != 'GAT':
            raise NotImplementedError('attention weights exist for the GAT backbone only (kgwas/utils.py:437-461)')
        if self.aggr != 'sum':
            raise NotImplementedError("the attention export is built for gnn_aggr='sum' (the reference default)")
        dev = torch.device(device) if device is not None else self.lin.weight.device
        sc = self.schema
        dg = DeviceGraph.get(graph, self.num_layers, dev, full_graph=True).with_all_relations_live()
        buf = BatchBuffers(dg)
        sample_into(dg, buf, None, 0)
        batch = finish_sample(dg, buf, sc.node_types[0], dg.n_nodes[0])
        m = batch.meta
        _, per_layer = self._forward_all_relations(batch, raw=True)
        ei = batch.edge_index_dict                         # full graph: local ids are the global ids
        seg_ptr = buf.seg_ptr
        layers = []
        for e_edge in per_layer:
            att = OrderedDict()
            for r, et in enumerate(self.edge_types):
                a, b = int(m.seg_off[0][r]), int(m.seg_off[0][r + 1])
                e0, e1 = (int(seg_ptr[a]), int(seg_ptr[b])) if b > a else (0, 0)
                att[et] = (ei[et], e_edge[e0:e1])
            layers.append(att)
        return layers

    def _coo_edge_attrs(self, g: HeteroGraph, edge_attr_dict):
        """``edge_attr_dict`` onto the relations of a graph built from plain COO inputs (a model with ``gat_edge_dim``)."""
        if self.edge_dim is None:
            return
        for r in self.attr_rels:
            et = self.edge_types[r]
            a = None if edge_attr_dict is None else edge_attr_dict.get(et)
            if a is None:
                raise ValueError(f'the model has edge attributes on {et}: edge_attr_dict needs an entry for it')
            g[et].edge_attr = a

    @torch.no_grad()
    def _forward_with_attention(self, x_dict, edge_index_dict, batch_size, edge_attr_dict=None):
        """forward(return_attention_weights=True) (kgwas/model.py:65-72,80-81): the reference runs EVERY edge type over
        every edge of the batch in both layers and returns the mean attention of all of them per layer, so this path
        does too -- the batch's subgraph as a full block with all relations live, no hop pruning (inference only)."""
        from .sampler import BatchBuffers, DeviceGraph, finish_sample, sample_into
        if self.backbone != 'GAT':
            raise NotImplementedError('attention weights exist for the GAT backbone only (kgwas/model.py:65-72)')
        if self.aggr != 'sum':
            raise NotImplementedError("attention weights are built for gnn_aggr='sum' (the reference default)")
        dev = next(iter(x_dict.values())).device if len(x_dict) else self.lin.weight.device
        g = HeteroGraph()
        for t in self.node_types:
            if t in x_dict:
                g[t].x = x_dict[t]
            else:
                g[t].num_nodes_ = 0
        for et in self.edge_types:
            ei = edge_index_dict.get(et)
            g[et].edge_index = ei if ei is not None else torch.zeros(2, 0, dtype=torch.long)
        self._coo_edge_attrs(g, edge_attr_dict)
        dg = DeviceGraph(g, self.num_layers, dev, full_graph=True).with_all_relations_live()
        buf = BatchBuffers(dg)
        sample_into(dg, buf, None, 0)
        sc = self.schema
        batch = finish_sample(dg, buf, sc.node_types[0], dg.n_nodes[0])
        h, per_layer = self._forward_all_relations(batch, raw=False)
        self.last_attention = per_layer
        out = self.ReLU(self._readout(h['SNP'][:batch_size]))
        return out, [a.mean() if a.numel() else a.sum() for a in per_layer]

    # ------------------------------------------------------------------------------------------
    def _block_from_coo(self, x_dict, edge_index_dict, edge_attr_dict=None) -> SampledBatch:
        """Plain (x_dict, edge_index_dict) inputs: every row of every type is computed in every layer,
        exactly like the reference on a PyG batch / the full graph (kgwas/utils.py:446-461)."""
        dev = next(iter(x_dict.values())).device
        g = HeteroGraph()
        for t in self.node_types:
            g[t].num_nodes_ = int(x_dict[t].shape[0]) if t in x_dict else 0
        for et in self.edge_types:
            ei = edge_index_dict.get(et)
            g[et].edge_index = ei if ei is not None else torch.zeros(2, 0, dtype=torch.long)
        self._coo_edge_attrs(g, edge_attr_dict)
        return sample_full_graph(g, self.num_layers, dev)

    # --- reference-named parameters (checkpoints, tests) ------------------------------------------
    def _rel_items(self, grad: bool = False):
        """Yield (reference key, tensor | None | 'lazy') for every relation tensor of every layer."""
        for l in range(self.num_layers):
            for r, et in enumerate(self.edge_types):
                which, i = self._slot[l][r]
                pack = self.live_packs[l] if which == 'live' else self.dead_packs[l]
                for f in self._fields_of(r):
                    yield f'convs.{l}.convs.{edge_key(et)}.{f}', pack.get(i, f, grad)

    def _fields_of(self, r: int):
        """Reference names of relation r's tensors: an attributed relation (``gat_edge_dim``) also has lin_edge.weight / att_edge."""
        return self.rel_fields + EDGE_FIELDS if r in self.attr_rels else self.rel_fields

    def _dense_items(self, grad: bool = False, keep_vars: bool = False):
        """(reference key, tensor at the model's own width) of the feature MLPs and the read-out."""
        cl = self.hidden_logical
        for prefix, mod in (('snp_feat_mlp', self.snp_feat_mlp), ('go_feat_mlp', self.go_feat_mlp),
                            ('gene_feat_mlp', self.gene_feat_mlp), ('lin', self.lin)):
            for n, p in mod.named_parameters():
                t = p.grad if grad else (p if keep_vars else p.detach())
                if t is not None and cl != self.hidden:
                    if prefix == 'lin':
                        t = t[:, :cl] if n == 'weight' else t
                    elif n == 'FC_hidden.weight':
                        t = t[:cl]
                    elif n.endswith('weight'):
                        t = t[:cl, :cl]
                    else:
                        t = t[:cl]
                yield f'{prefix}.{n}', t

    def _norm_items(self, grad: bool = False, keep_vars: bool = False):
        """(``norms.<l>.<node type>.weight`` | ``.bias``, the type's row of the site's packed tensor at the model's own width) for the
        norm after ``convs.<l>`` -- nothing for a model without ``gnn_norm``.  ``grad``: rows of the packed gradient; a type without
        rows in the batch has a ZERO row there (ops.layer_norm_relu), not None."""
        cl = self.hidden_logical
        for l, (w, b) in enumerate(zip(self.norm_weight, self.norm_bias)):
            for t in self.norm_types:
                for f, p in (('weight', w), ('bias', b)):
                    v = p.grad if grad else (p if keep_vars else p.detach())
                    yield f'norms.{l}.{self.node_types[t]}.{f}', None if v is None else v[t, :cl]

    def _root_items(self, grad: bool = False, keep_vars: bool = False):
        """(``roots.<l>.<node type>.weight``, the type's slice of layer l + 1's packed root weights at the model's own width) --
        nothing for a model without ``gnn_root_weight``.  ``grad``: slices of the packed gradient; a type without rows in the batch
        has a ZERO slice there (ops.root_linear), not None."""
        cl = self.hidden_logical
        for l, w in enumerate(self.root_weight):
            for t in self.root_types:
                v = w.grad if grad else (w if keep_vars else w.detach())
                yield f'roots.{l}.{self.node_types[t]}.weight', None if v is None else v[t, :cl, :cl]

    def named_reference_tensors(self, grad: bool = False) -> "OrderedDict[str, Optional[torch.Tensor]]":
        """Parameters (or their gradients) under the reference's names.  Lazy lin_dst of same-type relations
        is omitted; structurally dead relations have gradient None."""
        out = OrderedDict()
        for k, v in self._rel_items(grad):
            if isinstance(v, str):
                continue
            out[k] = v
        for k, t in self._dense_items(grad):
            out[k] = t
        for k, t in self._norm_items(grad):
            out[k] = t
        for k, t in self._root_items(grad):
            out[k] = t
        return out

    def state_dict(self, *args, destination=None, prefix='', keep_vars=False):
        out = OrderedDict() if destination is None else destination
        for k, v in self._rel_items():
            out[prefix + k] = torch.nn.parameter.UninitializedParameter() if isinstance(v, str) else v.clone()
        for k, t in self._dense_items(keep_vars=keep_vars):
            out[prefix + k] = t
        for k, t in self._norm_items(keep_vars=keep_vars):
            out[prefix + k] = t.clone()
        for k, t in self._root_items(keep_vars=keep_vars):
            out[prefix + k] = t.clone()
        return out

    def load_state_dict(self, state_dict, strict=True, **kw):
        want = {}
        for l in range(self.num_layers):
            for r, et in enumerate(self.edge_types):
                for f in self._fields_of(r):
                    want[f'convs.{l}.convs.{edge_key(et)}.{f}'] = (l, r, f)
        rest = OrderedDict()
        seen = set()
        for k, v in state_dict.items():
            k2 = k.replace('<', '').replace('>', '').replace('___', '__')     # PyG >= 2.4 key style
            if k2 in want:
                l, r, f = want[k2]
                seen.add(k2)
                if isinstance(v, torch.nn.parameter.UninitializedParameter):
                    continue                  # never-materialised lazy lin_dst of same-type relations
                which, i = self._slot[l][r]
                (self.live_packs[l] if which == 'live' else self.dead_packs[l]).set(i, f, v)
            else:
                rest[k2] = v
        missing = [k for k, (l, r, f) in want.items() if k not in seen and
                   not (f == 'lin_dst.weight' and self.edge_types[r][0] == self.edge_types[r][2])]
        unexpected = []
        known = ('snp_feat_mlp.', 'go_feat_mlp.', 'gene_feat_mlp.', 'lin.', 'norms.', 'roots.')
        with torch.no_grad():
            for k, dst in list(self._dense_items()) + list(self._norm_items()) + list(self._root_items()):     # (views of the padded storage at the model's own width)
                if k in rest:
                    if tuple(rest[k].shape) != tuple(dst.shape):
                        raise RuntimeError(f'load_state_dict: {k} has shape {tuple(rest[k].shape)}, the model expects {tuple(dst.shape)}')
                    dst.copy_(rest[k])
                else:
                    missing.append(k)
        have = {k for k, _ in self._dense_items()} | {k for k, _ in self._norm_items()} | {k for k, _ in self._root_items()}
        unexpected += [k for k in rest if k.startswith(known) and k not in have]
        unexpected += [k for k in rest if not k.startswith(known)]
        if strict and (missing or unexpected):
            raise RuntimeError(f'load_state_dict: missing {missing[:5]} unexpected {unexpected[:5]}')
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)
