"""The SNP-sharded mode with every rank in ONE process on one device (tests/test_gpu_shard_kernels.py): a rank is a rank-local
graph (shard.shard_graph), a DeviceGraph, a BatchBuffers and the relation mask of its ShardExchange; the collectives of
kgwas_amd/shard.py are a MIN, a concatenation and a SUM of tensors that all live on the same GPU, so the ranks run one after the
other.  No torch.distributed process group, no spawned process, no environment variable.

  sample_ranks   = shard.sample_sharded with the all-reduce(MIN) of the frontier flags replaced by torch.minimum over the ranks'
                   g2l tables (ShardExchange.rep_runs: the replicated node types' regions);
  LayerExchange  = the object ops.gat_aggregate reads from ``batch.exchange`` (mask, staged, forward, backward).  The ranks run
                   one after the other, so the forward is done twice: pass 1 only packs (kgw_softmax_pack) and keeps every
                   rank's record, pass 2 packs again (must be the same bits), concatenates the records in rank order and merges
                   (kgw_softmax_merge).  The backward gathers the exchanged dZ rows (kgw_gather_rows), replaces them by the sum
                   over the ranks' rows and puts them back (kgw_scatter_rows), as ShardExchange.backward does around its
                   all-reduce."""
import ctypes as C

import numpy as np
import torch

W = 128                 # KGW_C
PS = 132                # floats per packed record: [0] = m, [1] = s, [2..3] = 0, [4..131] = acc


def _vp(t):
    return C.c_void_p(t.data_ptr())


class Rank:
    pass


def make_ranks(data, seeds, P, layers=2, sharded_type='SNP'):
    """P rank-local graphs of ``data`` with their device graphs, buffers and local seeds (the batch's seeds a rank owns, batch
    order).  Every rank must own a seed: a rank without one expands a stand-in node, which legitimately enlarges the frontier."""
    from kgwas_amd.sampler import BatchBuffers, DeviceGraph
    from kgwas_amd.shard import ShardExchange, shard_graph
    seeds = np.asarray(seeds, dtype=np.int64)
    ranks = []
    for p in range(P):
        rk = Rank()
        rk.p, rk.P = p, P
        rk.local, rk.lo, rk.hi = shard_graph(data, p, P, sharded_type)
        mine = seeds[(seeds >= rk.lo) & (seeds < rk.hi)] - rk.lo
        assert len(mine) > 0, f'rank {p} of {P} owns no seed of the batch: the comparison with the unsharded batch is void'
        rk.dg = DeviceGraph(rk.local, layers, 'cuda:0')
        rk.buf = BatchBuffers(rk.dg)
        rk.seeds = torch.from_numpy(np.ascontiguousarray(mine)).cuda()
        rk.seed_type = rk.dg.schema.type_id[sharded_type]
        rk.xchg = ShardExchange(rk.dg, sharded_type)      # (no process group: used for mask / seg_rows / rep_runs only)
        rk.batch = None
        ranks.append(rk)
    return ranks


def sample_parts(dg, buf, seeds, seed_type, begin, end):
    from kgwas_amd import _lib
    st = torch.cuda.current_stream()
    _lib.check(_lib.lib().kgw_sample_batch_parts(C.byref(dg.kg), C.byref(buf.c), _vp(seeds), int(seeds.numel()), seed_type, 0,
                                                 begin, end, C.c_void_p(st.cuda_stream)), 'kgw_sample_batch_parts')


def sample_ranks(ranks, no_merge=()):
    """shard.sample_sharded on every rank with the frontier all-reduce replaced by torch.minimum across the ranks' tables.
    ``no_merge``: ranks that do NOT receive the merged flags (a deliberately broken exchange, for the tests of the tests)."""
    from kgwas_amd.sampler import SampledBatch
    n_hops = ranks[0].dg.n_hops
    begin = 0
    for h in range(n_hops - 1):
        for rk in ranks:
            sample_parts(rk.dg, rk.buf, rk.seeds, rk.seed_type, begin, 2 * h)
        for i in range(len(ranks[0].xchg.rep_runs)):
            views = [rk.buf.g2l[rk.xchg.rep_runs[i][0]:rk.xchg.rep_runs[i][1]] for rk in ranks]
            mn = views[0].clone()
            for v in views[1:]:
                mn = torch.minimum(mn, v)
            for rk, v in zip(ranks, views):
                if rk.p not in no_merge:
                    v.copy_(mn)
        begin = 2 * h + 1
    for rk in ranks:
        sample_parts(rk.dg, rk.buf, rk.seeds, rk.seed_type, begin, 2 * n_hops)
    torch.cuda.synchronize()
    for rk in ranks:
        meta = rk.buf.read_meta()
        assert not meta.error, meta.error
        rk.batch = SampledBatch(rk.dg, rk.buf, meta, 'SNP', int(rk.seeds.numel()))
    return ranks


class LayerRun:
    """State shared by the ranks' LayerExchange objects over the two forward passes and the backward of one layer."""

    def __init__(self, n_ranks):
        self.P = n_ranks
        self.pass_ = 1
        self.records = [None] * n_ranks          # pass 1: every rank's packed partial states
        self.order = {}                          # rank -> order in which it concatenates the records (default: rank order)
        self.g_rows = [None] * n_ranks           # the exchanged rows of every rank's upstream gradient
        self.g_sum = None                        # ... summed over the ranks


class LayerExchange:
    staged = False

    def __init__(self, rk, run):
        self.rk, self.run = rk, run
        self.mask = rk.xchg.mask

    def forward(self, batch, layer, Z, stat):
        from kgwas_amd import _lib
        L, run, p = _lib.lib(), self.run, self.rk.p
        seg = self.rk.xchg.seg_rows(batch, layer)
        assert seg is not None
        n = int(seg.numel())
        mine = torch.full((n * PS,), float('nan'), device=Z.device)
        _lib.check(L.kgw_softmax_pack(_vp(Z), _vp(stat), _vp(seg), n, _vp(mine), _lib.stream_ptr()), 'kgw_softmax_pack')
        if run.pass_ == 1:
            run.records[p] = mine
            return
        assert torch.equal(mine, run.records[p]), f'rank {p}: the second pack differs from the first (not deterministic)'
        allp = torch.cat([run.records[q] for q in run.order.get(p, range(run.P))])
        _lib.check(L.kgw_softmax_merge(_vp(allp), run.P, _vp(seg), n, _vp(Z), _vp(stat), _lib.stream_ptr()), 'kgw_softmax_merge')

    def gather(self, batch, layer, dZ):
        from kgwas_amd import _lib
        seg = self.rk.xchg.seg_rows(batch, layer)
        n = int(seg.numel())
        rows = torch.full((n, W), float('nan'), device=dZ.device)
        _lib.check(_lib.lib().kgw_gather_rows(_vp(dZ), _vp(seg), n, W, _vp(rows), _lib.stream_ptr()), 'kgw_gather_rows')
        return rows

    def backward(self, batch, layer, dZ):
        from kgwas_amd import _lib
        run, p = self.run, self.rk.p
        seg = self.rk.xchg.seg_rows(batch, layer)
        rows = self.gather(batch, layer, dZ)
        assert torch.equal(rows, run.g_rows[p]), f'rank {p}: the exchanged dZ rows are not its upstream gradient'
        _lib.check(_lib.lib().kgw_scatter_rows(_vp(run.g_sum), _vp(seg), int(seg.numel()), W, _vp(dZ), _lib.stream_ptr()),
                   'kgw_scatter_rows')
        return dZ


def run_layer(batch, layer, H, U, V, kap, G, slope=0.2, temp=1.0, relu_input=False, backward=True):
    """One gat_aggregate call (with whatever ``batch.exchange`` holds) and, optionally, its backward under G."""
    from kgwas_amd import ops
    m, sc = batch.meta, batch.dg.schema
    z_rows = int(m.z_base[layer - 1][sc.NT])
    n_edges = int(m.n_edges[layer - 1])
    Hd, Ud, Vd = (t.cuda().requires_grad_(True) for t in (H, U, V))
    kd = kap.cuda().requires_grad_(True) if kap is not None else None
    Z, stat, e = ops.gat_aggregate(batch, layer, Hd, Ud, Vd, neg_slope=slope, temperature=temp, relu_input=relu_input,
                                   logit_bias=kd)
    out = dict(Z=Z.detach().cpu(), stat=stat[:z_rows].cpu(), e=e[:n_edges].cpu())
    if not backward:
        return out
    out['alpha'] = ops.edge_alpha(batch, layer, stat, e, temperature=temp).cpu()
    (Z * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    out.update(dH=Hd.grad.cpu(), dU=Ud.grad.cpu(), dV=Vd.grad.cpu(), dlb=kd.grad.cpu() if kd is not None else None)
    return out


def run_layer_on_ranks(ranks, layer, Hs, U, V, kap, Gs, slope=0.2, temp=1.0, relu_input=False, order=None):
    """The layer on every rank with the exchange done in process.  Returns (per-rank outputs as run_layer's, LayerRun)."""
    run = LayerRun(len(ranks))
    run.order = dict(order or {})
    ex = [LayerExchange(rk, run) for rk in ranks]
    try:
        for rk, x in zip(ranks, ex):
            rk.batch.exchange = x
        run.pass_ = 1
        for rk in ranks:
            run_layer(rk.batch, layer, Hs[rk.p], U, V, kap, None, slope, temp, relu_input, backward=False)
        assert all(r is not None for r in run.records)
        run.pass_ = 2
        for rk, x in zip(ranks, ex):                     # what the all-reduce(SUM) of the backward will deliver
            run.g_rows[rk.p] = x.gather(rk.batch, layer, Gs[rk.p].cuda().contiguous())
        run.g_sum = run.g_rows[0].clone()
        for r in run.g_rows[1:]:
            run.g_sum += r
        outs = [run_layer(rk.batch, layer, Hs[rk.p], U, V, kap, Gs[rk.p], slope, temp, relu_input) for rk in ranks]
    finally:
        for rk in ranks:
            rk.batch.exchange = None
    return outs, run
