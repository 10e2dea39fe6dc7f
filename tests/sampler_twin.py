"""The sampler's specification as plain numpy: every output of kgw_sample_batch (include/kgwas_hip.h), restated from
GraphSchema, build_csr and the header's prose -- host only, nothing here touches a GPU.  tests/test_gpu_sampler_exact.py compares
the HIP sampler with it array for array (np.array_equal); tests/test_sampler_twin.py checks the twin itself against the PyG
restatement (oracle/pyg_semantics.py, oracle/sampler_np.py) and the structural invariants below.

What a call writes (``sample_twin`` returns it as a dict):
  * nodes: per type the seeds in seed order, then each later hop's new nodes in ascending global id (``n_id``); ``g2l`` is the
    inverse over the KGW_TILE-padded node space, -1 everywhere else;
  * segments of hop h: relation-major, then the destination's local id within the hop; ``seg_ptr`` / ``seg_chptr`` are the
    running sums of ``seg_deg`` / ``seg_nch`` over ALL hops with one end sentinel; ``col_local`` = the CSR row of every segment, in
    CSR order, through g2l; ``chunks`` = every segment cut into pieces of KGW_CHUNK edges; ``multi`` = the segments of more than
    one chunk, per hop (an unordered list: compared as a sorted set of rows);
  * per layer l: the row-block layout (hop-pruned: layer l has the destination rows of hops <= hd = min(L - l, n_hops - 1) and
    the source rows of hops <= hd + 1; only for the types a live relation of the layer touches), and the src-major structure =
    the layer's live edges STABLY sorted by row key t_base[src type] + col_local * R_src + slot_src (np.argsort(kind='stable') is
    the specification of the order), with the Z row and relation of every entry, and the octet flags.
KgwBatchMeta.cur / pad_ and buffer contents past the counts are unspecified."""
from __future__ import annotations

import numpy as np

from kgwas_amd.graph import GraphSchema, build_csr

KGW_MAX_TYPES, KGW_MAX_RELS, KGW_MAX_LAYERS, KGW_CHUNK, KGW_TILE = 8, 64, 4, 128, 1024

META_FIELDS = ('hop_cnt', 'node_off', 'seg_off', 'seg_end', 'edge_end', 'chunk_end', 'multi_cnt', 'n_rows', 'z_base', 'n_src',
               'src_base', 't_base', 'lay_rows', 'lay_src', 'n_chunks', 'n_edges', 't_entries', 'error')


def meta_to_dict(m) -> dict:
    """The compared fields of a ctypes KgwBatchMeta as numpy arrays (``cur`` and ``pad_`` are unspecified)."""
    return {k: np.array(getattr(m, k), dtype=np.int64) for k in META_FIELDS}


class TwinGraph:
    """What is fixed per graph: schema, one dst-major CSR per relation (build_csr), the padded node space."""

    def __init__(self, data):
        self.schema = sc = GraphSchema(data.node_types, data.edge_types)
        self.n_nodes = [int(data[t].num_nodes) for t in sc.node_types]
        self.csr = []
        col_off, out_edges = 0, [0] * sc.NT
        self.col_off = []
        for r, et in enumerate(sc.edge_types):
            rp, col = build_csr(data[et].edge_index, self.n_nodes[sc.src_type[r]], self.n_nodes[sc.dst_type[r]])
            self.csr.append((rp, col.astype(np.int64)))
            self.col_off.append(col_off)
            col_off += len(col)
            out_edges[sc.src_type[r]] += len(col)
        self.node_base = np.zeros(sc.NT + 1, dtype=np.int64)
        for t, n in enumerate(self.n_nodes):
            self.node_base[t + 1] = self.node_base[t] + (n + KGW_TILE - 1) // KGW_TILE * KGW_TILE
        # KgwGraph.short_types: node types whose nodes average at most 4 out-edges
        self.short_mask = sum(1 << t for t in range(sc.NT) if out_edges[t] <= 4 * max(self.n_nodes[t], 1))
        # capacities as DeviceGraph sizes them (the static layout's bit-16 check and the multi slots need none of them here)
        self.trow_cap = int(sum(n * int(rs) for n, rs in zip(self.n_nodes, sc.R_src)))

    def rel_live(self, num_layers, all_live=False, out_type='SNP'):
        sc = self.schema
        live = np.zeros((num_layers, sc.NR), dtype=bool)
        if all_live:
            live[:] = True
        else:
            lr, _ = sc.live_relations(num_layers, out_type)
            for l in range(1, num_layers + 1):
                live[l - 1, lr[l]] = True
        return live


def _twin_graph(data) -> TwinGraph:
    extra = data._extra
    if '_sampler_twin' not in extra:
        extra['_sampler_twin'] = TwinGraph(data)
    return extra['_sampler_twin']


def _excl(a):
    out = np.zeros(len(a) + 1, dtype=np.int64)
    np.cumsum(a, out=out[1:])
    return out


def sample_twin(data, num_layers, seed_type, seeds, full_graph=False, all_live=False, caps=None, out_type='SNP') -> dict:
    """Every output of kgw_sample_batch for ``seeds`` (global ids of node type ``seed_type``: name or index) on ``data``.
    ``all_live``: the rel_live table of DeviceGraph.with_all_relations_live instead of GraphSchema.live_relations.
    ``caps``: a BatchCaps -- the static layout of DeviceGraph.with_static_caps (lay_* and the bases from the capacities)."""
    tg = _twin_graph(data)
    sc, L = tg.schema, int(num_layers)
    NT, NR = sc.NT, sc.NR
    n_hops = 1 if full_graph else L
    seed_t = sc.type_id[seed_type] if isinstance(seed_type, str) else int(seed_type)
    live = tg.rel_live(L, all_live, out_type)
    M = {k: np.zeros(s, dtype=np.int64) for k, s in (
        ('hop_cnt', (KGW_MAX_TYPES, KGW_MAX_LAYERS + 1)), ('node_off', (KGW_MAX_TYPES, KGW_MAX_LAYERS + 2)),
        ('seg_off', (KGW_MAX_LAYERS, KGW_MAX_RELS + 1)), ('seg_end', KGW_MAX_LAYERS), ('edge_end', KGW_MAX_LAYERS),
        ('chunk_end', KGW_MAX_LAYERS), ('multi_cnt', KGW_MAX_LAYERS), ('n_rows', (KGW_MAX_LAYERS, KGW_MAX_TYPES)),
        ('z_base', (KGW_MAX_LAYERS, KGW_MAX_TYPES + 1)), ('n_src', (KGW_MAX_LAYERS, KGW_MAX_TYPES)),
        ('src_base', (KGW_MAX_LAYERS, KGW_MAX_TYPES + 1)), ('t_base', (KGW_MAX_LAYERS, KGW_MAX_TYPES + 1)),
        ('lay_rows', (KGW_MAX_LAYERS, KGW_MAX_TYPES)), ('lay_src', (KGW_MAX_LAYERS, KGW_MAX_TYPES)),
        ('n_chunks', KGW_MAX_LAYERS), ('n_edges', KGW_MAX_LAYERS), ('t_entries', KGW_MAX_LAYERS), ('error', ()))}

    # ---- nodes and segments, hop by hop ------------------------------------------------------------------------------
    local = [np.full(n, -1, dtype=np.int64) for n in tg.n_nodes]
    if full_graph:
        nid = [[np.arange(n, dtype=np.int64)] for n in tg.n_nodes]
    else:
        nid = [[np.zeros(0, np.int64)] for _ in range(NT)]
        nid[seed_t] = [np.asarray(seeds, dtype=np.int64).reshape(-1)]
    for t in range(NT):
        local[t][nid[t][0]] = np.arange(len(nid[t][0]))
        M['hop_cnt'][t, 0] = M['node_off'][t, 1] = len(nid[t][0])
    seg_deg, seg_row, seg_rel, seg_g, seg_gpos, src_g, multi = [], [], [], [], [], [], []
    for h in range(n_hops):
        s = int(M['seg_end'][h - 1]) if h else 0
        reached = [[] for _ in range(NT)]
        for r in range(NR):
            d, st = int(sc.dst_type[r]), int(sc.src_type[r])
            M['seg_off'][h, r] = s
            g = nid[d][h]                                    # the destination type's nodes new at hop h, in local order
            s += len(g)
            rp, col = tg.csr[r]
            deg = rp[g + 1] - rp[g]
            seg_deg.append(deg)
            seg_row.append(M['node_off'][d, h] + np.arange(len(g)))
            seg_rel.append(np.full(len(g), r, dtype=np.int64))
            seg_gpos.append(tg.col_off[r] + rp[g])
            ex = _excl(deg)
            pos = np.arange(ex[-1]) - np.repeat(ex[:-1], deg) + np.repeat(rp[g], deg)     # the rows' entries, CSR order
            src_g.append((st, col[pos]))
            reached[st].append(col[pos])
        M['seg_off'][h, NR] = M['seg_end'][h] = s
        for t in range(NT):                                  # new at hop h + 1: not yet sampled, ascending global id
            got = np.unique(np.concatenate(reached[t])) if reached[t] else np.zeros(0, np.int64)
            new = got[local[t][got] < 0]
            local[t][new] = M['node_off'][t, h + 1] + np.arange(len(new))
            nid[t].append(new)
            M['hop_cnt'][t, h + 1] = len(new)
            M['node_off'][t, h + 2] = M['node_off'][t, h + 1] + len(new)
        deg_all = np.concatenate(seg_deg)
        M['edge_end'][h] = deg_all.sum()
        M['chunk_end'][h] = ((deg_all + KGW_CHUNK - 1) // KGW_CHUNK).sum()
    seg_deg = np.concatenate(seg_deg)
    seg_row, seg_rel, seg_gpos = np.concatenate(seg_row), np.concatenate(seg_rel), np.concatenate(seg_gpos)
    seg_nch = (seg_deg + KGW_CHUNK - 1) // KGW_CHUNK
    seg_ptr, seg_chptr = _excl(seg_deg), _excl(seg_nch)
    # (a source's local id is final once its hop is closed, and every source of hop h is known by the end of hop h)
    col_local = np.concatenate([local[st][g] for st, g in src_g]) if src_g else np.zeros(0, np.int64)

    # ---- chunks: every segment in pieces of KGW_CHUNK edges ---------------------------------------------------------------
    c_seg = np.repeat(np.arange(len(seg_deg)), seg_nch)
    c_idx = np.arange(len(c_seg)) - seg_chptr[c_seg]
    e0 = seg_ptr[c_seg] + KGW_CHUNK * c_idx
    gpos = seg_gpos[c_seg] + KGW_CHUNK * c_idx
    chunks = np.stack([e0, np.minimum(e0 + KGW_CHUNK, seg_ptr[c_seg + 1]), seg_row[c_seg], seg_rel[c_seg], seg_chptr[c_seg],
                       seg_nch[c_seg], (gpos & 0xFFFFFFFF).astype(np.uint32).astype(np.int32).astype(np.int64), gpos >> 32],
                      axis=1) if len(c_seg) else np.zeros((0, 8), np.int64)
    for h in range(n_hops):
        a, b = (int(M['seg_end'][h - 1]) if h else 0), int(M['seg_end'][h])
        big = a + np.nonzero(seg_nch[a:b] > 1)[0]
        M['multi_cnt'][h] = len(big)
        multi.append(sorted_rows(np.stack([seg_chptr[big], seg_nch[big], seg_row[big], seg_rel[big]], axis=1)))

    # ---- layer tables ---------------------------------------------------------------------------------------------------
    R_dst, R_src = sc.R_dst.astype(np.int64), sc.R_src.astype(np.int64)
    for l in range(1, L + 1):
        hd = min(L - l, n_hops - 1)
        zb = sb = tb = 0
        for t in range(NT):
            dst_live = bool(np.any(live[l - 1] & (sc.dst_type == t)))
            src_live = bool(np.any(live[l - 1] & (sc.src_type == t))) or dst_live
            nr = int(M['node_off'][t, hd + 1]) if dst_live else 0
            ns = int(M['node_off'][t, hd + 2]) if src_live else 0
            lr, ls = nr, ns
            if caps is not None:
                lr = int(caps.node_off[t][hd + 1]) if dst_live else 0
                ls = int(caps.node_off[t][hd + 2]) if src_live else 0
                if nr > lr or ns > ls:
                    M['error'] |= 32
            M['n_rows'][l - 1, t], M['n_src'][l - 1, t] = nr, ns
            M['lay_rows'][l - 1, t], M['lay_src'][l - 1, t] = lr, ls
            M['z_base'][l - 1, t], M['src_base'][l - 1, t], M['t_base'][l - 1, t] = zb, sb, tb
            zb += lr * R_dst[t]; sb += ls; tb += ls * R_src[t]
        M['z_base'][l - 1, NT], M['src_base'][l - 1, NT], M['t_base'][l - 1, NT] = zb, sb, tb
        M['n_chunks'][l - 1], M['n_edges'][l - 1] = M['chunk_end'][hd], M['edge_end'][hd]
        if tb > tg.trow_cap:
            M['error'] |= 16

    out = dict(meta=M, schema=sc, L=L, n_hops=n_hops, rel_live=live, short_mask=tg.short_mask, node_base=tg.node_base,
               n_id=[np.concatenate(x) for x in nid], seg_deg=seg_deg, seg_nch=seg_nch, seg_ptr=seg_ptr, seg_chptr=seg_chptr,
               col_local=col_local, chunks=chunks, multi=multi, t_ptr=[], t_edge=[], t_zrow=[], t_rel=[], flags=[])
    g2l = np.full(int(tg.node_base[NT]), -1, dtype=np.int64)
    for t in range(NT):
        g2l[tg.node_base[t]:tg.node_base[t] + tg.n_nodes[t]] = local[t]
    out['g2l'] = g2l
    if M['error']:
        return out                                           # (nothing past the layer tables is specified)

    # ---- src-major structures: the layer's live edges stably sorted by row -------------------------------------------------
    e_seg = np.repeat(np.arange(len(seg_deg)), seg_deg)
    e_rel, e_row = seg_rel[e_seg], seg_row[e_seg]
    for l in range(1, L + 1):
        ne = int(M['n_edges'][l - 1])
        edges = np.nonzero(live[l - 1][e_rel[:ne]])[0]
        rel = e_rel[edges]
        sT, dT = sc.src_type[rel], sc.dst_type[rel]
        key = M['t_base'][l - 1][sT] + col_local[edges] * R_src[sT] + sc.slot_src[rel]
        order = np.argsort(key, kind='stable')
        TR = int(M['t_base'][l - 1, NT])
        M['t_entries'][l - 1] = len(edges)
        t_ptr = np.searchsorted(key[order], np.arange(TR + 1), side='left')
        out['t_ptr'].append(t_ptr)
        out['t_edge'].append(edges[order])
        out['t_zrow'].append((M['z_base'][l - 1][dT] + e_row[edges] * R_dst[dT] + sc.slot_dst[rel])[order])
        out['t_rel'].append(rel[order])
        out['flags'].append(octet_flags(sc, tg.short_mask, M, l, t_ptr))
    return out


def sorted_rows(a):
    """The rows of a 2-D int array in lexicographic order (an unordered record list as a comparable value)."""
    a = np.asarray(a, dtype=np.int64)
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def octet_flags(sc, short_mask, M, l, t_ptr):
    """One flag per 8 consecutive source rows of layer l's input: eight real rows of ONE short-row node type
    (KgwGraph.short_types), none of them a destination row of the layer, each with at most 8 src-major entries over all its
    relation slots."""
    NT = sc.NT
    sb, tb = M['src_base'][l - 1], M['t_base'][l - 1]
    u0 = 8 * np.arange((int(sb[NT]) + 7) // 8, dtype=np.int64)
    ty = np.searchsorted(sb[1:NT], u0, side='right')
    j0 = u0 - sb[ty]
    short = np.array([(short_mask >> t) & 1 for t in range(NT)], dtype=bool)
    ok = short[ty] & (j0 + 8 <= M['n_src'][l - 1][ty]) & ~((sc.R_dst[ty] > 0) & (j0 < M['n_rows'][l - 1][ty]))
    Rs = sc.R_src.astype(np.int64)[ty]
    t0 = tb[ty] + j0 * Rs
    for q in range(8):
        i0, i1 = np.where(ok, t0 + q * Rs, 0), np.where(ok, t0 + (q + 1) * Rs, 0)
        ok &= t_ptr[i1] - t_ptr[i0] <= 8
    return ok.astype(np.int64)


def check_structures(v):
    """Structural invariants of a sampled batch given as the dict ``sample_twin`` returns (or the same read back from the device):
    the chunk list covers every local edge exactly once, multi-chunk segments are listed, the src-major structure of every layer is
    a permutation of the layer's live edges grouped by (source row, slot) in ascending edge order, octet flags by their rule."""
    sc, L, m = v['schema'], v['L'], v['meta']
    n_hops = v['n_hops']
    n_chunks_all = int(m['chunk_end'][n_hops - 1])
    n_edges_all = int(m['edge_end'][n_hops - 1])
    ch = np.asarray(v['chunks'])[:n_chunks_all]
    col = np.asarray(v['col_local'])[:n_edges_all]
    assert n_chunks_all > 0 and n_edges_all > 0
    # chunks tile [0, n_edges) in order
    assert ch[0, 0] == 0 and ch[-1, 1] == n_edges_all
    assert np.array_equal(ch[1:, 0], ch[:-1, 1])
    assert np.all(ch[:, 1] - ch[:, 0] <= KGW_CHUNK) and np.all(ch[:, 1] > ch[:, 0])
    n_multi = sum(int(m['multi_cnt'][h]) for h in range(n_hops))
    assert n_multi == len(np.unique(ch[ch[:, 5] > 1][:, 4]))
    if v.get('expect_multi', True):
        assert n_multi > 0, 'test graph should contain rows above KGW_CHUNK edges'
    for l in range(1, L + 1):
        nc, ne = int(m['n_chunks'][l - 1]), int(m['n_edges'][l - 1])
        live = np.asarray(v['rel_live'][l - 1], dtype=bool)
        chl = ch[:nc]
        chl = chl[live[chl[:, 3]]]
        n_live_edges = int((chl[:, 1] - chl[:, 0]).sum())
        assert int(m['t_entries'][l - 1]) == n_live_edges
        t_rows = int(m['t_base'][l - 1][sc.NT])
        tptr = np.asarray(v['t_ptr'][l - 1])[:t_rows + 1]
        tedge = np.asarray(v['t_edge'][l - 1])[:n_live_edges]
        tz = np.asarray(v['t_zrow'][l - 1])[:n_live_edges]
        trel = np.asarray(v['t_rel'][l - 1])[:n_live_edges]
        assert tptr[0] == 0 and tptr[-1] == n_live_edges and np.all(np.diff(tptr) >= 0)
        # permutation of the live edge ids
        expect = np.concatenate([np.arange(a, b) for a, b in chl[:, :2]]) if len(chl) else np.zeros(0, np.int64)
        assert np.array_equal(np.sort(tedge), np.sort(expect))
        # every entry sits in the row of its (source, slot) and carries its destination Z row
        e2chunk = np.searchsorted(ch[:, 1], tedge, side='right')
        rel = ch[e2chunk, 3]
        row = ch[e2chunk, 2]
        src_t = sc.src_type[rel]
        dst_t = sc.dst_type[rel]
        tb = np.array([m['t_base'][l - 1][t] for t in range(sc.NT + 1)])
        zb = np.array([m['z_base'][l - 1][t] for t in range(sc.NT + 1)])
        trow = tb[src_t] + col[tedge] * sc.R_src[src_t] + sc.slot_src[rel]
        pos = np.arange(n_live_edges)
        assert np.all(tptr[trow] <= pos) and np.all(pos < tptr[trow + 1])
        assert np.array_equal(tz, zb[dst_t] + row * sc.R_dst[dst_t] + sc.slot_dst[rel])
        assert np.array_equal(trel, rel)      # relation id per entry
        # octet flags (the backward's 8-rows-per-wavefront path): set exactly for the groups of 8 real source rows of one
        # short-row type that hold no destination row and no row above 8 entries
        n_src_rows = int(m['src_base'][l - 1][sc.NT])
        flags = np.asarray(v['flags'][l - 1])[:(n_src_rows + 7) // 8]
        sb = np.array([m['src_base'][l - 1][t] for t in range(sc.NT + 1)])
        for o in range(len(flags)):
            u0 = 8 * o
            ty = int(np.searchsorted(sb[1:], u0, side='right'))
            j0 = u0 - sb[ty]
            ok = bool((v['short_mask'] >> ty) & 1) and j0 + 8 <= int(m['n_src'][l - 1][ty]) and \
                not (sc.R_dst[ty] > 0 and j0 < int(m['n_rows'][l - 1][ty]))
            if ok:
                Rs = int(sc.R_src[ty])
                t0 = tb[ty] + j0 * Rs
                ok = all(tptr[t0 + (q + 1) * Rs] - tptr[t0 + q * Rs] <= 8 for q in range(8))
            assert bool(flags[o]) == ok, (l, o)
        assert ne <= n_edges_all
        # deterministic order: inside every src-major row the entries ascend by edge id (the structure is the edge list
        # STABLY sorted by row: k_ts_scatter / k_ts_rows rank equal keys by lane order, nothing depends on arrival order)
        row_of = np.repeat(np.arange(t_rows), np.diff(tptr))
        same = row_of[1:] == row_of[:-1]
        assert np.all(tedge[1:][same] > tedge[:-1][same])


def global_edges(v):
    """{edge type: (global src, global dst) pairs of the batch, sorted by (dst, src)} from the segment arrays."""
    sc, m = v['schema'], v['meta']
    out = {}
    for r, et in enumerate(sc.edge_types):
        s, d = int(sc.src_type[r]), int(sc.dst_type[r])
        pairs = [np.zeros((0, 2), np.int64)]
        for h in range(v['n_hops']):
            a, b = int(m['seg_off'][h][r]), int(m['seg_off'][h][r + 1])
            sp = np.asarray(v['seg_ptr'])[a:b + 1]
            if b <= a:
                continue
            rows = int(m['node_off'][d][h]) + np.repeat(np.arange(b - a), np.diff(sp))
            pairs.append(np.stack([v['n_id'][s][np.asarray(v['col_local'])[sp[0]:sp[-1]]], v['n_id'][d][rows]], axis=1))
        p = np.concatenate(pairs)
        out[et] = p[np.lexsort((p[:, 0], p[:, 1]))]
    return out
