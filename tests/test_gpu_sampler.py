"""-m gpu: kgw_sample_batch against the PyG NeighborLoader([-1]*L) restatement (oracle/pyg_semantics.py).
Integer work => exact comparisons."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pyg_semantics as P
from tests.helpers import global_edge_set

pytestmark = pytest.mark.gpu


def _loader(data, ids, bs, L=2, **kw):
    from kgwas_amd.sampler import NeighborLoader
    return NeighborLoader(data, num_neighbors=[-1] * L, input_nodes=('SNP', ids), batch_size=bs, device='cuda:0', **kw)


def _oracle_sets(data, seeds, L=2):
    smp = P.FullNeighborSampler(data.edge_index_dict, data.num_nodes_dict, L)
    n_id, ei, hops = smp.sample('SNP', seeds)
    edges = {}
    for et, e in ei.items():
        s, _, d = et
        pairs = np.stack([n_id[s].numpy()[e[0].numpy()], n_id[d].numpy()[e[1].numpy()]], axis=1) if e.shape[1] \
            else np.zeros((0, 2), np.int64)
        order = np.lexsort((pairs[:, 0], pairs[:, 1]))
        edges[et] = pairs[order]
    return n_id, edges, hops


@pytest.mark.parametrize('which', ['small', 'edge'])
@pytest.mark.parametrize('L', [1, 2, 3])
def test_sampler_matches_pyg_semantics(small_kg, edge_case_graph, which, L):
    data = small_kg.data if which == 'small' else edge_case_graph[0]
    n_snp = data['SNP'].x.shape[0]
    rng = np.random.default_rng(5)
    ids = rng.choice(n_snp, size=96, replace=False)
    ld = _loader(data, ids, 32, L=L)
    assert len(ld) == 3
    for b, batch in enumerate(ld):
        seeds = ids[b * 32:(b + 1) * 32]
        n_id_o, edges_o, hops_o = _oracle_sets(data, seeds, L)
        assert batch['SNP'].batch_size == 32
        # seeds first, in seed order (the only ordering contract the reference consumes, model.py:86)
        assert np.array_equal(batch.n_id('SNP')[:32].cpu().numpy(), seeds)
        for t in data.node_types:
            mine = batch.n_id(t).cpu().numpy()
            assert len(np.unique(mine)) == len(mine), f'duplicate nodes in {t}'
            assert np.array_equal(np.sort(mine), np.sort(n_id_o[t].numpy())), f'node set of {t} differs'
            # hop-major, ascending global id inside a hop (beyond the seeds)
            m = batch.meta
            ti = batch.dg.schema.type_id[t]
            for k in range(1, L + 1):
                a, bnd = int(m.node_off[ti][k]), int(m.node_off[ti][k + 1])
                seg = mine[a:bnd]
                assert np.all(np.diff(seg) > 0), f'{t} hop {k} not sorted'
                ref_hop = np.sort(n_id_o[t].numpy()[hops_o[t].numpy() == k])
                assert np.array_equal(seg, ref_hop), f'{t} hop {k} membership differs'
        for et in data.edge_types:
            assert np.array_equal(global_edge_set(batch, et), edges_o[et]), f'edge multiset of {et} differs'
        assert batch.n_edges_sampled == sum(len(v) for v in edges_o.values())


@pytest.mark.parametrize('which', ['small', 'edge'])
def test_block_structures_are_consistent(small_kg, edge_case_graph, which):
    """Chunk list covers every local edge exactly once; multi-chunk segments are listed; the src-major
    structure of every layer is a permutation of the layer's live edges grouped by (source row, slot)."""
    if which == 'small':
        data = small_kg.data
        ids = np.random.default_rng(0).choice(data['SNP'].x.shape[0], size=512, replace=False)
    else:   # seeds around the 1500-edge hub gene 0
        data = edge_case_graph[0]
        ids = np.random.default_rng(0).choice(1500, size=64, replace=False)
    check_block_structures(next(iter(_loader(data, ids, len(ids), L=2))))


def batch_view(batch):
    """A sampled batch read back as the plain-array dict of tests/sampler_twin.py (``sample_twin`` returns the same keys)."""
    from tests.sampler_twin import meta_to_dict
    dg, m, buf = batch.dg, batch.meta, batch.buf
    sc, L, H = dg.schema, dg.num_layers, dg.n_hops
    ns, ne, nc = int(m.seg_end[H - 1]), int(m.edge_end[H - 1]), int(m.chunk_end[H - 1])
    cpu = lambda t: t.cpu().numpy().astype(np.int64)
    mcap = int(buf.c.multi_cap)
    v = dict(meta=meta_to_dict(m), schema=sc, L=L, n_hops=H, short_mask=dg.short_type_mask,
             rel_live=np.array([[dg.kg.rel_live[l][r] for r in range(sc.NR)] for l in range(L)], dtype=bool),
             node_base=np.array(dg.node_base), g2l=cpu(buf.g2l),
             n_id=[cpu(buf.n_id[dg.node_base[t]:dg.node_base[t] + int(m.node_off[t][H + 1])]) for t in range(sc.NT)],
             seg_deg=cpu(buf.seg_deg[:ns]), seg_nch=cpu(buf.seg_nch[:ns]), seg_ptr=cpu(buf.seg_ptr[:ns + 1]),
             seg_chptr=cpu(buf.seg_chptr[:ns + 1]), col_local=cpu(buf.col_local[:ne]), chunks=cpu(buf.chunks[:nc * 8]).reshape(-1, 8),
             multi=[cpu(buf.multi[h * mcap * 4:(h * mcap + min(int(m.multi_cnt[h]), mcap)) * 4]).reshape(-1, 4) for h in range(H)],
             t_ptr=[], t_edge=[], t_zrow=[], t_rel=[], flags=[])
    for l in range(L):
        nt = int(m.t_entries[l])
        v['t_ptr'].append(cpu(buf.t_ptr[l][:int(m.t_base[l][sc.NT]) + 1]))
        v['t_edge'].append(cpu(buf.t_edge[l][:nt]))
        v['t_zrow'].append(cpu(buf.t_zrow[l][:nt]))
        v['t_rel'].append(cpu(buf.t_rel[l][:nt]))
        v['flags'].append(cpu(buf.t_cnt[l][:(int(m.src_base[l][sc.NT]) + 7) // 8]))
    return v


def check_block_structures(batch):
    """The body of test_block_structures_are_consistent on any sampled batch (tests/test_gpu_shard_kernels.py calls it on the
    rank-local batches of the SNP-sharded mode): the assertions live in tests/sampler_twin.py (check_structures), where the
    sampler's numpy twin is held to them too."""
    from tests.sampler_twin import check_structures
    check_structures(batch_view(batch))


def test_full_graph_block(edge_case_graph):
    """full_graph mode: identity node maps, every edge of every relation exactly once."""
    from kgwas_amd.sampler import sample_full_graph
    data = edge_case_graph[0]
    batch = sample_full_graph(data, 2, 'cuda:0')
    for t in data.node_types:
        n = data[t].x.shape[0]
        assert np.array_equal(batch.n_id(t).cpu().numpy(), np.arange(n))
    tot = 0
    for et in data.edge_types:
        ei = data[et].edge_index.numpy()
        got = global_edge_set(batch, et)
        order = np.lexsort((ei[0], ei[1]))
        assert np.array_equal(got, ei.T[order])
        tot += ei.shape[1]
    assert batch.n_edges_sampled == tot


def test_loader_contract(small_kg):
    """len / drop_last / prefetch on-off give identical batches (kgwas.py:93-94: fixed order, no shuffle)."""
    data = small_kg.data
    ids = np.asarray(small_kg.train_input_nodes[1][:200])
    a = _loader(data, ids, 64, drop_last=True)
    b = _loader(data, ids, 64, drop_last=False, prefetch=False)
    assert len(a) == 3 and len(b) == 4
    sizes = []
    for x, y in zip(a, b):
        assert np.array_equal(x.n_id('SNP').cpu().numpy(), y.n_id('SNP').cpu().numpy())
        assert x.n_edges_sampled == y.n_edges_sampled
        assert torch.equal(x['SNP'].y[:64], data['SNP'].y[x['SNP']['n_id'][:64].cpu()].cuda())
        sizes.append(x.n_edges_sampled)
    assert [bb['SNP'].batch_size for bb in b] == [64, 64, 64, 8]
    xd = next(iter(a)).x_dict
    assert set(xd.keys()) == set(data.node_types)


def test_loader_on_cached_graph_equals_direct(tiny_kg, tmp_path):
    """kgwas_amd/ingest.py: a DeviceGraph fed from the on-disk CSR cache samples exactly what one built from COO does."""
    from kgwas_amd import ingest
    from kgwas_amd.kgwas_data import KGWAS_Data
    cache = ingest.convert(tiny_kg, str(tmp_path / 'cache'))
    other = ingest.load(KGWAS_Data(str(tmp_path / 'dp')), cache)
    ids = np.random.default_rng(5).choice(tiny_kg.data['SNP'].x.shape[0], size=32, replace=False)
    a = next(iter(_loader(tiny_kg.data, ids, 32, L=2)))
    b = next(iter(_loader(other.data, ids, 32, L=2)))
    for t in tiny_kg.data.node_types:
        assert torch.equal(a.n_id(t), b.n_id(t))
        assert torch.equal(a.x_dict[t], b.x_dict[t])
    ea, eb = a.edge_index_dict, b.edge_index_dict
    for et in ea:
        assert torch.equal(ea[et], eb[et])


@pytest.mark.parametrize('shift', [8, 12, 14])
def test_coarse_bucket_sort_plans_build_the_same_structures(shift):
    """the src-major sort's coarse plans (2^12 rows per bucket, four wavefronts; 2^14, one wavefront) launch
    k_ts_rows with 64 KB of dynamic LDS + its static words -- above the 64 KB default limit -- and are only chosen above
    8 M / 65 M src-major rows, which no test graph has.  KGW_TS_MIN_SHIFT forces them (read once per process, hence the
    subprocess); the structure checks above must hold unchanged.  (8: the fine buckets that were the default until round 6 --
    the default is 2^11 rows now.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KGW_TS_MIN_SHIFT=str(shift))
    # ... and, array for array against the numpy twin, the ladder graph at L = 2 with one launch geometry per key-block count
    # (grid_blocks 1 / 256 / 0 -> 128 / 256 / 512 blocks): tests/test_gpu_sampler_exact.py
    p = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-m', 'gpu', os.path.join(root, 'tests', 'test_gpu_sampler.py'),
                        os.path.join(root, 'tests', 'test_gpu_sampler_exact.py'),
                        '-k', 'block_structures or matches_pyg_semantics or (launch_geometry and (g0001 or g0256 or g0000))'],
                       cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    assert ' passed' in p.stdout
