"""-m gpu: kgw_sample_batch against its numpy twin (tests/sampler_twin.py), EVERY array compared with np.array_equal -- at every
scan tile edge, node-tile edge, launch geometry and capacity; plus kgw_accumulate_stats[_tick] and kgw_segments_copy.
Everything the sampler writes is integer and deterministic (stable src-major sort, no atomics in the order of anything but the
``multi`` lists, which are compared as sorted sets of rows)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.sampler_twin import meta_to_dict, sample_twin, sorted_rows
from tests.test_gpu_sampler import batch_view
from tests.test_sampler_twin import (LADDER_CLOSED_SNP, LADDER_LONE_SNP, LADDER_N, LADDER_TILE_EDGE_SEEDS, ladder_seeds,
                                     make_ladder_graph, make_wide_graph, wide_seeds)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CANARY = 0x5A5A5A5A
GRIDS = (1, 3, 100, 255, 256, 1024, 2047, 2048, 0)


@pytest.fixture(scope='module')
def ladder_graph():
    return make_ladder_graph()


@pytest.fixture(scope='module')
def wide_graph():
    return make_wide_graph()


_BUFS = {}


def _dg(data, L, full=False, all_live=False):
    from kgwas_amd.sampler import DeviceGraph
    dg = DeviceGraph.get(data, L, DEV, full_graph=full)
    return dg.with_all_relations_live() if all_live else dg


def _buf(dg, grid=0):
    """One set of buffers per (resident graph, launch width): all the views of one DeviceGraph share them."""
    from kgwas_amd.sampler import BatchBuffers
    key = (dg.g_col.data_ptr(), dg.num_layers, dg.full_graph, grid)
    if key not in _BUFS:
        _BUFS[key] = BatchBuffers(dg, grid_blocks=grid)
    return _BUFS[key]


def _sample(dg, buf, seed_type, seeds):
    """One kgw_sample_batch call -> the batch read back as plain arrays (no exception on a capacity error: meta['error'])."""
    from kgwas_amd.sampler import SampledBatch, sample_into
    st = dg.schema.type_id[seed_type] if isinstance(seed_type, str) else seed_type
    ids = None if seeds is None else torch.from_numpy(np.asarray(seeds, dtype=np.int64)).to(DEV)
    sample_into(dg, buf, ids, st)
    torch.cuda.synchronize()
    meta = buf.read_meta()
    return SampledBatch(dg, buf, meta, 'SNP', 0 if seeds is None else len(seeds)), meta


def assert_same(got, want, what=''):
    """``got`` (device, read back) and ``want`` (twin, or another read-back) agree in every specified array."""
    for k in want['meta']:
        assert np.array_equal(got['meta'][k], want['meta'][k]), (what, 'meta.' + k, got['meta'][k], want['meta'][k])
    for k in ('g2l', 'seg_deg', 'seg_nch', 'seg_ptr', 'seg_chptr', 'col_local', 'chunks'):
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in ('n_id', 't_ptr', 't_edge', 't_zrow', 't_rel', 'flags'):
        assert len(got[k]) == len(want[k]), (what, k)
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert np.array_equal(a, b), (what, k, i)
    assert len(got['multi']) == len(want['multi'])
    for h, (a, b) in enumerate(zip(got['multi'], want['multi'])):
        assert np.array_equal(sorted_rows(a), sorted_rows(b)), (what, 'multi', h)       # (written in atomic arrival order)


def _exact(data, dg, buf, seed_type, seeds, what, **kw):
    batch, meta = _sample(dg, buf, seed_type, seeds)
    assert meta.error == 0, (what, meta.error)
    got = batch_view(batch)
    assert_same(got, sample_twin(data, dg.num_layers, seed_type, seeds, full_graph=dg.full_graph, **kw), what)
    return got


def _seed_sets(which, data):
    if which == 'ladder':
        return [('SNP', ladder_seeds('SNP', n)) for n in (1, 2, 32, 512)] + \
               [('MolecularFunction', ladder_seeds('MolecularFunction', n)) for n in LADDER_TILE_EDGE_SEEDS]
    n_snp = data['SNP'].x.shape[0]
    return [('SNP', np.random.default_rng(100 + n).choice(n_snp, size=n, replace=False)) for n in (1, 2, 32, 512)]


@pytest.mark.parametrize('all_live', [False, True], ids=['live_default', 'live_all'])
@pytest.mark.parametrize('L', [1, 2, 3])
@pytest.mark.parametrize('which', ['small', 'edge', 'ladder'])
def test_minibatch_equals_twin(small_kg, edge_case_graph, ladder_graph, which, L, all_live):
    data = {'small': small_kg.data, 'edge': edge_case_graph[0], 'ladder': ladder_graph}[which]
    dg = _dg(data, L, all_live=all_live)
    buf = _buf(dg)
    for seed_type, seeds in _seed_sets(which, data):
        _exact(data, dg, buf, seed_type, seeds, (which, L, seed_type, len(seeds)), all_live=all_live)


@pytest.mark.parametrize('which', ['edge', 'ladder', 'wide'])
def test_full_graph_equals_twin(edge_case_graph, ladder_graph, wide_graph, which):
    """n_hops = 1 under L = 2: both layers are hop-pruned to hd = min(L - l, n_hops - 1) = 0.  The wide graph has more than 256
    tiles of segments and of node slots (the second trip of k_scan_top's loop)."""
    data = {'edge': edge_case_graph[0], 'ladder': ladder_graph, 'wide': wide_graph}[which]
    dg = _dg(data, 2, full=True)
    got = _exact(data, dg, _buf(dg), 'SNP', None, which)
    if which == 'wide':
        assert int(got['meta']['seg_end'][0]) > 2 * 256 * 1024 and dg.node_slots // 1024 > 257
    assert list(got['meta']['n_edges'][:2]) == [int(got['meta']['edge_end'][0])] * 2


def test_wide_minibatch_equals_twin(wide_graph):
    """More than 256 node tiles (the second trip of k_scan_top_fixed), seeds in the first, a middle and the last of them."""
    dg = _dg(wide_graph, 2)
    seeds = wide_seeds(wide_graph['SNP'].x.shape[0])
    got = _exact(wide_graph, dg, _buf(dg), 'SNP', seeds, 'wide')
    assert dg.node_slots // 1024 > 257
    n = dg.n_nodes[0]
    assert {0, n // 2048, (n - 1) // 1024} <= set(got['n_id'][0][:len(seeds)] // 1024)


def test_ladder_graph_pins_the_edges(ladder_graph, capsys):
    """The conditions the ladder graph exists for, read back from the device: a later change of the graph cannot un-pin them
    silently.  States the 4 096-segment tiles of every hop's scan range and the range lengths mod 4 096 and mod 4."""
    data = ladder_graph
    dg3 = _dg(data, 3)
    sc = dg3.schema
    # node-tile ladder: 1025 | 1024 | a single node right behind the full tile | 1023 | the seed type of the tile-edge ranges
    assert dg3.n_nodes[:4] == [1025, 1024, 1, 1023] and dg3.n_nodes[4] >= max(LADDER_TILE_EDGE_SEEDS)
    assert dg3.node_base[2] % 1024 == 0 and dg3.node_base[2] - dg3.node_base[1] == dg3.n_nodes[1] == 1024
    seen_mod, later_long, lines = set(), False, []
    for n in LADDER_TILE_EDGE_SEEDS:
        batch, meta = _sample(dg3, _buf(dg3), 'MolecularFunction', ladder_seeds('MolecularFunction', n))
        ends = [0] + [int(meta.seg_end[h]) for h in range(3)]
        lens = np.diff(ends)
        assert lens[0] == n                         # one incoming relation: the hop-0 range is the seed count
        seen_mod.add(int(lens[0]) % 4096)
        later_long |= any(ends[h] > 0 and lens[h] > 4096 for h in (1, 2))
        lines.append(f'seeds {n}: ' + ', '.join(f'hop {h} begin {ends[h]} len {lens[h]} = {-(-lens[h] // 4096)} tiles, '
                                                  f'mod 4096 = {lens[h] % 4096}, mod 4 = {lens[h] % 4}' for h in range(3)))
    assert {4095, 0, 1} <= seen_mod and later_long
    assert [n % 4 for n in LADDER_TILE_EDGE_SEEDS] == [3, 0, 1, 0, 1] and [-(-n // 4096) for n in LADDER_TILE_EDGE_SEEDS] == [1, 1, 2, 2, 4]
    # SNP seeds: hub row over four chunks, rows of exactly 128 and 129, degree-0 rows, the empty relation, duplicates, self-loops
    dg2 = _dg(data, 2)
    v = batch_view(_sample(dg2, _buf(dg2), 'SNP', ladder_seeds('SNP', 512))[0])
    m = v['meta']
    deg = v['seg_deg']
    assert (deg == 128).any() and (deg == 129).any() and (deg == 0).any() and v['seg_nch'].max() > 4
    assert set(v['seg_nch'][deg == 128]) == {1} and set(v['seg_nch'][deg == 129]) == {2}
    r_empty = sc.edge_types.index(('SNP', 'EMPTY', 'Gene'))
    a, b = int(m['seg_off'][1][r_empty]), int(m['seg_off'][1][r_empty + 1])
    assert b > a and not deg[a:b].any()
    r_abc, r_g2g = sc.edge_types.index(('SNP', 'ABC', 'Gene')), sc.edge_types.index(('Gene', 'G2G', 'Gene'))
    seg_rel = np.repeat(np.arange(len(deg)), deg)
    dup = loops = False
    for s in np.nonzero(deg > 0)[0]:
        r = int(np.searchsorted(m['seg_off'][1][:sc.NR + 1], s, side='right') - 1) if s >= int(m['seg_end'][0]) else -1
        cols = v['col_local'][v['seg_ptr'][s]:v['seg_ptr'][s + 1]]
        if r == r_abc:
            dup |= bool((np.diff(cols) == 0).any())
        if r == r_g2g:
            loops |= bool((cols == int(m['node_off'][1][1]) + s - int(m['seg_off'][1][r])).any())
    assert dup and loops and len(seg_rel) == int(m['edge_end'][1])
    lone = int(np.nonzero(v['n_id'][0][:512] == LADDER_LONE_SNP)[0][0])       # a seed with no in-edge at all
    assert not any(deg[int(m['seg_off'][0][r]) + lone] for r in range(sc.NR) if int(sc.dst_type[r]) == 0)
    # the closed pair: hop 2 of 3 finds no new node of any type (and hop 3 has no segment at all)
    _, meta = _sample(dg3, _buf(dg3), 'SNP', np.array([LADDER_CLOSED_SNP]))
    assert all(int(meta.hop_cnt[t][2]) == 0 and int(meta.hop_cnt[t][3]) == 0 for t in range(sc.NT))
    assert int(meta.hop_cnt[1][1]) == 1 and int(meta.seg_end[2]) == int(meta.seg_end[1]) > int(meta.seg_end[0])
    with capsys.disabled():
        print('\n' + '\n'.join(lines))


@pytest.fixture(scope='module')
def geometry_ref(ladder_graph):
    """The ladder graph at L = 2 under the default launch width: what every other width must reproduce bit for bit."""
    dg = _dg(ladder_graph, 2)
    cases = [('SNP', ladder_seeds('SNP', 512)), ('MolecularFunction', ladder_seeds('MolecularFunction', 4097))]
    return cases, [batch_view(_sample(dg, _buf(dg, 0), t, s)[0]) for t, s in cases]


@pytest.mark.parametrize('grid', GRIDS, ids=['g%04d' % g for g in GRIDS])
def test_launch_geometry_changes_nothing(ladder_graph, geometry_ref, grid):
    """KgwBatchBuf.grid_blocks: the width of every grid-stride launch and, through it, the key-block count of the src-major sort
    (128 below 256, 256 below 2 048, else 512: k_ts_scan_rows<2|4|8>, ts_block_range)."""
    dg = _dg(ladder_graph, 2)
    cases, ref = geometry_ref
    for (seed_type, seeds), want in zip(cases, ref):
        got = _exact(ladder_graph, dg, _buf(dg, grid), seed_type, seeds, (grid, seed_type))
        assert_same(got, want, (grid, seed_type, 'vs grid 0'))


def _caps_from(meta, NT, L, extra=0):
    from kgwas_amd.sampler import BatchCaps
    return BatchCaps([[0] + [int(meta.node_off[t][k]) + extra for k in range(1, L + 2)] for t in range(NT)], [0] * L, [0] * L)


def test_static_layout_equals_twin(ladder_graph):
    dg = _dg(ladder_graph, 2)
    buf = _buf(dg)
    seeds = ladder_seeds('SNP', 512)
    _, clean = _sample(dg, buf, 'SNP', seeds)
    NT = dg.schema.NT
    for extra in (0, 37):                           # capacities equal to the batch's own counts, and well above them
        caps = _caps_from(clean, NT, 2, extra)
        got = _exact(ladder_graph, dg.with_static_caps(caps), buf, 'SNP', seeds, ('static', extra), caps=caps)
        assert np.array_equal(got['meta']['n_rows'], meta_to_dict(clean)['n_rows'])
        assert int(got['meta']['lay_src'][0][1]) == int(clean.n_src[0][1]) + extra
    gene = dg.schema.type_id['Gene']
    for field in ('cap_rows', 'cap_src'):           # one capacity one below need: rows, then sources
        dgs = dg.with_static_caps(_caps_from(clean, NT, 2))
        getattr(dgs.kg, field)[0][gene] -= 1
        _, meta = _sample(dgs, buf, 'SNP', seeds)
        assert meta.error == 32, (field, meta.error)


GUARDS = (('seg_cap', 1), ('edge_cap', 2), ('chunk_cap', 4), ('multi_cap', 8), ('trow_cap', 16))


def _guard_need(meta, L, NT):
    return dict(seg_cap=int(meta.seg_end[L - 1]), edge_cap=int(meta.edge_end[L - 1]), chunk_cap=int(meta.chunk_end[L - 1]),
                multi_cap=max(int(meta.multi_cnt[h]) for h in range(L)), trow_cap=max(int(meta.t_base[l][NT]) for l in range(L)))


def _fresh_guard_buf(dg):
    from kgwas_amd.sampler import BatchBuffers
    buf = BatchBuffers(dg)
    for t in buf.tensors():
        if t is not buf.meta:
            t.fill_(CANARY if t.dtype == torch.int32 else CANARY & 0xFF)
    return buf


@pytest.mark.parametrize('field,bit', GUARDS, ids=[g[0] for g in GUARDS])
def test_capacity_guards(ladder_graph, field, bit):
    """Only the capacity FIELD of KgwBatchBuf is lowered; the tensors keep their full size (a test of the status path, not of
    memory safety).  At need: no error, the batch equals the twin.  At need - 1: exactly the documented bit, and nothing at or past
    the lowered capacity was written."""
    dg = _dg(ladder_graph, 2)
    seeds = ladder_seeds('SNP', 512)
    L, NT = 2, dg.schema.NT
    _, clean = _sample(dg, _buf(dg), 'SNP', seeds)
    need = _guard_need(clean, L, NT)[field]
    assert need > 1
    buf = _fresh_guard_buf(dg)
    setattr(buf.c, field, need)
    _exact(ladder_graph, dg, buf, 'SNP', seeds, (field, 'need'))
    buf = _fresh_guard_buf(dg)
    cap = need - 1
    setattr(buf.c, field, cap)
    _, meta = _sample(dg, buf, 'SNP', seeds)
    assert meta.error == bit, (field, meta.error)
    past = {'seg_cap': [(buf.seg_deg, cap), (buf.seg_nch, cap), (buf.seg_ptr, cap + 1), (buf.seg_chptr, cap + 1)],
            'edge_cap': [(buf.col_local, cap)] + [(t, cap) for t in buf.t_edge + buf.t_zrow + buf.t_rel],
            'chunk_cap': [(buf.chunks, cap * 8)],
            'multi_cap': [(buf.multi, L * cap * 4)],
            'trow_cap': [(t, cap + 1) for t in buf.t_ptr + buf.t_cnt]}[field]
    for t, start in past:
        tail = t[start:].cpu().numpy()
        assert len(tail) and np.all(tail == (CANARY if t.dtype == torch.int32 else CANARY & 0xFF)), (field, start)


def test_accumulate_stats(ladder_graph):
    """stats[l] += n_edges of layer l + 1, stats[L] += edges sampled, stats[L + 1] |= error (sticky), tick += 1 -- over three
    batches, one of them past its edge capacity (error bit 1; its edge counts are still the batch's)."""
    from kgwas_amd import _lib
    lib = _lib.lib()
    dg = _dg(ladder_graph, 2)
    L = 2
    batches = [('SNP', ladder_seeds('SNP', 32)), ('SNP', ladder_seeds('SNP', 512)), ('MolecularFunction', ladder_seeds('MolecularFunction', 40))]
    _, clean = _sample(dg, _buf(dg), *batches[1])
    buf = _fresh_guard_buf(dg)
    stats = torch.zeros(L + 2, dtype=torch.int64, device=DEV)
    tick = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    want = np.zeros(L + 2, dtype=np.int64)
    p = lambda t: C.c_void_p(t.data_ptr())
    for i, (seed_type, seeds) in enumerate(batches):
        buf.c.edge_cap = int(clean.edge_end[L - 1]) - 1 if i == 1 else dg.edge_cap
        _, meta = _sample(dg, buf, seed_type, seeds)
        assert meta.error == (2 if i == 1 else 0)
        if i == 0:
            rc = lib.kgw_accumulate_stats(p(buf.meta), L, L, p(stats), _lib.stream_ptr())
        else:
            rc = lib.kgw_accumulate_stats_tick(p(buf.meta), L, L, p(stats), p(tick), _lib.stream_ptr())
        assert rc == 0
        tm = sample_twin(ladder_graph, L, seed_type, seeds)['meta']
        want[:L] += tm['n_edges'][:L]
        want[L] += tm['edge_end'][L - 1]
        want[L + 1] |= int(meta.error)
        assert np.array_equal(stats.cpu().numpy(), want), i
    assert want[L + 1] == 2 and int(tick.item()) == 7
    null = C.c_void_p(0)
    assert lib.kgw_accumulate_stats(null, L, L, p(stats), _lib.stream_ptr()) == -1            # KGW_E_NULL
    assert lib.kgw_accumulate_stats_tick(p(buf.meta), L, L, null, p(tick), _lib.stream_ptr()) == -1
    for nl, nh in ((0, 1), (5, 1), (2, 0), (2, 3)):                                               # KGW_E_RANGE
        assert lib.kgw_accumulate_stats(p(buf.meta), nl, nh, p(stats), _lib.stream_ptr()) == -2
    torch.cuda.synchronize()
    assert np.array_equal(stats.cpu().numpy(), want) and int(tick.item()) == 7                    # (a refused call does nothing)


@pytest.mark.parametrize('grid', [1, 0])
def test_segments_copy_round_trip(grid):
    """40 segments of unequal 16-byte unit counts (a zero-unit one among them) to slot 2 of 4 and back: the neighbouring slots,
    the bytes between the segments (in the slot and in the arrays) stay as they were."""
    from kgwas_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(3)
    n = _lib.KGW_SEGCOPY_MAX
    units = rng.integers(1, 700, n)
    units[7], units[0], units[39] = 0, 1, 5000
    gap = 16 * rng.integers(1, 4, n)                             # bytes between the segments, in the arrays and in the slot
    a_off = np.concatenate([[32], 32 + np.cumsum(16 * units + gap)[:-1]])
    s_off = np.concatenate([[16], 16 + np.cumsum(16 * units + 2 * gap)[:-1]])
    a_bytes = int(a_off[-1] + 16 * units[-1] + 48)
    stride = int(s_off[-1] + 16 * units[-1] + 32)
    src0 = torch.from_numpy(rng.integers(0, 256, a_bytes, dtype=np.uint8)).to(DEV)
    arr = src0.clone()
    slots = torch.full((4 * stride,), 0xC3, dtype=torch.uint8, device=DEV)
    idx = torch.tensor([2], dtype=torch.int64, device=DEV)
    plan = _lib.KgwSegCopy()
    plan.n, plan.to_slot = n, 1
    for j in range(n):
        plan.ptr[j], plan.units[j], plan.slot_off[j] = arr.data_ptr() + int(a_off[j]), int(units[j]), int(s_off[j])
    plan.slots, plan.slot_stride, plan.slot_index = slots.data_ptr(), stride, idx.data_ptr()
    assert lib.kgw_segments_copy(C.byref(plan), grid, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    want_slots = np.full(4 * stride, 0xC3, dtype=np.uint8)
    h0 = src0.cpu().numpy()
    for j in range(n):
        want_slots[2 * stride + s_off[j]:2 * stride + s_off[j] + 16 * units[j]] = h0[a_off[j]:a_off[j] + 16 * units[j]]
    assert np.array_equal(slots.cpu().numpy(), want_slots)
    assert torch.equal(arr, src0)
    arr.fill_(0x11)                                              # ... and back
    plan.to_slot = 0
    assert lib.kgw_segments_copy(C.byref(plan), grid, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    want_arr = np.full(a_bytes, 0x11, dtype=np.uint8)
    for j in range(n):
        want_arr[a_off[j]:a_off[j] + 16 * units[j]] = h0[a_off[j]:a_off[j] + 16 * units[j]]
    assert np.array_equal(arr.cpu().numpy(), want_arr)
    assert np.array_equal(slots.cpu().numpy(), want_slots)
    # refusals (nothing is launched)
    plan.ptr[3] += 4
    assert lib.kgw_segments_copy(C.byref(plan), grid, _lib.stream_ptr()) == -3                  # misaligned pointer
    plan.ptr[3] -= 4
    plan.slot_off[3] += 8
    assert lib.kgw_segments_copy(C.byref(plan), grid, _lib.stream_ptr()) == -3                  # misaligned offset
    plan.slot_off[3] -= 8
    plan.slot_stride = stride - 48                                                               # the last segment overruns the slot
    assert lib.kgw_segments_copy(C.byref(plan), grid, _lib.stream_ptr()) == -2
    plan.slot_stride = stride
    plan.n = n + 1
    assert lib.kgw_segments_copy(C.byref(plan), grid, _lib.stream_ptr()) == -2                  # n = 41
    plan.n = n
    plan.slot_index = None
    assert lib.kgw_segments_copy(C.byref(plan), grid, _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert np.array_equal(arr.cpu().numpy(), want_arr) and np.array_equal(slots.cpu().numpy(), want_slots)
