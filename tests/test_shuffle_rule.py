"""CPU: the per-epoch order of the training seeds (kgwperm_index, kgw_epoch_order) -- its numpy twin's properties, the host's word
and index, the header's statement of the rule, and the refusals that need no GPU."""
import os
import re

import numpy as np
import pytest

from tests import attn_dropout_ref, fanout_ref
from tests import shuffle_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 956, 1023, 1024, 1025, 4097, 65537, 489_839, 784_256]
WORDS = [0, (1 << 64) - 1, R.order_word(0, 0), R.order_word(42, 3), R.order_word(2 ** 63 + 5, 123456)]
N_BENCH = 489_839            # training SNPs of the benchmark graph: 956 batches of 512


def test_twin_is_a_permutation():
    """1. every n of the list, five words (0 and all-ones among them): a permutation of [0, n); the walks stay short -- the domain
    of the network is at most 4 n, so a walk takes at most 4 applications on average."""
    longest = 0
    for n in NS:
        for w in WORDS:
            p, walks = R.permutation(w, n, with_walks=True)
            assert p.shape == (n,) and np.array_equal(np.sort(p), np.arange(n)), (n, w)
            assert 1 << (2 * R.half_bits(n)) <= 4 * n
            assert walks.mean() <= 4.0, (n, w, walks.mean())
            longest = max(longest, int(walks.max()))
    print('longest walk', longest)
    assert R.half_bits(1) == R.half_bits(4) == 1 and R.half_bits(5) == 2 and R.half_bits(17) == 3 and R.half_bits(1 << 31) == 16


def test_order_word_is_its_own():
    from kgwas_amd.sampler import dropout_word, fanout_sample_word, order_word
    for s, e in ((0, 0), (42, 1), (2 ** 63 + 5, 123456)):
        assert order_word(s, e) == R.order_word(s, e)
        assert order_word(s, e) != dropout_word(s, e, 0) == attn_dropout_ref.dropout_word(s, e, 0)
        assert order_word(s, e) != fanout_sample_word(s, e, 0) == fanout_ref.sample_word(s, e, 0)
        assert order_word(s, e) != order_word(s, e + 1) and order_word(s, e) != order_word(s + 1, e)
    assert len({order_word(7, e) for e in range(100)}) == 100


def test_host_index_equals_the_twin():
    """2. epoch_order_index (python ints) against the twin, every i of the small n, a sample of the large ones."""
    from kgwas_amd.sampler import epoch_order_index, epoch_order_len
    rng = np.random.default_rng(0)
    for n in NS:
        for w in WORDS:
            p = R.permutation(w, n)
            idx = np.arange(n) if n <= 1025 else np.concatenate([[0, n - 1], rng.integers(0, n, 200)])
            assert [epoch_order_index(w, n, int(i)) for i in idx] == p[idx].tolist(), (n, w)
    for bad in ((0, 0), (5, 5), (5, -1), ((1 << 31) + 1, 0)):
        with pytest.raises(ValueError):
            epoch_order_index(0, *bad)
    assert epoch_order_index(R.order_word(1, 2), 1 << 31, (1 << 31) - 1) < 1 << 31
    for n, B, W in ((100, 32, 1), (100, 32, 2), (96, 32, 4), (5, 7, 1), (5, 8, 2)):
        assert epoch_order_len(n, B, W) == len(R.rank_positions(n, B, 0, W))


def test_header_names_the_rule():
    """3. the functions of the rule, built from kgwfan_step and kgwfan_mix32 with no constant of their own, ahead of the dropout's."""
    hdr = open(os.path.join(ROOT, 'include', 'kgwas_hip.h')).read()
    for name in ('kgwperm_base', 'kgwperm_half_bits', 'kgwperm_feistel', 'kgwperm_index', 'KGW_ORDER_SEEDS', 'KGW_ORDER_BATCHES',
                 'order_word(seed, epoch)'):
        assert name in hdr, name
    a, b = hdr.index('uint32_t kgwperm_base('), hdr.index('int kgw_epoch_order(')
    assert hdr.index('int kgw_sample_batch_fanout(') < a < b < hdr.index('uint32_t kgwdrop_base(')
    body = hdr[a:b]
    assert 'kgwfan_step(kgwfan_step(0u, (uint32_t)word), (uint32_t)(word >> 32))' in body
    assert 'kgwfan_mix32(kgwfan_step(base, r) ^ R) & mask' in body
    assert 'while ((int64_t)p >= n)' in body
    assert '0x' not in body and '0X' not in body                          # no constants of its own
    assert not re.search(r'\b\d{3,}', body)                               # ... in decimal either


def test_symbol_is_declared_exported_and_documented():
    """4."""
    from kgwas_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'kgwas_hip.h')).read()
    assert 'kgw_epoch_order' in _lib.EXPORTS and re.search(r'int\s+kgw_epoch_order\s*\(', hdr)
    assert '`kgw_epoch_order`' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert '#define KGW_VERSION      125' in hdr
    assert _lib.has_epoch_order() and _lib.lib().kgw_version() == 125
    assert (_lib.KGW_ORDER_SEEDS, _lib.KGW_ORDER_BATCHES) == tuple(
        int(re.search(r'#define %s\s+(\d+)' % n, hdr).group(1)) for n in ('KGW_ORDER_SEEDS', 'KGW_ORDER_BATCHES'))
    common = open(os.path.join(ROOT, 'kgwas_amd', 'csrc', 'kgw_common.h')).read()
    assert _lib.EPOCH_ORDER_BLOCK == int(re.search(r'KGW_BLK\s*=\s*(\d+)', common).group(1))
    assert _lib.EPOCH_ORDER_GRID == int(re.search(r'KGW_GRID\s*=\s*(\d+)', common).group(1))


def test_order_of_the_benchmark_is_far_from_the_genome_order():
    """5. n = 489 839: |corr(order, identity)| < 0.02, two epochs agree in fewer than n / 1000 positions; a batch of 512 draws from
    hundreds of the 956 genome windows."""
    n = N_BENCH
    a, b = R.permutation(R.order_word(0, 0), n), R.permutation(R.order_word(0, 1), n)
    corr = float(np.corrcoef(a, np.arange(n))[0, 1])
    same = int((a == b).sum())
    windows = len(np.unique(a[:512] // 512))
    print(f'corr {corr:.4f}, positions shared by two epochs {same}, windows in batch 0: {windows}')
    assert abs(corr) < 0.02
    assert same < n / 1000
    assert windows > 300


@pytest.mark.parametrize('W', [2, 4])
def test_ranks_partition_every_global_batch(W):
    """6. both modes: the ranks' slices, batch by batch, are exactly the global batch of the one-rank order, in rank order."""
    rng = np.random.default_rng(W)
    for n, B in ((1000, 64), (1024, 64), (517, 32), (40, 64)):
        ids = rng.permutation(10 * n)[:n]
        for mode in ('seeds', 'batches'):
            w = R.order_word(3, 1)
            whole = R.epoch_order(ids, B, mode, w)
            nb, per = n // B, B // W
            parts = [R.epoch_order(ids, B, mode, w, r, W) for r in range(W)]
            assert all(len(p) == nb * per for p in parts)
            for i in range(nb):
                got = np.concatenate([p[i * per:(i + 1) * per] for p in parts])
                assert np.array_equal(got, whole[i * B:(i + 1) * B]), (n, B, mode, i)
            assert len(whole) == n and np.array_equal(np.sort(whole), np.sort(ids))
            if mode == 'batches' and nb:
                assert np.array_equal(whole[nb * B:], ids[nb * B:])
                assert {tuple(whole[i * B:(i + 1) * B]) for i in range(nb)} == {tuple(ids[i * B:(i + 1) * B]) for i in range(nb)}


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path_factory.mktemp('shuf')))


def test_refusals(tiny):
    """7. a value of shuffle that is none of the three, a shuffle in the SNP-sharded mode, and the loader's shuffle=True."""
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    run = KGWAS(tiny, device='cpu', seed=1)
    run.initialize_model()
    for bad in ('x', 'seeds', 1, 0, None, 2.0):
        with pytest.raises(ValueError):
            run.train(epoch=1, shuffle=bad)
    for s in (True, 'batches'):
        with pytest.raises(NotImplementedError):
            run.train(epoch=1, parallelism='shard', shuffle=s)
    with pytest.raises(NotImplementedError, match='epoch_order'):
        NeighborLoader(tiny.data, [-1, -1], ('SNP', np.arange(8)), batch_size=4, shuffle=True)
    with pytest.raises(ValueError):
        NeighborLoader(tiny.data, [-1, -1], ('SNP', np.arange(8)), batch_size=4, epoch_order='random')
