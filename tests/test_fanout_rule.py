"""CPU: the finite fan-out rule itself (tests/fanout_ref.py, the numpy twin of include/kgwas_hip.h): it draws min(deg, k)
distinct positions in ascending order, and it is uniform to within a derived binomial bound."""
import os
import re

import numpy as np
import pytest

from tests import fanout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('k', [1, 10, 128])
def test_twin_draws_min_deg_k_distinct_ascending_positions(k):
    for deg in sorted({0, 1, max(k - 1, 0), k, k + 1, 127, 128, 129, 5_000, 75_000}):
        for word in (0, R.sample_word(0, 0, 0), R.sample_word(42, 3, 17)):
            p = R.draw(word, 2, 1234, deg, k)
            assert len(p) == min(deg, k), (deg, k)
            assert np.all(np.diff(p) > 0), (deg, k)                   # distinct and ascending
            assert len(p) == 0 or (p[0] >= 0 and p[-1] < deg)
            if deg > k:
                key = R.keys(word, 2, 1234, deg)
                rest = np.setdiff1d(np.arange(deg), p)
                assert key[p].max() <= key[rest].min()                # the k smallest keys
            assert np.array_equal(R.draw(word, 2, 1234, deg, -1), np.arange(deg))


def test_rule_is_uniform_within_the_binomial_bound():
    """Row of d = 40 entries, k = 10, N = 20 000 sample seeds: every entry's inclusion count is Binomial(N, p = k / d) under a
    uniform rule, so it lies within 5 sqrt(N p (1 - p)) of N p (5 sigma: ~6e-7 per entry for a sound mixer)."""
    d, k, N = 40, 10, 20_000
    p = k / d
    counts = np.zeros(d, dtype=np.int64)
    for n in range(N):
        counts[R.draw(R.sample_word(7, n // 100, n % 100), 5, 4321, d, k)] += 1
    bound = 5.0 * np.sqrt(N * p * (1 - p))
    dev = np.abs(counts - N * p)
    print(f'inclusion counts: min {counts.min()} max {counts.max()} expected {N * p:.0f}; largest deviation {dev.max():.1f}, bound {bound:.1f}')
    assert counts.sum() == N * k
    assert np.all(dev <= bound), (counts.tolist(), bound)


def test_rows_and_relations_draw_independently_of_each_other():
    """The key takes the relation and the destination in: two rows of one length do not keep the same positions."""
    w = R.sample_word(0, 0, 0)
    a = R.draw(w, 0, 10, 1000, 10)
    assert not np.array_equal(a, R.draw(w, 0, 11, 1000, 10))
    assert not np.array_equal(a, R.draw(w, 1, 10, 1000, 10))
    assert not np.array_equal(a, R.draw(R.sample_word(0, 1, 0), 0, 10, 1000, 10))
    assert np.array_equal(a, R.draw(w, 0, 10, 1000, 10))


def test_header_states_the_constants_the_twin_uses():
    hdr = open(os.path.join(ROOT, 'include', 'kgwas_hip.h')).read()
    body = hdr[hdr.index('kgwfan_mix32(uint32_t h)'):]
    for c in ('0x85ebca6bu', '0xc2b2ae35u', '0x9e3779b9u'):
        assert c in body
    assert re.search(r'int\s+kgw_sample_batch_fanout\s*\(', hdr)


def test_package_sample_word_equals_the_twin():
    from kgwas_amd.sampler import check_num_neighbors, fanout_sample_word
    for s, e, b in ((0, 0, 0), (42, 1, 7), (2 ** 63 + 5, 123456, 99999)):
        assert fanout_sample_word(s, e, b) == R.sample_word(s, e, b)
    assert check_num_neighbors([-1, -1]) is None and check_num_neighbors([10, -1]) == [10, -1]
    with pytest.raises(NotImplementedError):
        check_num_neighbors({('SNP', 'a', 'Gene'): [1, 1]})
    for bad in ([0, 1], [-2, 1]):
        with pytest.raises(ValueError):
            check_num_neighbors(bad)
