"""tests/tn_gemm_ref.py held to its own claims, on the CPU: the plan twin partitions the rows, its workspace need stays under
kgw_tn_gemm_workspace_floats' formula, every named edge of the case table is reached (asserted from the plan), the integer
generator stays exact in fp32, and reduce_in_kernel_order is a sum that depends on its order."""
import itertools

import pytest
import torch

from tests import tn_gemm_ref as T


def _all_plans():
    for name in T.CASES:
        for split in (True, False):
            yield name, T.case_plan(name, split)


@pytest.mark.parametrize('name', list(T.CASES))
def test_every_row_belongs_to_exactly_one_wavefront_and_ranges_start_even(name):
    rows = T.CASES[name][0]
    for split in (True, False):
        p = T.case_plan(name, split)
        for rd in [rows, 0, 1, 255, 257, rows - 1]:
            q = T.plan_dev(p, rd)
            assert len(q.waves) == 4 * q.nblk
            end = 0
            for (r0, r1), st, tl in zip(q.waves, q.steps, q.tails):
                assert r0 == end and r1 >= r0 and (r0 % 2 == 0 or r0 == q.rows)
                assert st * (16 if q.bf16 else 8) + tl == r1 - r0
                end = r1
            assert end == q.rows == min(rows, max(rd, 0))
        assert T.plan_dev(p, rows).waves == p.waves and T.plan_dev(p, rows + 100).waves == p.waves
        assert T.plan_dev(p, -3).rows == 0 and T.plan_dev(p, 0).rpw == 0


def test_workspace_need_is_within_the_library_bound():
    rows_s = [1, 2, 255, 256, 257, 1000, 5000, 70000, 300000, 2 * 10 ** 6]
    mn = [1, 2, 5, 31, 32, 33, 62, 64, 66, 127, 128, 130, 256, 2176]
    for rows, M, N in itertools.product(rows_s, mn, mn):
        bound = T.workspace_floats_bound(rows, M, N)
        for forced in [None] + T.TILINGS:
            for direct in (0, 2048):
                p = T.plan(rows, M, N, direct_rows=direct, forced=forced)
                assert p.need <= bound, (rows, M, N, forced, direct, p.need, bound)
                assert p.need == p.cs_off + p.nblk * p.gy * 32 * p.MT and p.cs_off == p.nblk * p.gy * p.gz * p.FRAG


def test_tiling_choice():
    assert T.tiling(128, 128, 128, 128) == (2, 2)
    assert T.tiling(128, 20, 128, 20) == (2, 1)
    assert T.tiling(6, 128, 6, 128) == (1, 4)
    assert T.tiling(6, 66, 6, 66) == (1, 2)
    assert T.tiling(5, 7, 5, 7) == (1, 1) and T.tiling(33, 31, 33, 31) == (1, 1)
    assert T.tiling(128, 128, 129, 128) == (1, 4) and T.tiling(128, 128, 128, 128, a_align=4) == (1, 4)
    assert T.tiling(128, 128, 128, 130) == (2, 2) and T.tiling(128, 128, 128, 129) == (2, 1)
    assert T.tiling(6, 128, 6, 128, b_align=8) == (1, 2) and T.tiling(128, 128, 129, 129) == (1, 1)
    assert T.tiling(62, 62, 62, 62) == (1, 1) and T.tiling(64, 64, 64, 64) == (2, 2)


def _main_loop_groups(nblk, n_groups, unroll):
    return [g for g in range(n_groups) if g + (unroll - 1) * n_groups < nblk]


def _tail_groups(nblk, n_groups, unroll):
    """groups whose tail loop adds at least one record"""
    out = []
    for g in range(n_groups):
        b = g
        while b + (unroll - 1) * n_groups < nblk:
            b += unroll * n_groups
        if b < nblk:
            out.append(g)
    return out


def test_every_named_edge_is_reached():
    P = {name: T.case_plan(name) for name in T.CASES}
    p = P['one-row']
    assert (p.MT, p.NT, p.nblk, p.bf16) == (2, 2, 1, True) and p.waves == [(0, 1), (1, 1), (1, 1), (1, 1)] and p.tails[0] == 1
    p = P['tail-only']
    assert p.nblk == 1 and p.steps == [0, 0, 0, 0] and p.tails == [4, 4, 4, 3]
    p = P['tail-only-63']
    assert p.nblk == 1 and p.steps == [1, 1, 1, 0] and p.tails == [0, 0, 0, 15] and p.flips == [0] * 4
    p = P['one-step']
    assert (p.MT, p.NT, p.nblk) == (2, 2, 1) and p.waves == [(0, 6), (6, 12), (12, 17), (17, 17)]
    p = P['last-single-block']
    assert p.nblk == 1 and p.rpw == 64 and p.steps == [4] * 4 and p.tails == [0] * 4 and p.flips == [0] * 4
    assert T.plan(257, 128, 128).nblk == 2
    p = P['first-split']
    assert p.nblk == 2 and p.rpw == 34 and p.waves[-1] == (238, 257)
    p = P['ragged-last-wave']
    assert (p.MT, p.NT, p.gy, p.gz, p.nblk, p.rpw) == (2, 2, 1, 2, 3, 44) and p.waves[-1] == (484, 513)
    for n in (5, 6, 9, 29, 30, 33, 34, 65, 66):
        p = P[f'nblk{n}']
        assert (p.MT, p.NT, p.gy, p.gz, p.nblk) == (2, 2, 2, 2, n) and p.nblk < p.cap
    # k_tn_reduce, product: 4 groups, 8 ways
    assert [_main_loop_groups(n, 4, 8) for n in (5, 6, 9, 29, 30)] == [[], [], [], [0], [0, 1]]
    assert _tail_groups(29, 4, 8) == [1, 2, 3] and _tail_groups(30, 4, 8) == [2, 3]
    for n in (33, 34, 65, 66):
        assert _main_loop_groups(n, 4, 8) == [0, 1, 2, 3]
    assert _tail_groups(33, 4, 8) == [0] and _tail_groups(34, 4, 8) == [0, 1] and _tail_groups(65, 4, 8) == [0] and _tail_groups(66, 4, 8) == [0, 1]
    # ... column sums on <1,4>: 8 groups, 4 ways
    for n in (25, 26, 33, 34):
        p = P[f'cs-nblk{n}']
        assert (p.MT, p.NT, p.gy, p.gz, p.nblk) == (1, 4, 1, 1, n) and 256 // (32 * p.MT) == 8
    assert [_main_loop_groups(n, 8, 4) for n in (25, 26)] == [[0], [0, 1]]
    assert _main_loop_groups(33, 8, 4) == list(range(8)) and _tail_groups(33, 8, 4) == [0] and _tail_groups(34, 8, 4) == [0, 1]
    assert [(P[k].MT, P[k].NT, P[k].nblk) for k in ('t21-nblk13', 't21-nblk14')] == [(2, 1, 13), (2, 1, 14)]
    assert (P['t12'].MT, P['t12'].NT, P['t12'].gz, P['t12'].nblk) == (1, 2, 2, 17)
    assert (P['t11'].MT, P['t11'].NT, P['t11'].nblk) == (1, 1, 8)
    p = P['t11-two-by']
    assert (p.MT, p.NT, p.gy, p.gz, p.nblk) == (1, 1, 2, 1, 1) and 33 - 32 * (p.gy - 1) == 1
    p = P['ragged-mn']
    assert (p.MT, p.NT, p.gy, p.gz) == (2, 2, 2, 3) and 66 - 64 * (p.gy - 1) == 2 and 130 - 64 * (p.gz - 1) == 2
    p = P['cap-rpw80']
    assert (p.cap, p.nblk, p.rpw) == (11, 11, 80) and T._cdiv(3520, 256) > p.cap
    assert p.steps == [5] * 44 and p.flips == [1] * 44 and p.tails == [0] * 44
    p = P['cap-empty-wave']
    assert (p.cap, p.nblk, p.rpw) == (11, 11, 82) and p.waves[-1] == (3521, 3521) and p.waves[-2] == (3444, 3521)
    p = P['cap-ragged']
    assert (p.cap, p.nblk, p.rpw) == (11, 11, 66) and T._cdiv(2817, 256) > p.cap and p.waves[-2] == (2772, 2817) and p.waves[-1] == (2817, 2817)
    p = P['cap-below-1']
    assert p.cap == 0 and p.nblk == 1 and p.gz == 257 and p.flips[0] == 1 and p.rpw == 86
    p = P['layer-transform']
    assert (p.gy, p.gz, p.cap, p.nblk, p.rpw) == (2, 34, 7, 5, 60)
    p = P['direct-transform']
    assert (p.nblk, p.rpw) == (1, 294) and p.flips == [4, 4, 4, 4] and p.steps[0] == 18
    p = P['direct-16-tiles']
    assert p.gy * p.gz == 16 and p.nblk == 1
    p = P['direct-16-tiles-300']
    assert p.gy * p.gz == 16 and p.nblk == 1 and T.plan(300, 256, 256).nblk == 2
    p = P['direct-15-tiles-not']
    assert p.gy * p.gz == 15 and p.nblk == 2
    assert max(c[0] for c in T.CASES.values()) == 16641                   # the largest operand of the table: 16 641 x 128


def test_integer_generator_stays_exact_in_fp32():
    for rows, M, N in [(16641, 128, 128), (3521, 128, 64), (9, 33, 31)]:
        A, B = T.gen('integer', rows, M, N, 3)
        assert float(A.abs().max()) <= T.INT_MAX_A and float(B.abs().max()) <= T.INT_MAX_B
        assert torch.equal(A, A.round()) and torch.equal(A.to(torch.bfloat16).float(), A) and torch.equal(B.to(torch.bfloat16).float(), B)
        r = T.ref64(A, B)
        assert float(r.S.max()) < 2 ** 24 and float(r.sa.max()) < 2 ** 24
        assert float(A[:, 0].mean()) > 2 and float(B[:, -1].mean()) < -1                   # the asymmetry is there
    assert T.INT_MAX_A * T.INT_MAX_B * max(c[0] for c in T.CASES.values()) < 2 ** 24
    A, B = T.gen('stamp', 3521, 4, 4, 0)
    assert float(T.ref64(A, B).S.max()) < 2 ** 24 and B[8, 0] == 2 and B[6, 3] == 7 and bool((A == 1).all())


@pytest.mark.parametrize('nblk', [2, 5, 9, 29, 33, 66])
def test_reduce_in_kernel_order_is_a_sum_and_depends_on_its_order(nblk):
    g = torch.Generator().manual_seed(nblk)
    s = torch.randn(nblk, 64, 96, generator=g) * torch.exp2(torch.randint(-4, 5, (nblk, 64, 96), generator=g).float())
    ref, mag = s.double().sum(0), s.double().abs().sum(0)
    got = T.reduce_in_kernel_order(s)
    assert got.dtype == torch.float32
    assert T.err_in_u(got, ref, mag) <= nblk + 2
    for MT in (1, 2):
        c = T.reduce_colsum_in_kernel_order(s, MT)
        assert T.err_in_u(c, ref, mag) <= nblk + 2
    if nblk >= 5:
        assert not torch.equal(got, s.sum(0)) or not torch.equal(got, s.flip(0).sum(0))
        seq = torch.zeros_like(s[0])
        for b in range(nblk):
            seq = seq + s[b]
        assert not torch.equal(got, seq), 'the order of additions does not show in the bits'
    # integers: any order gives the same
    si = torch.randint(-100, 101, (nblk, 7, 5), generator=g).float()
    assert torch.equal(T.reduce_in_kernel_order(si), si.sum(0)) and torch.equal(T.reduce_colsum_in_kernel_order(si, 1), si.sum(0))


@pytest.mark.parametrize('MT,NT', T.TILINGS)
def test_fragment_map_is_a_bijection(MT, NT):
    M, N = 32 * MT + 3 * MT, 32 * NT + NT
    p = T.plan(600, M, N, forced=(MT, NT))
    idx = T.frag_index(p, M, N)
    assert idx.unique().numel() == M * N and int(idx.max()) < p.cs_off
    m, n = T.frag_mn(p, 0, 0)
    assert torch.unique(m * 32 * NT + n).numel() == p.FRAG and int(m.max()) == 32 * MT - 1 and int(n.max()) == 32 * NT - 1
    ws = torch.arange(p.need, dtype=torch.float32)
    prod, cs = T.slabs_of(ws, p, M, N)
    assert prod.shape == (p.nblk, M, N) and cs.shape == (p.nblk, M)
    assert torch.equal(prod[1] - prod[0], torch.full((M, N), float(p.FRAG)))
    assert float(cs[0, 0]) == p.cs_off and float(cs[1, 0]) == p.cs_off + 32 * MT and float(cs[0, 32 * MT]) == p.cs_off + p.nblk * 32 * MT
