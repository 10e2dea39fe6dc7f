"""Twin of the weight-gradient product family C = A^T B over tall inputs (kgwas_amd/csrc/kgw_dense_tn.h): no GPU, no library.

plan()       restates tn_gemm_ex's tiling choice and launch_tn_jobs' row-block planner: the tiling <MT, NT> from parity, width and
             pointer alignment; gy x gz tiles of 32 MT x 32 NT; nblk = ceil(rows / 256) capped at 512 / (gy gz) (at least 1; 1 when
             the direct path is on, rows <= direct_rows and gy gz >= 16); rpw = ceil(rows / (4 nblk)) rounded up to even; wavefront
             w of the 4 nblk takes rows [min(rows, w rpw), min(rows, w rpw + rpw)).  The <2,2> tiling runs on the bf16 pipe when the
             split is on and lda, ldb are even: 16-row steps, the accumulator and the sign of A flip after every 4th step that has a
             successor, a masked tail of < 16 rows.  The fp32 pipe takes 8-row stages and a masked tail of < 8 rows.
plan_dev()   the device-side re-split for a row count read from memory: rows_eff = min(rows, max(rows_dev, 0)),
             rpw = (ceil(rows_eff / (4 nblk)) + 1) & ~1, nblk and the workspace layout unchanged.
Workspace    nblk gy gz FRAG floats of product slabs (FRAG = 1024 MT NT, slab ((bz gy + by) nblk + bx)), then nblk gy 32 MT floats
             of column-sum slabs ((by nblk + bx) 32 MT + c) at cs_off = nblk gy gz FRAG -- needed whether or not column sums are asked.
frag_index() the fragment -> (m, n) map of a slab: element f = ((ta NT + tb) 16 + e) 64 + lane holds
             ti = (e & 3) + 8 (e >> 2) + 4 (lane >> 5), tj = lane & 31, m = m0 + MT ti + ta, n = n0 + NT tj + tb.
reduce_in_kernel_order(), reduce_colsum_in_kernel_order()
             k_tn_reduce's order of fp32 additions: product record g + 4 j of group g goes to accumulator j mod 8, then
             ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)), then (g0+g1)+(g2+g3); column sums: NG = 256 / (32 MT) groups, record gq + NG j to
             accumulator j mod 4, (s0+s1)+(s2+s3), then the NG group sums in index order starting from 0.

Error bars.  On the fp32 pipe (every tiling but <2,2>, and <2,2> with kgw_tn_split(0)) an element of C is an exact-product FMA chain
over the wavefront's rows (mfma_f32_32x32x2f32: two rows per instruction, rpw fused multiply-adds in a chain), then fp32 additions:
2 in LDS ((w0+w2)+(w1+w3)), and in k_tn_reduce a chain of ceil(ceil(nblk / 4) / 8) into one of the eight accumulators, 3 to fold the
eight, 2 to fold the four groups.  Every term of the sum passes through at most
    depth = rpw + 2 + ceil(ceil(nblk / 4) / 8) + 3 + 2
roundings, each of relative size <= 2^-24 of a partial sum that is itself <= S = sum |a||b| (1 + small), so to first order
|got - ref| <= depth 2^-24 S; the bar is (depth + 2) 2^-24 S, the + 2 covering the second-order terms (depth 2^-24 < 2^-13 here) and
the reference's own float64 rounding.  It holds for ANY order of the same additions, so it does not lean on the order being right.  A
dropped or doubled row moves an element by ~ S / rows, hundreds of times the bar at these shapes.  S == 0: exactly 0.0.
The column sums are plain fp32 additions: a lane adds every second row of its wavefront's range (rpw / 2), + 1 for the two lane
halves, + 2 in LDS, then ceil(ceil(nblk / NG) / 4) + 2 + NG in the reduce: depth_cs, over sum |a|, same form.
The bf16 pipe's bars are the project's own (tests/test_gpu_dense.py): not derived here.

Generators: wide = randn 2^randint(-4, 4); positive = rand in (0, 1); integer = integers in [-8, 8] with A[:, 0] += 3 and
B[:, -1] -= 2 (|a| <= 11, |b| <= 10: every partial sum is an integer of magnitude <= 110 rows < 2^24 for rows <= 152 520, exact in
fp32 in any order, and every value is its own first bf16 piece); row-stamp = A all ones, B[r, n] = r mod 7 + 1."""
import collections

import torch

U = 2.0 ** -24
CAP_BLOCKS = 512                       # launch_tn_jobs: cap_small, taken by every tiling (MT NT <= 4)
ROWS_PER_BLOCK = 256                   # at least 64 rows per wavefront, 4 wavefronts per block
TN3_FLIP = 4
TILINGS = [(2, 2), (2, 1), (1, 4), (1, 2), (1, 1)]

Plan = collections.namedtuple('Plan', 'MT NT gy gz cap nblk rows rpw FRAG need cs_off waves bf16 steps flips tails depth depth_cs')


def tiling(M, N, lda, ldb, a_align=0, b_align=0):
    """tn_gemm_ex's choice; a_align / b_align: the operand's address modulo 16."""
    a2 = M % 2 == 0 and lda % 2 == 0 and a_align % 8 == 0 and M >= 64
    b2 = N % 2 == 0 and ldb % 2 == 0 and b_align % 8 == 0 and N >= 64
    b4 = N % 4 == 0 and ldb % 4 == 0 and b_align % 16 == 0 and N >= 128
    if a2 and b2:
        return 2, 2
    if a2:
        return 2, 1
    if b4:
        return 1, 4
    if b2:
        return 1, 2
    return 1, 1


def _cdiv(a, b):
    return -(-a // b)


def _waves(rows, nblk, rpw, bf16):
    waves, steps, flips, tails = [], [], [], []
    step = 16 if bf16 else 8
    for w in range(4 * nblk):
        r0 = min(rows, w * rpw)
        r1 = min(rows, r0 + rpw)
        n = r1 - r0
        waves.append((r0, r1))
        steps.append(n // step)
        tails.append(n % step)
        flips.append((n // 16 - 1) // TN3_FLIP if bf16 and n >= 16 else 0)
    return waves, steps, flips, tails


def _finish_plan(MT, NT, gy, gz, cap, nblk, rows, rpw, bf16):
    FRAG = MT * NT * 1024
    waves, steps, flips, tails = _waves(rows, nblk, rpw, bf16)
    NG = 256 // (32 * MT)
    depth = rpw + 2 + _cdiv(_cdiv(nblk, 4), 8) + 3 + 2
    depth_cs = rpw // 2 + 1 + 2 + _cdiv(_cdiv(nblk, NG), 4) + 2 + NG
    return Plan(MT, NT, gy, gz, cap, nblk, rows, rpw, FRAG, nblk * gy * gz * FRAG + nblk * gy * 32 * MT, nblk * gy * gz * FRAG,
                waves, bf16, steps, flips, tails, depth, depth_cs)


def plan(rows, M, N, lda=None, ldb=None, a_align=0, b_align=0, split=True, direct_rows=0, forced=None):
    """forced = (2, 2): the grouped forms (kgw_tn_gemm_multi, kgw_transform_bwd_ex), which run every job on that tiling."""
    lda = M if lda is None else lda
    ldb = N if ldb is None else ldb
    MT, NT = forced or tiling(M, N, lda, ldb, a_align, b_align)
    gy, gz = _cdiv(M, 32 * MT), _cdiv(N, 32 * NT)
    nblk = _cdiv(rows, ROWS_PER_BLOCK)
    cap = CAP_BLOCKS // (gy * gz)
    nblk = max(min(nblk, max(cap, 1)), 1)
    if rows <= direct_rows and gy * gz >= 16:
        nblk = 1
    rpw = (_cdiv(rows, nblk * 4) + 1) & ~1
    bf16 = (MT, NT) == (2, 2) and bool(split) and lda % 2 == 0 and ldb % 2 == 0
    return _finish_plan(MT, NT, gy, gz, cap, nblk, rows, rpw, bf16)


def plan_dev(p, rows_dev):
    re = min(p.rows, max(rows_dev, 0))
    rpw = (_cdiv(re, p.nblk * 4) + 1) & ~1
    return _finish_plan(p.MT, p.NT, p.gy, p.gz, p.cap, p.nblk, re, rpw, p.bf16)


def block_rows(p, bx):
    """Rows [r0, r1) of row block bx (its four wavefronts' ranges are adjacent)."""
    return p.waves[4 * bx][0], p.waves[4 * bx + 3][1]


def workspace_floats_bound(rows, M, N):
    """kgw_tn_gemm_workspace_floats restated."""
    gy1, gz1 = 4 * _cdiv(M, 128), 4 * _cdiv(N, 128)
    nblk = max(min(_cdiv(rows, 256), 1024), 1)
    return nblk * gy1 * gz1 * 1024 + nblk * gy1 * 32 + 4096


# ------------------------------------------------------ fragment map ---------------------------------------------------------

def frag_mn(p, by, bz):
    """(m, n) of every element f of the slab of tile (by, bz), two int64 tensors of FRAG."""
    f = torch.arange(p.FRAG)
    lane, e, t = f & 63, (f >> 6) & 15, f >> 10
    tb, ta = t % p.NT, t // p.NT
    ti = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
    tj = lane & 31
    return by * 32 * p.MT + p.MT * ti + ta, bz * 32 * p.NT + p.NT * tj + tb


def frag_index(p, M, N):
    """idx [M, N] int64: the offset of C[m][n] inside row block 0's part of the product workspace; row block bx adds bx FRAG."""
    idx = torch.full((M, N), -1, dtype=torch.int64)
    for bz in range(p.gz):
        for by in range(p.gy):
            m, n = frag_mn(p, by, bz)
            ok = (m < M) & (n < N)
            off = (bz * p.gy + by) * p.nblk * p.FRAG + torch.arange(p.FRAG)
            assert bool((idx[m[ok], n[ok]] == -1).all())
            idx[m[ok], n[ok]] = off[ok]
    assert bool((idx >= 0).all())
    return idx


def slabs_of(ws, p, M, N):
    """The workspace's product slabs as [nblk, M, N] and its column-sum slabs as [nblk, M] (ws: at least p.need floats)."""
    idx = frag_index(p, M, N).to(ws.device)
    bx = torch.arange(p.nblk, device=ws.device).view(-1, 1, 1) * p.FRAG
    prod = ws[(idx.unsqueeze(0) + bx).reshape(-1)].view(p.nblk, M, N)
    NC = 32 * p.MT
    cs = ws[p.cs_off:p.cs_off + p.nblk * p.gy * NC].view(p.gy, p.nblk, NC).permute(1, 0, 2).reshape(p.nblk, p.gy * NC)[:, :M]
    return prod, cs


# ------------------------------------------------------ k_tn_reduce's order --------------------------------------------------

def _strided_sum(slabs, first, stride, n_acc):
    acc = [torch.zeros_like(slabs[0]) for _ in range(n_acc)]
    for j, b in enumerate(range(first, slabs.shape[0], stride)):
        acc[j % n_acc] = acc[j % n_acc] + slabs[b]
    return acc


def reduce_in_kernel_order(slabs):
    """slabs: fp32 [nblk, ...] -> their sum in k_tn_reduce's order for the product."""
    assert slabs.dtype == torch.float32
    g = []
    for q in range(4):
        s = _strided_sum(slabs, q, 4, 8)
        g.append(((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7])))
    return (g[0] + g[1]) + (g[2] + g[3])


def reduce_colsum_in_kernel_order(slabs, MT):
    assert slabs.dtype == torch.float32
    NG = 256 // (32 * MT)
    t = torch.zeros_like(slabs[0])
    for gq in range(NG):
        s = _strided_sum(slabs, gq, NG, 4)
        t = t + ((s[0] + s[1]) + (s[2] + s[3]))
    return t


# ------------------------------------------------------ float64 reference ----------------------------------------------------

Ref = collections.namedtuple('Ref', 'C S cs sa')


def ref64(A, B, r0=0, r1=None):
    """C = A^T B, S = |A|^T |B|, column sums of A and of |A| over rows [r0, r1), float64 on the CPU."""
    a, b = A[r0:r1].double().cpu(), B[r0:r1].double().cpu()
    return Ref(a.t() @ b, a.abs().t() @ b.abs(), a.sum(0), a.abs().sum(0))


def ref64_blocks(A, B, p):
    return [ref64(A, B, *block_rows(p, bx)) for bx in range(p.nblk)]


def err_in_u(got, ref, scale):
    """max |got - ref| / (2^-24 scale); where scale == 0 the element must be exactly 0.0; a non-finite `got` gives inf."""
    got, ref, scale = got.detach().double().cpu(), ref.double().cpu(), scale.double().cpu()
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    zero = scale == 0
    assert not bool((zero & ((got != 0) | (ref != 0))).any()), 'elements of scale 0 are not exactly 0.0'
    err = (got - ref).abs() / torch.where(zero, torch.ones_like(scale), scale)
    return float(torch.where(zero, torch.zeros_like(err), err).max()) / U


# ------------------------------------------------------ generators -----------------------------------------------------------

INT_MAX_A, INT_MAX_B = 11, 10


def gen(kind, rows, M, N, seed, device='cpu'):
    g = torch.Generator(device=device).manual_seed(seed)
    if kind == 'wide':
        A = torch.randn(rows, M, generator=g, device=device) * torch.exp2(torch.randint(-4, 5, (rows, M), generator=g, device=device).float())
        B = torch.randn(rows, N, generator=g, device=device) * torch.exp2(torch.randint(-4, 5, (rows, N), generator=g, device=device).float())
    elif kind == 'positive':
        A = torch.rand(rows, M, generator=g, device=device)
        B = torch.rand(rows, N, generator=g, device=device)
    elif kind == 'integer':
        A = torch.randint(-8, 9, (rows, M), generator=g, device=device).float()
        B = torch.randint(-8, 9, (rows, N), generator=g, device=device).float()
        A[:, 0] += 3.0
        B[:, -1] -= 2.0
    elif kind == 'stamp':
        A = torch.ones(rows, M, device=device)
        B = ((torch.arange(rows, device=device) % 7) + 1).float().view(-1, 1).expand(rows, N).contiguous()
    else:
        raise ValueError(kind)
    return A, B


# ------------------------------------------------------ the case table -------------------------------------------------------
# name -> (rows, M, N, direct_rows); tests/test_tn_gemm_ref.py asserts from plan() that each reaches the edge its name states.

CASES = collections.OrderedDict([
    ('one-row', (1, 128, 128, 0)), ('tail-only', (15, 128, 128, 0)), ('tail-only-63', (63, 128, 128, 0)),
    ('one-step', (17, 64, 64, 0)), ('last-single-block', (256, 128, 128, 0)),
    ('first-split', (257, 128, 128, 0)), ('ragged-last-wave', (513, 64, 66, 0)),
    ('nblk5', (1025, 128, 128, 0)), ('nblk6', (1281, 128, 128, 0)), ('nblk9', (2049, 128, 128, 0)),
    ('nblk29', (7169, 128, 128, 0)), ('nblk30', (7425, 128, 128, 0)), ('nblk33', (8193, 128, 128, 0)),
    ('nblk34', (8449, 128, 128, 0)), ('nblk65', (16385, 128, 128, 0)), ('nblk66', (16641, 128, 128, 0)),
    ('cs-nblk25', (6145, 6, 128, 0)), ('cs-nblk26', (6401, 6, 128, 0)), ('cs-nblk33', (8193, 6, 128, 0)), ('cs-nblk34', (8449, 6, 128, 0)),
    ('t21-nblk13', (3073, 128, 20, 0)), ('t21-nblk14', (3329, 128, 20, 0)),
    ('t12', (4097, 6, 66, 0)), ('t11', (2000, 5, 7, 0)), ('t11-two-by', (9, 33, 31, 0)),
    ('ragged-mn', (700, 66, 130, 0)),
    ('cap-rpw80', (3520, 128, 1408, 0)), ('cap-empty-wave', (3521, 128, 1408, 0)), ('cap-ragged', (2817, 128, 1408, 0)),
    ('cap-below-1', (340, 128, 16448, 0)),
    ('layer-transform', (1171, 128, 2176, 0)),
    ('direct-transform', (1171, 128, 2176, 2048)), ('direct-16-tiles', (100, 256, 256, 2048)),
    ('direct-16-tiles-300', (300, 256, 256, 2048)), ('direct-15-tiles-not', (300, 320, 192, 2048)),
])


def case_plan(name, split=True):
    rows, M, N, direct = CASES[name]
    return plan(rows, M, N, split=split, direct_rows=direct)
