"""The fused two-layer MLP kernels (kgwas_amd/csrc/kgw_dense_linear.h: k_mlp2_fwd3 / k_mlp2_fwd, k_mlp2w_fwd,
k_mlp2_bwd_first3<PACK> / k_mlp2_bwd_first, k_mlp2_bwd_fold) called at their C ABI and compared with plain float64
(tests/mlp2_ref.py) at every tile, block and grid-cap edge, in every argument variant.

Inputs have a wide dynamic range (randn * 2^randint, as tests/test_gpu_gemm3.py) so that all three bf16 pieces of the split carry
signal; every error is relative to sum |a||b| of the element's own dot product; no element is left out of a comparison.  The bars:
  exact     gathers, masks (H1 is GIVEN at the C ABI: (dH2 W2) * (H1 > 0) is defined for every element, +-0.0 included), zero
            rows, sentinels behind every strided row, bit-identity between argument variants;
  derived   H1 of kgw_mlp2_fwd: an fp32 multiply-add chain over K1 + 1 terms is within (K1 + 2) 2^-24 sum |a||b| of the exact
            value (and ReLU is 1-Lipschitz, so a pre-activation that rounds across zero is covered);
  project   every 128-term product: the two assertions of test_gemm3_matches_float64_as_well_as_fp32 -- no worse than
            1.25 x the fp32 device pipeline of the same operands (or 4 u), and never above 16 u --, the first with a factor for
            the summation order (see ORDER), both for dW1 / db1 on the scale of the whole dot product (see _check_bwd), the second for the
            fp32-pipe variants at the ceiling of an fp32 chain (see _chain_ceiling);
            the one-sided-error bars of test_tn_gemm_on_the_bf16_pipe_has_no_one_sided_error.
KGW_MLP2_SPLIT=0 selects the fp32-pipe kernels; the library reads it once, so test_fp32_pipe_variants_hold_the_same_bars runs
this module again in a child process under it."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mlp2_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT = os.environ.get('KGW_MLP2_SPLIT', '')[:1] != '0'          # (the library's own test of the switch)
OK, E_NULL, E_RANGE, E_UNSUPPORTED = 0, -1, -2, -3
GRAD_DIRECT, GRAD_MLP2_W, GRAD_MLP2_B = 0, 3, 4                   # include/kgwas_hip.h: KGW_GRAD_*
U = R.U
SENT = -777.25                                                    # behind every strided row; must survive every call
MARK = 12345.5                                                    # in output elements a call must not write


def _L():
    from kgwas_amd import _lib
    return _lib.lib()


def _st():
    from kgwas_amd import _lib
    return _lib.stream_ptr()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _wide(g, shape, span):
    return torch.randn(shape, device='cuda', generator=g) * torch.exp2(
        torch.randint(-span, span + 1, shape, device='cuda', generator=g).float())


def _strided(M, ld):
    """A copy of M [rows, cols] with row stride ld, the sentinel behind every row."""
    rows, cols = M.shape
    buf = torch.full((rows, ld), SENT, device='cuda')
    buf[:, :cols] = M
    return buf


def _out(rows, cols, ld, fill=float('nan')):
    buf = torch.full((rows, ld), SENT, device='cuda')
    buf[:, :cols] = fill
    return buf


def _pad_ok(buf, cols):
    return bool((buf[:, cols:] == SENT).all())


# Two correct fp32 summation orders of one 128-term product do not have the same error.  Where one term dominates sum |a||b| (wide
# dynamic range: the usual case here), every rounding after that term has entered is up to u times the whole scale: at most 127 of
# them in ONE chain over k (what k_mlp2w_fwd and the fp32-pipe kernels are, two k per MFMA step), at most 7 + 15 + 1 = 23 when
# the sum is blocked 16 x 8 or 8 x 16 (a library GEMM, the yardstick).  Independent roundings add in quadrature, hence a factor
# sqrt(127 / 23) = 2.35 between the two orders; the project's own margin of 1.25 (two realisations of the SAME order,
# test_gemm3_matches_float64_as_well_as_fp32) stays on top of it.  Derived from the orders alone, not from a measured result; the
# figures that made it necessary are in profiles/mlp2_kernels/gputests.txt.
ORDER = (127.0 / 23.0) ** 0.5


# The 16 u ceiling is what the bf16-pipe products stay under (sixteen k per MFMA: few roundings at full magnitude), and it is asserted
# as it stands for them and for k_mlp2w_fwd.  The fp32-pipe variants of sections A and B (KGW_MLP2_SPLIT=0) are one chain: with a
# dominant first term, 127 roundings, each uniform within +-u of the scale (rms u / sqrt 3) -- a sum of rms sqrt(127 / 3) u =
# 6.5 u, whose largest of N values is expected at sqrt(2 ln 2N) times that: 28 u for 33 x 128 elements, 37 u for 65 825 x 128.
# The fp32 library product itself is above 16 u on these inputs from 4 097 rows on (16.3 u, 20.5 u at 32 769 rows).
def _chain_ceiling(numel):
    return (127.0 / 3.0) ** 0.5 * (2.0 * math.log(2.0 * numel)) ** 0.5 * U


def _bar(name, e3, e32, numel=None):
    """The project's bar for a 128-term product (tests/test_gpu_gemm3.py: within 1.25 x the fp32 device pipeline or 4 u, and never
    above 16 u), the first with the summation-order factor above; ``numel`` (sections A and B): the number of elements the
    maximum is over, for the ceiling of the fp32-pipe variants."""
    ceiling = 16 * U if SPLIT or numel is None else max(16 * U, _chain_ceiling(numel))
    print(f'[mlp2 {name}] e3 = {e3 / U:.3f} u, e32 = {e32 / U:.3f} u  (u = 2^-24, relative to sum |a||b|; ceiling {ceiling / U:.1f} u)')
    assert e3 <= max(1.25 * ORDER * e32, 4 * U), (name, e3, e32)
    assert e3 <= ceiling, (name, e3, ceiling)


# ====================================================== A. kgw_mlp2_fwd ======================================================

@functools.lru_cache(maxsize=None)
def _weights(K1):
    g = _gen(100 + K1)
    rs = torch.exp2(torch.randint(-10, 11, (128, 1), device='cuda', generator=g).float())     # the columns of H1 differ in magnitude
    W1 = _wide(g, (128, max(K1, 1)), 2)[:, :K1] * rs
    b1 = torch.randn(128, device='cuda', generator=g) * rs[:, 0]
    W2 = _wide(g, (128, 128), 8)
    W2[3] = W2[3].abs() * 32.0                    # one row and one column unlike the rest: a transposed or permuted operand cannot pass
    W2[:, 17] = -W2[:, 17].abs() / 32.0
    b2 = _wide(g, (128,), 4)
    return W1, b1, W2, b2


@functools.lru_cache(maxsize=4)
def _fwd_x(rows, K1):
    X = _wide(_gen(rows * 31 + K1), (rows, K1), 6)
    if rows > 2:
        X[rows // 2] = 0.0                        # (with b1 null: a row of H1 without a scale -- exactly zero)
    return X


FWD_LD = dict(ldx=24, ldw1=None, ldw2=132, ldh1=160, ldh2=136, ldxg=24)          # ldw1 None: K1 + 4


def _fwd(X, K1, W1, b1, W2, b2, rows, ld=FWD_LD, h1=True, rows_dev=None, ids=None, xg=False, expect=OK):
    ldw1 = ld['ldw1'] or K1 + 4
    Xs, W1s, W2s = _strided(X, ld['ldx']), _strided(W1, ldw1), _strided(W2, ld['ldw2'])
    H1 = _out(rows, 128, ld['ldh1']) if h1 else None
    H2 = _out(rows, 128, ld['ldh2'])
    Xg = _out(rows, K1, ld['ldxg']) if xg else None
    rd = None if rows_dev is None else torch.tensor([rows_dev], dtype=torch.int32, device='cuda')
    if rows_dev is not None:                      # padding rows of the static layout: NaN in every input
        n = max(0, min(rows_dev, rows))
        Xs[n:, :K1] = float('nan')
    rc = _L().kgw_mlp2_fwd(_p(Xs), ld['ldx'], K1, _p(W1s), ldw1, _p(b1), _p(W2s), ld['ldw2'], _p(b2), _p(H1), ld['ldh1'], _p(H2),
                           ld['ldh2'], rows, _p(rd), _p(ids), _p(Xg), ld['ldxg'], _st())
    assert rc == expect, rc
    assert _pad_ok(Xs, K1) and _pad_ok(W1s, K1) and _pad_ok(W2s, 128) and _pad_ok(H2, 128)
    assert (H1 is None or _pad_ok(H1, 128)) and (Xg is None or _pad_ok(Xg, K1))
    return (None if H1 is None else H1[:, :128]), H2[:, :128], (None if Xg is None else Xg[:, :K1])


def _check_fwd(name, X, K1, W1, b1, W2, b2, H1, H2):
    """H1 against float64 within the fp32 chain bound; H2 against float64 OF THE H1 THE KERNEL WROTE within the project's bar."""
    if X.shape[0] == 0:
        return
    z1, h1, s1 = R.ref_fwd(X, W1, b1, W2, b2)[:3]
    e1 = R.rel_err(H1, h1, s1)
    print(f'[mlp2 {name}] H1: {e1 / U:.3f} u of a bound of {K1 + 2} u')
    assert e1 <= (K1 + 2) * U, (name, e1)
    z2, s2 = R.ref_second(H1, W2, b2)
    ref = torch.relu(z2)
    y32 = H1 @ W2.t()
    e32 = R.rel_err(torch.relu(y32 if b2 is None else y32 + b2), ref, s2)
    _bar(name + ' H2', R.rel_err(H2, ref, s2), e32, H2.numel())


FWD_ROWS = [1, 31, 32, 33, 255, 256, 257, 513, 65536, 65537, 65536 + 256 + 33]
FWD_CASES = [(r, 20) for r in FWD_ROWS] + [(r, k) for r in (33, 257) for k in (4, 8, 12, 16)]


@pytest.mark.parametrize('rows,K1', FWD_CASES)
def test_fwd_matches_float64(rows, K1):
    """One block is 256 rows (128 on the fp32 pipe), the grid is capped at 256 blocks x 8 wavefronts x 32 rows = 65 536: one row,
    both sides of a tile and of a block, the cap exactly, one past it, and wavefronts with a ragged second tile.  K1 moves the
    bias slot k4 == K1 between the two lane groups."""
    W1, b1, W2, b2 = _weights(K1)
    X = _fwd_x(rows, K1)
    H1, H2, _ = _fwd(X, K1, W1, b1, W2, b2, rows)
    _check_fwd(f'fwd rows={rows} K1={K1}', X, K1, W1, b1, W2, b2, H1, H2)
    assert bool((H1 >= 0).all()) and bool((H2 >= 0).all())


@pytest.mark.parametrize('K1', [24, 6])
def test_fwd_refuses_widths_it_has_no_lanes_for(K1):
    W1, b1, W2, b2 = _weights(K1)
    X = _fwd_x(33, K1)
    ld = dict(FWD_LD, ldx=32)
    H1, H2, _ = _fwd(X, K1, W1, b1, W2, b2, 33, ld=ld, expect=E_UNSUPPORTED)
    assert bool(torch.isnan(H1).all()) and bool(torch.isnan(H2).all())          # nothing was launched


@pytest.mark.parametrize('rows', [33, 257, 65537])
def test_fwd_argument_variants(rows):
    K1 = 20
    W1, b1, W2, b2 = _weights(K1)
    X = _fwd_x(rows, K1)
    H1, H2, _ = _fwd(X, K1, W1, b1, W2, b2, rows)
    # null biases
    for nb1, nb2 in ((None, b2), (b1, None), (None, None)):
        h1, h2, _ = _fwd(X, K1, W1, nb1, W2, nb2, rows)
        _check_fwd(f'fwd rows={rows} b1={"null" if nb1 is None else "set"} b2={"null" if nb2 is None else "set"}', X, K1, W1, nb1, W2,
                   nb2, h1, h2)
        if nb1 is None and rows > 2:
            assert not h1[rows // 2].any()                                       # the zero row of X: H1 is exactly zero there
    # H1 not wanted: the same H2
    _, h2, _ = _fwd(X, K1, W1, b1, W2, b2, rows, h1=False)
    assert torch.equal(h2, H2)
    # rows gathered by the kernel (ids with duplicates) + the gathered copy
    g = _gen(rows)
    nsrc = rows // 2 + 3
    Xsrc = _wide(g, (nsrc, K1), 6)
    ids = torch.randint(0, nsrc, (rows,), device='cuda', generator=g).to(torch.int32)
    ids[0] = nsrc - 1
    ids[rows - 1] = 0
    Xe = Xsrc[ids.long()].contiguous()
    h1p, h2p, _ = _fwd(Xe, K1, W1, b1, W2, b2, rows)
    h1g, h2g, xg = _fwd(Xsrc, K1, W1, b1, W2, b2, rows, ids=ids, xg=True)
    assert torch.equal(xg, Xe) and torch.equal(h1g, h1p) and torch.equal(h2g, h2p)
    _check_fwd(f'fwd rows={rows} ids', Xe, K1, W1, b1, W2, b2, h1g, h2g)
    h1g2, h2g2, _ = _fwd(Xsrc, K1, W1, b1, W2, b2, rows, ids=ids)                # ... and without the copy
    assert torch.equal(h1g2, h1p) and torch.equal(h2g2, h2p)
    # dense leading dimensions: the same bits
    h1c, h2c, _ = _fwd(X, K1, W1, b1, W2, b2, rows, ld=dict(ldx=K1, ldw1=K1, ldw2=128, ldh1=128, ldh2=128, ldxg=K1))
    assert torch.equal(h1c, H1) and torch.equal(h2c, H2)
    # and again
    h1r, h2r, _ = _fwd(X, K1, W1, b1, W2, b2, rows)
    assert torch.equal(h1r, H1) and torch.equal(h2r, H2)


@pytest.mark.parametrize('rows', [257, 65537])
@pytest.mark.parametrize('rd', ['0', '1', '32', 'rows-1', 'rows', 'rows+5', '-3'])
def test_fwd_rows_dev(rows, rd):
    """The device row count of a static layout: correct rows before the clamped count, zeros at and past it, nothing but finite
    numbers although every padding row of X is NaN."""
    K1 = 20
    rdv = eval(rd, {'rows': rows})
    n = max(0, min(rdv, rows))
    W1, b1, W2, b2 = _weights(K1)
    X = _fwd_x(rows, K1)
    H1, H2, _ = _fwd(X, K1, W1, b1, W2, b2, rows, rows_dev=rdv)
    assert bool(torch.isfinite(H1).all()) and bool(torch.isfinite(H2).all())
    assert not H1[n:].any() and not H2[n:].any()
    _check_fwd(f'fwd rows={rows} rows_dev={rd}', X[:n], K1, W1, b1, W2, b2, H1[:n], H2[:n])


# ================================================== B. kgw_mlp2_bwd_first (+ fold) ==================================================

@functools.lru_cache(maxsize=4)
def _bwd_case(rows, K1, n_up=None):
    """dH2 [n_up or rows, 128], W2, H1 [rows, 128] -- ANY matrix, not a ReLU output: both signs, a quarter zeros of both signs, one
    zero row, one zero column --, X [rows, K1]."""
    g = _gen(rows * 37 + K1 + (n_up or 0))
    dH2 = _wide(g, (n_up or rows, 128), 6)
    W2 = _weights(20)[2]
    H1 = _wide(g, (rows, 128), 4)
    z = torch.rand(rows, 128, device='cuda', generator=g) < 0.25
    zs = torch.where(torch.rand(rows, 128, device='cuda', generator=g) < 0.5, 0.0, -0.0)
    H1 = torch.where(z, zs, H1)
    H1[:, 77] = -0.0
    if rows >= 4:
        H1[rows // 3] = 0.0
    X = _wide(g, (rows, max(K1, 1)), 6)[:, :K1]
    return dH2, W2, H1, X


def _bwd(dH2, W2, H1, X, K1, rows, rows_dev=None, in_ids=None, dz=False, dz_fill=float('nan'), ws_short=0, ldw1=None, call='plain',
         src=None, image=None, flip=0, expect=OK):
    ldw1 = K1 + 4 if ldw1 is None else ldw1
    ldx = K1 + 3
    L = _L()
    dHs, W2s, H1s = _strided(dH2, 136), _strided(W2, 132), _strided(H1, 160)
    Xs = _strided(X, ldx) if K1 > 0 else None
    rd = None if rows_dev is None else torch.tensor([rows_dev], dtype=torch.int32, device='cuda')
    if rows_dev is not None:                      # padding rows of the static layout: NaN in every input
        n = max(0, min(rows_dev, rows))
        H1s[n:, :128] = float('nan')
        if in_ids is None:
            dHs[n:, :128] = float('nan')
        if Xs is not None:
            Xs[n:, :K1] = float('nan')
    dW1 = _out(128, K1, ldw1) if K1 > 0 else None
    db1 = torch.full((128,), float('nan'), device='cuda')
    nws = int(L.kgw_mlp2_bwd_first_workspace_floats(rows)) - ws_short
    ws = torch.full((max(nws, 1),), float('nan'), device='cuda')
    dZ = _out(rows, 128, 160, dz_fill) if dz else None
    head = (_p(dHs), 136, _p(W2s), 132, _p(H1s), 160, _p(Xs), ldx if K1 > 0 else 0, K1, rows)
    tail = (_p(dW1), ldw1 if K1 > 0 else 0, _p(db1), _p(ws), nws, _p(in_ids), _p(dZ), 160 if dz else 0)
    if call == 'plain':
        rc = L.kgw_mlp2_bwd_first(*head, _p(rd), *tail, _st())
    elif call == 'partial':
        rc = L.kgw_mlp2_bwd_first_partial(*head, _p(rd), *tail, src, _st())
    else:
        assert rows_dev is None
        rc = L.kgw_mlp2_bwd_first_packed(*head, *tail, image, flip, src, _st())
    assert rc == expect, rc
    assert _pad_ok(dHs, 128) and _pad_ok(W2s, 128) and _pad_ok(H1s, 128) and (Xs is None or _pad_ok(Xs, K1))
    assert (dW1 is None or _pad_ok(dW1, K1)) and (dZ is None or _pad_ok(dZ, 128))
    return dict(dW1=torch.zeros(128, 0, device='cuda') if dW1 is None else dW1[:, :K1], db1=db1, dZ=None if dZ is None else dZ[:, :128],
                ws=ws)


def _pipe32(dH2, W2, H1, X, K1, in_ids, n):
    """The fp32 device pipeline of the same operands: ((dH2[src] @ W2) * (H1 > 0)).t() @ [X | 1]."""
    if in_ids is not None:
        ids = in_ids[:n].long()
        G = dH2[ids.clamp(min=0)]
        keep = (ids >= 0)[:, None]
    else:
        G, keep = dH2[:n], True
    D32 = (G @ W2) * ((H1[:n] > 0) & keep)
    Xp = torch.cat([X[:n, :K1], torch.ones(n, 1, device='cuda')], dim=1)
    return D32, D32.t() @ Xp


def _check_bwd(name, res, dH2, W2, H1, X, K1, in_ids=None, n=None):
    """dW1 | db1 against float64; dZ (when written) relative to |dH2[src]||W2|, masked.

    D is never an input of the kernel: it is computed, rounded, and summed over the rows at once.  Relative to |D|^T |[X | 1]| the
    error of that sum has no ceiling and no stable ratio to the fp32 pipeline's: where D cancels (|D| << |dH2||W2|) the
    pipeline itself is hundreds of u away over few rows, and the maximum sits on whichever element cancels most (rows = 1: the
    pipeline 209 u, the bf16-pipe kernel 186 u; rows = 33, K1 = 21: 27 u, the fp32-pipe kernel 109 u).  Both assertions are
    therefore made on the scale of the WHOLE dot product, sum_r sum_o |dH2[r, o]||W2[o, c]||x'[r, k]| masked, which bounds the
    roundings of both products; the figures relative to |D|^T |X'| are printed beside them."""
    n = H1.shape[0] if n is None else n
    D, sD, dW1, sW, db1, sb = R.ref_bwd(dH2, W2, H1, X, K1, in_ids=in_ids, rows_real=n)
    D32, C32 = _pipe32(dH2, W2, H1, X, K1, in_ids, n)
    got = torch.cat([res['dW1'], res['db1'][:, None]], dim=1)
    ref, sc = torch.cat([dW1, db1[:, None]], dim=1), torch.cat([sW, sb[:, None]], dim=1)
    print(f'[mlp2 {name} dW1|db1 relative to |D|^T |X\'|] e3 = {R.rel_err(got, ref, sc) / U:.3f} u, e32 = {R.rel_err(C32, ref, sc) / U:.3f} u')
    sc2 = R.scale_bwd_whole(sD, X, K1)
    _bar(name + ' dW1|db1', R.rel_err(got, ref, sc2), R.rel_err(C32, ref, sc2), got.numel())
    if res['dZ'] is not None and n > 0:
        _bar(name + ' dZ', R.rel_err(res['dZ'][:n], D, sD), R.rel_err(D32, D, sD), D.numel())
    return D


BWD_ROWS = [1, 31, 32, 33, 127, 128, 129, 4097, 32768, 32769, 32768 + 128 + 33]
BWD_CASES = [(r, 20) for r in BWD_ROWS] + [(r, k) for r in (33, 129) for k in (0, 1, 4, 21, 31)]


@pytest.mark.parametrize('rows,K1', BWD_CASES)
def test_bwd_first_matches_float64(rows, K1):
    """One block is 128 rows, the grid is capped at 256 blocks x 4 wavefronts x 32 rows = 32 768.  K1 = 0: no X, no dW1, only db1;
    K1 = 31: the bias row of the second product is lane 31.  The mask is (H1 > 0) of an arbitrary H1."""
    dH2, W2, H1, X = _bwd_case(rows, K1)
    res = _bwd(dH2, W2, H1, X, K1, rows)
    _check_bwd(f'bwd rows={rows} K1={K1}', res, dH2, W2, H1, X, K1)
    assert not res['db1'][77].any() and not res['dW1'][77].any()                 # the zero column of H1
    again = _bwd(dH2, W2, H1, X, K1, rows)
    assert torch.equal(again['dW1'], res['dW1']) and torch.equal(again['db1'], res['db1'])


def test_bwd_first_argument_checks():
    rows, K1 = 129, 20
    dH2, W2, H1, X = _bwd_case(rows, K1)
    res = _bwd(dH2, W2, H1, X, K1, rows, ws_short=1, expect=E_RANGE)
    assert bool(torch.isnan(res['db1']).all()) and bool(torch.isnan(res['dW1']).all()) and bool(torch.isnan(res['ws']).all())
    g = _gen(1)
    X32 = _wide(g, (rows, 32), 6)
    res = _bwd(dH2, W2, H1, X32, 32, rows, expect=E_UNSUPPORTED)
    assert bool(torch.isnan(res['db1']).all()) and bool(torch.isnan(res['dW1']).all())


def _injection(rows, g):
    """in_ids: a partial injection of the rows into a shorter dH2 -- ~40 % of the rows, one whole 32-row tile, row 0 and the last
    row are not in the batch (-1)."""
    ids = torch.full((rows,), -1, dtype=torch.int64, device='cuda')
    keep = torch.rand(rows, device='cuda', generator=g) >= 0.4
    ntiles = (rows + 31) // 32
    t = 1 if ntiles > 2 else ntiles - 1
    keep[32 * t:32 * t + 32] = False
    keep[0] = False
    keep[rows - 1] = False
    if not bool(keep.any()):
        keep[1] = True
    m = int(keep.sum())
    ids[keep] = torch.randperm(m + 5, device='cuda', generator=g)[:m]
    return ids.to(torch.int32), m + 5


@pytest.mark.parametrize('rows', [33, 129, 4097, 32769])
@pytest.mark.parametrize('K1', [20, 0])
def test_bwd_first_row_injection_and_dz(rows, K1):
    g = _gen(rows + K1)
    ids, n_up = _injection(rows, g)
    dH2, W2, H1, X = _bwd_case(rows, K1, n_up)
    res = _bwd(dH2, W2, H1, X, K1, rows, in_ids=ids, dz=True)
    _check_bwd(f'bwd rows={rows} K1={K1} in_ids', res, dH2, W2, H1, X, K1, in_ids=ids)
    assert bool((res['dZ'][ids < 0] == 0).all()) and bool((res['dZ'][:, 77] == 0).all())
    assert bool(((res['dZ'] == 0) | (H1 > 0)).all())                             # the mask is `> 0` and nothing else
    plain = _bwd(dH2, W2, H1, X, K1, rows, in_ids=ids)
    assert torch.equal(plain['dW1'], res['dW1']) and torch.equal(plain['db1'], res['db1'])


def test_bwd_first_dz_rows_past_rows_dev_are_left_alone():
    """include/kgwas_hip.h: dZ rows at and past *rows_dev are NOT written."""
    rows, K1, n = 129, 4, 70
    g = _gen(5)
    ids, n_up = _injection(rows, g)
    dH2, W2, H1, X = _bwd_case(rows, K1, n_up)
    res = _bwd(dH2, W2, H1, X, K1, rows, rows_dev=n, in_ids=ids, dz=True, dz_fill=MARK)
    assert bool((res['dZ'][n:] == MARK).all())
    _check_bwd(f'bwd rows={rows} rows_dev={n} in_ids dZ', res, dH2, W2, H1, X, K1, in_ids=ids, n=n)
    assert bool((res['dZ'][:n][ids[:n] < 0] == 0).all())


@pytest.mark.parametrize('rows', [129, 32769])
@pytest.mark.parametrize('rd', ['0', '1', 'rows-1', 'rows'])
def test_bwd_first_rows_dev(rows, rd):
    """The padding rows of dH2, H1 and X hold NaN: dW1 / db1 are the sums over the real rows, exactly zero for an empty batch."""
    K1 = 20
    n = eval(rd, {'rows': rows})
    dH2, W2, H1, X = _bwd_case(rows, K1)
    res = _bwd(dH2, W2, H1, X, K1, rows, rows_dev=n)
    _check_bwd(f'bwd rows={rows} rows_dev={rd}', res, dH2, W2, H1, X, K1, n=n)
    if n == 0:
        assert not res['dW1'].any() and not res['db1'].any()


def test_bwd_first_partial_describes_its_partials():
    from kgwas_amd import _lib
    rows, K1 = 129, 20
    dH2, W2, H1, X = _bwd_case(rows, K1)
    src = (_lib.KgwGradSrc * 2)()
    res = _bwd(dH2, W2, H1, X, K1, rows, ldw1=K1, call='partial', src=src)
    for s, kind in zip(src, (GRAD_MLP2_W, GRAD_MLP2_B)):
        assert (s.kind, s.nblk, s.K1, s.ws) == (kind, 2, K1, res['ws'].data_ptr())
    assert bool(torch.isfinite(res['ws'][:2 * 4096]).all())                      # every block wrote its partial sums
    src = (_lib.KgwGradSrc * 2)()
    res = _bwd(dH2, W2, H1, X[:, :0], 0, rows, call='partial', src=src)
    assert (src[0].kind, src[0].ws) == (GRAD_DIRECT, None) and (src[1].kind, src[1].nblk, src[1].K1) == (GRAD_MLP2_B, 2, 0)
    src = (_lib.KgwGradSrc * 2)()
    res = _bwd(dH2, W2, H1, X, K1, rows, ldw1=K1 + 4, call='partial', src=src, expect=E_UNSUPPORTED)
    assert bool(torch.isnan(res['ws']).all())
    assert _L().kgw_mlp2_bwd_first_partial(*([None, 0] * 4), K1, rows, None, None, K1, None, None, 0, None, None, 0, None, None) == E_NULL


def test_bwd_first_has_no_one_sided_error():
    """k_mlp2_bwd_first3 multiplies odd rows negated so that the bf16 MFMA's truncation (a negative mean error) cancels in the row
    sums dW1 / db1.  Positive operands, every mask bit set (the worst case: every partial sum has one sign); the bars of
    test_tn_gemm_on_the_bf16_pipe_has_no_one_sided_error."""
    rows, K1 = 32768, 20
    g = _gen(7)
    dH2 = torch.rand(rows, 128, device='cuda', generator=g)
    W2 = torch.rand(128, 128, device='cuda', generator=g) * (57.0 / (32.0 * rows))            # db1 ~57
    H1 = torch.rand(rows, 128, device='cuda', generator=g) + 0.125
    X = torch.rand(rows, K1, device='cuda', generator=g)
    res = _bwd(dH2, W2, H1, X, K1, rows)
    _, _, dW1, _, db1, _ = R.ref_bwd(dH2, W2, H1, X, K1)
    C32 = _pipe32(dH2, W2, H1, X, K1, None, rows)[1]
    for name, got, g32, ref in (('db1', res['db1'], C32[:, K1], db1), ('dW1', res['dW1'], C32[:, :K1], dW1)):
        e3, e32 = got.double() - ref, g32.double() - ref
        m3, m32, a3, a32 = e3.mean().item(), e32.mean().item(), e3.abs().mean().item(), e32.abs().mean().item()
        print(f'[mlp2 bwd bias] {name}: mean error {m3:.3e} (fp32 pipeline {m32:.3e}), mean |error| {a3:.3e} ({a32:.3e}), '
              f'mean result {ref.mean().item():.1f}')
        assert abs(m3) <= max(2.0 * abs(m32), 0.1 * a3), (name, m3, m32)
        assert a3 <= 1.25 * a32, (name, a3, a32)


# ================================================== C. kgw_mlp2_bwd_first_packed ==================================================

def _image(rows32):
    return torch.full((int(_L().kgw_gemm3_packed_bytes(rows32)),), 0xA5, dtype=torch.uint8, device='cuda')


@pytest.mark.parametrize('with_ids', [False, True])
@pytest.mark.parametrize('flip', ['0', '1', '2', 'F'])
@pytest.mark.parametrize('rows', ['1', '33', '389', '2*32*F+7'])
def test_bwd_first_packed_image(rows, flip, with_ids):
    """The masked dh1 rows as kgw_gemm3's B operand image, written by k_mlp2_bwd_first3<true> alone: decoded it is dZ bit for bit,
    negated in every tile whose sign period (tile / flip) is odd, zero behind the last row."""
    from kgwas_amd import ops
    F = int(_L().kgw_gemm3_flip())
    rows, flip = eval(rows, {'F': F}), eval(flip, {'F': F})
    rows32 = (rows + 31) // 32 * 32
    K1 = 4
    g = _gen(rows * 5 + flip)
    ids, n_up = _injection(rows, g) if with_ids and rows > 1 else (None, None)
    dH2, W2, H1, X = _bwd_case(rows, K1, n_up)
    img = _image(rows32)
    if not SPLIT:                                 # the image is written by the bf16-pipe kernel only
        _bwd(dH2, W2, H1, X, K1, rows, in_ids=ids, dz=True, call='packed', image=_p(img), flip=flip, expect=E_UNSUPPORTED)
        assert bool((img == 0xA5).all())
        return
    res = _bwd(dH2, W2, H1, X, K1, rows, in_ids=ids, dz=True, call='packed', image=_p(img), flip=flip)
    _check_bwd(f'packed rows={rows} flip={flip} ids={with_ids}', res, dH2, W2, H1, X, K1, in_ids=ids)
    dZ = res['dZ'].contiguous()
    dec = R.decode_g3_image(img, rows32)
    sign = torch.ones(rows32)
    if flip:
        sign[((torch.arange(rows32) // 32 // flip) & 1) == 1] = -1.0
    assert flip == 0 or rows <= 32 * flip or bool((sign[:rows] < 0).any())       # (the long case crosses a sign period)
    assert np.array_equal(dec[:rows], (dZ.cpu() * sign[:rows, None]).numpy())
    assert not dec[rows:].any()
    assert np.array_equal(img.cpu().numpy(), R.encode_g3_image(dZ.cpu().numpy(), flip))       # and piece by piece
    if flip == F:
        pack = ops.gemm3_pack(dZ, rows32, True, k_valid=rows)
        assert torch.equal(img, pack)
        A = _wide(g, (64, rows32), 6)
        assert torch.equal(ops.gemm3(A, img), ops.gemm3(A, pack))
    img2 = _image(rows32)
    res2 = _bwd(dH2, W2, H1, X, K1, rows, in_ids=ids, call='packed', image=_p(img2), flip=flip)          # dZ null
    assert torch.equal(img2, img) and torch.equal(res2['dW1'], res['dW1']) and torch.equal(res2['db1'], res['db1'])


def test_bwd_first_packed_argument_checks():
    rows, K1 = 33, 4
    dH2, W2, H1, X = _bwd_case(rows, K1)
    img = _image(64 + 32)
    res = _bwd(dH2, W2, H1, X, K1, rows, call='packed', image=_p(img), flip=3, expect=E_RANGE)
    assert bool(torch.isnan(res['db1']).all())
    res = _bwd(dH2, W2, H1, X, K1, rows, call='packed', image=C.c_void_p(img.data_ptr() + 8), flip=2, expect=E_UNSUPPORTED)
    assert bool(torch.isnan(res['db1']).all())
    res = _bwd(dH2, W2, H1, X, K1, rows, call='packed', image=None, flip=2, expect=E_NULL)
    assert bool(torch.isnan(res['db1']).all()) and bool((img == 0xA5).all())


# ====================================================== D. kgw_mlp2w_fwd ======================================================

@functools.lru_cache(maxsize=None)
def _wide_weights():
    g = _gen(77)
    rs = torch.exp2(torch.randint(-6, 7, (128, 1), device='cuda', generator=g).float())
    W1 = _wide(g, (128, 128), 4) * rs
    b1 = torch.randn(128, device='cuda', generator=g) * rs[:, 0] * 8.0
    return W1, b1


def _mlp2w(n_rows, W1, b1, W2, b2, seed, expect=OK, n_jobs=None):
    g = _gen(seed)
    heights = [50, 9, 301, 77, 13]
    rows = sum(n_rows)
    srcs = [_strided(_wide(g, (heights[j], 128), 6), 160) for j in range(len(n_rows))]     # different heights, one row stride
    idss = [torch.randint(0, heights[j], (max(n, 1),), device='cuda', generator=g).to(torch.int32) for j, n in enumerate(n_rows)]
    W1s, W2s = _strided(W1, 132), _strided(W2, 132)
    Xg, H1, H2 = (_out(max(rows, 1), 128, 160, MARK) for _ in range(3))
    n = len(n_rows)
    S = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
    I = (C.c_void_p * n)(*[i.data_ptr() for i in idss])
    N = (C.c_int64 * n)(*n_rows)
    rc = _L().kgw_mlp2w_fwd(n if n_jobs is None else n_jobs, S, I, N, 160, _p(W1s), 132, _p(b1), _p(W2s), 132, _p(b2), _p(Xg), _p(H1),
                            _p(H2), 160, _st())
    assert rc == expect, rc
    assert all(_pad_ok(b, 128) for b in srcs + [W1s, W2s, Xg, H1, H2])
    x = torch.cat([s[:, :128][i[:k].long()] for s, i, k in zip(srcs, idss, n_rows)]) if rows else None
    return x, Xg[:, :128], H1[:, :128], H2[:, :128]


MLP2W_JOBS = [[1], [31], [32], [33], [63], [64], [65], [5, 40, 0, 19], [0, 7], [377, 0, 5003, 1201]]


@pytest.mark.parametrize('null_biases', [False, True])
@pytest.mark.parametrize('n_rows', MLP2W_JOBS, ids=lambda j: '-'.join(map(str, j)))
def test_mlp2w_matches_float64(n_rows, null_biases):
    """A block is two 32-row tiles x two column halves: one tile, both sides of a block, row tiles that straddle jobs, empty jobs at
    the front and in the middle.  Both products are 128 terms on the fp32 pipe; every column of every row is compared, so both
    column-half wavefronts of a tile are."""
    W1, b1 = _wide_weights()
    W2, b2 = _weights(20)[2:]
    if null_biases:
        b1 = b2 = None
    x, Xg, H1, H2 = _mlp2w(n_rows, W1, b1, W2, b2, sum(n_rows))
    name = f'mlp2w jobs={n_rows} biases={"null" if null_biases else "set"}'
    assert torch.equal(Xg, x)
    z1 = x.double() @ W1.double().t()
    s1 = x.double().abs() @ W1.double().abs().t()
    y32 = x @ W1.t()
    if b1 is not None:
        z1, s1, y32 = z1 + b1.double(), s1 + b1.double().abs(), y32 + b1
    _bar(name + ' H1', R.rel_err(H1, torch.relu(z1), s1), R.rel_err(torch.relu(y32), torch.relu(z1), s1))
    z2, s2 = R.ref_second(H1, W2, b2)
    y32 = H1 @ W2.t()
    _bar(name + ' H2', R.rel_err(H2, torch.relu(z2), s2), R.rel_err(torch.relu(y32 if b2 is None else y32 + b2), torch.relu(z2), s2))


def test_mlp2w_empty_and_too_many_jobs():
    W1, b1 = _wide_weights()
    W2, b2 = _weights(20)[2:]
    for n_rows, n_jobs, expect in (([0, 0], None, OK), ([3, 4, 5, 6, 7], 5, E_RANGE)):
        _, Xg, H1, H2 = _mlp2w(n_rows, W1, b1, W2, b2, 1, expect=expect, n_jobs=n_jobs)
        assert all(bool((t == MARK).all()) for t in (Xg, H1, H2))                # nothing was written


# ================================================== E. the fp32-pipe variants ==================================================

def test_fp32_pipe_variants_hold_the_same_bars():
    """KGW_MLP2_SPLIT=0: k_mlp2_fwd and k_mlp2_bwd_first instead of the bf16-pipe kernels.  The switch is read once per process,
    hence one child; there kgw_mlp2_bwd_first_packed must refuse (test_bwd_first_packed_image's other branch)."""
    env = dict(os.environ, KGW_MLP2_SPLIT='0')
    p = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-m', 'gpu', os.path.join('tests', 'test_gpu_mlp2_kernels.py'),
                        '-k', 'not fp32_pipe_variants'],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    assert ' passed' in p.stdout
