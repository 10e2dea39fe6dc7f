"""The weight-gradient product family C = A^T B (+ column sums of A) over tall inputs -- k_tn_gemm<MT, NT>, k_tn_reduce, k_tn_gemm_ride
and the reduce blocks carried by k_transform_bwd and k_adam_fused<false> (kgwas_amd/csrc/kgw_dense_tn.h, kgw_dense_transform.h,
kgw_dense_optim.h) -- called at the C ABI and compared with plain float64 at the planner, tiling, reduce and carrier edges of
tests/tn_gemm_ref.py's case table (test_tn_gemm_ref.py asserts from the plan twin that each case reaches the edge it is named for).

Every call: C and the column sums pre-filled with NaN, ldc wider than the row with MARK in the padding, MARK in the colsum rows
past colsum_repeat, NaN in the operands' padding columns, inputs compared with a copy afterwards, the workspace EXACTLY the twin's
need in floats with the sentinel directly behind it, kgw_tn_split / kgw_tn_direct_rows restored in `finally`.  The bars:
  derived   fp32 pipe (every tiling but <2,2>; <2,2> under kgw_tn_split(0)): |got - ref| <= (depth + 2) 2^-24 S element by element,
            depth from the plan (tn_gemm_ref's docstring); the column sums likewise with depth_cs over sum |a|.  S == 0: exactly 0.0.
  exact     the integer and row-stamp generators under torch.equal on both pipes and every tiling; bit-identity between entry
            points, carriers, two runs; k_tn_reduce's order of additions restated in torch on the workspace's own slabs.
  project   bf16 x 3 pipe: e3 <= max(1.25 e32, 4 2^-24) and e3 <= 16 2^-24 with e = max |C - ref| / S and e32 the fp32 pipe's on the
            same operands (tests/test_gpu_dense.py), and that file's mean-error test on positive data.
Under -s every comparison prints its largest err / (2^-24 S) next to its bar."""
import ctypes as C
import functools

import pytest
import torch

from tests import tn_gemm_ref as T
from tests.test_gpu_param_kernels import (E_NULL, E_RANGE, E_UNSUPPORTED, MARK, NAN, OK, SENT, Arena, _finish, _L, _lib, _p, _same, _st,
                                          _untouched)

pytestmark = pytest.mark.gpu

DIRECT, TN, TN_COLSUM = 0, 1, 2                                    # KgwGradSrc.kind (include/kgwas_hip.h)
_WORST = {}


class knobs:
    """kgw_tn_split / kgw_tn_direct_rows for the length of a `with`, restored in `finally`."""

    def __init__(self, split=True, direct=0):
        self.split, self.direct = split, direct

    def __enter__(self):
        L = _L()
        self.was_split = L.kgw_tn_split(-1)
        self.was_direct = L.kgw_tn_direct_rows(-1)
        L.kgw_tn_split(1 if self.split else 0)
        L.kgw_tn_direct_rows(self.direct)

    def __exit__(self, *exc):
        L = _L()
        L.kgw_tn_split(self.was_split)
        L.kgw_tn_direct_rows(self.was_direct)


# ====================================================== operands ============================================================

class Operands:
    """A [rows, M] and B [rows, N] as columns of wider NaN-filled matrices (lda, ldb), optionally off the 16-byte boundary by
    a_off / b_off floats, optionally with NaN in every row from `nan_from` on."""

    def __init__(self, A, B, lda=None, ldb=None, a_off=0, b_off=0, nan_from=None):
        self.rows, self.M, self.N = A.shape[0], A.shape[1], B.shape[1]
        self.lda, self.ldb = lda or self.M, ldb or self.N
        self.Ar = Arena()
        self.A = self._place(A, self.lda, a_off, nan_from)
        self.B = self._place(B, self.ldb, b_off, nan_from)
        assert self.A.data_ptr() % 16 == 4 * a_off and self.B.data_ptr() % 16 == 4 * b_off
        self.keep = [(f, f.clone()) for f, _ in self.Ar.flats]

    def _place(self, X, ld, off, nan_from):
        rows, w = X.shape
        flat = self.Ar.out(rows * ld + off)
        v = flat[off:].view(rows, ld)[:, :w]
        v.copy_(X)
        if nan_from is not None:
            v[nan_from:] = NAN
        return v

    def align(self):
        return self.A.data_ptr() % 16, self.B.data_ptr() % 16

    def check(self):
        self.Ar.check()
        for f, k in self.keep:
            assert _same(f, k), 'a call wrote into an input'


@functools.lru_cache(maxsize=None)
def _data(kind, rows, M, N, seed=1):
    A, B = T.gen(kind, rows, M, N, 1000 * seed + rows + 3 * M + 7 * N)
    return A, B


@functools.lru_cache(maxsize=None)
def _ref(kind, rows, M, N, seed=1, n=None):
    A, B = _data(kind, rows, M, N, seed)
    return T.ref64(A, B, 0, n)


@functools.lru_cache(maxsize=None)
def _ops(kind, rows, M, N, seed=1):
    return Operands(*_data(kind, rows, M, N, seed))


# ====================================================== one call ============================================================

class Out:
    pass


def _call(op, entry='ex', c_t=0, colsum=True, rep=1, split=True, direct=0, rows_dev=None, ws_delta=0, expect=OK, ride=None, dense=None,
          null=None, **over):
    """One call of kgw_tn_gemm / _ex / _partial / _partial_ride under the conditions of the module docstring.  `over`: arguments
    replaced for the refusal tests (x_rows, x_M, x_lda, x_ldc, x_rep, x_cs_ld); `null`: the pointer passed as NULL."""
    L = _L()
    M, N = op.M, op.N
    p = T.plan(op.rows, M, N, op.lda, op.ldb, *op.align(), split=split, direct_rows=direct)
    partial = entry in ('partial', 'ride')
    dense = partial if dense is None else dense
    Ar = Arena()
    inner, outer = (M, N) if c_t else (N, M)
    ldc = inner + (0 if dense else 3)
    Cfull = Ar.out(outer, ldc)
    Cfull[:, inner:] = MARK
    cs_ld = M if (partial or entry == 'gemm') else M + 5
    if partial or entry == 'gemm':
        rep = 1
    csfull = Ar.out(rep + 1, cs_ld, fill=MARK)
    csfull[:rep, :M] = NAN
    ws = Ar.out(p.need + ws_delta)
    rd = None if rows_dev is None else Ar.ints([rows_dev])
    src = (_lib().KgwGradSrc * 2)()
    for s in src:
        s.kind = -9
    a = dict(A=_p(op.A), lda=op.lda, M=M, B=_p(op.B), ldb=op.ldb, N=N, rows=op.rows, C=_p(Cfull), ldc=ldc, rep=rep, cs_ld=cs_ld,
             cs=_p(csfull) if colsum else None, ws=_p(ws), nws=ws.numel())
    a.update({k[2:]: v for k, v in over.items()})
    if null:
        a[null] = None
    with knobs(split, direct):
        if entry == 'gemm':
            assert c_t == 0
            rc = L.kgw_tn_gemm(a['A'], a['lda'], a['M'], a['B'], a['ldb'], a['N'], a['rows'], a['C'], a['ldc'], a['cs'], a['ws'], a['nws'], _st())
        elif entry == 'ex':
            rc = L.kgw_tn_gemm_ex(a['A'], a['lda'], a['M'], a['B'], a['ldb'], a['N'], a['rows'], a['C'], a['ldc'], c_t, a['cs'], a['rep'],
                                  a['cs_ld'], a['ws'], a['nws'], _p(rd), _st())
        else:
            sp = None if null == 'src' else src
            args = [a['A'], a['lda'], a['M'], a['B'], a['ldb'], a['N'], a['rows'], a['C'], a['ldc'], c_t, a['cs'], a['ws'], a['nws'], _p(rd), sp]
            if entry == 'partial':
                rc = L.kgw_tn_gemm_partial(*args, _st())
            else:
                rc = L.kgw_tn_gemm_partial_ride(*args, None if ride is None else C.cast(C.pointer(ride), C.c_void_p), _st())
    assert rc == expect, (rc, expect)
    Ar.check()
    assert float(Ar.flats[2][0][p.need + ws_delta]) == SENT, 'the guard directly behind the workspace'
    if rd is not None:
        assert int(rd[0]) == rows_dev
    op.check()
    assert bool((Cfull[:, inner:] == MARK).all()), 'the padding of C was written'
    assert bool((csfull[rep:] == MARK).all()) and bool((csfull[:, M:] == MARK).all()), 'column sums written past colsum_repeat / M'
    o = Out()
    o.p, o.Cfull, o.csfull, o.ws, o.src, o.arena, o.c_t = p, Cfull, csfull, ws, src, Ar, c_t
    o.Cd = Cfull[:, :inner]
    o.C = o.Cd.t() if c_t else o.Cd                                # logical [M, N]
    o.cs = csfull[:rep, :M]
    if rc != OK:
        assert _untouched(o.Cd, NAN) and _untouched(o.cs, NAN) and _untouched(ws, NAN), 'a refused call wrote something'
        assert all(s.kind == -9 for s in src), 'a refused call wrote its records'
    elif not colsum:
        assert _untouched(o.cs, NAN), 'column sums written without colsum_a'
    return o


def _finish_out(o, colsum=True):
    """kgw_grad_finish on the records of a partial call; returns (fin, fin_cs): dst, the gradient tensors being o.Cd / o.cs."""
    Ar = Arena()
    d = dict(C=o.Cd, fin=Ar.out(*o.Cd.shape), cs=o.cs[0] if colsum else None, fin_cs=Ar.out(o.cs.shape[1]) if colsum else None)
    _finish([d], o.src)
    Ar.check()
    o.arena.check()
    return d['fin'], d['fin_cs']


def _u(tag, name, got, ref, scale, bar):
    e = T.err_in_u(got, ref, scale)
    _WORST[name] = max(_WORST.get(name, 0.0), e)
    print(f'[tn {tag}] {name}: err / (2^-24 S) = {e:.3f} of a bound of {bar}  (largest so far {_WORST[name]:.3f})')
    return e


def _check_fp32(tag, o, ref, colsum=True, p=None):
    p = p or o.p
    e = _u(tag, 'C fp32 pipe', o.C, ref.C, ref.S, p.depth + 2)
    assert e <= p.depth + 2, (tag, e, p.depth + 2)
    if colsum:
        _check_cs(tag, o, ref, p)
    return e


def _check_cs(tag, o, ref, p=None):
    p = p or o.p
    for q in range(o.cs.shape[0]):
        e = _u(tag, 'colsum', o.cs[q], ref.cs, ref.sa, p.depth_cs + 2)
        assert e <= p.depth_cs + 2, (tag, e, p.depth_cs + 2)
        assert _same(o.cs[q], o.cs[0])


def _check_bf16(tag, o, ref, e32, colsum=True, p=None):
    bar = max(1.25 * e32, 4.0)
    e3 = _u(tag, 'C bf16x3 pipe', o.C, ref.C, ref.S, f'max(1.25 x {e32:.3f}, 4) and 16')
    assert e3 <= bar, (tag, e3, e32)
    assert e3 <= 16, (tag, e3)
    if colsum:
        _check_cs(tag, o, ref, p)


def _both_pipes(tag, op, ref, p_of=None, **kw):
    """The call on the fp32 pipe under the derived bar and, where the plan says bf16, on that pipe under the project's bars."""
    o32 = _call(op, split=False, **kw)
    p32 = p_of(o32.p) if p_of else o32.p
    e32 = _check_fp32(tag, o32, ref, kw.get('colsum', True), p32)
    o3 = _call(op, split=True, **kw)
    p3 = p_of(o3.p) if p_of else o3.p
    if o3.p.bf16:
        _check_bf16(tag, o3, ref, e32, kw.get('colsum', True), p3)
    else:
        assert _same(o3.Cfull, o32.Cfull) and _same(o3.csfull, o32.csfull)
    return o32, o3


def _src_matches_twin(o, colsum=True):
    p, W, Bc = o.p, o.src[0], o.src[1]
    if p.nblk == 1:
        assert W.kind == DIRECT and Bc.kind == DIRECT
        return
    want = (TN, p.nblk, o.C.shape[0], o.C.shape[1], p.MT, p.NT, p.gy, p.gz, o.c_t)
    assert (W.kind, W.nblk, W.M, W.N, W.MT, W.NT, W.gy, W.gz, W.c_transposed) == want and W.ws == o.ws.data_ptr()
    if colsum:
        assert (Bc.kind, Bc.nblk, Bc.M, Bc.N, Bc.MT, Bc.NT, Bc.gy, Bc.gz, Bc.c_transposed) == (TN_COLSUM,) + want[1:]
        assert Bc.ws == o.ws.data_ptr() + 4 * p.cs_off
    else:
        assert Bc.kind == DIRECT


# ====================================================== A. the case table ===================================================

STAMPED = ['one-row', 'tail-only', 'one-step', 'first-split', 'cap-empty-wave', 'cap-ragged', 't11-two-by', 'direct-transform']


@pytest.mark.parametrize('name', list(T.CASES))
def test_case_against_float64(name):
    rows, M, N, direct = T.CASES[name]
    op, ref = _ops('wide', rows, M, N), _ref('wide', rows, M, N)
    c_t = 1 if len(name) % 2 else 0                                      # both store forms over the table
    o32, o3 = _both_pipes(name, op, ref, direct=direct, c_t=c_t)
    assert o3.p == T.case_plan(name) and o32.p == T.case_plan(name, split=False)
    if o3.p.bf16 and rows >= 64:
        assert not _same(o3.Cd, o32.Cd), 'the two pipes were not both exercised'
    again = _call(op, direct=direct, c_t=c_t)                            # two runs
    assert _same(again.Cfull, o3.Cfull) and _same(again.csfull, o3.csfull)
    # the plan against the library's own records, and the first launch alone
    for split, full in ((True, o3), (False, o32)):
        part = _call(op, 'partial', direct=direct, c_t=c_t, split=split)
        assert part.p == full.p
        _src_matches_twin(part)
        if part.p.nblk == 1:
            assert _same(part.Cd, full.Cd) and _same(part.cs, full.cs), 'one row block: complete after the one launch'
        else:
            assert _untouched(part.Cd, NAN) and _untouched(part.cs, NAN), 'partial wrote the result'
            fin, fin_cs = _finish_out(part)
            assert _same(part.Cd, full.Cd) and _same(fin, full.Cd) and _same(part.cs[0], full.cs[0]) and _same(fin_cs, full.cs[0])


@pytest.mark.parametrize('name', list(T.CASES))
def test_case_is_exact_on_integers(name):
    rows, M, N, direct = T.CASES[name]
    kinds = ['integer'] + (['stamp'] if name in STAMPED else [])
    for kind in kinds:
        op, ref = _ops(kind, rows, M, N), _ref(kind, rows, M, N)
        assert float(ref.S.max()) < 2 ** 24
        for split in (True, False):
            for c_t in (0, 1):
                o = _call(op, split=split, direct=direct, c_t=c_t, rep=2)
                assert torch.equal(o.C.double().cpu(), ref.C), (name, kind, split, c_t)
                assert torch.equal(o.cs[0].double().cpu(), ref.cs) and _same(o.cs[1], o.cs[0]), (name, kind, split)


def test_workspace_of_exactly_the_need_and_one_float_less():
    for name in ('one-row', 'nblk5', 'cs-nblk25', 't21-nblk13', 't12', 't11', 'cap-rpw80', 'direct-transform'):
        rows, M, N, direct = T.CASES[name]
        op = _ops('wide', rows, M, N)
        for entry in ('ex', 'partial'):
            _call(op, entry, direct=direct, ws_delta=-1, expect=E_RANGE)
            ok = _call(op, entry, direct=direct, colsum=False)              # no column sums: the same need
            _call(op, entry, direct=direct, colsum=False, ws_delta=-1, expect=E_RANGE)
            if ok.p.nblk > 1:
                assert not bool(torch.isnan(ok.ws[:ok.p.cs_off]).any()) and _untouched(ok.ws[ok.p.cs_off:], NAN)
            else:
                assert _untouched(ok.ws, NAN), 'one row block: the workspace is not used'


# ====================================================== B. tiling fallbacks ==================================================

# (M, N, lda, ldb, a_off, b_off) at 1025 rows -> tiling
FALLBACKS = {
    'odd-lda': ((128, 128, 129, 128, 0, 0), (1, 4)),
    'A+4bytes': ((128, 128, 128, 128, 1, 0), (1, 4)),
    'ldb-130': ((128, 128, 128, 130, 0, 0), (2, 2)),
    'ldb-129': ((128, 128, 128, 129, 0, 0), (2, 1)),
    'B+8bytes': ((128, 128, 128, 128, 0, 2), (2, 2)),
    'B+8bytes-narrow-A': ((6, 128, 6, 128, 0, 2), (1, 2)),
    'odd-lda-odd-ldb': ((128, 128, 129, 129, 0, 0), (1, 1)),
    'A+4bytes-B+4bytes': ((128, 128, 128, 128, 1, 1), (1, 1)),
    'odd-lda-B+8bytes': ((128, 128, 131, 132, 0, 2), (1, 2)),
}


@pytest.mark.parametrize('name', list(FALLBACKS))
def test_tiling_fallbacks(name):
    (M, N, lda, ldb, a_off, b_off), want = FALLBACKS[name]
    A, B = _data('wide', 1025, M, N)
    op = Operands(A, B, lda, ldb, a_off, b_off)
    ref = _ref('wide', 1025, M, N)
    o32, o3 = _both_pipes(name, op, ref)
    assert (o3.p.MT, o3.p.NT) == want
    part = _call(op, 'partial')
    assert (part.src[0].MT, part.src[0].NT) == want, 'the tiling read back from the library'
    _src_matches_twin(part)
    Ai, Bi = _data('integer', 1025, M, N)
    oi = _call(Operands(Ai, Bi, lda, ldb, a_off, b_off))
    ri = _ref('integer', 1025, M, N)
    assert torch.equal(oi.C.double().cpu(), ri.C) and torch.equal(oi.cs[0].double().cpu(), ri.cs)


# ====================================================== C. output forms ======================================================

@pytest.mark.parametrize('rows,M,N', [(1025, 128, 128), (700, 66, 130), (3073, 128, 20), (2000, 5, 7), (256, 128, 128)])
def test_output_forms(rows, M, N):
    op, ref = _ops('wide', rows, M, N), _ref('wide', rows, M, N)
    base = _call(op)
    for c_t in (0, 1):
        for rep in (1, 3):
            o = _call(op, c_t=c_t, rep=rep)
            assert _same(o.C, base.C) and all(_same(o.cs[q], base.cs[0]) for q in range(rep))
        o = _call(op, c_t=c_t, colsum=False)
        assert _same(o.C, base.C)
    g = _call(op, 'gemm')
    e = _call(op, 'ex', dense=True)
    assert _same(g.C, base.C) and _same(g.cs, base.cs) and _same(e.C, base.C)
    # operands as columns of a wider matrix (NaN in the other columns)
    A, B = _data('wide', rows, M, N)
    wide = Operands(A, B, M + 10, N + 36)
    o32, o3 = _both_pipes(f'strided {rows}x{M}x{N}', wide, ref)
    if (o3.p.MT, o3.p.NT) == (base.p.MT, base.p.NT):
        assert _same(o3.C, base.C) and _same(o3.cs, base.cs)


# ====================================================== D. rows_dev ==========================================================

@pytest.mark.parametrize('cap', [2049, 8193])
def test_rows_dev(cap):
    M = N = 128
    A, B = _data('wide', cap, M, N)
    Ai, Bi = _data('integer', cap, M, N)
    at_cap = _call(_ops('wide', cap, M, N), rows_dev=cap)
    assert _same(at_cap.Cfull, _call(_ops('wide', cap, M, N)).Cfull), 'rows_dev == rows is the static plan'
    for n in (0, -3, 1, 255, 257, cap - 1, cap, cap + 100):
        k = min(cap, max(n, 0))
        op = Operands(A, B, nan_from=k)
        ref = T.ref64(A, B, 0, k)
        tag = f'rows_dev {n} of {cap}'
        o32, o3 = _both_pipes(tag, op, ref, p_of=lambda p: T.plan_dev(p, n), rows_dev=n, rep=2)
        for o in (o32, o3):
            assert bool(torch.isfinite(o.Cd).all()) and bool(torch.isfinite(o.cs).all()), 'a row at or past the device count was read'
            if k == 0:
                assert bool((o.Cd == 0).all()) and bool((o.cs == 0).all())
        if n >= cap:
            assert _same(o3.Cfull, at_cap.Cfull) and _same(o3.cs[0], at_cap.cs[0])
        opi = Operands(Ai, Bi, nan_from=k)
        ri = T.ref64(Ai, Bi, 0, k)
        for split in (True, False):
            oi = _call(opi, rows_dev=n, split=split, c_t=1)
            assert torch.equal(oi.C.double().cpu(), ri.C) and torch.equal(oi.cs[0].double().cpu(), ri.cs), (n, split)
        part = _call(opi, 'partial', rows_dev=n)
        fin, fin_cs = _finish_out(part)
        assert torch.equal(fin.double().cpu(), ri.C) and torch.equal(fin_cs.double().cpu(), ri.cs)


def test_rows_dev_on_the_other_tilings_and_the_direct_path():
    for (rows, M, N, direct) in [(3073, 128, 20, 0), (6145, 6, 128, 0), (4097, 6, 66, 0), (2000, 5, 7, 0), (1171, 128, 2176, 2048), (256, 128, 128, 0)]:
        A, B = _data('stamp', rows, M, N)
        for n in (0, 1, rows // 2 + 1, rows - 1):
            op = Operands(A, B, nan_from=n)
            ri = T.ref64(A, B, 0, n)
            o = _call(op, rows_dev=n, direct=direct)
            assert torch.equal(o.C.double().cpu(), ri.C) and torch.equal(o.cs[0].double().cpu(), ri.cs), (rows, M, N, n)


# ====================================================== E. slabs and the reduce order ========================================

# nblk 5 and 33 on every tiling; 29 (<2,2>) and 26 (<1,4>, eight column-sum groups): a group's tail loop adds four records and more
SLAB_SHAPES = [(1025, 66, 130), (8193, 66, 130), (1025, 128, 20), (8193, 128, 20), (1025, 6, 128), (8193, 6, 128), (1025, 6, 66), (8193, 6, 66),
               (1025, 5, 7), (8193, 5, 7), (7169, 66, 130), (6401, 6, 128)]


@pytest.mark.parametrize('rows,M,N', SLAB_SHAPES)
def test_slabs_and_reduce_order(rows, M, N):
    for kind in ('wide', 'integer'):
        op = _ops(kind, rows, M, N)
        A, B = _data(kind, rows, M, N)
        for split in ((True, False) if T.tiling(M, N, M, N) == (2, 2) else (True,)):
            for c_t in (0, 1):
                part = _call(op, 'partial', split=split, c_t=c_t)
                p = part.p
                assert p.nblk in (5, 26, 29, 33)
                prod, cs = T.slabs_of(part.ws, p, M, N)
                if c_t == 0:
                    worst = worst_cs = 0.0
                    for bx in range(p.nblk):
                        r0, r1 = T.block_rows(p, bx)
                        rb = T.ref64(A, B, r0, r1)
                        if kind == 'integer':
                            assert torch.equal(prod[bx].double().cpu(), rb.C) and torch.equal(cs[bx].double().cpu(), rb.cs), (bx, split)
                        else:
                            worst = max(worst, T.err_in_u(prod[bx], rb.C, rb.S))
                            worst_cs = max(worst_cs, T.err_in_u(cs[bx], rb.cs, rb.sa))
                    if kind == 'wide':
                        bar = p.rpw + 2 + 2 if not p.bf16 else 16               # a block: the wave chain and the LDS sum / the project's
                        print(f'[tn slabs {rows}x{M}x{N} bf16={p.bf16}] per-block err / (2^-24 S) = {worst:.3f} of {bar}, colsum {worst_cs:.3f}')
                        assert worst <= bar and worst_cs <= p.rpw // 2 + 3 + 2
                full = _call(op, 'ex', split=split, c_t=c_t, dense=True)
                assert _same(full.C, T.reduce_in_kernel_order(prod)), 'k_tn_reduce does not add in the stated order'
                assert _same(full.cs[0], T.reduce_colsum_in_kernel_order(cs, p.MT))
                fin, fin_cs = _finish_out(part)
                assert _same(fin, full.Cd) and _same(part.Cd, full.Cd) and _same(fin_cs, full.cs[0]) and _same(part.cs[0], full.cs[0])


# One nonzero row per wavefront: A = w_q in every column, B = 1.  fp32 sums of (1, -1, -2^-24, 1.5 2^-24) in the kernel's order
# (w0 + w2) + (w1 + w3) give 2^-24; (w0 + w3) + (w1 + w2) gives 2^-23, (w0 + w1) + (w2 + w3) and the chain ((w0 + w1) + w2) + w3
# give 2^-25, the chains from the other end 0.  Every value is one bf16 piece and every product has one nonzero term: exact on both pipes.
PROBE = (1.0, -1.0, -2.0 ** -24, 1.5 * 2.0 ** -24)


@pytest.mark.parametrize('rows,M,N', [(256, 128, 128), (512, 128, 128), (512, 128, 20), (512, 6, 128), (512, 6, 66), (512, 5, 7), (1280, 128, 128)])
def test_block_adds_its_wavefronts_in_the_stated_order(rows, M, N):
    A, B = torch.zeros(rows, M), torch.zeros(rows, N)
    for split in (True, False):
        p = T.plan(rows, M, N, split=split)
        assert p.rpw == 64 and p.nblk == rows // 256
        for w, (r0, r1) in enumerate(p.waves):
            r = r0 + (5 if w % 2 == 0 else 2) + 8 * (w // 4)              # both lane halves, several steps
            A[r], B[r] = PROBE[w % 4], 1.0
        op = Operands(A, B)
        w = [torch.tensor(v, dtype=torch.float32) for v in PROBE]
        block = (w[0] + w[2]) + (w[1] + w[3])
        assert float(block) == 2.0 ** -24
        want = T.reduce_in_kernel_order(block.repeat(p.nblk, 1))[0]
        want_cs = T.reduce_colsum_in_kernel_order(block.repeat(p.nblk, 1), p.MT)[0]
        for c_t in (0, 1):
            o = _call(op, split=split, c_t=c_t)
            assert bool((o.C == want).all()) and bool((o.cs == want_cs).all()), (split, float(o.C[0, 0]), float(want), float(o.cs[0, 0]))


def test_grad_finish_mixes_sourced_and_direct_tensors():
    rows, M, N = 1025, 66, 130
    op = _ops('wide', rows, M, N)
    part, full = _call(op, 'partial'), _call(op, 'ex', dense=True)
    Ar = Arena()
    sizes = [1023, 1024, 1027]
    g = torch.Generator(device='cuda').manual_seed(5)
    direct = [Ar.inp(torch.randn(n, device='cuda', generator=g)) for n in sizes]
    dsts = [Ar.out(n + 1) for n in sizes]
    dst_v = [dsts[0][1:], dsts[1][:1024], dsts[2][1:]]                     # 4 bytes off, aligned, 4 bytes off
    finC, fincs = Ar.out(M, N), Ar.out(M)
    D = [finC, dst_v[0], fincs, dst_v[1], dst_v[2]]
    G = [part.Cd, direct[0], part.cs[0], direct[1], direct[2]]
    n = len(D)
    Dp, Gp, Np, S = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int64 * n)(), (_lib().KgwGradSrc * n)()
    for k in range(n):
        Dp[k], Gp[k], Np[k] = D[k].data_ptr(), G[k].data_ptr(), G[k].numel()
    C.memmove(C.byref(S[0]), C.byref(part.src[0]), C.sizeof(_lib().KgwGradSrc))
    C.memmove(C.byref(S[2]), C.byref(part.src[1]), C.sizeof(_lib().KgwGradSrc))
    assert _L().kgw_grad_finish(n, Dp, Gp, Np, S, _st()) == OK
    Ar.check()
    part.arena.check()
    assert _same(finC, full.Cd) and _same(part.Cd, full.Cd) and _same(fincs, full.cs[0]) and _same(part.cs[0], full.cs[0])
    for k in range(3):
        assert _same(dst_v[k][:sizes[k]], direct[k])
    assert bool(torch.isnan(dsts[0][0])) and bool(torch.isnan(dsts[1][1024])) and bool(torch.isnan(dsts[2][0]))


# ====================================================== F. grouped and carried forms =========================================

GROUP = [(257, 128, 128, 0, True), (1025, 64, 192, 1, False), (1, 128, 20, 0, True), (2049, 192, 64, 1, True)]      # rows, M, N, c_t, colsum
SECOND = [(513, 64, 66, 0, True), (1281, 128, 128, 1, True)]


class Group:
    """Jobs of the grouped forms with fresh outputs: dense C (the partial forms need it), colsum_repeat 1."""

    def __init__(self, specs, split=True, kind='wide'):
        self.specs, self.Ar = specs, Arena()
        self.jobs = (_lib().KgwTnJob * max(len(specs), 1))()
        self.src = (_lib().KgwGradSrc * max(2 * len(specs), 1))()
        self.outs, self.plans, self.ops = [], [], []
        for q, (rows, M, N, c_t, colsum) in enumerate(specs):
            op = _ops(kind, rows, M, N)
            p = T.plan(rows, M, N, split=split, forced=(2, 2))
            o = dict(C=self.Ar.out(N, M) if c_t else self.Ar.out(M, N), cs=self.Ar.out(M) if colsum else None, ws=self.Ar.out(p.need))
            j = self.jobs[q]
            j.A, j.lda, j.B, j.ldb, j.rows = op.A.data_ptr(), op.lda, op.B.data_ptr(), op.ldb, rows
            j.C, j.ldc = o['C'].data_ptr(), (M if c_t else N)
            j.colsum_a, j.colsum_ld, j.colsum_repeat = (o['cs'].data_ptr() if colsum else None), M, 1
            j.workspace, j.workspace_floats, j.rows_dev = o['ws'].data_ptr(), p.need, None
            j.M, j.N, j.c_transposed = M, N, c_t
            self.outs.append(o)
            self.plans.append(p)
            self.ops.append(op)

    def check(self):
        self.Ar.check()
        for op in self.ops:
            op.check()

    def same(self, other, qs=None):
        for q in (range(len(self.specs)) if qs is None else qs):
            a, b = self.outs[q], other.outs[q]
            assert _same(a['C'], b['C']), q
            assert a['cs'] is None or _same(a['cs'], b['cs']), q

    def pending(self):
        """C and the column sums of the jobs with more than one row block are still NaN, the others complete."""
        for o, p in zip(self.outs, self.plans):
            if p.nblk > 1:
                assert _untouched(o['C'], NAN) and (o['cs'] is None or _untouched(o['cs'], NAN))
            else:
                assert bool(torch.isfinite(o['C']).all())


def _plan_ptr(plan):
    return C.cast(C.pointer(plan), C.c_void_p)


@functools.lru_cache(maxsize=None)
def _group_ref(specs, split=True):
    """kgw_tn_gemm_multi on the jobs: the bits every other grouped or carried form must leave."""
    g = Group(list(specs), split)
    with knobs(split):
        assert _L().kgw_tn_gemm_multi(len(specs), g.jobs, _st()) == OK
    g.check()
    return g


def _tbwd(g, ride=None, defer=None, split=True):
    with knobs(split):
        rc = _L().kgw_transform_bwd_ex(len(g.specs), g.jobs, 0, None, 0, None, None if ride is None else _plan_ptr(ride),
                                       None if defer is None else _plan_ptr(defer), None, _st())
    assert rc == OK, rc
    g.check()


@pytest.mark.parametrize('n', [1, 2, 3, 4])
def test_multi_matches_single_calls_and_float64(n):
    specs = tuple(GROUP[:n])
    for split in (True, False):
        g = _group_ref(specs, split)
        for q, (rows, M, N, c_t, colsum) in enumerate(specs):
            one = _group_ref((specs[q],), split)
            assert _same(g.outs[q]['C'], one.outs[0]['C']) and (not colsum or _same(g.outs[q]['cs'], one.outs[0]['cs']))
            if n < 4 and q < n - 1:
                continue
            op, ref, p = g.ops[q], _ref('wide', rows, M, N), g.plans[q]
            ex = _call(op, 'ex', split=split, c_t=c_t, colsum=colsum, dense=True)
            o = Out()
            o.p, o.C, o.cs = p, (g.outs[q]['C'].t() if c_t else g.outs[q]['C']), (g.outs[q]['cs'].view(1, -1) if colsum else None)
            tag = f'multi job {q} {rows}x{M}x{N}'
            if split:
                c32 = _group_ref(specs, False).outs[q]['C']
                e32 = T.err_in_u(c32.t() if c_t else c32, ref.C, ref.S)
                _check_bf16(tag, o, ref, e32, colsum)
            else:
                _check_fp32(tag, o, ref, colsum)
            if (ex.p.MT, ex.p.NT) == (2, 2):
                assert _same(ex.C, o.C) and (not colsum or _same(ex.cs, o.cs)), 'the grouped call against kgw_tn_gemm_ex'
            else:
                assert (ex.p.MT, ex.p.NT) == (2, 1) and (M, N) == (128, 20)       # other bits: both are held to float64
                _check_fp32(tag + ' ex <2,1>', ex, ref, colsum)


def test_multi_partial_and_finish():
    specs = tuple(GROUP)
    ref = _group_ref(specs)
    g = Group(list(specs))
    with knobs():
        assert _L().kgw_tn_gemm_multi_partial(4, g.jobs, g.src, _st()) == OK
    g.check()
    g.pending()
    for q, p in enumerate(g.plans):
        W, Bc = g.src[2 * q], g.src[2 * q + 1]
        assert (W.kind, Bc.kind) == ((TN, TN_COLSUM if specs[q][4] else DIRECT) if p.nblk > 1 else (DIRECT, DIRECT))
        if p.nblk > 1:
            assert (W.nblk, W.MT, W.NT, W.gy, W.gz, W.c_transposed, W.ws) == (p.nblk, 2, 2, p.gy, p.gz, specs[q][3], g.outs[q]['ws'].data_ptr())
            assert Bc.kind == DIRECT or Bc.ws == W.ws + 4 * p.cs_off
    fins = Arena()
    outs = [dict(C=o['C'], fin=fins.out(*o['C'].shape), cs=o['cs'], fin_cs=None if o['cs'] is None else fins.out(*o['cs'].shape)) for o in g.outs]
    _finish(outs, g.src)
    fins.check()
    g.check()
    g.same(ref)
    for o, r in zip(outs, ref.outs):
        assert _same(o['fin'], r['C']) and (o['cs'] is None or _same(o['fin_cs'], r['cs']))


@pytest.mark.parametrize('split', [True, False], ids=['bf16', 'fp32'])
def test_transform_bwd_products_and_the_carried_plan(split):
    specs, second = tuple(GROUP), tuple(SECOND)
    ref, ref2 = _group_ref(specs, split), _group_ref(second, split)
    Plan = _lib().KgwTnReducePlan
    # no plan asked for: both launches
    g = Group(list(specs), split)
    _tbwd(g, split=split)
    g.same(ref)
    # the plan handed out; kgw_tn_reduce_launch runs it
    g, plan = Group(list(specs), split), Plan()
    _tbwd(g, defer=plan, split=split)
    assert plan.valid == 1 and plan.blocks == 64 * max(p.gy for p in g.plans) * max(p.gz for p in g.plans) * len(specs)
    g.pending()
    assert _L().kgw_tn_reduce_launch(_plan_ptr(plan), _st()) == OK
    g.check()
    g.same(ref)
    # every product with one row block: nothing pending
    small = ((1, 128, 20, 0, True), (256, 128, 128, 1, True))
    gs, ps = Group(list(small), split), Plan()
    ps.valid = 7
    _tbwd(gs, defer=ps, split=split)
    assert ps.valid == 0
    gs.same(_group_ref(small, split))
    # the plan rides in a second kgw_transform_bwd_ex
    g, plan = Group(list(specs), split), Plan()
    _tbwd(g, defer=plan, split=split)
    g2 = Group(list(second), split)
    _tbwd(g2, ride=plan, split=split)
    g.check()
    g.same(ref)
    g2.same(ref2)
    # ... in kgw_tn_gemm_partial_ride on a <2,2> product (blocks in front) and on a <2,1> product (a launch of its own ahead)
    for rows, M, N in ((1025, 128, 128), (3073, 128, 20)):
        op = _ops('wide', rows, M, N)
        plain = _call(op, 'partial', split=split)
        g, plan = Group(list(specs), split), Plan()
        _tbwd(g, defer=plan, split=split)
        assert plan.valid == 1
        rode = _call(op, 'ride', split=split, ride=plan)
        g.check()
        g.same(ref)
        assert _same(rode.ws, plain.ws) and _untouched(rode.Cd, NAN)
        _src_matches_twin(rode)
        fin, fin_cs = _finish_out(rode)
        full = _call(op, 'ex', split=split, dense=True)
        assert _same(fin, full.Cd) and _same(fin_cs, full.cs[0])
        # a plan that is not valid: the plain call
        empty = Plan()
        none = _call(op, 'ride', split=split, ride=empty)
        null = _call(op, 'ride', split=split, ride=None)
        assert _same(none.ws, plain.ws) and _same(null.ws, plain.ws)
    g3 = Group(list(second), split)
    _tbwd(g3, ride=Plan(), split=split)
    g3.same(ref2)


# ====================================================== G. pipes =============================================================

@pytest.mark.parametrize('rows,M,N', [(3520, 128, 1408), (8193, 128, 128)])
def test_bf16_pipe_has_no_one_sided_error_on_positive_data(rows, M, N):
    op = _ops('positive', rows, M, N)
    ref = _ref('positive', rows, M, N)
    o3, o32 = _call(op, split=True), _call(op, split=False)
    assert o3.p.bf16 and not o32.p.bf16
    e3, e32 = o3.C.double().cpu() - ref.C, o32.C.double().cpu() - ref.C
    m3, m32, a3, a32 = e3.mean().item(), e32.mean().item(), e3.abs().mean().item(), e32.abs().mean().item()
    print(f'[tn bias {rows}x{M}x{N}] mean error {m3:.3e} (fp32 pipe {m32:.3e}), mean |error| {a3:.3e} ({a32:.3e}), mean result {ref.C.mean().item():.1f}')
    assert abs(m3) <= max(2.0 * abs(m32), 0.1 * a3), (m3, m32)
    assert a3 <= 1.25 * a32, (a3, a32)


# ====================================================== H. refusals ==========================================================

def test_refusals_write_nothing():
    op = _ops('wide', 1025, 128, 128)
    for entry in ('ex', 'partial', 'gemm'):
        for null in ('A', 'B', 'C', 'ws'):
            _call(op, entry, null=null, expect=E_NULL)
        _call(op, entry, x_rows=0, expect=E_RANGE)
        _call(op, entry, x_M=0, expect=E_RANGE)
        _call(op, entry, x_lda=127, expect=E_RANGE)
        _call(op, entry, x_ldc=127, expect=E_RANGE)
    _call(op, 'ex', c_t=1, x_ldc=127, expect=E_RANGE)
    _call(op, 'ex', x_rep=0, expect=E_RANGE)
    _call(op, 'ex', rep=2, x_cs_ld=127, expect=E_RANGE)
    _call(op, 'partial', null='src', expect=E_NULL)
    _call(op, 'ride', null='src', expect=E_NULL)
    _call(op, 'partial', dense=False, expect=E_UNSUPPORTED)
    _call(op, 'partial', c_t=1, dense=False, expect=E_UNSUPPORTED)


def _grouped_forms(g):
    L = _L()
    yield L.kgw_tn_gemm_multi(len(g.specs), g.jobs, _st())
    yield L.kgw_tn_gemm_multi_partial(len(g.specs), g.jobs, g.src, _st())
    yield L.kgw_transform_bwd_ex(len(g.specs), g.jobs, 0, None, 0, None, None, None, None, _st())


def _nothing_written(g):
    g.check()
    for o in g.outs:
        assert _untouched(o['C'], NAN) and (o['cs'] is None or _untouched(o['cs'], NAN)) and _untouched(o['ws'], NAN)


def test_refusals_of_the_grouped_forms():
    L = _L()
    five = Group([GROUP[0]] * 5)
    assert L.kgw_tn_gemm_multi(5, five.jobs, _st()) == E_RANGE and L.kgw_tn_gemm_multi_partial(5, five.jobs, five.src, _st()) == E_RANGE
    assert L.kgw_transform_bwd_ex(5, five.jobs, 0, None, 0, None, None, None, None, _st()) == E_RANGE
    _nothing_written(five)
    g = Group(list(GROUP[:2]))
    assert L.kgw_tn_gemm_multi_partial(2, g.jobs, None, _st()) == E_NULL
    assert L.kgw_tn_gemm_multi(2, None, _st()) == E_NULL
    _nothing_written(g)

    def bad(change, want, q=1):
        g = Group(list(GROUP[:2]))
        change(g.jobs[q])
        for rc in _grouped_forms(g):
            assert rc == want, (rc, want)
        _nothing_written(g)

    bad(lambda j: setattr(j, 'M', 63), E_UNSUPPORTED)
    bad(lambda j: setattr(j, 'N', 191), E_UNSUPPORTED)
    bad(lambda j: setattr(j, 'lda', 65), E_UNSUPPORTED)
    bad(lambda j: setattr(j, 'A', j.A + 4), E_UNSUPPORTED)
    bad(lambda j: setattr(j, 'B', j.B + 4), E_UNSUPPORTED)
    bad(lambda j: setattr(j, 'rows', 0), E_RANGE)
    bad(lambda j: setattr(j, 'lda', 62), E_RANGE)
    bad(lambda j: setattr(j, 'colsum_repeat', 0), E_RANGE, q=0)
    bad(lambda j: setattr(j, 'workspace_floats', j.workspace_floats - 1), E_RANGE)
    bad(lambda j: setattr(j, 'C', None), E_NULL)
    # the partial form needs a dense gradient tensor
    g = Group(list(GROUP[:2]))
    g.jobs[1].ldc += 2
    assert L.kgw_tn_gemm_multi_partial(2, g.jobs, g.src, _st()) == E_UNSUPPORTED
    _nothing_written(g)
