"""The kgw_gemm3 family (kgwas_amd/csrc/kgw_gemm3.hip: k_g3_pack, k_g3_gemm on its row-major, tiled and operand-image routes,
k_g3_reduce, k_g3_reduce_t, kgw_gemm3_partial + the G3T unit of kgw_grad_finish) called at its C ABI and compared with plain
references (tests/gemm3_ref.py) at every K-range, sign-period, row-tile and grid edge -- the shapes of R.SHAPES, whose facts
tests/test_gemm3_ref.py asserts on the CPU.

The bars:
  exact     the operand image against its twin (int16 view); one-hot SELECTOR operands, whose product has one non-zero term per
            output element and is therefore exact in every order of summation -- a skipped or doubled chunk, a wrong sign, row or
            column, a lost piece of either operand shows as a wrong VALUE, not as an error figure; bit-identity between the A routes,
            runs, row / K slices and padding contents; the epilogues against the fp32 sum of the workspace the call left, taken
            in index order in torch; kgw_gemm3_partial's workspace and kgw_grad_finish's result against kgw_gemm3's own;
  project   wide-range operands (A randn * 2^[-20, 20], B randn * 2^[-8, 8]) against float64, relative to sum |a||b| of the
            element's own dot product, no element left out: the two assertions of test_gemm3_matches_float64_as_well_as_fp32 --
            no worse than 1.25 x the device's fp32 product of the same operands (or 4 u), never above 16 u.
            (tests/test_gemm3_ref.py shows that on these operands the loss of any one kept product is above 16 u.)
Every buffer a call must write completely is NaN-filled before it; every element it must not write holds a mark, every strided
row a sentinel (or NaN) behind it, and all of them are checked after the call."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import gemm3_ref as R

pytestmark = pytest.mark.gpu

OK, E_NULL, E_RANGE, E_UNSUPPORTED = 0, -1, -2, -3
GRAD_G3T = 5                                                      # include/kgwas_hip.h: KGW_GRAD_G3T
U = R.U
NAN = float('nan')
SENT = -777.25                                                    # behind every strided row; must survive every call
MARK = 12345.5                                                    # in elements a call must not write
TAIL = 64                                                         # marked floats behind every workspace


def _L():
    from kgwas_amd import _lib
    return _lib.lib()


def _st():
    from kgwas_amd import _lib
    return _lib.stream_ptr()


def _p(t, off=0):
    """Device pointer of a tensor (+ off BYTES); None stays a null pointer."""
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def _strided(M, ld, fill=SENT):
    """A copy of M [rows, cols] with row stride ld, ``fill`` behind every row."""
    rows, cols = M.shape
    buf = torch.full((rows, ld), fill, device='cuda')
    buf[:, :cols] = M
    return buf


def _out(rows, cols, ld, fill=NAN, extra_rows=0):
    """[rows + extra_rows, ld]: ``fill`` where the call writes, the sentinel behind every row, the mark in the extra rows."""
    buf = torch.full((rows + extra_rows, ld), SENT, device='cuda')
    buf[:rows, :cols] = fill
    buf[rows:, :cols] = MARK
    return buf


def _pad_ok(buf, cols, fill=SENT):
    pad = buf[:, cols:]
    return bool(torch.isnan(pad).all()) if fill != fill else bool((pad == fill).all())


def _ws(M, K, short=0):
    """A NaN-filled workspace of exactly kgw_gemm3_workspace_floats(M, K) floats (minus ``short``) + a marked tail."""
    n = R.splits(M, K) * M * 128
    assert n == int(_L().kgw_gemm3_workspace_floats(M, K))
    buf = torch.full((n - short + TAIL,), NAN, device='cuda')
    buf[n - short:] = MARK
    return buf, n - short


def _ws_ok(buf, n):
    return bool((buf[n:] == MARK).all())


# ================================================ A. kgw_gemm3_pack =================================================

def _pack_raw(S_ptr, lds, K, kv, kn, expect=OK, misalign=0):
    nb = max(K, 32) // 32 * 1536 * 16
    buf = torch.full((nb + 32,), 0xFF, dtype=torch.uint8, device='cuda')          # (0xFFFF: a bf16 NaN in every element)
    buf[nb:] = 0xA5
    rc = _L().kgw_gemm3_pack(S_ptr, lds, K, kv, 1 if kn else 0, _p(buf, misalign), _st())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert bool((buf[nb:] == 0xA5).all())
    if expect != OK:
        assert bool((buf[:nb] == 0xFF).all())                                      # nothing was launched
    return buf[:nb]


def _pack(B, kn=True):
    K = B.shape[0]
    S = B.contiguous() if kn else B.t().contiguous()
    return _pack_raw(_p(S), S.stride(0), K, K, kn)


PACK_FORMS = ['kn', 'kn_strided', 'nk_vector', 'nk_lds_odd', 'nk_misaligned']


@pytest.mark.parametrize('form', PACK_FORMS)
@pytest.mark.parametrize('K', [32, 64, 512, 544, 1056])
def test_pack_is_the_twin_bit_for_bit(K, form):
    """k_valid on both sides of the vector / element boundary k0 + 8 <= k_valid, 1 and 0; S = B^T on the vector path (contiguous,
    aligned, lds % 4 == 0), with lds % 4 != 0 and with a pointer 4 bytes off alignment; NaN in everything behind k_valid and in
    the stride padding; chunks from 16 on negated (K = 544, 1056)."""
    g = torch.Generator(device='cuda').manual_seed(K)
    B = R.wide(g, (K, 128), 30, 'cuda')
    for kv in sorted({K, K - 1, K - 7, K - 8, K - 9, K - 32, 1, 0}):
        kn = form.startswith('kn')
        if kn:
            lds = 128 if form == 'kn' else 132
            S = torch.full((K, lds), NAN, device='cuda')
            S[:kv, :128] = B[:kv]
            ptr = _p(S)
        else:
            lds = {'nk_vector': K, 'nk_lds_odd': K + 3, 'nk_misaligned': K + 4}[form]
            flat = torch.full((128 * lds + 8,), NAN, device='cuda')
            off = 1 if form == 'nk_misaligned' else 0
            S = flat[off:off + 128 * lds].view(128, lds)
            S[:, :kv] = B[:kv].t()
            ptr = _p(flat, 4 * off)
            assert (ptr.value % 16 == 0) == (off == 0)
        img = _pack_raw(ptr, lds, K, kv, kn)
        assert not bool(torch.isnan(img.view(torch.bfloat16)).any()), (K, kv, form)
        Sd = S[:, :128] if kn else S
        twin = R.pack_image(Sd, K, kv, kn)                                  # (the twin reads nothing behind k_valid either)
        assert torch.equal(img.view(torch.int16), twin.view(torch.int16)), (K, kv, form)


def test_pack_sizes_and_refusals():
    L = _L()
    for K in (32, 64, 544, 5120):
        assert int(L.kgw_gemm3_packed_bytes(K)) == K // 32 * 1536 * 16
    for K in (0, -32, 1, 31, 33, 40, 1000):
        assert int(L.kgw_gemm3_packed_bytes(K)) == 0
    S = torch.zeros(64, 128, device='cuda')
    assert L.kgw_gemm3_pack(None, 128, 64, 64, 1, _p(S), _st()) == E_NULL
    assert L.kgw_gemm3_pack(_p(S), 128, 64, 64, 1, None, _st()) == E_NULL
    _pack_raw(_p(S), 128, 64, -1, True, expect=E_RANGE)
    _pack_raw(_p(S), 128, 64, 65, True, expect=E_RANGE)
    _pack_raw(_p(S), 128, 0, 0, True, expect=E_RANGE)
    _pack_raw(_p(S), 128, 40, 40, True, expect=E_UNSUPPORTED)
    _pack_raw(_p(S), 128, 64, 64, True, expect=E_UNSUPPORTED, misalign=4)


# ================================================== the product call ==================================================

def _gemm3(A, lda, M, K, packed, ws, nws, out, ldo, bias=None, relu=0, transpose=0, row_map=None, out_rows=None, ld_rows=0,
           out_rows_n=0, real=None, expect=OK, a_off=0):
    rc = _L().kgw_gemm3(_p(A, a_off), lda, M, K, _p(packed), _p(ws), nws, _p(bias), relu, _p(out), ldo, transpose, _p(row_map),
                        _p(out_rows), ld_rows, out_rows_n, _p(real), _st())
    torch.cuda.synchronize()
    assert rc == expect, rc


def _product(A, lda, M, K, packed):
    """kgw_gemm3 without an epilogue -> (C [M, 128], workspace [ns, M, 128]); NaN-filled before, complete after, the rows of the
    output buffer past M and the floats behind the workspace untouched."""
    ws, n = _ws(M, K)
    out = _out(M, 128, 128, extra_rows=40)
    _gemm3(A, lda, M, K, packed, ws, n, out, 128)
    assert _ws_ok(ws, n) and bool((out[M:] == MARK).all())
    assert not bool(torch.isnan(ws[:n]).any()) and not bool(torch.isnan(out[:M]).any())
    return out[:M], ws[:n].view(-1, M, 128)


@functools.lru_cache(maxsize=2)
def _wide_case(M, K):
    """Wide-range operands of one shape, their image and the row-major result every other route is compared with."""
    A, B = R.wide_operands(M, K, 7 * M + K, 'cuda')
    packed = _pack(B, kn=(M + K // 32) % 2 == 0)
    out, ws = _product(A, K, M, K, packed)
    return A, B, packed, out, ws


def _ids(shapes):
    return [f'{m}x{k}' for m, k in shapes]


SHAPES = R.SHAPES


# ===================================================== B. the product =====================================================

def _explain(got, want, k_of, what):
    """Which terms a failed selector comparison lost: the first mismatches with their k, chunk and K range."""
    bad = (got != want).nonzero()
    lines = [f'{what}: {bad.shape[0]} of {got.numel()} elements differ']
    for m, n in bad[:8].tolist():
        k = int(k_of(m, n))
        lines.append(f'  C[{m}, {n}] = {got[m, n].item()!r}, want {want[m, n].item()!r}: k = {k}, chunk {k // 32} '
                     f'(period {k // 32 // R.FLIP}), k % 32 = {k % 32}')
    return '\n'.join(lines)


@pytest.mark.parametrize('M,K', SHAPES, ids=_ids(SHAPES))
def test_selector_b_gives_scaled_columns_of_a_exactly(M, K):
    """B has one non-zero per column, +-2^e at k(n): C[m, n] = +-2^e A[m, k(n)] exactly.  The 128 k's hold the first and last k
    of every K range, both sides of every sign-period boundary and the first and last k of the product."""
    A = _wide_case(M, K)[0]
    ks = R.edge_ks(M, K, 128)
    B, coef = R.selector_b(K, ks, device='cuda')
    for kn in (True, False):
        out, ws = _product(A, K, M, K, _pack(B, kn))
        want = A[:, ks].double() * coef
        assert torch.equal(out.double(), want), _explain(out.double(), want, lambda m, n: ks[n], f'selector B {M}x{K} kn={kn}')
        # one K range holds the term, every other range's partial sum is zero
        assert torch.equal(ws.double().sum(0), want)
        assert int((ws != 0).sum(0).max()) <= 1


@pytest.mark.parametrize('M,K', SHAPES, ids=_ids(SHAPES))
def test_selector_a_gives_scaled_rows_of_b_exactly(M, K):
    """A is one-hot per row, +-2^e at k(m), k(m) cycling over the same edge list (in as many passes as a short matrix needs to
    visit every edge): C[m, :] = +-2^e B[k(m), :] exactly, on the row-major and on the image route."""
    from kgwas_amd import ops
    _, B, packed, _, _ = _wide_case(M, K)
    edges = R.edge_ks(M, K, None)
    ks = R.edge_ks(M, K, max(257, len(edges)))
    for off in range(0, len(edges), M):
        A, km, coef = R.selector_a(M, K, ks[off:] + ks[:off], device='cuda')
        want = B[km].double() * coef[:, None]
        out, _ = _product(A, K, M, K, packed)
        assert torch.equal(out.double(), want), _explain(out.double(), want, lambda m, n: km[m], f'selector A {M}x{K} pass {off}')
        img = ops.gemm3_image(A)
        out, _ = _product(img, -img.stride(0), M, K, packed)
        assert torch.equal(out.double(), want), _explain(out.double(), want, lambda m, n: km[m], f'selector A image {M}x{K} pass {off}')


TWO_PIECE = [(33, 96), (257, 544), (64, 1504), (512, 4128)]


@pytest.mark.parametrize('M,K', TWO_PIECE, ids=_ids(TWO_PIECE))
def test_two_piece_selector_keeps_the_middle_product(M, K):
    """The one-piece selectors above never form the product (a2, b2).  Here A is one-hot with the value +-2^e (1 + 2^-8), whose
    split is a1 = +-2^e, a2 = +-2^(e-8), a3 = 0 (the tie rounds to even): C[m, :] = a B[k(m), :] is then the kernel's chain of
    FIVE products, a1 b3, a2 b2, a1 b2, a2 b1, a1 b1 in that order, in one output element -- no long accumulation, no statistics.
    The bound, relative to |a||b|: the first add is exact, each of the other four commits at most one ulp of its result (2 u: the
    MFMA's add truncates, kgw_gemm3.hip), the partial sums stay below |a||b| (1 + 2^-7), and the one product the kernel drops,
    a2 b3, is at most 2^-8 2^-16 = 1 u: 9 u (1 + 2^-7).  Without a2 b2 the error is up to 2^-16 |a||b| = 256 u."""
    from kgwas_amd import ops
    _, B, packed, _, _ = _wide_case(M, K)
    A, km, coef = R.selector_a(M, K, R.edge_ks(M, K, 257), device='cuda')
    A = A * (1.0 + 2.0 ** -8)
    p1, p2, p3 = R.split3(A)
    assert torch.equal(p1 * 2.0 ** -8, p2) and not p3.any()
    a = coef * (1.0 + 2.0 ** -8)
    want = B[km].double() * a[:, None]
    scale = want.abs()
    bound = 9 * U * (1 + 2.0 ** -7)
    img = ops.gemm3_image(A)
    for name, At, lda in (('row-major', A, K), ('image', img, -img.stride(0))):
        out, _ = _product(At, lda, M, K, packed)
        e = R.rel_err(out, want, scale)
        print(f'[gemm3 two-piece {M}x{K} {name}] {e / U:.3f} u of a bound of {bound / U:.2f} u')
        assert e <= bound, (M, K, name, e / U)


# The two bars of test_gemm3_matches_float64_as_well_as_fp32 -- e3 <= max(1.25 e32, 4 u) and e3 <= 16 u -- were measured at four
# shapes.  Taken over unchanged they are breached at two shapes of the edge table (MI355X, first run of this module, figures in
# profiles/gemm3_kernels/gputests.txt):
#     257 x 544    e3 = 12.87 u against e32 = 7.69 u   (1.25 e32 = 9.6 u)
#     32769 x 512  e3 = 20.15 u, above 16 u            (e32 = 22.32 u: the library's fp32 product is above it as well)
# and at neither is anything wrong with a value: the selector products of the same shapes are exact, the routes bit-identical,
# and an error-free sum of the six kept products is within 0.3 u (tests/test_gemm3_ref.py).  What the figures are is the length of
# the accumulation: with a wide dynamic range one term dominates sum |a||b|, and every rounding after it has entered is up to u
# times the WHOLE scale (the argument of ORDER and _chain_ceiling in tests/test_gpu_mlp2_kernels.py, which met the same thing).
# Both bars therefore get the factor that follows from the summation orders alone -- nothing below is fitted to a result:
#   roundings of the kernel, per output element: 12 MFMAs per 32-k chunk (two k16 steps x six piece products, each an add into an
#       accumulator of full magnitude, whichever pieces it multiplies) over the longest K range, + one add per further range in
#       the epilogue:  Rk = 12 max(c1 - c0) + ns - 1;
#   roundings of the yardstick at its best: a two-level blocked fp32 sum of K terms in blocks of b has (b - 1) + (K / b - 1) + 1
#       (the 7 + 15 + 1 = 23 of ORDER at K = 128), least at b ~ sqrt(K):  Rl = min_b;
#   independent roundings add in quadrature: two correct orders differ by sqrt(Rk / Rl) (never taken below 1), on top of which the
#       project's margin of 1.25 between two realisations of one order stays;
#   the ceiling: Rk roundings, each uniform within +-u of the scale (a truncating add has the same width, its mean is what the sign
#       periods cancel and test_gemm3_has_no_one_sided_error measures): rms sqrt(Rk / 3) u, the largest of N values expected at
#       sqrt(2 ln 2N) times that.  16 u stays wherever it is the larger of the two.
# A lost piece product is still seen: at 64 x 1504 the derived bars are 11.6 u and 28 u, the loss of the smallest product 57 u
# (tests/test_gemm3_ref.py), and the selector tests see all but the (a2, b2) product exactly, test_two_piece_selector that one.
def _roundings(M, K):
    b = R.k_bounds(M, K)
    return 12 * max(c1 - c0 for c0, c1 in zip(b[:-1], b[1:])) + len(b) - 2


def _yardstick_roundings(K):
    return min((b - 1) + (-(-K // b) - 1) + 1 for b in range(1, K + 1))


def _order(M, K):
    return max(1.0, (_roundings(M, K) / _yardstick_roundings(K)) ** 0.5)


def _ceiling(M, K):
    return max(16 * U, (_roundings(M, K) / 3.0) ** 0.5 * (2.0 * math.log(2.0 * M * 128)) ** 0.5 * U)


def _bar(M, K, e3, e32):
    order, ceiling = _order(M, K), _ceiling(M, K)
    print(f'[gemm3 {M}x{K} ns={R.splits(M, K)}] e3 = {e3 / U:.3f} u, e32 = {e32 / U:.3f} u  (u = 2^-24, relative to sum |a||b|; '
          f'order factor {order:.2f}, ceiling {ceiling / U:.1f} u)')
    assert e3 <= max(1.25 * order * e32, 4 * U), (M, K, e3 / U, e32 / U, order)
    assert e3 <= ceiling, (M, K, e3 / U, ceiling / U)


@pytest.mark.parametrize('M,K', SHAPES, ids=_ids(SHAPES))
def test_wide_range_product_matches_float64(M, K):
    """The project's own bars (test_gemm3_matches_float64_as_well_as_fp32, with the summation-order factors derived above) at
    every shape of the edge table, the error relative to sum |a||b| of the element's own dot product, no element left out; twice
    the same bits; exactly ns * M * 128 floats of workspace written (asserted in _product)."""
    A, B, packed, out, ws = _wide_case(M, K)
    ref, sc = R.ref64(A, B)
    _bar(M, K, R.rel_err(out, ref, sc), R.rel_err(A @ B, ref, sc))
    assert ws.shape[0] == R.splits(M, K)
    out2, ws2 = _product(A, K, M, K, packed)
    assert torch.equal(out2, out) and torch.equal(ws2, ws)                   # deterministic


# ===================================================== C. the A routes =====================================================

@pytest.mark.parametrize('M,K', SHAPES, ids=_ids(SHAPES))
def test_routes_are_bit_identical(M, K):
    """Row-major with lda = K + 4 and K + 36 (NaN behind every row), 32 x 32 tiles (lda = 0), the operand image (lda < 0): the
    result AND the workspace of the contiguous row-major call, bit for bit."""
    from kgwas_amd import ops
    A, _, packed, out, ws = _wide_case(M, K)
    for ld in (K + 4, K + 36):
        As = _strided(A, ld, NAN)
        o, w = _product(As, ld, M, K, packed)
        assert _pad_ok(As, K, NAN)
        assert torch.equal(o, out) and torch.equal(w, ws), ld
    o, w = _product(ops.gemm3_tile(A), 0, M, K, packed)
    assert torch.equal(o, out) and torch.equal(w, ws), 'tiled'
    img = ops.gemm3_image(A)
    assert img.stride(0) == K * 32
    o, w = _product(img, -img.stride(0), M, K, packed)
    assert torch.equal(o, out) and torch.equal(w, ws), 'image'


RAGGED = [s for s in SHAPES if s[0] % 32]


@pytest.mark.parametrize('M,K', RAGGED, ids=_ids(RAGGED))
def test_rows_past_m_may_hold_any_value(M, K):
    """include/kgwas_hip.h: in the tiled and image layouts the rows past M are 'present, any value'.  NaN in every one of them:
    the stored rows keep their bits, the output rows at or past M their mark (_product)."""
    from kgwas_amd import ops
    A, _, packed, out, ws = _wide_case(M, K)
    T = ops.gemm3_tile(A)
    T[-1, :, M % 32:, :] = NAN
    o, w = _product(T, 0, M, K, packed)
    assert torch.equal(o, out) and torch.equal(w, ws), 'tiled'
    img = ops.gemm3_image(A)
    f4 = img.view(img.shape[0], K // 32, 4, 2, 32, 4)                           # tile, chunk, q, lane >> 5, lane & 31 = row, e
    f4[-1, :, :, :, M % 32:, :] = NAN
    assert int(torch.isnan(img).sum()) == (32 - M % 32) * K
    o, w = _product(img, -img.stride(0), M, K, packed)
    assert torch.equal(o, out) and torch.equal(w, ws), 'image'


@pytest.mark.parametrize('M,K', SHAPES, ids=_ids(SHAPES))
def test_row_slices_of_an_image(M, K):
    """Tiles [2:] of a taller matrix's image: the row-major product of those rows."""
    from kgwas_amd import ops
    A, _, packed, out, ws = _wide_case(M, K)
    tall = torch.cat([torch.full((64, K), 3.0, device='cuda'), A])
    img = ops.gemm3_image(tall)[2:]
    o, w = _product(img, -img.stride(0), M, K, packed)
    assert torch.equal(o, out) and torch.equal(w, ws)


@pytest.mark.parametrize('c0,c1', [(0, 20), (3, 33), (16, 33), (17, 30)])
def test_k_slices_of_an_image(c0, c1):
    """[:, c0:c1] of an image with the FULL image's tile stride (-lda > K * 32) and a pack of that K range: the row-major product
    on A[:, 32 c0 : 32 c1] (itself a strided view), bit for bit."""
    from kgwas_amd import ops
    M, Kfull = 257, 1056
    A, B = _wide_case(M, Kfull)[:2]
    K = 32 * (c1 - c0)
    Asub, Bsub = A[:, 32 * c0:32 * c1], B[32 * c0:32 * c1]
    packed = _pack(Bsub, kn=True)
    assert Asub.data_ptr() % 16 == 0
    out, ws = _product(Asub, Kfull, M, K, packed)
    ref, sc = R.ref64(Asub, Bsub)
    _bar(M, K, R.rel_err(out, ref, sc), R.rel_err(Asub @ Bsub, ref, sc))
    img = ops.gemm3_image(A)
    sl = img[:, c0:c1]
    assert sl.stride(0) == Kfull * 32 > K * 32
    o, w = _product(sl, -sl.stride(0), M, K, packed)
    assert torch.equal(o, out) and torch.equal(w, ws)


# ===================================================== D. the epilogues =====================================================

EPI_K = {1: 1504, 31: 4096, 33: 800, 257: 544, 600: 800}                       # ns = 5, 16, 3, 2, 3


@functools.lru_cache(maxsize=None)
def _epi_case(M):
    K = EPI_K[M]
    g = torch.Generator(device='cuda').manual_seed(900 + M)
    A = R.wide(g, (M, K), 4, 'cuda')
    B = R.wide(g, (K, 128), 4, 'cuda')
    bias = R.wide(g, (128,), 4, 'cuda') * float((A @ B).abs().median())        # (of the results' size: it moves signs)
    return K, A, _pack(B), bias


def _index_order_sum(ws, ns, M, bias=None, relu=False):
    """ws[0] + ws[1] + ... in fp32, in index order, then + bias, then max(., 0): what the epilogues must equal bit for bit."""
    w = ws.view(ns, M, 128)
    s = w[0].clone()
    for k in range(1, ns):
        s = s + w[k]
    if bias is not None:
        s = s + bias
    return torch.clamp_min(s, 0.0) if relu else s


@pytest.mark.parametrize('M', sorted(EPI_K))
def test_reduce_is_the_index_order_sum_of_the_workspace(M):
    K, A, packed, bias = _epi_case(M)
    ns = R.splits(M, K)
    seen_neg = False
    for use_bias in (False, True):
        for relu in (0, 1):
            for ldo in (128, 132, 256):
                ws, n = _ws(M, K)
                out = _out(M, 128, ldo, extra_rows=3)
                _gemm3(A, K, M, K, packed, ws, n, out, ldo, bias=bias if use_bias else None, relu=relu)
                assert _ws_ok(ws, n) and _pad_ok(out, 128) and bool((out[M:, :128] == MARK).all())
                want = _index_order_sum(ws[:n], ns, M, bias if use_bias else None, relu)
                assert torch.equal(out[:M, :128], want), (use_bias, relu, ldo)
                seen_neg = seen_neg or (relu == 0 and bool((want < 0).any()))
    assert seen_neg                                                            # (the ReLU had something to do)


@pytest.mark.parametrize('M', sorted(EPI_K))
def test_reduce_t_is_the_transposed_index_order_sum(M):
    """k_g3_reduce_t at M % 32 != 0 as well, against the workspace in torch and not against C.t() of the same kernel family."""
    K, A, packed, _ = _epi_case(M)
    ns = R.splits(M, K)
    for ldo in (M, M + 5):
        ws, n = _ws(M, K)
        out = _out(128, M, ldo)
        _gemm3(A, K, M, K, packed, ws, n, out, ldo, transpose=1)
        assert _ws_ok(ws, n) and _pad_ok(out, M)
        assert torch.equal(out[:, :M], _index_order_sum(ws[:n], ns, M).t()), ldo


def _row_map(M, n_sel, n_dst, seed):
    """n_sel random rows of M mapped one-to-one into [0, n_dst), every other row -1."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    rm = torch.full((M,), -1, dtype=torch.int32, device='cuda')
    rows = torch.randperm(M, device='cuda', generator=g)[:n_sel]
    rm[rows] = torch.randperm(n_dst, device='cuda', generator=g)[:n_sel].to(torch.int32)
    return rm


@pytest.mark.parametrize('ld_rows', [128, 136])
@pytest.mark.parametrize('M', sorted(EPI_K))
def test_reduce_row_map_and_padding_rows(M, ld_rows):
    """row_map: the mapped rows of out_rows equal the rows of out, every other element of out_rows keeps its mark;
    out_rows_real: rows [real, out_rows_n) are zero (a negative count is 0), rows past out_rows_n keep the mark."""
    K, A, packed, bias = _epi_case(M)
    ns = R.splits(M, K)
    n_buf = M + 7
    half = M // 2
    #        out_rows_n, real (None: absent), rows mapped
    cases = [(0, None, max(1, half)),                   # absent: a plain gather into a larger buffer
             (M, half, half),                           # real < out_rows_n = M
             (max(half, 1), 0, 0),                      # real = 0, all -1
             (max(half, 1), max(half, 1), max(half, 1)),          # real = out_rows_n: nothing to zero
             (M, -3, 0),                                # a negative count: treated as 0
             (M, M, M)]                                 # out_rows_n = M, every row mapped
    for out_rows_n, real, n_sel in cases:
        n_dst = n_buf if real is None else max(real, 0)
        rm = _row_map(M, n_sel, max(n_dst, 1), M + out_rows_n)
        rd = None if real is None else torch.tensor([real], dtype=torch.int32, device='cuda')
        ws, n = _ws(M, K)
        out = _out(M, 128, 132)
        rows = _out(0, 128, ld_rows, extra_rows=n_buf)                         # all mark
        _gemm3(A, K, M, K, packed, ws, n, out, 132, bias=bias, relu=1, row_map=rm, out_rows=rows, ld_rows=ld_rows,
               out_rows_n=out_rows_n, real=rd)
        want = _index_order_sum(ws[:n], ns, M, bias, True)
        assert _ws_ok(ws, n) and _pad_ok(out, 128) and _pad_ok(rows, 128)
        assert torch.equal(out[:, :128], want)
        exp = torch.full((n_buf, 128), MARK, device='cuda')
        if real is not None:
            exp[max(real, 0):out_rows_n] = 0.0
        sel = rm >= 0
        assert int(sel.sum()) == n_sel
        exp[rm[sel].long()] = want[sel]
        assert torch.equal(rows[:, :128], exp), (out_rows_n, real, n_sel)


# ========================================= E. kgw_gemm3_partial and kgw_grad_finish =========================================

PARTIAL = [(32, 32, 1), (256, 512, 2), (608, 800, 3), (320, 1056, 4), (64, 1504, 5), (64, 2048, 8), (4352, 4096, 15), (32, 4096, 16)]


@pytest.mark.parametrize('M,K,ns', PARTIAL, ids=[f'{m}x{k}-ns{n}' for m, k, n in PARTIAL])
def test_partial_leaves_gemm3_s_workspace_and_grad_finish_its_result(M, K, ns):
    """ns over the edges of the finish's four-load unroll (1, 2, 3, 4, 5, 8, 15, 16).  On every A route: the workspace of
    kgw_gemm3(transpose_out) bit for bit, the record {G3T, ns, M, 128}, ``out`` untouched; kgw_grad_finish then writes ``out``
    and the bucket slot with k_g3_reduce_t's result."""
    from kgwas_amd import _lib, ops
    L = _L()
    assert R.splits(M, K) == ns
    A, B = R.wide_operands(M, K, 3 * M + K, 'cuda')
    packed = _pack(B)
    ws0, n = _ws(M, K)
    out_t = _out(128, M, M)
    _gemm3(A, K, M, K, packed, ws0, n, out_t, M, transpose=1)
    assert torch.equal(out_t, _index_order_sum(ws0[:n], ns, M).t())
    img = ops.gemm3_image(A)
    for name, a, lda in (('row-major', A, K), ('strided', _strided(A, K + 4, NAN), K + 4), ('tiled', ops.gemm3_tile(A), 0),
                         ('image', img, -img.stride(0))):
        ws, _ = _ws(M, K)
        out = torch.full((128, M), MARK, device='cuda')
        src = (_lib.KgwGradSrc * 1)()
        rc = L.kgw_gemm3_partial(_p(a), lda, M, K, _p(packed), _p(ws), n, _p(out), M, src, _st())
        torch.cuda.synchronize()
        assert rc == OK, (name, rc)
        assert _ws_ok(ws, n) and torch.equal(ws[:n], ws0[:n]), name
        s = src[0]
        assert (s.ws, s.kind, s.nblk, s.M, s.N) == (ws.data_ptr(), GRAD_G3T, ns, M, 128), name
        assert not s.packed and s.flip == 0
        assert bool((out == MARK).all()), name
        slot = torch.full((128 * M + 8,), NAN, device='cuda')
        slot[128 * M:] = MARK
        D, G, N = (C.c_void_p * 1)(slot.data_ptr()), (C.c_void_p * 1)(out.data_ptr()), (C.c_int64 * 1)(128 * M)
        rc = L.kgw_grad_finish(1, D, G, N, src, _st())
        torch.cuda.synchronize()
        assert rc == OK, (name, rc)
        assert torch.equal(out, out_t) and torch.equal(slot[:128 * M].view(128, M), out_t), name
        assert bool((slot[128 * M:] == MARK).all()) and torch.equal(ws[:n], ws0[:n])


# ======================================================= F. refusals =======================================================

def test_refusals_write_nothing():
    """-1 null, -2 range, -3 unsupported -- each before any launch: the NaN-filled output and workspace and the marked out_rows
    are as they were."""
    from kgwas_amd import _lib, ops
    L = _L()
    M, K = 64, 256
    A = torch.ones(M + 1, K + 4, device='cuda')
    packed = _pack(torch.ones(K, 128, device='cuda'))
    bias = torch.ones(132, device='cuda')
    rm = torch.zeros(M, dtype=torch.int32, device='cuda')
    rd = torch.zeros(1, dtype=torch.int32, device='cuda')
    img = ops.gemm3_image(torch.ones(M, K + 64, device='cuda'))

    def refused(expect, A_=A, lda=K + 4, M_=M, K_=K, packed_=packed, short=0, no_ws=False, no_out=False, ldo=128, out_off=0, **kw):
        ws, n = _ws(M, K, short=short)
        out = torch.full((M * 256 + 8,), NAN, device='cuda')
        rows = torch.full((M, 128), MARK, device='cuda')
        if kw.pop('rows', False):
            kw['out_rows'], kw['ld_rows'] = rows, 128
        rc = L.kgw_gemm3(_p(A_, kw.pop('a_off', 0)), lda, M_, K_, _p(packed_), None if no_ws else _p(ws), n, _p(kw.get('bias'), kw.get('bias_off', 0)),
                         kw.get('relu', 0), None if no_out else _p(out, out_off), ldo, kw.get('transpose', 0), _p(kw.get('row_map')),
                         _p(kw.get('out_rows')), kw.get('ld_rows', 0), kw.get('out_rows_n', 0), _p(kw.get('real')), _st())
        torch.cuda.synchronize()
        assert rc == expect, (rc, expect, lda, M_, K_, kw)
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws[:n]).all()) and _ws_ok(ws, n) and bool((rows == MARK).all())

    refused(E_NULL, A_=None)
    refused(E_NULL, packed_=None)
    refused(E_NULL, no_ws=True)
    refused(E_NULL, no_out=True)
    refused(E_RANGE, M_=0)
    refused(E_UNSUPPORTED, lda=K + 2)                                          # lda % 4 != 0
    refused(E_UNSUPPORTED, a_off=4)                                            # A not 16-byte aligned
    refused(E_UNSUPPORTED, K_=K - 24)                                          # K % 32 != 0
    refused(E_UNSUPPORTED, A_=img, lda=-(K * 32 + 4))                          # an image stride that is no multiple of 1024
    refused(E_UNSUPPORTED, A_=img, lda=-(K * 32 + 512))
    refused(E_UNSUPPORTED, A_=img, lda=-(K * 32 - 1024))                       # ... or below K * 32
    refused(E_UNSUPPORTED, ldo=130)                                            # non-transposed: ldo % 4, out and bias alignment
    refused(E_UNSUPPORTED, out_off=4)
    refused(E_UNSUPPORTED, bias=bias, bias_off=4)
    refused(E_UNSUPPORTED, transpose=1, ldo=M, bias=bias)                      # transpose with bias, relu or row_map
    refused(E_UNSUPPORTED, transpose=1, ldo=M, relu=1)
    refused(E_UNSUPPORTED, transpose=1, ldo=M, row_map=rm, rows=True)
    refused(E_UNSUPPORTED, row_map=rm)                                         # row_map without out_rows
    refused(E_RANGE, real=rd, rows=True, out_rows_n=M)                         # out_rows_real without row_map
    refused(E_RANGE, real=rd, row_map=rm, rows=True, out_rows_n=M + 1)         # out_rows_n > M
    refused(E_RANGE, short=1)                                                  # a workspace one float short

    # the same call, accepted: the refusals above are the arguments', not the harness's
    ws, n = _ws(M, K)
    out = _out(M, 128, 128)
    _gemm3(A, K + 4, M, K, packed, ws, n, out, 128)
    assert torch.equal(out, torch.full((M, 128), float(K), device='cuda'))

    def partial_refused(expect, M_=M, ldo=M, lda=K + 4, a_off=0, short=0, null=None):
        ws, n = _ws(M, K, short=short)
        out = torch.full((128 * (M + 32),), NAN, device='cuda')
        src = (_lib.KgwGradSrc * 1)()
        src[0].kind = 77
        args = dict(A=_p(A, a_off), packed=_p(packed), ws=_p(ws), out=_p(out), src=src)
        if null:
            args[null] = None
        rc = L.kgw_gemm3_partial(args['A'], lda, M_, K, args['packed'], args['ws'], n, args['out'], ldo, args['src'], _st())
        torch.cuda.synchronize()
        assert rc == expect, (rc, expect, M_, ldo, lda, null)
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws[:n]).all()) and _ws_ok(ws, n) and src[0].kind == 77

    for null in ('A', 'packed', 'ws', 'out', 'src'):
        partial_refused(E_NULL, null=null)
    partial_refused(E_UNSUPPORTED, M_=M - 16)                                  # M % 32 != 0
    partial_refused(E_UNSUPPORTED, M_=M - 16, ldo=M - 16)
    partial_refused(E_UNSUPPORTED, ldo=M + 4)                                  # ldo != M
    partial_refused(E_UNSUPPORTED, lda=K + 2)
    partial_refused(E_UNSUPPORTED, a_off=4)
    partial_refused(E_RANGE, short=1)
