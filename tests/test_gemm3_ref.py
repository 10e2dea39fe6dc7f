"""tests/gemm3_ref.py held to its own claims on the CPU: the split is exact, the operand-image twin round-trips, the K-range twin
equals the library's host arithmetic, the edge table reaches what it says it reaches, the six-product model is within the bound the
kernel file states -- and the GPU test's operand distribution makes the loss of any ONE kept product visible above its 16 u bar."""
import pytest
import torch

from tests import gemm3_ref as R

U = R.U


def _wide30(n, seed):
    g = torch.Generator().manual_seed(seed)
    return R.wide(g, (n,), 30, 'cpu')


def test_split3_is_exact():
    x = _wide30(1 << 20, 1)
    # values built so that a piece is exactly zero: bf16 numbers (p2 = p3 = 0), 16-bit significands (p3 = 0), a bf16 number plus a
    # far smaller one (a gap of zero bits inside the significand: the remainder skips eight binary places), zeros of both signs
    b = x[:4096].bfloat16().float()
    s16 = b + (b * 2.0 ** -9).bfloat16().float()
    far = b + (b * 2.0 ** -17).bfloat16().float()
    x = torch.cat([x, b, s16, far, torch.tensor([0.0, -0.0, 1.0, -1.0, 1.9999999, 1.0039062, 0.33333334])])
    p1, p2, p3 = R.split3(x)
    assert torch.equal(p1 + p2 + p3, x)                                      # bit for bit (both zeros compare equal: see below)
    assert torch.equal(p1.double() + p2.double() + p3.double(), x.double())
    for p in (p1, p2, p3):
        assert torch.equal(p.bfloat16().float(), p)                          # each piece IS a bf16 number
    n = 1 << 20
    assert not p2[n:n + 4096].any() and not p3[n:n + 4096].any()
    assert p2[n + 4096:n + 8192].any() and not p3[n + 4096:n + 8192].any()
    ax = x.double().abs()
    assert bool((p2.double().abs() <= ax * 2.0 ** -8).all()) and bool((p3.double().abs() <= ax * 2.0 ** -16).all())
    # the sign of zero: -0.0 splits into (-0.0, +0.0, +0.0), what the kernel's subtraction gives
    z = R.split3(torch.tensor([-0.0]))
    assert [torch.signbit(p).item() for p in z] == [True, False, False]


@pytest.mark.parametrize('K,kv', [(32, 32), (64, 57), (544, 544), (544, 1), (544, 0), (1056, 1047)])
@pytest.mark.parametrize('kn', [True, False])
def test_pack_image_round_trips(K, kv, kn):
    g = torch.Generator().manual_seed(K + kv)
    B = R.wide(g, (K, 128), 30, 'cpu')
    S = B[:kv] if kn else B.t().contiguous()[:, :kv]
    img = R.pack_image(S, K, kv, kn)
    assert img.dtype == torch.uint8 and img.numel() == K // 32 * 1536 * 16
    pieces = R.unpack_image(img, K)
    total = pieces[0].double() + pieces[1].double() + pieces[2].double()
    sign = 1.0 - 2.0 * ((torch.arange(K) // 32 // R.FLIP) & 1).double()
    want = B.double() * sign[:, None]
    want[kv:] = 0.0
    assert torch.equal(total, want)                                          # the pieces of every element sum to +-B or to 0
    # without sign periods the image is the plain split, and the negated chunks are its negation piece for piece
    plain = R.unpack_image(R.pack_image(S, K, kv, kn, flip=0), K)
    assert torch.equal(pieces, plain * sign[None, :, None].float())
    # the layout, spot-checked from the formula: element i of slot (((c*2+j)*3+p)*4+nt)*64+lane, low half-word first
    h = img.view(torch.int16)
    Bz = R.dense_b(S, K, kv, kn)
    for c, j, p, nt, lane, i in [(0, 0, 0, 0, 0, 0), (K // 32 - 1, 1, 2, 3, 63, 7), (K // 64, 1, 1, 2, 37, 3), (0, 1, 0, 1, 32, 1)]:
        k, n = 32 * c + 16 * j + 8 * (lane >> 5) + i, 32 * nt + (lane & 31)
        v = Bz[k, n] * (-1.0 if (c // R.FLIP) & 1 else 1.0)
        piece = R.split3(v.reshape(1))[p]
        got = h[((((c * 2 + j) * 3 + p) * 4 + nt) * 64 + lane) * 8 + i]
        assert got.item() == (piece.view(torch.int32) >> 16).to(torch.int16).item(), (c, j, p, nt, lane, i)


def _lib_splits(M, K):
    from kgwas_amd import _lib
    n = int(_lib.lib().kgw_gemm3_workspace_floats(M, K))                      # (host-only: no GPU is touched)
    assert n % (128 * M) == 0
    return n // (128 * M)


def test_splits_is_the_library_s_host_arithmetic():
    for M, K in R.SHAPES + [(608, 800), (4352, 4096), (64, 2048), (32, 32), (32, 4096)]:
        assert R.splits(M, K) == _lib_splits(M, K), (M, K)
    for M in (1, 255, 256, 257, 2048, 4096, 4097, 8192, 8193, 20032, 65536, 65537, 131073):
        for K in (32, 224, 256, 288, 512, 1056, 4064, 4096, 4128, 5120, 20032, 57760):
            assert R.splits(M, K) == _lib_splits(M, K), (M, K)


def _crossings(M, K):
    """Per K range: the loop indices c (relative to the range's first chunk, > 0) at which a sign-period boundary is crossed."""
    b = R.k_bounds(M, K)
    return [[c - c0 for c in range(c0 + 1, c1) if c % R.FLIP == 0] for c0, c1 in zip(b[:-1], b[1:])]


def test_the_edge_table_reaches_what_it_says():
    want_ns = {(1, 32): 1, (31, 64): 1, (33, 96): 1, (255, 256): 1, (256, 512): 2, (257, 544): 2, (600, 800): 3, (320, 1056): 4,
               (64, 1504): 5, (33, 4096): 16, (512, 4128): 16, (33, 19200): 16, (4097, 4096): 15, (32769, 512): 1}
    assert set(want_ns) == set(R.SHAPES)
    for s, ns in want_ns.items():
        assert R.splits(*s) == ns, s
    assert [R.k_bounds(M, K)[-1] for M, K in R.SHAPES[:3]] == [1, 2, 3]                 # nc = 1, 2, 3
    assert R.k_bounds(256, 512) == [0, 8, 16]                                          # second range ends on chunk 15
    assert R.k_bounds(257, 544) == [0, 8, 17] and _crossings(257, 544) == [[], [8]]    # boundary on the LAST chunk, even half
    assert R.grid(600, 800) == (9, 2, 16)                                              # 9 items, per_xcd 2, 7 idle blocks
    assert R.k_bounds(600, 800) == [0, 8, 16, 25]                                      # range 2 starts ON a boundary
    b = R.k_bounds(320, 1056)
    assert b == [0, 8, 16, 24, 33] and _crossings(320, 1056)[3] == [8]                 # boundary 32 on the last chunk
    assert any(c0 // 16 == (c1 - 1) // 16 and (c0 // 16) & 1 for c0, c1 in zip(b[:-1], b[1:]))   # a range wholly negated
    assert R.k_bounds(64, 1504) == [0, 9, 18, 28, 37, 47]
    assert _crossings(64, 1504) == [[], [7], [], [4], []]                              # odd half (c = 7), even half (c = 4)
    assert R.k_bounds(512, 4128)[-1] == 129
    cr = _crossings(33, 19200)
    assert {len(x) for x in cr} == {2, 3} and {e - s for s, e in zip(R.k_bounds(33, 19200)[:-1], R.k_bounds(33, 19200)[1:])} == {37, 38}
    assert R.grid(4097, 4096) == (255, 32, 256)                                        # one idle block
    par = {c & 1 for x in _crossings(4097, 4096) for c in x}
    assert par == {0, 1}
    assert R.grid(32769, 512)[0] == 129 and 512 // 32 // 8 == 2                        # the row tiles limit the ranges, not K
    # the closing flip is taken and not taken, and some tiles * ranges is no multiple of 8
    closing = {((c1 - 1) // 16) & 1 for s in R.SHAPES for c1 in R.k_bounds(*s)[1:]}
    assert closing == {0, 1}
    assert any(R.grid(*s)[0] % 8 for s in R.SHAPES)
    for M, K in R.SHAPES:
        assert len(R.edge_ks(M, K, 128)) == 128                                        # the edges fit one selector B


def test_six_product_model_is_within_the_kernel_file_s_bound():
    A, B = R.wide_operands(64, 1504, 64 + 1504, 'cpu')
    ref, sc = R.ref64(A, B)
    e = R.rel_err(R.six_product_model(A, B), ref, sc)
    print(f'[gemm3 model] six products against float64 at 64 x 1504: {e / U:.3f} u (bound 1.5 u)')
    assert e <= 3 * 2.0 ** -25


def test_a_dropped_product_is_above_the_bar_on_the_gpu_test_s_operands():
    """The proof that the 16 u bar of the GPU test CAN see a lost piece product: on its operand distribution an otherwise exact
    accumulation of five of the six products is already above it.  A condition on the inputs, not a tolerance for the kernel."""
    A, B = R.wide_operands(64, 1504, 64 + 1504, 'cpu')
    ref, sc = R.ref64(A, B)
    for t in range(6):
        e = R.rel_err(R.six_product_model(A, B, drop=t), ref, sc)
        print(f'[gemm3 model] product (A piece {R.TA[t]}, B piece {R.TB[t]}) dropped: {e / U:.3g} u')
        assert e > 16 * U, (t, e / U)


def test_selectors_select():
    ks = R.edge_ks(64, 1504, 128)
    B, coef = R.selector_b(1504, ks)
    assert int((B != 0).sum()) == 128 and bool(((B != 0).sum(0) == 1).all())
    A = R.wide(torch.Generator().manual_seed(2), (5, 1504), 20, 'cpu')
    assert torch.equal(A.double() @ B.double(), A[:, ks].double() * coef)
    A1, km, c1 = R.selector_a(300, 1504, R.edge_ks(64, 1504, 131))
    assert bool(((A1 != 0).sum(1) == 1).all()) and len(set(km.tolist())) > 100
    Bw = R.wide(torch.Generator().manual_seed(3), (1504, 128), 8, 'cpu')
    assert torch.equal(A1.double() @ Bw.double(), Bw[km].double() * c1[:, None])
