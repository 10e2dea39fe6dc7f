"""Plain references of the kgw_gemm3 family (kgwas_amd/csrc/kgw_gemm3.hip: k_g3_pack, k_g3_gemm, k_g3_reduce, k_g3_reduce_t) for
tests/test_gpu_gemm3_kernels.py: the exact three-way bf16 split, the bit-exact twin of the B operand image, the twin of the host's
K-range arithmetic, one-hot operands whose product is exact in every summation order, and the float64 model of the six piece
products the kernel keeps.  No project kernels: torch tensors on whatever device they arrive on, float64 where something is
computed.  tests/test_gemm3_ref.py holds this file to its own claims on the CPU."""
import torch

U = 2.0 ** -24                      # unit round-off of fp32
FLIP = 16                           # G3_FLIP: 32-k chunks per sign period of the accumulation
NW = 8                              # wavefronts per block of the build (g3_nw): 256-row tiles
MAX_ITEMS = 512                     # G3_MAX_ITEMS
# (piece of A, piece of B) of the six products the kernel keeps, in its order: smallest first (compute / compute_img)
TA = (0, 2, 1, 0, 1, 0)
TB = (2, 0, 1, 1, 0, 0)


def split3(x):
    """The three bf16 pieces of an fp32 tensor, as fp32: p1 + p2 + p3 == x exactly (kgw_split3x8)."""
    x = x.float()
    p1 = x.bfloat16().float()
    r = x - p1
    p2 = r.bfloat16().float()
    p3 = (r - p2).bfloat16().float()
    return p1, p2, p3


def dense_b(S, K, k_valid, s_is_kn):
    """B [K, 128] of a product from what kgw_gemm3_pack is given: S = B[:k_valid] (s_is_kn) or B^T[:, :k_valid]; rows at or past
    k_valid are zero."""
    S = S.float()
    B = torch.zeros(K, 128, dtype=torch.float32, device=S.device)
    if k_valid > 0:
        B[:k_valid] = S[:k_valid, :128] if s_is_kn else S[:128, :k_valid].t()
    return B


def pack_image(S, K, k_valid, s_is_kn, flip=FLIP):
    """Bit-exact twin of k_g3_pack, as a uint8 tensor of K / 32 * 1536 * 16 bytes.  bf16 element i of the 16-byte slot
    (((c * 2 + j) * 3 + p) * 4 + nt) * 64 + lane is piece p of B[32 c + 16 j + 8 (lane >> 5) + i, 32 nt + (lane & 31)], the low
    half of each 32-bit word first; chunks c with (c // flip) & 1 hold the pieces of the NEGATED value (negated first, then
    split, as the kernel does: a zero row of such a chunk is -0.0, whose first piece has the sign bit set)."""
    assert K > 0 and K % 32 == 0 and 0 <= k_valid <= K
    B = dense_b(S, K, k_valid, s_is_kn)
    nch = K // 32
    if flip:
        neg = ((torch.arange(nch, device=B.device) // flip) & 1).bool()
        B = B.view(nch, 32, 128).clone()
        B[neg] = -B[neg]
        B = B.view(K, 128)
    pieces = torch.stack(split3(B))                                        # [p, k, n]
    hw = (pieces.contiguous().view(torch.int32) >> 16).to(torch.int16)    # the bf16 bit patterns
    #        p, c, j, g, i, nt, m   ->   c, j, p, nt, g, m, i      (lane = 32 g + m)
    hw = hw.view(3, nch, 2, 2, 8, 4, 32).permute(1, 2, 0, 5, 3, 6, 4).contiguous()
    return hw.view(torch.uint8).reshape(-1)


def unpack_image(img, K):
    """The three pieces [3, K, 128] (fp32) an image holds: the inverse of pack_image's layout, signs as stored."""
    hw = img.contiguous().view(torch.int16).view(K // 32, 2, 3, 4, 2, 32, 8)          # c, j, p, nt, g, m, i
    f = (hw.to(torch.int32) << 16).view(torch.float32)
    return f.permute(2, 0, 1, 4, 6, 3, 5).reshape(3, K, 128)


def splits(M, K):
    """Twin of g3_splits: the number of K ranges of an [M, K] x [K, 128] product."""
    tiles = (M + 32 * NW - 1) // (32 * NW)
    nch = K // 32
    return max(1, min((MAX_ITEMS * 4 // NW) // tiles, nch // 8, 16))


def k_bounds(M, K):
    """Twin of the kernel's c0 / c1: the chunk bounds [c_0 = 0, c_1, ..., c_ns = K / 32] of the K ranges."""
    ns, nch = splits(M, K), K // 32
    return [nch * s // ns for s in range(ns + 1)]


def grid(M, K):
    """(items, per_xcd, blocks launched) of the product's launch."""
    items = (M + 32 * NW - 1) // (32 * NW) * splits(M, K)
    per_xcd = (items + 7) // 8
    return items, per_xcd, per_xcd * 8


def edge_ks(M, K, n, flip=FLIP):
    """n values of k for a selector operand: the first and last k of every K range, both sides of every sign-period boundary, the
    first and last k of the product -- and, up to n, a fixed pseudo-random fill that moves through every position inside a chunk.
    Edges first; a list too short for them is an error.  n = None: the edges alone."""
    ks = []
    b = k_bounds(M, K)
    for c0, c1 in zip(b[:-1], b[1:]):
        ks += [32 * c0, 32 * c1 - 1]
    for c in range(flip, K // 32, flip):
        ks += [32 * c - 1, 32 * c]
    ks += [0, K - 1]
    ks = list(dict.fromkeys(ks))
    if n is None:
        return ks                                                          # the edges alone
    assert len(ks) <= n, (len(ks), n)
    x = 12345
    while len(ks) < n:
        x = (x * 1103515245 + 12345) % (1 << 31)
        ks.append((x >> 8) % K)
    return ks


def _coef(n, device):
    i = torch.arange(n, device=device)
    signs = 1.0 - 2.0 * ((i * 7 + 3) % 5 < 2).double()
    exps = ((i * 11) % 17 - 8).double()                                    # -8 .. 8
    return signs, exps


def selector_b(K, ks, signs=None, exps=None, device='cpu'):
    """B [K, 128] with ONE non-zero per column: B[ks[n], n] = signs[n] * 2^exps[n].  Then (A B)[m, n] = +-2^e A[m, ks[n]] exactly,
    in any order of summation.  Returns B (fp32) and the float64 coefficients [128]."""
    assert len(ks) == 128
    s, e = _coef(128, device)
    signs = s if signs is None else torch.as_tensor(signs, dtype=torch.float64, device=device)
    exps = e if exps is None else torch.as_tensor(exps, dtype=torch.float64, device=device)
    coef = signs * torch.exp2(exps)
    B = torch.zeros(K, 128, dtype=torch.float32, device=device)
    B[torch.as_tensor(ks, device=device), torch.arange(128, device=device)] = coef.float()
    return B, coef


def selector_a(M, K, ks, signs=None, exps=None, device='cpu'):
    """A [M, K] one-hot per row: A[m, k(m)] = +-2^e with k(m) = ks[m % len(ks)] (coefficients cycle with the row as well).  Then
    (A B)[m, :] = +-2^e B[k(m), :] exactly.  Returns A, k(m) [M] and the float64 coefficients [M]."""
    rows = torch.arange(M, device=device)
    km = torch.as_tensor(ks, device=device)[rows % len(ks)]
    s, e = _coef(M, device)
    signs = s if signs is None else torch.as_tensor(signs, dtype=torch.float64, device=device)[rows % len(signs)]
    exps = e if exps is None else torch.as_tensor(exps, dtype=torch.float64, device=device)[rows % len(exps)]
    coef = signs * torch.exp2(exps)
    A = torch.zeros(M, K, dtype=torch.float32, device=device)
    A[rows, km] = coef.float()
    return A, km, coef


def ref64(A, B):
    """float64 product and its scale sum_k |a||b| (what every rounding-error bound of a dot product is relative to)."""
    A, B = A.double(), B.double()
    return A @ B, A.abs() @ B.abs()


def six_product_model(A, B, drop=None):
    """float64 sum of the six piece products the kernel keeps -- each bf16 x bf16 product is exact, so this is the value an
    error-free accumulation of the kernel's terms would give.  ``drop``: index into (TA, TB) of one product to leave out."""
    pa = [p.double() for p in split3(A)]
    pb = [p.double() for p in split3(B)]
    out = None
    for t in range(6):
        if t == drop:
            continue
        term = pa[TA[t]] @ pb[TB[t]]
        out = term if out is None else out + term
    return out


def rel_err(got, ref, scale):
    """max |got - ref| / scale over ALL elements; an element of scale 0 must equal the reference.  Non-finite: inf."""
    got, ref, scale = got.double(), ref.double(), scale.double()
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    zero = scale == 0
    assert not bool((zero & (got != ref)).any()), 'an element of scale 0 differs from the reference'
    err = (got - ref).abs() / torch.where(zero, torch.ones_like(scale), scale)
    return float(torch.where(zero, torch.zeros_like(err), err).max())


def wide(g, shape, span, device):
    """randn * 2^randint(-span .. span): every piece of the split carries signal."""
    return torch.randn(shape, device=device, generator=g) * torch.exp2(
        torch.randint(-span, span + 1, shape, device=device, generator=g).float())


def wide_operands(M, K, seed, device):
    """The GPU test's operand distribution: A randn * 2^[-20, 20], B randn * 2^[-8, 8], one row of A and one column of B unlike
    the rest (a transposed or permuted operand cannot pass)."""
    g = torch.Generator(device=device).manual_seed(seed)
    A = wide(g, (M, K), 20, device)
    B = wide(g, (K, 128), 8, device)
    A[M // 2] = A[M // 2].abs() * 32.0
    B[:, 17] = -B[:, 17].abs() / 32.0
    return A, B


# (M, K) of the edge table: the smallest shapes that reach each K-range, sign-period, row and grid edge (facts asserted in
# tests/test_gemm3_ref.py)
SHAPES = [(1, 32), (31, 64), (33, 96), (255, 256), (256, 512), (257, 544), (600, 800), (320, 1056), (64, 1504), (33, 4096),
          (512, 4128), (33, 19200), (4097, 4096), (32769, 512)]
