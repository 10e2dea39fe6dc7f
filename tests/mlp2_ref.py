"""Plain float64 references of the fused two-layer MLP kernels (kgwas_amd/csrc/kgw_dense_linear.h: kgw_mlp2_fwd, kgw_mlp2w_fwd,
kgw_mlp2_bwd_first, kgw_mlp2_bwd_first_packed) and the error measures tests/test_gpu_mlp2_kernels.py holds them to.  No GPU
code: torch tensors on whatever device they arrive on (float64 throughout), numpy for the operand image.

Every error is RELATIVE TO sum |a||b| of the dot product that made the element (what every rounding-error bound of a dot product
is relative to, tests/test_gpu_gemm3.py): an element whose scale is zero -- a masked gradient, a row of zeros -- has no
rounding to forgive and must be exact."""
import numpy as np
import torch

from tests.test_split3_bound import bf16_rne, split3          # the numpy restatement of kgw_split3x8

U = 2.0 ** -24                                          # unit round-off of fp32


def _d(t):
    return None if t is None else t.double()


def ref_fwd(X, W1, b1, W2, b2):
    """h = relu(relu(X W1^T + b1) W2^T + b2) in float64.  Returns z1, h1, s1, z2, h2, s2 with the per-element scales
    s1 = |X||W1|^T + |b1| and s2 = h1 |W2|^T + |b2| (h1 >= 0).  b1 / b2 may be None."""
    X, W1, b1, W2, b2 = _d(X), _d(W1), _d(b1), _d(W2), _d(b2)
    z1 = X @ W1.t()
    s1 = X.abs() @ W1.abs().t()
    if b1 is not None:
        z1 = z1 + b1
        s1 = s1 + b1.abs()
    h1 = torch.relu(z1)
    z2, s2 = ref_second(h1, W2, b2)
    return z1, h1, s1, z2, torch.relu(z2), s2


def ref_second(H1, W2, b2):
    """The second product alone, from a GIVEN hidden state (the one a kernel wrote): z2 = H1 W2^T + b2 and its scale
    |H1||W2|^T + |b2|."""
    H1, W2, b2 = _d(H1), _d(W2), _d(b2)
    z2 = H1 @ W2.t()
    s2 = H1.abs() @ W2.abs().t()
    if b2 is not None:
        z2 = z2 + b2
        s2 = s2 + b2.abs()
    return z2, s2


def ref_bwd(dH2, W2, H1, X, K1, in_ids=None, rows_real=None):
    """D = (dH2[src] W2) * (H1 > 0) -- rows with in_ids < 0 zero, src = in_ids (or the row itself) --, dW1 = D^T X [128, K1],
    db1 = colsum D, over the first ``rows_real`` rows (default: all), in float64.  The mask is `> 0` and nothing else: H1 is
    any matrix, +0.0 and -0.0 both mask.  Returns D, sD, dW1, sW, db1, sb with the scales sD = |dH2[src]||W2| (masked like D),
    sW = |D|^T |X|, sb = colsum |D|.  K1 = 0: dW1 and sW are [128, 0]."""
    dH2, W2, H1 = _d(dH2), _d(W2), _d(H1)
    rows = H1.shape[0]
    n = rows if rows_real is None else max(0, min(int(rows_real), rows))
    H1 = H1[:n]
    if in_ids is not None:
        ids = in_ids[:n].long()
        keep = ids >= 0
        G = dH2[ids.clamp(min=0)]
    else:
        keep = torch.ones(n, dtype=torch.bool, device=H1.device)
        G = dH2[:n]
    m = ((H1 > 0) & keep[:, None]).double()
    D = (G @ W2) * m
    sD = (G.abs() @ W2.abs()) * m
    if K1 > 0:
        Xr = _d(X)[:n, :K1]
        dW1, sW = D.t() @ Xr, D.abs().t() @ Xr.abs()
    else:
        dW1 = sW = D.new_zeros(D.shape[1], 0)
    return D, sD, dW1, sW, D.sum(0), D.abs().sum(0)


def scale_bwd_whole(sD, X, K1):
    """sum_r sum_o |dH2[src r, o]||W2[o, c]| m[r, c] |x'[r, k]|, x' = [x | 1]: sum |a||b||c| of dW1 | db1 [128, K1 + 1] taken as ONE
    dot product over (r, o) -- the scale that bounds the roundings of both products of kgw_mlp2_bwd_first (|D| <= sD)."""
    n = sD.shape[0]
    Xp = torch.cat([_d(X)[:n, :K1].abs(), torch.ones(n, 1, dtype=torch.float64, device=sD.device)], dim=1) if K1 > 0 else \
        torch.ones(n, 1, dtype=torch.float64, device=sD.device)
    return sD.t() @ Xp


def rel_err(got, ref, scale):
    """max |got - ref| / scale; where scale == 0 the element must EQUAL the reference (no division, no tolerance): the
    function raises AssertionError there otherwise.  A non-finite `got` gives inf."""
    got, ref, scale = _d(got), _d(ref), _d(scale)
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    zero = scale == 0
    if bool(zero.any()):
        bad = zero & (got != ref)
        assert not bool(bad.any()), f'{int(bad.sum())} elements of scale 0 differ from the reference'
    err = (got - ref).abs() / torch.where(zero, torch.ones_like(scale), scale)
    err = torch.where(zero, torch.zeros_like(err), err)
    return float(err.max())


# ---- kgw_gemm3's B operand image, s_is_kn form --------------------------------------------------------------------------------
# uint4 index (((tile * 2 + j) * 3 + p) * 4 + nt) * 64 + lane holds the eight bf16 (i = 0..7, low half-word first) of piece p
# of rows 32 tile + 16 j + 8 (lane >> 5) + i, column 32 nt + (lane & 31): the map of the PACK branch of k_mlp2_bwd_first3, and of
# k_g3_pack.

def _as_u8(buf):
    if torch.is_tensor(buf):
        buf = buf.detach().cpu().numpy()
    if not isinstance(buf, np.ndarray):
        buf = np.frombuffer(bytes(buf), dtype=np.uint8)
    return np.ascontiguousarray(buf).view(np.uint8).reshape(-1)


def decode_g3_image(buf, rows32):
    """The fp32 matrix [rows32, 128] an image holds: the three bf16 pieces of every element added (exactly: the pieces of an
    fp32 value sum to it in float64, and the sum is an fp32 number)."""
    assert rows32 % 32 == 0
    u8 = _as_u8(buf)
    assert u8.size == rows32 // 32 * 2 * 3 * 4 * 64 * 16, (u8.size, rows32)
    h = u8.view('<u2').reshape(rows32 // 32, 2, 3, 4, 2, 32, 8)          # tile, j, piece, nt, lane >> 5, lane & 31, i
    f = (h.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    v = f[:, :, 0] + f[:, :, 1] + f[:, :, 2]                             # tile, j, nt, lk, li, i
    out = v.transpose(0, 1, 3, 5, 2, 4).reshape(rows32, 128)             # (tile, j, lk, i) x (nt, li)
    o32 = out.astype(np.float32)
    assert np.array_equal(o32.astype(np.float64), out)
    return o32


def encode_g3_image(M, flip=0):
    """numpy twin of the packing: M [rows, 128] fp32 -> image bytes (uint8) over rows rounded up to 32 (zero rows behind M), tiles
    with (tile // flip) & 1 set negated (flip = 0: none)."""
    M = np.asarray(M, dtype=np.float32)
    rows = M.shape[0]
    rows32 = (rows + 31) // 32 * 32
    P = np.zeros((rows32, 128), dtype=np.float32)
    P[:rows] = M
    if flip:
        neg = ((np.arange(rows32 // 32) // flip) & 1).astype(bool)
        P = P.reshape(-1, 32, 128).copy()
        P[neg] = -P[neg]
        P = P.reshape(rows32, 128)
    p1, p2, p3, _, _ = split3(P)
    pieces = np.stack([p1, p2, p3])                                       # piece, row, col
    hw = (pieces.view(np.uint32) >> 16).astype('<u2')
    #             piece, tile, j, lk, i, nt, li   ->   tile, j, piece, nt, lk, li, i
    hw = hw.reshape(3, rows32 // 32, 2, 2, 8, 4, 32).transpose(1, 2, 0, 5, 3, 6, 4)
    return np.ascontiguousarray(hw).view(np.uint8).reshape(-1)


__all__ = ['U', 'ref_fwd', 'ref_second', 'ref_bwd', 'scale_bwd_whole', 'rel_err', 'decode_g3_image', 'encode_g3_image', 'bf16_rne', 'split3']
