"""The float64 references tests/test_gpu_mlp2_kernels.py compares the fused MLP kernels with (tests/mlp2_ref.py), checked on the
CPU against what they restate: ref_bwd against float64 autograd of the two layers, decode_g3_image against a numpy encoder of the
operand image built from the split of tests/test_split3_bound.py, rel_err's handling of elements without a scale."""
import numpy as np
import pytest
import torch

from tests import mlp2_ref as R


def _case(rows, K1, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(rows, K1, generator=g, dtype=torch.float64)
    W1 = torch.randn(128, K1, generator=g, dtype=torch.float64)
    b1 = torch.randn(128, generator=g, dtype=torch.float64)
    W2 = torch.randn(128, 128, generator=g, dtype=torch.float64) / 8
    b2 = torch.randn(128, generator=g, dtype=torch.float64)
    up = torch.randn(rows, 128, generator=g, dtype=torch.float64)
    return X, W1, b1, W2, b2, up


@pytest.mark.parametrize('rows,K1', [(37, 20), (5, 1), (64, 31)])
def test_ref_bwd_is_float64_autograd_of_the_two_layers(rows, K1):
    X, W1, b1, W2, b2, up = _case(rows, K1, rows + K1)
    P = [p.clone().requires_grad_() for p in (W1, b1)]
    z1 = X @ P[0].t() + P[1]
    h1 = torch.relu(z1)
    z2 = h1 @ W2.t() + b2
    # no pre-activation near zero: autograd's ReLU masks are then unambiguous
    assert float(z1.detach().abs().min()) > 1e-6 and float(z2.detach().abs().min()) > 1e-6
    torch.relu(z2).backward(up)
    # the kernel's contract: the upstream gradient arrives already multiplied by (h2 > 0)
    dH2 = up * (z2 > 0)
    D, sD, dW1, sW, db1, sb = R.ref_bwd(dH2, W2, h1.detach(), X, K1)
    assert float((dW1 - P[0].grad).abs().max()) <= 1e-12 * float(sW.max())
    assert float((db1 - P[1].grad).abs().max()) <= 1e-12 * float(sb.max())
    assert D.shape == sD.shape == (rows, 128) and dW1.shape == sW.shape == (128, K1)
    assert bool((sD >= D.abs() - 1e-12 * sD).all()) and bool((sD[h1 <= 0] == 0).all())
    sc2 = R.scale_bwd_whole(sD, X, K1)                                         # the whole dot product's scale bounds both others
    assert sc2.shape == (128, K1 + 1) and bool((sc2[:, :K1] >= sW * (1 - 1e-12)).all()) and bool((sc2[:, K1] >= sb * (1 - 1e-12)).all())
    # and the forward reference is the same function
    z1r, h1r, s1, z2r, h2r, s2 = R.ref_fwd(X, W1, b1, W2, b2)
    assert torch.equal(z1r, z1.detach()) and torch.equal(h2r, torch.relu(z2).detach())
    assert bool((s1 >= z1r.abs() * (1 - 1e-12)).all()) and bool((s2 >= z2r.abs() * (1 - 1e-12)).all())


def test_ref_bwd_row_injection_mask_and_real_rows():
    """in_ids: row r reads dH2[in_ids[r]], a negative entry zeroes the row; H1 is any matrix and masks with `> 0` alone (both
    zeros mask); rows_real cuts the sums."""
    g = torch.Generator().manual_seed(3)
    rows, m, K1 = 11, 6, 4
    dH2 = torch.randn(m, 128, generator=g)
    W2 = torch.randn(128, 128, generator=g)
    X = torch.randn(rows, K1, generator=g)
    H1 = torch.randn(rows, 128, generator=g)
    H1[:, 5] = 0.0
    H1[2] = -0.0
    ids = torch.tensor([-1, 3, 0, -1, 5, 1, -7, 2, 4, -1, -1], dtype=torch.int32)
    D, sD, dW1, sW, db1, sb = R.ref_bwd(dH2, W2, H1, X, K1, in_ids=ids)
    want = torch.zeros(rows, 128, dtype=torch.float64)
    for r in range(rows):
        if ids[r] >= 0:
            want[r] = (dH2[ids[r]].double() @ W2.double()) * (H1[r] > 0)
    assert torch.allclose(D, want, rtol=1e-13, atol=0) and bool((D[ids < 0] == 0).all())
    assert bool((D[:, 5] == 0).all()) and bool((D[2] == 0).all()) and bool((sD[:, 5] == 0).all())
    assert torch.allclose(dW1, want.t() @ X.double(), rtol=1e-12, atol=1e-12)
    D7 = R.ref_bwd(dH2, W2, H1, X, K1, in_ids=ids, rows_real=7)
    assert D7[0].shape == (7, 128) and torch.allclose(D7[4], want[:7].sum(0), rtol=1e-12, atol=1e-12)
    D0 = R.ref_bwd(dH2, W2, H1, X, K1, in_ids=ids, rows_real=0)
    assert D0[2].shape == (128, K1) and float(D0[2].abs().max()) == 0 and float(D0[4].abs().max()) == 0
    Dk0 = R.ref_bwd(dH2, W2, H1, None, 0, in_ids=ids)
    assert Dk0[2].shape == (128, 0) and torch.equal(Dk0[4], db1)


def test_rel_err_requires_equality_where_there_is_no_scale():
    ref = torch.tensor([1.0, 0.0, 2.0], dtype=torch.float64)
    sc = torch.tensor([2.0, 0.0, 4.0], dtype=torch.float64)
    assert R.rel_err(torch.tensor([1.5, 0.0, 2.0]), ref, sc) == 0.25
    assert R.rel_err(torch.tensor([1.0, -0.0, 1.0]), ref, sc) == 0.25          # -0.0 equals 0.0
    with pytest.raises(AssertionError):
        R.rel_err(torch.tensor([1.0, 1e-30, 2.0]), ref, sc)
    assert R.rel_err(torch.tensor([1.0, float('nan'), 2.0]), ref, sc) == float('inf')
    assert R.rel_err(torch.zeros(0, 4), torch.zeros(0, 4), torch.zeros(0, 4)) == 0.0


@pytest.mark.parametrize('rows', [1, 33, 70, 96])
@pytest.mark.parametrize('flip', [0, 1, 2])
def test_decode_g3_image_inverts_the_numpy_encoder(rows, flip):
    g = np.random.default_rng(rows * 7 + flip)
    M = (g.standard_normal((rows, 128)) * np.exp2(g.integers(-30, 31, (rows, 128)))).astype(np.float32)
    M[0, 3] = 0.0
    M[rows - 1, 127] = np.float32(1.00390625 + 2.0 ** -16)                     # all three pieces non-zero
    rows32 = (rows + 31) // 32 * 32
    img = R.encode_g3_image(M, flip)
    assert img.dtype == np.uint8 and img.size == rows32 // 32 * 2 * 3 * 4 * 64 * 16
    out = R.decode_g3_image(img, rows32)
    sign = np.ones(rows32, dtype=np.float32)
    if flip:
        sign[((np.arange(rows32) // 32 // flip) & 1) == 1] = -1.0
    assert np.array_equal(out[:rows], M * sign[:rows, None])                   # bit for bit (value equality: the image has no -0.0 sum)
    assert not out[rows:].any()
    # the index map, spelled out for single elements: uint4 (((tile * 2 + j) * 3 + p) * 4 + nt) * 64 + lane, half-word i
    h = img.view('<u2')
    for r, c in [(0, 0), (rows - 1, 127), (rows // 2, 37)]:
        tile, j, lk, i, nt, li = r // 32, (r % 32) // 16, (r % 16) // 8, r % 8, c // 32, c % 32
        v = 0.0
        for p in range(3):
            u4 = (((tile * 2 + j) * 3 + p) * 4 + nt) * 64 + 32 * lk + li
            v += float((np.array([int(h[u4 * 8 + i]) << 16], dtype=np.uint32)).view(np.float32)[0])
        assert np.float32(v) == M[r, c] * sign[r], (r, c)
