"""kgw_gemm3 on the A operand IMAGE (ops.gemm3_image, lda < 0): the resident copies the kernel reads straight into its operand
registers.  Same products in the same order as the row-major route, so every result must be BIT-identical to it: forward with
bias and ReLU, the transposed weight-gradient output, the partial (optimiser-finished) route, ragged row counts, a mode='full'
K, row / K slices of an image (GeneLayerShard's ranges) and a whole training step with the rider blocks."""
import ctypes

import numpy as np
import pytest
import torch


def _unimage(img, M):
    """inverse of ops.gemm3_image: [Mt, nch, 1024] -> the row-major [M, nch * 32] it was built from (zero padding dropped)."""
    Mt, nch, _ = img.shape
    return img.reshape(Mt, nch, 2, 2, 2, 32, 4).permute(0, 5, 1, 2, 4, 3, 6).reshape(Mt * 32, nch * 32)[:M]


def test_image_layout_is_the_operand_order():
    """CPU: float4 q * 64 + lane of (tile t, chunk c) = row 32 t + lane % 32, k = 32 c + 16 (q // 2) + 8 (lane // 32) + 4 (q % 2)."""
    from kgwas_amd import ops
    M, K = 70, 90
    A = torch.arange(M * K, dtype=torch.float32).view(M, K) + 1.0
    img = ops.gemm3_image(A)
    assert img.shape == (3, 3, 1024) and img.is_contiguous()
    f4 = img.view(3, 3, 4, 64, 4)
    for t in range(3):
        for c in range(3):
            for q in range(4):
                for lane in (0, 5, 31, 32, 47, 63):
                    row = 32 * t + lane % 32
                    k0 = 32 * c + 16 * (q // 2) + 8 * (lane // 32) + 4 * (q % 2)
                    want = [float(A[row, k0 + e]) if row < M and k0 + e < K else 0.0 for e in range(4)]
                    assert f4[t, c, q, lane].tolist() == want, (t, c, q, lane)
    assert torch.equal(_unimage(img, M)[:, :K], A)
    assert torch.equal(ops.gemm3_image(A.t()), ops.gemm3_image(A.t().contiguous()))


def _operands(M, K, seed, kn):
    g = torch.Generator(device='cuda').manual_seed(seed)
    A = torch.randn(M, K, device='cuda', generator=g) * torch.exp2(torch.randint(-10, 11, (M, K), device='cuda', generator=g).float())
    B = torch.randn(K, 128, device='cuda', generator=g) / K ** 0.5
    return A, B if kn else B.t().contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize('M,K,kn,transpose', [(20032, 5120, False, False), (5120, 20032, True, True), (4100, 1024, False, False),
                                              (4100, 1024, True, True), (2048, 57760, True, True), (2048, 57760, False, False)])
def test_image_route_is_bit_identical_to_the_row_major_route(M, K, kn, transpose):
    from kgwas_amd import ops
    A, S = _operands(M, K, M + K, kn)
    packed = ops.gemm3_pack(S, K, kn)
    img = ops.gemm3_image(A)
    if transpose:
        ref = ops.gemm3(A, packed, transpose_out=True)
        got = ops.gemm3(img, packed, transpose_out=True, image_rows=M)
    else:
        b = torch.randn(128, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
        ref = ops.gemm3(A, packed, bias=b, relu=True)
        got = ops.gemm3(img, packed, bias=b, relu=True, image_rows=M)
        assert float((ref > 0).float().mean()) > 0.2
    assert torch.equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize('M,K', [(5120, 20032), (4096, 2048)])
def test_image_route_partial_is_bit_identical(M, K):
    """kgw_gemm3_partial (the weight gradient that kgw_adam_fused finishes): same partial sums in the workspace, same record."""
    from kgwas_amd import _lib, ops
    L = _lib.lib()
    A, S = _operands(M, K, 7, True)
    packed = ops.gemm3_pack(S, K, True)
    img = ops.gemm3_image(A)
    nws = int(L.kgw_gemm3_workspace_floats(M, K))
    res = []
    for a, lda in ((A, A.stride(0)), (img, -img.stride(0))):
        ws = torch.full((nws,), float('nan'), device='cuda')
        out = torch.empty(128, M, device='cuda')
        src = _lib.KgwGradSrc()
        _lib.check(L.kgw_gemm3_partial(a.data_ptr(), lda, M, K, packed.data_ptr(), ws.data_ptr(), nws, out.data_ptr(), M, ctypes.byref(src),
                                       _lib.stream_ptr()), 'kgw_gemm3_partial')
        torch.cuda.synchronize()
        res.append((ws, src.kind, src.nblk, src.M, src.N))
    assert res[0][1:] == res[1][1:]
    assert torch.equal(res[0][0], res[1][0])
    assert not bool(torch.isnan(res[1][0]).any())


@pytest.mark.gpu
def test_image_slices_are_the_shard_ranges():
    """GeneLayerShard: rows [lo, hi) of the forward (lo a multiple of 32) and K range [lo, lo + kin) of the weight gradient."""
    from kgwas_amd import ops
    N, K = 4131, 1056
    g = torch.Generator(device='cuda').manual_seed(4)
    X = torch.randn(N, K, device='cuda', generator=g)
    W = torch.randn(128, K, device='cuda', generator=g) / K ** 0.5
    b = torch.randn(128, device='cuda', generator=g)
    dz = torch.randn(N, 128, device='cuda', generator=g)
    Xi, Xt = ops._resident_copies(X)
    assert Xi.shape == (130, 33, 1024) and Xt.shape == (33, 130, 1024)
    packed = ops.gemm3_pack(W, K, False)
    for lo, hi in ((0, 2080), (2080, 4131), (4096, 4131)):
        ref = ops.gemm3(X[lo:hi], packed, bias=b, relu=True)
        got = ops.gemm3(Xi[lo // 32:(hi + 31) // 32], packed, bias=b, relu=True, image_rows=hi - lo)
        assert torch.equal(got, ref), (lo, hi)
    Np = Xt.shape[1] * 32
    XT = torch.nn.functional.pad(X.t(), (0, Np - N))
    for lo, kin in ((0, 2080), (2080, Np - 2080)):
        pk = ops.gemm3_pack(dz[lo:lo + kin], kin, True, k_valid=min(N, lo + kin) - lo)
        ref = ops.gemm3(XT[:, lo:lo + kin], pk, transpose_out=True)
        got = ops.gemm3(Xt[:, lo // 32:(lo + kin) // 32], pk, transpose_out=True, image_rows=K)
        assert torch.equal(got, ref), (lo, kin)


@pytest.mark.gpu
def test_images_are_rebuilt_when_the_matrix_changes_in_place():
    from kgwas_amd import ops
    N, K = 4100, 1056
    X = torch.randn(N, K, device='cuda')
    W = torch.randn(128, K, device='cuda') / K ** 0.5
    b = torch.zeros(128, device='cuda')
    h1, _ = ops.resident_first_linear(X, W, b)
    h1 = h1.clone()
    X.add_(1.0)
    Xi, Xt = ops._resident_copies(X)
    assert torch.equal(Xi, ops.gemm3_image(X)) and torch.equal(Xt, ops.gemm3_image(X.t()))
    h2, _ = ops.resident_first_linear(X, W, b)
    assert not torch.equal(h1, h2)
    assert torch.equal(h2, ops.gemm3(X, ops.gemm3_pack(W, K, False), bias=b, relu=True))


@pytest.fixture(scope='module')
def wide_kg():
    from kgwas_amd.kgwas_data import KGWAS_Data
    # 4 607 genes x 1 024 features: the first gene Linear takes the resident kgw_gemm3 route (>= 4 096 rows, >= 512 wide)
    return KGWAS_Data.from_synthetic(scale=0.23, seed=2, feat_dims={'Gene': 1024}, data_path='/tmp/kgwas_synth_image')


@pytest.mark.gpu
def test_training_step_with_riders_is_bit_identical_on_the_row_major_route(wide_kg, monkeypatch):
    """A whole step (forward with the rider blocks on the product's launch, backward, both gene-layer products): the images against
    the row-major copies they were built from."""
    from kgwas_amd import ops
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.sampler import NeighborLoader
    run = KGWAS(wide_kg, device='cuda:0', seed=9)
    run.initialize_model()
    ids = np.asarray(wide_kg.train_input_nodes[1][:256])
    batch = next(iter(NeighborLoader(wide_kg.data, [-1, -1], ('SNP', ids), batch_size=256, device='cuda:0')))
    ld_w = run._ld_weight_vector()
    run.model.train()
    monkeypatch.setattr(ops, '_G3_RIDERS', True)
    gemm3 = ops.gemm3
    seen = []

    def row_major(A, packed, image_rows=0, **kw):
        if image_rows:
            seen.append(image_rows)
            A = _unimage(A, image_rows)
        return gemm3(A, packed, **kw)

    def step():
        for p in run.model.parameters():
            p.grad = None
        loss, pred = run.model.forward_loss(batch.x_dict, batch.edge_index_dict, 256, batch.n_id('SNP'), batch.dg.y['SNP'], ld_w)
        loss.backward()
        torch.cuda.synchronize()
        return (loss.detach().clone(), pred.detach().clone(), {n: p.grad.clone() for n, p in run.model.named_parameters() if p.grad is not None},
                run.model.last_riders_taken)

    a = step()
    monkeypatch.setattr(ops, 'gemm3', row_major)
    b = step()
    assert len(seen) == 2, 'forward and weight gradient of the gene layer on the image'
    assert a[3] == 1 and b[3] == 1, 'the parameter-only work rode on the forward product'
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys()
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n
