"""k_mlp2_bwd_first3<PACK> (kgwas_amd/csrc/kgw_dense_linear.h) at the edges of its tile loop, with and without the packed image.

The kernel requests its first tile's rows before it builds the W2 operand image, loads the second product's x' column without lane
conditions (clamped rows and columns, selected afterwards), reads the W2 operands a step ahead and hands the masked tile through a
wavefront-private LDS tile: every one of those is wrong first at a row count where a wavefront has no tile, a partial tile, exactly
its tiles or one tile more than its neighbours.  One block is 4 wavefronts x 32 rows and the grid is capped at G = 256 blocks, so
4 * 32 * G + 1 rows is the first size at which one wavefront takes a second tile.

Inputs, the float64 reference and every bar are those of tests/test_gpu_mlp2_kernels.py (its helpers are imported; no number of
this module's own); the packed image is compared for equality with kgw_gemm3_pack's."""
import pytest
import torch

from tests import test_gpu_mlp2_kernels as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not M.SPLIT, reason='the bf16-pipe kernels are switched off (KGW_MLP2_SPLIT=0)')]

G = 256                                            # the grid cap of kgw_mlp2_bwd_first (kgw_mlp2_bwd_first_workspace_floats / 4096)
EDGE_ROWS = [1, 31, 32, 33, 4 * 32 * G - 1, 4 * 32 * G, 4 * 32 * G + 1]


def _blocks(rows):
    return int(M._L().kgw_mlp2_bwd_first_workspace_floats(rows)) // 4096


def _packed(dH2, W2, H1, X, K1, rows, ids, dz):
    """The packed call at the library's own sign period, its image beside kgw_gemm3_pack's of the same rows."""
    from kgwas_amd import ops
    F = int(M._L().kgw_gemm3_flip())
    rows32 = (rows + 31) // 32 * 32
    img = M._image(rows32)
    res = M._bwd(dH2, W2, H1, X, K1, rows, in_ids=ids, dz=dz, call='packed', image=M._p(img), flip=F)
    return res, img, (lambda dZ: ops.gemm3_pack(dZ.contiguous(), rows32, True, k_valid=rows))


@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('rows', EDGE_ROWS)
def test_row_count_edges(rows, packed):
    assert _blocks(4 * 32 * G + 1) == G and _blocks(rows) == min(G, (rows + 127) // 128)
    K1 = 20
    dH2, W2, H1, X = M._bwd_case(rows, K1)
    plain = M._bwd(dH2, W2, H1, X, K1, rows, dz=True)
    M._check_bwd(f'edges rows={rows}', plain, dH2, W2, H1, X, K1)
    assert not plain['db1'][77].any() and not plain['dW1'][77].any()             # the zero column of H1
    assert bool(((plain['dZ'] == 0) | (H1 > 0)).all())
    if packed:
        res, img, pack = _packed(dH2, W2, H1, X, K1, rows, None, True)
        assert torch.equal(res['dZ'], plain['dZ']) and torch.equal(res['dW1'], plain['dW1']) and torch.equal(res['db1'], plain['db1'])
        assert torch.equal(img, pack(res['dZ']))
        res2, img2, _ = _packed(dH2, W2, H1, X, K1, rows, None, False)           # dZ null: the same image, the same sums
        assert torch.equal(img2, img) and torch.equal(res2['dW1'], plain['dW1']) and torch.equal(res2['db1'], plain['db1'])
    else:
        nodz = M._bwd(dH2, W2, H1, X, K1, rows)
        assert torch.equal(nodz['dW1'], plain['dW1']) and torch.equal(nodz['db1'], plain['db1'])


@pytest.mark.parametrize('cap,rd', [(129, 0), (129, 1), (129, 33), (129, 128), (4 * 32 * G + 1, 0), (4 * 32 * G + 1, 31),
                                    (4 * 32 * G + 1, 4 * 32 * G), (4 * 32 * G + 1, 4 * 32 * G + 1)])
def test_rows_dev_below_capacity(cap, rd):
    """The static layout: `cap` rows of capacity, *rows_dev real ones, NaN in every padding row of every input (the packed call
    takes no rows_dev)."""
    K1 = 20
    dH2, W2, H1, X = M._bwd_case(cap, K1)
    res = M._bwd(dH2, W2, H1, X, K1, cap, rows_dev=rd, dz=True, dz_fill=M.MARK)
    M._check_bwd(f'edges cap={cap} rows_dev={rd}', res, dH2, W2, H1, X, K1, n=rd)
    assert bool((res['dZ'][rd:] == M.MARK).all())
    if rd == 0:
        assert not res['dW1'].any() and not res['db1'].any()


@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('K1', [20, 0])
@pytest.mark.parametrize('rows', [33, 4 * 32 * G + 1])
def test_injection_with_missing_rows(rows, K1, packed):
    """in_ids: a permutation of a shorter dH2 with -1 entries (a whole tile of them, the first row and the last); K1 = 0 with dZ
    set: no X at all, only db1 and the masked rows."""
    g = M._gen(rows + K1 + 11)
    ids, n_up = M._injection(rows, g)
    kept = ids[ids >= 0]
    assert bool((ids < 0).any()) and bool((kept[1:] < kept[:-1]).any())          # rows missing, and the kept ones out of order
    dH2, W2, H1, X = M._bwd_case(rows, K1, n_up)
    if packed:
        res, img, pack = _packed(dH2, W2, H1, X, K1, rows, ids, True)
        assert torch.equal(img, pack(res['dZ']))
    else:
        res = M._bwd(dH2, W2, H1, X, K1, rows, in_ids=ids, dz=True)
    M._check_bwd(f'edges rows={rows} K1={K1} in_ids packed={packed}', res, dH2, W2, H1, X, K1, in_ids=ids)
    assert bool((res['dZ'][ids < 0] == 0).all()) and bool((res['dZ'][:, 77] == 0).all())
    assert bool(((res['dZ'] == 0) | (H1 > 0)).all())                             # the mask is `> 0` and nothing else
