"""-m gpu: identities of the single-column read-out node that hold to the BIT because its entry points share one per-seed kernel
(k_readout_1<MODE>), one fold (k_readout_fold) and one statement of each summation order (kgw_readout_order.h): the fused training
call against forward + backward with a loss gradient of 1, the two-call form (_train_parts, kgw_readout_train_fold) against the fused
one, and the node's loss against kgw_wmse_fwd of its predictions.  Shapes: 1, 2, 7, 8, 28, 29, 65, 129 blocks of four seeds (the fold's
seven row groups and rounds of 28; 257 and 513 seeds cross the 256 accumulators of the float64 sum), rows = n, n + 3, n + 9."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (1, 5, 28, 29, 112, 113, 257, 513)
EXTRA = (0, 3, 9)
N_SNP = 700


def _call(name, *args):
    from kgwas_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*[C.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args], _lib.stream_ptr()), name)


def _nans(*shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device='cuda')


@pytest.fixture(scope='module')
def runs():
    """{(n, rows, relu word): {form: (pred, loss, dH, dw_lin, db_lin)}, 'wmse': loss} -- every form once, on the same inputs."""
    from kgwas_amd import _lib
    rng = np.random.default_rng(7)
    one = torch.ones((), dtype=torch.float64, device='cuda')
    out = {}
    for n in NS:
        for rows in (n + e for e in EXTRA):
            H = torch.from_numpy(rng.standard_normal((rows, 128)).astype(np.float32)).cuda()
            wl = torch.from_numpy((rng.standard_normal(128) / 8).astype(np.float32)).cuda()
            bl = torch.from_numpy(rng.standard_normal(1).astype(np.float32)).cuda()
            n_id = torch.from_numpy(rng.permutation(N_SNP)[:rows].astype(np.int32)).cuda()
            y = torch.from_numpy(rng.standard_normal(N_SNP).astype(np.float32)).cuda()
            w = torch.from_numpy(rng.uniform(0.1, 2.0, N_SNP)).cuda()
            terms, part = torch.empty(n, dtype=torch.float64, device='cuda'), torch.empty(((rows + 3) // 4) * 129, device='cuda')
            for word in range(4):                                  # bit 0: ReLU on the prediction; bit 1: H is a ReLU's output
                r = out[(n, rows, word)] = {}
                pred, loss, dH, dw, db = _nans(n), _nans(dtype=torch.float64), _nans(rows, 128), _nans(128), _nans(1)
                _call('kgw_readout_wmse_train', H, wl, bl, n_id, y, w, n, rows, word, pred, loss, dH, dw, db, terms, part)
                r['train'] = (pred, loss, dH, dw, db)
                pred, loss, dH, dw, db = _nans(n), _nans(dtype=torch.float64), _nans(rows, 128), _nans(128), _nans(1)
                f = _lib.KgwReadoutFold()
                _call('kgw_readout_wmse_train_parts', H, wl, bl, n_id, y, w, n, rows, word, pred, loss, dH, dw, db, terms, part, C.byref(f))
                _call('kgw_readout_train_fold', C.byref(f))
                r['parts'] = (pred, loss, dH, dw, db)
                pred, loss, dH, dw, db = _nans(n), _nans(dtype=torch.float64), _nans(rows, 128), _nans(128), _nans(1)
                _call('kgw_readout_wmse_fwd', H, wl, bl, n_id, y, w, n, word & 1, pred, loss, terms)
                _call('kgw_readout_wmse_bwd', H, wl, pred, n_id, y, w, n, rows, word, one, dH, dw, db, part)
                r['fwd_bwd'] = (pred, loss, dH, dw, db)
                r['wmse'] = _nans(dtype=torch.float64)
                _call('kgw_wmse_fwd', pred, n_id, y, w, n, r['wmse'])
    torch.cuda.synchronize()
    return out


def _same_bits(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.shape == b.shape and not np.isnan(a).any() and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _assert_forms_equal(runs, fa, fb):
    for key, r in runs.items():
        for name, a, b in zip(('pred', 'loss', 'dH', 'dw_lin', 'db_lin'), r[fa], r[fb]):
            assert _same_bits(a, b), f'{name} of {fa} and {fb} differ at (n, rows, relu word) = {key}'


def test_train_is_forward_then_backward_with_unit_gradient(runs):
    _assert_forms_equal(runs, 'train', 'fwd_bwd')


def test_train_parts_then_fold_is_train(runs):
    _assert_forms_equal(runs, 'parts', 'train')


def test_readout_loss_is_wmse_of_its_predictions(runs):
    """Both sums run through kgw_sum256_f64: the same accumulators, the same tree.  Equal on these fixed inputs, not by construction for
    n > 256: kgw_wmse_fwd adds w * d^2 to its accumulator with one fused multiply-add where the node rounds the term to float64 first,
    so an accumulator's second and later terms may round differently (measured on random inputs: 0 of 300 seeds differ at n = 256,
    9 at n = 300, 23 at n = 513)."""
    for key, r in runs.items():
        assert _same_bits(r['fwd_bwd'][1], r['wmse']), f'loss {r["fwd_bwd"][1].item()!r} vs kgw_wmse_fwd {r["wmse"].item()!r} at {key}'
