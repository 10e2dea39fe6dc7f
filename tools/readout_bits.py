"""Every read-out / loss entry point of the library on fixed-seed inputs, all outputs to one .npz -- for a bit-for-bit comparison of two
builds (KGW_LIB_PATH selects the library; one fresh process per library):

    KGW_LIB_PATH=$PWD/kgwas_amd/csrc/libkgwas_hip_prev.so python tools/readout_bits.py /tmp/prev.npz
    python tools/readout_bits.py /tmp/cur.npz
    python tools/readout_bits.py --compare /tmp/prev.npz /tmp/cur.npz          (exit status 1 unless every array has equal bits)

Shapes: the smallest that reach every edge of the kernels -- n seeds in 1, 2, 7, 8, 28, 29 (and 65, 129) blocks of four (the fold's
seven row groups and its rounds of 28), 257 and 513 across the 256 accumulators of the float64 sum; rows = n, n + 3, n + 9 (rows
without a seed inside the last seeded block, blocks without seeds); relu x h_is_relu; a loss gradient other than 1 for the _bwd calls."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NS = (1, 5, 28, 29, 112, 113, 257, 513)
EXTRA = (0, 3, 9)
TS = (1, 4, 32)
N_SNP, GLOSS = 700, 0.37


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    keys = sorted(set(a.files) | set(b.files))
    bad = [k for k in keys if k not in a.files or k not in b.files or a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or
           not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))]
    by_entry = {}
    for k in keys:
        e = k.split('/')[1]
        by_entry.setdefault(e, [0, 0])[0] += 1
        by_entry[e][1] += k in bad
    for e, (tot, nbad) in sorted(by_entry.items()):
        print('%-34s %5d arrays  %5d with other bits' % (e, tot, nbad))
    for k in bad[:40]:
        print('DIFFERENT', k)
    print('%d arrays compared on their raw bits, %d different: %s' % (len(keys), len(bad), 'EQUAL' if not bad else 'NOT EQUAL'))
    return 1 if bad or not keys else 0


def run(out_path):
    import torch
    from kgwas_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(20261018)
    out = {}

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def nans(*shape, dtype=torch.float32):
        return torch.full(shape, float('nan'), dtype=dtype, device='cuda')

    def call(name, *args):
        _lib.check(getattr(L, name)(*[C.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args], _lib.stream_ptr()), name)

    def keep(case, entry, **arrays):
        for k, v in arrays.items():
            out['%s/%s/%s' % (case, entry, k)] = v.cpu().numpy()

    gl = dev(np.array(GLOSS, dtype=np.float64))
    for n in NS:
        for rows in (n + e for e in EXTRA):
            H = dev(rng.standard_normal((rows, 128)).astype(np.float32))
            n_id = dev(rng.permutation(N_SNP)[:rows].astype(np.int32))
            w1 = dev(rng.uniform(0.1, 2.0, N_SNP))
            nb4 = (rows + 3) // 4
            for T in TS:
                W = dev((rng.standard_normal((T, 128)) / 8).astype(np.float32))
                b = dev(rng.standard_normal(T).astype(np.float32) / 4)
                y = dev(rng.standard_normal((N_SNP, T)).astype(np.float32))
                wT = dev(rng.uniform(0.1, 2.0, (N_SNP, T)) * (rng.random((N_SNP, T)) > 0.3))
                for relu in (0, 1):
                    for hr in (0, 1):
                        case, word = 'n%d_rows%d_T%d_relu%d_hrelu%d' % (n, rows, T, relu, hr), relu | 2 * hr
                        terms, part = nans(n, dtype=torch.float64), nans(nb4 * T * 129)
                        for fam, w in (('mt', w1), ('mtw', wT)):
                            pred, loss = nans(n, T), nans(dtype=torch.float64)
                            call('kgw_readout_wmse_%s_fwd' % fam, H, W, b, n_id, y, w, n, T, relu, pred, loss, terms)
                            keep(case, fam + '_fwd', pred=pred, loss=loss)
                            dH, dW, db = nans(rows, 128), nans(T, 128), nans(T)
                            call('kgw_readout_wmse_%s_bwd' % fam, H, W, pred, n_id, y, w, n, rows, T, word, gl, dH, dW, db, part)
                            keep(case, fam + '_bwd', dH=dH, dW=dW, db=db)
                            pred, loss, dH, dW, db = nans(n, T), nans(dtype=torch.float64), nans(rows, 128), nans(T, 128), nans(T)
                            call('kgw_readout_wmse_%s_train' % fam, H, W, b, n_id, y, w, n, rows, T, word, pred, loss, dH, dW, db, terms,
                                 part)
                            keep(case, fam + '_train', pred=pred, loss=loss, dH=dH, dW=dW, db=db)
                        pred = nans(n, T)
                        call('kgw_readout_mt_pred', H, W, b, n, T, relu, pred)
                        dH, dW, db = nans(rows, 128), nans(T, 128), nans(T)
                        call('kgw_readout_mt_pred_bwd', H, W, pred, n, rows, T, word, dH, dW, db, part)
                        keep(case, 'mt_pred', pred=pred, dH=dH, dW=dW, db=db)
                        if T != 1:
                            continue
                        # the single-column node: w_lin = W [1][128], b_lin = b [1], y [N_SNP][1] = [N_SNP]
                        pred, loss = nans(n), nans(dtype=torch.float64)
                        call('kgw_readout_wmse_fwd', H, W, b, n_id, y, w1, n, relu, pred, loss, terms)
                        keep(case, 'readout_wmse_fwd', pred=pred, loss=loss)
                        dH, dw, db = nans(rows, 128), nans(128), nans(1)
                        call('kgw_readout_wmse_bwd', H, W, pred, n_id, y, w1, n, rows, word, gl, dH, dw, db, part)
                        keep(case, 'readout_wmse_bwd', dH=dH, dw=dw, db=db)
                        loss2, dpred = nans(dtype=torch.float64), nans(n)
                        call('kgw_wmse_fwd', pred, n_id, y, w1, n, loss2)
                        call('kgw_wmse_bwd', pred, n_id, y, w1, n, gl, dpred)
                        keep(case, 'wmse', loss=loss2, dpred=dpred)
                        pred, loss, dH, dw, db = nans(n), nans(dtype=torch.float64), nans(rows, 128), nans(128), nans(1)
                        call('kgw_readout_wmse_train', H, W, b, n_id, y, w1, n, rows, word, pred, loss, dH, dw, db, terms, part)
                        keep(case, 'readout_wmse_train', pred=pred, loss=loss, dH=dH, dw=dw, db=db)
                        pred, loss, dH, dw, db = nans(n), nans(dtype=torch.float64), nans(rows, 128), nans(128), nans(1)
                        f = _lib.KgwReadoutFold()
                        call('kgw_readout_wmse_train_parts', H, W, b, n_id, y, w1, n, rows, word, pred, loss, dH, dw, db, terms, part,
                             C.byref(f))
                        call('kgw_readout_train_fold', C.byref(f))
                        keep(case, 'readout_wmse_train_parts_fold', pred=pred, loss=loss, dH=dH, dw=dw, db=db)
    # the same node through ops.readout_weighted_mse (autograd): forward + backward of a scaled loss, and the unit-gradient form
    from kgwas_amd import ops
    for T, cols in ((1, False), (4, False), (4, True)):
        W = dev((rng.standard_normal((T, 128)) / 8).astype(np.float32)).requires_grad_()
        b = dev(rng.standard_normal(T).astype(np.float32) / 4).requires_grad_()
        y = dev(rng.standard_normal((N_SNP, T)).astype(np.float32))
        w = dev(rng.uniform(0.1, 2.0, (N_SNP, T)) * (rng.random((N_SNP, T)) > 0.3)) if cols else w1
        for unit in (False, True):
            Hg = H.clone().requires_grad_()
            W.grad = b.grad = None
            loss, pred = ops.readout_weighted_mse(Hg, W, b, n_id, y, w, n, relu=True, h_is_relu=True, unit_grad=unit)
            if unit:
                loss.backward(gradient=ops.unit_gradient(loss.device))
            else:
                (GLOSS * loss).backward()
            keep('ops_T%d_w%dd_unit%d' % (T, w.dim(), unit), 'ops_readout_weighted_mse', pred=pred.detach(), loss=loss.detach(), dH=Hg.grad,
                 dW=W.grad, db=b.grad)
    torch.cuda.synchronize()
    np.savez(out_path, **out)
    print('%s: %d arrays from %s' % (out_path, len(out), _lib.LIB_PATH))
    return 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(run(sys.argv[1]))
