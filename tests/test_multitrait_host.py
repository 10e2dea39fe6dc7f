"""CPU: the host side of multi-trait training (T label columns on one shared trunk) and the float64 twin of its loss node."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests.multitrait_ref import make_case, readout_wmse_np


@pytest.fixture(scope='module')
def tiny3(tmp_path_factory):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path_factory.mktemp('mt')),
                                     n_traits=3)


def test_synthetic_traits_keep_column_zero(tiny3, tmp_path):
    from kgwas_amd.kgwas_data import KGWAS_Data
    one = KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path))
    y1, y3 = one.data['SNP'].y.numpy(), tiny3.data['SNP'].y.numpy()
    assert y1.ndim == 1 and y3.shape == (y1.shape[0], 3) and y3.dtype == np.float32
    assert np.array_equal(y3[:, 0], y1)
    assert np.array_equal(one.train_input_nodes[1], tiny3.train_input_nodes[1])
    lab = np.asarray(tiny3.all_ids)
    unl = np.setdiff1d(np.arange(y1.shape[0]), lab)
    assert (y3[unl] == -1).all() and (y3[lab] >= 0).all()
    # the columns are different draws, and each trait's table carries its own chi / P over the same SNPs
    assert not np.array_equal(y3[lab, 1], y3[lab, 0]) and not np.array_equal(y3[lab, 2], y3[lab, 1])
    for t in range(3):
        tab = tiny3.trait_table(t)
        assert np.array_equal(tab.ID.values, tiny3.lr_uni.ID.values)
        assert np.array_equal(tab.y.values.astype(np.float32), y3[lab, t])
    with pytest.raises(ValueError):
        KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path), n_traits=0, split=False)


def test_single_trait_config_has_no_new_key_and_three_traits_round_trip(tiny3, tmp_path):
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.utils import save_model
    run = KGWAS(tiny3, device='cpu', seed=1)
    run.initialize_model()
    assert sorted(run.config) == ['gat_num_head', 'gnn_aggr', 'gnn_backbone', 'gnn_hidden_dim', 'gnn_num_layers']
    assert run.model.lin.out_features == 1
    run.initialize_model(out_channels=3)
    assert run.config['out_channels'] == 3 and tuple(run.model.lin.weight.shape) == (3, 128)
    with torch.no_grad():
        run.model.lin.weight.normal_()
    path = os.path.join(str(tmp_path), 'ckpt')
    save_model(run.model, run.config, path)
    with open(os.path.join(path, 'config.pkl'), 'rb') as f:
        assert pickle.load(f)['out_channels'] == 3
    run2 = KGWAS(tiny3, device='cpu', seed=2)
    run2.load_pretrained(path)
    assert run2.config == run.config and run2.model.lin.out_features == 3
    sd, sd2 = run.model.state_dict(), run2.model.state_dict()
    assert list(sd) == list(sd2)
    lazy = torch.nn.parameter.UninitializedParameter
    for k in sd:
        assert isinstance(sd[k], lazy) == isinstance(sd2[k], lazy), k
        if not isinstance(sd[k], lazy):
            assert torch.equal(sd[k].cpu(), sd2[k].cpu()), k
    assert torch.equal(sd['lin.weight'], sd2['lin.weight']) and tuple(sd2['lin.weight'].shape) == (3, 128)
    for bad in (0, 33):
        with pytest.raises(NotImplementedError):
            run.initialize_model(out_channels=bad)


@pytest.mark.parametrize('relu', [0, 1, 2, 3])
@pytest.mark.parametrize('T,n,rows', [(1, 5, 5), (3, 7, 9), (8, 64, 71), (32, 33, 33)])
def test_numpy_twin_matches_autograd(T, n, rows, relu):
    """The twin's loss and its three gradients against torch.autograd in float64 (gloss = 0.7)."""
    H, W, b, n_id, y, w = make_case(n, T, rows, seed=100 * T + n)
    pred, loss, dH, dW, db = readout_wmse_np(H, W, b, n_id, y, w, n, relu, gloss=0.7, rows=rows)
    Hin = torch.tensor(H, dtype=torch.float64, requires_grad=True)
    Wt = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    # bit 1: H is the output of a ReLU whose backward is folded into the node -- autograd sees that ReLU as part of the graph
    Ht = torch.relu(Hin) if relu & 2 else Hin
    ids = torch.tensor(n_id.astype(np.int64))
    z = Ht[:n] @ Wt.T + bt
    p = torch.relu(z) if relu & 1 else z
    lt = (torch.tensor(w)[ids][:, None] * (p - torch.tensor(y, dtype=torch.float64)[ids]) ** 2).mean()
    (0.7 * lt).backward()
    assert np.allclose(pred, p.detach().numpy(), rtol=1e-12, atol=1e-14)
    assert abs(loss - float(lt.detach())) <= 1e-12 * abs(float(lt.detach()))
    for mine, ref, what in ((dH, Hin.grad, 'dH'), (dW, Wt.grad, 'dW'), (db, bt.grad, 'db')):
        assert np.allclose(mine, ref.numpy(), rtol=1e-10, atol=1e-14), what
    assert not dH[n:].any()
    if T == 1:          # the single-column definition (kgw_readout_wmse_*): mean over the seeds
        d = pred[:, 0] - y[n_id[:n].astype(np.int64), 0]
        assert abs(loss - float(np.mean(w[n_id[:n].astype(np.int64)] * d * d))) <= 1e-12 * max(loss, 1e-300)


def test_binding_declares_the_multitrait_entry_points():
    from kgwas_amd import _lib
    lib = _lib.lib()
    for name in ('kgw_readout_mt_pred', 'kgw_readout_mt_pred_bwd', 'kgw_readout_wmse_mt_fwd', 'kgw_readout_wmse_mt_bwd',
                 'kgw_readout_wmse_mt_train'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    # argument errors come back as status codes before anything is launched (no GPU needed): null pointers, T out of range
    assert lib.kgw_readout_wmse_mt_train(*([None] * 6), 4, 4, 3, 1, *([None] * 8)) == -1
    assert lib.kgw_readout_mt_pred(None, None, None, 4, 3, 0, None, None) == -1
