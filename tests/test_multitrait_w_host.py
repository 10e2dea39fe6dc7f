"""CPU: per-trait LD weights and per-trait SNP lists of multi-trait training -- the float64 twin of the loss node with a weight matrix
(tests/multitrait_w_ref.py), the C ABI of its three entry points, the data layer and the host side of KGWAS.train."""
import math
import os

import numpy as np
import pytest
import torch

from tests.multitrait_ref import make_case, readout_wmse_np
from tests.multitrait_w_ref import make_case_w, readout_wmse_w_np

SIZES, COVER = [5000, 20000, 387113], [1.0, 0.6, 0.3]


@pytest.mark.parametrize('relu', [0, 1, 2, 3])
@pytest.mark.parametrize('T,n,rows', [(1, 5, 5), (3, 7, 9), (8, 64, 71), (32, 33, 33)])
def test_equal_columns_give_the_shared_weight_twin(T, n, rows, relu):
    """w[:, t] = w0 for every t: the twin with a weight matrix equals tests/multitrait_ref.readout_wmse_np to 1e-12 relative."""
    H, W, b, n_id, y, w0 = make_case(n, T, rows, seed=100 * T + n)
    ref = readout_wmse_np(H, W, b, n_id, y, w0, n, relu, gloss=0.7, rows=rows)
    got = readout_wmse_w_np(H, W, b, n_id, y, np.repeat(w0[:, None], T, 1), n, relu, gloss=0.7, rows=rows)
    assert abs(got[1] - ref[1]) <= 1e-12 * abs(ref[1])
    for a, r, what in zip(got, ref, ('pred', 'loss', 'dH', 'dW', 'db')):
        a, r = np.asarray(a), np.asarray(r)
        assert np.all(np.abs(a - r) <= 1e-12 * np.abs(r)), what


def test_twin_never_reads_an_unobserved_label():
    """NaN / +-Inf under every zero weight: every output is finite and equals the outputs with those labels replaced by 7."""
    case = make_case_w(9, 5, 11, seed=4)
    H, W, b, n_id, y, w = case
    assert (w == 0).any() and not np.isfinite(y[w == 0]).any() and np.isfinite(y[w != 0]).all()
    y7 = np.where(w == 0, np.float32(7), y)
    for relu in (0, 3):
        a = readout_wmse_w_np(H, W, b, n_id, y, w, 9, relu, 0.7, 11)
        c = readout_wmse_w_np(H, W, b, n_id, y7, w, 9, relu, 0.7, 11)
        for u, v in zip(a, c):
            assert np.isfinite(u).all() and np.array_equal(u, v)


@pytest.mark.parametrize('relu', [0, 1, 2, 3])
@pytest.mark.parametrize('T,n,rows,seed', [(1, 5, 5, 0), (3, 7, 9, 0), (4, 9, 10, 0)])
def test_twin_gradients_match_central_differences(T, n, rows, seed, relu):
    """The twin's dH, dW, db against central differences of its own loss, element by element, at the tolerance
    tests/test_multitrait_host.py holds the shared-weight twin to against autograd (rtol 1e-10, atol 1e-14).  The loss is piecewise
    quadratic, so a central difference has no truncation error as long as no pre-activation changes sign inside the step (asserted:
    step 2^-10, every |z| beyond the largest change the step can cause); what is left is rounding, eps |loss| / step, which in
    float64 (1e-13) would eat the tolerance -- so the differences are taken with the twin run in numpy's long double (x87 extended
    precision, eps 1.1e-19: 1e-16), the gradients themselves in float64."""
    assert np.finfo(np.longdouble).eps < 1e-18, 'this check needs an extended-precision long double'
    H, W, b, n_id, y, w = make_case_w(n, T, rows, seed=31 * T + n + seed, poison=True)
    gloss = 0.7
    _, _, dH, dW, db = readout_wmse_w_np(H, W, b, n_id, y, w, n, relu, gloss, rows)
    ld = np.longdouble
    step = ld(2.0) ** -10
    z = H[:n].astype(np.float64) @ W.astype(np.float64).T + b
    reach = float(step) * max(1.0, float(np.abs(H).max()), float(np.abs(W).max()))
    if relu & 1:
        assert np.abs(z).min() > 2 * reach, 'a pre-activation sits within the step of its kink: choose another seed'
    base = [H.astype(ld), W.astype(ld), b.astype(ld)]

    def loss_at(k, idx, delta):
        args = [v.copy() for v in base]
        args[k][idx] += delta
        return readout_wmse_w_np(args[0], args[1], args[2], n_id, y, w, n, relu & 1, 1.0, rows, dtype=ld)[1]

    for k, (mine, what) in enumerate(((dH, 'dH'), (dW, 'dW'), (db, 'db'))):
        fd = np.zeros(mine.shape)
        it = np.ndindex(*((n, 128) if k == 0 else mine.shape))          # (rows beyond the seeds never enter the loss)
        for idx in it:
            fd[idx] = float(gloss * (loss_at(k, idx, step) - loss_at(k, idx, -step)) / (2 * step))
        if k == 0 and relu & 2:          # bit 1: H is a ReLU's output and the node folds that ReLU's backward in
            fd *= H > 0
        assert np.allclose(mine, fd, rtol=1e-10, atol=1e-14), (what, float(np.abs(mine - fd).max()))
    assert not dH[n:].any()


def test_binding_declares_the_weight_matrix_entry_points():
    from kgwas_amd import _lib
    lib = _lib.lib()
    for name in ('kgw_readout_wmse_mtw_fwd', 'kgw_readout_wmse_mtw_bwd', 'kgw_readout_wmse_mtw_train'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    # argument errors come back as status codes before anything is launched (no GPU needed)
    assert lib.kgw_readout_wmse_mtw_train(*([None] * 6), 4, 4, 3, 1, *([None] * 8)) == -1
    assert lib.kgw_readout_wmse_mtw_fwd(*([None] * 6), 4, 3, 1, *([None] * 4)) == -1
    assert lib.kgw_readout_wmse_mtw_bwd(*([None] * 6), 4, 4, 3, 1, *([None] * 6)) == -1


def _synth(path, **kw):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(path), n_traits=3, **kw)


@pytest.fixture(scope='module')
def tiny3w(tmp_path_factory):
    return _synth(tmp_path_factory.mktemp('mtw'), trait_sample_sizes=SIZES, trait_coverage=COVER)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if hasattr(a, 'equals'):
        return bool(a.equals(b))
    return a == b


def test_synthetic_per_trait_weights(tiny3w, tmp_path):
    from kgwas_amd.utils import ldsc_regression_weights
    d = tiny3w
    n = len(d.all_ids)
    w, obs = d.ldsc_weight_traits, d.trait_observed
    assert w.shape == (n, 3) and w.dtype == np.float64 and obs.shape == (n, 3) and obs.dtype == bool
    y = d.data['SNP'].y
    assert tuple(y.shape) == (d.data['SNP'].x.shape[0], 3)
    ld, w_ld = d._synth_ld
    for t in range(3):
        o = obs[:, t]
        assert int(o.sum()) == math.ceil(COVER[t] * n)
        assert abs(w[o, t].mean() - 1.0) <= 1e-12 and (w[o, t] > 0).all()
        assert not w[~o, t].any()
        ref = ldsc_regression_weights(np.asarray(ld), np.asarray(w_ld), SIZES[t], 15000000, 0.5)
        assert np.allclose(w[o, t], ref[o] / ref[o].mean(), rtol=1e-13, atol=0)
        assert not y[torch.from_numpy(d.all_ids[~o]), t].ne(0).any()
        tab = d.trait_table(t)
        assert np.array_equal(tab.ID.values, d.lr_uni.ID.values[o]) and (tab.N.values == SIZES[t]).all()
        assert np.array_equal(tab.y.values.astype(np.float32), y[torch.from_numpy(d.all_ids[o]), t].numpy())
        assert np.array_equal(d.trait_rows(t), np.nonzero(o)[0])
    assert obs[:, 0].all() and not np.array_equal(obs[:, 1], obs[:, 2])
    both = obs[:, 1] & obs[:, 2]
    # the shape of a column follows its N: after each column's own normalisation they still differ where both are observed
    assert both.sum() > 10 and not np.allclose(w[both, 0], w[both, 1], rtol=1e-3) and not np.allclose(w[both, 1], w[both, 2], rtol=1e-3)
    again = _synth(tmp_path, trait_sample_sizes=SIZES, trait_coverage=COVER)
    assert np.array_equal(again.ldsc_weight_traits, w) and np.array_equal(again.trait_observed, obs)
    assert torch.equal(again.data['SNP'].y, y)
    for bad in ({'trait_sample_sizes': [1, 2]}, {'trait_coverage': [1.0, 0.5, 0.0]}, {'trait_coverage': [1.0, 0.5, 1.5]}):
        with pytest.raises(ValueError):
            _synth(tmp_path, split=False, **bad)


def test_default_arguments_change_nothing(tiny3w, tmp_path):
    """Both new arguments None: the object of from_synthetic(n_traits=3) as it was -- no new attribute -- and the 1-D weights, the
    labelled list and the split do not depend on them either."""
    plain = _synth(tmp_path / 'a')
    explicit = _synth(tmp_path / 'b', trait_sample_sizes=None, trait_coverage=None)
    for name in ('ldsc_weight_traits', 'trait_observed', 'trait_sample_sizes', '_trait_frames'):
        assert not hasattr(plain, name) and not hasattr(explicit, name)
    va, vb = vars(plain), vars(explicit)
    assert sorted(va) == sorted(vb)
    for k in va:
        if k not in ('data', 'data_path', 'idx2id', 'id2idx'):
            assert _same(va[k], vb[k]), k
    assert torch.equal(plain.data['SNP'].y, explicit.data['SNP'].y)
    assert plain.ldsc_weight.ndim == 1 and np.array_equal(plain.ldsc_weight, tiny3w.ldsc_weight)
    assert np.array_equal(plain.all_ids, tiny3w.all_ids)
    for s in ('train_input_nodes', 'val_input_nodes', 'test_input_nodes'):
        assert np.array_equal(getattr(plain, s)[1], getattr(tiny3w, s)[1])
    lab = torch.from_numpy(tiny3w.all_ids)
    obs = torch.from_numpy(tiny3w.trait_observed)
    assert torch.equal(plain.data['SNP'].y[lab][obs], tiny3w.data['SNP'].y[lab][obs])
    assert torch.equal(plain.data['SNP'].y[:, 0], tiny3w.data['SNP'].y[:, 0])


def test_external_files_per_trait(tmp_path):
    """Three overlapping summary-statistics files and the two LD-score files, all written here."""
    import pandas as pd
    from scipy.stats import chi2
    from kgwas_amd.kgwas_data import KGWAS_Data
    from kgwas_amd.utils import ldsc_regression_weights
    d = KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path), split=False)
    n_snp = len(d.idx2id['SNP'])
    rng = np.random.default_rng(0)
    picks = [np.arange(0, 120), np.arange(60, 200)[::-1], np.concatenate([np.arange(100, 130), np.arange(300, 340)])]
    sizes = [4000.0, 52000.0, 387113.0]
    files, tables = [], []
    for t, ids in enumerate(picks):
        df = pd.DataFrame({'CHR': 1, 'SNP': [f'rs{i}' for i in ids] + [f'rs{n_snp + 5 + t}'],       # (the last: not in the KG)
                           'P': rng.uniform(1e-6, 1.0, len(ids) + 1), 'N': sizes[t]})
        if t == 1:                                  # BETA / SE win over P in the 'chi' branch order; a NaN label becomes 0
            df['BETA'], df['SE'] = rng.standard_normal(len(df)), rng.uniform(0.5, 1.5, len(df))
            df.loc[3, 'BETA'] = np.nan
        path = os.path.join(str(tmp_path), f'trait{t}.tsv')
        df.to_csv(path, sep='\t', index=False)
        files.append(path)
        tables.append(df.iloc[:-1])
    os.makedirs(os.path.join(str(tmp_path), 'ld_score'))
    ld_ids = [f'rs{i}' for i in range(0, 330)]                      # (rs330.. take the minimum)
    ld, wld = rng.uniform(1, 200, len(ld_ids)), rng.uniform(0, 10, len(ld_ids))
    pd.DataFrame({'SNP': ld_ids, 'L2': ld}).to_csv(os.path.join(str(tmp_path), 'ld_score/filter_genotyped_ldscores.csv'), index=False)
    pd.DataFrame({'SNP': ld_ids, 'L2': wld}).to_csv(os.path.join(str(tmp_path), 'ld_score/ldscores_from_data.csv'), index=False)
    d.load_external_gwas_traits(files, seed=42)
    union = list(dict.fromkeys(i for ids in picks for i in ids))
    assert np.array_equal(d.all_ids, np.asarray(union)) and list(d.lr_uni.ID.values) == [f'rs{i}' for i in union]
    assert d.trait_sample_sizes == sizes and d.ldsc_weight_traits.shape == (len(union), 3)
    pos = {i: r for r, i in enumerate(union)}
    ld_of = lambda i: ld[i] if i < 330 else ld.min()
    wld_of = lambda i: 1 + (wld[i] if i < 330 else wld.min())
    for t, ids in enumerate(picks):
        rows = np.asarray([pos[i] for i in ids])
        assert np.array_equal(d.trait_rows(t), rows)
        o = np.zeros(len(union), bool)
        o[rows] = True
        assert np.array_equal(d.trait_observed[:, t], o)
        ref = ldsc_regression_weights(np.asarray([ld_of(i) for i in ids]), np.asarray([wld_of(i) for i in ids]), sizes[t], 15000000, 0.5)
        assert np.allclose(d.ldsc_weight_traits[rows, t], ref / ref.mean(), rtol=1e-12, atol=0)
        assert not d.ldsc_weight_traits[~o, t].any()
        src = tables[t]
        if t == 1:
            lab = np.nan_to_num((src.BETA / src.SE).values ** 2, nan=0.0)
            assert lab[3] == 0.0
        else:
            lab = chi2.ppf(1 - src.P.values, 1)
        tab = d.trait_table(t)
        assert list(tab.ID.values) == [f'rs{i}' for i in ids] and (tab.N.values == sizes[t]).all()
        assert np.allclose(tab.y.values, lab, rtol=1e-9, atol=0) and np.allclose(tab.P.values, src.P.values, rtol=1e-12)
    assert np.array_equal(d.ldsc_weight, d.ldsc_weight_traits[:, 0])
    d.prepare_split()
    y = d.data['SNP'].y
    assert tuple(y.shape) == (n_snp, 3)
    lab_ids = torch.from_numpy(d.all_ids)
    for t in range(3):
        col = np.zeros(len(union), np.float32)
        col[d.trait_rows(t)] = d.trait_table(t).y.values.astype(np.float32)
        assert np.array_equal(y[lab_ids, t].numpy(), col)
    unl = np.setdiff1d(np.arange(n_snp), d.all_ids)
    assert (y[torch.from_numpy(unl)] == -1).all()
    with pytest.raises(ValueError):
        bad = os.path.join(str(tmp_path), 'bad.tsv')
        tables[0].drop(columns=['N']).to_csv(bad, sep='\t', index=False)
        d.load_external_gwas_traits([files[0], bad])


def test_metrics_mask_per_trait(tiny3w):
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.utils import compute_metrics
    run = KGWAS(tiny3w, device='cpu', seed=1)
    run.initialize_model(out_channels=3)
    rng = np.random.default_rng(5)
    n = 40
    res = {'pred': rng.standard_normal((n, 3)).astype(np.float32), 'truth': rng.standard_normal((n, 3)).astype(np.float32)}
    obs = rng.random((n, 3)) < 0.6
    obs[:, 2] = False
    obs[7, 2] = True                                    # one observed label: no Pearson
    res['truth'][~obs] = np.nan                         # an unobserved label must not reach a metric
    m = run._metrics(res, obs)
    for t in (0, 1):
        ref = compute_metrics({'pred': res['pred'][obs[:, t], t], 'truth': res['truth'][obs[:, t], t]})
        assert m['per_trait'][t]['mse'] == ref['mse'] and m['per_trait'][t]['pearsonr'] == ref['pearsonr']
    assert np.isnan(m['per_trait'][2]['mse']) and np.isnan(m['per_trait'][2]['pearsonr'])
    assert m['mse'] == float(np.mean([m['per_trait'][t]['mse'] for t in (0, 1)]))
    assert m['pearsonr'] == float(np.mean([m['per_trait'][t]['pearsonr'] for t in (0, 1)]))
    obs[:] = False
    obs[0, :] = True
    with pytest.raises(ValueError):
        run._metrics(res, obs)
    # without a mask: what it was
    res['truth'] = rng.standard_normal((n, 3)).astype(np.float32)
    m = run._metrics(res)
    assert m['per_trait'][1]['mse'] == compute_metrics({'pred': res['pred'][:, 1], 'truth': res['truth'][:, 1]})['mse']
    w = run._ld_weight_vector()
    assert tuple(w.shape) == (tiny3w.data['SNP'].x.shape[0], 3) and w.dtype == torch.float64 and w.is_contiguous()
    assert torch.equal(w[torch.from_numpy(tiny3w.all_ids)], torch.from_numpy(tiny3w.ldsc_weight_traits))


def test_weight_matrix_is_validated_before_any_library_call():
    from kgwas_amd import ops
    H, n_id = torch.zeros(4, 128), torch.zeros(4, dtype=torch.int32)
    W3, b3, y3 = torch.zeros(3, 128), torch.zeros(3), torch.zeros(5, 3)
    for w in (torch.zeros(5, 2, dtype=torch.float64), torch.zeros(5, 4, dtype=torch.float64), torch.zeros(5, 3),
              torch.zeros(3, 5, dtype=torch.float64).t(), torch.zeros(6, 3, dtype=torch.float64),
              torch.zeros(5, 3, 1, dtype=torch.float64)):
        with pytest.raises(ValueError):
            ops.readout_weighted_mse(H, W3, b3, n_id, y3, w, 4)
    with pytest.raises(ValueError):                     # one column: [N, 1] is the only matrix
        ops.readout_weighted_mse(H, torch.zeros(1, 128), torch.zeros(1), n_id, torch.zeros(5), torch.zeros(5, 2, dtype=torch.float64), 4)
