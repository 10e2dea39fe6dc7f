"""CPU: the attention-dropout rule (gat_dropout=p) -- its numpy twin's statistics, the host's word, and the host-side plumbing
that needs no GPU (construction-time refusals, config, the ABI mirror)."""
import ctypes
import os
import pickle

import numpy as np
import pytest

from tests import attn_dropout_ref as R
from tests import fanout_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1_000_000
WORDS = [R.dropout_word(0, 0, 0), R.dropout_word(42, 3, 17), 0, 1, (1 << 64) - 1]


@pytest.mark.parametrize('p', [0.1, 0.25, 0.5])
def test_keep_fraction_is_one_minus_p(p):
    """10^6 consecutive local edges, five words, both layers: the kept fraction is within 5 sigma of the binomial's 1 - p."""
    sigma = np.sqrt(p * (1 - p) / N)
    e = np.arange(N)
    for w in WORDS:
        for layer in (1, 2):
            f = float(R.keep(w, layer, e, p).mean())
            print(f'p {p} word {w:#x} layer {layer}: kept {f:.6f} ({(f - (1 - p)) / sigma:+.2f} sigma)')
            assert abs(f - (1 - p)) <= 5 * sigma, (p, w, layer, f)


def test_layers_and_words_draw_independently():
    """At p = 0.5 two independent masks agree on half the edges (5 sigma of 10^6 fair coins), and a mask does not repeat with lag 1."""
    e = np.arange(N)
    sigma = 0.5 / np.sqrt(N)
    w = WORDS[1]
    a = R.keep(w, 1, e, 0.5)
    for other in (R.keep(w, 2, e, 0.5), R.keep(w + 1, 1, e, 0.5), R.keep(R.dropout_word(42, 4, 17), 1, e, 0.5),
                  R.keep(R.dropout_word(42, 3, 18), 1, e, 0.5)):
        assert abs(float((a == other).mean()) - 0.5) <= 5 * sigma
    assert abs(float((a[1:] == a[:-1]).mean()) - 0.5) <= 5 * sigma
    assert np.array_equal(a, R.keep(w, 1, e, 0.5))                       # a pure function


def test_p_zero_keeps_everything_and_scale_is_float32():
    assert R.thresh(0.0) == 0 and bool(R.keep(WORDS[0], 1, np.arange(N), 0.0).all())
    f = R.factor(WORDS[0], 2, 1000, 0.1)
    assert set(f.tolist()) == {0.0, float(np.float32(1.0 / 0.9))}


def test_package_word_and_parameters_equal_the_twin():
    from kgwas_amd.sampler import dropout_params, dropout_word, fanout_sample_word
    for s, e, b in ((0, 0, 0), (42, 1, 7), (2 ** 63 + 5, 123456, 99999)):
        assert dropout_word(s, e, b) == R.dropout_word(s, e, b)
        assert dropout_word(s, e, b) != fanout_sample_word(s, e, b) == fanout_ref.sample_word(s, e, b)
    assert len({dropout_word(1, 0, 0), dropout_word(0, 1, 0), dropout_word(0, 0, 1), dropout_word(0, 0, 0)}) == 4
    for p in (0.0, 0.1, 0.25, 0.5, 0.999):
        assert dropout_params(p) == (R.thresh(p), float(np.float32(1.0 / (1.0 - p))))
    for bad in (-0.1, 1.0, 1.5, float('nan')):
        with pytest.raises(ValueError):
            dropout_params(bad)


def test_header_names_the_rule():
    hdr = open(os.path.join(ROOT, 'include', 'kgwas_hip.h')).read()
    for name in ('kgwdrop_base', 'kgwdrop_keep', 'drop_word_dev', 'drop_thresh', 'drop_scale', 'floor(p * 2^32)'):
        assert name in hdr, name
    body = hdr[hdr.index('uint32_t kgwdrop_base('):hdr.index('int kgw_gat_aggregate_fwd')]
    assert 'kgwfan_step' in body and 'kgwfan_mix32(base ^ local_edge) >= thresh' in body
    assert '0x' not in body.split('KGWFAN_INLINE', 1)[1]                    # no constants of its own
    assert '#define KGW_VERSION      125' in hdr


def test_layer_args_mirror_matches_the_library():
    from kgwas_amd import _lib
    sizes = (ctypes.c_int64 * 7)()
    assert _lib.lib().kgw_struct_sizes(sizes, 7) == 0
    assert sizes[4] == ctypes.sizeof(_lib.KgwLayerArgs)
    f = _lib.KgwLayerArgs
    assert f.drop_word_dev.offset + 16 == ctypes.sizeof(f) and f.drop_thresh.offset == f.drop_word_dev.offset + 8
    assert f.drop_scale.offset == f.drop_word_dev.offset + 12 and _lib.lib().kgw_has_dropout


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path_factory.mktemp('drop')))


def test_construction_refusals(tiny):
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(tiny, device='cpu', seed=1)
    with pytest.raises(ValueError):
        run.initialize_model(gnn_backbone='SAGE', gat_dropout=0.1)
    for bad in (-0.1, 1.0, 2.0):
        with pytest.raises(ValueError):
            run.initialize_model(gat_dropout=bad)
    run.initialize_model(gnn_backbone='SAGE')                                # (no dropout: SAGE as before)
    run.initialize_model(gat_dropout=0.25)
    assert run.model.gat_dropout == 0.25
    with pytest.raises(NotImplementedError):
        run.train(epoch=1, parallelism='shard')


def test_model_owns_the_word_and_drops_only_in_training(tiny):
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(tiny, device='cpu', seed=1)
    run.initialize_model(gat_dropout=0.25)
    m = run.model
    assert m.drop_word.dtype.is_floating_point is False and m.drop_word.numel() == 1
    assert int(m.drop_word) & ((1 << 64) - 1) == R.dropout_word(0, 0, 0)
    m.set_dropout_word(R.dropout_word(7, 1, 2))
    assert int(m.drop_word) & ((1 << 64) - 1) == R.dropout_word(7, 1, 2)
    assert 'drop_word' not in m.state_dict()
    m.train()
    assert m._dropout()[0] == 0.25 and m._dropout()[1] is m.drop_word
    m.eval()
    assert m._dropout() is None
    run.initialize_model()
    run.model.train()
    assert run.model.gat_dropout == 0.0 and run.model._dropout() is None


def test_config_carries_the_key_only_when_set(tiny, tmp_path):
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.utils import save_model
    run = KGWAS(tiny, device='cpu', seed=1)
    run.initialize_model()
    assert sorted(run.config) == ['gat_num_head', 'gnn_aggr', 'gnn_backbone', 'gnn_hidden_dim', 'gnn_num_layers']
    run.initialize_model(gat_dropout=0.0)
    assert 'gat_dropout' not in run.config
    run.initialize_model(gat_dropout=0.25)
    assert run.config['gat_dropout'] == 0.25
    path = os.path.join(str(tmp_path), 'ckpt')
    save_model(run.model, run.config, path)
    with open(os.path.join(path, 'config.pkl'), 'rb') as f:
        assert pickle.load(f)['gat_dropout'] == 0.25
    run2 = KGWAS(tiny, device='cpu', seed=2)
    run2.load_pretrained(path)
    assert run2.config == run.config and run2.model.gat_dropout == 0.25
