"""CPU: the hidden-state dropout rule (gnn_dropout=p) -- its numpy twin's statistics, the header's text, the C ABI's refusals (by
value: nothing here can launch) and the host-side plumbing that needs no GPU (construction-time refusals, config, checkpoints)."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from tests import attn_dropout_ref as A
from tests import hidden_dropout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 1 << 13                                  # x 128 columns = 2^20 elements
N = ROWS * R.C
WORDS = [R.dropout_word(0, 0, 0), R.dropout_word(42, 3, 17)]


@pytest.mark.parametrize('p', [0.1, 0.5, 0.9])
def test_keep_fraction_is_one_minus_p(p):
    """2^20 elements, two words, two layers, two node types: the kept fraction lies within 5 sigma of the binomial's 1 - p,
    sigma = sqrt(p (1 - p) / n) -- a bound derived from the binomial, not measured; the twin alone has to meet it."""
    sigma = np.sqrt(p * (1 - p) / N)
    for w in WORDS:
        for layer in (1, 2):
            for t in (0, 3):
                f = float(R.keep(w, layer, t, ROWS, p).mean())
                print(f'p {p} word {w:#x} layer {layer} type {t}: kept {f:.6f} ({(f - (1 - p)) / sigma:+.2f} sigma)')
                assert abs(f - (1 - p)) <= 5 * sigma, (p, w, layer, t, f)


def test_masks_differ_between_layers_types_words_and_from_the_attention_masks():
    """At p = 0.5 two independent masks agree on half the elements (5 sigma of 2^20 fair coins)."""
    sigma = 0.5 / np.sqrt(N)
    w = WORDS[1]
    a = R.keep(w, 1, 0, ROWS, 0.5)
    others = {'layer': R.keep(w, 2, 0, ROWS, 0.5), 'type': R.keep(w, 1, 1, ROWS, 0.5), 'word': R.keep(WORDS[0], 1, 0, ROWS, 0.5),
              'word + 1': R.keep(w + 1, 1, 0, ROWS, 0.5),
              # the attention-dropout mask of the same (word, layer) over the same running index row * 128 + c
              'attention': A.keep(w, 1, np.arange(N), 0.5).reshape(ROWS, R.C)}
    for what, b in others.items():
        agree = float((a == b).mean())
        print(f'{what}: agree on {agree:.6f}')
        assert not np.array_equal(a, b) and abs(agree - 0.5) <= 5 * sigma, what
    assert np.array_equal(a, R.keep(w, 1, 0, ROWS, 0.5))                                   # a pure function
    # the rows of a longer matrix are the rows of a shorter one: no size enters
    assert np.array_equal(a[:100], R.keep(w, 1, 0, 100, 0.5)) and np.array_equal(a[100:200], R.keep(w, 1, 0, 100, 0.5, row0=100))


def test_p_zero_keeps_everything_and_the_scale_is_float32():
    assert R.thresh(0.0) == 0 and bool(R.keep(WORDS[0], 1, 0, 1000, 0.0).all())
    f = R.factor(WORDS[0], 2, 1, 100, 0.1)
    assert f.dtype == np.float32 and set(f.reshape(-1).tolist()) == {0.0, float(np.float32(1.0 / 0.9))}
    y = np.random.default_rng(0).standard_normal((64, R.C)).astype(np.float32)
    assert np.array_equal(R.apply(y, WORDS[0], 1, 0, 0.0).view(np.uint32), y.view(np.uint32))
    y[0, 0], y[1, 1] = np.nan, np.inf
    out = R.apply(y, WORDS[1], 1, 0, 0.5)
    k = R.keep(WORDS[1], 1, 0, 64, 0.5)
    assert np.all(out[~k] == 0.0) and not np.signbit(out[~k]).any()


def test_header_names_the_rule():
    hdr = open(os.path.join(ROOT, 'include', 'kgwas_hip.h')).read()
    for name in ('KGW_HDROP_TAG', 'kgwhdrop_base', 'kgwhdrop_keep', 'KgwHDropJob', 'kgw_hidden_dropout', 'floor(p * 2^32)',
                 'kgwfan_step(kgwfan_step(kgwdrop_base(word, layer), KGW_HDROP_TAG), (uint32_t)type)',
                 'kgwfan_mix32(base ^ (row * 128u + col)) >= thresh'):
        assert name in hdr, name
    tag = int(hdr.split('#define KGW_HDROP_TAG', 1)[1].split()[0].rstrip('u'))
    assert tag == R.HDROP_TAG == int.from_bytes(b'hdrp', 'big')
    assert hdr.index('int kgwdrop_keep(') < hdr.index('#define KGW_HDROP_TAG') < hdr.index('int kgw_gat_aggregate_fwd')
    assert '#define KGW_VERSION      125' in hdr


def test_symbol_binding_and_struct_sizes():
    from kgwas_amd import _lib
    L = _lib.lib()
    assert hasattr(L, 'kgw_hidden_dropout') and _lib.has_hidden_dropout() and 'kgw_hidden_dropout' in _lib.EXPORTS
    assert L.kgw_version() == 125
    j = _lib.KgwHDropJob
    assert C.sizeof(j) == 40 and (j.src.offset, j.lds.offset, j.dst.offset, j.ldd.offset, j.rows.offset, j.type.offset) == (0, 8, 16, 24, 32, 36)
    # the ABI is the one it was: the calls with 7 and with 8 entries answer as before
    s7, s8 = (C.c_int64 * 7)(), (C.c_int64 * 8)()
    assert L.kgw_struct_sizes(s7, 7) == 0 and L.kgw_struct_sizes(s8, 8) == 0
    assert list(s7) == list(s8)[:7] and s8[4] == C.sizeof(_lib.KgwLayerArgs) and s8[7] == C.sizeof(_lib.KgwEdgeAttr)


def _job(rows=4, src=None, dst=None, lds=128, ldd=128, t=0):
    from kgwas_amd import _lib
    j = _lib.KgwHDropJob()
    j.src, j.lds, j.dst, j.ldd, j.rows, j.type = src, lds, dst, ldd, rows, t
    return j


def test_refusals_by_value_before_any_launch():
    """Every call here is refused (or has no rows) before a kernel could be launched: the pointers are host memory or NULL."""
    from kgwas_amd import _lib
    L = _lib.lib()
    E_NULL, E_RANGE, E_UNSUPPORTED = -1, -2, _lib.KGW_E_UNSUPPORTED
    buf = np.zeros(8 * 128 + 8, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16                     # a 16-byte aligned host address
    word = np.zeros(1, dtype=np.uint64)
    wp = word.ctypes.data

    def call(jobs, n=None, layer=1, w=wp, thresh=1 << 31, scale=2.0):
        arr = (_lib.KgwHDropJob * max(1, len(jobs)))(*jobs)
        return L.kgw_hidden_dropout(len(jobs) if n is None else n, arr, layer, w, thresh, scale, None)

    good = _job(4, p, p)
    assert L.kgw_hidden_dropout(1, None, 1, wp, 0, 1.0, None) == E_NULL
    assert call([good], w=None) == E_NULL
    assert call([_job(4, None, p)]) == E_NULL and call([_job(4, p, None)]) == E_NULL
    assert call([good], n=0) == E_RANGE and call([good] * 8, n=9) == E_RANGE and call([good], n=-1) == E_RANGE
    assert call([good], layer=0) == E_RANGE and call([good], layer=-3) == E_RANGE
    for bad in (0.5, 0.999, float('inf'), float('nan'), -2.0):
        assert call([good], scale=bad) == E_RANGE, bad
    assert call([_job(-1, p, p)]) == E_RANGE
    assert call([_job((1 << 25) + 1, p, p)]) == E_RANGE                # row * 128 + c must fit 32 bits
    assert call([_job(4, p, p, lds=64)]) == E_RANGE and call([_job(4, p, p, ldd=124)]) == E_RANGE
    assert call([_job(4, p + 4, p)]) == E_UNSUPPORTED and call([_job(4, p, p + 8)]) == E_UNSUPPORTED
    assert call([_job(4, p, p, lds=130)]) == E_UNSUPPORTED and call([_job(4, p, p, ldd=258)]) == E_UNSUPPORTED
    assert call([good, _job(4, p, p, lds=130)]) == E_UNSUPPORTED       # any job of the list
    # jobs without rows launch nothing: 0
    assert call([_job(0, p, p), _job(0, None, None)]) == 0


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path_factory.mktemp('hdrop')))


def test_construction_and_refusals(tiny):
    from kgwas_amd.kgwas import KGWAS
    run = KGWAS(tiny, device='cpu', seed=1)
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError):
            run.initialize_model(gnn_dropout=bad)
    with pytest.raises(ValueError):
        run.initialize_model(gnn_num_layers=1, gnn_dropout=0.2)
    run.initialize_model(gnn_num_layers=1)                                   # (no dropout: one layer as before)
    for kw in ({'gnn_backbone': 'SAGE'}, {'gnn_aggr': 'max'}, {'gat_num_head': 2}, {'gat_sigmoid': True}, {'gat_dropout': 0.1},
               {'gnn_num_layers': 3}):
        run.initialize_model(gnn_dropout=0.2, **kw)                          # independent of the backbone and of every switch
        assert run.model.gnn_dropout == 0.2
    run.initialize_model(gnn_dropout=0.2)
    m = run.model
    assert m.gnn_dropout == 0.2 and m.gat_dropout == 0.0 and m.fold_fc
    m.train()
    assert m._hidden_dropout()[0] == 0.2 and m._hidden_dropout()[1] is m.drop_word and m._dropout() is None
    m.eval()
    assert m._hidden_dropout() is None
    with pytest.raises(NotImplementedError):
        run.train(epoch=1, parallelism='shard')
    run.initialize_model()
    run.model.train()
    assert run.model.gnn_dropout == 0.0 and run.model._hidden_dropout() is None


def test_config_carries_the_key_only_when_set(tiny, tmp_path):
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.utils import save_model
    run = KGWAS(tiny, device='cpu', seed=1)
    run.initialize_model()
    default = dict(run.config)
    assert sorted(default) == ['gat_num_head', 'gnn_aggr', 'gnn_backbone', 'gnn_hidden_dim', 'gnn_num_layers']
    run.initialize_model(gnn_dropout=0.0)
    assert run.config == default
    run.initialize_model(gnn_dropout=0.2)
    assert run.config == dict(default, gnn_dropout=0.2)
    path = os.path.join(str(tmp_path), 'ckpt')
    save_model(run.model, run.config, path)
    with open(os.path.join(path, 'config.pkl'), 'rb') as f:
        assert pickle.load(f)['gnn_dropout'] == 0.2
    run2 = KGWAS(tiny, device='cpu', seed=2)
    run2.load_pretrained(path)
    assert run2.config == run.config and run2.model.gnn_dropout == 0.2 and 'drop_word' not in run2.model.state_dict()
