"""CPU: the weight-averaging rule (include/kgwas_hip.h: KgwWeightAvg, kgwavg_alpha; the host export kgw_weight_avg_alpha), its
ctypes mirror and optim.parse_weight_average, against the restatement of tests/weight_avg_ref.py.  No kernel is launched."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

from tests import weight_avg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['kgw_weight_avg_update', 'kgw_weight_avg_alpha']


def _cfg(kind, start_step=1, every=1, warmup=True, decay=0.999):
    from kgwas_amd import _lib
    return _lib.KgwWeightAvg(R.KINDS[kind], start_step, every, int(warmup), decay)


def _alpha(cfg, n):
    from kgwas_amd import _lib
    ev = C.c_int32(-7)
    a = _lib.lib().kgw_weight_avg_alpha(C.byref(cfg), n, C.byref(ev))
    return ev.value, a


def _bad_configs():
    from kgwas_amd._lib import KgwWeightAvg as A
    return [A(2, 1, 1, 1, 0.9), A(-1, 1, 1, 1, 0.9), A(0, 0, 1, 1, 0.9), A(0, -3, 1, 1, 0.9), A(1, 0, 1, 0, 0.0), A(0, 1, 0, 1, 0.9),
            A(1, 1, 0, 0, 0.0), A(1, 1, -1, 0, 0.0), A(0, 1, 1, 2, 0.9), A(0, 1, 1, -1, 0.9), A(0, 1, 1, 1, 0.0), A(0, 1, 1, 1, 1.0),
            A(0, 1, 1, 1, -0.5), A(0, 1, 1, 1, 1.5), A(0, 1, 1, 0, float('nan')), A(0, 1, 1, 0, float('inf'))]


def test_header_names_the_rule_and_the_mirror_matches():
    from kgwas_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, 'include', 'kgwas_hip.h')).read()
    for word in ('typedef struct KgwWeightAvg', 'KGW_AVG_EMA = 0', 'KGW_AVG_SWA = 1', 'kgwavg_alpha', 'kgwavg_valid',
                 '#define KGW_WEIGHT_AVG_MAX 64', '#define KGW_WEIGHT_AVG_UNIT 1024', 'fmaf(alpha, p - s, s)'):
        assert word in hdr, word
    assert re.search(r'KGWFAN_INLINE int kgwavg_alpha\(const KgwWeightAvg\* \w+, int32_t n, float\* alpha\)', hdr)
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS and re.search(r'\b' + name + r'\s*\(', hdr), name
    assert _lib.has_weight_avg()
    assert L.kgw_version() == 125 and re.search(r'#define KGW_VERSION\s+125\b', hdr)           # detected by symbol: the version stays
    assert (_lib.KGW_AVG_EMA, _lib.KGW_AVG_SWA) == (0, 1) and _lib.AVG_KINDS == R.KINDS
    assert (_lib.WEIGHT_AVG_MAX, _lib.WEIGHT_AVG_UNIT) == (64, 1024)
    # the struct: five 4-byte fields, no padding
    A = _lib.KgwWeightAvg
    assert [f[0] for f in A._fields_] == ['kind', 'start_step', 'every', 'warmup', 'decay']
    assert [getattr(A, f[0]).offset for f in A._fields_] == [0, 4, 8, 12, 16] and C.sizeof(A) == 20
    # the eleventh entry of kgw_struct_sizes; the first ten keep their values and shorter calls their results
    s11 = (C.c_int64 * 12)(*([-1] * 12))
    assert L.kgw_struct_sizes(s11, 11) == 0 and s11[10] == C.sizeof(A) and s11[11] == -1
    mine = [C.sizeof(_lib.KgwGraph), C.sizeof(_lib.KgwBatchMeta), C.sizeof(_lib.KgwChunk), C.sizeof(_lib.KgwBatchBuf),
            C.sizeof(_lib.KgwLayerArgs), C.sizeof(_lib.KgwTnJob), C.sizeof(_lib.KgwGradSrc), C.sizeof(_lib.KgwEdgeAttr),
            C.sizeof(_lib.KgwLrSchedule), C.sizeof(_lib.KgwOptimCtl)]
    assert list(s11)[:10] == mine and mine[8:] == [24, 40]
    for n in (0, 1, 7, 8, 10):
        s = (C.c_int64 * 12)(*([-1] * 12))
        assert L.kgw_struct_sizes(s, n) == 0 and list(s) == mine[:n] + [-1] * (12 - n), n
    s = (C.c_int64 * 12)(*([-1] * 12))
    assert L.kgw_struct_sizes(s, 12) == 0 and list(s) == list(s11)                               # (nothing past the eleventh)


CASES = [dict(start_step=s, every=e) for s, e in itertools.product((1, 3, 7), (1, 2, 5))]


@pytest.mark.parametrize('kind,warmup,decay', [('ema', True, 0.5), ('ema', False, 0.5), ('ema', True, 0.999), ('ema', False, 0.999),
                                               ('swa', False, 0.0)])
def test_host_rule_equals_the_restatement(kind, warmup, decay):
    """n = 1 .. 40 at start_step 1, 3, 7 x every 1, 2, 5: an event exactly where the rule says, alpha equal as float32.  decay 0.5
    with the warm-up: (1 + k) / (10 + k) reaches the cap at k = 8, inside the range."""
    events = 0
    for case in CASES:
        cfg = _cfg(kind, warmup=warmup, decay=decay, **case)
        kw = dict(case, warmup=warmup, decay=decay)
        for n in range(1, 41):
            ev, a = _alpha(cfg, n)
            ref_ev, ref_a = R.alpha_at(kind, n, **kw)
            want = n >= case['start_step'] and (n - case['start_step']) % case['every'] == 0
            assert bool(ev) == ref_ev == want, (kind, kw, n)
            if not ev:
                assert a == 0.0
                continue
            events += 1
            assert np.float32(a) == ref_a and a == float(np.float32(a)), (kind, kw, n, a, ref_a)
            k = (n - case['start_step']) // case['every']
            if k == 0:
                assert a == 1.0                                                    # the first event is a copy, both kinds
            elif kind == 'swa':
                assert a == float(np.float32(1.0) / np.float32(k + 1))
            elif not warmup:
                assert a == float(np.float32(1.0) - np.float32(decay))
    assert events > 100
    if kind == 'ema' and warmup and decay == 0.5:                                  # the cap binds from k = 8 on, not before
        cfg = _cfg('ema', warmup=True, decay=0.5)
        alphas = [_alpha(cfg, 1 + k)[1] for k in range(0, 12)]
        assert alphas[0] == 1.0 and all(a > 0.5 for a in alphas[1:8]) and all(a == 0.5 for a in alphas[8:])
        assert alphas[1] == float(np.float32(1.0) - np.float32(2.0) / np.float32(11.0))


def test_refused_configurations():
    """Whatever kgwavg_valid refuses: NaN from the host evaluation, KGW_E_RANGE from the entry point -- before any launch (no GPU
    here) and before anything else is looked at; a NULL cfg or table: KGW_E_NULL."""
    from kgwas_amd import _lib
    from kgwas_amd.optim import parse_weight_average
    L = _lib.lib()
    one = (C.c_int64 * 1)(4)
    for cfg in _bad_configs():
        what = (cfg.kind, cfg.start_step, cfg.every, cfg.warmup, cfg.decay)
        ev = C.c_int32(-7)
        assert math.isnan(L.kgw_weight_avg_alpha(C.byref(cfg), 1, C.byref(ev))) and ev.value == 0, what
        assert L.kgw_weight_avg_update(0, None, None, None, None, C.byref(cfg), None) == -2, what
        assert L.kgw_weight_avg_update(1, None, None, one, None, C.byref(cfg), None) == -2, what
        with pytest.raises(ValueError):
            parse_weight_average(cfg)
    ok = _cfg('ema')
    assert math.isnan(L.kgw_weight_avg_alpha(None, 1, None)) and math.isnan(L.kgw_weight_avg_alpha(C.byref(ok), 0, None))
    assert L.kgw_weight_avg_alpha(C.byref(ok), 1, None) == 1.0
    # SWA reads neither warmup nor decay
    assert _alpha(_lib.KgwWeightAvg(1, 1, 1, 5, float('nan')), 2) == (1, 0.5)
    assert L.kgw_weight_avg_update(0, None, None, None, None, None, None) == -1
    assert L.kgw_weight_avg_update(0, None, None, None, None, C.byref(ok), None) == 0
    assert L.kgw_weight_avg_update(65, None, None, None, None, C.byref(ok), None) == -2
    assert L.kgw_weight_avg_update(-1, None, None, None, None, C.byref(ok), None) == -2
    assert L.kgw_weight_avg_update(1, None, None, None, None, C.byref(ok), None) == -1


def test_parse_weight_average():
    from kgwas_amd import _lib
    from kgwas_amd.optim import parse_weight_average
    assert parse_weight_average(None, 10) is None

    def fields(a):
        return (a.kind, a.start_step, a.every, a.warmup, a.decay)
    f999 = float(np.float32(0.999))
    assert fields(parse_weight_average('ema', 10)) == (0, 1, 1, 1, f999)
    assert fields(parse_weight_average('swa', 10))[:3] == (1, 1, 1)
    assert fields(parse_weight_average(0.5, 10)) == (0, 1, 1, 1, 0.5)
    assert fields(parse_weight_average(np.float32(0.25))) == (0, 1, 1, 1, 0.25)
    assert fields(parse_weight_average({'kind': 'ema', 'decay': 0.75, 'warmup': False, 'start_step': 7, 'every': 'epoch'}, 13)) == \
        (0, 7, 13, 0, 0.75)
    assert fields(parse_weight_average({'kind': 'swa', 'start_step': np.int64(30), 'every': 5.0}))[:3] == (1, 30, 5)
    s = parse_weight_average({'kind': 'ema'}, 3)
    assert fields(s) == (0, 1, 1, 1, f999) and parse_weight_average(s) is s
    bad = ['emma', '', 7, 1, 0, 1.0, 0.0, -0.5, float('nan'), float('inf'), True, False, ['ema'], ('ema', 0.9), {}, {'decay': 0.9},
           {'kind': 'EMA'}, {'kind': 0}, {'kind': 'ema', 'decay': 1.0}, {'kind': 'ema', 'decay': 0.0}, {'kind': 'ema', 'decay': '0.9'},
           {'kind': 'ema', 'decay': True}, {'kind': 'ema', 'decay': float('nan')}, {'kind': 'ema', 'decay': 1.0 - 1e-12},
           {'kind': 'ema', 'start_step': 0}, {'kind': 'ema', 'start_step': 1.5}, {'kind': 'ema', 'start_step': 2 ** 31},
           {'kind': 'ema', 'start_step': True}, {'kind': 'ema', 'every': 0}, {'kind': 'ema', 'every': -2}, {'kind': 'ema', 'every': 'step'},
           {'kind': 'ema', 'every': 2.5}, {'kind': 'ema', 'warmup': 2}, {'kind': 'ema', 'warmup': 'yes'}, {'kind': 'ema', 'warmup': None},
           {'kind': 'swa', 'decay': 0.9}, {'kind': 'swa', 'warmup': False}, {'kind': 'ema', 'steps': 3},
           _lib.KgwWeightAvg(2, 1, 1, 1, 0.9)]
    for spec in bad:
        with pytest.raises(ValueError):
            parse_weight_average(spec, 10)
    with pytest.raises(ValueError):
        parse_weight_average({'kind': 'swa', 'every': 'epoch'})              # nobody named the batches of an epoch
    with pytest.raises(ValueError):
        parse_weight_average({'kind': 'swa', 'every': 'epoch'}, 0)
    # what the parser builds evaluates like the restatement
    s = parse_weight_average({'kind': 'ema', 'decay': 0.5, 'start_step': 3, 'every': 2}, 10)
    for n in range(1, 41):
        ev, a = _alpha(s, n)
        ref_ev, ref_a = R.alpha_at('ema', n, start_step=3, every=2, warmup=True, decay=0.5)
        assert bool(ev) == ref_ev and (not ev or np.float32(a) == ref_a)


def test_the_restatement_replays_a_trajectory():
    """weight_avg_ref.replay on numbers small enough to do by hand: SWA is the mean of the snapshots at its events, EMA the weighted
    sum, a non-event changes nothing and the first event forgets what the shadow held."""
    snaps = [[np.array([float(n), -2.0 * n])] for n in range(1, 9)]
    nan0 = [np.array([np.nan, np.nan])]
    swa = R.replay(nan0, snaps[:6], 'swa', start_step=3, every=2)                  # (events at 3 and 5: alpha 1 and 1/2, exact)
    assert np.array_equal(swa[0], np.array([4.0, -8.0]))
    swa = R.replay(nan0, snaps, 'swa', start_step=3, every=2)                      # (a third at 7: alpha = float32(1/3), 2^-25 off)
    assert np.allclose(swa[0], np.mean([[3.0, -6.0], [5.0, -10.0], [7.0, -14.0]], axis=0), rtol=1e-7, atol=0)
    assert np.isnan(R.replay(nan0, snaps[:2], 'swa', start_step=3, every=2)[0]).all()
    ema = R.replay(nan0, snaps[:3], 'ema', warmup=False, decay=0.5)
    assert np.array_equal(ema[0], np.array([0.25 * 1 + 0.25 * 2 + 0.5 * 3, -2 * (0.25 * 1 + 0.25 * 2 + 0.5 * 3)]))


def test_the_argument_exists_at_every_level_and_defaults_to_off():
    import inspect
    from kgwas_amd.graph_step import GraphTrainStep, keep_training_state
    from kgwas_amd.kgwas import KGWAS
    from kgwas_amd.optim import WeightAverage
    for fn in (KGWAS.train, GraphTrainStep.__init__, KGWAS._train_sharded):
        assert inspect.signature(fn).parameters['weight_average'].default is None
    assert inspect.signature(keep_training_state).parameters['avg'].default is None
    assert list(inspect.signature(WeightAverage.__init__).parameters)[1:] == ['model', 'opt', 'cfg']
