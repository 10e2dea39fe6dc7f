"""The consumer side of ops.GradSink on CPU tensors with no GPU and no library: what it holds (GradRecord), how launches are parked
in it (park_*), issued on their own (settle), carried by later launches (ride_*) or merged ahead of the optimiser's (flush), and how
the optimiser settles the books (claim).  The stand-in for _lib.lib() records the name of every entry called and returns 0.

The expected call lists of the settle and flush cases were written down from the PARENT of the commit that introduced settle / park /
ride / claim, not from the new code:

    python tests/test_grad_sink_protocol.py

prints every such case's list; run on that parent, where it first gives the old GradSink the new names (bare tuples in the same
field order, ``settle`` = its pair launch_pending_tail(); launch_pending_reduce())."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kgwas_amd import _lib, ops      # noqa: E402

REDUCE, FOLD, RELVEC, RFOLD = 'kgw_tn_reduce_launch', 'kgw_fold_bwd', 'kgw_relvec_bwd_multi', 'kgw_readout_train_fold'
TAIL, MULTI = 'kgw_param_tail', 'kgw_tn_gemm_multi_partial'
SLOTS = ('fold_bwd', 'relvec_bwd', 'pending_reduce', 'pending_fold')


class _Lib:
    """``calls``: the entries called, in order; ``rows``: per grouped launch the row counts of its jobs, in grid order.  ``rc``:
    entry -> a status other than 0.  (The workspace-size query launches nothing and is not recorded.)"""

    def __init__(self, rc=None):
        self.calls, self.rows, self.rc = [], [], rc or {}

    def kgw_tn_gemm_workspace_floats(self, rows, M, N):
        return 0

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append(name)
            if name in (TAIL, MULTI):
                self.rows.append([args[1][k].rows for k in range(args[0])])
            return self.rc.get(name, 0)
        return entry


def _install(setattr_, rc=None):
    lib = _Lib(rc)
    setattr_(_lib, 'lib', lambda: lib)
    setattr_(_lib, 'stream_ptr', lambda: None)
    for switch in ('_PARAM_TAIL', '_DEFER_PRODUCTS', '_DEFER_REDUCE'):       # (whatever the environment says)
        setattr_(ops, switch, True)
    return lib


@pytest.fixture
def lib(monkeypatch):
    return _install(monkeypatch.setattr)


# ---- filling the slots: empty structs, CPU tensors of distinct sizes as the leaf gradients the launches write -------------------
def _fold(outs, dU=None):
    a = _lib.KgwFoldArgs()
    a.dU = dU                              # (None: equal to an empty job's dU_full -- the fold IS that job's; else no job's)
    return ops.ParkedFoldBwd(a, 'fold operands', ops._outs(outs))


def _relvec(outs):
    return ops.ParkedRelvecBwd(1, (_lib.KgwRelvecJob * 1)(), 'relvec operands', ops._outs(outs))


def _reduce():
    return ops.ParkedReduce(_lib.KgwTnReducePlan(), 'workspaces')


def _rfold():
    return ops.ParkedReadoutFold(_lib.KgwReadoutFold(), 'partials')


def _product(rows):
    dY, X, dW, db = torch.zeros(rows, 4), torch.zeros(rows, 6), torch.empty(4, 6), torch.empty(4)
    return ops.DeferredProduct(dY, X, dW.data_ptr(), db.data_ptr(), (dW, db), None), [dW, db]


def _sink(slots=(), products=(), fold_dU=None):
    """A GradSink with ``slots`` filled and ``products`` (row counts) deferred; also the tensors every launch is to write."""
    sink, outs = ops.GradSink(), {}
    for slot in slots:
        outs[slot] = [torch.empty(3 + len(outs)), torch.empty(7 + len(outs))] if slot in ('fold_bwd', 'relvec_bwd') else []
    make = {'fold_bwd': lambda: _fold(outs['fold_bwd'], fold_dU), 'relvec_bwd': lambda: _relvec(outs['relvec_bwd']),
            'pending_reduce': _reduce, 'pending_fold': _rfold}
    for slot in slots:
        setattr(sink, slot, make[slot]())
    written = [t for ts in outs.values() for t in ts]
    for rows in products:
        p, ts = _product(rows)
        sink.products.append(p)
        written += ts
    return sink, written


def _parked(sink):
    return [slot for slot in SLOTS if getattr(sink, slot) is not None]


def _sourceless(sink, tensors):
    """Every tensor of ``tensors``, and nothing else, has a source-less record with its numel."""
    assert sorted(sink.records) == sorted(t.data_ptr() for t in tensors)
    for t in tensors:
        r = sink.records[t.data_ptr()]
        assert isinstance(r, ops.GradRecord) and r.src is None and r.numel == t.numel() and r[0] is None


# name -> (slots filled, the calls in order, slots still filled afterwards): the parent's lists
SETTLE = {
    'all four': (SLOTS, [REDUCE, FOLD, RELVEC], ['pending_fold']),
    'fold alone': (('fold_bwd',), [FOLD], []),
    'relation vectors alone': (('relvec_bwd',), [RELVEC], []),
    'reduce alone': (('pending_reduce',), [REDUCE], []),
    'read-out fold alone': (('pending_fold',), [], ['pending_fold']),
}
# name -> (_sink keywords, status of kgw_param_tail, the calls in order, tail_taken, row counts per grouped launch)
FLUSH = {
    'no product, a parked tail': (dict(slots=SLOTS), 0, [REDUCE, RFOLD, TAIL], 1, [[]]),
    'the fold is not the relation job\'s': (dict(slots=SLOTS[:2], fold_dU=4096), 0, [FOLD, RELVEC], 0, []),
    'kgw_param_tail unsupported': (dict(slots=SLOTS[:2], products=[9]), _lib.KGW_E_UNSUPPORTED, [TAIL, FOLD, RELVEC, MULTI], 0,
                                   [[9], [9]]),
    'a fold without relation vectors': (dict(slots=SLOTS[:1], products=[9]), 0, [FOLD, MULTI], 0, [[9]]),
    'five products': (dict(products=[10, 50, 30, 20, 40]), 0, [MULTI, MULTI], 0, [[50, 40, 30, 20], [10]]),
}


@pytest.mark.parametrize('name', list(SETTLE))
def test_settle(monkeypatch, name):
    slots, calls, left = SETTLE[name]
    lib = _install(monkeypatch.setattr)
    sink, written = _sink(slots)
    sink.settle()
    assert lib.calls == calls and _parked(sink) == left
    _sourceless(sink, written)
    assert sink.tail_taken == sink.reduces_ridden == sink.folds_ridden == 0


@pytest.mark.parametrize('name', list(FLUSH))
def test_flush(monkeypatch, name):
    kw, rc, calls, taken, rows = FLUSH[name]
    lib = _install(monkeypatch.setattr, {TAIL: rc})
    sink, written = _sink(**kw)
    expected = []
    real = sink.expect
    monkeypatch.setattr(sink, 'expect', lambda *outs: (expected.extend(o[0] for o in outs), real(*outs)))
    sink.flush()
    assert lib.calls == calls and lib.rows == rows and sink.tail_taken == taken
    assert _parked(sink) == [] and sink.products == []
    _sourceless(sink, written)                                   # (the stand-in leaves kind 0: every product "came out complete")
    assert len(expected) == len(set(expected))                   # nothing registered twice
    assert sink.reduces_ridden == sink.folds_ridden == 0


# ---- parking ----------------------------------------------------------------------------------------------------------------------
def _park_fold(sink):
    return sink.park_fold_bwd(_lib.KgwFoldArgs(), 'operands', [torch.empty(3)])


def _park_relvec(sink):
    return sink.park_relvec_bwd(1, (_lib.KgwRelvecJob * 1)(), 'operands', [torch.empty(5), torch.empty(6)])


def test_parking_takes_a_free_slot_and_lists_the_outputs(lib):
    sink = ops.GradSink()
    assert _park_fold(sink) and _park_relvec(sink)               # (the relation vectors behind a parked fold: their own slot is free)
    assert [o[1] for o in sink.fold_bwd.outs] == [3] and [o[1] for o in sink.relvec_bwd.outs] == [5, 6] and sink.relvec_bwd.n == 1
    assert not sink.records and not lib.calls                    # (registered when issued, not when parked)


@pytest.mark.parametrize('taken', ['fold_bwd', 'relvec_bwd'])
def test_the_fold_is_refused_when_either_slot_is_taken(lib, taken):
    sink, _ = _sink([taken])
    was = getattr(sink, taken)
    assert not _park_fold(sink) and getattr(sink, taken) is was
    assert _park_relvec(sink) == (taken == 'fold_bwd')           # the relation vectors: only their own slot counts


@pytest.mark.parametrize('switch', ['_PARAM_TAIL', '_DEFER_PRODUCTS'])
def test_both_are_refused_with_a_switch_off(lib, monkeypatch, switch):
    monkeypatch.setattr(ops, switch, False)
    sink = ops.GradSink()
    assert not _park_fold(sink) and not _park_relvec(sink) and _parked(sink) == []


def test_parking_the_second_launches(lib, monkeypatch):
    sink, plan = ops.GradSink(), _lib.KgwTnReducePlan()
    dW, db, dw, dbl = torch.empty(8), torch.empty(2), torch.empty(4), torch.empty(1)
    plan.blocks = ops._RIDE_MAX_BLOCKS + 1
    assert not sink.park_reduce(plan, 'ws', dW, db) and sink.pending_reduce is None and not sink.records
    plan.blocks = ops._RIDE_MAX_BLOCKS
    assert sink.park_reduce(plan, 'ws', dW, db) and sink.pending_reduce.plan is plan
    _sourceless(sink, [db])                                      # (d W goes on through the relation vectors' node)
    assert sink.park_readout_fold('fold', 'partials', dw, dbl) and sink.pending_fold.fold == 'fold'
    _sourceless(sink, [db, dw, dbl])
    assert not sink.park_readout_fold('another', 'partials', dw, dbl) and sink.pending_fold.fold == 'fold'
    monkeypatch.setattr(ops, '_DEFER_REDUCE', False)
    assert not ops.GradSink().park_reduce(plan, 'ws', dW, db)


# ---- riding -----------------------------------------------------------------------------------------------------------------------
def test_riding_empties_the_slot_keeps_the_record_and_counts_once(lib):
    sink, _ = _sink(('pending_reduce', 'pending_fold'))
    r, f = sink.pending_reduce, sink.pending_fold
    assert sink.ride_reduce() is r and sink.pending_reduce is None and sink.keep == [r] and sink.reduces_ridden == 1
    assert sink.ride_fold() is f and sink.pending_fold is None and sink.keep == [r, f] and sink.folds_ridden == 1
    assert sink.ride_reduce() is None and sink.ride_fold() is None             # empty slots: nothing, and nothing counted
    assert sink.keep == [r, f] and (sink.reduces_ridden, sink.folds_ridden) == (1, 1) and not lib.calls


# ---- claim ------------------------------------------------------------------------------------------------------------------------
def _sourced(sink, g):
    src = _lib.KgwGradSrc()
    src.kind, src.nblk = 1, 3
    sink.add(g, src, torch.empty(2))


def test_claim_returns_the_sourced_records_by_parameter(lib):
    sink = ops.GradSink()
    g = [torch.empty(4), torch.empty(5), torch.empty(6)]
    _sourced(sink, g[0])
    sink.expect(*ops._outs([g[1]]))                              # (matched, not returned; g[2]: a complete tensor nobody announced)
    p, (dW, db) = _product(9)
    sink.products.append(p)
    assert sink.deferred_gradients == 1 + 2
    got = sink.claim(dict(enumerate(g + [dW, db])))
    assert lib.calls == [MULTI]                                  # (it flushes first)
    assert list(got) == [0] and got[0].src.kind == 1 and got[0].src.nblk == 3 and got[0].numel == 4 and got[0][0] is got[0].src
    assert not sink.records and sink.deferred_gradients == 0


def test_claim_refuses_a_record_that_describes_another_tensor(lib):
    sink, g = ops.GradSink(), torch.empty(4)
    sink.expect((g.data_ptr(), 5, g.untyped_storage()))
    with pytest.raises(ops.GradSinkMismatch, match='does not describe'):
        sink.claim({'w': g})


def test_claim_fails_on_a_left_over_record_and_clears_the_books(lib):
    sink, g, lost = ops.GradSink(), torch.empty(4), torch.empty(4)
    _sourced(sink, g)
    _sourced(sink, lost)
    with pytest.raises(ops.GradSinkMismatch, match='1 deferred gradient'):
        sink.claim({'w': g})
    assert sink.records == {}


def test_claim_goes_through_take(lib, monkeypatch):
    seen, real = [], ops.GradSink.take
    monkeypatch.setattr(ops.GradSink, 'take', lambda self, grad: (seen.append(grad), real(self, grad))[1])
    sink, g = ops.GradSink(), [torch.empty(4), torch.empty(5)]
    _sourced(sink, g[1])
    assert list(sink.claim(dict(enumerate(g)))) == [1] and seen[0] is g[0] and seen[1] is g[1] and len(seen) == 2


if __name__ == '__main__':
    if not hasattr(ops.GradSink, 'settle'):                      # the parent: the old forms under the new names
        ops.ParkedFoldBwd = ops.ParkedRelvecBwd = ops.ParkedReduce = ops.ParkedReadoutFold = lambda *fields: fields
        ops.DeferredProduct = lambda dY, X, dW, db, keep, rows_dev: (dY, X, dW, db, keep, keep, rows_dev)
        ops._outs = lambda tensors: [(t.data_ptr(), t.numel(), t.untyped_storage()) for t in tensors]
        ops.GradSink.settle = lambda self: (self.launch_pending_tail(), self.launch_pending_reduce())
    for name, (slots, _, _) in SETTLE.items():
        lib = _install(setattr)
        sink, _ = _sink(slots)
        sink.settle()
        print(f'settle | {name}: {lib.calls}, still parked {_parked(sink)}, {len(sink.records)} records')
    for name, (kw, rc, _, _, _) in FLUSH.items():
        lib = _install(setattr, {TAIL: rc})
        sink, _ = _sink(**kw)
        sink.flush()
        print(f'flush | {name}: {lib.calls}, tail_taken {sink.tail_taken}, rows {lib.rows}, {len(sink.records)} records')
