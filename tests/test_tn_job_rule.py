"""The job record and the eligibility rule of the grouped split-K weight-gradient kernel (ops._tn_job, ops._tn_multi_ok) on CPU
tensors: no GPU and no library -- the ctypes struct definitions and a stand-in for the one library call (the workspace size).

_tn_job must write every field of a KgwTnJob as the five sites that used to fill one by hand did -- one case per site's argument
pattern, strided views and colsum_repeat > 1 among them.  _tn_multi_ok: one case per clause, each failing that clause alone."""
import pytest
import torch

from kgwas_amd import _lib, ops


class _Lib:
    asked = []

    @classmethod
    def kgw_tn_gemm_workspace_floats(cls, rows, M, N):
        cls.asked.append((rows, M, N))
        return 7 * rows + 3 * M + N


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    _Lib.asked = []
    monkeypatch.setattr(_lib, 'lib', lambda: _Lib)


def _fields(j):
    return {name: getattr(j, name) or 0 for name, _ in _lib.KgwTnJob._fields_}


def _check(j, ws, A, B, **want):
    """The operand and workspace fields follow from A and B at every site; ``want``: the fields that differ between the sites."""
    rows, M, N = A.shape[0], A.shape[1], B.shape[1]
    assert _Lib.asked[-1] == (rows, M, N)
    assert ws.dtype == torch.float32 and ws.numel() == 7 * rows + 3 * M + N
    want.update(A=A.data_ptr(), lda=A.stride(0), B=B.data_ptr(), ldb=B.stride(0), rows=rows, M=M, N=N, workspace=ws.data_ptr(),
                workspace_floats=ws.numel())
    assert _fields(j) == want and len(want) == len(_lib.KgwTnJob._fields_)


def test_deferred_product_of_the_grad_sink():
    """GradSink._tn_jobs: raw addresses for the outputs (no second tensor reference), dense [M, N] and [M], the row count on the device."""
    dY, X, rows_dev = torch.randn(300, 128), torch.randn(300, 64), torch.tensor([290], dtype=torch.int32)
    dW, db = torch.empty(128, 64), torch.empty(128)
    jobs, src, keep = ops.GradSink()._tn_jobs([ops.DeferredProduct(dY, X, dW.data_ptr(), db.data_ptr(), None, rows_dev)])
    assert len(jobs) == 1 and len(src) == 2 and len(keep) == 1
    _check(jobs[0], keep[0], dY, X, C=dW.data_ptr(), ldc=64, colsum_a=db.data_ptr(), colsum_ld=128, rows_dev=rows_dev.data_ptr(),
           c_transposed=0, colsum_repeat=1)


def test_grouped_pair_of_weight_grads():
    """weight_grads: fresh dense outputs; the second operand a strided view (columns of a wider matrix)."""
    dY, X = torch.randn(1024, 128), torch.randn(1024, 96)[:, :64]
    dW, db = torch.empty(128, 64), torch.empty(128)
    j = _lib.KgwTnJob()
    ws = ops._tn_job(j, dY, X, dW.data_ptr(), X.shape[1], db.data_ptr(), dY.shape[1], rows_dev=None)
    assert X.stride(0) == 96
    _check(j, ws, dY, X, C=dW.data_ptr(), ldc=64, colsum_a=db.data_ptr(), colsum_ld=128, rows_dev=0, c_transposed=0, colsum_repeat=1)


def test_transposed_product_into_the_packed_relation_weights():
    """_tn_gemm_group and _transform_bwd_merged, the two routes of _LayerTransform.backward (one argument pattern): x = R relations'
    columns of the aggregate's output, the product stored TRANSPOSED into rows [lo, hi) of the packed [n, C, C] weights, the column
    sums written R times -- once per relation's bias row."""
    C, R, rows, lo = 128, 3, 40, 2
    Z, dz = torch.randn(500, C), torch.randn(rows, C)
    dWp, dbp = torch.empty(7, C, C), torch.empty(7, C)
    x = Z[120:120 + rows * R].view(rows, R * C)
    out, bs = dWp[lo:lo + R].view(R * C, C), dbp[lo:lo + R]
    j = _lib.KgwTnJob()
    ws = ops._tn_job(j, dz, x, out.data_ptr(), out.stride(0), bs.data_ptr(), bs.stride(0), c_transposed=True, colsum_repeat=bs.shape[0])
    _check(j, ws, dz, x, C=dWp.data_ptr() + 4 * lo * C * C, ldc=C, colsum_a=dbp.data_ptr() + 4 * lo * C, colsum_ld=C, rows_dev=0,
           c_transposed=1, colsum_repeat=R)
    assert _fields(j)['N'] == R * C and _fields(j)['ldb'] == R * C


def test_root_weight_slice_without_column_sums():
    """_root_weight_grad: slice t of the packed [n_types, 128, 128] gradient, no column sums."""
    g, x, dW = torch.randn(77, 128), torch.randn(200, 128)[:77], torch.zeros(4, 128, 128)
    j = _lib.KgwTnJob()
    ws = ops._tn_job(j, g, x, dW[2].data_ptr(), 128, 0, 128)
    _check(j, ws, g, x, C=dW.data_ptr() + 4 * 2 * 128 * 128, ldc=128, colsum_a=0, colsum_ld=128, rows_dev=0, c_transposed=0, colsum_repeat=1)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def _clauses(A, B):
    """The rule's clauses one by one, for the operand pair (A, B)."""
    d = {'fp32': A.dtype == torch.float32 and B.dtype == torch.float32, 'inner stride 1': A.stride(1) == 1 and B.stride(1) == 1,
         'rows': A.shape[0] == B.shape[0] and A.shape[0] > 0, 'even M': A.shape[1] % 2 == 0, 'even N': B.shape[1] % 2 == 0,
         '>= 64': A.shape[1] >= 64 and B.shape[1] >= 64, 'even row strides': A.stride(0) % 2 == 0 and B.stride(0) % 2 == 0,
         '8-byte aligned': A.data_ptr() % 8 == 0 and B.data_ptr() % 8 == 0}
    return [k for k, v in d.items() if not v]


def _good(rows=128):
    return torch.randn(rows, 64)


BAD = {                                                    # clause -> an operand [128, .] that fails it, and it alone
    'odd width': lambda: torch.randn(128, 66)[:, :65],
    'odd row stride': lambda: torch.randn(128, 67)[:, :64],
    '4-byte-misaligned base': lambda: torch.randn(128, 66)[:, 1:65],
    'width 62': lambda: torch.randn(128, 62),
    'float64': lambda: torch.randn(128, 64, dtype=torch.float64),
    'inner stride 2': lambda: torch.randn(128, 128)[:, ::2],
}
FAILS = {'odd width': None, 'odd row stride': 'even row strides', '4-byte-misaligned base': '8-byte aligned', 'width 62': '>= 64',
         'float64': 'fp32', 'inner stride 2': 'inner stride 1'}


def test_the_rule_takes_a_good_pair():
    A, B = _good(), _good()
    assert _clauses(A, B) == [] and ops._tn_multi_ok(A, B) and ops._tn_multi_ok(A, B, narrow=True)


@pytest.mark.parametrize('side', ['A', 'B'])
@pytest.mark.parametrize('what', list(BAD))
def test_each_clause_alone_refuses(what, side):
    bad = BAD[what]()
    A, B = (bad, _good()) if side == 'A' else (_good(), bad)
    clause = FAILS[what] or ('even M' if side == 'A' else 'even N')
    assert _clauses(A, B) == [clause], (what, _clauses(A, B))
    assert not ops._tn_multi_ok(A, B)
    # (the width clause is the only one ``narrow`` -- weight_grads' stated exception -- drops)
    assert ops._tn_multi_ok(A, B, narrow=True) == (what == 'width 62')


def test_no_rows_and_unequal_rows_refuse():
    A, B = _good(0), _good(0)
    assert _clauses(A, B) == ['rows'] and not ops._tn_multi_ok(A, B) and not ops._tn_multi_ok(A, B, narrow=True)
    assert not ops._tn_multi_ok(_good(128), _good(64))
