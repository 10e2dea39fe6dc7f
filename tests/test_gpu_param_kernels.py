"""The parameter-only kernels of a step -- k_relvec_fwd / k_relvec_bwd and k_param_tail (kgwas_amd/csrc/kgw_dense_relvec.h),
k_fold_fwd / k_fold_bwd (kgw_fold.hip), their one-wavefront copies (kgw_riders.h) -- called at the C ABI and compared with plain
float64 (tests/param_kernels_ref.py: kgwas/conv.py:138-151, kgwas/model.py:15,21 under float64 autograd) at the relation layouts
where each piece of index arithmetic can go wrong (param_kernels_ref.LAYOUTS: L1 .. L5).

Every output is pre-filled with NaN (every element must be written), a sentinel sits behind every buffer and in every tensor a
call must not write, inputs are randn and, second parametrisation, randn * 2^randint(-4, 4); no element is left out.  The bars:
  derived   |got - ref| <= (n_terms + 2) 2^-24 S element by element for every value of the fp32 pipe (fmaf chains, wave sums,
            mfma_f32_32x32x2f32): the first-order worst case of an fp32 sum of n_terms products in ANY order, S = sum |terms| from
            the reference's magnitude pass.  A dropped or doubled term is ~ S / n_terms, a thousand times the bar.  S == 0: exactly 0.0.
            The column sums of a weight-gradient product are plain fp32 sums of `rows` terms: the same bar with n_terms = rows.
  exact     bit-identity between variants (pieces / complete, a k-job call / k calls, v_by_rel 0 / 1, riders / stand-alone,
            merged tail / three launches, two runs), cleared buffers, sentinels;
  project   the weight-gradient products of k_param_tail (bf16 x 3 pipe): max |C - ref| / sum |a||b| <= 16 * 2^-24 after
            kgw_grad_finish, as test_tn_gemm_on_the_bf16_pipe_is_as_close_to_float64_as_on_the_fp32_pipe requires, and
            bit-identity with kgw_tn_gemm_multi_partial + kgw_grad_finish.
Under -s every comparison prints its largest err / (2^-24 S) next to its bar."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import param_kernels_ref as R

pytestmark = pytest.mark.gpu

CH = R.C
OK, E_NULL, E_RANGE, E_UNSUPPORTED = 0, -1, -2, -3
SENT = -777.25                                                    # behind every buffer; must survive every call
MARK = 12345.5                                                    # in tensors a call must not write
GUARD = 64
NAN = float('nan')
LAYS = ['L1', 'L2', 'L3', 'L4', 'L5']
WIDE = pytest.mark.parametrize('wide', [False, True], ids=['randn', 'wide'])


def _lib():
    from kgwas_amd import _lib
    return _lib


def _L():
    return _lib().lib()


def _st():
    return _lib().stream_ptr()


def _p(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _rand(g, shape, wide):
    x = torch.randn(shape, device='cuda', generator=g)
    if wide:
        x = x * torch.exp2(torch.randint(-4, 5, shape, device='cuda', generator=g).float())
    return x


class Arena:
    """Buffers with the sentinel behind them; inputs with a copy to compare with afterwards."""

    def __init__(self):
        self.flats, self.inputs = [], []

    def out(self, *shape, fill=NAN):
        n = int(np.prod(shape)) if shape else 1
        flat = torch.full((n + GUARD,), SENT, device='cuda')
        flat[:n] = fill
        self.flats.append((flat, n))
        return flat[:n].view(*shape)

    def inp(self, t):
        v = self.out(*t.shape, fill=0.0)
        v.copy_(t)
        self.inputs.append((v, v.clone()))
        return v

    def ints(self, values):
        t = torch.tensor(list(values), dtype=torch.int32, device='cuda')
        self.inputs.append((t, t.clone()))
        return t

    def check(self):
        torch.cuda.synchronize()
        for flat, n in self.flats:
            assert bool((flat[n:] == SENT).all()), 'a call wrote behind a buffer'
        for v, keep in self.inputs:
            assert torch.equal(v, keep), 'a call wrote into an input'


def _same(a, b):
    """Bit-identity, NaN included."""
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _untouched(t, fill):
    return bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())


_WORST = {}


def _bar(tag, name, got, ref, scale, n_terms):
    e = R.err_in_u(got, ref, scale)
    _WORST[name] = max(_WORST.get(name, 0.0), e)
    print(f'[param {tag}] {name}: err / (2^-24 S) = {e:.3f} of a bound of {n_terms + 2}  (largest so far {_WORST[name]:.3f})')
    assert e <= n_terms + 2, (tag, name, e, n_terms + 2)


# ====================================================== problems ===========================================================

class Rel:
    """One layer's packed relation parameters on the device, its index arrays, and gradients arriving from above as the eight
    pieces per value the aggregate's riders leave + their sums in k_duv_fold's order."""

    def __init__(self, name, seed, wide):
        lay = self.lay = R.LAYOUTS[name]
        A = self.A = Arena()
        g = _gen(1000 * seed + 7 * lay.n + (1 if wide else 0))
        self.w_src_t = A.inp(_rand(g, (lay.n, CH, CH), wide))
        self.w_dst_t = A.inp(_rand(g, (lay.n_bip, CH, CH), wide)) if lay.n_bip else None
        self.att_src, self.att_dst = A.inp(_rand(g, (lay.n, CH), wide)), A.inp(_rand(g, (lay.n, CH), wide))
        self.bias = A.inp(_rand(g, (lay.n, CH), wide))
        self.live_of_rel, self.rel_ids, self.bip_pos = A.ints(lay.live_of_rel), A.ints(lay.rel_ids), A.ints(lay.bip_pos)
        self.ids = torch.tensor(lay.rel_ids, dtype=torch.long, device='cuda')
        p = self.pieces = A.inp(_rand(g, (2, lay.n_rels, 8, CH), wide))          # dU_full / dV by relation id, dead rows alive too
        s = ((p[:, :, 0] + p[:, :, 1]) + (p[:, :, 2] + p[:, :, 3])) + ((p[:, :, 4] + p[:, :, 5]) + (p[:, :, 6] + p[:, :, 7]))
        self.dU, self.dV = A.inp(s[0]), A.inp(s[1])
        self.pieces_slot, self.dV_slot = A.inp(p[1][self.ids]), A.inp(s[1][self.ids])          # dV by packed slot (v_by_rel = 0)
        self.acc = A.inp(_rand(g, (lay.n, CH, CH), wide))
        self.blk = {}

    def host(self):
        wd = self.w_dst_t if self.w_dst_t is not None else torch.zeros(0, CH, CH)
        return self.w_src_t, wd, self.att_src, self.att_dst

    def blk_of_live(self, n_blk):
        if n_blk not in self.blk:
            rs = np.random.RandomState(17 + n_blk + self.lay.n)
            v = rs.randint(-1, max(n_blk, 1), size=self.lay.n).tolist()
            self.blk[n_blk] = (v, self.A.ints(v))
        return self.blk[n_blk]

    @functools.lru_cache(maxsize=None)
    def fwd_ref(self):
        return R.relvec_fwd_ref(self.lay, *self.host())


@functools.lru_cache(maxsize=None)
def _rel(name, seed, wide):
    return Rel(name, seed, wide)


# ====================================================== A. kgw_relvec_fwd ====================================================

def _fwd_outs(A, rel, n_blk, zero_floats):
    lay = rel.lay
    o = dict(U=A.out(lay.n_rels, CH), V=A.out(lay.n_rels, CH), Vs=A.out(lay.n, CH),
             bsum=A.out(max(n_blk, 1), CH, fill=NAN if n_blk else MARK))
    o['zero'] = None if zero_floats is None else A.out(max(zero_floats, 4), fill=NAN if zero_floats else MARK)
    return o


def _fwd_job(j, rel, o, n_blk, zero_floats):
    lay = rel.lay
    j.n_rels_total, j.n_live, j.n_blk = lay.n_rels, lay.n, n_blk
    j.live_of_rel, j.rel_ids, j.bip_pos = rel.live_of_rel.data_ptr(), rel.rel_ids.data_ptr(), rel.bip_pos.data_ptr()
    j.w_src_t, j.w_dst_t = rel.w_src_t.data_ptr(), (None if rel.w_dst_t is None else rel.w_dst_t.data_ptr())
    j.att_src, j.att_dst = rel.att_src.data_ptr(), rel.att_dst.data_ptr()
    j.U_full, j.V = o['U'].data_ptr(), o['V'].data_ptr()
    j.bias, j.blk_of_live, j.bias_sum = rel.bias.data_ptr(), rel.blk_of_live(n_blk)[1].data_ptr(), o['bsum'].data_ptr()
    if zero_floats is not None:
        j.zero_buf, j.zero_floats = o['zero'].data_ptr(), zero_floats


def _fwd_single(rel, n_blk, zero_floats, v_by_rel):
    A, lay = Arena(), rel.lay
    o = _fwd_outs(A, rel, n_blk, zero_floats)
    V = o['V'] if v_by_rel else o['Vs']
    rc = _L().kgw_relvec_fwd(lay.n_rels, _p(rel.live_of_rel), _p(rel.bip_pos), _p(rel.w_src_t), _p(rel.w_dst_t), _p(rel.att_src),
                             _p(rel.att_dst), _p(o['U']), _p(V), v_by_rel, lay.n, _p(rel.bias), _p(rel.blk_of_live(n_blk)[1]), n_blk,
                             _p(o['bsum']), _p(o['zero']), zero_floats or 0, _st())
    assert rc == OK, rc
    A.check()
    rel.A.check()
    return o


def _fwd_multi(cfgs):
    """cfgs: [(rel, n_blk, zero_floats) or None (a job with n_rels_total = 0: skipped, its buffers untouched)]."""
    A = Arena()
    jobs = (_lib().KgwRelvecJob * len(cfgs))()
    outs = []
    for q, cfg in enumerate(cfgs):
        if cfg is None:
            rel = _rel('L2', 9, False)
            o = {k: A.out(*v.shape, fill=MARK) for k, v in _fwd_outs(Arena(), rel, 3, 64).items()}
            _fwd_job(jobs[q], rel, o, 3, 64)
            jobs[q].n_rels_total = 0
            o['empty'] = True
        else:
            o = _fwd_outs(A, *cfg)
            _fwd_job(jobs[q], cfg[0], o, cfg[1], cfg[2])
        outs.append(o)
    rc = _L().kgw_relvec_fwd_multi(len(cfgs), jobs, _st())
    assert rc == OK, rc
    A.check()
    for cfg in cfgs:
        if cfg is not None:
            cfg[0].A.check()
    return outs


def _check_fwd(tag, rel, o, n_blk, zero_floats, v_by_rel):
    lay = rel.lay
    (Uf, Vr, Vs), (sU, sVr, sVs) = rel.fwd_ref()
    _bar(tag, 'U', o['U'], Uf, sU, R.N_TERMS['U'])
    if v_by_rel:
        _bar(tag, 'V', o['V'], Vr, sVr, R.N_TERMS['V'])
        assert _untouched(o['Vs'], NAN)
    else:
        _bar(tag, 'V', o['Vs'], Vs, sVs, R.N_TERMS['V'])
        assert _untouched(o['V'], NAN)
    if n_blk:
        ref, s = R.bias_sums(rel.bias, rel.blk_of_live(n_blk)[0], n_blk)
        _bar(tag, 'bias_sum', o['bsum'], ref, s, lay.n)
    else:
        assert _untouched(o['bsum'], MARK)
    if zero_floats:
        z = o['zero']
        assert z.numel() == zero_floats and bool((z.view(torch.int32) == 0).all()), 'exactly zero_floats floats cleared (+0.0)'
    elif zero_floats == 0:
        assert _untouched(o['zero'], MARK)


# (layout, n_blk, zero_floats): n_blk over {0, 1, 3, 8}; zero_floats over none / 0 with a buffer / one float4 / the edges of one
# zero-fill block of 1 024 threads x 4 float4
FWD_CASES = [('L1', 0, None), ('L2', 3, 4), ('L3', 8, 16380), ('L4', 1, 16384), ('L5', 3, 16388), ('L2', 8, 0), ('L4', 0, 4)]


@WIDE
@pytest.mark.parametrize('v_by_rel', [0, 1])
@pytest.mark.parametrize('name,n_blk,zf', FWD_CASES, ids=[f'{a}-blk{b}-z{c}' for a, b, c in FWD_CASES])
def test_relvec_fwd_matches_float64(name, n_blk, zf, v_by_rel, wide):
    rel = _rel(name, 1, wide)
    o = _fwd_single(rel, n_blk, zf, v_by_rel)
    _check_fwd(f'relvec_fwd {name} v_by_rel={v_by_rel}', rel, o, n_blk, zf, v_by_rel)
    o2 = _fwd_single(rel, n_blk, zf, v_by_rel)                    # two runs of the same call
    assert all(o[k] is None or _same(o[k], o2[k]) for k in o)
    if v_by_rel == 0:                                            # v_by_rel 0 against 1 on the live rows
        o1 = _fwd_single(rel, n_blk, zf, 1)
        assert _same(o['Vs'], o1['V'][rel.ids]) and _same(o['U'], o1['U']) and _same(o['bsum'], o1['bsum'])


def test_relvec_fwd_zero_fill_past_the_block_cap():
    """4 (1 024 * 4 096 + 1) floats: one float4 more than 1 024 zero-fill blocks clear in one pass (the grid-stride loop's second
    round); the guard float behind them stays."""
    rel = _rel('L1', 1, False)
    zf = 4 * (1024 * 4096 + 1)
    for mode in (0, 1):
        o = _fwd_single(rel, 1, zf, 1) if mode == 0 else _fwd_multi([(rel, 1, zf)])[0]
        _check_fwd('relvec_fwd zero fill past the cap', rel, o, 1, zf, 1)
        del o


MULTI = {1: [('L3', 8, 16380)],
         2: [('L1', 0, None), ('L2', 3, 4)],
         3: [('L4', 1, 16384), None, ('L5', 3, 16388)],
         4: [('L3', 8, 16380), ('L2', 8, 0), None, ('L1', 1, 4)]}


@WIDE
@pytest.mark.parametrize('n_jobs', [1, 2, 3, 4])
def test_relvec_fwd_multi_matches_float64_and_the_single_calls(n_jobs, wide):
    cfgs = [None if c is None else (_rel(c[0], 2 + q, wide), c[1], c[2]) for q, c in enumerate(MULTI[n_jobs])]
    outs = _fwd_multi(cfgs)
    again = _fwd_multi(cfgs)
    for q, (cfg, o, o2) in enumerate(zip(cfgs, outs, again)):
        if cfg is None:
            assert all(_untouched(v, MARK) for k, v in o.items() if k != 'empty'), 'a skipped job keeps its buffers'
            continue
        rel, n_blk, zf = cfg
        _check_fwd(f'relvec_fwd_multi {n_jobs} jobs, job {q} {rel.lay}', rel, o, n_blk, zf, 1)
        s = _fwd_single(rel, n_blk, zf, 1)
        for k in ('U', 'V', 'bsum', 'zero'):
            assert o[k] is None or (_same(o[k], s[k]) and _same(o[k], o2[k])), (q, k)


# ====================================================== B. kgw_relvec_bwd ====================================================

def _bwd_outs(A, rel):
    lay = rel.lay
    return dict(dws=A.out(lay.n, CH, CH), dwd=A.out(lay.n_bip, CH, CH) if lay.n_bip else None, das=A.out(lay.n, CH), dad=A.out(lay.n, CH))


def _bwd_job(j, rel, o, dU, dV, acc, pieces):
    lay = rel.lay
    j.n_rels_total, j.n_live, j.duv_pieces = lay.n_rels, lay.n, 1 if pieces else 0
    j.live_of_rel, j.rel_ids, j.bip_pos = rel.live_of_rel.data_ptr(), rel.rel_ids.data_ptr(), rel.bip_pos.data_ptr()
    j.w_src_t, j.w_dst_t = rel.w_src_t.data_ptr(), (None if rel.w_dst_t is None else rel.w_dst_t.data_ptr())
    j.att_src, j.att_dst = rel.att_src.data_ptr(), rel.att_dst.data_ptr()
    j.dU_full, j.dV = (None if dU is None else dU.data_ptr()), (None if dV is None else dV.data_ptr())
    j.dw_src_acc = None if acc is None else acc.data_ptr()
    j.dw_src_t, j.dw_dst_t = o['dws'].data_ptr(), (None if o['dwd'] is None else o['dwd'].data_ptr())
    j.datt_src, j.datt_dst = o['das'].data_ptr(), o['dad'].data_ptr()


def _bwd_single(rel, use_dU, use_dV, use_acc, v_by_rel):
    A = Arena()
    o = _bwd_outs(A, rel)
    dV = rel.dV if v_by_rel else rel.dV_slot
    rc = _L().kgw_relvec_bwd_acc(rel.lay.n, _p(rel.rel_ids), _p(rel.bip_pos), _p(rel.w_src_t), _p(rel.w_dst_t), _p(rel.att_src),
                                 _p(rel.att_dst), _p(rel.dU if use_dU else None), _p(dV if use_dV else None),
                                 _p(rel.acc if use_acc else None), _p(o['dws']), _p(o['dwd']), _p(o['das']), _p(o['dad']), v_by_rel, _st())
    assert rc == OK, rc
    A.check()
    rel.A.check()
    return o


def _bwd_multi(cfgs, pieces):
    """cfgs: [(rel, use_dU, use_dV, use_acc) or None (n_live = 0: skipped)]; v_by_rel = 1."""
    A = Arena()
    jobs = (_lib().KgwRelvecJob * len(cfgs))()
    outs = []
    for q, cfg in enumerate(cfgs):
        if cfg is None:
            rel = _rel('L2', 9, False)
            o = {k: A.out(*v.shape, fill=MARK) for k, v in _bwd_outs(Arena(), rel).items() if v is not None}
            _bwd_job(jobs[q], rel, o, rel.dU, rel.dV, rel.acc, False)
            jobs[q].n_live = 0
        else:
            rel, use_dU, use_dV, use_acc = cfg
            o = _bwd_outs(A, rel)
            dU, dV = (rel.pieces[0], rel.pieces[1]) if pieces else (rel.dU, rel.dV)
            _bwd_job(jobs[q], rel, o, dU if use_dU else None, dV if use_dV else None, rel.acc if use_acc else None, pieces)
        outs.append(o)
    rc = _L().kgw_relvec_bwd_multi(len(cfgs), jobs, _st())
    assert rc == OK, rc
    A.check()
    for cfg in cfgs:
        if cfg is not None:
            cfg[0].A.check()
    return outs


def _check_bwd(tag, rel, o, dU, dV, acc):
    """dU, dV by relation id (None: zero) and acc as the kernel was given them (fp32 tensors)."""
    g, s = R.relvec_bwd_ref(rel.lay, *rel.host(), dU, dV, 1, acc)
    _bar(tag, 'dw_src_t', o['dws'], g[0], s[0], R.N_TERMS['dw_src_t'])
    if o['dwd'] is not None:
        _bar(tag, 'dw_dst_t', o['dwd'], g[1], s[1], R.N_TERMS['dw_dst_t'])
    _bar(tag, 'datt_src', o['das'], g[2], s[2], R.N_TERMS['datt_src'])
    _bar(tag, 'datt_dst', o['dad'], g[3], s[3], R.N_TERMS['datt_dst'])


NULLS = [(True, True), (False, True), (True, False)]            # both given / dU_full null / dV null


@WIDE
@pytest.mark.parametrize('name', LAYS)
def test_relvec_bwd_acc_matches_float64(name, wide):
    rel = _rel(name, 3, wide)
    for use_dU, use_dV in NULLS:
        for use_acc in (False, True):
            o1 = _bwd_single(rel, use_dU, use_dV, use_acc, 1)
            tag = f'relvec_bwd_acc {name} dU={int(use_dU)} dV={int(use_dV)} acc={int(use_acc)}'
            _check_bwd(tag, rel, o1, rel.dU if use_dU else None, rel.dV if use_dV else None, rel.acc if use_acc else None)
            o0 = _bwd_single(rel, use_dU, use_dV, use_acc, 0)   # v_by_rel 0: the same values from dV by slot
            assert all(o1[k] is None or _same(o1[k], o0[k]) for k in o1), tag
    again = _bwd_single(rel, use_dU, use_dV, use_acc, 1)          # two runs of the same call
    assert all(o1[k] is None or _same(o1[k], again[k]) for k in o1)


BWD_MULTI = {1: [('L3', True, True, True)],
             2: [('L1', True, True, False), ('L2', False, True, True)],
             3: [('L4', True, False, True), None, ('L5', True, True, True)],
             4: [('L3', True, True, False), ('L2', True, False, False), None, ('L1', False, True, True)]}


@WIDE
@pytest.mark.parametrize('n_jobs', [1, 2, 3, 4])
def test_relvec_bwd_multi_matches_float64_pieces_and_the_single_calls(n_jobs, wide):
    cfgs = [None if c is None else (_rel(c[0], 4 + q, wide),) + c[1:] for q, c in enumerate(BWD_MULTI[n_jobs])]
    whole, parts, again = _bwd_multi(cfgs, False), _bwd_multi(cfgs, True), _bwd_multi(cfgs, True)
    for q, cfg in enumerate(cfgs):
        if cfg is None:
            assert all(_untouched(v, MARK) for v in whole[q].values()) and all(_untouched(v, MARK) for v in parts[q].values())
            continue
        rel, use_dU, use_dV, use_acc = cfg
        tag = f'relvec_bwd_multi {n_jobs} jobs, job {q} {rel.lay}'
        _check_bwd(tag, rel, whole[q], rel.dU if use_dU else None, rel.dV if use_dV else None, rel.acc if use_acc else None)
        one = _bwd_multi([cfg], True)[0]                          # a k-job call against k calls
        single = _bwd_single(rel, use_dU, use_dV, use_acc, 1)
        for k, v in whole[q].items():
            if v is not None:
                assert _same(v, parts[q][k]), (tag, k, 'pieces against complete')
                assert _same(v, one[k]) and _same(v, single[k]), (tag, k, 'multi against single')
                assert _same(parts[q][k], again[q][k]), (tag, k, 'two runs')


# ====================================================== C. kgw_fold_fwd / kgw_fold_bwd =======================================

class Fold:
    """The FC_output fold over a layer's relations: FC_output.weight / .bias of n_mlp MLPs, U, V by relation id (given: any
    values), and the gradients of U', V', kappa, W', gamma arriving from above (dU', dV' = rel.pieces / rel.dU, rel.dV)."""

    def __init__(self, rel, seed, wide):
        lay = self.lay = rel.lay
        self.rel = rel
        A = self.A = Arena()
        g = _gen(5000 + seed + (1 if wide else 0))
        self.fcw = [A.inp(_rand(g, (CH, CH), wide)) for _ in range(lay.n_mlp)]
        self.fcb = [A.inp(_rand(g, (CH,), wide)) for _ in range(lay.n_mlp)]
        self.U, self.V = A.inp(_rand(g, (lay.n_rels, CH), wide)), A.inp(_rand(g, (lay.n_rels, CH), wide))
        self.dkappa, self.dWp, self.dgamma = A.inp(_rand(g, (lay.n_rels,), wide)), A.inp(_rand(g, (lay.n, CH, CH), wide)), A.inp(_rand(g, (lay.n, CH), wide))
        self.h_ids, self.h_sm, self.h_dm = (np.asarray(x, dtype=np.int32) for x in (lay.rel_ids, lay.src_m, lay.dst_m))

    def args(self, U=None, V=None):
        lay = self.lay
        a = _lib().KgwFoldArgs()
        a.n, a.n_rels, a.n_mlp = lay.n, lay.n_rels, lay.n_mlp
        a.rel_ids_host, a.src_mlp_host, a.dst_mlp_host = self.h_ids.ctypes.data, self.h_sm.ctypes.data, self.h_dm.ctypes.data
        a.w_src_t = self.rel.w_src_t.data_ptr()
        a.U, a.V = (self.U if U is None else U).data_ptr(), (self.V if V is None else V).data_ptr()
        for m in range(lay.n_mlp):
            a.fc_weight[m], a.fc_bias[m] = self.fcw[m].data_ptr(), self.fcb[m].data_ptr()
        return a

    def host(self, U=None, V=None):
        return self.rel.w_src_t, (self.U if U is None else U), (self.V if V is None else V), torch.stack(self.fcw), torch.stack(self.fcb)

    def set_fwd(self, a, o):
        a.Up, a.Vp, a.kappa, a.Wp, a.gamma = (o[k].data_ptr() for k in ('Up', 'Vp', 'kappa', 'Wp', 'gamma'))

    def set_bwd(self, a, o, pieces):
        rel = self.rel
        a.dUp, a.dVp = (rel.pieces[0].data_ptr(), rel.pieces[1].data_ptr()) if pieces else (rel.dU.data_ptr(), rel.dV.data_ptr())
        a.duv_pieces = 1 if pieces else 0
        a.dkappa, a.dWp, a.dgamma = self.dkappa.data_ptr(), self.dWp.data_ptr(), self.dgamma.data_ptr()
        a.dU, a.dV, a.dws = o['dU'].data_ptr(), o['dV'].data_ptr(), o['dws'].data_ptr()
        for m in range(self.lay.n_mlp):
            a.d_fc_weight[m], a.d_fc_bias[m] = o['dfcw'][m].data_ptr(), o['dfcb'][m].data_ptr()

    def fwd_outs(self, A, fill=NAN):
        lay = self.lay
        return dict(Up=A.out(lay.n_rels, CH, fill=fill), Vp=A.out(lay.n_rels, CH, fill=fill), kappa=A.out(lay.n_rels, fill=fill),
                    Wp=A.out(lay.n, CH, CH, fill=fill), gamma=A.out(lay.n, CH, fill=fill))

    def bwd_outs(self, A, fill=NAN, fill_uv=None):
        lay = self.lay
        f2 = fill if fill_uv is None else fill_uv
        return dict(dU=A.out(lay.n_rels, CH, fill=f2), dV=A.out(lay.n_rels, CH, fill=f2), dws=A.out(lay.n, CH, CH, fill=f2),
                    dfcw=[A.out(CH, CH, fill=fill) for _ in range(lay.n_mlp)], dfcb=[A.out(CH, fill=fill) for _ in range(lay.n_mlp)])

    def check(self):
        self.A.check()
        self.rel.A.check()


@functools.lru_cache(maxsize=None)
def _fold(name, seed, wide):
    return Fold(_rel(name, seed, wide), seed, wide)


def _fold_fwd(F, U=None, V=None):
    A = Arena()
    o = F.fwd_outs(A)
    a = F.args(U, V)
    F.set_fwd(a, o)
    rc = _L().kgw_fold_fwd(C.byref(a), _st())
    assert rc == OK, rc
    A.check()
    F.check()
    return o


def _fold_bwd(F, pieces):
    A = Arena()
    o = F.bwd_outs(A)
    a = F.args()
    F.set_bwd(a, o, pieces)
    rc = _L().kgw_fold_bwd(C.byref(a), _st())
    assert rc == OK, rc
    A.check()
    F.check()
    return o


def _check_fold_fwd(tag, F, o, U=None, V=None):
    ref, s = R.fold_fwd_ref(F.lay, *F.host(U, V))
    for k, name in enumerate(('Up', 'Vp', 'kappa', 'Wp', 'gamma')):
        _bar(tag, name, o[name], ref[k], s[k], R.N_TERMS[name])
    for r in F.lay.dead:
        assert float(o['Up'][r].abs().max()) == 0.0 and float(o['Vp'][r].abs().max()) == 0.0 and float(o['kappa'][r]) == 0.0


def _check_fold_bwd(tag, F, o):
    lay, rel = F.lay, F.rel
    (dws, dU, dV, dfcw, dfcb), (s_ws, s_U, s_V, s_fw, s_fb) = R.fold_bwd_ref(lay, *F.host(), rel.dU, rel.dV, F.dkappa, F.dWp, F.dgamma)
    _bar(tag, 'fold_dws', o['dws'], dws, s_ws, R.N_TERMS['fold_dws'])
    _bar(tag, 'fold_dU', o['dU'], dU, s_U, R.N_TERMS['fold_dU'])
    _bar(tag, 'fold_dV', o['dV'], dV, s_V, R.N_TERMS['fold_dV'])
    for m in range(lay.n_mlp):
        _bar(tag, 'd_fc_weight', o['dfcw'][m], dfcw[m], s_fw[m], R.n_terms_fc(lay, m))
        _bar(tag, 'd_fc_bias', o['dfcb'][m], dfcb[m], s_fb[m], R.n_terms_fc(lay, m))
        if lay.n_src(m) + lay.n_dst(m) == 0:
            assert float(o['dfcw'][m].abs().max()) == 0.0 and float(o['dfcb'][m].abs().max()) == 0.0


def _same_tree(a, b):
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            if x is not None and not _same(x, y):
                return False
    return True


@WIDE
@pytest.mark.parametrize('name', LAYS)
def test_fold_fwd_and_bwd_match_float64(name, wide):
    F = _fold(name, 6, wide)
    o = _fold_fwd(F)
    _check_fold_fwd(f'fold_fwd {name}', F, o)
    assert _same_tree(o, _fold_fwd(F)), 'two runs'
    b = _fold_bwd(F, False)
    _check_fold_bwd(f'fold_bwd {name}', F, b)
    parts = _fold_bwd(F, True)
    assert _same_tree(b, parts), 'pieces against complete'
    assert _same_tree(parts, _fold_bwd(F, True)), 'two runs'


# ====================================================== D. kgw_gemm3_riders ==================================================

def _g3_product(seed):
    M, K = 256, 32
    g = _gen(seed)
    Am, Bm = torch.randn(M, K, device='cuda', generator=g), torch.randn(K, CH, device='cuda', generator=g)
    packed = torch.zeros(int(_L().kgw_gemm3_packed_bytes(K)), dtype=torch.uint8, device='cuda')
    assert _L().kgw_gemm3_pack(_p(Bm), CH, K, K, 1, _p(packed), _st()) == OK
    return M, K, Am, packed


def _g3_call(prod, A, riders=None, expect=OK):
    """kgw_gemm3 (riders None) or kgw_gemm3_riders(riders = (jobs, n, fold args or None, fold_job))."""
    M, K, Am, packed = prod
    nws = int(_L().kgw_gemm3_workspace_floats(M, K))
    fill = NAN if expect == OK else MARK
    ws, out = A.out(nws, fill=fill), A.out(M, CH, fill=fill)
    head = (_p(Am), K, M, K, _p(packed), _p(ws), nws, None, 0, _p(out), CH, 0, None, None, 0, 0, None)
    if riders is None:
        rc = _L().kgw_gemm3(*head, _st())
    else:
        jobs, n, fa, fj = riders
        rc = _L().kgw_gemm3_riders(*head, n, C.cast(jobs, C.c_void_p), None if fa is None else C.cast(C.pointer(fa), C.c_void_p), fj, _st())
    assert rc == expect, rc
    return out


def _riders_against_standalone(cfgs, fold_of, wide):
    """cfgs: [(rel, n_blk, zero_floats)]; fold_of: (job index, Fold) or None."""
    prod = _g3_product(31)
    runs = []
    for riders in (True, False):
        A = Arena()
        jobs = (_lib().KgwRelvecJob * len(cfgs))()
        outs = [_fwd_outs(A, *cfg) for cfg in cfgs]
        for q, cfg in enumerate(cfgs):
            _fwd_job(jobs[q], cfg[0], outs[q], cfg[1], cfg[2])
        fa, fo, fj = None, None, 0
        if fold_of is not None:
            fj, F = fold_of
            fo = F.fwd_outs(A)
            fa = F.args(outs[fj]['U'], outs[fj]['V'])           # the fold reads u_r / v_r where the relation task leaves them
            F.set_fwd(fa, fo)
        if riders:
            y = _g3_call(prod, A, (jobs, len(cfgs), fa, fj))
        else:
            y = _g3_call(prod, A)
            assert _L().kgw_relvec_fwd_multi(len(cfgs), jobs, _st()) == OK
            assert fa is None or _L().kgw_fold_fwd(C.byref(fa), _st()) == OK
        A.check()
        runs.append((y, outs, fo))
    (ya, oa, fa_), (yb, ob, fb_) = runs
    assert _same(ya, yb) and not bool(torch.isnan(ya).any()), 'the product itself is what kgw_gemm3 computes'
    for q, cfg in enumerate(cfgs):
        for k in ('U', 'V', 'bsum', 'zero'):
            assert oa[q][k] is None or _same(oa[q][k], ob[q][k]), (q, k)
        _check_fwd(f'riders job {q} {cfg[0].lay}', cfg[0], oa[q], cfg[1], cfg[2], 1)
    if fold_of is not None:
        assert _same_tree(fa_, fb_), 'fold vectors and tiles'
        fj, F = fold_of
        _check_fold_fwd(f'riders fold {F.lay}', F, fa_, oa[fj]['U'], oa[fj]['V'])


@WIDE
def test_riders_with_fewer_tasks_than_rider_wavefronts(wide):
    assert int(_L().kgw_gemm3_rider_blocks(256, 32)) > 0, 'the smallest product with rider blocks'
    F = _fold('L1', 6, wide)
    _riders_against_standalone([(F.rel, 1, 4)], (0, F), wide)    # 1 relation + 1 bias + 16 tiles


@WIDE
def test_riders_with_many_times_as_many_tasks(wide):
    """Four layers of 64 relations, the fold of L3 on job 1: 256 + 4 + 1 024 tasks for at most 128 rider wavefronts."""
    F = _fold('L3', 6, wide)
    cfgs = [(_rel('L3', 11, wide), 8, 16380), (F.rel, 3, 16388), (_rel('L3', 12, wide), 0, None), (_rel('L3', 13, wide), 1, 4)]
    _riders_against_standalone(cfgs, (1, F), wide)


# ====================================================== E. kgw_param_tail ====================================================

class Product:
    """C[M, N] = A[:rows]^T B[:rows] (+ column sums of A) as a deferred weight-gradient product."""

    def __init__(self, seed, rows, M, N, colsum, c_t, rows_dev, wide):
        self.rows, self.M, self.N, self.colsum, self.c_t = rows, M, N, colsum, c_t
        self.Ar = Arena()
        g = _gen(7000 + seed)
        self.A, self.B = self.Ar.inp(_rand(g, (rows, M), wide)), self.Ar.inp(_rand(g, (rows, N), wide))
        self.rd = None if rows_dev is None else (rows - 1 if rows_dev == 'rows-1' else 0)
        self.rows_dev = None if self.rd is None else self.Ar.ints([self.rd])
        # (twice the documented size: room for every block index a permuted tile map could produce, so that a wrong map gives
        #  wrong numbers, not a write outside the workspace)
        self.nws = 2 * int(_L().kgw_tn_gemm_workspace_floats(rows, M, N)) + 65536

    def job(self, j, A):
        o = dict(C=A.out(*((self.N, self.M) if self.c_t else (self.M, self.N))), cs=A.out(self.M) if self.colsum else None,
                 ws=A.out(self.nws), fin=A.out(self.M * self.N), fin_cs=A.out(self.M) if self.colsum else None)
        j.A, j.lda, j.B, j.ldb, j.rows = self.A.data_ptr(), self.M, self.B.data_ptr(), self.N, self.rows
        j.C, j.ldc = o['C'].data_ptr(), (self.M if self.c_t else self.N)
        j.colsum_a, j.colsum_ld, j.colsum_repeat = (o['cs'].data_ptr() if self.colsum else None), self.M, 1
        j.workspace, j.workspace_floats = o['ws'].data_ptr(), self.nws
        j.rows_dev = None if self.rows_dev is None else self.rows_dev.data_ptr()
        j.M, j.N, j.c_transposed = self.M, self.N, 1 if self.c_t else 0
        return o

    def check(self, tag, o):
        n = self.rows if self.rd is None else self.rd
        a, b = self.A[:n].double().cpu(), self.B[:n].double().cpu()
        ref, s = a.t() @ b, a.abs().t() @ b.abs()
        got = o['C'].t() if self.c_t else o['C']
        e = R.err_in_u(got, ref, s)
        print(f'[param {tag}] product {self.rows} x {self.M} x {self.N} rows_dev={self.rd}: err / (2^-24 sum |a||b|) = {e:.3f} of 16')
        assert e <= 16, (tag, e)
        if self.colsum:
            _bar(tag, 'colsum', o['cs'], a.sum(0), a.abs().sum(0), max(n, 1))


def _finish(outs, src):
    """kgw_grad_finish over [C, colsum] of every product: the finished gradient into `fin` and into the tensor itself."""
    D, G, N, idx = [], [], [], []
    for q, o in enumerate(outs):
        D.append(o['fin']); G.append(o['C']); idx.append(2 * q)
        if o['cs'] is not None:
            D.append(o['fin_cs']); G.append(o['cs']); idx.append(2 * q + 1)
    n = len(D)
    if n == 0:
        return
    Dp, Gp, Np = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int64 * n)()
    S = (_lib().KgwGradSrc * n)()
    for k in range(n):
        Dp[k], Gp[k], Np[k] = D[k].data_ptr(), G[k].data_ptr(), G[k].numel()
        C.memmove(C.byref(S[k]), C.byref(src[idx[k]]), C.sizeof(_lib().KgwGradSrc))
    rc = _L().kgw_grad_finish(n, Dp, Gp, Np, S, _st())
    assert rc == OK, rc


PRODUCTS4 = [(1, 128, 128, True, 0, None), (256, 128, 20, False, 1, 'rows-1'), (257, 128, 128, True, 1, 0), (1000, 256, 128, True, 0, None)]
# (fold layout, layouts of the relvec jobs, fold_job, products)
TAIL = {
    'fold-L2+2jobs': ('L2', ['L2', 'L4'], 0, []),
    'fold-L3+4jobs+4products': ('L3', ['L5', 'L2', 'L1', 'L3'], 3, PRODUCTS4),
    '1job+1product': (None, ['L4'], -1, [(1000, 256, 128, False, 1, 'rows-1')]),
    '2products': (None, [], -1, [(257, 128, 128, True, 0, 'rows-1'), (256, 128, 20, True, 0, 0)]),
}


def _tail_run(merged, F, rels, fold_job, prods, pieces):
    """The parameter-only end of a backward pass: merged (kgw_param_tail) or as kgw_tn_gemm_multi_partial, kgw_fold_bwd,
    kgw_relvec_bwd_multi one after the other; then kgw_grad_finish.  Returns (product outputs, fold outputs, job outputs)."""
    L, A = _L(), Arena()
    n_tn = len(prods)
    tn = (_lib().KgwTnJob * max(n_tn, 1))()
    src = (_lib().KgwGradSrc * max(2 * n_tn, 1))()
    pouts = [p.job(tn[q], A) for q, p in enumerate(prods)]
    fa = fo = None
    if F is not None:
        # merged: fold->dU / dV / dws are not written (sentinel); the three launches hand them to the fold's job
        fo = F.bwd_outs(A, fill_uv=MARK if merged else None)
        fa = F.args()
        F.set_bwd(fa, fo, pieces)
    jobs = (_lib().KgwRelvecJob * max(len(rels), 1))()
    jouts = []
    for q, rel in enumerate(rels):
        o = _bwd_outs(A, rel)
        if F is not None and q == fold_job:
            if merged:                                           # not read: NaN in all three
                lay = rel.lay
                dU, dV, acc = A.out(lay.n_rels, CH), A.out(lay.n_rels, CH), A.out(lay.n, CH, CH)
            else:
                dU, dV, acc = fo['dU'], fo['dV'], fo['dws']
            _bwd_job(jobs[q], rel, o, dU, dV, acc, False)
        else:
            use_acc = q % 2 == 0
            dU, dV = (rel.pieces[0], rel.pieces[1]) if pieces else (rel.dU, rel.dV)
            _bwd_job(jobs[q], rel, o, dU, dV, rel.acc if use_acc else None, pieces)
        jouts.append(o)
    if merged:
        rc = L.kgw_param_tail(n_tn, C.cast(tn, C.c_void_p), C.cast(src, C.c_void_p), None if fa is None else C.cast(C.pointer(fa), C.c_void_p),
                              len(rels), C.cast(jobs, C.c_void_p), fold_job if F is not None else 0, _st())
        assert rc == OK, rc
    else:
        assert L.kgw_tn_gemm_multi_partial(n_tn, tn, src, _st()) == OK
        assert fa is None or L.kgw_fold_bwd(C.byref(fa), _st()) == OK
        assert L.kgw_relvec_bwd_multi(len(rels), jobs, _st()) == OK
    _finish(pouts, src)
    A.check()
    for rel in rels:
        rel.A.check()
    for p in prods:
        p.Ar.check()
    if F is not None:
        F.check()
    return pouts, fo, jouts


@WIDE
@pytest.mark.parametrize('pieces', [False, True], ids=['complete', 'pieces'])
@pytest.mark.parametrize('case', list(TAIL))
def test_param_tail_is_the_three_launches_and_matches_float64(case, pieces, wide):
    fold_lay, job_lays, fold_job, prod_cfgs = TAIL[case]
    F = _fold(fold_lay, 6, wide) if fold_lay else None
    rels = [F.rel if (F is not None and q == fold_job) else _rel(nm, 20 + q, wide) for q, nm in enumerate(job_lays)]
    prods = [Product(q, *cfg, wide) for q, cfg in enumerate(prod_cfgs)]
    sp, sf, sj = _tail_run(False, F, rels, fold_job, prods, pieces)
    mp, mf, mj = _tail_run(True, F, rels, fold_job, prods, pieces)
    ap, af, aj = _tail_run(True, F, rels, fold_job, prods, pieces)
    tag = f'param_tail {case}'
    # ---- the three launches against float64, kernel by kernel (each on the fp32 values it was given)
    for q, p in enumerate(prods):
        p.check(tag, sp[q])
        assert _same(sp[q]['fin'], sp[q]['C'].reshape(-1)) and (sp[q]['cs'] is None or _same(sp[q]['fin_cs'], sp[q]['cs']))
    if F is not None:
        _check_fold_bwd(tag, F, sf)
    for q, rel in enumerate(rels):
        if F is not None and q == fold_job:
            _check_bwd(f'{tag} job {q} (the fold\'s)', rel, sj[q], sf['dU'], sf['dV'], sf['dws'])
        else:
            _check_bwd(f'{tag} job {q}', rel, sj[q], rel.dU, rel.dV, rel.acc if q % 2 == 0 else None)
    # ---- merged against the three launches, bit for bit; two merged runs
    for q in range(len(prods)):
        for k in ('C', 'cs', 'fin', 'fin_cs'):
            assert sp[q][k] is None or (_same(sp[q][k], mp[q][k]) and _same(mp[q][k], ap[q][k])), (tag, 'product', q, k)
    if F is not None:
        for k in ('dfcw', 'dfcb'):
            for m in range(F.lay.n_mlp):
                assert _same(sf[k][m], mf[k][m]) and _same(mf[k][m], af[k][m]), (tag, k, m)
        for k in ('dU', 'dV', 'dws'):
            assert _untouched(mf[k], MARK), (tag, k, 'the merged launch does not write the fold\'s hand-over tensors')
            assert not bool(torch.isnan(sf[k]).any())
    for q in range(len(rels)):
        for k, v in sj[q].items():
            assert v is None or (_same(v, mj[q][k]) and _same(mj[q][k], aj[q][k])), (tag, 'job', q, k)


# ====================================================== F. return codes ======================================================

def test_refusals_launch_nothing():
    L, lib = _L(), _lib()
    A = Arena()
    rel, F = _rel('L2', 1, False), _fold('L2', 6, False)
    lay = rel.lay

    def fwd_jobs(n, zero_floats=64, zero_off=0):
        jobs = (lib.KgwRelvecJob * n)()
        outs = []
        for q in range(n):
            o = {k: (None if v is None else A.out(*v.shape, fill=MARK)) for k, v in _fwd_outs(Arena(), rel, 3, 64).items()}
            _fwd_job(jobs[q], rel, o, 3, 64)
            jobs[q].zero_buf, jobs[q].zero_floats = o['zero'].data_ptr() + zero_off, zero_floats
            outs.append(o)
        return jobs, outs

    def bwd_jobs(n, n_live=None):
        jobs = (lib.KgwRelvecJob * n)()
        outs = []
        for q in range(n):
            o = {k: (None if v is None else A.out(*v.shape, fill=MARK)) for k, v in _bwd_outs(Arena(), rel).items()}
            _bwd_job(jobs[q], rel, o, rel.dU, rel.dV, None, False)
            if n_live is not None:
                jobs[q].n_live = n_live
            outs.append(o)
        return jobs, outs

    def fold_args(fwd=True, bwd=True, **kw):
        a = F.args()
        if fwd:
            F.set_fwd(a, F.fwd_outs(A, fill=MARK))
        if bwd:
            F.set_bwd(a, F.bwd_outs(A, fill=MARK), False)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    # ---- kgw_relvec_fwd / _multi, kgw_relvec_bwd_multi
    for zf, off, want in ((6, 0, E_UNSUPPORTED), (64, 4, E_UNSUPPORTED), (-4, 0, E_UNSUPPORTED)):
        jobs, _ = fwd_jobs(1, zf, off)
        assert L.kgw_relvec_fwd_multi(1, jobs, _st()) == want
        j = jobs[0]
        assert L.kgw_relvec_fwd(j.n_rels_total, j.live_of_rel, j.bip_pos, j.w_src_t, j.w_dst_t, j.att_src, j.att_dst, j.U_full, j.V, 1,
                                j.n_live, j.bias, j.blk_of_live, j.n_blk, j.bias_sum, j.zero_buf, j.zero_floats, _st()) == want
    jobs, _ = fwd_jobs(5)
    assert L.kgw_relvec_fwd_multi(5, jobs, _st()) == E_RANGE
    jobs, _ = bwd_jobs(5)
    assert L.kgw_relvec_bwd_multi(5, jobs, _st()) == E_RANGE
    # ---- kgw_fold_fwd / kgw_fold_bwd
    bad_ids, bad_m = np.array([29] + lay.rel_ids[1:], dtype=np.int32), np.array([3] + lay.src_m[1:], dtype=np.int32)
    for kw in (dict(n=0), dict(n=65), dict(n_rels=lay.n - 1), dict(n_rels=65), dict(n_mlp=0), dict(n_mlp=5),
               dict(rel_ids_host=bad_ids.ctypes.data), dict(src_mlp_host=bad_m.ctypes.data), dict(dst_mlp_host=bad_m.ctypes.data)):
        a = fold_args(**kw)
        assert L.kgw_fold_fwd(C.byref(a), _st()) == E_RANGE, kw
        assert L.kgw_fold_bwd(C.byref(a), _st()) == E_RANGE, kw
    for k in ('Up', 'Vp', 'kappa', 'Wp', 'gamma'):
        a = fold_args(**{k: None})
        assert L.kgw_fold_fwd(C.byref(a), _st()) == E_NULL, k
    for k in ('dUp', 'dVp', 'dkappa', 'dWp', 'dgamma', 'dU', 'dV', 'dws'):
        a = fold_args(**{k: None})
        assert L.kgw_fold_bwd(C.byref(a), _st()) == E_NULL, k
    a = fold_args()
    a.d_fc_weight[1] = None
    assert L.kgw_fold_bwd(C.byref(a), _st()) == E_NULL
    # ---- kgw_param_tail
    def tail(n_tn, tn, fa, n_rv, jobs, fj):
        src = (lib.KgwGradSrc * 10)()
        return L.kgw_param_tail(n_tn, None if tn is None else C.cast(tn, C.c_void_p), C.cast(src, C.c_void_p),
                                None if fa is None else C.cast(C.pointer(fa), C.c_void_p), n_rv, C.cast(jobs, C.c_void_p), fj, _st())
    jobs, _ = bwd_jobs(2)
    for fj in (-1, 2):
        assert tail(0, None, fold_args(), 2, jobs, fj) == E_RANGE
    jobs, _ = bwd_jobs(2, n_live=lay.n - 1)
    assert tail(0, None, fold_args(), 2, jobs, 0) == E_RANGE, 'relvec[fold_job].n_live != fold->n'
    jobs, _ = bwd_jobs(2)
    jobs[1].n_live = 0
    assert tail(0, None, fold_args(), 2, jobs, 0) == E_UNSUPPORTED, 'an empty job that is not the fold\'s'
    jobs, _ = bwd_jobs(1)
    prod = Product(0, 40, 128, 128, True, 0, None, False)
    tn = (lib.KgwTnJob * 5)()
    pouts = [prod.job(tn[q], A) for q in range(5)]
    for o in pouts:
        for t in o.values():
            if t is not None:
                t.fill_(MARK)
    assert tail(5, tn, None, 1, jobs, 0) == E_RANGE
    tn[0].M = 127
    assert tail(1, tn, None, 1, jobs, 0) == E_UNSUPPORTED
    tn[0].M, tn[0].lda = 126, 127
    assert tail(1, tn, None, 1, jobs, 0) == E_UNSUPPORTED
    # ---- kgw_gemm3_riders
    g3 = _g3_product(5)
    jobs, fouts = fwd_jobs(1)
    fa = fold_args()                                             # its U is not the job's U_full
    _g3_call(g3, A, (jobs, 1, fa, 0), expect=E_UNSUPPORTED)
    fa = fold_args(U=jobs[0].U_full, V=jobs[0].V, n_rels=lay.n_rels + 1)
    _g3_call(g3, A, (jobs, 1, fa, 0), expect=E_RANGE)
    # ---- nothing was launched: every output of every refused call holds its mark, every guard its sentinel
    torch.cuda.synchronize()
    for flat, n in A.flats:
        assert bool((flat[:n] == MARK).all()) and bool((flat[n:] == SENT).all())
    rel.A.check()
    F.check()
