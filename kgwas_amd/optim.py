"""FusedAdam: torch.optim.Adam(lr, betas, eps, weight_decay) semantics (kgwas/kgwas.py:116) in ONE launch over all
parameter tensors (kgw_adam), with the step counter on the device so it can sit inside a captured HIP graph.

Two extensions, off by default (the reference trains at one rate and bounds no step): a learning-rate schedule evaluated INSIDE the
Adam kernels from the device step counter (include/kgwas_hip.h: KgwLrSchedule, kgwlr_at), so that a captured step replays with a
moving rate, and torch.nn.utils.clip_grad_norm_'s coefficient from two launches ahead of Adam (kgw_grad_norm_partial / _fold).

A third, off by default too: WeightAverage, an EMA or SWA shadow of the weights updated by one launch behind the optimiser's
(kgw_weight_avg_update), driven by the same device counter."""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import NamedTuple

import numpy as np
import torch

from . import _lib

_SCHEDULE_KEYS = ('kind', 'warmup_steps', 'min_lr', 'step_size', 'gamma', 'total_steps')


def _steps(name, v, least, what='lr_schedule'):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v != int(v):
        raise ValueError(f'{what}: {name} = {v!r} is not a whole number of steps')
    if int(v) < least or int(v) >= 2 ** 31:
        raise ValueError(f'{what}: {name} = {v!r} must be at least {least} (and fit 31 bits)')
    return int(v)


def parse_lr_schedule(spec, lr, total_steps=None):
    """``spec`` -> _lib.KgwLrSchedule (the rule: include/kgwas_hip.h), or None for None.  ``spec``: a kind ('constant', 'linear',
    'cosine', 'step') or a dict with ``kind`` and any of ``warmup_steps`` (0), ``min_lr`` (0.0: where 'linear' / 'cosine' end;
    the schedule keeps min_lr / lr), ``step_size`` ('step': required), ``gamma`` ('step': 0.1, torch's StepLR default) and
    ``total_steps`` (else the argument: the update at which the decay ends).  Anything else is a ValueError; no device is needed."""
    if spec is None:
        return None
    if isinstance(spec, _lib.KgwLrSchedule):      # (built by an earlier call, or by hand: only checked)
        out = spec
    else:
        if isinstance(spec, str):
            spec = {'kind': spec}
        if not isinstance(spec, dict):
            raise ValueError(f'lr_schedule {spec!r}: None, a kind {sorted(_lib.LR_KINDS)} or a dict with "kind"')
        unknown = sorted(set(spec) - set(_SCHEDULE_KEYS))
        if unknown:
            raise ValueError(f'lr_schedule: unknown key(s) {unknown}; known: {list(_SCHEDULE_KEYS)}')
        d = spec
        if not isinstance(d.get('kind'), str) or d['kind'] not in _lib.LR_KINDS:
            raise ValueError(f'lr_schedule: kind {d.get("kind")!r}; one of {sorted(_lib.LR_KINDS)}')
        kind = _lib.LR_KINDS[d['kind']]
        lr = float(lr)
        if not math.isfinite(lr) or lr < 0:
            raise ValueError(f'lr_schedule: lr = {lr!r} must be finite and >= 0')
        total = d.get('total_steps', total_steps)
        if total is None:
            raise ValueError('lr_schedule: total_steps is needed (the update at which the decay ends)')
        min_lr = d.get('min_lr', 0.0)
        if isinstance(min_lr, bool) or not isinstance(min_lr, numbers.Real) or not math.isfinite(min_lr) or min_lr < 0 or min_lr > lr:
            raise ValueError(f'lr_schedule: min_lr = {min_lr!r} must lie in [0, lr = {lr}]')
        gamma = d.get('gamma', 0.1)
        if isinstance(gamma, bool) or not isinstance(gamma, numbers.Real) or not math.isfinite(gamma) or gamma <= 0:
            raise ValueError(f'lr_schedule: gamma = {gamma!r} must be finite and > 0')
        if kind == _lib.KGW_LR_STEP and d.get('step_size') is None:
            raise ValueError("lr_schedule: kind 'step' needs step_size")
        out = _lib.KgwLrSchedule(kind, _steps('warmup_steps', d.get('warmup_steps', 0), 0), _steps('total_steps', total, 1),
                                 _steps('step_size', d['step_size'], 1) if d.get('step_size') is not None else 1,
                                 float(min_lr) / lr if lr > 0 else 0.0, float(gamma))
    ok = (0 <= out.kind <= 3 and out.warmup_steps >= 0 and out.total_steps >= 1 and (out.kind != _lib.KGW_LR_STEP or out.step_size >= 1)
          and 0.0 <= out.min_ratio <= 1.0 and math.isfinite(out.gamma) and out.gamma > 0)
    if not ok:
        raise ValueError('lr_schedule: a KgwLrSchedule outside the rule\'s ranges (include/kgwas_hip.h: kgwlr_valid)')
    return out


def check_grad_clip_norm(v):
    """``grad_clip_norm`` -> float or None; a ValueError unless it is None or finite and > 0."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v <= 0:
        raise ValueError(f'grad_clip_norm = {v!r} must be finite and > 0')
    return float(v)


_AVERAGE_KEYS = ('kind', 'decay', 'warmup', 'start_step', 'every')


def parse_weight_average(spec, batches_per_epoch=None):
    """``spec`` -> _lib.KgwWeightAvg (the rule: include/kgwas_hip.h), or None for None.  ``spec``: 'ema' | 'swa' | a float (EMA with
    that decay) | a dict with ``kind`` and any of ``decay`` (EMA: 0.999, in (0, 1)), ``warmup`` (EMA: True, the cap
    (1 + k) / (10 + k) on the decay of event k), ``start_step`` (1: the update that is the first event) and ``every`` (1, or 'epoch'
    = ``batches_per_epoch``: updates between events).  Anything else is a ValueError; no device is needed."""
    if spec is None:
        return None
    if isinstance(spec, _lib.KgwWeightAvg):       # (built by an earlier call, or by hand: only checked)
        out = spec
    else:
        if isinstance(spec, str):
            spec = {'kind': spec}
        elif not isinstance(spec, (bool, dict)) and isinstance(spec, numbers.Real):
            spec = {'kind': 'ema', 'decay': spec}
        if not isinstance(spec, dict):
            raise ValueError(f'weight_average {spec!r}: None, a kind {sorted(_lib.AVG_KINDS)}, a decay or a dict with "kind"')
        unknown = sorted(set(spec) - set(_AVERAGE_KEYS))
        if unknown:
            raise ValueError(f'weight_average: unknown key(s) {unknown}; known: {list(_AVERAGE_KEYS)}')
        d = spec
        if not isinstance(d.get('kind'), str) or d['kind'] not in _lib.AVG_KINDS:
            raise ValueError(f'weight_average: kind {d.get("kind")!r}; one of {sorted(_lib.AVG_KINDS)}')
        kind = _lib.AVG_KINDS[d['kind']]
        if kind == _lib.KGW_AVG_SWA and ('decay' in d or 'warmup' in d):
            raise ValueError("weight_average: decay / warmup belong to kind 'ema'; 'swa' weighs its events equally")
        decay = d.get('decay', 0.999)
        if isinstance(decay, bool) or not isinstance(decay, numbers.Real) or not 0.0 < C.c_float(decay).value < 1.0:
            raise ValueError(f'weight_average: decay = {decay!r} must lie in (0, 1) as a float32')
        warmup = d.get('warmup', True)
        if not isinstance(warmup, (bool, np.bool_)):
            raise ValueError(f'weight_average: warmup = {warmup!r} must be True or False')
        every = d.get('every', 1)
        if isinstance(every, str):
            if every != 'epoch':
                raise ValueError(f"weight_average: every = {every!r}; a number of updates or 'epoch'")
            if batches_per_epoch is None:
                raise ValueError("weight_average: every = 'epoch' needs the batches of an epoch")
            every = batches_per_epoch
        out = _lib.KgwWeightAvg(kind, _steps('start_step', d.get('start_step', 1), 1, 'weight_average'),
                                _steps('every', every, 1, 'weight_average'), int(bool(warmup)), float(decay))
    ok = (out.kind in (_lib.KGW_AVG_EMA, _lib.KGW_AVG_SWA) and out.start_step >= 1 and out.every >= 1 and
          (out.kind != _lib.KGW_AVG_EMA or (out.warmup in (0, 1) and 0.0 < out.decay < 1.0)))
    if not ok:
        raise ValueError('weight_average: a KgwWeightAvg outside the rule\'s ranges (include/kgwas_hip.h: kgwavg_valid)')
    return out


LossRule = NamedTuple('LossRule', [('kind', str), ('delta', tuple)])      # what parse_loss returns: immutable, one knee per label column
_LOSS_KEYS = ('kind', 'delta')


def parse_loss(loss, T):
    """``loss`` -> None (the weighted MSE: the default route, untouched) or a LossRule (kind 'huber', ``delta``: a tuple of T knees; the
    rule: include/kgwas_hip.h, KgwReadoutLossArgs).  ``loss``: None | 'mse' | 'huber' (delta 1.0, torch's default) | a float (Huber with
    that delta) | a dict with ``kind`` and, for 'huber', ``delta``: a float > 0 (+inf: the MSE through the Huber kernels) or a
    sequence of T of them, one per label column.  Anything else is a ValueError; no device is needed."""
    T = int(T)
    if T < 1:
        raise ValueError(f'loss: {T} label columns')
    if loss is None:
        return None
    if isinstance(loss, LossRule):                # (built by an earlier call, or by hand: checked below)
        spec = {'kind': loss.kind, 'delta': loss.delta}
    elif isinstance(loss, str):
        spec = {'kind': loss}
    elif not isinstance(loss, (bool, np.bool_, dict)) and isinstance(loss, numbers.Real):
        spec = {'kind': 'huber', 'delta': loss}
    elif isinstance(loss, dict):
        spec = loss
    else:
        raise ValueError(f'loss {loss!r}: None, a kind {sorted(_lib.LOSS_KINDS)}, a delta or a dict with "kind"')
    unknown = sorted(set(spec) - set(_LOSS_KEYS))
    if unknown:
        raise ValueError(f'loss: unknown key(s) {unknown}; known: {list(_LOSS_KEYS)}')
    kind = spec.get('kind')
    if not isinstance(kind, str) or kind not in _lib.LOSS_KINDS:
        raise ValueError(f'loss: kind {kind!r}; one of {sorted(_lib.LOSS_KINDS)}')
    if kind == 'mse':
        if 'delta' in spec:
            raise ValueError("loss: delta belongs to kind 'huber'")
        return None
    delta = spec.get('delta', 1.0)
    if isinstance(delta, (str, bytes, dict)):
        raise ValueError(f'loss: delta = {delta!r} must be a float > 0 or a sequence of {T}')
    if isinstance(delta, numbers.Real):
        delta = [delta] * T
    else:
        try:
            delta = list(delta)
        except TypeError:
            raise ValueError(f'loss: delta = {delta!r} must be a float > 0 or a sequence of {T}') from None
        if len(delta) != T:
            raise ValueError(f'loss: {len(delta)} deltas for {T} label column(s)')
    for d in delta:                               # (NaN fails the comparison; the kernels take the knee as a float32)
        if isinstance(d, (bool, np.bool_)) or not isinstance(d, numbers.Real) or not C.c_float(d).value > 0.0:
            raise ValueError(f'loss: delta = {d!r} must be > 0 as a float32 (+inf: the MSE)')
    return LossRule('huber', tuple(float(C.c_float(d).value) for d in delta))       # (the float32 values the kernels compare against)


class WeightAverage:
    """The averaged copy of a model's weights (EMA or SWA; the rule: include/kgwas_hip.h, KgwWeightAvg): ``avg_model``, a deep copy
    in evaluation mode whose parameters ARE the shadow.  ``update()`` is one launch per 64 tensors (kgw_weight_avg_update) that reads
    the optimiser's device step counter ``opt.step_dev`` -- after the launch that advanced it -- and decides on the device whether
    this update is an event: it can sit inside a captured step and replays with a moving alpha.  The tables cover every parameter,
    those that never get a gradient included (the first event copies them, the later ones leave them where they are)."""

    def __init__(self, model, opt, cfg):
        from copy import deepcopy
        self.cfg = parse_weight_average(cfg)
        if self.cfg is None:
            raise ValueError('WeightAverage needs a configuration (optim.parse_weight_average)')
        if not _lib.has_weight_avg():
            raise _lib.KgwasHipError('the loaded library has no weight averaging (kgw_weight_avg_update): weight_average needs it')
        self.model, self.opt = model, opt
        self.avg_model = deepcopy(model).eval()
        self._tables = []
        pairs = list(zip(self.avg_model.parameters(), model.parameters()))
        for i in range(0, len(pairs), _lib.WEIGHT_AVG_MAX):
            chunk = pairs[i:i + _lib.WEIGHT_AVG_MAX]
            n = len(chunk)
            S = (C.c_void_p * n)(); P = (C.c_void_p * n)(); N = (C.c_int64 * n)()
            for k, (s, p) in enumerate(chunk):
                if not (s.is_contiguous() and p.is_contiguous() and s.dtype == p.dtype == torch.float32 and s.shape == p.shape and
                        s.device == p.device == opt.step_dev.device and s.data_ptr() != p.data_ptr()):
                    raise _lib.KgwasHipError('WeightAverage needs contiguous fp32 parameters on the optimiser\'s device')
                S[k], P[k], N[k] = s.data_ptr(), p.data_ptr(), p.numel()
            self._tables.append((n, S, P, N))

    def started(self, n_updates: int) -> bool:
        """Has the first event happened once ``n_updates`` updates are done?  Host arithmetic; nothing is read back."""
        return int(n_updates) >= self.cfg.start_step

    def parameters(self):
        return list(self.avg_model.parameters())

    @torch.no_grad()
    def update(self):
        for n, S, P, N in self._tables:
            _lib.check(_lib.lib().kgw_weight_avg_update(n, S, P, N, self.opt.step_dev.data_ptr(), C.byref(self.cfg), _lib.stream_ptr()),
                       'kgw_weight_avg_update')


class FusedAdam:
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, lr_schedule=None, grad_clip_norm=None):
        """``lr_schedule`` (None: one rate): a _lib.KgwLrSchedule, or a spec for parse_lr_schedule that names its own total_steps; the
        rate of update t is formed in the kernels from ``step_dev``.  ``grad_clip_norm`` (None: off): ``step`` takes the global 2-norm
        of the gradients it is about to use and scales them by min(1, max_norm / (norm + 1e-6)) INSIDE the update -- the gradient
        tensors themselves stay unscaled, unlike after torch's in-place clip_grad_norm_.  With either set the calls go to the
        ``_ctl`` entry points and ``last_lr`` (a device float) holds the rate of the latest update; ``last_grad_norm`` and
        ``last_clip_scale`` (device floats) the latest norm and coefficient."""
        self.params = [p for p in params]
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.state = {}
        dev = self.params[0].device if self.params else torch.device('cuda')
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.packed_images = {}        # parameter -> persistent kgw_gemm3 operand image its fused update keeps current (step_fused)
        self.param_groups = [{'params': self.params, 'lr': lr, 'betas': betas, 'eps': eps, 'weight_decay': weight_decay}]
        self.lr_schedule = parse_lr_schedule(lr_schedule, self.lr)
        self.grad_clip_norm = check_grad_clip_norm(grad_clip_norm)
        self._ctl = None
        if self.lr_schedule is not None or self.grad_clip_norm is not None:
            if not _lib.has_optim_ctl():
                raise _lib.KgwasHipError('the loaded library has no optimiser controls (kgw_adam_ctl): lr_schedule / grad_clip_norm '
                                         'need them')
            self.last_lr = torch.full((1,), self.lr, dtype=torch.float32, device=dev)
            self.last_grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)
            self.last_clip_scale = torch.ones(1, dtype=torch.float32, device=dev)
            self._norm_ws = None
            # (clipping alone: the constant schedule, whose rate is ``lr`` to the bit)
            sched = self.lr_schedule if self.lr_schedule is not None else _lib.KgwLrSchedule(_lib.KGW_LR_CONSTANT, 0, 1, 1, 0.0, 1.0)
            self._ctl = _lib.KgwOptimCtl(sched, self.last_clip_scale.data_ptr() if self.grad_clip_norm is not None else None,
                                         self.last_lr.data_ptr())

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _state(self, p):
        st = self.state.get(p)
        if st is None:      # like torch: state is created the first time a parameter has a gradient
            st = {'exp_avg': torch.zeros_like(p, memory_format=torch.preserve_format),
                  'exp_avg_sq': torch.zeros_like(p, memory_format=torch.preserve_format)}
            self.state[p] = st
        return st

    def init_state(self):
        for p in self.params:
            if p.requires_grad:
                self._state(p)

    @torch.no_grad()
    def step_fused(self, sink, meta_ptr=None, n_layers=0, n_hops=0, stats=None):
        """The optimiser launch of a captured single-GPU step (kgw_adam_fused): the update of every parameter that has a gradient,
        the last reduction of the gradients whose producers left partial sums with ``sink`` (ops.GradSink), the step counter and
        -- ``meta_ptr``: device KgwBatchMeta of the batch, ``stats``: the trainer's int64 totals -- kgw_accumulate_stats_tick, in ONE
        launch.  Raises ops.GradSinkMismatch (nothing launched) when the fused form does not apply; the caller then runs the
        unfused step."""
        from . import ops
        if self.grad_clip_norm is not None:
            raise ops.GradSinkMismatch('grad_clip_norm needs every gradient finished before the optimiser launch: the global norm is '
                                       'taken over finished tensors, and a deferred gradient is only finished inside kgw_adam_fused')
        live = [p for p in self.params if p.grad is not None]
        # (claim: the deferred weight-gradient products' one launch, just ahead of this one, then the sourced record of every gradient)
        recs = sink.claim({p: p.grad for p in live}) if sink is not None else {}
        # a weight whose kgw_gemm3 operand image this launch keeps current must arrive as a KGW_GRAD_G3T record: updated from any other
        # kind of gradient (a complete tensor, a TN product, something autograd accumulated) the weight would change and the image the
        # next forward reads would not -- the HIP launches do not move the tensor's version counter, so nobody would notice
        for p in live:
            if p in self.packed_images and (p not in recs or recs[p].src.kind != _lib.KGW_GRAD_G3T):
                raise ops.GradSinkMismatch('the gradient of a weight with a persistent kgw_gemm3 operand image did not arrive as the '
                                           'partial sums of kgw_gemm3_partial: its image would go stale')
        if len(live) > _lib.ADAM_FUSED_MAX or len(recs) > _lib.ADAM_FUSED_SRC:
            raise ops.GradSinkMismatch(f'{len(live)} tensors / {len(recs)} deferred gradients exceed the fused launch\'s tables')
        live.sort(key=lambda p: 0 if p in recs else 1)           # the longer work units first
        n = len(live)
        if not hasattr(self, 'done_dev'):
            self.done_dev = torch.zeros(_lib.ADAM_FUSED_COUNTERS, dtype=torch.int32, device=self.step_dev.device)
        P = (C.c_void_p * n)(); G = (C.c_void_p * n)(); M = (C.c_void_p * n)(); V = (C.c_void_p * n)()
        N = (C.c_int64 * n)()
        S = (_lib.KgwGradSrc * max(n, 1))()
        for k, p in enumerate(live):
            g = p.grad
            if not (p.is_contiguous() and g.is_contiguous() and p.dtype == torch.float32 and g.dtype == torch.float32):
                raise _lib.KgwasHipError('FusedAdam needs contiguous fp32 parameters and gradients')
            st = self._state(p)
            P[k], G[k], M[k], V[k], N[k] = p.data_ptr(), g.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), p.numel()
            if p in recs:
                C.memmove(C.byref(S[k]), C.byref(recs[p].src), C.sizeof(_lib.KgwGradSrc))
                img = self.packed_images.get(p)
                if img is not None and S[k].kind == _lib.KGW_GRAD_G3T:               # the updated weight's operand image rides along
                    S[k].packed, S[k].flip = img.data_ptr(), int(_lib.lib().kgw_gemm3_flip())
        args = (n, P, G, M, V, N, S, self.step_dev.data_ptr(), self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                meta_ptr, n_layers, n_hops, stats.data_ptr() if stats is not None else None, self.done_dev.data_ptr())
        if self._ctl is not None:                  # (a schedule: the same launch, its rate formed in the kernel)
            rc = _lib.lib().kgw_adam_fused_ctl(*args, C.byref(self._ctl), _lib.stream_ptr())
        else:
            rc = _lib.lib().kgw_adam_fused(*args, _lib.stream_ptr())
        _lib.check(rc, 'kgw_adam_fused')
        # (``recs`` -- and with it the partial-sum workspaces -- lives until here: the launch that reads them is enqueued)

    @torch.no_grad()
    def finish_into(self, sink, pairs):
        """Multi-GPU step: ``pairs`` = [(parameter, its slot in a flat all-reduce bucket)].  One launch (kgw_grad_finish) writes every
        parameter's FINISHED gradient into its slot -- a copy of ``p.grad`` where that is complete, the sum of the partial records its
        producer left with ``sink`` otherwise -- instead of the producers' second launches + the bucket's concatenation.  Raises
        ops.GradSinkMismatch (nothing launched) like step_fused."""
        from . import ops
        recs = sink.claim({p: p.grad for p, _ in pairs})
        if len(recs) > _lib.ADAM_FUSED_SRC:
            raise ops.GradSinkMismatch(f'{len(recs)} deferred gradients exceed the fused launch\'s table')
        pairs = sorted(pairs, key=lambda pd: 0 if pd[0] in recs else 1)
        for i in range(0, len(pairs), _lib.ADAM_FUSED_MAX):
            chunk = pairs[i:i + _lib.ADAM_FUSED_MAX]
            n = len(chunk)
            D = (C.c_void_p * n)(); G = (C.c_void_p * n)(); N = (C.c_int64 * n)()
            S = (_lib.KgwGradSrc * n)()
            for k, (p, dst) in enumerate(chunk):
                g = p.grad
                if not (g.is_contiguous() and dst.is_contiguous() and g.dtype == torch.float32 and dst.dtype == torch.float32 and
                        dst.numel() == g.numel()):
                    raise _lib.KgwasHipError('finish_into needs contiguous fp32 gradients and bucket slots of the same size')
                D[k], G[k], N[k] = dst.data_ptr(), g.data_ptr(), g.numel()
                if p in recs:
                    C.memmove(C.byref(S[k]), C.byref(recs[p].src), C.sizeof(_lib.KgwGradSrc))
            _lib.check(_lib.lib().kgw_grad_finish(n, D, G, N, S, _lib.stream_ptr()), 'kgw_grad_finish')

    @torch.no_grad()
    def step(self, grads=None, tick=True):
        """``grads``: optional {parameter: gradient tensor} to use instead of ``p.grad`` (the all-reduced bucket's
        views in the multi-GPU step); parameters missing from it are skipped.  ``tick=False``: the caller advances
        ``step_dev`` itself after this call (kgw_accumulate_stats_tick in the captured step: one launch less)."""
        if grads is not None:
            live = [p for p in self.params if p in grads]
        else:
            live = [p for p in self.params if p.grad is not None]     # grad None => skipped, exactly like torch
        if not live:
            return
        tables = []
        for i in range(0, len(live), 64):
            chunk = live[i:i + 64]
            n = len(chunk)
            P = (C.c_void_p * n)(); G = (C.c_void_p * n)(); M = (C.c_void_p * n)(); V = (C.c_void_p * n)()
            N = (C.c_int64 * n)()
            for k, p in enumerate(chunk):
                g = grads[p] if grads is not None else p.grad
                if not (p.is_contiguous() and g.is_contiguous() and p.dtype == torch.float32 and g.dtype == torch.float32):
                    raise _lib.KgwasHipError('FusedAdam needs contiguous fp32 parameters and gradients')
                st = self._state(p)
                P[k], G[k], M[k], V[k], N[k] = p.data_ptr(), g.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), p.numel()
            tables.append((i, n, P, G, M, V, N))
        if self.grad_clip_norm is not None:
            # the global norm of exactly the gradients the update below reads (the all-reduced bucket's views when ``grads`` is
            # given: the same coefficient on every rank): one sum of squares per work unit, then one block for the rest
            L = _lib.lib()
            units = [int(L.kgw_grad_norm_workspace_doubles(n, N)) for _, n, _, _, _, _, N in tables]
            if sum(units) > 0:
                if self._norm_ws is None or self._norm_ws.numel() < sum(units):
                    self._norm_ws = torch.empty(sum(units), dtype=torch.float64, device=self.step_dev.device)
                off = 0
                for (_, n, _, G, _, _, N), u in zip(tables, units):
                    _lib.check(L.kgw_grad_norm_partial(n, G, N, self._norm_ws.data_ptr(), off, _lib.stream_ptr()), 'kgw_grad_norm_partial')
                    off += u
                _lib.check(L.kgw_grad_norm_fold(self._norm_ws.data_ptr(), off, self.grad_clip_norm, self.last_grad_norm.data_ptr(),
                                                self.last_clip_scale.data_ptr(), _lib.stream_ptr()), 'kgw_grad_norm_fold')
        for i, n, P, G, M, V, N in tables:
            # chunks > 0 must not advance the step counter again: only the last call ticks it
            last = i + 64 >= len(live)
            if self._ctl is not None:
                rc = _lib.lib().kgw_adam_ctl(n, P, G, M, V, N, self.step_dev.data_ptr(), self.lr, self.betas[0], self.betas[1],
                                             self.eps, self.weight_decay, int(tick and last), C.byref(self._ctl), _lib.stream_ptr())
                _lib.check(rc, 'kgw_adam_ctl')
                continue
            fn = _lib.lib().kgw_adam if (tick and last) else _lib.lib().kgw_adam_notick      # only the last chunk ticks
            rc = fn(n, P, G, M, V, N, self.step_dev.data_ptr(), self.lr, self.betas[0], self.betas[1],
                    self.eps, self.weight_decay, _lib.stream_ptr())
            _lib.check(rc, 'kgw_adam')
