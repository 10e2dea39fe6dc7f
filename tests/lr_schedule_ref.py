"""The learning-rate rule of include/kgwas_hip.h (KgwLrSchedule, kgwlr_at), torch's clip_grad_norm_ coefficient and
torch.optim.Adam with L2 weight decay, in numpy float64.  A twin written from the rule's text: it calls nothing from the package.

    s = t - 1                                   (t: the 1-based index of the update)
    warm(s)  = W > 0 and s < W ? (s + 1) / W : 1
    u(s)     = clamp((s - W) / max(N - W, 1), 0, 1)
    decay(s) = constant: 1 | linear: 1 - (1 - r) u | cosine: r + (1 - r) (1 + cos(pi u)) / 2 | step: gamma ^ floor(max(s - W, 0) / step_size)
    lr_t     = float32(float64(lr) * warm * decay)

lr, r = min_lr / lr and gamma are what the C structs hold: float32 values, widened."""
import math

import numpy as np

KINDS = {'constant': 0, 'linear': 1, 'cosine': 2, 'step': 3}


def f32(x):
    """The float32 nearest to ``x``, as a Python float (what a C float argument or field holds)."""
    return float(np.float32(x))


def factor(kind, t, W=0, N=1, r=0.0, step_size=1, gamma=0.1):
    """warm(s) * decay(s) in float64 (the product the rule forms after lr * warm: here without lr)."""
    s = max(int(t) - 1, 0)
    warm = (s + 1) / W if (W > 0 and s < W) else 1.0
    u = min(max((s - W) / max(N - W, 1), 0.0), 1.0)
    r, gamma = f32(r), f32(gamma)
    if kind == 'constant':
        decay = 1.0
    elif kind == 'linear':
        decay = 1.0 - (1.0 - r) * u
    elif kind == 'cosine':
        decay = r + (1.0 - r) * (1.0 + math.cos(math.pi * u)) / 2.0
    elif kind == 'step':
        decay = gamma ** (max(s - W, 0) // step_size)
    else:
        raise ValueError(kind)
    return warm, decay


def lr_at(kind, lr, t, **kw):
    """lr_t as a numpy float32."""
    warm, decay = factor(kind, t, **kw)
    return np.float32(f32(lr) * warm * decay)


def ulp32(x):
    """The spacing of float32 at |x| (at least the smallest normal's), as a Python float."""
    return float(np.spacing(np.float32(max(abs(float(x)), 1.1754944e-38))))


def grad_norm(grads):
    """The global 2-norm of ``grads`` (arrays of any shape), float64."""
    return math.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads))


def clip_scale(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient: min(1, max_norm / (norm + 1e-6)), float64."""
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


class Adam64:
    """torch.optim.Adam(lr, betas, eps, weight_decay as L2) on float64 copies; ``step(grads, lr_t, scale)`` scales the gradients
    BEFORE the L2 term is added (clip_grad_norm_ first, then Adam).  The hyper-parameters are the float32 values the kernels get."""

    def __init__(self, params, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.p = [np.asarray(p, dtype=np.float64).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.b1, self.b2, self.eps, self.wd = f32(betas[0]), f32(betas[1]), f32(eps), f32(weight_decay)
        self.t = 0

    def step(self, grads, lr_t, scale=1.0):
        self.t += 1
        bc1, bc2 = 1.0 - self.b1 ** self.t, 1.0 - self.b2 ** self.t
        for k, g in enumerate(grads):
            if g is None:
                continue
            g = np.asarray(g, dtype=np.float64) * float(scale) + self.wd * self.p[k]
            self.m[k] = self.m[k] + (1.0 - self.b1) * (g - self.m[k])
            self.v[k] = self.v[k] * self.b2 + (1.0 - self.b2) * g * g
            self.p[k] = self.p[k] - (float(lr_t) / bc1) * (self.m[k] / (np.sqrt(self.v[k]) / math.sqrt(bc2) + self.eps))
