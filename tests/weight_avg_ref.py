"""numpy restatement of the weight-averaging rule (include/kgwas_hip.h: KgwWeightAvg, kgwavg_alpha) and of a whole trajectory of
shadows.  alpha is the float32 value the rule defines (its few operations are float32 by definition); the shadows are carried in
float64: s <- s + alpha (p - s), a copy of p where alpha == 1."""
import numpy as np

KINDS = {'ema': 0, 'swa': 1}
DEFAULTS = dict(start_step=1, every=1, warmup=True, decay=0.999)


def alpha_at(kind, n, start_step=1, every=1, warmup=True, decay=0.999):
    """(is update n an averaging event, alpha as np.float32 or None).  n = the number of updates done, n >= 1."""
    if n < start_step or (n - start_step) % every != 0:
        return False, None
    k = (n - start_step) // every
    if kind == 'swa':
        return True, np.float32(1.0) / np.float32(k + 1)
    if k == 0:
        return True, np.float32(1.0)
    d = np.float32(decay)
    if warmup:
        d = min(d, np.float32(1 + k) / np.float32(10 + k))
    return True, np.float32(1.0) - np.float32(d)


def update(shadow, params, kind, n, **cfg):
    """The float64 shadows after update n: ``shadow`` / ``params`` lists of arrays; returns new arrays (the old ones on a non-event)."""
    event, a = alpha_at(kind, n, **cfg)
    if not event:
        return [np.asarray(s, np.float64) for s in shadow]
    if a == np.float32(1.0):
        return [np.asarray(p, np.float64).copy() for p in params]
    a = np.float64(a)
    return [np.asarray(s, np.float64) + a * (np.asarray(p, np.float64) - np.asarray(s, np.float64)) for s, p in zip(shadow, params)]


def replay(shadow0, snapshots, kind, first_n=1, **cfg):
    """``snapshots[i]``: the parameters after update first_n + i.  Returns the float64 shadows after the last of them."""
    s = [np.asarray(x, np.float64) for x in shadow0]
    for i, params in enumerate(snapshots):
        s = update(s, params, kind, first_n + i, **cfg)
    return s
