"""Float64 numpy statement of the read-out + loss node with a loss kind (kgw_readout_loss_*, include/kgwas_hip.h: KgwReadoutLossArgs):
the specification the CPU test checks against torch's huber_loss with autograd and against tests/multitrait_w_ref.py at delta = +inf,
and the GPU tests check the kernels against.

    pred[i][t] = [relu](<H[i], W[t]> + b[t])                                          i < n, t < T
    r[i][t]    = pred[i][t] - y[n_id[i]][t]   where the pair's weight != 0,   0 elsewhere    (an unobserved pair never reads its label)
    rho_d(r)   = r^2 if |r| <= d else d (2 |r| - d);      rho_d'(r) = 2 clamp(r, -d, d)
    loss       = 1 / (n T) * sum_i sum_t w * rho_delta[t](r[i][t])                     (n T whatever is observed)
    g[i][t]    = gloss / (n T) * w * rho_delta[t]'(r[i][t])                             (0 where the ReLU is off)
    dH[i] = sum_t g[i][t] W[t]  (rows n.. are zero; relu bit 1: dH *= H > 0),   dW[t] = sum_i g[i][t] H[i],   db[t] = sum_i g[i][t]

w is [N] (one weight per node, shared by the columns) or [N, T].  At delta = +inf every expression is readout_wmse_w_np's, in its
order: the outputs are equal, not just close."""
import numpy as np

from tests.multitrait_ref import make_case                  # noqa: F401  (the cases of the tests that use this twin)
from tests.multitrait_w_ref import make_case_w              # noqa: F401


def weights_of_seeds(w, n_id, n, T):
    """w [N] or [N, T] -> the float64 weights [n, T] of the seeds' pairs."""
    ids = np.asarray(n_id, np.int64)[:n]
    w = np.asarray(w, np.float64)
    return np.repeat(w[ids][:, None], T, axis=1) if w.ndim == 1 else w[ids].reshape(n, T)


def residuals_np(H, W, b, n_id, y, w, n, relu):
    """(z, pred, r, wi, seen) of the statement above, all [n, T] float64."""
    H, W, b = np.asarray(H, np.float64), np.asarray(W, np.float64).reshape(-1, H.shape[1]), np.asarray(b, np.float64).reshape(-1)
    ids = np.asarray(n_id, np.int64)[:n]
    T = W.shape[0]
    wi = weights_of_seeds(w, n_id, n, T)
    seen = wi != 0
    yi = np.zeros((n, T))
    yi[seen] = np.asarray(y).reshape(-1, T)[ids][seen].astype(np.float64)     # masked BEFORE the subtraction
    z = H[:n] @ W.T + b
    pred = np.maximum(z, 0) if relu & 1 else z
    return z, pred, np.where(seen, pred - yi, 0), wi, seen


def readout_loss_np(H, W, b, n_id, y, w, n, relu, gloss, rows, delta):
    """Returns (pred [n,T], loss, dH [rows,128], dW [T,128], db [T]) in float64.  ``delta``: one knee or T of them, each > 0 or +inf;
    ``relu``: bit 0 = ReLU on pred, bit 1 = fold dH *= (H > 0)."""
    H = np.asarray(H, np.float64)
    W = np.asarray(W, np.float64).reshape(-1, H.shape[1])
    T = W.shape[0]
    rows = H.shape[0] if rows is None else rows
    delta = np.broadcast_to(np.asarray(delta, np.float64), (T,))
    assert (delta > 0).all()
    z, pred, d, wi, _ = residuals_np(H, W, b, n_id, y, w, n, relu)
    quad = np.abs(d) <= delta
    with np.errstate(invalid='ignore'):                      # (the branch not taken: inf - inf at delta = +inf)
        terms = np.where(quad, wi * d * d, wi * (delta * (2 * np.abs(d) - delta)))
        dc = np.where(quad, d, np.sign(d) * delta)           # clamp(d, -delta, delta)
    loss = terms.sum() / (n * T)
    g = gloss * 2 * wi * dc / (n * T)
    if relu & 1:
        g = g * (z > 0)
    dH = np.zeros((rows, H.shape[1]))
    dH[:n] = g @ W
    if relu & 2:
        dH[:n] *= H[:n] > 0
    return pred, float(loss), dH, g.T @ H[:n], g.sum(0)
