"""Float64 numpy statement of the multi-trait read-out + loss node with a weight MATRIX (kgw_readout_wmse_mtw_*): the specification
the CPU test checks against tests/multitrait_ref.py and finite differences, and the GPU tests check the kernels against.

    pred[i][t] = [relu](<H[i], W[t]> + b[t])                                          i < n, t < T
    r[i][t]    = pred[i][t] - y[n_id[i]][t]   where w[n_id[i]][t] != 0,   0 elsewhere    (an unobserved pair never reads its label)
    loss       = 1 / (n T) * sum_i sum_t w[n_id[i]][t] * r[i][t]^2                     (n T whatever is observed)
    g[i][t]    = gloss / (n T) * w[n_id[i]][t] * 2 r[i][t]                              (0 where the ReLU is off)
    dH[i] = sum_t g[i][t] W[t]  (rows n.. are zero; relu bit 1: dH *= H > 0),   dW[t] = sum_i g[i][t] H[i],   db[t] = sum_i g[i][t]
"""
import numpy as np

from tests.multitrait_ref import make_case


def readout_wmse_w_np(H, W, b, n_id, y, w, n, relu=1, gloss=1.0, rows=None, dtype=np.float64):
    """Returns (pred [n,T], loss, dH [rows,128], dW [T,128], db [T]).  ``w`` [N,T]; ``relu``: bit 0 = ReLU on pred, bit 1 = fold
    dH *= (H > 0).  ``dtype``: float64, the statement; a wider type serves the finite-difference check of the statement itself."""
    H, W, b = np.asarray(H, dtype), np.asarray(W, dtype), np.asarray(b, dtype)
    ids = np.asarray(n_id, np.int64)[:n]
    T = W.shape[0]
    rows = H.shape[0] if rows is None else rows
    wi = np.asarray(w, dtype)[ids].reshape(n, T)
    seen = wi != 0
    yi = np.zeros((n, T), dtype)
    yi[seen] = np.asarray(y).reshape(-1, T)[ids][seen].astype(dtype)          # masked BEFORE the subtraction
    z = H[:n] @ W.T + b
    pred = np.maximum(z, 0) if relu & 1 else z
    d = np.where(seen, pred - yi, 0)
    loss = (wi * d * d).sum() / (n * T)
    g = gloss * 2 * wi * d / (n * T)
    if relu & 1:
        g = g * (z > 0)
    dH = np.zeros((rows, H.shape[1]), dtype)
    dH[:n] = g @ W
    if relu & 2:
        dH[:n] *= H[:n] > 0
    return pred, (float(loss) if dtype is np.float64 else loss), dH, g.T @ H[:n], g.sum(0)


def make_case_w(n, T, rows, seed, p_zero=0.5, poison=True):
    """make_case's inputs with a weight matrix [N, T]: every entry 0 with probability ``p_zero``, U(0.5, 1.5) otherwise; with
    ``poison`` the label of every zero-weight entry is NaN, +Inf or -Inf in turn."""
    H, W, b, n_id, y, _ = make_case(n, T, rows, seed)
    rng = np.random.default_rng(seed + 1_000_003)
    N = y.shape[0]
    w = rng.uniform(0.5, 1.5, (N, T)) * (rng.random((N, T)) >= p_zero)
    if poison:
        y = y.copy()
        r, c = np.nonzero(w == 0)
        y[r, c] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(len(r)) % 3]
    return H, W, b, n_id, y, np.ascontiguousarray(w)
