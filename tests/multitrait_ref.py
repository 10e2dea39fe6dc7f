"""Float64 numpy statement of the multi-trait read-out + loss node (kgw_readout_wmse_mt_*): the specification the CPU test checks
against torch.autograd and the GPU tests check the kernels against.

    pred[i][t] = [relu](<H[i], W[t]> + b[t])                                   i < n, t < T
    loss       = 1 / (n T) * sum_i sum_t w[n_id[i]] * (pred[i][t] - y[n_id[i]][t])^2
    g[i][t]    = gloss / (n T) * w[n_id[i]] * 2 (pred[i][t] - y[n_id[i]][t])      (0 where the ReLU is off)
    dH[i] = sum_t g[i][t] W[t]  (rows n.. are zero; relu bit 1: dH *= H > 0),   dW[t] = sum_i g[i][t] H[i],   db[t] = sum_i g[i][t]
"""
import numpy as np


def readout_wmse_np(H, W, b, n_id, y, w, n, relu=1, gloss=1.0, rows=None):
    """Returns (pred [n,T], loss, dH [rows,128], dW [T,128], db [T]) in float64.  ``relu``: bit 0 = ReLU on pred, bit 1 = fold
    dH *= (H > 0)."""
    H, W, b = np.asarray(H, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    y, w = np.asarray(y, np.float64), np.asarray(w, np.float64)
    ids = np.asarray(n_id, np.int64)[:n]
    T = W.shape[0]
    rows = H.shape[0] if rows is None else rows
    z = H[:n] @ W.T + b
    pred = np.maximum(z, 0.0) if relu & 1 else z
    wi = w[ids][:, None]
    d = pred - y[ids].reshape(n, T)
    loss = float((wi * d * d).sum() / (n * T))
    g = gloss * 2.0 * wi * d / (n * T)
    if relu & 1:
        g = g * (z > 0)
    dH = np.zeros((rows, H.shape[1]))
    dH[:n] = g @ W
    if relu & 2:
        dH[:n] *= H[:n] > 0
    return pred, loss, dH, g.T @ H[:n], g.sum(0)


def make_case(n, T, rows, seed, n_nodes=None):
    """Inputs of one kernel case: H is a ReLU output (exact zeros, so bit 1 of ``relu`` matters), n_id repeats ids (drawn with
    replacement from a table shorter than n when n > 2), and the node of seed 0 has weight 0."""
    rng = np.random.default_rng(seed)
    N = n_nodes or max(3, (n * 2) // 3)
    H = np.maximum(rng.standard_normal((rows, 128)), 0.0).astype(np.float32)
    W = (rng.standard_normal((T, 128)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(T) * 0.1).astype(np.float32)
    n_id = rng.integers(0, N, size=n).astype(np.int32)
    if n >= 3:
        n_id[2] = n_id[1]
    y = (rng.standard_normal((N, T)) ** 2).astype(np.float32)
    w = rng.uniform(0.5, 1.5, N)
    w[n_id[0]] = 0.0
    return H, W, b, n_id, y, w
