"""numpy twin of the per-epoch order of the training seeds (kgw_epoch_order), restated from include/kgwas_hip.h:

    base             = step(step(0, lo32(word)), hi32(word))                  step(h, x) = mix32((h ^ x) + 0x9e3779b9)
    hb               : k = max(2, bit_length(n - 1));  k += k & 1;  hb = k / 2
    feistel(p)       : L = p >> hb, R = p & mask;  r = 0 .. 3:  F = mix32(step(base, r) ^ R) & mask;  (L, R) = (R, L ^ F)
                       result (L << hb) | R
    index(base, n, i): p = i;  do p = feistel(p) while (p >= n)

and of the host's word, order_word(seed, epoch).  Nothing here calls the package."""
import numpy as np

from tests.fanout_ref import M32, M64, _splitmix64, _step, mix32

ORDER_TAG = int.from_bytes(b'shuffle!', 'big')


def order_word(seed, epoch):
    z = _splitmix64(ORDER_TAG)
    z = _splitmix64(z ^ (int(seed) & M64))
    return _splitmix64(z ^ (int(epoch) & M64))


def base(word):
    word = int(word) & M64
    return int(_step(_step(0, word & M32), word >> 32))


def half_bits(n):
    k = max(2, int(n - 1).bit_length())
    k += k & 1
    return k // 2


def feistel(b, hb, p):
    """One application of the four-round network to the uint64 array ``p`` of 2 * hb-bit words."""
    mask = np.uint64((1 << hb) - 1)
    p = np.asarray(p, dtype=np.uint64)
    L, R = p >> np.uint64(hb), p & mask
    for r in range(4):
        F = mix32(np.uint64(int(_step(b, r))) ^ R) & mask
        L, R = R, L ^ F
    return (L << np.uint64(hb)) | R


def permutation(word, n, with_walks=False):
    """int64 [n]: index(base(word), n, i) for every i < n (and, on request, the number of applications each walk took)."""
    b, hb = base(word), half_bits(n)
    p = np.arange(n, dtype=np.uint64)
    out = np.empty(n, dtype=np.int64)
    walks = np.zeros(n, dtype=np.int64)
    todo = np.arange(n)
    while todo.size:
        p = feistel(b, hb, p)
        walks[todo] += 1
        done = p < np.uint64(n)
        out[todo[done]] = p[done].astype(np.int64)
        todo, p = todo[~done], p[~done]
    return (out, walks) if with_walks else out


def epoch_positions(word, n, B, mode):
    """int64 [n]: the index into ids that every position of the epoch holds; ``mode`` 'seeds' or 'batches', ``B`` the GLOBAL batch."""
    if mode == 'seeds':
        return permutation(word, n)
    assert mode == 'batches'
    nb = n // B
    out = np.arange(n, dtype=np.int64)
    if nb:
        src = permutation(word, nb)
        out[:nb * B] = (src[:, None] * B + np.arange(B)[None, :]).reshape(-1)
    return out


def rank_positions(n, B, rank, world):
    """Positions of the epoch that rank ``rank`` of ``world`` holds, in the order it visits them: its slice of every full batch,
    and for one rank the partial batch behind them."""
    nb, per = n // B, B // world
    pos = (np.arange(nb)[:, None] * B + rank * per + np.arange(per)[None, :]).reshape(-1)
    return np.concatenate([pos, np.arange(nb * B, n)]) if world == 1 else pos


def epoch_order(ids, B, mode, word, rank=0, world=1):
    """What kgw_epoch_order writes for this rank."""
    ids = np.asarray(ids, dtype=np.int64)
    n = len(ids)
    return ids[epoch_positions(word, n, B, mode)[rank_positions(n, B, rank, world)]]
