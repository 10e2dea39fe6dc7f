"""numpy twin of the finite fan-out rule of kgw_sample_batch_fanout, restated from include/kgwas_hip.h:

    key(p)  = mix32(row_hash(sample_seed, relation id, global destination id) ^ p)      p = position in the CSR row
    segment = the k entries with the smallest (key, position), kept in CSR order

and of the hop-by-hop expansion around it (a node is expanded once, at the hop that first reached it; the nodes new at a
hop are ordered by global id).  Nothing here calls the package: the tests hand it the graph's CSR."""
import numpy as np

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1


def mix32(h):
    """MurmurHash3's 32-bit finaliser on a uint64 array / int holding 32-bit words."""
    h = np.asarray(h, dtype=np.uint64) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return h


def _step(h, x):
    return mix32(((np.uint64(h) ^ np.uint64(x & M32)) + np.uint64(0x9E3779B9)) & np.uint64(M32))


def row_hash(sample_seed, rel, dst):
    sample_seed = int(sample_seed) & M64
    h = _step(0, sample_seed & M32)
    h = _step(h, sample_seed >> 32)
    h = _step(h, int(rel))
    return _step(h, int(dst))


def keys(sample_seed, rel, dst, deg):
    return mix32(np.uint64(row_hash(sample_seed, rel, dst)) ^ np.arange(deg, dtype=np.uint64))


def draw(sample_seed, rel, dst, deg, k):
    """Positions (ascending) of the entries of a row of ``deg`` entries kept at fan-out ``k`` (-1 = all)."""
    if k < 0 or deg <= k:
        return np.arange(deg, dtype=np.int64)
    pos = np.arange(deg, dtype=np.int64)
    order = np.lexsort((pos, keys(sample_seed, rel, dst, deg)))        # by key, position breaks ties
    return np.sort(order[:k])


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_word(seed, epoch, batch):
    """The loader's 64-bit sample seed of (seed, epoch, batch index)."""
    z = _splitmix64(int(seed) & M64)
    z = _splitmix64(z ^ (int(epoch) & M64))
    return _splitmix64(z ^ (int(batch) & M64))


def sample_batch(csr, src_type, dst_type, n_types, seed_type, seeds, fanout, word):
    """``csr``: per relation (rowptr, col) of the dst-major CSR.  Returns (hops, segs): hops[h][t] = global ids new at hop h
    (seeds in seed order, later hops ascending), segs[(h, r)] = list, per node of hops[h][dst_type[r]], of the global source
    ids its segment holds."""
    seen = [set() for _ in range(n_types)]
    hops = [[np.zeros(0, np.int64) for _ in range(n_types)]]
    hops[0][seed_type] = np.asarray(seeds, dtype=np.int64)
    seen[seed_type].update(int(s) for s in seeds)
    segs = {}
    for h, k in enumerate(fanout):
        reached = [set() for _ in range(n_types)]
        for r, (rp, col) in enumerate(csr):
            out = []
            for v in hops[h][dst_type[r]]:
                row = np.asarray(col[rp[v]:rp[v + 1]], dtype=np.int64)
                row = row[draw(word, r, int(v), len(row), k)]
                out.append(row)
                reached[src_type[r]].update(int(s) for s in row)
            segs[(h, r)] = out
        nxt = []
        for t in range(n_types):
            new = np.array(sorted(reached[t] - seen[t]), dtype=np.int64)
            seen[t].update(int(s) for s in new)
            nxt.append(new)
        hops.append(nxt)
    return hops, segs
