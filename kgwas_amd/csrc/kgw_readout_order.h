// kgw_readout_order.h -- the summation orders of the read-out node's fold (kgw_dense_loss.h: k_wmse_fwd, k_readout_fold;
// kgw_dense_transform.h: readout_train_fold_block256), each stated ONCE.  "No float atomics: reruns are bit-identical", and the fold of
// a step may run as its own launch or as one more block of k_transform_bwd: every place that adds these numbers up does it here.
#pragma once
#include "kgw_common.h"

// term(0) + ... + term(n - 1) in float64: thread x < 256 adds up q = x, x + 256, ... and a halving tree over sd[256] finishes.  EVERY
// thread of the block calls it (barriers inside; the first one also publishes what the caller wrote to LDS before); all get the sum.
template <class F>
__device__ __forceinline__ double kgw_sum256_f64(double* sd, int n, F term) {
    if (threadIdx.x < 256) {
        double acc = 0.0;
        for (int q = threadIdx.x; q < n; q += 256) acc += term(q);
        sd[threadIdx.x] = acc;
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sd[threadIdx.x] += sd[threadIdx.x + o];
        __syncthreads();
    }
    return sd[0];
}

// Column sums of the per-block partials (rows of 129 = 128 weight columns + the bias term): pair (c, g), g < 7, walks the rows
// q = g, g + 7, ... < nb of its column p (row stride ld) with four interleaved accumulators -- rounds of 28 rows, the rest into a0.
struct KgwWalk4 { float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f; };

__device__ __forceinline__ void kgw_walk_round(KgwWalk4& a, const float* __restrict__ p, int q, int64_t ld) {
    a.a0 += p[(int64_t)q * ld];        a.a1 += p[(int64_t)(q + 7) * ld];
    a.a2 += p[(int64_t)(q + 14) * ld]; a.a3 += p[(int64_t)(q + 21) * ld];
}

// the walk from row q on (q = g: all of it; later: the rounds before q are in `a` already) and the pair's sum
__device__ __forceinline__ float kgw_walk_finish(KgwWalk4& a, const float* __restrict__ p, int q, int nb, int64_t ld) {
    for (; q + 21 < nb; q += 28) kgw_walk_round(a, p, q, ld);
    for (; q < nb; q += 7) a.a0 += p[(int64_t)q * ld];
    return (a.a0 + a.a1) + (a.a2 + a.a3);
}

// column c's total from the seven groups' sums sm[g][c]
__device__ __forceinline__ float kgw_tree7(const float (*sm)[KGW_C + 1], int c) {
    return ((sm[0][c] + sm[1][c]) + (sm[2][c] + sm[3][c])) + ((sm[4][c] + sm[5][c]) + sm[6][c]);
}
