// kgw_dense_wavg.h -- weight averaging (KGWAS.train(weight_average=...)): the shadow copy of every parameter moves towards the
// parameter in one element-wise launch behind the optimiser's (the rule: KgwWeightAvg / kgwavg_alpha in include/kgwas_hip.h; alpha
// is formed in the kernel from the device step counter, so a captured step replays with a moving alpha).  Part of kgw_dense.hip.
#pragma once

namespace {
struct WAvgTab {
    float* s[KGW_WEIGHT_AVG_MAX]; const float* p[KGW_WEIGHT_AVG_MAX];
    int64_t off[KGW_WEIGHT_AVG_MAX + 1];      // prefix sums of element counts
    int64_t coff[KGW_WEIGHT_AVG_MAX + 1];     // prefix sums of work units
    unsigned char vec[KGW_WEIGHT_AVG_MAX];    // both pointers 16-byte aligned: float4 path
    int n;
};

__device__ __forceinline__ float wavg_elem(float alpha, float p, float s) {
#pragma clang fp contract(off)
    return fmaf(alpha, p - s, s);
}

// Work unit = k_adam's (KGW_WEIGHT_AVG_UNIT consecutive elements of ONE tensor, 256 threads x float4; the unit's tensor found with
// wave-uniform comparisons).  The counter is a kernel-argument pointer loaded before any store: one scalar load per wavefront, and
// with it event and alpha are wave-uniform -- a non-event returns before anything else is read.  Memory-bound on an event: 8 bytes
// in and 4 out per element (4 in with alpha == 1: the shadow is not read, so whatever it held -- a NaN -- cannot reach the copy).
__global__ void __launch_bounds__(256) k_weight_avg(WAvgTab T, const int32_t* __restrict__ step, KgwWeightAvg A) {
    float alpha = 0.0f;
    if (!kgwavg_alpha(&A, *step, &alpha)) return;
    const bool copy = alpha == 1.0f;
    const int64_t units = T.coff[T.n];
    for (int64_t c = blockIdx.x; c < units; c += gridDim.x) {
        int lo = 0, hi = T.n;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (T.coff[mid] <= c) lo = mid; else hi = mid; }
        const int64_t n = T.off[lo + 1] - T.off[lo];
        const int64_t j = (c - T.coff[lo]) * KGW_WEIGHT_AVG_UNIT + (int64_t)threadIdx.x * 4;
        float* __restrict__ S = T.s[lo];
        const float* __restrict__ P = T.p[lo];
        if (j + 4 <= n && T.vec[lo]) {
            const float4 p = *(const float4*)(P + j);
            if (copy) {
                *(float4*)(S + j) = p;
            } else {
                const float4 s = *(const float4*)(S + j);
                *(float4*)(S + j) = make_float4(wavg_elem(alpha, p.x, s.x), wavg_elem(alpha, p.y, s.y), wavg_elem(alpha, p.z, s.z),
                                                wavg_elem(alpha, p.w, s.w));
            }
        } else {
            for (int64_t i = j; i < n && i < j + 4; ++i) S[i] = copy ? P[i] : wavg_elem(alpha, P[i], S[i]);
        }
    }
}
}  // namespace

extern "C" int kgw_weight_avg_update(int32_t n_tensors, float* const* shadow, const float* const* params, const int64_t* numel,
                                     const int32_t* step_dev, const KgwWeightAvg* cfg, kgw_stream_t stream_) {
    if (!cfg) return KGW_E_NULL;
    if (!kgwavg_valid(cfg)) return KGW_E_RANGE;
    if (n_tensors < 0 || n_tensors > KGW_WEIGHT_AVG_MAX) return KGW_E_RANGE;
    if (n_tensors == 0) return KGW_OK;
    if (!shadow || !params || !numel || !step_dev) return KGW_E_NULL;
    WAvgTab T;
    T.n = n_tensors;
    T.off[0] = 0;
    T.coff[0] = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] < 0) return KGW_E_RANGE;
        if ((!shadow[i] || !params[i]) && numel[i] > 0) return KGW_E_NULL;
        T.s[i] = shadow[i]; T.p[i] = params[i];
        T.off[i + 1] = T.off[i] + numel[i];
        T.coff[i + 1] = T.coff[i] + (numel[i] + KGW_WEIGHT_AVG_UNIT - 1) / KGW_WEIGHT_AVG_UNIT;
        T.vec[i] = (((uintptr_t)shadow[i] | (uintptr_t)params[i]) & 15) == 0;
    }
    int64_t g = T.coff[n_tensors];
    if (g < 1) return KGW_OK;                                          // (empty tensors only: no unit, nothing to write)
    if (g > 4 * KGW_GRID) g = 4 * KGW_GRID;
    k_weight_avg<<<(int)g, 256, 0, (hipStream_t)stream_>>>(T, step_dev, *cfg);
    KGW_LAUNCH_CHECK();
    return KGW_OK;
}

extern "C" float kgw_weight_avg_alpha(const KgwWeightAvg* cfg, int32_t n, int32_t* event) {
    if (event) *event = 0;
    if (!cfg || !kgwavg_valid(cfg) || n < 1) return NAN;
    float alpha = 0.0f;
    const int ev = kgwavg_alpha(cfg, n, &alpha);
    if (event) *event = ev;
    return ev ? alpha : 0.0f;
}
