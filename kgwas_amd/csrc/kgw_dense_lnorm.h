// kgw_dense_lnorm.h -- layer normalisation + ReLU between the message-passing layers (HeteroGNN(gnn_norm='layer')): the forward,
// the backward with per-block partial column sums, and their fold (the rule: kgwlnorm_* in include/kgwas_hip.h).  Part of
// kgw_dense.hip.
#pragma once

namespace {
constexpr int LN_SLOTS = KGW_BLK / 32;      // rows a block holds at a time: 32 lanes per row
constexpr int LN_ROWS_PER_BLOCK = 64;       // backward: rows per block before the grid cap doubles it

struct LNormFwd {
    int n;                          // jobs with rows > 0
    int c;                          // c_logical
    float cf, eps;                  // (float)c_logical
    int64_t total;                  // rows of all jobs
    int64_t end[8];                 // end[j]: rows of jobs 0 .. j
    KgwLNormJob j[8];
};

// sum over the 32 lanes of a row: xor 16, 8, 4, 2, 1 stay inside a 32-lane half, so the two rows of a wavefront never mix
__device__ __forceinline__ float ln_row_sum(float v) {
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The differences y_c - mean of a row, given a float32 mean m (the forward's first quotient, or the stored mean): r_c = y_c - m,
// *corr = sum(r) / Cl, d_c = r_c - *corr.  A float32 mean of a row around 1e4 is good to half an ulp of 1e4, 5e-4, which against
// a unit spread would shift every xh by that much; the residuals are small, so their mean is known to ~1e-7 of the spread and
// m + *corr is the mean as well as float32 holds it.  (0 for the columns past Cl; a constant row: r = 0, *corr = 0, d = 0.)
__device__ __forceinline__ float4 ln_centre(float4 y, float m, float cf, bool v0, bool v1, bool v2, bool v3, float* corr) {
    const float r0 = v0 ? y.x - m : 0.f, r1 = v1 ? y.y - m : 0.f, r2 = v2 ? y.z - m : 0.f, r3 = v3 ? y.w - m : 0.f;
    const float c = ln_row_sum((r0 + r1) + (r2 + r3)) / cf;
    *corr = c;
    return make_float4(v0 ? r0 - c : 0.f, v1 ? r1 - c : 0.f, v2 ? r2 - c : 0.f, v3 ? r3 - c : 0.f);
}

// One float4 per lane, 32 lanes per row, two rows per wavefront, grid-stride over the rows of all jobs (k_hidden_dropout's
// mapping).  Memory-bound: 512 B in, 520 B out per row; the row stays in registers between the passes (mean, its correction,
// variance).
__global__ void __launch_bounds__(KGW_BLK) k_layer_norm_relu_fwd(LNormFwd J) {
    const int c4 = threadIdx.x & 31;
    const int col = 4 * c4;
    const int64_t stride = (int64_t)gridDim.x * LN_SLOTS;
    const bool v0 = col < J.c, v1 = col + 1 < J.c, v2 = col + 2 < J.c, v3 = col + 3 < J.c;
    for (int64_t r = (int64_t)blockIdx.x * LN_SLOTS + (threadIdx.x >> 5); r < J.total; r += stride) {
        int q = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) q += (k < J.n - 1 && r >= J.end[k]) ? 1 : 0;
        const KgwLNormJob& jb = J.j[q];
        const int64_t row = r - (q ? J.end[q - 1] : 0);
        const float4 y = ((const float4*)(jb.src + row * jb.lds))[c4];
        const float4 w = ((const float4*)jb.weight)[c4];
        const float4 b = ((const float4*)jb.bias)[c4];
        // (divisions, not products with 1 / Cl: a constant row of exactly summable values then has mean = the value and var = 0)
        const float m0 = ln_row_sum(((v0 ? y.x : 0.f) + (v1 ? y.y : 0.f)) + ((v2 ? y.z : 0.f) + (v3 ? y.w : 0.f))) / J.cf;
        float corr;
        const float4 d = ln_centre(y, m0, J.cf, v0, v1, v2, v3, &corr);
        const float mean = m0 + corr;
        const float var = ln_row_sum((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) / J.cf;
        const float rstd = 1.0f / sqrtf(var + J.eps);
        float4 o;
        o.x = v0 ? kgwlnorm_out(d.x * rstd, w.x, b.x) : 0.0f;
        o.y = v1 ? kgwlnorm_out(d.y * rstd, w.y, b.y) : 0.0f;
        o.z = v2 ? kgwlnorm_out(d.z * rstd, w.z, b.z) : 0.0f;
        o.w = v3 ? kgwlnorm_out(d.w * rstd, w.w, b.w) : 0.0f;
        ((float4*)(jb.dst + row * jb.ldd))[c4] = o;
        if (c4 == 0) ((float2*)jb.stat)[row] = make_float2(mean, rstd);
    }
}

struct LNormBwd {
    int n;                          // jobs with rows > 0
    int c;
    float cf, inv_c;                // (float)c_logical and its reciprocal
    float* partial;                 // [grid][2][128]
    int bend[8];                    // bend[j]: blocks of jobs 0 .. j
    KgwLNormBwdJob j[8];
};

// The blocks [bend[q - 1], bend[q]) belong to job q and walk its rows with stride 8 * (their number): which block adds which
// rows, and in which order, depends on the row counts alone.  Per row three butterflies (the centring, mean(gh), mean(gh xh));
// the column sums of a slot stay in registers over its rows and the 8 slots are added through LDS in slot order.
__global__ void __launch_bounds__(KGW_BLK) k_layer_norm_bwd(LNormBwd J) {
    // (no contraction here: a product g w fused into the row sum would differ, in its last bit, from the rounded gh that dy
    //  subtracts the sum's mean from -- with one column that difference, times rstd, is all of dy)
#pragma clang fp contract(off)
    __shared__ __align__(16) float sm[LN_SLOTS][2][KGW_C];
    const int c4 = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const int col = 4 * c4;
    int q = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) q += (k < J.n - 1 && (int)blockIdx.x >= J.bend[k]) ? 1 : 0;
    const KgwLNormBwdJob& jb = J.j[q];
    const int b0 = q ? J.bend[q - 1] : 0;
    const int64_t stride = (int64_t)(J.bend[q] - b0) * LN_SLOTS;
    const bool v0 = col < J.c, v1 = col + 1 < J.c, v2 = col + 2 < J.c, v3 = col + 3 < J.c;
    const float4 w = ((const float4*)jb.weight)[c4];
    float4 aw = make_float4(0.f, 0.f, 0.f, 0.f), ab = aw;
    for (int64_t row = (int64_t)((int)blockIdx.x - b0) * LN_SLOTS + slot; row < jb.rows; row += stride) {
        float4 g = ((const float4*)(jb.g + row * jb.ldg))[c4];
        const float4 y = ((const float4*)(jb.y + row * jb.ldy))[c4];
        const float2 st = ((const float2*)jb.stat)[row];
        if (jb.out) {
            const float4 o = ((const float4*)(jb.out + row * jb.ldo))[c4];
            g.x = o.x > 0.f ? g.x : 0.f; g.y = o.y > 0.f ? g.y : 0.f; g.z = o.z > 0.f ? g.z : 0.f; g.w = o.w > 0.f ? g.w : 0.f;
        }
        g.x = v0 ? g.x : 0.f; g.y = v1 ? g.y : 0.f; g.z = v2 ? g.z : 0.f; g.w = v3 ? g.w : 0.f;
        float corr;                 // (the stored mean is the forward's, rounded once more: centre again, as the forward did)
        const float4 dc = ln_centre(y, st.x, J.cf, v0, v1, v2, v3, &corr);
        const float4 xh = make_float4(dc.x * st.y, dc.y * st.y, dc.z * st.y, dc.w * st.y);
        const float4 gh = make_float4(g.x * w.x, g.y * w.y, g.z * w.z, g.w * w.w);
        const float m1 = ln_row_sum(gh.x + gh.y + gh.z + gh.w) * J.inv_c;
        const float m2 = ln_row_sum(gh.x * xh.x + gh.y * xh.y + gh.z * xh.z + gh.w * xh.w) * J.inv_c;
        float4 d;
        d.x = v0 ? kgwlnorm_dy(gh.x, xh.x, st.y, m1, m2) : 0.0f; d.y = v1 ? kgwlnorm_dy(gh.y, xh.y, st.y, m1, m2) : 0.0f;
        d.z = v2 ? kgwlnorm_dy(gh.z, xh.z, st.y, m1, m2) : 0.0f; d.w = v3 ? kgwlnorm_dy(gh.w, xh.w, st.y, m1, m2) : 0.0f;
        ((float4*)(jb.dy + row * jb.lddy))[c4] = d;
        aw.x += g.x * xh.x; aw.y += g.y * xh.y; aw.z += g.z * xh.z; aw.w += g.w * xh.w;
        ab.x += g.x; ab.y += g.y; ab.z += g.z; ab.w += g.w;
    }
    ((float4*)sm[slot][0])[c4] = aw;
    ((float4*)sm[slot][1])[c4] = ab;
    __syncthreads();
    const int k = threadIdx.x >> 7, c = threadIdx.x & (KGW_C - 1);
    float s = sm[0][k][c];
#pragma unroll
    for (int i = 1; i < LN_SLOTS; ++i) s += sm[i][k][c];
    J.partial[(int64_t)blockIdx.x * (2 * KGW_C) + threadIdx.x] = s;
}

struct LNormFold {
    const float* partial;
    float* dweight; float* dbias;   // [n_types][128]
    int b0[8], b1[8];               // by node type: its job's blocks [b0, b1) of the backward's grid; b0 == b1: none
};

// block t: thread (k, c) adds partial[b][k][c] over the blocks of type t's job in ascending order
__global__ void __launch_bounds__(KGW_BLK) k_layer_norm_fold(LNormFold F) {
    const int t = blockIdx.x, k = threadIdx.x >> 7, c = threadIdx.x & (KGW_C - 1);
    float s = 0.0f;
#pragma unroll 8
    for (int b = F.b0[t]; b < F.b1[t]; ++b) s += F.partial[(int64_t)b * (2 * KGW_C) + threadIdx.x];
    (k ? F.dbias : F.dweight)[t * KGW_C + c] = s;
}

// blocks per job of the backward's grid, as prefix sums over ALL jobs (empty ones take none); returns the grid, or a status < 0
int lnorm_plan(int32_t n_jobs, const KgwLNormBwdJob* jobs, int* bend) {
    if (!jobs) return KGW_E_NULL;
    if (n_jobs < 1 || n_jobs > 8) return KGW_E_RANGE;
    for (int k = 0; k < n_jobs; ++k)
        if (jobs[k].rows < 0 || jobs[k].rows > (1 << 25)) return KGW_E_RANGE;
    for (int64_t per = LN_ROWS_PER_BLOCK;; per *= 2) {
        int64_t total = 0;
        for (int k = 0; k < n_jobs; ++k) {
            total += (jobs[k].rows + per - 1) / per;
            bend[k] = (int)total;
        }
        if (total <= KGW_GRID) return (int)total;
    }
}

int lnorm_check_bwd(int32_t n_jobs, const KgwLNormBwdJob* jobs, int32_t max_type) {
    for (int k = 0; k < n_jobs; ++k) {
        const KgwLNormBwdJob& j = jobs[k];
        if (j.type < 0 || j.type >= max_type) return KGW_E_RANGE;
        for (int i = 0; i < k; ++i)
            if (jobs[i].type == j.type) return KGW_E_RANGE;
        if (j.rows > 0 && (!j.g || !j.y || !j.dy || !j.weight || !j.stat)) return KGW_E_NULL;
        if (j.rows > 1 && (j.ldg < KGW_C || j.ldy < KGW_C || j.lddy < KGW_C || (j.out && j.ldo < KGW_C))) return KGW_E_RANGE;
        if ((((uintptr_t)j.g | (uintptr_t)j.y | (uintptr_t)j.out | (uintptr_t)j.dy | (uintptr_t)j.weight) & 15) ||
            ((uintptr_t)j.stat & 7) || (j.ldg & 3) || (j.ldy & 3) || (j.lddy & 3) || (j.out && (j.ldo & 3)))
            return KGW_E_UNSUPPORTED;
    }
    return KGW_OK;
}
}  // namespace

extern "C" int kgw_layer_norm_relu_fwd(int32_t n_jobs, const KgwLNormJob* jobs, int32_t c_logical, float eps, kgw_stream_t stream_) {
    if (!jobs) return KGW_E_NULL;
    // (a NaN fails the first comparison, an infinity the second)
    if (n_jobs < 1 || n_jobs > 8 || c_logical < 1 || c_logical > KGW_C || !(eps >= 0.0f && eps <= 3.402823466e38f)) return KGW_E_RANGE;
    for (int k = 0; k < n_jobs; ++k) {
        const KgwLNormJob& j = jobs[k];
        if (j.rows < 0 || j.rows > (1 << 25)) return KGW_E_RANGE;
        if (j.rows > 0 && (!j.src || !j.dst || !j.weight || !j.bias || !j.stat)) return KGW_E_NULL;
        if (j.rows > 1 && (j.lds < KGW_C || j.ldd < KGW_C)) return KGW_E_RANGE;
        if ((((uintptr_t)j.src | (uintptr_t)j.dst | (uintptr_t)j.weight | (uintptr_t)j.bias) & 15) || ((uintptr_t)j.stat & 7) ||
            (j.lds & 3) || (j.ldd & 3) || (j.rows > 0 && j.src == j.dst))
            return KGW_E_UNSUPPORTED;
    }
    LNormFwd J;
    J.n = 0; J.c = c_logical; J.cf = (float)c_logical; J.eps = eps; J.total = 0;
    for (int k = 0; k < 8; ++k) { J.end[k] = 0; J.j[k] = KgwLNormJob{nullptr, 0, nullptr, 0, 0, 0, nullptr, nullptr, nullptr}; }
    for (int k = 0; k < n_jobs; ++k) {
        if (jobs[k].rows == 0) continue;
        J.total += jobs[k].rows;
        J.end[J.n] = J.total;
        J.j[J.n++] = jobs[k];
    }
    if (J.total == 0) return KGW_OK;
    int64_t g = (J.total + LN_SLOTS - 1) / LN_SLOTS;
    if (g > KGW_GRID) g = KGW_GRID;
    k_layer_norm_relu_fwd<<<(int)g, KGW_BLK, 0, (hipStream_t)stream_>>>(J);
    KGW_LAUNCH_CHECK();
    return KGW_OK;
}

extern "C" int64_t kgw_layer_norm_partial_floats(int32_t n_jobs, const KgwLNormBwdJob* jobs) {
    int bend[8];
    const int g = lnorm_plan(n_jobs, jobs, bend);
    return g < 0 ? g : (int64_t)g * (2 * KGW_C);
}

extern "C" int kgw_layer_norm_bwd(int32_t n_jobs, const KgwLNormBwdJob* jobs, int32_t c_logical, float* partial,
                                  int64_t partial_floats, kgw_stream_t stream_) {
    int bend[8];
    const int grid = lnorm_plan(n_jobs, jobs, bend);
    if (grid < 0) return grid;
    if (!partial) return KGW_E_NULL;
    if (c_logical < 1 || c_logical > KGW_C || partial_floats < (int64_t)grid * (2 * KGW_C)) return KGW_E_RANGE;
    const int rc = lnorm_check_bwd(n_jobs, jobs, KGW_MAX_TYPES);
    if (rc != KGW_OK) return rc;
    if (grid == 0) return KGW_OK;
    LNormBwd J;
    J.n = 0; J.c = c_logical; J.cf = (float)c_logical; J.inv_c = 1.0f / (float)c_logical; J.partial = partial;
    for (int k = 0; k < 8; ++k) {
        J.bend[k] = 0;
        J.j[k] = KgwLNormBwdJob{nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, 0, 0, nullptr, nullptr};
    }
    for (int k = 0; k < n_jobs; ++k) {
        if (jobs[k].rows == 0) continue;
        J.bend[J.n] = bend[k];
        J.j[J.n++] = jobs[k];
    }
    k_layer_norm_bwd<<<grid, KGW_BLK, 0, (hipStream_t)stream_>>>(J);
    KGW_LAUNCH_CHECK();
    return KGW_OK;
}

extern "C" int kgw_layer_norm_fold(int32_t n_jobs, const KgwLNormBwdJob* jobs, const float* partial, int64_t partial_floats,
                                   int32_t n_types, float* dweight, float* dbias, kgw_stream_t stream_) {
    int bend[8];
    const int grid = lnorm_plan(n_jobs, jobs, bend);
    if (grid < 0) return grid;
    if (!partial || !dweight || !dbias) return KGW_E_NULL;
    if (n_types < 1 || n_types > KGW_MAX_TYPES || partial_floats < (int64_t)grid * (2 * KGW_C)) return KGW_E_RANGE;
    const int rc = lnorm_check_bwd(n_jobs, jobs, n_types);
    if (rc != KGW_OK) return rc;
    LNormFold F;
    F.partial = partial; F.dweight = dweight; F.dbias = dbias;
    for (int t = 0; t < 8; ++t) F.b0[t] = F.b1[t] = 0;
    for (int k = 0; k < n_jobs; ++k) {
        F.b0[jobs[k].type] = k ? bend[k - 1] : 0;
        F.b1[jobs[k].type] = bend[k];
    }
    k_layer_norm_fold<<<n_types, KGW_BLK, 0, (hipStream_t)stream_>>>(F);
    KGW_LAUNCH_CHECK();
    return KGW_OK;
}
