// kgw_dense_root.h -- the root weight of a message-passing layer (HeteroGNN(gnn_root_weight=True)): dst = act(y + x W^T) for the
// destination rows of every node type of a layer in one launch, and its backward dx = gm W (the rule: kgwroot_* in
// include/kgwas_hip.h).  Part of kgw_dense.hip.
#pragma once

namespace {
constexpr int ROOT_TILES_PER_BLOCK = 2;     // 32-row tiles a block takes before the grid cap doubles it

// one job of either direction: acc = A_rows * Wop, then the epilogue
struct RootJ {
    const float* a; int64_t lda;    // MFMA operand rows: x (forward) / g (backward)
    const float* m; int64_t ldm;    // backward: mask the operand by (m > 0), or null
    const float* e; int64_t lde;    // epilogue operand: y, added (forward) / x, dx *= (x > 0) (backward, or null)
    float* o; int64_t ldo;          // dst / dx
    float* gm; int64_t ldgm;        // backward: the masked operand, or null
    const float* W;
    int rows;
};

struct RootArgs {
    int n;                          // jobs with rows > 0
    int relu;
    int bend[8];                    // bend[j]: blocks of jobs 0 .. j
    RootJ j[8];
};

// k_linear_wreg_half's mapping with the tile loop of a weight-stationary kernel: the blocks [bend[q - 1], bend[q]) belong to job q;
// a block stages W_q in LDS once (k contiguous per output column; the backward stages W^T), wavefront w keeps the 64 output columns
// of half (w & 1) in 128 registers and takes the tiles (block - b0) * 2 + (w >> 1) + 2 nb i.  Lane (li, lk) supplies row li of the
// tile and the k of half lk; an output element is the sum over k in the MFMA's own order, whichever block computes it.
template <bool BWD>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) k_root_linear(RootArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Wl = lds;                                         // [128 n][WST]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lk = lane >> 5;
    int q = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) q += (k < A.n - 1 && (int)blockIdx.x >= A.bend[k]) ? 1 : 0;
    const RootJ& jb = A.j[q];
    const int b0 = q ? A.bend[q - 1] : 0;
    const int64_t tstride = (int64_t)(A.bend[q] - b0) * 2;
    {   // stage W: all 16 loads of a thread in flight before the first LDS write
        f32x4 wv[16];
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int idx = tid + 256 * it;
            if (!BWD) wv[it] = *(const f32x4*)(jb.W + (idx >> 5) * KGW_C + (idx & 31) * 4);
            else wv[it] = *(const f32x4*)(jb.W + (idx & 127) * KGW_C + (idx >> 7) * 4);
        }
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int idx = tid + 256 * it;
            if (!BWD) {
                *(f32x4*)(Wl + (idx >> 5) * WST + (idx & 31) * 4) = wv[it];
            } else {
                const int k = idx & 127, n4 = (idx >> 7) * 4;
                Wl[(n4 + 0) * WST + k] = wv[it].x; Wl[(n4 + 1) * WST + k] = wv[it].y;
                Wl[(n4 + 2) * WST + k] = wv[it].z; Wl[(n4 + 3) * WST + k] = wv[it].w;
            }
        }
    }
    __syncthreads();
    const int t0 = (wave & 1) * 2;                           // this wavefront's two 32-column blocks
    f32x4 bw[2][16];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int qq = 0; qq < 16; ++qq) bw[t][qq] = *(const f32x4*)(Wl + ((t0 + t) * 32 + li) * WST + lk * 64 + 4 * qq);
    const int64_t ntiles = ((int64_t)jb.rows + 31) / 32;
    for (int64_t tile = (int64_t)((int)blockIdx.x - b0) * 2 + (wave >> 1); tile < ntiles; tile += tstride) {
        const int64_t row = tile * 32 + li;
        const bool live = row < jb.rows;
        const int64_t rc = live ? row : (int64_t)jb.rows - 1;
        f32x4 xa[16];
        {
            const float* xp = jb.a + rc * jb.lda + lk * 64;
#pragma unroll
            for (int qq = 0; qq < 16; ++qq) xa[qq] = *(const f32x4*)(xp + 4 * qq);
        }
        if (BWD && jb.m) {
            const float* mp = jb.m + rc * jb.ldm + lk * 64;
#pragma unroll
            for (int qq = 0; qq < 16; ++qq) {
                const f32x4 o = *(const f32x4*)(mp + 4 * qq);
                xa[qq].x = kgwroot_mask(xa[qq].x, o.x); xa[qq].y = kgwroot_mask(xa[qq].y, o.y);
                xa[qq].z = kgwroot_mask(xa[qq].z, o.z); xa[qq].w = kgwroot_mask(xa[qq].w, o.w);
            }
            if (jb.gm && t0 == 0 && live) {                  // (both column halves hold the row: one of them writes it)
                float* gp = jb.gm + row * jb.ldgm + lk * 64;
#pragma unroll
                for (int qq = 0; qq < 16; ++qq) *(f32x4*)(gp + 4 * qq) = xa[qq];
            }
        }
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
#pragma unroll
        for (int qq = 0; qq < 16; ++qq) {
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bw[t][qq].x, xa[qq].x, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bw[t][qq].y, xa[qq].y, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bw[t][qq].z, xa[qq].z, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bw[t][qq].w, xa[qq].w, acc[t], 0, 0, 0);
        }
        if (live) {
            float* op = jb.o + row * jb.ldo + 4 * lk;
            const float* ep = jb.e ? jb.e + row * jb.lde + 4 * lk : nullptr;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = (t0 + t) * 32 + 8 * g;
                    f32x4 v;
                    if (!BWD) {
                        const f32x4 y4 = *(const f32x4*)(ep + c);
                        v.x = kgwroot_out(y4.x, acc[t][4 * g + 0], A.relu); v.y = kgwroot_out(y4.y, acc[t][4 * g + 1], A.relu);
                        v.z = kgwroot_out(y4.z, acc[t][4 * g + 2], A.relu); v.w = kgwroot_out(y4.w, acc[t][4 * g + 3], A.relu);
                    } else {
                        v.x = acc[t][4 * g + 0]; v.y = acc[t][4 * g + 1]; v.z = acc[t][4 * g + 2]; v.w = acc[t][4 * g + 3];
                        if (ep) {
                            const f32x4 x4 = *(const f32x4*)(ep + c);
                            v.x = kgwroot_mask(v.x, x4.x); v.y = kgwroot_mask(v.y, x4.y);
                            v.z = kgwroot_mask(v.z, x4.z); v.w = kgwroot_mask(v.w, x4.w);
                        }
                    }
                    *(f32x4*)(op + c) = v;
                }
            }
        }
    }
}

// blocks per job as prefix sums over the LIVE jobs of ``rows`` (in order); returns the grid
int root_plan(int n, const int* rows, int* bend) {
    for (int64_t per = ROOT_TILES_PER_BLOCK;; per *= 2) {
        int64_t total = 0;
        for (int k = 0; k < n; ++k) {
            const int64_t tiles = ((int64_t)rows[k] + 31) / 32;
            total += (tiles + per - 1) / per;
            bend[k] = (int)total;
        }
        if (total <= KGW_GRID) return (int)total;
    }
}

template <bool BWD>
int root_launch(RootArgs& A, hipStream_t st) {
    if (A.n == 0) return KGW_OK;
    int rows[8];
    for (int k = 0; k < A.n; ++k) rows[k] = A.j[k].rows;
    const int grid = root_plan(A.n, rows, A.bend);
    const size_t lds = (size_t)(128 * WST) * sizeof(float);
    static KgwPerDevice attr_once;
    if (attr_once.need())
        KGW_HIP(hipFuncSetAttribute((const void*)k_root_linear<BWD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    k_root_linear<BWD><<<grid, 256, lds, st>>>(A);
    KGW_LAUNCH_CHECK();
    return KGW_OK;
}

inline bool root_mis16(const void* p) { return ((uintptr_t)p & 15) != 0; }
}  // namespace

extern "C" int kgw_root_linear_fwd(int32_t n_jobs, const KgwRootJob* jobs, int32_t relu, kgw_stream_t stream_) {
    if (!jobs) return KGW_E_NULL;
    if (n_jobs < 1 || n_jobs > 8) return KGW_E_RANGE;
    for (int k = 0; k < n_jobs; ++k) {
        const KgwRootJob& j = jobs[k];
        if (j.rows < 0 || j.rows > (1 << 25) || j.type < 0 || j.type >= KGW_MAX_TYPES) return KGW_E_RANGE;
        for (int i = 0; i < k; ++i)
            if (jobs[i].type == j.type) return KGW_E_RANGE;
        if (j.rows > 0 && (!j.x || !j.y || !j.dst || !j.W)) return KGW_E_NULL;
        if (j.rows > 1 && (j.ldx < KGW_C || j.ldy < KGW_C || j.ldd < KGW_C)) return KGW_E_RANGE;
        if (root_mis16(j.x) || root_mis16(j.y) || root_mis16(j.dst) || root_mis16(j.W) || (j.ldx & 3) || (j.ldy & 3) || (j.ldd & 3) ||
            (j.rows > 0 && (j.dst == j.y || j.dst == j.x)))
            return KGW_E_UNSUPPORTED;
    }
    RootArgs A;
    A.n = 0; A.relu = relu ? 1 : 0;
    for (int k = 0; k < 8; ++k) {
        A.bend[k] = 0;
        A.j[k] = RootJ{nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0};
    }
    for (int k = 0; k < n_jobs; ++k) {
        const KgwRootJob& j = jobs[k];
        if (j.rows == 0) continue;
        A.j[A.n++] = RootJ{j.x, j.ldx, nullptr, 0, j.y, j.ldy, j.dst, j.ldd, nullptr, 0, j.W, j.rows};
    }
    return root_launch<false>(A, (hipStream_t)stream_);
}

extern "C" int kgw_root_linear_bwd(int32_t n_jobs, const KgwRootBwdJob* jobs, kgw_stream_t stream_) {
    if (!jobs) return KGW_E_NULL;
    if (n_jobs < 1 || n_jobs > 8) return KGW_E_RANGE;
    for (int k = 0; k < n_jobs; ++k) {
        const KgwRootBwdJob& j = jobs[k];
        if (j.rows < 0 || j.rows > (1 << 25) || j.type < 0 || j.type >= KGW_MAX_TYPES) return KGW_E_RANGE;
        for (int i = 0; i < k; ++i)
            if (jobs[i].type == j.type) return KGW_E_RANGE;
        if (j.rows > 0 && (!j.g || !j.dx || !j.W || (j.x_premasked && !j.x))) return KGW_E_NULL;
        if (j.rows > 1 && (j.ldg < KGW_C || j.lddx < KGW_C || (j.out && j.ldo < KGW_C) || (j.x_premasked && j.ldx < KGW_C) ||
                           (j.gm && j.ldgm < KGW_C)))
            return KGW_E_RANGE;
        if (root_mis16(j.g) || root_mis16(j.out) || root_mis16(j.dx) || root_mis16(j.W) || root_mis16(j.gm) ||
            (j.x_premasked && root_mis16(j.x)) || (j.ldg & 3) || (j.lddx & 3) || (j.out && (j.ldo & 3)) ||
            (j.x_premasked && (j.ldx & 3)) || (j.gm && (j.ldgm & 3)) ||
            // (an output that IS an input: the two column halves of a tile read whole rows of g / out while the other stores)
            (j.rows > 0 && ((const float*)j.dx == j.g || (const float*)j.gm == j.g || (const float*)j.dx == j.out ||
                            (j.gm && ((const float*)j.gm == j.out || j.gm == j.dx)) ||
                            (j.x_premasked && ((const float*)j.dx == j.x || (const float*)j.gm == j.x)))))
            return KGW_E_UNSUPPORTED;
    }
    RootArgs A;
    A.n = 0; A.relu = 0;
    for (int k = 0; k < 8; ++k) {
        A.bend[k] = 0;
        A.j[k] = RootJ{nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0};
    }
    for (int k = 0; k < n_jobs; ++k) {
        const KgwRootBwdJob& j = jobs[k];
        if (j.rows == 0) continue;
        A.j[A.n++] = RootJ{j.g, j.ldg, j.out, j.ldo, j.x_premasked ? j.x : nullptr, j.ldx, j.dx, j.lddx, j.out ? j.gm : nullptr,
                           j.ldgm, j.W, j.rows};
    }
    return root_launch<true>(A, (hipStream_t)stream_);
}
