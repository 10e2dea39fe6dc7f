// kgw_dense_hdrop.h -- hidden-state dropout between the message-passing layers (HeteroGNN(gnn_dropout=p)): one element-wise kernel,
// run on the layer outputs Y in the forward and on dY in the backward (the rule: kgwhdrop_keep in include/kgwas_hip.h; the mask is
// recomputed, never stored).  Part of kgw_dense.hip.
#pragma once

namespace {
struct HDropJobs {
    int n;                          // jobs with rows > 0
    int layer;
    uint32_t thresh;
    float scale;
    const uint64_t* word;           // device: the step's 64-bit word, read when the kernel runs
    int64_t total;                  // rows of all jobs
    int64_t end[8];                 // end[j]: rows of jobs 0 .. j
    KgwHDropJob j[8];
};

// One float4 per lane, 32 lanes per row (the aggregate kernels' row mapping): a wavefront takes two rows at a time, the grid
// strides over the rows of all jobs.  Memory-bound: rows x 512 B in, the same out; 4 hashes per lane.  Which elements are kept
// depends on (word, layer, type, row within the job, column) alone -- the grid only decides who computes them.
__global__ void __launch_bounds__(KGW_BLK) k_hidden_dropout(HDropJobs J) {
    const int c4 = threadIdx.x & 31;
    const int64_t stride = (int64_t)gridDim.x * (KGW_BLK / 32);
    const uint32_t lbase = kgwfan_step(kgwdrop_base(*J.word, J.layer), KGW_HDROP_TAG);
    for (int64_t r = (int64_t)blockIdx.x * (KGW_BLK / 32) + (threadIdx.x >> 5); r < J.total; r += stride) {
        int q = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) q += (k < J.n - 1 && r >= J.end[k]) ? 1 : 0;
        const KgwHDropJob& jb = J.j[q];
        const uint32_t row = (uint32_t)(r - (q ? J.end[q - 1] : 0));
        const uint32_t base = kgwfan_step(lbase, (uint32_t)jb.type);
        const float4 y = ((const float4*)(jb.src + (int64_t)row * jb.lds))[c4];
        const uint32_t col = 4u * (uint32_t)c4;
        float4 o;
        o.x = kgwhdrop_keep(base, row, col, J.thresh) ? y.x * J.scale : 0.0f;
        o.y = kgwhdrop_keep(base, row, col + 1u, J.thresh) ? y.y * J.scale : 0.0f;
        o.z = kgwhdrop_keep(base, row, col + 2u, J.thresh) ? y.z * J.scale : 0.0f;
        o.w = kgwhdrop_keep(base, row, col + 3u, J.thresh) ? y.w * J.scale : 0.0f;
        ((float4*)(jb.dst + (int64_t)row * jb.ldd))[c4] = o;
    }
}
}  // namespace

extern "C" int kgw_hidden_dropout(int32_t n_jobs, const KgwHDropJob* jobs, int32_t layer, const uint64_t* word_dev, uint32_t thresh,
                                  float scale, kgw_stream_t stream_) {
    if (!jobs || !word_dev) return KGW_E_NULL;
    // (a NaN fails the first comparison, an infinity the second)
    if (n_jobs < 1 || n_jobs > 8 || layer < 1 || !(scale >= 1.0f && scale <= 3.402823466e38f)) return KGW_E_RANGE;
    for (int k = 0; k < n_jobs; ++k) {
        const KgwHDropJob& j = jobs[k];
        if (j.rows < 0 || j.rows > (1 << 25)) return KGW_E_RANGE;
        if (j.rows > 0 && (!j.src || !j.dst)) return KGW_E_NULL;
        if (j.rows > 1 && (j.lds < KGW_C || j.ldd < KGW_C)) return KGW_E_RANGE;
        if ((((uintptr_t)j.src | (uintptr_t)j.dst) & 15) || (j.lds & 3) || (j.ldd & 3)) return KGW_E_UNSUPPORTED;
    }
    HDropJobs J;
    J.n = 0; J.layer = layer; J.thresh = thresh; J.scale = scale; J.word = word_dev; J.total = 0;
    for (int k = 0; k < 8; ++k) { J.end[k] = 0; J.j[k] = KgwHDropJob{nullptr, 0, nullptr, 0, 0, 0}; }
    for (int k = 0; k < n_jobs; ++k) {
        if (jobs[k].rows == 0) continue;
        J.total += jobs[k].rows;
        J.end[J.n] = J.total;
        J.j[J.n++] = jobs[k];
    }
    if (J.total == 0) return KGW_OK;
    // (8 rows per block; at most 8 blocks of 256 threads per CU on 256 CUs, the stride takes the rest)
    int64_t g = (J.total + KGW_BLK / 32 - 1) / (KGW_BLK / 32);
    if (g > KGW_GRID) g = KGW_GRID;
    k_hidden_dropout<<<(int)g, KGW_BLK, 0, (hipStream_t)stream_>>>(J);
    KGW_LAUNCH_CHECK();
    return KGW_OK;
}
