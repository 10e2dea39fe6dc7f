// kgw_edge_attr.h -- edge attributes (GATConv edge_dim, include/kgwas_hip.h: KgwEdgeAttr): the per-edge logit term
//      t_e = sum_{d < D} A_r[p(e)][d] w_r[d]
// of one layer and the gradient of w_r.  Included by kgw_aggregate.hip inside its namespace (KgwChunk, load_chunk, KGW_BLK).
//
// Traffic per edge: 4 D bytes of attributes in, 4 bytes of term out (k_edge_term); the forward aggregate reads the term beside
// col_local; the backward reads d pre_e in place from adp (8-byte stride) and the 4 D bytes again.  Nothing here is on the 512
// bytes per edge of the row gather.
#pragma once

struct EdgeTab {
    int64_t col_off[KGW_MAX_RELS];     // KgwGraph.col_off
    int64_t attr_off[KGW_MAX_RELS];    // first attribute row of the relation, -1 = none
    int32_t live[KGW_MAX_RELS];        // the layer computes the relation
    int32_t n_rels, dim;
};

// position of the chunk's first edge inside g_col; negative for the chunks of a drawn segment (finite fan-out)
__device__ __forceinline__ int64_t eattr_gpos(const KgwChunk& c) { return ((int64_t)c.gpos_hi << 32) | (uint32_t)c.gpos_lo; }

// one wavefront per chunk, one lane per edge
__global__ void __launch_bounds__(KGW_BLK) k_edge_term(EdgeTab E, const KgwChunk* __restrict__ chunks,
                                                       const KgwBatchMeta* __restrict__ meta, int layer,
                                                       const float* __restrict__ attr, const float* __restrict__ w,
                                                       float* __restrict__ term) {
    const int lane = kgw_lane();
    const int nw = gridDim.x * 4;
    const int n_chunks = meta->n_chunks[layer - 1];
    for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n_chunks; c += nw) {
        const KgwChunk ck = load_chunk(chunks, c);
        const int r = ck.rel;
        const int n = ck.e1 - ck.e0;
        const int64_t a0 = E.attr_off[r];
        if (!E.live[r] || a0 < 0) { for (int t = lane; t < n; t += 64) term[ck.e0 + t] = 0.0f; continue; }
        if (ck.gpos_hi < 0) {          // a drawn segment: its entries' positions are not recorded
            for (int t = lane; t < n; t += 64) term[ck.e0 + t] = __builtin_nanf("");
            continue;
        }
        float wv[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) wv[d] = d < E.dim ? w[r * 8 + d] : 0.f;
        const int64_t row0 = a0 + (eattr_gpos(ck) - E.col_off[r]);
        for (int t = lane; t < n; t += 64) {
            const float* __restrict__ ar = attr + (row0 + t) * E.dim;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < 8; ++d)
                if (d < E.dim) s = fmaf(ar[d], wv[d], s);
            term[ck.e0 + t] = s;
        }
    }
}

// level 1 of d w_r: part[c][d] = sum over the chunk's edges of d_term_e A[p(e)][d].  A lane adds its edges in ascending order,
// the lanes are added by a fixed butterfly.  Only the chunks of live attributed relations are written (the fold reads no others).
__global__ void __launch_bounds__(KGW_BLK) k_edge_term_bwd(EdgeTab E, const KgwChunk* __restrict__ chunks,
                                                           const KgwBatchMeta* __restrict__ meta, int layer,
                                                           const float* __restrict__ attr, const float* __restrict__ d_term,
                                                           int64_t stride, float* __restrict__ part) {
    const int lane = kgw_lane();
    const int nw = gridDim.x * 4;
    const int n_chunks = meta->n_chunks[layer - 1];
    for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n_chunks; c += nw) {
        const KgwChunk ck = load_chunk(chunks, c);
        const int r = ck.rel;
        const int64_t a0 = E.attr_off[r];
        if (!E.live[r] || a0 < 0) continue;
        const int n = ck.e1 - ck.e0;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (ck.gpos_hi < 0) {
#pragma unroll
            for (int d = 0; d < 8; ++d) acc[d] = __builtin_nanf("");
        } else {
            const int64_t row0 = a0 + (eattr_gpos(ck) - E.col_off[r]);
            for (int t = lane; t < n; t += 64) {
                const float g = d_term[(int64_t)(ck.e0 + t) * stride];
                const float* __restrict__ ar = attr + (row0 + t) * E.dim;
#pragma unroll
                for (int d = 0; d < 8; ++d)
                    if (d < E.dim) acc[d] = fmaf(g, ar[d], acc[d]);
            }
#pragma unroll
            for (int d = 0; d < 8; ++d)
                for (int o = 32; o > 0; o >>= 1) acc[d] += __shfl_xor(acc[d], o, 64);
        }
        if (lane == 0) {
            float* p = part + (int64_t)c * 8;
#pragma unroll
            for (int d = 0; d < 8; ++d) p[d] = acc[d];
        }
    }
}

// level 2: one block per relation over the relation's chunks (contiguous per destination hop, as the d u_r riders walk them):
// thread (g = tid / 8, d = tid % 8) adds chunks g, g + 32, ... in order, then a fixed tree over the 32 groups
__global__ void __launch_bounds__(KGW_BLK) k_edge_term_bwd_fold(EdgeTab E, const KgwBatchMeta* __restrict__ meta,
                                                                const int32_t* __restrict__ seg_chptr, int n_hops,
                                                                const float* __restrict__ part, float* __restrict__ d_w) {
    __shared__ float sm[KGW_BLK];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int d = tid & 7, g = tid >> 3;
    float s = 0.f;
    if (E.live[r] && E.attr_off[r] >= 0) {
        for (int h = 0; h < n_hops; ++h) {
            const int c0 = seg_chptr[meta->seg_off[h][r]];
            const int c1 = (r + 1 < E.n_rels) ? seg_chptr[meta->seg_off[h][r + 1]] : meta->chunk_end[h];
            for (int c = c0 + g; c < c1; c += 32) s += part[(int64_t)c * 8 + d];
        }
    }
    sm[tid] = s;
    __syncthreads();
    for (int o = KGW_BLK / 2; o >= 8; o >>= 1) {
        if (tid < o) sm[tid] += sm[tid + o];
        __syncthreads();
    }
    if (tid < 8) d_w[r * 8 + tid] = sm[tid];
}
