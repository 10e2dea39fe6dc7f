// kgw_aggregate_heads.h -- the attention aggregate with NH = 2 or 4 heads (KgwLayerArgs.n_heads), included by kgw_aggregate.hip
// inside its anonymous namespace, after the single-head kernels whose helpers it reuses.
//
// Every head-carrying array is NH planes of today's layout (include/kgwas_hip.h).  The aggregate gathers the layer INPUT and the
// caller applies W_src afterwards, so all heads of an edge share the one 512-byte row: the mapping is the single-head kernels' --
// one wavefront per chunk, a 32-lane half per edge, one float4 per lane, groups of 8 with kgw_half_reduce8 -- and each gathered
// row x[p] is loaded ONCE and used for the NH dot products.  What grows with NH is per-row state: (m, s, acc) in the forward,
// (dz, cdot, M, 1/den) and the d u_r accumulators in the dst-major backward.  The chunks are not software-pipelined here (PIPE of
// the single-head kernels): the registers go to the heads.  No atomics; every sum has one fixed order, so reruns give the same bits.
#pragma once

// heads per launch of the dst-major backward (k_agg_bwd_dst_heads<NH, HB>, HB = min(NH, this)): 4 = one pass for every NH
#ifndef KGW_BWD_DST_HEADS_PER_PASS
#define KGW_BWD_DST_HEADS_PER_PASS 4
#endif

struct HeadDims {
    int64_t z_rows;       // rows per plane of Z / dZ / stat / da_dst   (meta_host->z_base[layer - 1][n_types])
    int64_t n_edges;      // entries per plane of e_edge / adp          (meta_host->n_edges[layer - 1])
    int64_t n_chunks;     // records per plane of part / part_da / part_du  (KgwLayerArgs.n_chunks)
};

template <int G>
__device__ __forceinline__ void grp_load(const float4* __restrict__ Hb4, int colv, int q0, int hn, int nb, int half, int hl,
                                         float4 (&x)[G], bool (&valid)[G]) {
#pragma unroll
    for (int p = 0; p < G; ++p) {
        const int q = q0 + p, i = half * hn + q;
        valid[p] = (q < hn) && (i < nb);
        const int cj = __shfl(colv, valid[p] ? i : 0, 64);
        x[p] = Hb4[(int64_t)cj * 32 + hl];
    }
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// the row tails (4 or 2 edges per half) of fwd_group, on rows already in registers
template <int G>
__device__ __forceinline__ void fwd_tail_compute(const float4 (&x)[G], const bool (&valid)[G], int q0, int hl, const float4& u4,
                                                 float ad, float slope, float inv_temp, float& m, float& s, float4& acc, float& ev) {
    float t[G];
    float mb = -INFINITY;
#pragma unroll
    for (int p = 0; p < G; ++p) {
        float d = kgw_half_allsum(dot4(x[p], u4)) + ad;
        d = d > 0.f ? d : d * slope;
        ev = (hl == q0 + p) ? d : ev;              // lane (half, hl) keeps the logit of edge half*hn+hl
        t[p] = valid[p] ? d * inv_temp : -INFINITY;
        mb = fmaxf(mb, t[p]);
    }
    const float mn = fmaxf(m, mb);
    const float sc = __expf(m - mn);
    s *= sc; scale4(acc, sc); m = mn;
#pragma unroll
    for (int p = 0; p < G; ++p) {
        const float w = __expf(t[p] - mn);
        s += w;
        fma4(acc, w, x[p]);
    }
}

template <int NH>
__global__ void __launch_bounds__(KGW_BLK) k_agg_fwd_heads(LayerTab T, AggPtrs P, HeadDims Dm, float slope, float inv_temp) {
    const int lane = kgw_lane(), half = lane >> 5, hl = lane & 31;
    const int nw = gridDim.x * 4;
    const DropCtx D = {0u, 0u, 1.0f};
    const int n_items = P.meta->n_chunks[P.layer - 1];
    const int64_t NRC = (int64_t)T.n_rels * KGW_C;
    for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n_items; c += nw) {
        const KgwChunk ck = load_chunk(P.chunks, c);
        const int r = ck.rel;
        if (!T.live[r]) continue;
        const int zrow = T.z0[r] + ck.row * T.zstride[r];
        const float4 hd4 = ((const float4*)(P.H + ((int64_t)T.dst_hbase[r] + ck.row) * KGW_C))[hl];
        float ad[NH], m[NH], s[NH];
        float4 u4[NH], acc[NH];
#pragma unroll
        for (int h = 0; h < NH; ++h) {          // a_d^h = <h_dst[row], v_r^h>, both halves compute it
            const float4 v4 = ((const float4*)(P.V + h * NRC + (int64_t)r * KGW_C))[hl];
            ad[h] = kgw_half_allsum(dot4(hd4, v4));
            u4[h] = ((const float4*)(P.U + h * NRC + (int64_t)r * KGW_C))[hl];
            m[h] = NEG_BIG; s[h] = 0.f;
            acc[h] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float4* Hb4 = (const float4*)(P.H + (int64_t)T.src_base[r] * KGW_C);
        const int n = ck.e1 - ck.e0;
        for (int b = 0; b < n; b += 64) {
            const int nb = min(64, n - b);
            const int hn = (nb + 1) >> 1;
            const int colv = (lane < nb) ? P.col_local[ck.e0 + b + lane] : 0;
            float ev[NH];
#pragma unroll
            for (int h = 0; h < NH; ++h) ev[h] = 0.f;
            for (int q0 = 0; q0 < hn;) {
                const int rem = hn - q0;
                if (rem > 4) {
                    float4 x[8];
                    grp8_load(Hb4, colv, q0, hn, nb, half, hl, x);
#pragma unroll
                    for (int h = 0; h < NH; ++h)
                        fwd_grp8_compute<false, false>(x, q0, hn, nb, half, hl, u4[h], ad[h], slope, inv_temp, m[h], s[h], acc[h], ev[h], D, 0);
                    q0 += 8;
                } else if (rem > 2) {
                    float4 x[4];
                    bool valid[4];
                    grp_load<4>(Hb4, colv, q0, hn, nb, half, hl, x, valid);
#pragma unroll
                    for (int h = 0; h < NH; ++h)
                        fwd_tail_compute<4>(x, valid, q0, hl, u4[h], ad[h], slope, inv_temp, m[h], s[h], acc[h], ev[h]);
                    q0 += 4;
                } else {
                    float4 x[2];
                    bool valid[2];
                    grp_load<2>(Hb4, colv, q0, hn, nb, half, hl, x, valid);
#pragma unroll
                    for (int h = 0; h < NH; ++h)
                        fwd_tail_compute<2>(x, valid, q0, hl, u4[h], ad[h], slope, inv_temp, m[h], s[h], acc[h], ev[h]);
                    q0 += 2;
                }
            }
            const int i = half * hn + hl;
            if (hl < hn && i < nb) {
#pragma unroll
                for (int h = 0; h < NH; ++h) P.e_edge[h * Dm.n_edges + ck.e0 + b + i] = ev[h];
            }
        }
        // merge the two half-wave states, head by head
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const float mo = kgw_xhalf(m[h]);
            const float M = fmaxf(m[h], mo);
            const float f = __expf(m[h] - M);
            float sh = s[h] * f;
            float4 a = acc[h];
            scale4(a, f);
            const float S = sh + kgw_xhalf(sh);
            a.x += kgw_xhalf(a.x); a.y += kgw_xhalf(a.y);
            a.z += kgw_xhalf(a.z); a.w += kgw_xhalf(a.w);
            if (ck.nch == 1) {
                const float den = S + 1e-16f;
                const float inv = 1.0f / den;
                const int64_t zr = h * Dm.z_rows + zrow;
                if (half == 0) {
                    scale4(a, inv);
                    ((float4*)(P.Z + zr * KGW_C))[hl] = a;
                }
                if (lane == 0) { P.stat[2 * zr] = M; P.stat[2 * zr + 1] = den; }
            } else {
                float* pr = P.part + (h * Dm.n_chunks + c) * PART_STRIDE;
                if (half == 0) ((float4*)(pr + 4))[hl] = a;
                if (lane == 0) { pr[0] = M; pr[1] = S; }
            }
        }
    }
}

// one wavefront per multi-chunk segment and head: merge partial (max, sum, acc), chunk order
template <int NH>
__global__ void __launch_bounds__(KGW_BLK) k_agg_fwd_combine_heads(LayerTab T, AggPtrs P, HeadDims Dm, int n_hops) {
  for (int hop = 0; hop < n_hops; ++hop) {
    const int lane = kgw_lane();
    const int nw = gridDim.x * 4;
    const int n_multi = P.meta->multi_cnt[hop];
    const int32_t* mm = P.multi + (int64_t)hop * P.multi_cap * 4;
    for (int kh = blockIdx.x * 4 + (threadIdx.x >> 6); kh < n_multi * NH; kh += nw) {
        const int k = kh / NH, h = kh % NH;
        const int first = mm[4 * k], nch = mm[4 * k + 1], row = mm[4 * k + 2], r = mm[4 * k + 3];
        if (!T.live[r]) continue;
        const int64_t zr = h * Dm.z_rows + T.z0[r] + row * T.zstride[r];
        const float* part = P.part + h * Dm.n_chunks * PART_STRIDE;
        float mx = NEG_BIG;
        for (int c = lane; c < nch; c += 64) mx = fmaxf(mx, part[(int64_t)(first + c) * PART_STRIDE]);
        const float M = wave_allmax(mx);
        float S = 0.f;
        float2 acc = make_float2(0.f, 0.f);
        for (int c = 0; c < nch; ++c) {
            const float* pr = part + (int64_t)(first + c) * PART_STRIDE;
            const float f = __expf(pr[0] - M);
            S = fmaf(pr[1], f, S);
            const float2 a = ((const float2*)(pr + 4))[lane];
            acc.x = fmaf(a.x, f, acc.x); acc.y = fmaf(a.y, f, acc.y);
        }
        const float den = S + 1e-16f, inv = 1.0f / den;
        ((float2*)(P.Z + zr * KGW_C))[lane] = make_float2(acc.x * inv, acc.y * inv);
        if (lane == 0) { P.stat[2 * zr] = M; P.stat[2 * zr + 1] = den; }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward, dst-major pass
// ------------------------------------------------------------------------------------------------
// the sums one head keeps per chunk: d a_dst = D0 - (E / S) B (see k_agg_bwd_dst), `own` = the part from the edges taken 8 at a
// time (one copy per edge in the first 8-lane group of a half), the rest from the row tails (every lane holds every edge)
struct HeadSums {
    float dsum, esum, bsum, ssum, dsum_own, esum_own, bsum_own, ssum_own;
};

template <int G>
__device__ __forceinline__ void bwd_tail_compute(const float4 (&x)[G], const bool (&valid)[G], float evin, int q0, int half, int hl,
                                                 const float4& dz4, float cdot, float M, float inv_den, float slope, float inv_temp,
                                                 float& av, float& dv, float4& ua, HeadSums& S) {
#pragma unroll
    for (int p = 0; p < G; ++p) {
        const int q = q0 + p;
        const float e = __shfl(evin, half * 32 + (q & 31), 64);   // logit kept by lane (half, q)
        const float t = valid[p] ? e : -INFINITY;
        const float dalpha = kgw_half_allsum(dot4(x[p], dz4));
        const float alpha = __expf(t * inv_temp - M) * inv_den;
        const float dlogit = alpha * (dalpha - cdot);
        const float sfac = inv_temp * (t > 0.f ? 1.0f : slope);
        const float dpre = dlogit * sfac;
        av = (hl == q) ? alpha : av;
        dv = (hl == q) ? dpre : dv;
        S.dsum += dpre; S.esum += dlogit; S.bsum += alpha * sfac; S.ssum += alpha;
        fma4(ua, dpre, x[p]);
    }
}

// HB heads of the NH per launch (head h0 + k, k < HB): NH = 4 may run as two passes of two heads should one pass of four not
// fit the register file without scratch (profiles/multihead/resource_usage.txt says which the host selects)
template <int NH, int HB>
__global__ void __launch_bounds__(KGW_BLK) k_agg_bwd_dst_heads(LayerTab T, AggPtrs P, HeadDims Dm, int h0, float slope, float inv_temp) {
    const int lane = kgw_lane(), half = lane >> 5, hl = lane & 31;
    const int nw = gridDim.x * 4;
    const DropCtx D = {0u, 0u, 1.0f};
    const int n_items = P.meta->n_chunks[P.layer - 1];
    for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n_items; c += nw) {
        const KgwChunk ck = load_chunk(P.chunks, c);
        const int r = ck.rel;
        if (!T.live[r]) continue;
        const int zrow = T.z0[r] + ck.row * T.zstride[r];
        float4 dz4[HB], ua[HB];
        float cdot[HB], M[HB], inv_den[HB];
        HeadSums S[HB];
#pragma unroll
        for (int k = 0; k < HB; ++k) {
            const int64_t zr = (h0 + k) * Dm.z_rows + zrow;
            dz4[k] = ((const float4*)(P.dZ + zr * KGW_C))[hl];
            const float4 z4 = ((const float4*)(P.Z + zr * KGW_C))[hl];
            cdot[k] = kgw_half_allsum(dot4(dz4[k], z4));          // <dz_i, z_i> of the head, from the stored aggregate
            M[k] = P.stat[2 * zr];
            inv_den[k] = 1.0f / P.stat[2 * zr + 1];
            ua[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            S[k] = HeadSums{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        }
        const float4* Hb4 = (const float4*)(P.H + (int64_t)T.src_base[r] * KGW_C);
        const int n = ck.e1 - ck.e0;
        for (int b = 0; b < n; b += 64) {
            const int nb = min(64, n - b);
            const int hn = (nb + 1) >> 1;
            const int i = half * hn + hl;
            const bool mine = (hl < hn) && (i < nb);
            const int colv = (lane < nb) ? P.col_local[ck.e0 + b + lane] : 0;
            float evin[HB], av[HB], dv[HB];
#pragma unroll
            for (int k = 0; k < HB; ++k) {
                evin[k] = mine ? P.e_edge[(h0 + k) * Dm.n_edges + ck.e0 + b + i] : 0.f;
                av[k] = 0.f; dv[k] = 0.f;
            }
            for (int q0 = 0; q0 < hn;) {
                const int rem = hn - q0;
                if (rem > 4) {
                    float4 x[8];
                    grp8_load(Hb4, colv, q0, hn, nb, half, hl, x);
#pragma unroll
                    for (int k = 0; k < HB; ++k)
                        bwd_grp8_compute<false>(x, evin[k], q0, hn, nb, half, hl, dz4[k], cdot[k], M[k], inv_den[k], slope, inv_temp,
                                                av[k], dv[k], S[k].dsum_own, ua[k], S[k].esum_own, S[k].bsum_own, S[k].ssum_own, D, 0);
                    q0 += 8;
                } else if (rem > 2) {
                    float4 x[4];
                    bool valid[4];
                    grp_load<4>(Hb4, colv, q0, hn, nb, half, hl, x, valid);
#pragma unroll
                    for (int k = 0; k < HB; ++k)
                        bwd_tail_compute<4>(x, valid, evin[k], q0, half, hl, dz4[k], cdot[k], M[k], inv_den[k], slope, inv_temp,
                                            av[k], dv[k], ua[k], S[k]);
                    q0 += 4;
                } else {
                    float4 x[2];
                    bool valid[2];
                    grp_load<2>(Hb4, colv, q0, hn, nb, half, hl, x, valid);
#pragma unroll
                    for (int k = 0; k < HB; ++k)
                        bwd_tail_compute<2>(x, valid, evin[k], q0, half, hl, dz4[k], cdot[k], M[k], inv_den[k], slope, inv_temp,
                                            av[k], dv[k], ua[k], S[k]);
                    q0 += 2;
                }
            }
            if (mine) {
#pragma unroll
                for (int k = 0; k < HB; ++k) ((float2*)P.adp)[(h0 + k) * Dm.n_edges + ck.e0 + b + i] = make_float2(av[k], dv[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < HB; ++k) {
            const int64_t hc = (h0 + k) * Dm.n_chunks + c;
            float4 u = ua[k];
            u.x += kgw_xhalf(u.x); u.y += kgw_xhalf(u.y); u.z += kgw_xhalf(u.z); u.w += kgw_xhalf(u.w);
            if (half == 0) ((float4*)(P.part_du + hc * KGW_C))[hl] = u;
            const float dsum = S[k].dsum + kgw_sum8(S[k].dsum_own);      // lanes 0..7 of each half: the edges handled 8 at a time
            const float esum = S[k].esum + kgw_sum8(S[k].esum_own);
            const float bsum = S[k].bsum + kgw_sum8(S[k].bsum_own);
            const float ssum = S[k].ssum + kgw_sum8(S[k].ssum_own);
            const float tot = dsum + kgw_xhalf(dsum);
            const float te = esum + kgw_xhalf(esum), tb = bsum + kgw_xhalf(bsum), ts = ssum + kgw_xhalf(ssum);
            if (lane == 0) {
                if (ck.nch == 1) P.da_dst[(h0 + k) * Dm.z_rows + zrow] = tot - (te / ts) * tb;
                else ((float4*)P.part_da)[hc] = make_float4(tot, te, tb, ts);
            }
        }
    }
}

template <int NH>
__global__ void __launch_bounds__(KGW_BLK) k_agg_bwd_combine_heads(LayerTab T, AggPtrs P, HeadDims Dm, int n_hops) {
  for (int hop = 0; hop < n_hops; ++hop) {
    const int lane = kgw_lane();
    const int nw = gridDim.x * 4;
    const int n_multi = P.meta->multi_cnt[hop];
    const int32_t* mm = P.multi + (int64_t)hop * P.multi_cap * 4;
    for (int kh = blockIdx.x * 4 + (threadIdx.x >> 6); kh < n_multi * NH; kh += nw) {
        const int k = kh / NH, h = kh % NH;
        const int first = mm[4 * k], nch = mm[4 * k + 1], row = mm[4 * k + 2], r = mm[4 * k + 3];
        if (!T.live[r]) continue;
        const int zrow = T.z0[r] + row * T.zstride[r];
        // fixed-order tree: lane-strided partial sums, then butterfly -- of the four per-chunk sums (D0, E, B, S) of the dst pass
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c = lane; c < nch; c += 64) {
            const float4 p = ((const float4*)P.part_da)[h * Dm.n_chunks + first + c];
            s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
        }
        s.x = wave_allsum_slow(s.x); s.y = wave_allsum_slow(s.y); s.z = wave_allsum_slow(s.z); s.w = wave_allsum_slow(s.w);
        if (lane == 0) P.da_dst[h * Dm.z_rows + zrow] = s.x - (s.y / s.w) * s.z;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward, src-major pass: one wavefront per source row (the general path; no pair / octet forms with heads)
// ------------------------------------------------------------------------------------------------
//      dH_j = sum_h [ sum_e adp[h][e].x dZ[h][zrow(e)] + sum_slots d a_src^h u_r^h + sum_dslots d a_dst^h v_r^h ]   (then relu_in)
// The entries (t_edge, t_zrow) of a block of 64 are loaded once; each head reads its own adp plane and gathers its own dZ plane.
template <int NH>
__device__ __forceinline__ void bwd_src_one_row_heads(const LayerTab& T, const AggPtrs& P, const HeadDims& Dm, int u) {
    const int lane = kgw_lane(), half = lane >> 5, hl = lane & 31;
    const int64_t NRC = (int64_t)T.n_rels * KGW_C;
    int ty = 0;
    while (ty + 1 < T.n_types && u >= T.type_src_base[ty + 1]) ++ty;
    const int j = u - T.type_src_base[ty];
    const int Rs = T.type_R_src[ty];
    const int tb = T.type_t_base[ty] + j * Rs;
    if (j >= P.meta->n_src[P.layer - 1][ty]) {          // padding row of a static layout: no gradient
        if (half == 0) ((float4*)(P.dH + (int64_t)u * KGW_C))[hl] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int tpv = (lane <= Rs) ? P.t_ptr[tb + lane] : 0;
    const int p0 = __shfl(tpv, 0, 64), p1 = __shfl(tpv, Rs, 64);
    const int tpn = __shfl_down(tpv, 1, 64);
    const unsigned long long slots = __ballot(lane < Rs && tpn > tpv);      // bit k: slot k has entries
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float dasv[NH];                                      // lane k holds d a_src of slot k, per head
#pragma unroll
    for (int h = 0; h < NH; ++h) dasv[h] = 0.f;
    for (int pb = p0; pb < p1; pb += 64) {
        const int nb = min(64, p1 - pb);
        const int hn = (nb + 1) >> 1;
        int te = 0, tz = 0;
        if (lane < nb) {
            te = P.t_edge[pb + lane];
            tz = P.t_zrow[pb + lane];
        }
        // segment heads of the per-slot sums (entries of one source are grouped by slot): scalar work, once for all heads
        unsigned long long heads = 1ull;
        for (unsigned long long left = slots; left; left &= left - 1) {
            const int k = __builtin_ctzll(left);
            const int s0 = __builtin_amdgcn_readlane(tpv, k);
            if (s0 > pb && s0 < pb + nb) heads |= 1ull << (s0 - pb);
        }
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            float al = 0.f, dp = 0.f;
            if (lane < nb) {
                const float2 a2 = ((const float2*)P.adp)[h * Dm.n_edges + te];
                al = a2.x; dp = a2.y;
            }
            float sv = dp;                               // one segmented inclusive scan over the 64 lanes (fixed tree)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const float o = __shfl_up(sv, d, 64);
                const bool open = lane >= d && ((heads >> (lane - d + 1)) & ((1ull << d) - 1ull)) == 0ull;
                sv += open ? o : 0.f;
            }
            for (unsigned long long left = slots; left; left &= left - 1) {
                const int k = __builtin_ctzll(left);
                const int s0 = __builtin_amdgcn_readlane(tpv, k), s1 = __builtin_amdgcn_readlane(tpv, k + 1);
                if (s1 <= pb || s0 >= pb + nb) continue;
                const int last = min(s1, pb + nb) - 1 - pb;
                const float sk = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sv), last));
                dasv[h] += (lane == k) ? sk : 0.f;
            }
            const float4* dZ4 = (const float4*)(P.dZ + h * Dm.z_rows * KGW_C);
            for (int q0 = 0; q0 < hn;) {
                const int rem = hn - q0;
                if (rem > 4)      { src_group<8>(dZ4, tz, al, q0, hn, nb, half, hl, acc); q0 += 8; }
                else if (rem > 2) { src_group<4>(dZ4, tz, al, q0, hn, nb, half, hl, acc); q0 += 4; }
                else              { src_group<2>(dZ4, tz, al, q0, hn, nb, half, hl, acc); q0 += 2; }
            }
        }
    }
    acc.x += kgw_xhalf(acc.x); acc.y += kgw_xhalf(acc.y);
    acc.z += kgw_xhalf(acc.z); acc.w += kgw_xhalf(acc.w);
    if (p1 > p0) {
        // d a_src flows back into h_src through a_s^h = <h_src, u_r^h>
        for (unsigned long long left = slots; left; left &= left - 1) {
            const int k = __builtin_ctzll(left);
            const int r = T.rel_of_slot[ty][k];
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const float dk = __shfl(dasv[h], k, 64);
                const float4 u4 = ((const float4*)(P.U + h * NRC + (int64_t)r * KGW_C))[hl];
                fma4(acc, dk, u4);
            }
        }
    }
    // destination side of the same node: a_d^h[i, r] = <h[i], v_r^h> sends d a_d back into h[i]
    const int Rd = T.type_R_dst[ty];
    const bool is_dst = Rd > 0 && j < P.meta->n_rows[P.layer - 1][ty];
    const int zb = T.type_z_base[ty] + j * Rd;
    if (is_dst) {
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const float dav = (lane < Rd) ? P.da_dst[h * Dm.z_rows + zb + lane] : 0.f;
            for (int k = 0; k < Rd; ++k) {
                const float dk = __shfl(dav, k, 64);
                if (dk != 0.f) {
                    const int r = T.rel_of_dslot[ty][k];
                    const float4 v4 = ((const float4*)(P.V + h * NRC + (int64_t)r * KGW_C))[hl];
                    fma4(acc, dk, v4);
                }
            }
        }
    }
    if (P.relu_in) {
        const float4 h4 = ((const float4*)(P.H + (int64_t)u * KGW_C))[hl];
        acc.x = h4.x > 0.f ? acc.x : 0.f; acc.y = h4.y > 0.f ? acc.y : 0.f;
        acc.z = h4.z > 0.f ? acc.z : 0.f; acc.w = h4.w > 0.f ? acc.w : 0.f;
    }
    if (half == 0) ((float4*)(P.dH + (int64_t)u * KGW_C))[hl] = acc;
}

// Rider blocks [0, n_riders) of the grid, head-major: head h's 2 * 8 * n_rels blocks are the single-head riders (bwd_src_rider:
// the pieces of d u_r^h from part_du[h], of d v_r^h from da_dst[h]) run on head h's planes, into duv_ws[h] = [2][n_rels][8][128].
template <int NH>
__global__ void __launch_bounds__(KGW_BLK) k_agg_bwd_src_heads(LayerTab T, AggPtrs P, HeadDims Dm, int n_src_rows, int main_blocks,
                                                               int n_riders) {
    __shared__ float s_dp[KGW_BLK];
    if ((int)blockIdx.x < n_riders) {
        const int per_head = 2 * KGW_DUV_SPLIT * T.n_rels;
        const int h = (int)blockIdx.x / per_head;
        AggPtrs Q = P;
        Q.part_du = P.part_du + h * Dm.n_chunks * KGW_C;
        Q.da_dst = P.da_dst + h * Dm.z_rows;
        Q.duv_ws = P.duv_ws + (int64_t)h * per_head * KGW_C;
        bwd_src_rider(T, Q, (int)blockIdx.x - h * per_head, nullptr, s_dp);
        return;
    }
    // a wavefront takes one source row at a time, LAST rows first (the long rows of the genes / GO terms start the kernel)
    const int nw = main_blocks * 4;
    const int w0 = ((int)blockIdx.x - n_riders) * 4 + (threadIdx.x >> 6);
    for (int i0 = w0; i0 < n_src_rows; i0 += nw)
        bwd_src_one_row_heads<NH>(T, P, Dm, __builtin_amdgcn_readfirstlane(n_src_rows - 1 - i0));
}

// d u_r^h / d v_r^h from their eight pieces: blockIdx.z = head
template <int NH>
__global__ void __launch_bounds__(KGW_C) k_duv_fold_heads(int n_rels, const float* __restrict__ ws, float* __restrict__ dU,
                                                           float* __restrict__ dV) {
    const int r = blockIdx.x, v = blockIdx.y, h = blockIdx.z, c = threadIdx.x;
    const float* p = ws + (((int64_t)h * 2 + v) * n_rels + r) * KGW_DUV_SPLIT * KGW_C + c;
    (v ? dV : dU)[((int64_t)h * n_rels + r) * KGW_C + c] = kgw_duv_sum8(p);
}
