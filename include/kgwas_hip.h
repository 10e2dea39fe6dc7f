/*
 * kgwas_hip.h -- C ABI of libkgwas_hip.so, the MI355X (gfx950) hot path of KGWAS.
 *
 * The reference (snap-stanford/KGWAS) is pure Python and has NO FFI / plugin boundary of its own
 * (SURVEY.md 8b): its native work happens inside third-party wheels (torch_geometric,
 * torch_sparse / pyg_lib, torch_scatter).  This header is therefore the seam *under* the
 * reference's Python API; each entry point names the reference call site whose native work it
 * replaces.  All pointers are device pointers unless named *_host; all buffers are owned by the
 * caller (torch-allocated); no function allocates, frees or synchronises; every function only
 * enqueues work on `stream` (a hipStream_t) and returns a status:
 *      0 = ok, <0 = argument error (KGW_E_*), >0 = hipError_t from a launch.
 * No C++ exceptions cross this boundary.  Functions are re-entrant (no global mutable state).  What the library keeps per
 * process is immutable after first use: a handful of routing constants read ONCE from KGW_* environment variables (A/B
 * experiments: KGW_TN_SPLIT, KGW_TN_DIRECT_ROWS, KGW_MLP2_SPLIT, KGW_TS_MIN_SHIFT -- unset in normal use) and the one-time
 * hipFuncSetAttribute calls of the kernels that take more than 64 KB of LDS.
 *
 * Vocabulary (the reference's domain): node types, relations (= edge types), seeds, hops,
 * segments (= one destination row of one relation), chunks (<= KGW_CHUNK edges of one segment).
 */
#ifndef KGWAS_HIP_H
#define KGWAS_HIP_H

#include <math.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KGW_VERSION      125          /* 0.2.5 */
#define KGW_MAX_TYPES    8
#define KGW_MAX_RELS     64
#define KGW_MAX_LAYERS   4
#define KGW_CHUNK        128          /* edges per chunk (one wavefront processes one chunk; the longest chunks set
                                         the aggregate kernels' tail: 256 -> 128 took k_agg_fwd 64 -> 56 us)           */
#define KGW_TILE         1024         /* scan tile; per-type node regions are padded to this  */
#define KGW_C            128          /* hidden width (gnn_hidden_dim, kgwas/kgwas.py:52)     */

#define KGW_F_RAW_WEIGHTS 1           /* KgwLayerArgs.flags: no softmax (the reference's attention export,
                                         kgwas/utils.py:446-461 with return_raw_attention_weights)      */
#define KGW_F_DUV_PIECES  4           /* bwd_src with dU / dV riders: leave d u_r / d v_r as their eight level-1 pieces in duv_ws
                                         ([2][n_rels][8][128]: k_duv_fold is not launched, dU / dV are not written) -- the consumer
                                         adds them: KgwRelvecJob.duv_pieces / KgwFoldArgs.duv_pieces                              */
#define KGW_F_RELU_INPUT  2           /* bwd_src: H is the output of a ReLU (model.py:75) whose backward is folded
                                         into this pass: dH *= (H > 0)                                   */
#define KGW_F_SIGMOID_GATE 8          /* forward and bwd_dst: every edge is weighted by sigmoid(e / T) instead of by the softmax over
                                         its row (the reference GATConv's sigmoid_gat, kgwas/conv.py:49,219-220; the rule:
                                         kgwgate_weight below).  bwd_src ignores it.  Together with KGW_F_RAW_WEIGHTS, n_heads > 1, a
                                         non-zero partial_rels or a non-NULL drop_word_dev: KGW_E_UNSUPPORTED -- before any launch  */

#define KGW_OK           0
#define KGW_E_NULL      -1
#define KGW_E_RANGE     -2
#define KGW_E_UNSUPPORTED -3

typedef void* kgw_stream_t;           /* hipStream_t */

/* Resident knowledge graph: one dst-major CSR per relation, (dst, src)-sorted like the CSC that
 * NeighborLoader builds once per edge type (kgwas/kgwas.py:99-113; PyG to_csc).               */
typedef struct KgwGraph {
    int32_t n_types, n_rels, n_layers, n_hops;  /* n_hops = n_layers (minibatch) or 1 (full graph) */
    int32_t n_nodes[KGW_MAX_TYPES];       /* N_T                                             */
    int32_t node_base[KGW_MAX_TYPES + 1]; /* KGW_TILE-aligned start of type T in g2l / n_id   */
    int32_t R_dst[KGW_MAX_TYPES];         /* #relations whose destination type is T           */
    int32_t R_src[KGW_MAX_TYPES];         /* #relations whose source type is T                */
    int32_t rel_src[KGW_MAX_RELS];
    int32_t rel_dst[KGW_MAX_RELS];
    int32_t rel_slot_dst[KGW_MAX_RELS];   /* column block of relation r in Z[dst type]        */
    int32_t rel_slot_src[KGW_MAX_RELS];
    int64_t rowptr_off[KGW_MAX_RELS];     /* element offset of relation r inside g_rowptr     */
    int64_t col_off[KGW_MAX_RELS];        /* element offset of relation r inside g_col        */
    uint8_t rel_live[KGW_MAX_LAYERS][KGW_MAX_RELS]; /* [l-1][r]: layer l computes relation r  */
    /* Static layout (HIP-graph capture): when static_layout != 0 the row blocks of layer l are laid out
     * with these fixed capacities instead of the batch's own counts, so every buffer address and launch
     * geometry is batch independent; a batch that needs more sets KgwBatchMeta.error bit 5.          */
    int32_t static_layout;
    int32_t cap_rows[KGW_MAX_LAYERS][KGW_MAX_TYPES];  /* destination rows of type T in layer l        */
    int32_t cap_src[KGW_MAX_LAYERS][KGW_MAX_TYPES];   /* source rows of type T in layer l             */
    uint32_t short_types;                 /* bit T: nodes of type T have few out-edges (mean <= 4): kgw_sample_batch marks the
                                             groups of 8 consecutive source rows of such a type that the backward can process
                                             8 lanes per row (KgwLayerArgs.oct_flags); a scheduling hint, never a correctness one */
    const int32_t* g_rowptr;              /* per relation N_dst+1 entries, relative to col_off */
    const int32_t* g_col;                 /* global source ids                                */
} KgwGraph;

/* Counts and layouts of one sampled batch; written by the device, copied to meta_host.        */
typedef struct KgwBatchMeta {
    int32_t hop_cnt[KGW_MAX_TYPES][KGW_MAX_LAYERS + 1];   /* new nodes of type T at hop k      */
    int32_t node_off[KGW_MAX_TYPES][KGW_MAX_LAYERS + 2];  /* prefix over hops (local id ranges) */
    int32_t seg_off[KGW_MAX_LAYERS][KGW_MAX_RELS + 1];    /* first segment of (dst hop h, rel r) */
    int32_t seg_end[KGW_MAX_LAYERS];     /* cumulative #segments through dst hop h             */
    int32_t edge_end[KGW_MAX_LAYERS];    /* cumulative #edges    through dst hop h             */
    int32_t chunk_end[KGW_MAX_LAYERS];   /* cumulative #chunks   through dst hop h             */
    int32_t multi_cnt[KGW_MAX_LAYERS];   /* #multi-chunk segments in dst hop h                 */
    /* per layer l (index l-1): */
    int32_t n_rows[KGW_MAX_LAYERS][KGW_MAX_TYPES];   /* destination rows of type T            */
    int32_t z_base[KGW_MAX_LAYERS][KGW_MAX_TYPES + 1]; /* first Z row (of 128 floats) of type T */
    int32_t n_src[KGW_MAX_LAYERS][KGW_MAX_TYPES];    /* source rows of type T in the layer input */
    int32_t src_base[KGW_MAX_LAYERS][KGW_MAX_TYPES + 1]; /* first H row of type T             */
    int32_t t_base[KGW_MAX_LAYERS][KGW_MAX_TYPES + 1];   /* first transposed row of type T    */
    int32_t lay_rows[KGW_MAX_LAYERS][KGW_MAX_TYPES]; /* row-block sizes the bases above were built from */
    int32_t lay_src[KGW_MAX_LAYERS][KGW_MAX_TYPES];  /*  (= n_rows / n_src unless static_layout)        */
    int32_t n_chunks[KGW_MAX_LAYERS];    /* chunks used by layer l                             */
    int32_t n_edges[KGW_MAX_LAYERS];     /* edges aggregated by layer l                        */
    int32_t t_entries[KGW_MAX_LAYERS];   /* entries in the layer's src-major structure         */
    int32_t cur[8];                      /* device-side scratch cursors                        */
    int32_t error;                       /* !=0: a capacity was exceeded                       */
    int32_t pad_[3];
} KgwBatchMeta;

/* Chunk record: <= KGW_CHUNK consecutive edges of one segment.  8 x int32 = 32 bytes.          */
typedef struct KgwChunk {
    int32_t e0, e1;        /* local (batch) edge range                                        */
    int32_t row;           /* destination row (local id inside its node type)                 */
    int32_t rel;           /* relation id                                                     */
    int32_t first;         /* index of the first chunk of this segment                        */
    int32_t nch;           /* #chunks of this segment (1 => this chunk writes final results)   */
    int32_t gpos_lo, gpos_hi; /* position of edge e0 inside g_col (64-bit)                     */
} KgwChunk;

/* Buffers of one sampled batch (all device memory, worst-case sized by the caller).            */
typedef struct KgwBatchBuf {
    int32_t* g2l;          /* [node_base[n_types]] global -> local id, -1 = not sampled        */
    int32_t* n_id;         /* [node_base[n_types]] local -> global id, per type region         */
    int32_t* seg_deg;      /* [seg_cap]                                                        */
    int32_t* seg_nch;      /* [seg_cap]                                                        */
    int32_t* seg_ptr;      /* [seg_cap + 1]  first local edge of each segment                  */
    int32_t* seg_chptr;    /* [seg_cap + 1]  first chunk of each segment                       */
    int32_t* col_local;    /* [edge_cap]     source local id of each local edge                */
    KgwChunk* chunks;      /* [chunk_cap]                                                      */
    int32_t* multi;        /* [n_hops][multi_cap][4] = {first, nch, row, rel}                  */
    int32_t* t_cnt[KGW_MAX_LAYERS];   /* [trow_cap + 1] histogram / cursor scratch             */
    int32_t* t_ptr[KGW_MAX_LAYERS];   /* [trow_cap + 1] src-major row pointers                 */
    int32_t* t_edge[KGW_MAX_LAYERS];  /* [edge_cap] local edge id of each entry                */
    int32_t* t_zrow[KGW_MAX_LAYERS];  /* [edge_cap] Z row (dst row * R_dst + slot) of the entry */
    uint8_t* t_rel[KGW_MAX_LAYERS];   /* [edge_cap] relation id of the entry (optional: NULL = not written)  */
    int32_t* scan_tmp;     /* [scan_cap] >= kgw_sampler_scan_ints(seg_cap, node slots, trow_cap): scan scratch of the hops, then
                              the [layer][bucket][block] counts of the src-major sort                                             */
    int32_t* t_tmp;        /* [8 * (edge_cap + 1)], 16-B aligned, four arrays of edge_cap + 1 per layer of a pair (the second layer's
                              behind the first's): row key of every edge | (first layer's slot only) chunk of every edge, written
                              hop by hop by the relabelling pass and shared by all layers | keys | edge ids stably sorted by bucket
                              (the src-major radix sort)                                                                           */
    KgwBatchMeta* meta;    /* device                                                           */
    KgwBatchMeta* meta_host; /* pinned host mirror (async D2H at the end of sampling)          */
    int64_t seg_cap, edge_cap, chunk_cap, multi_cap, trow_cap, scan_cap;
    int32_t grid_blocks;   /* blocks of the sampler's grid-stride launches; 0 = default (2048: the call has the GPU to
                              itself).  A sampler replayed BESIDE a training step (second HIP graph on a side stream):
                              1024 -- what it costs the step is how long each of its kernels stays resident */
    int32_t pad_;
} KgwBatchBuf;

/* One attention-aggregate layer over a sampled batch (kgwas/conv.py:177-190 for every relation
 * of the layer at once + the relation sum of PyG HeteroConv, kgwas/model.py:74).               */
typedef struct KgwLayerArgs {
    int32_t layer;                 /* 1-based                                                  */
    int32_t n_chunks, n_multi_hops;/* launch-size HINT (>= the batch's chunk count; the kernels read the
                                      actual counts from meta_dev) ; multi lists of dst hops [0,n_multi_hops) */
    int32_t n_src_rows;            /* rows of H / dH in the layout (src_base[n_types])         */
    float   neg_slope, inv_temp;   /* LeakyReLU slope (0.2), 1/temperature (1)                 */
    int32_t flags;                 /* KGW_F_RAW_WEIGHTS: forward weights messages by the raw logits   */
    /* Attention heads (this word was padding that callers zeroed: the struct keeps its size and offsets).  0 or 1: one head -- the
     * kernels, layouts and bits of a call that left it zero.  NH = 2 or 4: NH heads
     * over the SAME layer input (the aggregate gathers H and the caller applies W_src afterwards, so a head is a pair (u_r^h, v_r^h)
     * and all heads share the one row gather per edge).  Every head-carrying array is then NH PLANES, head-major, plane h having
     * exactly the single-head layout:
     *      U, V, dU, dV      [NH][n_rels][128]
     *      Z, dZ             [NH][z rows][128]          stat [NH][z rows][2]          da_dst [NH][z rows]
     *      e_edge            [NH][n_edges]              adp  [NH][n_edges][2]
     *      part              [NH][n_chunks][132]        part_da [NH][n_chunks][4]     part_du [NH][n_chunks][128]
     *      duv_ws            [NH][2][n_rels][8][128]    (KGW_F_DUV_PIECES leaves the pieces there, head by head)
     * with the plane sizes taken from the LAYOUT the caller allocated by: z rows = meta_host->z_base[layer-1][n_types], n_edges =
     * meta_host->n_edges[layer-1], n_chunks = this struct's n_chunks.  H, dH (summed over the heads), chunks, col_local, t_* and
     * meta_* are as with one head.  Per head, relation and destination:  e^h_ij = leaky_relu(<x_j, u_r^h> + <x_i, v_r^h>),
     * alpha^h = softmax_j(e^h / T), Z[h][i, r] = sum_j alpha^h_ij x_j.
     * Any other value: KGW_E_RANGE.  NH > 1 together with KGW_F_RAW_WEIGHTS, partial_rels, drop_word_dev, logit_bias / rel_sums,
     * a_dst without V, or da_src (d u_r / d v_r come from the part_du .. dV route only): KGW_E_UNSUPPORTED -- before any launch.
     * kgw_edge_alpha is single-head (NH > 1: KGW_E_UNSUPPORTED; call it per plane); t_rel / oct_flags are hints and ignored.      */
    int32_t n_heads;
    const KgwGraph* graph_host;    /* host copy, passed by value to the kernels               */
    const KgwBatchMeta* meta_host; /* host struct holding the LAYOUT (z_base, src_base, t_base, lay_*) */
    const KgwBatchMeta* meta_dev;  /* device struct written by kgw_sample_batch (actual counts)        */
    const KgwChunk* chunks;
    const int32_t* multi;  int64_t multi_cap;
    const int32_t* col_local;
    const float* H;                /* [n_src_rows][128] layer input, type-major (src_base)     */
    const float* a_dst;            /* [z rows]  <h_dst[i], W_dst^T att_dst> per (row, relation); read only if V == NULL */
    const float* V;                /* [n_rels][128]  v_r = W_dst^T att_dst: a_dst is computed in-kernel from the
                                      destination node's own row of H (every destination type has a block in H)  */
    const float* U;                /* [n_rels][128]  u_r = W_src^T att_src                     */
    float* Z;                      /* [z rows][128]  sum_j alpha_ij h_src[j]  (pre-zeroed)      */
    float* stat;                   /* [z rows][2]    (row max, denominator)                    */
    float* e_edge;                 /* [n_edges]      leaky_relu logits per local edge          */
    float* part;                   /* [n_chunks][130] partial (m, s, acc) of multi-chunk segs  */
    /* backward */
    const float* dZ;               /* [z rows][128]                                            */
    float* adp;                    /* [n_edges][2]   (alpha, d pre-activation) per local edge  */
    float* da_dst;                 /* [z rows]                                                 */
    float* part_da;                /* [n_chunks][4], 16-byte aligned: per-chunk sums of a multi-chunk row's d a_dst */
    const int32_t* t_ptr; const int32_t* t_edge; const int32_t* t_zrow;
    float* dH;                     /* [n_src_rows][128]                                        */
    /* optional profiling hooks (NULL = off): hipEvent_t handles owned by the caller, recorded on `stream`
     * immediately before and after the MAIN kernel of the call (k_agg_fwd / k_agg_bwd_dst / k_agg_bwd_src), i.e.
     * excluding the small combine launches for hub rows -- bench.py's per-kernel roofline timing */
    void* ev_before; void* ev_after;
    float* da_src;                 /* [n_src_rows][2*ld], ld = (n_rels+3)&~3: columns [0,ld) d a_src, [ld,2ld) d a_dst
                                      of the node, one column per relation id (n_rels <= KGW_MAX_RELS)  */
    const float* logit_bias;       /* optional [n_rels]: constant added to the pre-activation logit of every edge of relation r
                                      (FC_output folded into the layer-1 relation parameters: the feature MLP's last Linear
                                      H = h2 T + c enters conv.py:150-152 only through <H, u_r> and <H, v_r>, whose constant
                                      parts <c_src, u_r> + <c_dst, v_r> land here while T is multiplied into U and V)     */
    uint64_t partial_rels;         /* forward: bit r set => the segments of relation r are written as PARTIAL online-softmax
                                      states -- Z = sum_j exp(e_ij - m) h_j (not divided), stat = (m, sum_j exp(e_ij - m)) --
                                      for the caller to merge across GPUs (SNP-sharded mode: a rank holds only its own SNP
                                      sources of a SNP->Gene relation; kgw_softmax_merge) before anything reads them;
                                      backward (dst pass): d a_dst of these rows is the plain sum over this rank's edges (the
                                      ranks' values are added), without the row-consistent correction of whole rows          */
    const uint8_t* t_rel;          /* optional (NULL = off), backward src pass: relation id of every src-major entry
                                      (KgwBatchBuf.t_rel) and                                                              */
    const int32_t* oct_flags;      /* one flag per group of 8 consecutive source rows (row index / 8; KgwBatchBuf.t_cnt[layer-1]
                                      after kgw_sample_batch): != 0 => the eight rows are real rows of one node type of
                                      KgwGraph.short_types, none of them a destination row of the layer, each with at most 8
                                      entries.  Such a group is processed by ONE wavefront, 8 lanes per row, without the per-row
                                      slot bookkeeping of the general path (the SNP rows: ~2 entries, two thirds of all rows)   */
    float* rel_sums;               /* optional, kgw_gat_aggregate_bwd_src: [n_rels] <- per relation, the sum of d a_dst over its
                                      destination rows = the gradient of logit_bias (what kgw_relation_sums computes), by
                                      n_rels extra blocks of the same launch.  Needs V (in-kernel a_dst) so that da_dst is final */
    /* d u_r / d v_r without the [d a_src | d a_dst] rows (da_src may then be NULL): kgw_gat_aggregate_bwd_dst leaves, per chunk,
     * sum_e dpre_e h_src(e) in part_du [n_chunks][128]; kgw_gat_aggregate_bwd_src adds them up per relation (and
     * d v_r = sum_i d a_dst[i, r] h_dst[i] over the destination rows) with extra blocks of its launch plus one small fold launch,
     * into dU / dV [n_rels][128] (zero rows for relations the layer does not compute).  seg_chptr = KgwBatchBuf.seg_chptr;
     * duv_ws: 2 * n_rels * 8 * 128 floats of workspace.  All five or none.                                              */
    float* part_du; const int32_t* seg_chptr; float* duv_ws; float* dU; float* dV;
    /* optional attention dropout (rule: kgwdrop_keep below), read by kgw_gat_aggregate_fwd and kgw_gat_aggregate_bwd_dst, which
     * must be given the same three values for one layer of one step.  Together with KGW_F_RAW_WEIGHTS or a non-zero partial_rels
     * the calls return KGW_E_UNSUPPORTED; a drop_scale that is not finite or < 1 returns KGW_E_RANGE -- before any launch.       */
    const uint64_t* drop_word_dev; /* device, one 64-bit word read when the kernels run (NULL = no dropout: the plain kernels)   */
    uint32_t drop_thresh;          /* floor(p * 2^32), 0 <= p < 1                                                               */
    float drop_scale;              /* (float)(1 / (1 - p))                                                                      */
} KgwLayerArgs;

/* ---- entry points ------------------------------------------------------------------------ */

int kgw_version(void);
const char* kgw_status_string(int status);
/* sizeof() of the ABI structs in the order Graph, BatchMeta, Chunk, BatchBuf, LayerArgs, TnJob, GradSrc, EdgeAttr, LrSchedule,
 * OptimCtl -- lets a binding verify its mirror structs (the first n; a library that predates an entry leaves it untouched).   */
int kgw_struct_sizes(int64_t* out, int n);

/* Replaces: NeighborLoader.__next__ (kgwas/kgwas.py:99-113,129; torch_sparse/pyg_lib
 * hetero_neighbor_sample + relabel).  Expands `n_seeds` seed nodes of type `seed_type` over
 * n_hops hops taking ALL in-neighbours, writes local ids, per-segment CSR, chunk lists and the
 * src-major (transposed) structure of every layer, then copies KgwBatchMeta to meta_host.
 * full_graph != 0: every node of every type is a seed (whole-graph inference / attention export,
 * kgwas/utils.py:446-461).                                                                    */
int kgw_sample_batch(const KgwGraph* graph, const KgwBatchBuf* buf, const int64_t* seeds,
                     int32_t n_seeds, int32_t seed_type, int32_t full_graph, kgw_stream_t stream);
/* ints KgwBatchBuf.scan_tmp must hold (KgwBatchBuf.scan_cap) for buffers of these capacities.  (The src-major sort of
 * kgw_sample_batch takes blocks of up to 147 M src-major rows = sum over node types of rows x relations leaving the type;
 * beyond that the call returns KGW_E_UNSUPPORTED.)                                                                          */
int64_t kgw_sampler_scan_ints(int64_t seg_cap, int64_t node_slots, int64_t trow_cap);
/* The same call in parts [part_begin, part_end] (kgw_sample_batch = parts 0 .. 2*n_hops): hop h is part 2h (its segments
 * and chunks, and the flag KGW_PENDING = -2 in g2l on every not-yet-sampled source node) and part 2h+1 (flags -> local
 * ids, relabelled edges); part 2*n_hops = layer tables, src-major structures, meta export.  SNP-sharded multi-GPU mode
 * (BASELINE.json north_star; no counterpart in the single-device reference, kgwas/kgwas.py:38-39): between parts 2h and
 * 2h+1 the ranks take the element-wise MIN of the g2l regions of the REPLICATED node types (one RCCL all-reduce of
 * ~44 k int32), so every rank expands the same Gene / GO frontier although it only sees its own SNP seeds.        */
int kgw_sample_batch_parts(const KgwGraph* graph, const KgwBatchBuf* buf, const int64_t* seeds,
                           int32_t n_seeds, int32_t seed_type, int32_t full_graph, int32_t part_begin,
                           int32_t part_end, kgw_stream_t stream);

/* Finite fan-out: PyG's NeighborLoader(num_neighbors=[k_1, ..., k_L]) (list form, without replacement).  An EXTENSION of the
 * reference's loader, which trains with [-1] * L only (kgwas/kgwas.py:99-113).  fanout[h] (h = 0 .. n_hops-1; -1 or >= 1)
 * applies to the expansion of the nodes first reached at hop h (hop 0 = the seeds), to every relation alike: a segment holds
 * min(deg, fanout[h]) entries of its CSR row, in CSR order; -1 keeps the row.  A node is expanded once, at the hop that first
 * reached it, so everything else about a batch (hop-pruned layers, chunk lists, src-major structures) keeps its meaning, and
 * a call whose every fanout[h] is at least the largest degree writes the buffers of the plain call bit for bit.
 *
 * WHICH entries is a pure function of (sample seed, relation, destination, position) -- not of launch geometry, wavefront
 * order or atomics -- so that anyone can restate it:
 *      key(p) = kgwfan_key(sample_seed, relation id, GLOBAL destination id, position p in the row)           (below)
 *      the segment = the fanout[h] entries with the smallest (key, position), i.e. position breaks ties
 * (kgwfan_mix32 is a bijection of the 32-bit words, so the keys of one row are in fact pairwise distinct).
 * sample_seed is a 64-bit word READ FROM DEVICE MEMORY (sample_seed_dev) when the kernels run: the call can be captured in a HIP
 * graph once and replayed with another word for every batch.  The loader sets it to mix(loader seed, epoch, batch index).    */
#ifdef __HIPCC__
#define KGWFAN_INLINE static __host__ __device__ __forceinline__
#else
#define KGWFAN_INLINE static inline
#endif
KGWFAN_INLINE uint32_t kgwfan_mix32(uint32_t h) {            /* the 32-bit finaliser of MurmurHash3 (public domain) */
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
KGWFAN_INLINE uint32_t kgwfan_step(uint32_t h, uint32_t x) { return kgwfan_mix32((h ^ x) + 0x9e3779b9u); }
KGWFAN_INLINE uint32_t kgwfan_row_hash(uint64_t sample_seed, int32_t rel, int32_t dst_global) {
    uint32_t h = kgwfan_step(0u, (uint32_t)(sample_seed & 0xffffffffu));
    h = kgwfan_step(h, (uint32_t)(sample_seed >> 32));
    h = kgwfan_step(h, (uint32_t)rel);
    return kgwfan_step(h, (uint32_t)dst_global);
}
KGWFAN_INLINE uint32_t kgwfan_key(uint64_t sample_seed, int32_t rel, int32_t dst_global, uint32_t position) {
    return kgwfan_mix32(kgwfan_row_hash(sample_seed, rel, dst_global) ^ position);
}
int kgw_sample_batch_fanout(const KgwGraph* graph, const KgwBatchBuf* buf, const int64_t* seeds, int32_t n_seeds,
                            int32_t seed_type, const int32_t* fanout /* [n_hops], host */, const uint64_t* sample_seed_dev,
                            kgw_stream_t stream);

/* Per-epoch order of the training seeds: what PyG's NeighborLoader(shuffle=True) does on the host.  An EXTENSION: the reference
 * passes no shuffle= (kgwas/kgwas.py:93-94) and visits its seeds in genome order every epoch.  The order of an epoch is a pure
 * function of (word, n) -- no launch geometry, no sort, no atomics -- so every rank of a multi-GPU run computes the same order
 * without talking to the others, and anyone can restate it: a 4-round Feistel network on 2 * hb bits, walked along its cycle
 * until it is back inside [0, n):
 *      base             = kgwfan_step(kgwfan_step(0, lo32(word)), hi32(word))                                 (kgwperm_base)
 *      hb               : k = max(2, bit_length(n - 1));  k += k & 1;  hb = k / 2        (1 <= n <= 2^31)     (kgwperm_half_bits)
 *      feistel(p)       : L = p >> hb, R = p & mask;  four times, r = 0 .. 3:
 *                             F = kgwfan_mix32(kgwfan_step(base, r) ^ R) & mask;  (L, R) = (R, L ^ F)
 *                         result (L << hb) | R                                                               (kgwperm_feistel)
 *      index(base, n, i): p = i;  do p = feistel(p) while (p >= n);  result p                                 (kgwperm_index)
 * feistel is a bijection of [0, 2^(2 hb)) whatever F is; following i along its cycle until the cycle re-enters [0, n) restricts
 * it to a bijection of [0, n), and the walk ends because i itself lies on the cycle.  2^(2 hb) <= 4 n, so a walk takes 4
 * applications or fewer on average.  The rule has no constants of its own.  The trainer sets word to order_word(seed, epoch)
 * (kgwas_amd/sampler.py).
 *
 * Two orders over ids[0 .. n) with GLOBAL batch size B, nb = n / B full batches:
 *      KGW_ORDER_SEEDS     position p holds ids[index(base, n, p)], every p < n (the n % B left-over seeds differ per epoch);
 *      KGW_ORDER_BATCHES   the fixed, contiguous batches, visited in another order: position q * B + j (q < nb, j < B) holds
 *                          ids[index(base, nb, q) * B + j]; positions from nb * B on keep ids[p].
 * Rank ``rank`` of ``world`` takes positions [i * B + rank * B / world, i * B + (rank + 1) * B / world) of batch i, i < nb (the
 * slices of the fixed order's multi-GPU runs).  kgw_epoch_order writes them batch after batch: nb * B / world entries, and for
 * world == 1 the tail behind them, positions nb * B .. n - 1 (several ranks drop the partial batch).  One launch, one index per
 * element, plain loads and stores; ids and out are device arrays.
 * n < 1, n > 2^31, B < 1, B % world != 0, a mode other than the two, rank outside [0, world): KGW_E_RANGE, nothing launched.    */
#define KGW_ORDER_SEEDS   1
#define KGW_ORDER_BATCHES 2
KGWFAN_INLINE uint32_t kgwperm_base(uint64_t word) {
    return kgwfan_step(kgwfan_step(0u, (uint32_t)word), (uint32_t)(word >> 32));
}
KGWFAN_INLINE int32_t kgwperm_half_bits(int64_t n) {
    int32_t k = 0;
    for (uint64_t v = (uint64_t)(n - 1); v; v >>= 1) ++k;         /* bit_length(n - 1) */
    if (k < 2) k = 2;
    k += k & 1;
    return k / 2;
}
KGWFAN_INLINE uint32_t kgwperm_feistel(uint32_t base, int32_t hb, uint32_t p) {
    const uint32_t mask = (1u << hb) - 1u;
    uint32_t L = p >> hb, R = p & mask;
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t F = kgwfan_mix32(kgwfan_step(base, r) ^ R) & mask;
        const uint32_t t = L ^ F;
        L = R; R = t;
    }
    return (L << hb) | R;
}
KGWFAN_INLINE uint32_t kgwperm_index(uint32_t base, int64_t n, uint32_t i) {       /* i < n <= 2^31 */
    const int32_t hb = kgwperm_half_bits(n);
    uint32_t p = i;
    do p = kgwperm_feistel(base, hb, p); while ((int64_t)p >= n);
    return p;
}
int kgw_epoch_order(const int64_t* ids, int64_t n, int64_t batch, int32_t mode, int32_t rank, int32_t world, uint64_t word,
                    int64_t* out, kgw_stream_t stream);

/* Attention dropout: alpha = F.dropout(alpha, p, training) after the softmax (kgwas/conv.py:224; the reference's HeteroGNN
 * never passes p, so like the finite fan-out this is an EXTENSION, off by default).  For LOCAL edge e of the batch (the index
 * of col_local / e_edge / adp) in layer l:
 *      base(word, l) = kgwfan_step(kgwfan_step(kgwfan_step(0, lo32(word)), hi32(word)), l)                  (kgwdrop_base)
 *      keep(e)       = kgwfan_mix32(base ^ e) >= thresh,   thresh = floor(p * 2^32)                          (kgwdrop_keep)
 *      m'(e)         = keep(e) ? scale : 0,                scale = (float)(1 / (1 - p))
 *      Z[i, r]       = sum_j m'(e_ij) alpha_ij H_src[j]    (alpha: the UNDROPPED softmax)
 * -- a pure function of (word, layer, local edge index), and the sampler's edge layout is itself specified exactly, so the
 * mask depends on no launch geometry, wavefront order or atomic.  stat (row max, denominator), e_edge and kgw_edge_alpha
 * describe the undropped softmax; a row whose edges are all dropped gets Z = 0.  Backward: because the stored Z is the dropped
 * one, <dZ_i, Z_i> = sum_k alpha_k dalpha'_k with dalpha'_e = m'(e) <dZ_i, H_j>, so d logit_e = alpha_e (dalpha'_e - <dZ_i, Z_i>)
 * and the record of the src-major pass is adp[e] = (alpha_e m'(e), d pre-activation_e).  thresh = 0, scale = 1 computes the
 * bits of the plain call.  word is READ FROM DEVICE MEMORY (KgwLayerArgs.drop_word_dev) when the kernels run: a captured step
 * replays with another word for every batch.  The trainer sets it to dropout_word(seed, epoch, batch) (kgwas_amd/sampler.py). */
KGWFAN_INLINE uint32_t kgwdrop_base(uint64_t word, int32_t layer) {
    uint32_t h = kgwfan_step(0u, (uint32_t)(word & 0xffffffffu));
    h = kgwfan_step(h, (uint32_t)(word >> 32));
    return kgwfan_step(h, (uint32_t)layer);
}
KGWFAN_INLINE int kgwdrop_keep(uint32_t base, uint32_t local_edge, uint32_t thresh) {
    return kgwfan_mix32(base ^ local_edge) >= thresh;
}

/* Learning-rate schedule: the rate of update t (1-based, the index the Adam kernels already form for their bias corrections:
 * t = *step_dev + 1) as a pure function of t -- the reference trains at one rate (kgwas/kgwas.py:116), so like the dropouts this is
 * an EXTENSION, off by default.  With s = t - 1, W = warmup_steps >= 0, N = total_steps >= 1, r = min_ratio in [0, 1] (min_lr / lr),
 * step_size >= 1 and gamma > 0:
 *      warm(s)  = W > 0 && s < W ? (s + 1) / W : 1
 *      u(s)     = clamp((s - W) / max(N - W, 1), 0, 1)                    (0 while s < W, 1 from s = N on)
 *      decay(s) = KGW_LR_CONSTANT: 1
 *                 KGW_LR_LINEAR:   1 - (1 - r) u
 *                 KGW_LR_COSINE:   r + (1 - r) (1 + cos(pi u)) / 2
 *                 KGW_LR_STEP:     gamma ^ floor(max(s - W, 0) / step_size)
 *      lr_t     = (float)((double)lr * warm * decay)                       (kgwlr_at: all arithmetic in double, rounded once)
 * bc1, bc2 and step_size = lr_t / bc1 stay what they are.  KGW_LR_CONSTANT with W = 0 gives lr_t == lr to the bit.  t is READ FROM
 * DEVICE MEMORY when the kernels run, so a captured step replays with a moving rate: no host copy, no capture per step.  Host and
 * device evaluate cos / pow in double; they may differ in the last bit before the one rounding (1 float32 ulp of lr_t at most). */
enum { KGW_LR_CONSTANT = 0, KGW_LR_LINEAR = 1, KGW_LR_COSINE = 2, KGW_LR_STEP = 3 };
typedef struct KgwLrSchedule {
    int32_t kind, warmup_steps, total_steps, step_size;     /* step_size: read by KGW_LR_STEP only                               */
    float min_ratio, gamma;                                 /* min_ratio: LINEAR / COSINE; gamma: STEP                           */
} KgwLrSchedule;
/* 1: the schedule is one the rule above defines.  Otherwise (an unknown kind, W < 0, N < 1, step_size < 1 on STEP, min_ratio
 * outside [0, 1], gamma not finite or <= 0) every entry point that takes it returns KGW_E_RANGE before any launch.              */
KGWFAN_INLINE int kgwlr_valid(const KgwLrSchedule* S) {
    if (S->kind < KGW_LR_CONSTANT || S->kind > KGW_LR_STEP || S->warmup_steps < 0 || S->total_steps < 1) return 0;
    if (S->kind == KGW_LR_STEP && S->step_size < 1) return 0;
    if (!(S->min_ratio >= 0.0f && S->min_ratio <= 1.0f)) return 0;
    if (!(S->gamma > 0.0f && S->gamma <= 3.4028234663852886e38f)) return 0;
    return 1;
}
KGWFAN_INLINE double kgwlr_warm(const KgwLrSchedule* S, int32_t s) {
    return (S->warmup_steps > 0 && s < S->warmup_steps) ? (double)(s + 1) / (double)S->warmup_steps : 1.0;
}
KGWFAN_INLINE double kgwlr_decay(const KgwLrSchedule* S, int32_t s) {
    const int32_t W = S->warmup_steps, span = S->total_steps - W > 1 ? S->total_steps - W : 1;
    double u = ((double)s - (double)W) / (double)span;
    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    const double r = (double)S->min_ratio;
    if (S->kind == KGW_LR_LINEAR) return 1.0 - (1.0 - r) * u;
    if (S->kind == KGW_LR_COSINE) return r + (1.0 - r) * (1.0 + cos(3.14159265358979323846 * u)) / 2.0;
    if (S->kind == KGW_LR_STEP) return pow((double)S->gamma, (double)((s > W ? s - W : 0) / S->step_size));
    return 1.0;
}
KGWFAN_INLINE float kgwlr_at(const KgwLrSchedule* S, float lr, int32_t t) {      /* t < 1 is taken as t = 1 */
    const int32_t s = t > 1 ? t - 1 : 0;
    return (float)((double)lr * kgwlr_warm(S, s) * kgwlr_decay(S, s));
}

/* Weight averaging: a shadow copy s of every parameter p, updated on the device after the optimiser's update -- the reference
 * evaluates, selects and saves the raw weights (kgwas/kgwas.py:153-173), so like the schedules this is an EXTENSION, off by default.
 * n = the optimiser's device step counter AFTER its tick = the number of updates done, n >= 1.  With start_step >= 1, every >= 1:
 *      event(n) = n >= start_step && (n - start_step) % every == 0
 *      k        = (n - start_step) / every                                (the number of events before this one)
 *      alpha    = KGW_AVG_EMA: k == 0 ? 1 : 1.0f - d,   d = warmup ? fminf(decay, (float)(1 + k) / (float)(10 + k)) : decay
 *                 KGW_AVG_SWA: 1.0f / (float)(k + 1)
 *      s        = fmaf(alpha, p - s, s)                                   (float32; alpha == 1: the bits of p are stored, a copy)
 * EMA: s <- d s + (1 - d) p, d capped from below by TF's (1 + k) / (10 + k) warm-up; SWA: the equal-weight mean of the parameters at
 * the events so far (torch.optim.swa_utils).  On a non-event s is not written.  n is READ FROM DEVICE MEMORY when the kernel runs:
 * a captured step replays with a moving alpha.  kgwavg_alpha returns event(n) and, on an event, stores alpha.                     */
enum { KGW_AVG_EMA = 0, KGW_AVG_SWA = 1 };
typedef struct KgwWeightAvg {
    int32_t kind, start_step, every, warmup;                /* warmup (0 | 1), decay: read by KGW_AVG_EMA only                    */
    float decay;                                            /* 0 < decay < 1                                                      */
} KgwWeightAvg;
/* 1: a configuration the rule above defines.  Otherwise (an unknown kind, start_step < 1, every < 1, on EMA a warmup other than
 * 0 / 1 or a decay outside (0, 1) or NaN) every entry point that takes it returns KGW_E_RANGE before any launch.                 */
KGWFAN_INLINE int kgwavg_valid(const KgwWeightAvg* A) {
    if (A->kind < KGW_AVG_EMA || A->kind > KGW_AVG_SWA || A->start_step < 1 || A->every < 1) return 0;
    if (A->kind == KGW_AVG_EMA && (A->warmup < 0 || A->warmup > 1 || !(A->decay > 0.0f && A->decay < 1.0f))) return 0;
    return 1;
}
KGWFAN_INLINE int kgwavg_alpha(const KgwWeightAvg* A, int32_t n, float* alpha) {
    if (n < A->start_step || (n - A->start_step) % A->every != 0) return 0;
    const int32_t k = (n - A->start_step) / A->every;
    if (A->kind == KGW_AVG_SWA) {
        *alpha = 1.0f / (float)(k + 1);
    } else if (k == 0) {
        *alpha = 1.0f;
    } else {
        const float d = A->warmup ? fminf(A->decay, (float)(1 + k) / (float)(10 + k)) : A->decay;
        *alpha = 1.0f - d;
    }
    return 1;
}

/* Hidden-state dropout: x = F.dropout(x, p, training) on the OUTPUT of message-passing layer l, 1 <= l <= L - 1 (after its ReLU,
 * kgwas/model.py:75; never on the feature MLPs' output, never on the last layer).  The reference's HeteroGNN has no such line:
 * like the attention dropout an EXTENSION, off by default.  For stored column c (0 .. 127) of the node with LOCAL index row within
 * node type t of the batch (the index into the type's n_id; NOT the row of the type-major layer input, whose bases differ between
 * a batch's own layout and the static one of a captured step):
 *      base(word, l, t) = kgwfan_step(kgwfan_step(kgwdrop_base(word, l), KGW_HDROP_TAG), t)                 (kgwhdrop_base)
 *      keep(row, c)     = kgwfan_mix32(base ^ (row * 128 + c)) >= thresh,   thresh = floor(p * 2^32)          (kgwhdrop_keep)
 *      y'(row, c)       = keep ? y * scale : 0.0f,                          scale = (float)(1 / (1 - p))
 * -- a pure function of (word, layer, node type, local row, column): no launch geometry and no capacity of a layout enters, and
 * the tag keeps the masks apart from the attention-dropout masks of the same (word, layer).  A dropped element is exactly 0.0f
 * whatever bits it held (a select, not a product: NaN and Inf do not survive a drop); thresh = 0, scale = 1 gives the input bits
 * back.  The backward of y' = m' y is dy = m' dy' with the same mask, recomputed: kgw_hidden_dropout is called on dY with the
 * values of the forward call, and no mask is stored.  word is READ FROM DEVICE MEMORY when the kernel runs, as above.
 *
 * One launch for up to 8 jobs (the destination types of one layer): job j drops rows [0, rows) of 128 floats, row i at
 * src + i * lds, into dst + i * ldd.  dst == src (and ldd == lds) drops in place; any other overlap is undefined.  One float4 per
 * lane, 32 lanes per row, grid-stride over the rows of all jobs; no atomics, no LDS.  Refused before any launch: jobs or word_dev
 * NULL, src or dst of a job with rows > 0 NULL: KGW_E_NULL;  n_jobs outside [1, 8], layer < 1, a scale that is not finite or < 1,
 * rows < 0 or > 2^25 (row * 128 + c must fit 32 bits), lds or ldd < 128 with rows > 1: KGW_E_RANGE;  a src or dst that is not
 * 16-byte aligned, lds % 4 or ldd % 4 != 0: KGW_E_UNSUPPORTED.  Jobs without rows are skipped; no rows at all: KGW_OK, no launch. */
#define KGW_HDROP_TAG 1751413360u     /* the bytes of 'hdrp', big-endian */
KGWFAN_INLINE uint32_t kgwhdrop_base(uint64_t word, int32_t layer, int32_t type) {
    return kgwfan_step(kgwfan_step(kgwdrop_base(word, layer), KGW_HDROP_TAG), (uint32_t)type);
}
KGWFAN_INLINE int kgwhdrop_keep(uint32_t base, uint32_t row, uint32_t col, uint32_t thresh) {
    return kgwfan_mix32(base ^ (row * 128u + col)) >= thresh;
}
typedef struct KgwHDropJob {
    const float* src; int64_t lds;    /* rows of 128 floats, leading dimension in floats                                          */
    float* dst; int64_t ldd;
    int32_t rows;                     /* local rows 0 .. rows - 1 of the type                                                      */
    int32_t type;                     /* node type id of the schema                                                                */
} KgwHDropJob;
int kgw_hidden_dropout(int32_t n_jobs, const KgwHDropJob* jobs, int32_t layer, const uint64_t* word_dev, uint32_t thresh,
                       float scale, kgw_stream_t stream);

/* Layer normalisation between the message-passing layers: x = relu(LayerNorm(y)) on the PRE-ACTIVATION output y of layer l,
 * 1 <= l <= L - 1, per node and per node type (torch.nn.LayerNorm(hidden, eps = 1e-5) / PyG's LayerNorm(mode='node') duplicated
 * per node type; the sites of the hidden-state dropout, which then follows the ReLU).  The reference's HeteroGNN has no norm: an
 * EXTENSION, off by default -- but unlike the dropouts it has learned parameters and is live in evaluation.  For one row y of
 * 128 stored columns of a model Cl = c_logical wide (columns Cl .. 127 are the zero padding of a narrower model):
 *      mean = (1 / Cl) sum_{c < Cl} y_c        var = (1 / Cl) sum_{c < Cl} (y_c - mean)^2      (passes over registers: the
 *      rstd = 1 / sqrt(var + eps)              xh_c = (y_c - mean) * rstd                       differences are formed BEFORE they
 *      out_c = max(0, xh_c * w_c + b_c)  for c < Cl,      out_c = 0.0f exactly for Cl <= c < 128    are squared, no E[y^2] - mean^2)
 * (kgwlnorm_out; the row sums go over the 32 lanes of a row by a butterfly, xor 16, 8, 4, 2, 1).  In float32 the mean is refined
 * once -- m0 = sum(y) / Cl, mean = m0 + sum(y - m0) / Cl, y_c - mean taken as (y_c - m0) - sum(y - m0) / Cl -- because at a row
 * mean of 1e4 a single float32 quotient is good to 5e-4 only, which a unit spread would see in every xh; the backward centres the
 * row again the same way around the stored mean.  Sums and means are correctly rounded divisions by Cl, so a constant row of
 * exactly summable values has mean = the value, var = 0, rstd = 1 / sqrt(eps) and out = max(0, b) bit for bit.  Backward, with
 * g the upstream gradient ALREADY masked by (out > 0) -- the consumer did it (out == NULL) or the kernel does it from the saved out:
 *      gh_c = g_c w_c       dy_c = rstd (gh_c - mean_c(gh) - xh_c mean_c(gh xh))     (means over c < Cl;  dy_c = 0.0f for c >= Cl)
 *      dw_c = sum_rows g_rc xh_rc           db_c = sum_rows g_rc                     (kgwlnorm_dy; 0.0f for c >= Cl)
 *
 * kgw_layer_norm_relu_fwd: one launch for up to 8 jobs (the destination types of one layer), the row mapping of
 * kgw_hidden_dropout (one float4 per lane, 32 lanes per row, grid-stride over the rows of all jobs, no LDS, no atomics).  Job j
 * reads rows [0, rows) at src + i * lds, writes out to dst + i * ldd and stat[2 i], stat[2 i + 1] = (mean, rstd); weight / bias
 * point at the 128 floats of the job's node type.  src is only read (whoever produced it may have saved it): dst == src is refused.
 * kgw_layer_norm_bwd: job j reads g, the saved y, stat, weight and (out != NULL) the saved out, and writes dy.  The column sums
 * are left as PER-BLOCK partial sums: job j owns the blocks [b0_j, b0_j + nb_j) of the grid, nb_j = ceil(rows_j / P) with P = 64
 * doubled until the grid has at most 2048 blocks -- a function of the row counts alone, so the layout and with it the bits are the
 * same on every run and every device.  A block walks its job's rows with stride 8 nb_j (8 row slots), every slot adds its rows in
 * ascending order, the 8 slots are added through LDS in slot order, and the block writes partial[block][2][128] = (dw, db).
 * kgw_layer_norm_partial_floats: the floats ``partial`` must hold for these jobs.  (One job per block rather than a
 * [block][job] table: the same fixed order, an eighth of the partial sums.)
 * kgw_layer_norm_fold: the SAME jobs; block t of n_types adds the partial sums of the job whose ``type`` is t in ascending block
 * order into dweight[t][128], dbias[t][128]; a type without a job, or whose job has no rows, gets zero rows.  No floating-point
 * atomics anywhere.
 * Refused before any launch: a NULL jobs / partial / dweight / dbias, a NULL pointer of a job with rows > 0 (``out`` may be
 * NULL): KGW_E_NULL;  n_jobs outside [1, 8], c_logical outside [1, 128], an eps that is not finite or < 0, rows < 0 or > 2^25, a
 * leading dimension < 128 with rows > 1, partial_floats too small, n_types outside [1, 8], a type outside [0, 8) / [0, n_types),
 * two jobs of one type (bwd, fold): KGW_E_RANGE;  a row pointer or weight / bias not 16-byte aligned, stat not 8-byte aligned, a
 * leading dimension % 4 != 0, dst == src: KGW_E_UNSUPPORTED.  Jobs without rows are skipped; no rows at all: no fwd / bwd launch. */
#define KGW_LNORM_EPS 1e-5f
KGWFAN_INLINE float kgwlnorm_out(float xh, float w, float b) { const float v = xh * w + b; return v > 0.0f ? v : 0.0f; }
KGWFAN_INLINE float kgwlnorm_dy(float gh, float xh, float rstd, float mean_gh, float mean_ghxh) {
    return rstd * (gh - mean_gh - xh * mean_ghxh);
}
typedef struct KgwLNormJob {
    const float* src; int64_t lds;    /* y: rows of 128 floats, leading dimension in floats                                        */
    float* dst; int64_t ldd;          /* out                                                                                       */
    int32_t rows;
    int32_t type;                     /* node type id of the schema (names the job; weight / bias already point at its row)        */
    const float* weight; const float* bias;       /* [128] each, columns c_logical .. 127 ignored                                 */
    float* stat;                      /* [rows][2]: (mean, rstd)                                                                   */
} KgwLNormJob;
typedef struct KgwLNormBwdJob {
    const float* g; int64_t ldg;      /* upstream gradient                                                                         */
    const float* y; int64_t ldy;      /* the forward's src                                                                         */
    const float* out; int64_t ldo;    /* the forward's dst, to mask g by (out > 0); NULL: g arrives masked                         */
    float* dy; int64_t lddy;
    int32_t rows;
    int32_t type;                     /* node type id: the row of dweight / dbias the fold writes                                  */
    const float* weight;              /* [128]                                                                                     */
    const float* stat;                /* [rows][2] of the forward                                                                  */
} KgwLNormBwdJob;
int kgw_layer_norm_relu_fwd(int32_t n_jobs, const KgwLNormJob* jobs, int32_t c_logical, float eps, kgw_stream_t stream);
int64_t kgw_layer_norm_partial_floats(int32_t n_jobs, const KgwLNormBwdJob* jobs);      /* (< 0: a status)                        */
int kgw_layer_norm_bwd(int32_t n_jobs, const KgwLNormBwdJob* jobs, int32_t c_logical, float* partial, int64_t partial_floats,
                       kgw_stream_t stream);
int kgw_layer_norm_fold(int32_t n_jobs, const KgwLNormBwdJob* jobs, const float* partial, int64_t partial_floats, int32_t n_types,
                        float* dweight, float* dbias, kgw_stream_t stream);

/* Root weight: a learned self term per layer and node type, y_i += W_root[l][t] x_i with x_i node i's OWN layer-l input (PyG's
 * SAGEConv.lin_r / RGCNConv.root / GATConv(residual=True); the reference builds GATConv(add_self_loops=False) for every relation
 * and a SNP has no SNP-SNP relation, so its own state never enters its own update: an EXTENSION, off by default, learned and live in
 * every mode).  For one destination row of 128 stored columns, W [128][128] in nn.Linear layout [out][in], bias-free:
 *      dst_n = act(y_n + sum_k x_k W[n][k])                 act = max(0, .) iff relu          (kgwroot_out)
 * with y the relation combine's pre-activation (the transform run with relu = 0).  Backward, g the upstream gradient:
 *      gm_n = out ? (out_n > 0 ? g_n : 0) : g_n             (out == NULL: g arrives masked, or no ReLU was applied)
 *      dx_k = sum_n gm_n W[n][k]                            times (x_k > 0) iff x_premasked    (kgwroot_mask)
 *      d y  = gm                                            (written to ``gm`` when the kernel had to mask: the transform behind it is
 *                                                            premasked and takes gm as its dY)
 *      dW[n][k] = sum_rows gm_n x_k                         by kgw_tn_gemm_multi, not here.
 * x_premasked: x is a ReLU output (possibly dropped) whose producer runs premasked -- the consumer of that state multiplies the
 * gradient by (x > 0) itself, as kgw_gat_aggregate_bwd does with KGW_F_RELU_INPUT for the same rows -- so the kernel does too.
 * Columns of a narrower model: with the pad columns of x, y and the pad rows / columns of W zero, the pad columns of dst and dx
 * are exactly 0.0f.
 *
 * kgw_root_linear_fwd / kgw_root_linear_bwd: one launch for up to 8 jobs (the destination types of one layer).  fp32 arithmetic on
 * the fp32 MFMA pipe (v_mfma_f32_32x32x2_f32, as kgw_linear).  A job owns a range of the grid's blocks -- ceil(tiles / P) of them,
 * 32-row tiles, P = 2 doubled until the grid has at most 2048 blocks; a block stages its job's 128 x 128 weights in LDS once, every
 * wavefront keeps its half (64 output columns) in registers and walks the job's row tiles.  Every output element is one
 * wavefront's sum in ascending k: no atomics, no partial sums, the bits do not depend on the grid.
 * Refused before any launch: a NULL jobs, a NULL x / y / dst / W (fwd) or g / dx / W, or x with x_premasked (bwd) of a job with
 * rows > 0 (``out`` and ``gm`` may be NULL; gm == NULL with out != NULL: the masked gradient is not written): KGW_E_NULL;  n_jobs
 * outside [1, 8], rows < 0 or > 2^25, a leading dimension < 128 with rows > 1, a type outside [0, 8) or given twice: KGW_E_RANGE;
 * a pointer not 16-byte aligned, a leading dimension % 4 != 0, an output that is one of the call's inputs or its other output
 * (dst == y, dst == x;  dx or gm == g, out or -- with x_premasked -- x;  gm == dx): KGW_E_UNSUPPORTED.  Beyond these equalities
 * the caller owes the kernels outputs that overlap NO input and no other output, of this job or another of the launch: a tile's two
 * column halves read whole rows of x / g / out while the other half stores, and partial overlaps are not looked for.  Jobs without
 * rows are skipped; no rows at all: KGW_OK without a launch. */
KGWFAN_INLINE float kgwroot_out(float y, float xw, int relu) { const float v = y + xw; return (relu && !(v > 0.0f)) ? 0.0f : v; }
KGWFAN_INLINE float kgwroot_mask(float g, float by) { return by > 0.0f ? g : 0.0f; }
typedef struct KgwRootJob {
    const float* x; int64_t ldx;      /* the destination rows' own layer input: rows of 128 floats                                 */
    const float* y; int64_t ldy;      /* the pre-activation of the relation combine                                                */
    float* dst; int64_t ldd;
    int32_t rows;
    int32_t type;                     /* node type id (names the job; W already points at its slice)                               */
    const float* W;                   /* [128][128], [out][in]                                                                     */
} KgwRootJob;
typedef struct KgwRootBwdJob {
    const float* g; int64_t ldg;      /* upstream gradient                                                                         */
    const float* out; int64_t ldo;    /* the forward's dst, to mask g by (out > 0); NULL: g is used as it is                       */
    const float* x; int64_t ldx;      /* the forward's x: read only with x_premasked                                               */
    float* gm; int64_t ldgm;          /* the masked gradient (written only when out != NULL), or NULL                              */
    float* dx; int64_t lddx;
    int32_t rows;
    int32_t type;
    const float* W;
    int32_t x_premasked;              /* dx *= (x > 0)                                                                             */
    int32_t reserved;
} KgwRootBwdJob;
int kgw_root_linear_fwd(int32_t n_jobs, const KgwRootJob* jobs, int32_t relu, kgw_stream_t stream);
int kgw_root_linear_bwd(int32_t n_jobs, const KgwRootBwdJob* jobs, kgw_stream_t stream);

/* Sigmoid-gated attention (KGW_F_SIGMOID_GATE): alpha = sigmoid(leaky_relu(a_j + a_i) / T) instead of the softmax over the row
 * (kgwas/conv.py:49,219-220, the reference GATConv's sigmoid_gat; its HeteroGNN never passes it, so like the dropout this is an
 * EXTENSION, off by default).  The gates are independent per edge and are not normalised by the row's degree.  With
 * d_e = <H_src[j], u_r> + a_d(i, r) (+ logit_bias[r]),  e_e = d_e > 0 ? d_e : slope * d_e,  inv_temp = 1 / T:
 *      g_e           = 1 / (1 + exp(-e_e * inv_temp))                                                        (kgwgate_weight)
 *      Z[i, r]       = sum_j g_e H_src[j]           (no row max, no denominator; a row without in-edges stays 0)
 *      d g_e         = <dZ[i, r], H_src[j]>
 *      d pre_e       = g_e (1 - g_e) d g_e inv_temp (e_e > 0 ? 1 : slope)
 *      adp[e]        = (g_e, d pre_e)               (the record of the src-major pass, which does not change)
 *      d a_dst[i, r] = sum_e d pre_e                (a plain sum: there is no common-shift invariance to restore)
 * e_edge keeps the leaky_relu logit e_e, as in every other mode; stat is (0, 1) on visited rows, as with KGW_F_RAW_WEIGHTS.  The
 * backward re-forms g_e from the stored e_edge with this one expression, so both passes see the same bits.  In fp32 the gate is
 * exactly 0 below e / T ~ -88.7 (the exponential overflows to +inf) and exactly 1 above ~ 16.7; both ends have d pre_e = 0. */
#ifdef __HIPCC__
static __device__ __forceinline__ float kgwgate_weight(float e, float inv_temp) { return 1.0f / (1.0f + __expf(-e * inv_temp)); }
#endif

/* Replaces: GATConv.edge_update + message + aggregate (kgwas/conv.py:200-228,182) and their
 * autograd for all relations of one layer.                                                    */
int kgw_gat_aggregate_fwd(const KgwLayerArgs* args, kgw_stream_t stream);
int kgw_gat_aggregate_bwd_dst(const KgwLayerArgs* args, kgw_stream_t stream);
int kgw_gat_aggregate_bwd_src(const KgwLayerArgs* args, kgw_stream_t stream);

/* SNP-sharded mode, the exchange step of a layer: the softmax of kgwas/conv.py:223 runs over ALL
 * in-edges of a destination gene, but a rank only aggregated the edges whose SNP source it owns.
 * kgw_softmax_pack: record x (132 floats: [0] = m, [1] = s, [4..131] = acc) <- the partial state of segment
 *   seg_zrow[x] (Z row / stat pair written by kgw_gat_aggregate_fwd under KgwLayerArgs.partial_rels).
 * kgw_softmax_merge: parts [n_ranks][n_seg][132] (every rank's pack, gathered in rank order) ->
 *   Z[seg_zrow[x]] = sum_p acc_p e^(m_p - m*) / (sum_p s_p e^(m_p - m*) + 1e-16), stat = (m*, that denominator), with
 *   m* = max over the ranks that saw an edge (s_p > 0); fixed rank order, so every rank computes the same bits.
 * kgw_scatter_rows: dst[ids[i]] = src[i] (rows of `width` floats): puts the all-reduced dZ rows of the exchanged segments
 *   back (the gather is kgw_gather_rows).                                                                          */
int kgw_softmax_pack(const float* Z, const float* stat, const int32_t* seg_zrow, int64_t n_seg, float* parts,
                     kgw_stream_t stream);
int kgw_softmax_merge(const float* parts, int32_t n_ranks, const int32_t* seg_zrow, int64_t n_seg, float* Z,
                      float* stat, kgw_stream_t stream);
int kgw_scatter_rows(const float* src, const int32_t* ids, int64_t n_rows, int32_t width, float* dst,
                     kgw_stream_t stream);

/* out[r] = sum over the destination rows i of relation r of x[Z row of segment (i, r)] for every relation the layer
 * computes, 0 for the others (x: one float per segment, e.g. KgwLayerArgs.da_dst).  The gradient of the per-relation
 * logit constant (KgwLayerArgs.logit_bias) is the sum of d pre-activation over all edges of the relation = this sum of
 * d a_dst.  One block per relation, fixed reduction tree.                                                          */
int kgw_relation_sums(const KgwLayerArgs* args, const float* x, float* out, kgw_stream_t stream);

/* Running totals over the batches of a captured training loop: stats[l] += edges aggregated by layer l+1 (l < n_layers),
 * stats[n_layers] += edges sampled, stats[n_layers+1] |= KgwBatchMeta.error.  stats: n_layers + 2 device int64.   */
int kgw_accumulate_stats(const KgwBatchMeta* meta_dev, int32_t n_layers, int32_t n_hops, int64_t* stats,
                         kgw_stream_t stream);
/* ... and, tick != NULL, advances that int32 by one in the same launch: the step counter of a kgw_adam_notick earlier in the
 * captured step (one single-thread launch less per step).                                                           */
int kgw_accumulate_stats_tick(const KgwBatchMeta* meta_dev, int32_t n_layers, int32_t n_hops, int64_t* stats, int32_t* tick,
                              kgw_stream_t stream);

/* A sampled batch kept for later epochs.  The reference's training loader has a fixed batch order (NeighborLoader without
 * shuffle, kgwas/kgwas.py:93-101), so epoch >= 2 asks the sampler for exactly the structures of epoch 1.  kgw_segments_copy moves
 * up to KGW_SEGCOPY_MAX device segments (the arrays of a KgwBatchBuf the training step reads) to slot *slot_index of a resident
 * cache (to_slot != 0) or back, in ONE launch; the slot index is read on the DEVICE, so one record serves every batch (the
 * trainer issues the launch eagerly on the sampler's stream, after an asynchronous copy of the index).  Pointers,
 * slot offsets and the stride are 16-byte aligned; units = 16-byte units of the segment.                                      */
#define KGW_SEGCOPY_MAX 40
typedef struct KgwSegCopy {
    int32_t n, to_slot;
    void* ptr[KGW_SEGCOPY_MAX];
    int64_t units[KGW_SEGCOPY_MAX];
    int64_t slot_off[KGW_SEGCOPY_MAX];
    uint8_t* slots;                  /* [n slots][slot_stride] */
    int64_t slot_stride;
    const int64_t* slot_index;       /* device */
} KgwSegCopy;
int kgw_segments_copy(const KgwSegCopy* plan, int32_t grid_blocks /* 0: default */, kgw_stream_t stream);

/* Replaces: the index_select feature slicing of the loader (x[n_id], kgwas/kgwas.py:135).      */
int kgw_gather_rows(const float* src, const int32_t* ids, int64_t n_rows, int32_t width,
                    float* dst, kgw_stream_t stream);
/* The same for up to 8 (src, ids, dst) jobs of one row width in a single launch (the three GO node
 * types' features go through one shared MLP as one matrix, kgwas/model.py:58-60).               */
int kgw_gather_rows_multi(int32_t n_jobs, const float* const* src, const int32_t* const* ids,
                          const int64_t* n_rows, int32_t width, float* const* dst, kgw_stream_t stream);

/* Backward of "rows n_id of relu(X W^T + b) computed on the RESIDENT feature matrix" (the wide gene layer,
 * kgwas/model.py:17-19 applied before the x[n_id] slicing of kgwas/kgwas.py:135): for every row of the resident
 * matrix dz[row] = g[g2l[row]] * (h[row] > 0) (zero where g2l[row] < 0: node not in the batch) and
 * colsum[c] = sum_row dz[row][c] (the bias gradient).  g [n_batch][128], h / dz [n_rows][128], g2l [n_rows];
 * workspace: kgw_scatter_relu_rows_workspace_floats(n_rows) floats.  Two launches, deterministic.        */
int64_t kgw_scatter_relu_rows_workspace_floats(int64_t n_rows);
int kgw_scatter_relu_rows(const float* g, const int32_t* g2l, const float* h, int64_t n_rows, float* dz,
                          float* colsum, float* workspace, kgw_stream_t stream);

/* alpha_e = exp(e - max)/den per local edge of one layer (attention export,
 * kgwas/conv.py:192-196; kgwas/utils.py:446-461).                                             */
int kgw_edge_alpha(const KgwLayerArgs* args, float* alpha_out, kgw_stream_t stream);

/* Edge attributes: GATConv(edge_dim = D) (kgwas/conv.py:46,95-101,207-215; the reference's HeteroGNN never passes it and its
 * load_kg keeps no edge evidence, so like the dropout and the gate this is an EXTENSION, off by default).  Every edge of an
 * attributed relation r carries D floats; a bias-free lin_edge [C, D] maps them to the hidden width and <lin_edge(attr_e), att_edge>
 * joins the attention logit BEFORE the LeakyReLU.  The messages do not change.  Re-associated the way u_r and v_r are:
 *      w_r      = lin_edge.weight^T att_edge                 in R^D          (formed by the caller; w [n_rels][8], stride 8)
 *      t_e      = sum_{d < D} A_r[p(e)][d] w_r[d]            fp32, fmaf, ascending d, starting from 0
 *      pre_e    = <x_j, u_r> + <x_i, v_r> (+ kappa_r) + t_e
 *      e_e      = leaky_relu(pre_e), then the softmax over the row of e / T, or (KGW_F_RAW_WEIGHTS) the raw weights -- unchanged
 *      d w_r[d] = sum_{e in r} d pre_e A_r[p(e)][d]          (no gradient to the attributes)
 * A_r [E_r][D]: row p belongs to entry p of relation r's dst-major CSR (the order of g_col: KgwGraph.col_off[r] + p; parallel edges
 * keep their own rows).  A relation without attributes (attr_off[r] < 0) has t_e = 0.  1 <= D <= 8, one D for all relations.
 * Where a local edge sits in the CSR is read from its chunk: gpos - col_off[rel] + (e - e0).  The chunks of a segment that a finite
 * fan-out DREW carry no position (gpos = -1): their terms are written as quiet NaN, so that misuse cannot pass silently.
 * The softmax still sums to one, and the backward kernels do not change: kgw_gat_aggregate_bwd_dst re-forms the weights from the
 * STORED logits and its adp[e] = (alpha_e, d pre_e) already holds the gradient of t_e.                                             */
typedef struct KgwEdgeAttr {
    const float* attr;               /* [sum of E_r over the attributed relations][dim], relation after relation               */
    int64_t attr_off[KGW_MAX_RELS];  /* first ROW of relation r inside attr; -1 = the relation has no attributes               */
    int32_t dim, pad_;               /* D                                                                                      */
    const float* w;                  /* [n_rels][8] w_r, zero beyond dim (rows of unattributed relations are not read)         */
    float* term;                     /* kgw_edge_term_fwd: [n_edges] t_e per local edge of the layer                           */
    const float* d_term;             /* kgw_edge_term_bwd: gradient of t_e, element e at d_term[e * d_term_stride] --          */
    int64_t d_term_stride;           /*   KgwLayerArgs.adp + 1 with stride 2 reads d pre_e in place                            */
    float* d_w;                      /* kgw_edge_term_bwd: [n_rels][8]; exact zeros for relations the layer does not compute,  */
                                     /*   for unattributed ones and beyond dim                                                 */
    float* workspace;                /* kgw_edge_term_bwd: kgw_edge_term_workspace_floats(args) floats                         */
} KgwEdgeAttr;
/* term[e] for every local edge of the layer (0.0f on relations without attributes or not live in the layer).  Reads of args:
 * layer, n_chunks, graph_host, meta_dev, chunks.  dim outside [1, 8]: KGW_E_RANGE.  One launch.                                 */
int kgw_edge_term_fwd(const KgwLayerArgs* args, const KgwEdgeAttr* ea, kgw_stream_t stream);
/* d_w from d_term and the attribute rows.  No float atomics, a fixed two-level order (per-chunk sums over a wavefront's fixed tree,
 * then one block per relation over its chunks, as part_du -> k_duv_fold): reruns are bit-identical.  Reads of args as above plus
 * n_multi_hops and seg_chptr.  Two launches.                                                                                   */
int kgw_edge_term_bwd(const KgwLayerArgs* args, const KgwEdgeAttr* ea, kgw_stream_t stream);
int64_t kgw_edge_term_workspace_floats(const KgwLayerArgs* args);
/* kgw_gat_aggregate_fwd with pre_e += term[e] (term: [n_edges], kgw_edge_term_fwd's): the softmax route, or with KGW_F_RAW_WEIGHTS
 * the raw weights of the attention export.  Hub rows, partial records and the combine are those of the plain call.  With
 * KGW_F_SIGMOID_GATE, n_heads > 1, drop_word_dev or partial_rels: KGW_E_UNSUPPORTED -- before any launch.                        */
int kgw_gat_aggregate_fwd_eterm(const KgwLayerArgs* args, const float* term, kgw_stream_t stream);

/* Where a gradient tensor's values are when its producer left the last reduction to the optimiser's launch
 * (kgw_adam_fused): DIRECT = in the gradient tensor itself; the other kinds = per-block partial sums in a workspace, added by
 * kgw_adam_fused in exactly the order the producer's own second launch (k_tn_reduce / k_mlp2_bwd_fold) uses -- bit-identical
 * gradients, one launch less per product.  Filled by kgw_tn_gemm_partial / kgw_tn_gemm_multi_partial /
 * kgw_mlp2_bwd_first_partial; the caller only carries the record to kgw_adam_fused.  (Weight / bias gradients of the Linears of
 * kgwas/model.py:13-21 on their way to the Adam update of kgwas/kgwas.py:116,151.)                                             */
enum { KGW_GRAD_DIRECT = 0, KGW_GRAD_TN = 1, KGW_GRAD_TN_COLSUM = 2, KGW_GRAD_MLP2_W = 3, KGW_GRAD_MLP2_B = 4, KGW_GRAD_G3T = 5 };
typedef struct KgwGradSrc {
    const float* ws;                 /* first partial record                                                     */
    int32_t kind, nblk;              /* KGW_GRAD_*; partial records per output element                           */
    int32_t M, N, MT, NT, gy, gz;    /* TN kinds: product shape and tiling; G3T: M = rows of the kgw_gemm3 product */
    int32_t K1, c_transposed;        /* MLP2 kinds: width of the first layer's input; TN: C stored transposed     */
    /* G3T only, set by the CALLER of kgw_adam_fused (NULL: off): the kgw_gemm3 operand image of the UPDATED parameter
     * ([128, M] = the B^T of the layer's forward product) is written by the same launch -- what kgw_gemm3_pack(S = parameter,
     * K = M, k_valid = M, s_is_kn = 0) would produce for the next forward, without that launch.                          */
    void* packed;
    int32_t flip, pad_;              /* sign period of the image in 32-k chunks (kgw_gemm3_flip()), 0 = none      */
} KgwGradSrc;

/* C[M,N] = A[rows,M]^T * B[rows,N] (row-major, leading dimensions lda/ldb/ldc), optionally
 * colsum_a[M] = column sums of A.  Split-K over the rows on fp32 MFMA, deterministic.  Replaces the
 * weight / bias gradient GEMMs autograd runs for the Linear layers of the path
 * (kgwas/model.py:13-21,50; kgwas/conv.py:82-89,150-151) whose reduction dimension is the number of
 * sampled nodes.  workspace: kgw_tn_gemm_workspace_floats(rows, M, N) floats.                    */
int64_t kgw_tn_gemm_workspace_floats(int64_t rows, int32_t M, int32_t N);
/* One product of kgw_tn_gemm_multi: the arguments of kgw_tn_gemm_ex as a record.                  */
typedef struct KgwTnJob {
    const float* A; int64_t lda; const float* B; int64_t ldb;
    int64_t rows;
    float* C; int64_t ldc;
    float* colsum_a; int64_t colsum_ld;
    float* workspace; int64_t workspace_floats;
    const int32_t* rows_dev;
    int32_t M, N, c_transposed, colsum_repeat;
} KgwTnJob;
/* Up to 4 such products in ONE pair of launches (the weight / bias gradients of the Linears of one
 * MLP, kgwas/model.py:17-21, become available together at the end of its backward).  Needs even M, N,
 * lda, ldb and 8-byte aligned A, B (else KGW_E_UNSUPPORTED: use kgw_tn_gemm_ex per product).        */
int kgw_tn_gemm_multi(int32_t n_jobs, const KgwTnJob* jobs, kgw_stream_t stream);
int kgw_tn_gemm(const float* A, int64_t lda, int32_t M, const float* B, int64_t ldb, int32_t N,
                int64_t rows, float* C, int64_t ldc, float* colsum_a, float* workspace,
                int64_t workspace_floats, kgw_stream_t stream);
/* Same product with two output options that let the gradient land where the caller keeps it (no copy / reduce
 * launches afterwards): c_transposed != 0 stores C^T, i.e. element (m,n) at C[n*ldc + m] (the packed per-relation
 * weights are kept transposed, [in, out]); colsum_a is written colsum_repeat times, copy q at
 * colsum_a + q*colsum_ld (the bias gradient of every relation summed into one destination type is the same
 * vector: HeteroConv sum, kgwas/model.py:74).  rows_dev (nullable, device int32): actual row count <= rows (static
 * capacity of a captured step); only those rows are read.                                                   */
int kgw_tn_gemm_ex(const float* A, int64_t lda, int32_t M, const float* B, int64_t ldb, int32_t N,
                   int64_t rows, float* C, int64_t ldc, int32_t c_transposed, float* colsum_a,
                   int32_t colsum_repeat, int64_t colsum_ld, float* workspace, int64_t workspace_floats,
                   const int32_t* rows_dev, kgw_stream_t stream);

/* The first launch of kgw_tn_gemm_ex / kgw_tn_gemm_multi only (colsum_repeat 1, dense C): src[0] / src[1] (per job: src[2q],
 * src[2q + 1]) describe the partial sums of the product / of the column sums for kgw_adam_fused; C and colsum_a are the
 * gradient tensors that launch will also fill.                                                                            */
int kgw_tn_gemm_partial(const float* A, int64_t lda, int32_t M, const float* B, int64_t ldb, int32_t N,
                        int64_t rows, float* C, int64_t ldc, int32_t c_transposed, float* colsum_a,
                        float* workspace, int64_t workspace_floats, const int32_t* rows_dev, KgwGradSrc* src,
                        kgw_stream_t stream);
int kgw_tn_gemm_multi_partial(int32_t n_jobs, const KgwTnJob* jobs, KgwGradSrc* src, kgw_stream_t stream);
/* The products that run on the 64 x 64-per-wavefront tiling (M, N, lda, ldb even, 8-byte aligned operands: every weight-gradient
 * product of the step but the narrow ones) use the BF16 matrix pipe with fp32 error since round 5: each operand value is split
 * exactly into three bf16 pieces and the six piece products of weight >= 2^-16 are accumulated in fp32 (the scheme of kgw_gemm3;
 * the dropped products are below the rounding of one fp32 multiply-add), 24 MFMAs of 32 cycles per 16 rows against 32 of 64 on
 * the fp32 pipe.  kgw_tn_split(0 / 1) selects the fp32 / bf16 pipe for later calls and returns the previous setting (< 0: query);
 * the environment variable KGW_TN_SPLIT=0 sets the initial value.                                                              */
int kgw_tn_split(int on);
/* Products of up to this many rows (and at least 16 output tiles) run as ONE row block whose blocks write the result directly: no
 * partial slabs, no second launch.  Default 0 (never): measured -3 us per step and one launch less at 2 048, but a wavefront's
 * seven-times longer sum then shows twice the error of the row-blocked form (on either pipe).  Sets the limit for later calls
 * (< 0: query), returns the previous one; KGW_TN_DIRECT_ROWS sets the initial value.                                           */
int64_t kgw_tn_direct_rows(int64_t rows);

/* A product group's SECOND launch (the sums over its row blocks: k_tn_reduce) that has not been issued.  The gradients it
 * finishes -- the relation transform's d W^T / d bias, kgwas/conv.py:138,190 -- feed nothing before the end of the backward pass,
 * so in a captured step its few blocks ride in a later launch instead of being one of their own (5 - 8 us each):
 *   kgw_transform_bwd_ex(.., ride_in, defer_out, ..)  kgw_transform_bwd that (ride_in, nullable) carries a pending plan's blocks
 *                                                      and (defer_out, nullable) leaves its own second launch as a plan;
 *   kgw_tn_gemm_partial_ride(.., ride_in, ..)          kgw_tn_gemm_partial that carries a pending plan's blocks;
 *   kgw_tn_reduce_launch(plan)                          the plan as a launch of its own (nothing came by to carry it).
 * Same blocks, same code, same order of additions wherever they run.  plan->valid == 0: nothing pending (a group whose products
 * all had one row block).  The plan points into the products' workspaces and outputs: keep them alive until it has run.
 * Riding pays for a SMALL plan only: the blocks take the carrier kernel's registers and LDS, so a carrier built for one or two
 * blocks per CU runs thousands of them a few at a time (measured: layer 1's 9 088 blocks in the SNP product's launch, 78 us against
 * 8 + 47 apart) -- ``blocks`` is there for the caller to decide.                                                               */
/* The read-out node's SECOND launch in a training step (kgw_readout_wmse_train: the single-block fold of the per-block partial sums
 * into d w_lin, d b_lin and the loss), not issued: nothing reads the three before the optimiser / the host, so in a captured step the
 * fold is one more block of the launch that follows (kgw_transform_bwd_ex's fold_in) instead of a 5 us launch of one block.
 * Filled by kgw_readout_wmse_train_parts; kgw_readout_train_fold runs it as a launch of its own.                                */
typedef struct KgwReadoutFold {
    const float* scratch; const double* terms; float* dw_lin; float* db_lin; double* loss;
    int32_t nb, n;
} KgwReadoutFold;

typedef struct KgwTnReducePlan { int32_t valid; int32_t blocks /* 256-thread blocks of the launch */; int32_t reserved[2]; int64_t opaque[96]; } KgwTnReducePlan;
int kgw_tn_reduce_launch(const KgwTnReducePlan* plan, kgw_stream_t stream);
int kgw_tn_gemm_partial_ride(const float* A, int64_t lda, int32_t M, const float* B, int64_t ldb, int32_t N, int64_t rows,
                             float* C, int64_t ldc, int32_t c_transposed, float* colsum_a, float* workspace,
                             int64_t workspace_floats, const int32_t* rows_dev, KgwGradSrc* src, const KgwTnReducePlan* ride_in,
                             kgw_stream_t stream);

/* Y[rows,N] = act(X[rows,K] * Wop + bias) * (mask > 0): the Linear layers of the path on fp32 MFMA.
 * w_is_kn = 0: W is [N,K] (nn.Linear / PyG Linear forward, kgwas/model.py:13-21,50; kgwas/conv.py:138,142);
 * w_is_kn = 1: W is [K,N] (the dX = dY * W product of their backward).  bias, mask may be NULL; relu 0/1.
 * K, ldx, ldw (and N when w_is_kn) must be multiples of 4, X and W 16-byte aligned, else KGW_E_UNSUPPORTED.
 * rows_dev (nullable, device int32): the number of rows the batch really has when `rows` is the static capacity of a
 * captured step (KgwBatchMeta.n_src / n_rows entry): rows [*rows_dev, rows) are not computed, Y gets zeros there. */
int kgw_linear(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias,
               const float* mask, int64_t ldm, float* Y, int64_t ldy, int64_t rows, int32_t K, int32_t N,
               int32_t relu, int32_t w_is_kn, const int32_t* rows_dev, kgw_stream_t stream);

/* SimpleMLP's two hidden layers (kgwas/model.py:17-20) for a NARROW input in one launch:
 * H2 = relu(relu(X W1^T + b1) W2^T + b2), X [rows, K1] with K1 <= 20 and K1 % 4 == 0 (the 20-wide SNP features), W1 [128, K1],
 * W2 [128, 128] (nn.Linear layout), hidden width 128.  The hidden state goes from the first product's accumulators straight
 * into the second product's operand registers; it is ALSO written to H1 (nullable) for the backward, which reads it as the
 * ReLU mask and in the weight gradient.  rows_dev: see kgw_linear.  ids (nullable): input row r is X[ids[r]] -- the
 * loader's x[n_id] slicing (kgwas/kgwas.py:135) folded in; Xg (nullable) then receives the gathered rows [rows, K1] for the
 * backward's first-layer weight gradient.                                                                          */
int kgw_mlp2_fwd(const float* X, int64_t ldx, int32_t K1, const float* W1, int64_t ldw1, const float* b1, const float* W2,
                 int64_t ldw2, const float* b2, float* H1, int64_t ldh1, float* H2, int64_t ldh2, int64_t rows,
                 const int32_t* rows_dev, const int32_t* ids, float* Xg, int64_t ldxg, kgw_stream_t stream);

/* The same two layers for a 128-WIDE input on few rows, the rows gathered from up to four resident feature matrices
 * (src[j] [*, 128] with row stride ldx, ids[j] [n_rows[j]]: the three GO node types share go_feat_mlp, kgwas/model.py:58-60):
 * rows of job 0, then job 1, ...  Outputs [sum n_rows, 128] with row stride ldo: Xg = the gathered input rows, H1, H2.    */
int kgw_mlp2w_fwd(int32_t n_jobs, const float* const* src, const int32_t* const* ids, const int64_t* n_rows, int64_t ldx,
                  const float* W1, int64_t ldw1, const float* b1, const float* W2, int64_t ldw2, const float* b2, float* Xg,
                  float* H1, float* H2, int64_t ldo, kgw_stream_t stream);

/* Backward of the NARROW first layer behind kgw_mlp2_fwd (no input gradient wanted): d W1 [128, K1] (row stride ldw1) and
 * d b1 [128] of  h1 = relu(x W1^T + b1)  given the upstream dH2 [rows, 128] of h2 = relu(h1 W2^T + b2) (already multiplied
 * by h2 > 0), W2, h1 and x [rows, K1 <= 31]: dh1 = (dH2 W2) * (h1 > 0) is formed tile by tile and consumed in place by the
 * d W1 product -- never written.  workspace: kgw_mlp2_bwd_first_workspace_floats(rows) floats.
 * Variant for a WIDE first layer computed on a resident feature matrix (the gene layer): in_ids [rows] (row r of the product
 * reads dH2[in_ids[r]], < 0: the node is not in the batch, its dh1 row is zero), dZ [rows, 128] receives the masked dh1 rows
 * (the layer's own weight gradient is a library product over them) and K1 = 0 leaves only d b1 (X, dW1 unused).
 * rows_dev (see kgw_linear): rows [*rows_dev, rows) take no part in d W1 / d b1 and are not read; dZ rows at and past
 * *rows_dev are NOT written -- they keep what the buffer held (unlike kgw_linear's Y, which gets zeros there).           */
int64_t kgw_mlp2_bwd_first_workspace_floats(int64_t rows);
int kgw_mlp2_bwd_first(const float* dH2, int64_t ldd, const float* W2, int64_t ldw2, const float* H1, int64_t ldh1,
                       const float* X, int64_t ldx, int32_t K1, int64_t rows, const int32_t* rows_dev, float* dW1,
                       int64_t ldw1, float* db1, float* workspace, int64_t workspace_floats, const int32_t* in_ids, float* dZ,
                       int64_t ldz, kgw_stream_t stream);

/* The same without the second launch (the fold of the blocks' partial d W1 / d b1): src[0] describes d W1's partial sums,
 * src[1] d b1's, for kgw_adam_fused (ldw1 must be K1: a dense gradient tensor).                                             */
int kgw_mlp2_bwd_first_partial(const float* dH2, int64_t ldd, const float* W2, int64_t ldw2, const float* H1, int64_t ldh1,
                               const float* X, int64_t ldx, int32_t K1, int64_t rows, const int32_t* rows_dev, float* dW1,
                               int64_t ldw1, float* db1, float* workspace, int64_t workspace_floats, const int32_t* in_ids,
                               float* dZ, int64_t ldz, KgwGradSrc* src, kgw_stream_t stream);
/* ... that ALSO writes the masked dh1 rows as kgw_gemm3's B operand image (packed: kgw_gemm3_packed_bytes(rows rounded up to 32)
 * bytes, the s_is_kn form of kgw_gemm3_pack; flip = kgw_gemm3_flip()): the resident first layer's weight gradient
 * (kgwas/model.py:13 under loss.backward(), dW1 = dh1^T X on kgw_gemm3) then needs neither the kgw_gemm3_pack launch nor the fp32
 * rows -- dZ may be null.  src nullable (null: the fold launch runs here).  KGW_E_UNSUPPORTED: the fp32-pipe variant is selected.  */
int kgw_mlp2_bwd_first_packed(const float* dH2, int64_t ldd, const float* W2, int64_t ldw2, const float* H1, int64_t ldh1,
                              const float* X, int64_t ldx, int32_t K1, int64_t rows, float* dW1, int64_t ldw1, float* db1,
                              float* workspace, int64_t workspace_floats, const int32_t* in_ids, float* dZ, int64_t ldz,
                              void* packed, int32_t flip, KgwGradSrc* src, kgw_stream_t stream);

/* C[M, 128] = A[M, K] B[K, 128] for a tall RESIDENT fp32 matrix A -- the first gene Linear, kgwas/model.py:13,19 over the
 * 5 120-wide gene features (kgwas_data.py:236,244): forward with A = X [genes, K], B = W1^T (out = relu(C + bias)), and its
 * weight gradient with A = X^T [K, genes], B = dz (transpose_out: out[n, m] = C[m, n], i.e. dW1 [128, K]).  Runs on the bf16
 * matrix pipe with fp32 error: every fp32 operand is split exactly into three bf16 pieces and the six piece products of
 * weight >= 2^-16 are accumulated in fp32; the dropped products are below the rounding of one fp32 multiply-add (see
 * kgwas_amd/csrc/kgw_gemm3.hip).  kgw_gemm3_pack splits B once per call into the kernel's operand image (packed:
 * kgw_gemm3_packed_bytes(K) bytes; s_is_kn: B[k, n] = S[k * lds + n], else B[k, n] = S[n * lds + k], n < 128; S holds
 * k < k_valid only, B[k >= k_valid] = 0: a gene count / feature width that is not a multiple of 32 is padded HERE and in a
 * zero-padded resident A, never by falling back to a library product).  A is split in
 * the kernel.  lda == 0: A is stored in 32 x 32 tiles, [ceil(M / 32)][K / 32][32][32] floats (rows past M present, any value) --
 * the layout for a resident copy, every 4 KB a wavefront reads per step is contiguous.  lda < 0: A is the OPERAND IMAGE, per
 * 32-row tile t and 32-k chunk c 1 024 floats at A[t * (-lda) + c * 1024], float4 q * 64 + l (q < 4, l < 64) holding row
 * 32 t + l % 32, k = 32 c + 16 (q / 2) + 8 (l / 32) + 4 (q % 2) + 0..3 (rows past M present, any value; -lda a multiple of
 * 1 024 and >= K * 32) -- loaded straight into the kernel's operand registers; same results, bit for bit, as row-major A.
 * Also for kgw_gemm3_partial and kgw_gemm3_riders.  K % 32 == 0, lda % 4 == 0, 16-byte aligned pointers, else
 * KGW_E_UNSUPPORTED.  workspace:
 * kgw_gemm3_workspace_floats(M, K) floats (partial products of the K ranges, added in index order: deterministic).      */
int64_t kgw_gemm3_packed_bytes(int64_t K);
int64_t kgw_gemm3_workspace_floats(int64_t M, int64_t K);
int kgw_gemm3_pack(const float* S, int64_t lds, int64_t K, int64_t k_valid, int32_t s_is_kn, void* packed, kgw_stream_t stream);
int kgw_gemm3(const float* A, int64_t lda, int64_t M, int64_t K, const void* packed, float* workspace, int64_t workspace_floats,
              const float* bias, int32_t relu, float* out, int64_t ldo, int32_t transpose_out, const int32_t* row_map,
              float* out_rows, int64_t ld_rows, int64_t out_rows_n, const int32_t* out_rows_real, kgw_stream_t stream);
/* row_map (nullable, not with transpose_out) [M]: row m of the result is ALSO written to out_rows[row_map[m]] when
 * row_map[m] >= 0 -- the loader's x[n_id] slicing of the layer's output (kgwas/kgwas.py:135) without a gather launch.
 * out_rows_real (nullable, device int32) with out_rows_n (<= M): out_rows is a row block of out_rows_n rows of which only the
 * first *out_rows_real are the batch's (static capacity of a captured step); the rest is written as zeros by the same launch. */

/* The same product for FEW rows when one of K, N is 128 and the other a multiple of 128 -- the per-relation transform
 * of a layer after aggregate-then-transform, [N_dst, R*128] x [R*128, 128] with N_dst ~ 0.5-1.2 k destination rows of a
 * 512-seed batch (kgwas/conv.py:138-144 for all relations into one destination type + bias :190 + HeteroConv sum
 * model.py:74 + ReLU :75), and its dZ twin [N_dst, 128] x [128, R*128]: the long dimension is cut into 128-wide slabs
 * (= relations); a block keeps its slab's 128 x 128 weights stationary in MFMA operand registers and streams 32-row
 * tiles through LDS; K slabs are added in order by a second launch (deterministic).  workspace:
 * kgw_linear_splitk_workspace_floats floats (0 when K == 128).  Other shapes: KGW_E_UNSUPPORTED (use kgw_linear).   */
int64_t kgw_linear_splitk_workspace_floats(int64_t rows, int32_t K, int32_t N);
int kgw_linear_splitk(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, float* Y,
                      int64_t ldy, int64_t rows, int32_t K, int32_t N, int32_t relu, int32_t w_is_kn,
                      float* workspace, int64_t workspace_floats, const int32_t* rows_dev, kgw_stream_t stream);
/* The forward transform (N == 128, K = R*128) with a per-segment constant: Y[i] = act(X[i] W + bias + sum_r ind(i, r)
 * gamma[r]), ind(i, r) = seg_stat[2 (i R + r) + 1] > 0 -- segment (destination row i, relation slot r) has at least one
 * edge (its softmax denominator as kgw_gat_aggregate_fwd left it).  With FC_output folded into layer 1 the aggregate
 * works on the MLP's hidden state h2 and the bias c of the folded Linear re-enters as c W_r wherever the attention
 * weights of a segment sum to 1, i.e. wherever it is not empty.  gamma [R][128].  kgw_ind_colsum is the backward:
 * dgamma[r] = sum_i ind(i, r) dY[i]  (one block per relation slot, rows added in order: deterministic).           */
int kgw_linear_splitk_ind(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, float* Y,
                          int64_t ldy, int64_t rows, int32_t K, int32_t relu, const float* seg_stat, const float* gamma,
                          float* workspace, int64_t workspace_floats, const int32_t* rows_dev, kgw_stream_t stream);
int kgw_ind_colsum(const float* seg_stat, const float* dY, int64_t ldy, int64_t rows, int32_t R, float* dgamma,
                   kgw_stream_t stream);
/* One product of kgw_linear_splitk_multi / one sum of kgw_ind_colsum_multi: the arguments above as a record.  A layer has one
 * transform per DESTINATION TYPE (kgwas/model.py:74: HeteroConv sums the relations into each type) -- genes and seed SNPs in
 * layer 1 of a 512-seed batch -- and each of them is a problem of a few hundred rows that leaves most of the chip idle: all of
 * a layer's forward transforms go in ONE launch, all its dZ twins in one, all its d gamma sums in one.                        */
typedef struct KgwSplitKJob {
    const float* X; int64_t ldx;
    const float* W; int64_t ldw;
    const float* bias;            /* nullable */
    float* Y; int64_t ldy;
    int64_t rows;
    const float* seg_stat;        /* forward with a per-segment constant (kgw_linear_splitk_ind), else NULL; for
                                     kgw_ind_colsum_multi: the segment statistics (required)                       */
    const float* gamma;           /* with seg_stat (forward); kgw_ind_colsum_multi: unused                       */
    float* dgamma;                /* kgw_ind_colsum_multi: output [K / 128][128]; X / W / bias / gamma unused, Y = dY */
    int32_t K, N, relu, w_is_kn;
} KgwSplitKJob;
/* Up to 4 products in one launch.  Every job must be of the SAME kind: either the forward transform (K > 128 a multiple of
 * 128, N == 128, w_is_kn = 1: what kgw_linear_splitk / _ind run as ONE launch) or the dZ twin (K == 128, N a multiple of 128,
 * no seg_stat); anything else: KGW_E_UNSUPPORTED (use the single-product calls).                                           */
int kgw_linear_splitk_multi(int32_t n_jobs, const KgwSplitKJob* jobs, kgw_stream_t stream);
/* dgamma of up to 4 transforms in one launch (job: seg_stat, Y = dY, ldy, rows, K = R * 128, dgamma).                        */
int kgw_ind_colsum_multi(int32_t n_jobs, const KgwSplitKJob* jobs, kgw_stream_t stream);

/* The backward of a layer's relation transform (kgwas/conv.py:138-144,190 + kgwas/model.py:74-75 under loss.backward()) in ONE
 * launch (+ the split-K products' second): everything that is a function of d(output) alone -- the weight / bias gradients of
 * every destination type (tn_jobs: the records of kgw_tn_gemm_multi), the dZ twins (sk_jobs: kgw_linear_splitk_multi's K == 128
 * records with [N, K] weights) and the d gamma sums of a folded layer (cs_jobs: kgw_ind_colsum_multi's records) -- as blocks of
 * one grid; values identical to the three separate calls.  Any of the three lists may be empty.                              */
int kgw_transform_bwd(int32_t n_tn, const KgwTnJob* tn_jobs, int32_t n_sk, const KgwSplitKJob* sk_jobs, int32_t n_cs,
                      const KgwSplitKJob* cs_jobs, kgw_stream_t stream);
/* ... with the pending second launch of an EARLIER product group riding as extra blocks (ride_in) and / or this call's own second
 * launch left pending (defer_out): see KgwTnReducePlan.                                                                         */
int kgw_transform_bwd_ex(int32_t n_tn, const KgwTnJob* tn_jobs, int32_t n_sk, const KgwSplitKJob* sk_jobs, int32_t n_cs,
                         const KgwSplitKJob* cs_jobs, const KgwTnReducePlan* ride_in, KgwTnReducePlan* defer_out,
                         const KgwReadoutFold* fold_in /* nullable: see KgwReadoutFold */, kgw_stream_t stream);

/* One Adam step (torch.optim.Adam semantics, weight_decay as L2: kgwas/kgwas.py:116,151) over up to 64
 * parameter tensors in a single launch.  The pointer arrays are HOST arrays of device pointers (passed to the
 * kernel by value); step_dev is a device int32 counter incremented by the call (graph-capturable).        */
int kgw_adam(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
             float* const* exp_avg_sq, const int64_t* numel, int32_t* step_dev, float lr, float beta1,
             float beta2, float eps, float weight_decay, kgw_stream_t stream);
/* The same, leaving *step_dev alone: the caller advances it after this call (kgw_accumulate_stats_tick).            */
int kgw_adam_notick(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const int64_t* numel, int32_t* step_dev, float lr, float beta1,
                    float beta2, float eps, float weight_decay, kgw_stream_t stream);

/* The weight-gradient form of kgw_gemm3 (transpose_out: out [128, M], ldo == M, M a multiple of 32) without its range-sum
 * launch: src describes the K ranges' partial products for kgw_adam_fused.  kgw_gemm3_flip(): the sign period kgw_gemm3_pack
 * builds its images with (KgwGradSrc.flip).                                                                                */
int kgw_gemm3_partial(const float* A, int64_t lda, int64_t M, int64_t K, const void* packed, float* workspace,
                      int64_t workspace_floats, float* out, int64_t ldo, KgwGradSrc* src, kgw_stream_t stream);
int kgw_gemm3_flip(void);

/* The optimiser launch of a captured training step: kgw_adam_notick over up to KGW_ADAM_FUSED_MAX tensors, and in the SAME launch
 * (a) the last reduction of every gradient whose producer left partial sums (src[i].kind != KGW_GRAD_DIRECT, at most
 *     KGW_ADAM_FUSED_SRC of them; src == NULL: all direct) -- the sums are taken in the producers' own order and also written
 *     to grads[i], so the gradient tensors hold what the unfused path leaves in them;
 * (b) kgw_accumulate_stats_tick (meta_dev != NULL: the running totals; the step counter advances in any case) -- done by the
 *     block that finishes last (done_counters: KGW_ADAM_FUSED_COUNTERS device int32 the caller zeroes once; the launch leaves
 *     them at zero).                                                                                                         */
enum { KGW_ADAM_FUSED_MAX = 40, KGW_ADAM_FUSED_SRC = 12, KGW_ADAM_FUSED_COUNTERS = 65 * 32 };
int kgw_adam_fused(int32_t n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const int64_t* numel, const KgwGradSrc* src, int32_t* step_dev, float lr,
                   float beta1, float beta2, float eps, float weight_decay, const KgwBatchMeta* meta_dev, int32_t n_layers,
                   int32_t n_hops, int64_t* stats, int32_t* done_counters, kgw_stream_t stream);

/* The same work units WITHOUT the update, for the multi-GPU step (the ranks' gradients must be complete before the all-reduce):
 * dst[i] (the tensor's slot in a flat gradient bucket) = the finished gradient of tensor i -- a copy of grads[i] where src[i] is
 * KGW_GRAD_DIRECT (or src NULL), the sum of the producer's partial records otherwise (then also stored into grads[i]).  One launch
 * instead of the producers' second launches + the bucket's concatenation.                                                      */
int kgw_grad_finish(int32_t n_tensors, float* const* dst, float* const* grads, const int64_t* numel, const KgwGradSrc* src,
                    kgw_stream_t stream);

/* Optimiser controls (EXTENSIONS, see KgwLrSchedule above): a learning-rate schedule evaluated inside the Adam kernels and a
 * clipping coefficient read from device memory.  New entry points only: the calls above keep their signatures and their bits, and
 * the kernels behind them are the instantiations without the controls.  The feature is detected by symbol (the version stays).
 *   sched           every thread forms lr_t = kgwlr_at(&sched, lr, t) from the t it loaded for the bias corrections.
 *   grad_scale_dev  nullable device float: the gradient element is g * scale BEFORE + weight_decay * p -- torch's order, where
 *                   clip_grad_norm_ scales and Adam then adds the L2 term.  The gradient TENSORS are left unscaled: unlike torch's
 *                   in-place clip, p.grad after the step is what the backward pass wrote.
 *   lr_out_dev      nullable device float: thread 0 of block 0 stores lr_t there.
 * kgw_adam_ctl: kgw_adam_notick's arguments, tick (non-zero: advance *step_dev afterwards like kgw_adam) and ctl.
 * kgw_adam_fused_ctl: kgw_adam_fused's arguments and ctl; grad_scale_dev != NULL: KGW_E_UNSUPPORTED (a deferred gradient is only
 * finished inside the launch, so no norm of it exists before it -- clipping takes the unfused route).
 * ctl == NULL forwards to the call without controls.  A schedule kgwlr_valid refuses: KGW_E_RANGE.  Both before any launch.      */
typedef struct KgwOptimCtl {
    KgwLrSchedule sched;
    const float* grad_scale_dev;
    float* lr_out_dev;
} KgwOptimCtl;
int kgw_adam_ctl(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, const int64_t* numel, int32_t* step_dev, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int32_t tick, const KgwOptimCtl* ctl, kgw_stream_t stream);
int kgw_adam_fused_ctl(int32_t n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const int64_t* numel, const KgwGradSrc* src, int32_t* step_dev, float lr,
                       float beta1, float beta2, float eps, float weight_decay, const KgwBatchMeta* meta_dev, int32_t n_layers,
                       int32_t n_hops, int64_t* stats, int32_t* done_counters, const KgwOptimCtl* ctl, kgw_stream_t stream);
/* Host evaluation of the rule (bindings, tests): (double)kgwlr_at(sched, lr, t); NaN for a NULL or refused schedule.            */
double kgw_lr_at(const KgwLrSchedule* sched, float lr, int32_t t);

/* Global gradient norm and torch.nn.utils.clip_grad_norm_'s coefficient (norm_type 2), in two launches without atomics:
 *   kgw_grad_norm_partial   one float64 sum of squares per work unit of KGW_GRAD_NORM_UNIT consecutive elements of ONE tensor, into
 *                           partial[partial_offset + unit] (units numbered tensor after tensor; a tensor of n elements has
 *                           ceil(n / unit) of them).  Inside a unit every thread squares and adds its four elements in double and
 *                           the 256 threads' sums meet in a fixed binary tree: a unit's value depends on its elements alone.  Up to
 *                           64 tensors per call; more tensors: further calls with the offset moved on.
 *   kgw_grad_norm_fold      one block; one thread adds partial[0 .. count) in index order, norm = sqrt(sum) in double, and
 *                           c = max_norm / (norm + 1e-6), scale = (float)(c >= 1 ? 1 : c).  *norm_out_dev (nullable) = (float)norm.
 * Reruns give equal bits.  All-zero gradients: norm 0, scale exactly 1.  A NaN norm gives a NaN scale and an infinite norm the
 * scale 0 (whose product with the infinite element is NaN): in both cases the update is not finite -- torch's default
 * (error_if_nonfinite=False) does the same; nothing is skipped.  kgw_grad_norm_workspace_doubles: the units of n_tensors tensors =
 * the doubles ``partial`` needs for them.  Refused before any launch: a NULL table, tensor or output: KGW_E_NULL; n_tensors outside
 * [0, 64], a negative numel or offset, count < 1, max_norm not finite or <= 0: KGW_E_RANGE.                                      */
#define KGW_GRAD_NORM_UNIT 1024
int64_t kgw_grad_norm_workspace_doubles(int32_t n_tensors, const int64_t* numel);
int kgw_grad_norm_partial(int32_t n_tensors, const float* const* grads, const int64_t* numel, double* partial,
                          int64_t partial_offset, kgw_stream_t stream);
int kgw_grad_norm_fold(const double* partial, int64_t count, double max_norm, float* norm_out_dev, float* scale_out_dev,
                       kgw_stream_t stream);

/* Weight averaging (an EXTENSION, the rule: KgwWeightAvg above): shadow[i] of up to KGW_WEIGHT_AVG_MAX tensors moves towards
 * params[i] in ONE launch that follows the optimiser's -- after the launch that advanced *step_dev, which this one never does.
 * Every wavefront loads n = *step_dev once (a wave-uniform load) and evaluates kgwavg_alpha: a non-event ends it there, so the
 * launch stays in a captured graph and touches nothing but the counter.  On an event a work unit is KGW_WEIGHT_AVG_UNIT consecutive
 * elements of ONE tensor (float4 where both pointers are 16-byte aligned, the tensor's tail and unaligned tensors element by
 * element); s = fmaf(alpha, p - s, s), with alpha == 1 the bits of p.  Element-wise, no LDS, no atomics: every mapping gives the
 * same bits.  More tensors: further calls.  shadow[i] and params[i] must not overlap.  Refused before any launch: a NULL table,
 * tensor, counter or cfg: KGW_E_NULL; n_tensors outside [0, 64] or a negative numel: KGW_E_RANGE; a cfg kgwavg_valid refuses:
 * KGW_E_RANGE.  The feature is detected by symbol (the version stays).
 * kgw_weight_avg_alpha: host evaluation of the rule (bindings, tests): *event (nullable) = kgwavg_alpha's result, the return value
 * its alpha (0 on a non-event); NaN and *event = 0 for a NULL or refused cfg or n < 1.                                             */
#define KGW_WEIGHT_AVG_MAX 64
#define KGW_WEIGHT_AVG_UNIT 1024
int kgw_weight_avg_update(int32_t n_tensors, float* const* shadow, const float* const* params, const int64_t* numel,
                          const int32_t* step_dev, const KgwWeightAvg* cfg, kgw_stream_t stream);
float kgw_weight_avg_alpha(const KgwWeightAvg* cfg, int32_t n, int32_t* event);

/* Attention vectors of all relations of a layer (kgwas/conv.py:138-151 reduced to what the path consumes):
 * U_full[r] = W_src^T att_src for every relation id r the layer computes (live_of_rel[r] = its index i in the
 * packed parameter arrays, -1 => row of zeros), V[i] = W_dst^T att_dst (bip_pos[i] >= 0: index into w_dst_t) or
 * W_src^T att_dst (same-type relation).  Packed weights are transposed: w_*_t[i][k][c] = W_i[c][k], C = 128.
 * v_by_rel != 0: V / dV are [n_rels_total][128] indexed by relation id like U_full (zero rows for relations the
 * layer does not compute) -- the form kgw_gat_aggregate_* consume.
 * Optional (bias != NULL): bias_sum[b] = sum of bias[i] over the packed relations i with blk_of_live[i] == b, the
 * bias of the relation-summed output of destination block b (HeteroConv sum of conv.py:190's bias, model.py:74).
 * Optional (zero_buf != NULL): zero_floats (multiple of 4) floats at zero_buf are cleared by extra blocks of the same
 * launch -- the Z / stat / d a_dst workspace of the kgw_gat_aggregate_fwd call that follows (it needs them zeroed).
 * _bwd: gradients of the packed parameters from (dU_full, dV); every output element is written.          */
int kgw_relvec_fwd(int32_t n_rels_total, const int32_t* live_of_rel, const int32_t* bip_pos, const float* w_src_t,
                   const float* w_dst_t, const float* att_src, const float* att_dst, float* U_full, float* V,
                   int32_t v_by_rel, int32_t n_live, const float* bias, const int32_t* blk_of_live, int32_t n_blk,
                   float* bias_sum, float* zero_buf, int64_t zero_floats, kgw_stream_t stream);
int kgw_relvec_bwd(int32_t n_live, const int32_t* rel_ids, const int32_t* bip_pos, const float* w_src_t,
                   const float* w_dst_t, const float* att_src, const float* att_dst, const float* dU_full,
                   const float* dV, float* dw_src_t, float* dw_dst_t, float* datt_src, float* datt_dst,
                   int32_t v_by_rel, kgw_stream_t stream);
/* The relation vectors of SEVERAL layers in one launch (and their backward in one): they depend on the parameters only, a
 * model has one pack per layer (kgwas/model.py:47: one HeteroConv per layer), and each launch is ~30 blocks of latency.  A job =
 * the arguments of kgw_relvec_fwd (v_by_rel = 1) / kgw_relvec_bwd_acc as a record; the forward reads the first group of fields,
 * the backward the second.  Up to KGW_MAX_LAYERS jobs.                                                                  */
typedef struct KgwRelvecJob {
    int32_t n_rels_total, n_live, n_blk;
    int32_t duv_pieces;              /* backward, != 0: dU_full / dV point at [rows][8][128] pieces (KGW_F_DUV_PIECES), added here
                                        in k_duv_fold's order                                                                 */
    const int32_t* live_of_rel; const int32_t* rel_ids; const int32_t* bip_pos;
    const float* w_src_t; const float* w_dst_t; const float* att_src; const float* att_dst;
    /* forward */
    float* U_full; float* V; const float* bias; const int32_t* blk_of_live; float* bias_sum;
    float* zero_buf; int64_t zero_floats;
    /* backward (dU_full / dV / dw_src_acc nullable = zero) */
    const float* dU_full; const float* dV; const float* dw_src_acc;
    float* dw_src_t; float* dw_dst_t; float* datt_src; float* datt_dst;
} KgwRelvecJob;
int kgw_relvec_fwd_multi(int32_t n_jobs, const KgwRelvecJob* jobs, kgw_stream_t stream);
int kgw_relvec_bwd_multi(int32_t n_jobs, const KgwRelvecJob* jobs, kgw_stream_t stream);
/* _bwd_acc: the same with (a) dw_src_acc (nullable): a gradient of w_src_t that reached the caller by another path -- the
 * layer's transform GEMM (conv.py:138-144) or the FC_output fold use the same weights -- and is added into dw_src_t here
 * instead of by a separate launch; (b) dU_full / dV nullable = zero.                                              */
int kgw_relvec_bwd_acc(int32_t n_live, const int32_t* rel_ids, const int32_t* bip_pos, const float* w_src_t,
                       const float* w_dst_t, const float* att_src, const float* att_dst, const float* dU_full,
                       const float* dV, const float* dw_src_acc, float* dw_src_t, float* dw_dst_t, float* datt_src,
                       float* datt_dst, int32_t v_by_rel, kgw_stream_t stream);

/* FC_output of the feature MLPs folded into the layer-1 relation parameters (exact re-association; no counterpart call in
 * the reference, which runs SimpleMLP.FC_output, kgwas/model.py:15,21, on every sampled node).  H = h2 T + c with
 * T = FC_output.weight^T enters GATConv only through <H_j, u_r>, <H_i, v_r> and sum_j alpha_ij H_j (kgwas/conv.py:150-152,
 * 227-228), so layer 1 runs on h2 with
 *     U'_r = T_src U_r,  V'_r = T_dst V_r,  kappa_r = <c_src, U_r> + <c_dst, V_r>,  W'_i = T_src W_i^T,  gamma_i = c_src W_i^T
 * (src / dst: the MLP of the relation's source / destination node type).  n packed relations (slot i = relation id
 * rel_ids_host[i]) of n_rels; n_mlp <= 4 MLPs.  U, V / U', V' / kappa are indexed by relation id (rows of relations
 * outside the pack are written as zeros), W_i^T / W'_i / gamma_i by packed slot.  _fwd fills Up, Vp, kappa, Wp, gamma;
 * _bwd fills dU, dV (feed kgw_relvec_bwd), dws (the fold's share of d W_i^T), d_fc_weight[m], d_fc_bias[m] from dUp, dVp,
 * dkappa, dWp, dgamma -- every element written, fixed summation order.  *_host arrays are host int32 arrays.          */
typedef struct KgwFoldArgs {
    int32_t n, n_rels, n_mlp;
    int32_t duv_pieces;              /* kgw_fold_bwd, != 0: dUp / dVp point at [n_rels][8][128] pieces (KGW_F_DUV_PIECES)        */
    const int32_t* rel_ids_host; const int32_t* src_mlp_host; const int32_t* dst_mlp_host;
    const float* w_src_t;            /* [n][128][128]                                   */
    const float* fc_weight[4];       /* FC_output.weight [128 out][128 in] of MLP m     */
    const float* fc_bias[4];         /* FC_output.bias [128]                            */
    const float* U; const float* V;  /* [n_rels][128]                                   */
    float* Up; float* Vp; float* kappa; float* Wp; float* gamma;
    const float* dUp; const float* dVp; const float* dkappa; const float* dWp; const float* dgamma;
    float* dU; float* dV; float* dws;
    float* d_fc_weight[4]; float* d_fc_bias[4];
} KgwFoldArgs;
int kgw_fold_fwd(const KgwFoldArgs* args, kgw_stream_t stream);
int kgw_fold_bwd(const KgwFoldArgs* args, kgw_stream_t stream);

/* The END of a captured step's backward pass as ONE launch: the deferred weight-gradient products of the MLPs (n_tn jobs + their
 * 2 n_tn records: kgw_tn_gemm_multi_partial's arguments), kgw_fold_bwd (fold, nullable) and kgw_relvec_bwd_multi (n_relvec jobs) as
 * the blocks of one grid -- parameter-only work that nothing but the optimiser waits for and of which no launch fills the chip.
 * Job fold_job of relvec is the fold's layer: its dU_full / dV / dw_src_acc are NOT read -- the blocks of that layer compute the
 * fold's d U_r, d V_r and d W share themselves and hand them on through LDS -- and fold->dU / dV / dws are not written.  Every value
 * is computed with the expressions and in the order of the kernel it comes from (bit-identical to the three launches).
 * KGW_E_UNSUPPORTED (nothing launched): a product outside the 64 x 64-per-wavefront tiling, an empty job.                       */
int kgw_param_tail(int32_t n_tn, const KgwTnJob* tn_jobs, KgwGradSrc* src, const KgwFoldArgs* fold, int32_t n_relvec,
                   const KgwRelvecJob* relvec, int32_t fold_job, kgw_stream_t stream);

/* kgw_gemm3 with RIDERS: the launch carries the step's parameter-only forward work as extra blocks on the compute units the
 * product leaves idle (the benchmark's forward product: 240 one-CU blocks on 256 CUs for ~145 us) -- what kgw_relvec_fwd_multi
 * (n_relvec jobs: the relation vectors of every layer, summed biases, the aggregates' zero fills; kgwas/conv.py:138-151) and
 * kgw_fold_fwd (fold, nullable: FC_output into the relations of job fold_job, kgwas/model.py:15,21; its U / V must be that
 * job's U_full / V) compute, with the same arithmetic (bit-identical values), one wavefront per task, no launch of their own.
 * kgw_gemm3_rider_blocks(M, K): the idle compute units such a launch has (0: none worth using -- kgw_gemm3_riders then returns
 * KGW_E_UNSUPPORTED before launching anything and the caller runs the riders' own kernels).                                   */
int kgw_gemm3_rider_blocks(int64_t M, int64_t K);

int kgw_gemm3_riders(const float* A, int64_t lda, int64_t M, int64_t K, const void* packed, float* workspace, int64_t workspace_floats,
                     const float* bias, int32_t relu, float* out, int64_t ldo, int32_t transpose_out, const int32_t* row_map,
                     float* out_rows, int64_t ld_rows, int64_t out_rows_n, const int32_t* out_rows_real, int32_t n_relvec,
                     const KgwRelvecJob* relvec, const KgwFoldArgs* fold, int32_t fold_job, kgw_stream_t stream);

/* LD-score weighted MSE over the seed rows (kgwas/kgwas.py:139-145): loss = mean_i w[n_id[i]] * (pred[i] - y[n_id[i]])^2,
 * float32 residual / square, float64 weight and mean; _bwd: dpred[i] = grad_loss * d loss / d pred[i].
 * y [N] float32 labels and w [N] float64 weights are indexed by GLOBAL node id, n_id [n] = the seeds' global ids. */
int kgw_wmse_fwd(const float* pred, const int32_t* n_id, const float* y, const double* w, int32_t n,
                 double* loss, kgw_stream_t stream);
int kgw_wmse_bwd(const float* pred, const int32_t* n_id, const float* y, const double* w, int32_t n,
                 const double* grad_loss, float* dpred, kgw_stream_t stream);

/* The training step's tail as two launches: read-out pred[i] = [relu](<H[i], w_lin> + b_lin) of the n seed rows
 * (HeteroGNN.lin, kgwas/model.py:50,83-86; hidden 128 -> 1) fused with the weighted MSE above; _bwd writes dH [rows][128]
 * (zero beyond the seeds), d w_lin [128] and d b_lin [1].  `relu` bit 0: ReLU on pred; bit 1 (_bwd): H is itself a ReLU
 * output whose backward is folded in (dH *= H > 0).  One wavefront per seed; partial results go to `scratch`
 * (_fwd: n doubles; _bwd: ceil(rows/4) * 129 floats) and a second single-block launch folds them in index order
 * (deterministic).                                                                                              */
int kgw_readout_wmse_fwd(const float* H, const float* w_lin, const float* b_lin, const int32_t* n_id,
                         const float* y, const double* w, int32_t n, int32_t relu, float* pred, double* loss,
                         double* scratch, kgw_stream_t stream);
int kgw_readout_wmse_bwd(const float* H, const float* w_lin, const float* pred, const int32_t* n_id,
                         const float* y, const double* w, int32_t n, int64_t rows, int32_t relu,
                         const double* grad_loss, float* dH, float* dw_lin, float* db_lin, float* scratch,
                         kgw_stream_t stream);

/* The two calls above fused for a training step whose loss gradient is 1 (loss.backward() of kgwas/kgwas.py:147):
 * prediction, loss, dH (zero beyond the seeds), d w_lin, d b_lin in two launches instead of four.  relu: bit 0 = ReLU
 * read-out, bit 1 = H is the output of a ReLU whose backward is folded in (dH *= H > 0).  terms [n] doubles and
 * scratch [((rows+3)/4) * 129] floats are workspaces.                                                             */
int kgw_readout_wmse_train(const float* H, const float* w_lin, const float* b_lin, const int32_t* n_id, const float* y,
                           const double* w, int32_t n, int64_t rows, int32_t relu, float* pred, double* loss, float* dH,
                           float* dw_lin, float* db_lin, double* terms, float* scratch, kgw_stream_t stream);
/* kgw_readout_wmse_train's first launch only; *fold_out describes the second (KgwReadoutFold).                                 */
int kgw_readout_wmse_train_parts(const float* H, const float* w_lin, const float* b_lin, const int32_t* n_id, const float* y,
                                 const double* w, int32_t n, int64_t rows, int32_t relu, float* pred, double* loss, float* dH,
                                 float* dw_lin, float* db_lin, double* terms, float* scratch, KgwReadoutFold* fold_out,
                                 kgw_stream_t stream);
int kgw_readout_train_fold(const KgwReadoutFold* fold, kgw_stream_t stream);

/* The read-out node for T label columns on one shared trunk (HeteroGNN(out_channels = T), kgwas/model.py:25,50), 1 <= T <= 32
 * (anything else: KGW_E_RANGE, nothing launched).  H [rows][128], W [T][128], b [T], n_id [n] global ids of the seeds,
 * y [N][T] row-major float32 labels and w [N] float64 weights indexed by global id (ONE weight per node, shared by the columns):
 *     pred[i][t] = [relu](<H[i], W[t]> + b[t])                                                         pred [n][T] row-major
 *     loss       = 1 / (n T) * sum_i sum_t w[n_id[i]] * (pred[i][t] - y[n_id[i]][t])^2
 * with the dot product, the residual, its square, the weight and the sum all in float64 (pred is the float64 dot product rounded
 * once to float32), so the loss agrees with its float64 statement to ~1e-15 relative even where a prediction nearly meets its
 * label; T = 1 is kgw_readout_wmse_*'s definition (which takes the residual in float32).  `relu` bit 0: ReLU on pred; bit 1 (backward): H is a ReLU output whose backward is folded in (dH *= H > 0).
 * Backward: g[i][t] = grad_loss / (n T) * w * 2 (pred - y) (0 where the ReLU is off), dH[i] = sum_t g[i][t] W[t] (t ascending;
 * rows n..rows-1 are written as zeros), dW[t] = sum_i g[i][t] H[i], db[t] = sum_i g[i][t].
 * Order of the sums (no float atomics, so a rerun is bit-identical): one wavefront per seed, four seeds per block; seed i's loss
 * term is its sum over t ascending (float64); the block's partial of dW / db is (g0 h0 + g1 h1) + (g2 h2 + g3 h3) over its four
 * seeds; a second launch folds them: block t adds the partials of column t -- seven groups of blocks q = g, g + 7, ..., each in
 * four interleaved accumulators (q, q+7, q+14, q+21 | +28), combined ((0+1)+(2+3)) + ((4+5)+6) -- and block 0 adds the n loss
 * terms (256 strided accumulators, binary tree) and divides by n T.  The folds' order is the single-column calls' order; a seed's dot product is a float64 xor butterfly
 * (1, 2, 4, ..., 32) over the lanes' two products, so T = 1 agrees with them to float32 rounding, not to the bit.
 * Workspaces: terms / _fwd's scratch [n] doubles; scratch of the backward forms [ceil(n/4) * T * 129] floats.
 *   kgw_readout_mt_pred        predictions only (HeteroGNN.forward, evaluation): one launch
 *   kgw_readout_mt_pred_bwd    its backward from dpred [n][T]: dH, dW, db (relu: bit 1 only)
 *   kgw_readout_wmse_mt_fwd    predictions and loss;  _bwd: dH, dW, db for any grad_loss;  two launches each
 *   kgw_readout_wmse_mt_train  both for a loss gradient of exactly 1, in two launches (kgw_readout_wmse_train's form)
 * kgw_readout_wmse_mtw_fwd / _bwd / _train: the same three calls -- arguments, grids, folds, workspaces, status codes -- with a weight
 * MATRIX, const double* w [N_SNP][T], row = global SNP id: loss = 1 / (n T) sum_i sum_t w[n_id[i]][t] (pred[i][t] - y[n_id[i]][t])^2,
 * the divisor n T whatever is observed.  w[g][t] == 0.0 means "column t is not observed at SNP g": that pair's loss term and d pred
 * are exactly 0 whatever bits y[g][t] holds (NaN and +-Inf included); pred[i][t] is still written.  Where every column of a row holds
 * the row's shared weight, the outputs equal those of the kgw_readout_wmse_mt_* call bit for bit.                                */
int kgw_readout_mt_pred(const float* H, const float* W, const float* b, int32_t n, int32_t T, int32_t relu, float* pred,
                        kgw_stream_t stream);
int kgw_readout_mt_pred_bwd(const float* H, const float* W, const float* dpred, int32_t n, int64_t rows, int32_t T, int32_t relu,
                            float* dH, float* dW, float* db, float* scratch, kgw_stream_t stream);
int kgw_readout_wmse_mt_fwd(const float* H, const float* W, const float* b, const int32_t* n_id, const float* y, const double* w,
                            int32_t n, int32_t T, int32_t relu, float* pred, double* loss, double* scratch, kgw_stream_t stream);
int kgw_readout_wmse_mt_bwd(const float* H, const float* W, const float* pred, const int32_t* n_id, const float* y, const double* w,
                            int32_t n, int64_t rows, int32_t T, int32_t relu, const double* grad_loss, float* dH, float* dW,
                            float* db, float* scratch, kgw_stream_t stream);
int kgw_readout_wmse_mt_train(const float* H, const float* W, const float* b, const int32_t* n_id, const float* y, const double* w,
                              int32_t n, int64_t rows, int32_t T, int32_t relu, float* pred, double* loss, float* dH, float* dW,
                              float* db, double* terms, float* scratch, kgw_stream_t stream);
int kgw_readout_wmse_mtw_fwd(const float* H, const float* W, const float* b, const int32_t* n_id, const float* y,
                             const double* w /* [N_SNP][T], row = global SNP id */, int32_t n, int32_t T, int32_t relu, float* pred,
                             double* loss, double* scratch, kgw_stream_t stream);
int kgw_readout_wmse_mtw_bwd(const float* H, const float* W, const float* pred, const int32_t* n_id, const float* y,
                             const double* w /* [N_SNP][T] */, int32_t n, int64_t rows, int32_t T, int32_t relu,
                             const double* grad_loss, float* dH, float* dW, float* db, float* scratch, kgw_stream_t stream);
int kgw_readout_wmse_mtw_train(const float* H, const float* W, const float* b, const int32_t* n_id, const float* y,
                               const double* w /* [N_SNP][T] */, int32_t n, int64_t rows, int32_t T, int32_t relu, float* pred,
                               double* loss, float* dH, float* dW, float* db, double* terms, float* scratch, kgw_stream_t stream);

/* The read-out node with a choice of loss (an EXTENSION: the reference knows the weighted MSE only).  THE RULE, for seed i, column t,
 * global id g = n_id[i], residual r = pred[i][t] - y[g][t], weight w = w[g] or w[g][t], N = n T and one knee delta[t] per column:
 *     rho_delta(r)  = r^2                      if |r| <= delta
 *                   = delta (2 |r| - delta)    otherwise              ( = 2 * torch.nn.functional.huber_loss(delta = delta) )
 *     rho_delta'(r) = 2 clamp(r, -delta, delta)
 *     loss          = 1 / N * sum_i sum_t w * rho_delta[t](r)
 *     d loss / d pred[i][t] = grad_loss / N * w * rho_delta[t]'(r)         (0 where the read-out ReLU is off)
 * The loss is C1: both branches give delta^2 and +-2 delta at the knee.  delta[t] is finite and > 0, or +inf; delta = +inf IS the
 * weighted MSE above and gives its bits (|r| <= delta is evaluated as !(|r| > delta): a NaN residual stays on the quadratic branch
 * and propagates as it does today).  A pair whose weight w[g][t] is exactly 0 has its residual taken as 0 before the label is
 * touched, as in kgw_readout_wmse_mtw_*: an exact 0 in the loss and in every gradient whatever bits its label holds.  (As there,
 * this is the weight MATRIX's convention, T > 1 with w_cols; the shared-weight and single-column kernels multiply the residual by
 * the weight as they always did, so a zero weight wants a finite label.)
 * Arithmetic, that of the kernels the loss is compiled into (a compile-time loss kind of k_readout_1 / k_readout_mt: the MSE
 * instantiations are the expressions they were, the Huber ones replace d * d and 2 d):
 *   T = 1 (k_readout_1):  float32 residual; the quadratic branch is its float32 square; weight and sum float64; the clamp on the
 *                         float32 residual.
 *   T > 1 (k_readout_mt): float64 dot product, residual and term; the gradient from the residual rounded to float32, the clamp
 *                         applied to that float32 value (the term's branch is decided on the float64 residual).
 *   The linear branch's term delta (2 |r| - delta) is formed in float64 in both.
 * delta travels BY VALUE in the kernel argument (lane t holds delta[t], a readlane picks column t's): no device array, and every
 * value is checked before any launch.  The second launch (k_readout_fold), the per-seed terms, the [T][129] partials, their
 * order and the workspaces are those of the calls above: no float atomics, a rerun is bit-identical.
 *
 * ONE argument record for the three families above (single column, _mt_, _mtw_) instead of a twin per entry point:
 *   T == 1           k_readout_1, the kgw_readout_wmse_* calls (w_cols is irrelevant: [N][1] is [N]);
 *   T > 1, w_cols 0  k_readout_mt, w [N]: kgw_readout_wmse_mt_*;    w_cols != 0: w [N][T], kgw_readout_wmse_mtw_*.
 * With loss_kind = KGW_LOSS_MSE (delta is not read) the outputs are those calls' outputs bit for bit.
 *   kgw_readout_loss_fwd    pred, loss (needs H W b n_id y w pred loss terms; `rows` is not read; relu: bit 0)
 *   kgw_readout_loss_bwd    dH dW db for any *grad_loss from the forward's predictions pred_in (needs H W pred_in n_id y w grad_loss
 *                           dH dW db scratch)
 *   kgw_readout_loss_train  both for a loss gradient of exactly 1 (needs H W b n_id y w pred loss dH dW db terms scratch).
 *                           fold_out != NULL with T == 1: kgw_readout_wmse_train_parts' form -- the first launch only, *fold_out
 *                           describes the second (kgw_readout_train_fold, or a later launch's fold_in);  with T > 1:
 *                           KGW_E_UNSUPPORTED.
 * Workspaces: terms [n] doubles, scratch [ceil(n / 4) * T * 129] floats (only a block that holds seeds leaves a partial).  Two
 * launches each.
 * Refused before any launch: a needed pointer NULL: KGW_E_NULL;  n < 1, rows < n, T outside [1, 32], a loss_kind other than the two,
 * and with KGW_LOSS_HUBER any of delta[0 .. T-1] that is NaN, <= 0 or -inf: KGW_E_RANGE.
 * KGW_VERSION stays: the feature is detected by symbol.                                                                          */
#define KGW_LOSS_MSE   0
#define KGW_LOSS_HUBER 1
#define KGW_READOUT_LOSS_ARGS_BYTES 288        /* sizeof(KgwReadoutLossArgs): asserted where the library is built and by the bindings */
typedef struct KgwReadoutLossArgs {
    const float* H;            /* [rows][128] */
    const float* W;            /* [T][128] (w_lin) */
    const float* b;            /* [T] */
    const int32_t* n_id;       /* [n] global ids of the seeds */
    const float* y;            /* [N][T] labels by global id */
    const double* w;           /* [N], or [N][T] with w_cols */
    const float* pred_in;      /* _bwd: the forward's predictions [n][T] */
    const double* grad_loss;   /* _bwd */
    float* pred; double* loss; float* dH; float* dW; float* db;
    double* terms; float* scratch;
    KgwReadoutFold* fold_out;  /* _train, optional */
    int64_t rows;
    int32_t n, T, relu;
    int32_t w_cols;            /* 0: w [N];  != 0: w [N][T], a weight of exactly 0 = unobserved pair */
    int32_t loss_kind;         /* KGW_LOSS_* */
    int32_t reserved;
    float delta[32];           /* KGW_LOSS_HUBER: the first T are read */
} KgwReadoutLossArgs;
int kgw_readout_loss_fwd(const KgwReadoutLossArgs* args, kgw_stream_t stream);
int kgw_readout_loss_bwd(const KgwReadoutLossArgs* args, kgw_stream_t stream);
int kgw_readout_loss_train(const KgwReadoutLossArgs* args, kgw_stream_t stream);

/* Self-test of the cross-lane reductions used by the aggregate kernels (one wavefront):
 * out_half[l] = sum over l's 32-lane half, out_wave[l] = sum over the wavefront,
 * out_steps[4][64] = the four intra-row DPP butterfly stages.                                  */
int kgw_debug_reduce(const float* in, float* out_half, float* out_wave, float* out_steps,
                     kgw_stream_t stream);
/* Self-test of the transposed 8-way reduction primitives (kgw_common.h): in [64][8]; out [6][64] = half_reduce8,
 * max8, sum8, bcast8<3>, xor4, xor8 of (in[lane][*] resp. in[lane][0]).                                          */
int kgw_debug_reduce8(const float* in, float* out, kgw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGWAS_HIP_H */
