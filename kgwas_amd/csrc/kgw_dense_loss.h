// kgw_dense_loss.h -- part of kgw_dense.hip (ONE translation unit, split by kernel family in round 6; include order matters:
// later families use device functions of earlier ones): LD-weighted MSE (kgw_wmse) and the fused read-out + loss node (kgw_readout_wmse*).
#pragma once

// ======================================================================================================
// kgw_wmse: LD-score weighted MSE of the seed predictions, loss = mean(w[n_id] * (pred - y[n_id])^2) in float64
// (kgwas/kgwas.py:139-145: float32 residual and square, float64 weight, float64 mean), and its gradient.
// One block; fixed-order reduction.
// ======================================================================================================
namespace {

__global__ void __launch_bounds__(256) k_wmse_fwd(const float* __restrict__ pred, const int32_t* __restrict__ n_id,
                                                  const float* __restrict__ y, const double* __restrict__ w, int n,
                                                  double* __restrict__ loss) {
    __shared__ double sd[256];
    const double total = kgw_sum256_f64(sd, n, [&](int i) {
        const int g = n_id[i];
        const float d = pred[i] - y[g];
        return w[g] * (double)(d * d);
    });
    if (threadIdx.x == 0) loss[0] = total / (double)n;
}

__global__ void __launch_bounds__(256) k_wmse_bwd(const float* __restrict__ pred, const int32_t* __restrict__ n_id,
                                                  const float* __restrict__ y, const double* __restrict__ w, int n,
                                                  const double* __restrict__ gloss, float* __restrict__ dpred) {
    const double g0 = gloss[0] / (double)n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int g = n_id[i];
        const float d = pred[i] - y[g];
        dpred[i] = (float)(g0 * w[g]) * (2.0f * d);        // the float64 product meets the float32 square here
    }
}

}  // namespace

extern "C" int kgw_wmse_fwd(const float* pred, const int32_t* n_id, const float* y, const double* w, int32_t n,
                            double* loss, kgw_stream_t stream_) {
    if (!pred || !n_id || !y || !w || !loss) return KGW_E_NULL;
    if (n <= 0) return KGW_E_RANGE;
    k_wmse_fwd<<<1, 256, 0, (hipStream_t)stream_>>>(pred, n_id, y, w, n, loss);
    KGW_LAUNCH_CHECK();
    return KGW_OK;
}

extern "C" int kgw_wmse_bwd(const float* pred, const int32_t* n_id, const float* y, const double* w, int32_t n,
                            const double* grad_loss, float* dpred, kgw_stream_t stream_) {
    if (!pred || !n_id || !y || !w || !grad_loss || !dpred) return KGW_E_NULL;
    if (n <= 0) return KGW_E_RANGE;
    k_wmse_bwd<<<(n + 255) / 256, 256, 0, (hipStream_t)stream_>>>(pred, n_id, y, w, n, grad_loss, dpred);
    KGW_LAUNCH_CHECK();
    return KGW_OK;
}

// ======================================================================================================
// kgw_readout_wmse: read-out Linear(128 -> 1) (+ ReLU) of the seed rows (kgwas/model.py:86) fused with the
// LD-score weighted MSE (kgwas/kgwas.py:139-145).  One wavefront per seed, four per block (k_readout_1); per-seed loss terms and
// per-block weight-gradient partials go to scratch buffers and a second, single-block launch (k_readout_fold, shared with the
// multi-trait node below) folds them in a fixed order -- parallel across the chip, yet a fixed summation order.  (A "last block
// folds" hand-off inside one launch was tried: its device-scope fence cost more than the second launch.)  _bwd and _train also
// produce the gradients of the read-out weight / bias and dH (zero for the rows beyond the seeds).
// ======================================================================================================
namespace {

enum { KGW_MT_FWD = 0, KGW_MT_TRAIN = 1, KGW_MT_BWD = 2, KGW_MT_BWD_PRED = 3 };    // (the last: k_readout_mt only)
// The kernels' one mode argument also carries the loss kind: bit 3 set = the Huber instantiation of that mode.  The MSE
// instantiations therefore keep their names (k_readout_1<1>, k_readout_mt<1, true>: launch fixtures and profiles know them).
enum { KGW_MT_HUBER = 8, KGW_MT_MODE_MASK = 7 };
constexpr int kgw_mt_loss(int mode_l) { return (mode_l & KGW_MT_HUBER) ? KGW_LOSS_HUBER : KGW_LOSS_MSE; }
constexpr int kgw_mt_mode_l(int mode, int loss) { return mode | (loss == KGW_LOSS_HUBER ? KGW_MT_HUBER : 0); }

// The loss kind of the read-out kernels is a compile-time argument (LOSS = KGW_LOSS_MSE | KGW_LOSS_HUBER, include/kgwas_hip.h): the MSE
// instantiations compile from the expressions they had, the Huber ones put rho_delta / rho_delta' in the place of d * d / 2 d.  The knees
// delta[t] travel BY VALUE in the kernel argument (an empty record for MSE), so the C call has checked them before any launch.
template <int LOSS> struct KgwKnees { float v[32]; };
template <> struct KgwKnees<KGW_LOSS_MSE> {};

// |d| <= delta as !(|d| > delta): a NaN residual stays on the quadratic branch and propagates as it does under MSE, and delta = +inf
// never leaves that branch, whatever d holds -- the MSE bits.
__device__ __forceinline__ bool kgw_huber_quadratic(float d, float delta) { return !(fabsf(d) > delta); }
__device__ __forceinline__ bool kgw_huber_quadratic(double d, double delta) { return !(fabs(d) > delta); }
// rho_delta'(d) / 2 = clamp(d, -delta, delta)
__device__ __forceinline__ float kgw_huber_clamp(float d, float delta) { return kgw_huber_quadratic(d, delta) ? d : copysignf(delta, d); }
// the linear branch's term delta (2 |d| - delta), in float64
__device__ __forceinline__ double kgw_huber_linear(double d, double delta) { return delta * (2.0 * fabs(d) - delta); }

// _FWD: prediction and loss term of seed i.  _TRAIN (a unit loss gradient: loss.backward()): forward and backward in ONE launch --
// prediction, loss term, d prediction, the dH row and the block's weight-gradient partial.  _BWD: the same from the forward's
// predictions and the loss gradient gloss[0].
template <int MODE_L>
__global__ void __launch_bounds__(256) k_readout_1(const float* __restrict__ H, const float* __restrict__ wl, const float* __restrict__ bl,
                                                   const float* __restrict__ pred_in, const int32_t* __restrict__ n_id,
                                                   const float* __restrict__ y, const double* __restrict__ w, int n, int64_t rows,
                                                   int relu, const double* __restrict__ gloss, float* __restrict__ pred,
                                                   double* __restrict__ terms, float* __restrict__ dH, float* __restrict__ part,
                                                   const KgwKnees<kgw_mt_loss(MODE_L)> knees) {
    constexpr int MODE = MODE_L & KGW_MT_MODE_MASK, LOSS = kgw_mt_loss(MODE_L);
    __shared__ float sw[4][KGW_C + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    float2 dw = make_float2(0.f, 0.f);
    float dp = 0.f;
    if (i < n) {
        const float2 w2 = ((const float2*)wl)[lane];
        const float2 h2 = ((const float2*)(H + i * KGW_C))[lane];
        float p;
        if (MODE == KGW_MT_BWD) {
            p = pred_in[i];
        } else {
            p = kgw_wave_allsum(fmaf(h2.x, w2.x, h2.y * w2.y)) + bl[0];
            if (relu & 1) p = fmaxf(p, 0.f);
        }
        const int g = n_id[i];
        const float d = p - y[g];
        double rho = (double)(d * d);                      // MSE: the float32 square;  dc: rho' / 2
        float dc = d;
        if constexpr (LOSS == KGW_LOSS_HUBER) {
            const float delta = knees.v[0];
            if (!kgw_huber_quadratic(d, delta)) rho = kgw_huber_linear((double)d, (double)delta);
            dc = kgw_huber_clamp(d, delta);
        }
        if (MODE != KGW_MT_BWD && lane == 0) {
            pred[i] = p;
            terms[i] = w[g] * rho;
        }
        if (MODE == KGW_MT_FWD) return;
        dp = (float)((MODE == KGW_MT_BWD ? gloss[0] : 1.0) / (double)n * w[g]) * (2.0f * dc);
        if ((relu & 1) && !(p > 0.f)) dp = 0.f;
        // (bit 1 of `relu`: H itself is the output of a ReLU whose backward the caller folds in here: dH *= (H > 0))
        const bool mk = (relu & 2) != 0;
        ((float2*)(dH + i * KGW_C))[lane] = make_float2((!mk || h2.x > 0.f) ? dp * w2.x : 0.f,
                                                         (!mk || h2.y > 0.f) ? dp * w2.y : 0.f);
        dw = make_float2(dp * h2.x, dp * h2.y);
    } else if (MODE != KGW_MT_FWD && i < rows) {
        ((float2*)(dH + i * KGW_C))[lane] = make_float2(0.f, 0.f);
    }
    if (MODE == KGW_MT_FWD || (int64_t)blockIdx.x * 4 >= n) return;            // blocks without seeds hold no partial
    sw[wave][2 * lane] = dw.x; sw[wave][2 * lane + 1] = dw.y;
    if (lane == 0) sw[wave][KGW_C] = dp;
    __syncthreads();
    if (threadIdx.x <= KGW_C) {                    // block partial: 128 weight columns + the bias term
        const int c = threadIdx.x;
        part[(int64_t)blockIdx.x * (KGW_C + 1) + c] = (sw[0][c] + sw[1][c]) + (sw[2][c] + sw[3][c]);
    }
}

// The second launch of every read-out entry point, single-column (T = 1) and multi-trait.  Block t: d W[t] [128] and d b[t] from the
// per-block partials [nb][T][129] (thread = (c, g): 129 columns x 7 row groups, kgw_walk_finish, then kgw_tree7); block 0 also the loss
// from the per-seed terms (kgw_sum256_f64, divided by n T).  part == nullptr: the loss only;  terms == nullptr: the gradients only.
__global__ void __launch_bounds__(1024) k_readout_fold(const float* __restrict__ part, int nb, int T, const double* __restrict__ terms,
                                                       int n, float* __restrict__ dW, float* __restrict__ db,
                                                       double* __restrict__ loss) {
    __shared__ float sm[7][KGW_C + 1];
    __shared__ double sd[256];
    const int c = threadIdx.x % (KGW_C + 1), g = threadIdx.x / (KGW_C + 1), t = blockIdx.x;
    if (part != nullptr && g < 7) {
        KgwWalk4 a;
        sm[g][c] = kgw_walk_finish(a, part + (int64_t)t * (KGW_C + 1) + c, g, nb, (int64_t)T * (KGW_C + 1));
    }
    if (terms != nullptr && t == 0) {                                    // (uniform over the block)
        const double total = kgw_sum256_f64(sd, n, [&](int q) { return terms[q]; });
        if (threadIdx.x == 0) loss[0] = total / ((double)n * (double)T);
    } else {
        __syncthreads();
    }
    if (part != nullptr && g == 0) {
        const float s = kgw_tree7(sm, c);
        if (c < KGW_C) dW[(int64_t)t * KGW_C + c] = s; else db[t] = s;
    }
}

inline int kgw_readout_fold_launch(const float* part, int nb, int T, const double* terms, int n, float* dW, float* db, double* loss,
                                   hipStream_t st) {
    k_readout_fold<<<part != nullptr ? T : 1, 1024, 0, st>>>(part, nb, T, terms, n, dW, db, loss);
    KGW_LAUNCH_CHECK();
    return KGW_OK;
}

// the first launch of the single-column entries: _FWD covers the seeds, the others every row of dH
template <int MODE, int LOSS = KGW_LOSS_MSE>
int kgw_readout_1_launch(const float* H, const float* w_lin, const float* b_lin, const float* pred_in, const int32_t* n_id, const float* y,
                         const double* w, int32_t n, int64_t rows, int32_t relu, const double* gloss, float* pred, double* terms, float* dH,
                         float* part, hipStream_t st, const KgwKnees<LOSS> knees = KgwKnees<LOSS>{}) {
    if (n <= 0 || rows < n) return KGW_E_RANGE;
    k_readout_1<kgw_mt_mode_l(MODE, LOSS)><<<(unsigned)(((MODE == KGW_MT_FWD ? n : rows) + 3) / 4), 256, 0, st>>>(H, w_lin, b_lin, pred_in, n_id, y, w, n, rows,
                                                                                                  relu, gloss, pred, terms, dH, part, knees);
    KGW_LAUNCH_CHECK();
    return KGW_OK;
}

}  // namespace

extern "C" int kgw_readout_wmse_fwd(const float* H, const float* w_lin, const float* b_lin, const int32_t* n_id,
                                    const float* y, const double* w, int32_t n, int32_t relu, float* pred,
                                    double* loss, double* scratch, kgw_stream_t stream_) {
    if (!H || !w_lin || !b_lin || !n_id || !y || !w || !pred || !loss || !scratch) return KGW_E_NULL;
    hipStream_t st = (hipStream_t)stream_;
    // (this entry's `relu` is a truth value, the others' a bit set)
    const int rc = kgw_readout_1_launch<KGW_MT_FWD>(H, w_lin, b_lin, nullptr, n_id, y, w, n, n, relu != 0, nullptr, pred, scratch, nullptr,
                                                    nullptr, st);
    return rc != KGW_OK ? rc : kgw_readout_fold_launch(nullptr, 0, 1, scratch, n, nullptr, nullptr, loss, st);
}

extern "C" int kgw_readout_wmse_bwd(const float* H, const float* w_lin, const float* pred, const int32_t* n_id,
                                    const float* y, const double* w, int32_t n, int64_t rows, int32_t relu,
                                    const double* grad_loss, float* dH, float* dw_lin, float* db_lin, float* scratch,
                                    kgw_stream_t stream_) {
    if (!H || !w_lin || !pred || !n_id || !y || !w || !grad_loss || !dH || !dw_lin || !db_lin || !scratch)
        return KGW_E_NULL;
    hipStream_t st = (hipStream_t)stream_;
    const int rc = kgw_readout_1_launch<KGW_MT_BWD>(H, w_lin, nullptr, pred, n_id, y, w, n, rows, relu, grad_loss, nullptr, nullptr, dH,
                                                    scratch, st);
    return rc != KGW_OK ? rc : kgw_readout_fold_launch(scratch, (n + 3) / 4, 1, nullptr, n, dw_lin, db_lin, nullptr, st);
}

// (round 4, measured and dropped: the whole training node as ONE block of 16 wavefronts walking the 512 rows -- no partial buffer, no
//  fold launch -- ran the step 40 - 45 us SLOWER: 32 dependent row trips per wavefront instead of one)
extern "C" int kgw_readout_wmse_train_parts(const float* H, const float* w_lin, const float* b_lin, const int32_t* n_id,
                                            const float* y, const double* w, int32_t n, int64_t rows, int32_t relu, float* pred,
                                            double* loss, float* dH, float* dw_lin, float* db_lin, double* terms, float* scratch,
                                            KgwReadoutFold* fold_out, kgw_stream_t stream_) {
    if (!H || !w_lin || !b_lin || !n_id || !y || !w || !pred || !loss || !dH || !dw_lin || !db_lin || !terms || !scratch || !fold_out)
        return KGW_E_NULL;
    const int rc = kgw_readout_1_launch<KGW_MT_TRAIN>(H, w_lin, b_lin, nullptr, n_id, y, w, n, rows, relu, nullptr, pred, terms, dH, scratch,
                                                      (hipStream_t)stream_);
    if (rc == KGW_OK) *fold_out = KgwReadoutFold{scratch, terms, dw_lin, db_lin, loss, (n + 3) / 4, n};
    return rc;
}

extern "C" int kgw_readout_train_fold(const KgwReadoutFold* f, kgw_stream_t stream_) {
    if (!f || !f->scratch || !f->terms || !f->dw_lin || !f->db_lin || !f->loss) return KGW_E_NULL;
    if (f->n <= 0 || f->nb <= 0) return KGW_E_RANGE;
    return kgw_readout_fold_launch(f->scratch, f->nb, 1, f->terms, f->n, f->dw_lin, f->db_lin, f->loss, (hipStream_t)stream_);
}

extern "C" int kgw_readout_wmse_train(const float* H, const float* w_lin, const float* b_lin, const int32_t* n_id,
                                      const float* y, const double* w, int32_t n, int64_t rows, int32_t relu, float* pred,
                                      double* loss, float* dH, float* dw_lin, float* db_lin, double* terms, float* scratch,
                                      kgw_stream_t stream_) {
    KgwReadoutFold f;
    const int rc = kgw_readout_wmse_train_parts(H, w_lin, b_lin, n_id, y, w, n, rows, relu, pred, loss, dH, dw_lin, db_lin, terms, scratch,
                                                &f, stream_);
    return rc != KGW_OK ? rc : kgw_readout_train_fold(&f, stream_);
}

// ======================================================================================================
// kgw_readout_mt_* / kgw_readout_wmse_mt_*: the read-out node for T label columns on ONE shared trunk (HeteroGNN(out_channels = T),
// kgwas/model.py:25,50): pred[i][t] = [relu](<H[i], W[t]> + b[t]) and
//     loss = 1 / (n T) * sum_i sum_t w[n_id[i]] * (pred[i][t] - y[n_id[i]][t])^2      (float64 throughout: see below).
// One wavefront per seed, four per block, as in the single-column node above: a lane holds its two columns of H[i] ONCE and walks the
// T rows of W in LDS (<= 16 KB; a lane's float2 of a row: 32 lanes x 8 B = one conflict-free 256-B bank row per half), reusing the
// row for the T dot products and for dH[i] = sum_t g[i][t] W[t] (t ascending).  Lane t of the wavefront carries column t's label,
// bias, prediction and d prediction, so the per-seed global traffic is one coalesced access each.  The block's weight-gradient
// partial [T][129] (128 columns + the bias term) is (g0 h0 + g1 h1) + (g2 h2 + g3 h3) of its four seeds; a second launch of T blocks
// (k_readout_fold above) folds the partials of column t (seven row groups, four interleaved accumulators, one tree) and block 0 adds up
// the per-seed loss terms (256 float64 accumulators, one tree).  No float atomics: reruns are bit-identical.
// The forward's dot product, the residual and its square are float64 (the float32 products are exact in it; xor butterfly 1, 2, ...,
// 32, so every lane holds the same bits), and pred is that sum rounded once to float32.  Where a prediction nearly meets its label the
// residual is the small difference of two large numbers, and a float32 dot product's rounding (~1e-7 |pred|) would show in the loss at
// 1e-7 |pred| / |residual|; in float64 the loss agrees with its float64 statement to rounding of the sum.  The gradients take the
// residual rounded to float32.  T = 1 therefore agrees with the single-column node to float32 rounding, not to the bit.
// kgw_readout_wmse_mtw_*: the same node with a weight MATRIX w [N_SNP][T] (a trait's LD-score regression weight depends on its own
// sample size, and a trait covers its own subset of the SNPs):
//     loss = 1 / (n T) * sum_i sum_t w[n_id[i]][t] * (pred[i][t] - y[n_id[i]][t])^2      (the divisor is n T whatever is observed).
// Lane t loads w[g][t] once per seed (coalesced, like the label); iteration t of the column loop reads it with two 32-bit readlanes
// and then uses the shared-weight kernel's expressions in their order, so equal columns give equal bits.  w[g][t] == 0.0 means "trait
// t is not observed at SNP g": the residual of that pair is taken as 0 before the label is touched, so its loss term and its d pred
// are exactly 0 whatever bits y[g][t] holds (NaN, +-Inf); pred[i][t] is still written.  A compile-time variant (W_COLS) of
// k_readout_mt: the shared-weight instantiations compile from the expressions they had.
// ======================================================================================================
namespace {

constexpr int KGW_MT_MAX = 32;                      // T <= 32: one lane of a 32-lane half per column, W <= 16 KB of LDS
struct KgwMtArgs {
    const float* H; const float* W; const float* b; const int32_t* n_id; const float* y; const double* w;
    const float* pred_in;               // _BWD: the forward's predictions;  _BWD_PRED: d loss / d pred [n][T]
    const double* gloss;                // _BWD: the loss gradient
    float* pred; double* terms; float* dH; float* part;
    int64_t rows;
    int n, T, relu;
};

__device__ __forceinline__ float kgw_lane_value(float v, int lane_uniform) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane_uniform));
}

__device__ __forceinline__ double kgw_lane_value_f64(double v, int lane_uniform) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane_uniform);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane_uniform);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ double kgw_wave_allsum_f64(double v) {
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// W_COLS: a.w is [N_SNP][T] (one weight per SNP and column, 0.0 = unobserved) instead of [N_SNP]
template <int MODE_L, bool W_COLS = false>
__global__ void __launch_bounds__(256) k_readout_mt(const KgwMtArgs a, const KgwKnees<kgw_mt_loss(MODE_L)> knees = KgwKnees<kgw_mt_loss(MODE_L)>{}) {
    constexpr int MODE = MODE_L & KGW_MT_MODE_MASK, LOSS = kgw_mt_loss(MODE_L);
    __shared__ float sW[KGW_MT_MAX * KGW_C];
    __shared__ float sH[4][KGW_C + 1];
    __shared__ float sG[4][KGW_MT_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    const int T = a.T, n = a.n;
    if ((int64_t)blockIdx.x * 4 >= n) {                   // a block without seeds: its rows of dH are zero, it holds no partial
        if (MODE != KGW_MT_FWD && i < a.rows) ((float2*)(a.dH + i * KGW_C))[lane] = make_float2(0.f, 0.f);
        return;
    }
    for (int q = threadIdx.x; q < T * (KGW_C / 2); q += 256) ((float2*)sW)[q] = ((const float2*)a.W)[q];
    __syncthreads();
    float2 h2 = make_float2(0.f, 0.f);
    float g_mine = 0.f;                                    // lane t: d loss / d (pre-activation of column t) of this seed
    if (i < n) {
        h2 = ((const float2*)(a.H + i * KGW_C))[lane];
        const bool labelled = MODE == KGW_MT_TRAIN || MODE == KGW_MT_BWD || (MODE == KGW_MT_FWD && a.y != nullptr);
        const bool mine = lane < T;
        double wg = 0.0, w_mine = 0.0, base = 0.0;         // (W_COLS: lane t holds w[g][t]; base = the part of `scale` before w)
        float y_mine = 0.f, b_mine = 0.f, in_mine = 0.f, p_mine = 0.f, scale = 0.f;
        if (labelled) {
            const int g = a.n_id[i];
            if (W_COLS) { if (mine) w_mine = a.w[(int64_t)g * T + lane]; }
            else wg = a.w[g];
            if (mine) y_mine = a.y[(int64_t)g * T + lane];
        }
        if ((MODE == KGW_MT_FWD || MODE == KGW_MT_TRAIN) && mine) b_mine = a.b[lane];
        float knee_mine = 0.f;                             // (Huber: lane t holds delta[t]; iteration t reads it with a readlane)
        if constexpr (LOSS == KGW_LOSS_HUBER) knee_mine = knees.v[lane & (KGW_MT_MAX - 1)];
        if ((MODE == KGW_MT_BWD || MODE == KGW_MT_BWD_PRED) && mine) in_mine = a.pred_in[i * T + lane];
        if (W_COLS) {
            if (MODE == KGW_MT_TRAIN) base = 1.0 / ((double)n * (double)T);
            if (MODE == KGW_MT_BWD) base = a.gloss[0] / ((double)n * (double)T);
        } else {
            if (MODE == KGW_MT_TRAIN) scale = (float)(1.0 / ((double)n * (double)T) * wg);
            if (MODE == KGW_MT_BWD) scale = (float)(a.gloss[0] / ((double)n * (double)T) * wg);
        }
        double term = 0.0;
        float2 dh = make_float2(0.f, 0.f);
        for (int t = 0; t < T; ++t) {
            const float2 w2 = ((const float2*)(sW + t * KGW_C))[lane];
            float p = 0.f, dp = 0.f;
            double p64 = 0.0;
            if (MODE == KGW_MT_FWD || MODE == KGW_MT_TRAIN) {
                p64 = kgw_wave_allsum_f64(fma((double)h2.x, (double)w2.x, (double)h2.y * (double)w2.y)) +
                      (double)kgw_lane_value(b_mine, t);
                if (a.relu & 1) p64 = fmax(p64, 0.0);
                p = (float)p64;
                if (lane == t) p_mine = p;
            } else {
                p = kgw_lane_value(in_mine, t);
                p64 = (double)p;
            }
            if (MODE == KGW_MT_BWD_PRED) {
                dp = p;                                    // (the caller's ReLU, if any, is its own autograd node)
            } else if (labelled) {
                double d64;
                if (W_COLS) {                              // (t is wavefront-uniform; an unobserved pair never reads its label)
                    wg = kgw_lane_value_f64(w_mine, t);
                    scale = (float)(base * wg);
                    d64 = wg != 0.0 ? p64 - (double)kgw_lane_value(y_mine, t) : 0.0;
                } else {
                    d64 = p64 - (double)kgw_lane_value(y_mine, t);
                }
                const float d = (float)d64;
                double rho = d64 * d64;                    // MSE: the float64 square;  dc: rho' / 2 of the float32 residual
                float dc = d;
                if constexpr (LOSS == KGW_LOSS_HUBER) {    // (the term from the float64 residual, the gradient from the clamped float32 one)
                    const float delta = kgw_lane_value(knee_mine, t);
                    if (!kgw_huber_quadratic(d64, (double)delta)) rho = kgw_huber_linear(d64, (double)delta);
                    dc = kgw_huber_clamp(d, delta);
                }
                if (MODE != KGW_MT_BWD) term += wg * rho;
                if (MODE != KGW_MT_FWD) {
                    dp = scale * (2.0f * dc);
                    if ((a.relu & 1) && !(p > 0.f)) dp = 0.f;
                }
            }
            if (MODE != KGW_MT_FWD) {
                dh.x = fmaf(dp, w2.x, dh.x); dh.y = fmaf(dp, w2.y, dh.y);
                if (lane == t) g_mine = dp;
            }
        }
        if ((MODE == KGW_MT_FWD || MODE == KGW_MT_TRAIN) && mine) a.pred[i * T + lane] = p_mine;
        if ((MODE == KGW_MT_FWD || MODE == KGW_MT_TRAIN) && labelled && lane == 0) a.terms[i] = term;
        if (MODE != KGW_MT_FWD) {
            // (bit 1 of `relu`: H itself is the output of a ReLU whose backward the caller folds in here: dH *= (H > 0))
            const bool mk = (a.relu & 2) != 0;
            ((float2*)(a.dH + i * KGW_C))[lane] = make_float2((!mk || h2.x > 0.f) ? dh.x : 0.f, (!mk || h2.y > 0.f) ? dh.y : 0.f);
        }
    } else if (MODE != KGW_MT_FWD && i < a.rows) {
        ((float2*)(a.dH + i * KGW_C))[lane] = make_float2(0.f, 0.f);
    }
    if (MODE == KGW_MT_FWD) return;
    sH[wave][2 * lane] = h2.x; sH[wave][2 * lane + 1] = h2.y;          // (a wavefront past the seeds: zeros times zeros)
    if (lane == 0) sH[wave][KGW_C] = 1.0f;                              // the bias column: g * 1
    if (lane < KGW_MT_MAX) sG[wave][lane] = g_mine;
    __syncthreads();
    float* part = a.part + (int64_t)blockIdx.x * T * (KGW_C + 1);
    for (int q = threadIdx.x; q < T * (KGW_C + 1); q += 256) {
        const int t = q / (KGW_C + 1), c = q - t * (KGW_C + 1);
        part[q] = (__fmul_rn(sG[0][t], sH[0][c]) + __fmul_rn(sG[1][t], sH[1][c])) +
                  (__fmul_rn(sG[2][t], sH[2][c]) + __fmul_rn(sG[3][t], sH[3][c]));
    }
}

inline int kgw_mt_range(int32_t n, int64_t rows, int32_t T) {
    return (n <= 0 || rows < n || T < 1 || T > KGW_MT_MAX || (rows + 3) / 4 > 0x7fffffff) ? KGW_E_RANGE : KGW_OK;
}

}  // namespace

extern "C" int kgw_readout_mt_pred(const float* H, const float* W, const float* b, int32_t n, int32_t T, int32_t relu, float* pred,
                                   kgw_stream_t stream_) {
    if (!H || !W || !b || !pred) return KGW_E_NULL;
    if (kgw_mt_range(n, n, T)) return KGW_E_RANGE;
    KgwMtArgs a{};
    a.H = H; a.W = W; a.b = b; a.pred = pred; a.rows = n; a.n = n; a.T = T; a.relu = relu;
    k_readout_mt<KGW_MT_FWD><<<(n + 3) / 4, 256, 0, (hipStream_t)stream_>>>(a);
    KGW_LAUNCH_CHECK();
    return KGW_OK;
}

extern "C" int kgw_readout_mt_pred_bwd(const float* H, const float* W, const float* dpred, int32_t n, int64_t rows, int32_t T,
                                       int32_t relu, float* dH, float* dW, float* db, float* scratch, kgw_stream_t stream_) {
    if (!H || !W || !dpred || !dH || !dW || !db || !scratch) return KGW_E_NULL;
    if (kgw_mt_range(n, rows, T)) return KGW_E_RANGE;
    hipStream_t st = (hipStream_t)stream_;
    KgwMtArgs a{};
    a.H = H; a.W = W; a.pred_in = dpred; a.dH = dH; a.part = scratch; a.rows = rows; a.n = n; a.T = T; a.relu = relu & 2;
    k_readout_mt<KGW_MT_BWD_PRED><<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(a);
    KGW_LAUNCH_CHECK();
    return kgw_readout_fold_launch(scratch, (n + 3) / 4, T, nullptr, n, dW, db, nullptr, st);
}

namespace {

// the three loss forms, W_COLS = false: w [N_SNP] (kgw_readout_wmse_mt_*);  true: w [N_SNP][T] (kgw_readout_wmse_mtw_*).  Same grids,
// same folds, same workspaces.
template <bool W_COLS>
int kgw_mt_wmse_fwd(const float* H, const float* W, const float* b, const int32_t* n_id, const float* y, const double* w, int32_t n,
                    int32_t T, int32_t relu, float* pred, double* loss, double* scratch, kgw_stream_t stream_) {
    if (!H || !W || !b || !n_id || !y || !w || !pred || !loss || !scratch) return KGW_E_NULL;
    if (kgw_mt_range(n, n, T)) return KGW_E_RANGE;
    hipStream_t st = (hipStream_t)stream_;
    KgwMtArgs a{};
    a.H = H; a.W = W; a.b = b; a.n_id = n_id; a.y = y; a.w = w; a.pred = pred; a.terms = scratch; a.rows = n; a.n = n; a.T = T;
    a.relu = relu;
    k_readout_mt<KGW_MT_FWD, W_COLS><<<(n + 3) / 4, 256, 0, st>>>(a);
    KGW_LAUNCH_CHECK();
    return kgw_readout_fold_launch(nullptr, 0, T, scratch, n, nullptr, nullptr, loss, st);
}

template <bool W_COLS>
int kgw_mt_wmse_bwd(const float* H, const float* W, const float* pred, const int32_t* n_id, const float* y, const double* w, int32_t n,
                    int64_t rows, int32_t T, int32_t relu, const double* grad_loss, float* dH, float* dW, float* db, float* scratch,
                    kgw_stream_t stream_) {
    if (!H || !W || !pred || !n_id || !y || !w || !grad_loss || !dH || !dW || !db || !scratch) return KGW_E_NULL;
    if (kgw_mt_range(n, rows, T)) return KGW_E_RANGE;
    hipStream_t st = (hipStream_t)stream_;
    KgwMtArgs a{};
    a.H = H; a.W = W; a.pred_in = pred; a.n_id = n_id; a.y = y; a.w = w; a.gloss = grad_loss; a.dH = dH; a.part = scratch;
    a.rows = rows; a.n = n; a.T = T; a.relu = relu;
    k_readout_mt<KGW_MT_BWD, W_COLS><<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(a);
    KGW_LAUNCH_CHECK();
    return kgw_readout_fold_launch(scratch, (n + 3) / 4, T, nullptr, n, dW, db, nullptr, st);
}

template <bool W_COLS>
int kgw_mt_wmse_train(const float* H, const float* W, const float* b, const int32_t* n_id, const float* y, const double* w, int32_t n,
                      int64_t rows, int32_t T, int32_t relu, float* pred, double* loss, float* dH, float* dW, float* db, double* terms,
                      float* scratch, kgw_stream_t stream_) {
    if (!H || !W || !b || !n_id || !y || !w || !pred || !loss || !dH || !dW || !db || !terms || !scratch) return KGW_E_NULL;
    if (kgw_mt_range(n, rows, T)) return KGW_E_RANGE;
    hipStream_t st = (hipStream_t)stream_;
    KgwMtArgs a{};
    a.H = H; a.W = W; a.b = b; a.n_id = n_id; a.y = y; a.w = w; a.pred = pred; a.terms = terms; a.dH = dH; a.part = scratch;
    a.rows = rows; a.n = n; a.T = T; a.relu = relu;
    k_readout_mt<KGW_MT_TRAIN, W_COLS><<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(a);
    KGW_LAUNCH_CHECK();
    return kgw_readout_fold_launch(scratch, (n + 3) / 4, T, terms, n, dW, db, loss, st);
}

}  // namespace

extern "C" int kgw_readout_wmse_mt_fwd(const float* H, const float* W, const float* b, const int32_t* n_id, const float* y,
                                       const double* w, int32_t n, int32_t T, int32_t relu, float* pred, double* loss,
                                       double* scratch, kgw_stream_t stream_) {
    return kgw_mt_wmse_fwd<false>(H, W, b, n_id, y, w, n, T, relu, pred, loss, scratch, stream_);
}

extern "C" int kgw_readout_wmse_mt_bwd(const float* H, const float* W, const float* pred, const int32_t* n_id, const float* y,
                                       const double* w, int32_t n, int64_t rows, int32_t T, int32_t relu, const double* grad_loss,
                                       float* dH, float* dW, float* db, float* scratch, kgw_stream_t stream_) {
    return kgw_mt_wmse_bwd<false>(H, W, pred, n_id, y, w, n, rows, T, relu, grad_loss, dH, dW, db, scratch, stream_);
}

extern "C" int kgw_readout_wmse_mt_train(const float* H, const float* W, const float* b, const int32_t* n_id, const float* y,
                                         const double* w, int32_t n, int64_t rows, int32_t T, int32_t relu, float* pred,
                                         double* loss, float* dH, float* dW, float* db, double* terms, float* scratch,
                                         kgw_stream_t stream_) {
    return kgw_mt_wmse_train<false>(H, W, b, n_id, y, w, n, rows, T, relu, pred, loss, dH, dW, db, terms, scratch, stream_);
}

extern "C" int kgw_readout_wmse_mtw_fwd(const float* H, const float* W, const float* b, const int32_t* n_id, const float* y,
                                        const double* w, int32_t n, int32_t T, int32_t relu, float* pred, double* loss,
                                        double* scratch, kgw_stream_t stream_) {
    return kgw_mt_wmse_fwd<true>(H, W, b, n_id, y, w, n, T, relu, pred, loss, scratch, stream_);
}

extern "C" int kgw_readout_wmse_mtw_bwd(const float* H, const float* W, const float* pred, const int32_t* n_id, const float* y,
                                        const double* w, int32_t n, int64_t rows, int32_t T, int32_t relu, const double* grad_loss,
                                        float* dH, float* dW, float* db, float* scratch, kgw_stream_t stream_) {
    return kgw_mt_wmse_bwd<true>(H, W, pred, n_id, y, w, n, rows, T, relu, grad_loss, dH, dW, db, scratch, stream_);
}

extern "C" int kgw_readout_wmse_mtw_train(const float* H, const float* W, const float* b, const int32_t* n_id, const float* y,
                                          const double* w, int32_t n, int64_t rows, int32_t T, int32_t relu, float* pred,
                                          double* loss, float* dH, float* dW, float* db, double* terms, float* scratch,
                                          kgw_stream_t stream_) {
    return kgw_mt_wmse_train<true>(H, W, b, n_id, y, w, n, rows, T, relu, pred, loss, dH, dW, db, terms, scratch, stream_);
}

// ======================================================================================================
// kgw_readout_loss_*: the three read-out families above behind ONE argument record with a loss kind (the rule: include/kgwas_hip.h,
// KgwReadoutLossArgs).  T == 1: k_readout_1; T > 1: k_readout_mt, the weight form chosen by w_cols.  KGW_LOSS_MSE launches the very
// instantiations of the calls above; KGW_LOSS_HUBER theirs with the knees in the kernel argument.  Same grids, folds and workspaces.
// ======================================================================================================
namespace {

enum { KGW_RL_FWD = 0, KGW_RL_BWD = 1, KGW_RL_TRAIN = 2 };

// every refusal of the three calls: nothing is launched unless this returns KGW_OK
inline int kgw_readout_loss_check(const KgwReadoutLossArgs* a, int form) {
    if (!a || !a->H || !a->W || !a->n_id || !a->y || !a->w) return KGW_E_NULL;
    if (form != KGW_RL_BWD && (!a->b || !a->pred || !a->loss || !a->terms)) return KGW_E_NULL;
    if (form == KGW_RL_BWD && (!a->pred_in || !a->grad_loss)) return KGW_E_NULL;
    if (form != KGW_RL_FWD && (!a->dH || !a->dW || !a->db || !a->scratch)) return KGW_E_NULL;
    if (kgw_mt_range(a->n, form == KGW_RL_FWD ? (int64_t)a->n : a->rows, a->T)) return KGW_E_RANGE;
    if (a->loss_kind != KGW_LOSS_MSE && a->loss_kind != KGW_LOSS_HUBER) return KGW_E_RANGE;
    if (a->loss_kind == KGW_LOSS_HUBER)
        for (int t = 0; t < a->T; ++t)
            if (!(a->delta[t] > 0.f)) return KGW_E_RANGE;                  // NaN, 0, negative, -inf (+inf passes: the MSE)
    if (form == KGW_RL_TRAIN && a->fold_out != nullptr && a->T > 1) return KGW_E_UNSUPPORTED;
    return KGW_OK;
}

template <int MODE, bool W_COLS, int LOSS>
int kgw_readout_loss_mt(const KgwReadoutLossArgs* r, const KgwKnees<LOSS> knees, hipStream_t st) {
    KgwMtArgs a{};
    a.H = r->H; a.W = r->W; a.n_id = r->n_id; a.y = r->y; a.w = r->w; a.n = r->n; a.T = r->T; a.relu = r->relu;
    a.rows = MODE == KGW_MT_FWD ? (int64_t)r->n : r->rows;
    if (MODE != KGW_MT_BWD) { a.b = r->b; a.pred = r->pred; a.terms = r->terms; }
    if (MODE == KGW_MT_BWD) { a.pred_in = r->pred_in; a.gloss = r->grad_loss; }
    if (MODE != KGW_MT_FWD) { a.dH = r->dH; a.part = r->scratch; }
    k_readout_mt<kgw_mt_mode_l(MODE, LOSS), W_COLS><<<(unsigned)((a.rows + 3) / 4), 256, 0, st>>>(a, knees);
    KGW_LAUNCH_CHECK();
    if (MODE == KGW_MT_FWD) return kgw_readout_fold_launch(nullptr, 0, r->T, r->terms, r->n, nullptr, nullptr, r->loss, st);
    return kgw_readout_fold_launch(r->scratch, (r->n + 3) / 4, r->T, MODE == KGW_MT_TRAIN ? r->terms : nullptr, r->n, r->dW, r->db,
                                   MODE == KGW_MT_TRAIN ? r->loss : nullptr, st);
}

template <int MODE, int LOSS>
int kgw_readout_loss_run(const KgwReadoutLossArgs* r, const KgwKnees<LOSS> knees, hipStream_t st) {
    if (r->T > 1) return r->w_cols ? kgw_readout_loss_mt<MODE, true, LOSS>(r, knees, st) : kgw_readout_loss_mt<MODE, false, LOSS>(r, knees, st);
    const int nb = (r->n + 3) / 4;
    if (MODE == KGW_MT_FWD) {
        const int rc = kgw_readout_1_launch<MODE, LOSS>(r->H, r->W, r->b, nullptr, r->n_id, r->y, r->w, r->n, r->n, r->relu & 1, nullptr,
                                                        r->pred, r->terms, nullptr, nullptr, st, knees);
        return rc != KGW_OK ? rc : kgw_readout_fold_launch(nullptr, 0, 1, r->terms, r->n, nullptr, nullptr, r->loss, st);
    }
    if (MODE == KGW_MT_BWD) {
        const int rc = kgw_readout_1_launch<MODE, LOSS>(r->H, r->W, nullptr, r->pred_in, r->n_id, r->y, r->w, r->n, r->rows, r->relu,
                                                        r->grad_loss, nullptr, nullptr, r->dH, r->scratch, st, knees);
        return rc != KGW_OK ? rc : kgw_readout_fold_launch(r->scratch, nb, 1, nullptr, r->n, r->dW, r->db, nullptr, st);
    }
    const int rc = kgw_readout_1_launch<MODE, LOSS>(r->H, r->W, r->b, nullptr, r->n_id, r->y, r->w, r->n, r->rows, r->relu, nullptr, r->pred,
                                                    r->terms, r->dH, r->scratch, st, knees);
    if (rc != KGW_OK) return rc;
    const KgwReadoutFold f{r->scratch, r->terms, r->dW, r->db, r->loss, nb, r->n};
    if (r->fold_out != nullptr) { *r->fold_out = f; return KGW_OK; }           // (kgw_readout_wmse_train_parts' form)
    return kgw_readout_train_fold(&f, (kgw_stream_t)st);
}

template <int MODE>
int kgw_readout_loss_entry(const KgwReadoutLossArgs* r, int form, kgw_stream_t stream_) {
    static_assert(sizeof(KgwReadoutLossArgs) == KGW_READOUT_LOSS_ARGS_BYTES, "KgwReadoutLossArgs: the size the bindings assert");
    const int rc = kgw_readout_loss_check(r, form);
    if (rc != KGW_OK) return rc;
    if (r->loss_kind == KGW_LOSS_MSE) return kgw_readout_loss_run<MODE, KGW_LOSS_MSE>(r, KgwKnees<KGW_LOSS_MSE>{}, (hipStream_t)stream_);
    KgwKnees<KGW_LOSS_HUBER> knees;
    for (int t = 0; t < KGW_MT_MAX; ++t) knees.v[t] = r->delta[t];
    return kgw_readout_loss_run<MODE, KGW_LOSS_HUBER>(r, knees, (hipStream_t)stream_);
}

}  // namespace

extern "C" int kgw_readout_loss_fwd(const KgwReadoutLossArgs* args, kgw_stream_t stream_) {
    return kgw_readout_loss_entry<KGW_MT_FWD>(args, KGW_RL_FWD, stream_);
}

extern "C" int kgw_readout_loss_bwd(const KgwReadoutLossArgs* args, kgw_stream_t stream_) {
    return kgw_readout_loss_entry<KGW_MT_BWD>(args, KGW_RL_BWD, stream_);
}

extern "C" int kgw_readout_loss_train(const KgwReadoutLossArgs* args, kgw_stream_t stream_) {
    return kgw_readout_loss_entry<KGW_MT_TRAIN>(args, KGW_RL_TRAIN, stream_);
}
