// lipvq_gmm.hip -- the policy's output head: what the reference runs on the last T positions of the
// backbone output (robomimic/models/obs_nets.py:2602-2605): the ObservationDecoder's three Linears mean | scale | logits
// (obs_nets.py:747-771, policy_nets.py:2507-2516), tanh / softplus + min_std, the Normal / Independent / Categorical /
// MixtureSameFamily log_prob (policy_nets.py:2545-2575, algo/icl.py:947), the NLL's sum (icl.py:966) and .sample() (policy_nets.py:2599).
//
// MI355X design.  The three Linears are ONE [rows, E] x [E, P] product, P = M (2 A + 1) columns mean | scale | logits, on the
// fp32 MFMA with linear_kernel's k-ordered chain started from the bias (lipvq_embed.hip; same bits as lipvq_linear_act_f32 on
// the concatenated parameters -- which are never concatenated: a column picks its row of one of the three weights).  A
// workgroup owns 32 rows and ALL P columns (up to 16 column tiles, wave w takes tiles w, w + 4, ...), because the mixture needs
// a whole row: the accumulators go to an LDS tile [32][P], and the epilogue -- tanh, softplus, the per-mode Gaussian
// log-densities, log_softmax and logsumexp (both max-subtracted), or the inverse-CDF draw -- reads that tile.  Nothing of size
// [rows, M, A] goes to HBM unless the caller asks for it (the pre-activations for the backward, mean / scale / logits for the
// distribution object).  Input row (b, t) is read at x + b bstride + t E: the last T positions of the [B, 3T, E] backbone output
// are addressed in place.  The NLL's sum is per-workgroup partial sums (32 rows, in row order) reduced by one workgroup in a
// fixed order: no float atomics, the same bits on every run.
// The backward (gmm_head_bwd_kernel) is one pass over the saved pre-activations, 32 rows per workgroup through the same LDS
// tile: responsibilities r_m = softmax_m(log pi_m + l_m), then the closed forms of include/lipvq.h; again no atomics.
// The _mp entry points pick the product stage: LIPVQ_MATMUL_BF16 / _BF16X3 run it on the bf16 matrix pipe with the bits of
// lipvq_linear_act_bf16 / _bf16x3 (lq_head_product_bf16); every epilogue is the same code on the same tile.
// ABI: include/lipvq.h.
#include <math.h>

#include "lipvq_common.h"
#include "lipvq_head_product.h"
#include "lipvq_rng.h"

#define GMM_ROWS HEAD_ROWS
#define GMM_MAXM 16
#define GMM_MAXA 64
#define GMM_MAXP 512
#define GMM_MAXE 1024
#define GMM_LOW_NOISE_STD 1e-4f                       // policy_nets.py:2557
#define GMM_HALF_LOG_2PI 0.91893853320467274178f
#define GMM_DEPTHB 2                                  // chunks of 32 features in flight in the bf16 product stage
#define GMM_SIDE (2 * GMM_ROWS * (GMM_MAXM + 1) + GMM_ROWS)      // floats after the tile: ell, logit copies, row results

struct GmmArgs {
    const float* x;
    const float* Wm; const float* Ws; const float* Wl;
    const float* bm; const float* bs; const float* bl;
    const float* actions;
    union { const float* u; const int64_t* snap; };                 // the sampling epilogue's noise: u / eps read, or (the DRAW
    union { const float* eps; const int64_t* streams; };            // instances) snap / streams and the noise drawn in the kernel
    float* log_prob; float* pre; float* mean; float* scale; float* logits; float* partial; float* sample;
    int64_t N, bstride;
    int T, E, M, A, P, PS, scale_mode;
    float min_std;
};

// torch.exp of the EXP mode's pre-activation: lq_expf clamps its result to 3.4e38 by design (lipvq_math.h); a pre-activation that
// IS +inf -- a diverged run -- gives +inf here, as torch does, so that it shows in the scale, the log-probability and the gradient
__device__ __forceinline__ float gmm_exp(float p) { return p == INFINITY ? INFINITY : lq_expf(p); }

__device__ __forceinline__ float gmm_sigma(float p, int mode, float min_std) {
    if (mode == LIPVQ_GMM_LOW_NOISE) return GMM_LOW_NOISE_STD;
    return (mode == LIPVQ_GMM_EXP ? gmm_exp(p) : lq_softplus(p)) + min_std;
}

// one component of a sample from the picked mode's pre-activations: the ONE expression behind both noise sources
__device__ __forceinline__ float gmm_sample_value(float pmean, float pscale, float eps, int mode, float min_std) {
    return tanhf(pmean) + gmm_sigma(pscale, mode, min_std) * eps;
}

// d sigma / d p at the pre-activation p
__device__ __forceinline__ float gmm_dsigma(float p, int mode) {
    if (mode == LIPVQ_GMM_LOW_NOISE) return 0.0f;
    if (mode == LIPVQ_GMM_EXP) return gmm_exp(p);
    return p > 20.0f ? 1.0f : lq_sigmoid(p);
}

// l_m = sum_a [ -(x_a - mu)^2 / (2 sigma^2) - log sigma - 1/2 log 2 pi ] of one mode; prow = the row's pre-activations (LDS)
__device__ __forceinline__ float gmm_mode_ll(const float* prow, const float* __restrict__ act, int m, int A, int MA, int mode,
                                             float min_std) {
    float s = 0.0f;
    for (int a = 0; a < A; ++a) {
        const float mu = tanhf(prow[m * A + a]);
        const float sg = gmm_sigma(prow[MA + m * A + a], mode, min_std);
        const float z = (act[a] - mu) / sg;
        s += (-0.5f * z) * z - logf(sg) - GMM_HALF_LOG_2PI;
    }
    return s;
}

// max and log-sum-exp normaliser of the M logits of a row: returns logZ = max + log sum exp(l - max)
__device__ __forceinline__ float gmm_logz(const float* lg, int M) {
    float mx = lg[0];
    for (int m = 1; m < M; ++m) mx = fmaxf(mx, lg[m]);
    float se = 0.0f;
    for (int m = 0; m < M; ++m) se += lq_expf(lg[m] - mx);
    return mx + logf(se);
}

// the P columns mean | scale | logits of the product (lipvq_head_product.h): a column picks its row of one of the three weights
struct GmmCols {
    const float* Wm; const float* Ws; const float* Wl;
    const float* bm; const float* bs; const float* bl;
    int MA, P, E;
    __device__ __forceinline__ float bias(int c) const {
        float b0 = 0.0f;
        if (c < MA) b0 = bm[c];
        else if (c < 2 * MA) b0 = bs[c - MA];
        else if (c < P) b0 = bl[c - 2 * MA];
        return b0;
    }
    __device__ __forceinline__ const float* wrow(int c) const {
        return c < MA ? Wm + (size_t)c * E : c < 2 * MA ? Ws + (size_t)(c - MA) * E : c < P ? Wl + (size_t)(c - 2 * MA) * E : nullptr;
    }
};

// ---------------------------------------------------------------------------------------------------
// forward / sampling.  NT = column tiles per wave (P <= 128 NT), KC = input features staged per step: the product stage of
// lipvq_head_product.h, then the epilogues on its LDS tile.
// dynamic LDS: max(staging [32 + 128 NT][KC + 1] (MP: the bf16 images), tile [32][PS]) floats, then GMM_SIDE floats.
// ---------------------------------------------------------------------------------------------------
template <int NT, int KC, bool DRAW, int MP>
__global__ __launch_bounds__(256) void gmm_head_kernel(const GmmArgs a, int side_off) {
    extern __shared__ __attribute__((aligned(16))) float gmm_lds[];
    float* pt = gmm_lds;                                            // [32][PS], after the product
    float* s_ell = gmm_lds + side_off;                              // [32][17]
    float* s_lp = s_ell + 2 * GMM_ROWS * (GMM_MAXM + 1);            // [32]
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * GMM_ROWS;
    const int M = a.M, A = a.A, MA = a.M * a.A, P = a.P, PS = a.PS;
    lq_head_product_mp<MP, NT, KC, 1, GMM_DEPTHB>(gmm_lds, a.x, a.bstride, a.N, a.T, a.E, P, PS, GmmCols{a.Wm, a.Ws, a.Wl, a.bm, a.bs, a.bl, MA, P, a.E});
    const int64_t live = (a.N - row0 < GMM_ROWS) ? (a.N - row0) : GMM_ROWS;      // rows of this tile that exist
    if (a.pre) {
        float* dst = a.pre + (size_t)row0 * P;
        for (int i = tid; i < (int)live * P; i += 256) dst[i] = pt[(i / P) * PS + (i % P)];
    }
    if (a.mean) {
        float* dst = a.mean + (size_t)row0 * MA;
        for (int i = tid; i < (int)live * MA; i += 256) dst[i] = tanhf(pt[(i / MA) * PS + (i % MA)]);
    }
    if (a.scale) {
        float* dst = a.scale + (size_t)row0 * MA;
        for (int i = tid; i < (int)live * MA; i += 256) dst[i] = gmm_sigma(pt[(i / MA) * PS + MA + (i % MA)], a.scale_mode, a.min_std);
    }
    if (a.logits) {
        float* dst = a.logits + (size_t)row0 * M;
        for (int i = tid; i < (int)live * M; i += 256) dst[i] = pt[(i / M) * PS + 2 * MA + (i % M)];
    }
    if (a.actions) {                                               // uniform
        for (int i = tid; i < GMM_ROWS * M; i += 256) {            // item = (row, mode)
            const int row = i & 31, m = i >> 5;
            if (row < live)
                s_ell[row * (GMM_MAXM + 1) + m] = gmm_mode_ll(pt + row * PS, a.actions + (size_t)(row0 + row) * A, m, A, MA, a.scale_mode, a.min_std);
        }
        __syncthreads();
        if (tid < GMM_ROWS) {
            float lp = 0.0f;
            if (tid < live) {
                const float* lg = pt + tid * PS + 2 * MA;
                const float* el = s_ell + tid * (GMM_MAXM + 1);
                const float logz = gmm_logz(lg, M);
                float mx = (lg[0] - logz) + el[0];
                for (int m = 1; m < M; ++m) mx = fmaxf(mx, (lg[m] - logz) + el[m]);
                float se = 0.0f;
                for (int m = 0; m < M; ++m) se += lq_expf(((lg[m] - logz) + el[m]) - mx);
                lp = mx + logf(se);
                if (a.log_prob) a.log_prob[row0 + tid] = lp;
            }
            s_lp[tid] = lp;
        }
        __syncthreads();
        if (a.partial && tid == 0) {
            float s = 0.0f;
            for (int r = 0; r < GMM_ROWS; ++r) s += s_lp[r];       // row order
            a.partial[blockIdx.x] = s;
        }
    }
    if (a.sample) {                                                // uniform
        const int row = tid & 31, part = tid >> 5;
        lq_dropout dr;
        uint32_t rw = 0;
        if constexpr (DRAW) {
            // the row's uniform is drawn once, by part 0, and handed to the row's other seven items through s_lp (free in this mode)
            dr = lq_sample_load(a.snap);
            if (row < live) {
                rw = lq_sample_row(a.streams, row0 + row, a.T);
                if (part == 0) s_lp[row] = lq_sample_u(dr, rw);
            }
            __syncthreads();
        }
        if (row < live) {
            const float* pr = pt + row * PS;
            const float* lg = pr + 2 * MA;
            float mx = lg[0];
            for (int m = 1; m < M; ++m) mx = fmaxf(mx, lg[m]);
            float se = 0.0f;
            for (int m = 0; m < M; ++m) se += lq_expf(lg[m] - mx);
            float uu;
            if constexpr (DRAW) uu = s_lp[row];
            else uu = a.u[row0 + row];
            float cdf = 0.0f;
            int pick = M - 1;                                      // the last mode if rounding leaves none
            for (int m = 0; m < M; ++m) {
                cdf += lq_expf(lg[m] - mx) / se;
                if (uu < cdf) { pick = m; break; }
            }
            float* dst = a.sample + (size_t)(row0 + row) * A;
            // a row whose mixture weights are not numbers (a NaN or +inf logit: se is a NaN) has no draw: every comparison above was
            // false and `pick` is the last mode -- the sample is a NaN, not that mode's finite draw
            if constexpr (DRAW) {
                // item (row, part) owns the draws part, part + 8, ...: each Philox call is made once and serves its four components
                for (int g = part; 4 * g < A; g += 8) {
                    const lq_philox4 r = lq_sample_eps_draw(dr, rw, (uint32_t)g);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int aa = 4 * g + k;
                        if (aa < A)
                            dst[aa] = se == se ? gmm_sample_value(pr[pick * A + aa], pr[MA + pick * A + aa], lq_normal_icdf(lq_sample_open(r.w[k])),
                                                                  a.scale_mode, a.min_std) : se;
                    }
                }
            } else {
                const float* ep = a.eps + (size_t)(row0 + row) * A;
                for (int aa = part; aa < A; aa += 8)
                    dst[aa] = se == se ? gmm_sample_value(pr[pick * A + aa], pr[MA + pick * A + aa], ep[aa], a.scale_mode, a.min_std) : se;
            }
        }
    }
}

// the noise the DRAW instances form, written out: u [rows] and eps [rows][A] (tests, users).  One thread per draw: item (row, g)
// with g < G = ceil(A / 4) is the normals 4 g .. 4 g + 3 of the row, g == G its uniform.
__global__ __launch_bounds__(256) void gmm_noise_kernel(const int64_t* __restrict__ snap, const int64_t* __restrict__ streams,
                                                        float* __restrict__ u, float* __restrict__ eps, int64_t rows, int T, int A) {
    const int G = (A + 3) / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * (G + 1)) return;
    const int64_t row = i / (G + 1);
    const int g = (int)(i - row * (G + 1));
    const lq_dropout dr = lq_sample_load(snap);
    const uint32_t rw = lq_sample_row(streams, row, T);
    if (g == G) { u[row] = lq_sample_u(dr, rw); return; }
    const lq_philox4 r = lq_sample_eps_draw(dr, rw, (uint32_t)g);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * g + k < A) eps[row * A + 4 * g + k] = lq_normal_icdf(lq_sample_open(r.w[k]));
}

// sum of the per-workgroup partial sums in a fixed order (thread t: partials t, t + 256, ...; then a fixed tree)
__global__ __launch_bounds__(256) void gmm_sum_kernel(const float* __restrict__ partial, int64_t n, float* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t i = tid; i < n; i += 256) s += (double)partial[i];
    red[tid] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) out[0] = (float)red[0];
}

// ---------------------------------------------------------------------------------------------------
// backward of log_prob with respect to the pre-activations: gpre [N][P] from pre [N][P], actions [N][A] and the rows' upstream
// gradient g[n] (+ gsum[0], the gradient of the sum output).  32 rows per workgroup; the tile is overwritten in place (an item
// (row, mode) reads and writes only its own columns; the logits are read from a copy).
// ---------------------------------------------------------------------------------------------------
struct GmmBwdArgs {
    const float* pre; const float* actions; const float* g; const float* gsum;
    float* gpre;
    int64_t N;
    int M, A, P, PS, scale_mode;
    float min_std;
};

__global__ __launch_bounds__(256) void gmm_head_bwd_kernel(const GmmBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gmm_lds[];
    float* pt = gmm_lds;                                            // [32][PS]
    float* s_ell = gmm_lds + GMM_ROWS * a.PS;                       // [32][17]
    float* s_lg = s_ell + GMM_ROWS * (GMM_MAXM + 1);                // [32][17]
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * GMM_ROWS;
    const int M = a.M, A = a.A, MA = a.M * a.A, P = a.P, PS = a.PS;
    const int live = (int)((a.N - row0 < GMM_ROWS) ? (a.N - row0) : GMM_ROWS);
    const float* src = a.pre + (size_t)row0 * P;
    for (int i = tid; i < live * P; i += 256) pt[(i / P) * PS + (i % P)] = src[i];
    __syncthreads();
    for (int i = tid; i < GMM_ROWS * M; i += 256) {
        const int row = i & 31, m = i >> 5;
        if (row < live) {
            s_ell[row * (GMM_MAXM + 1) + m] = gmm_mode_ll(pt + row * PS, a.actions + (size_t)(row0 + row) * A, m, A, MA, a.scale_mode, a.min_std);
            s_lg[row * (GMM_MAXM + 1) + m] = pt[row * PS + 2 * MA + m];
        }
    }
    __syncthreads();
    const float gs = a.gsum ? a.gsum[0] : 0.0f;
    for (int i = tid; i < GMM_ROWS * M; i += 256) {
        const int row = i & 31, m = i >> 5;
        if (row >= live) continue;
        const float* lg = s_lg + row * (GMM_MAXM + 1);
        const float* el = s_ell + row * (GMM_MAXM + 1);
        const float logz = gmm_logz(lg, M);
        float mx = (lg[0] - logz) + el[0];
        for (int j = 1; j < M; ++j) mx = fmaxf(mx, (lg[j] - logz) + el[j]);
        float se = 0.0f;
        for (int j = 0; j < M; ++j) se += lq_expf(((lg[j] - logz) + el[j]) - mx);
        const float resp = lq_expf(((lg[m] - logz) + el[m]) - mx) / se;          // r_m
        const float pi = lq_expf(lg[m] - logz);
        const float g = (a.g ? a.g[row0 + row] : 0.0f) + gs;
        const float gr = g * resp;
        float* pr = pt + row * PS;
        const float* act = a.actions + (size_t)(row0 + row) * A;
        for (int aa = 0; aa < A; ++aa) {
            const float pm = pr[m * A + aa], psc = pr[MA + m * A + aa];
            const float mu = tanhf(pm);
            const float sg = gmm_sigma(psc, a.scale_mode, a.min_std);
            const float z = (act[aa] - mu) / sg;
            pr[m * A + aa] = gr * (z / sg) * (1.0f - mu * mu);
            pr[MA + m * A + aa] = gr * ((z * z - 1.0f) / sg) * gmm_dsigma(psc, a.scale_mode);
        }
        pr[2 * MA + m] = g * (resp - pi);
    }
    __syncthreads();
    float* dst = a.gpre + (size_t)row0 * P;
    for (int i = tid; i < live * P; i += 256) dst[i] = pt[(i / P) * PS + (i % P)];
}

// backward of the mean / scale / logits outputs (the distribution object's path): gpre = gmean (1 - tanh^2) | gscale sigma' | glogits
__global__ __launch_bounds__(256) void gmm_params_bwd_kernel(const float* __restrict__ pre, const float* __restrict__ gmean,
                                                             const float* __restrict__ gscale, const float* __restrict__ glogits,
                                                             float* __restrict__ gpre, int64_t N, int M, int A, int scale_mode) {
    const int MA = M * A, P = 2 * MA + M;
    const size_t total = (size_t)N * P;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t n = e / P;
        const int c = (int)(e - n * P);
        const float p = pre[e];
        float v;
        if (c < MA) {
            const float mu = tanhf(p);
            v = gmean ? gmean[n * MA + c] * (1.0f - mu * mu) : 0.0f;
        } else if (c < 2 * MA) {
            v = gscale ? gscale[n * MA + (c - MA)] * gmm_dsigma(p, scale_mode) : 0.0f;
        } else {
            v = glogits ? glogits[n * M + (c - 2 * MA)] : 0.0f;
        }
        gpre[e] = v;
    }
}

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------
static int gmm_check(const char* what, int64_t N, int T, int E, int M, int A, int scale_mode, int64_t bstride) {
    if (N < 0 || T <= 0 || E <= 0 || bstride < 0)
        return fail(LIPVQ_EINVAL, "%s: bad sizes N=%lld T=%d E=%d bstride=%lld", what, (long long)N, T, E, (long long)bstride);
    if (M < 1 || M > GMM_MAXM) return fail(LIPVQ_EUNSUPPORTED, "%s: num_modes M=%d (1..%d)", what, M, GMM_MAXM);
    if (A < 1 || A > GMM_MAXA) return fail(LIPVQ_EUNSUPPORTED, "%s: ac_dim A=%d (1..%d)", what, A, GMM_MAXA);
    if (M * (2 * A + 1) > GMM_MAXP)
        return fail(LIPVQ_EUNSUPPORTED, "%s: P = M (2 A + 1) = %d output columns (<= %d)", what, M * (2 * A + 1), GMM_MAXP);
    if (E > GMM_MAXE || (E & 3) != 0) return fail(LIPVQ_EUNSUPPORTED, "%s: E=%d (a multiple of 4, <= %d)", what, E, GMM_MAXE);
    if (scale_mode < LIPVQ_GMM_SOFTPLUS || scale_mode > LIPVQ_GMM_LOW_NOISE) return fail(LIPVQ_EINVAL, "%s: bad scale mode %d", what, scale_mode);
    if ((bstride & 3) != 0) return fail(LIPVQ_EINVAL, "%s: the batch stride must be a multiple of 4 floats", what);
    if ((N + GMM_ROWS - 1) / GMM_ROWS > 0x7fffffffLL) return fail(LIPVQ_EUNSUPPORTED, "%s: N=%lld", what, (long long)N);
    return LIPVQ_OK;
}

template <int MP>
static int gmm_launch_mp(const char* what, GmmArgs& a, hipStream_t st, bool draw) {
    a.P = a.M * (2 * a.A + 1);
    a.PS = a.P | 1;                                                 // odd row stride: the items of a wave differ in the row
    const int tiles = (a.P + 31) / 32, nt = (tiles + 3) / 4;
    const int NT = nt <= 1 ? 1 : (nt <= 2 ? 2 : 4), KC = NT == 4 ? 16 : 32;
    const int stage = MP == LIPVQ_MATMUL_FP32 ? lq_head_stage_floats(NT, KC) : lq_head_stage_floats_bf16(NT, MP == LIPVQ_MATMUL_BF16X3);
    const int tile = GMM_ROWS * a.PS;
    const int side_off = stage > tile ? stage : tile;
    const size_t lds = (size_t)(side_off + GMM_SIDE) * sizeof(float);          // at the most 89.5 KB (NT = 4, bf16x3)
    typedef void (*fn_t)(const GmmArgs, int);
    const fn_t kfn = draw ? (NT == 1 ? (fn_t)gmm_head_kernel<1, 32, true, MP> : (NT == 2 ? (fn_t)gmm_head_kernel<2, 32, true, MP> : (fn_t)gmm_head_kernel<4, 16, true, MP>))
                          : (NT == 1 ? (fn_t)gmm_head_kernel<1, 32, false, MP> : (NT == 2 ? (fn_t)gmm_head_kernel<2, 32, false, MP> : (fn_t)gmm_head_kernel<4, 16, false, MP>));
    static LqLdsReserve reserved[6];                                // (one array per MP: a static of the template instance)
    if (lds > 64 * 1024)
        if (int rc = lipvq_reserve_lds(reserved[(NT == 1 ? 0 : (NT == 2 ? 1 : 2)) + (draw ? 3 : 0)], (const void*)kfn, lds, what)) return rc;
    const dim3 grid((unsigned)((a.N + GMM_ROWS - 1) / GMM_ROWS)), block(256);
    hipLaunchKernelGGL(kfn, grid, block, lds, st, a, side_off);
    return check_launch(what);
}

static int gmm_launch(const char* what, GmmArgs& a, hipStream_t st, int matmul, bool draw = false) {
    if (matmul == LIPVQ_MATMUL_FP32) return gmm_launch_mp<LIPVQ_MATMUL_FP32>(what, a, st, draw);
    if (matmul == LIPVQ_MATMUL_BF16) return gmm_launch_mp<LIPVQ_MATMUL_BF16>(what, a, st, draw);
    return gmm_launch_mp<LIPVQ_MATMUL_BF16X3>(what, a, st, draw);
}

static int gmm_forward(const char* what, const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws,
                       const float* bs, const float* Wl, const float* bl, const float* actions, float* log_prob, float* pre,
                       float* mean, float* scale, float* logits, float* lp_sum, void* workspace, int64_t N, int T, int E,
                       int M, int A, int scale_mode, float min_std, int matmul, void* stream) {
    if (int rc = gmm_check(what, N, T, E, M, A, scale_mode, bstride)) return rc;
    if (int rc = lq_head_matmul_check(what, matmul, E)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        if (lp_sum && hipMemsetAsync(lp_sum, 0, sizeof(float), st) != hipSuccess) return fail(LIPVQ_EHIP, "%s: memset failed", what);
        return LIPVQ_OK;
    }
    if (!x || !Wm || !bm || !Ws || !bs || !Wl || !bl) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if ((log_prob || lp_sum) && !actions) return fail(LIPVQ_EINVAL, "%s: log_prob needs actions", what);
    if (lp_sum && !workspace) return fail(LIPVQ_EINVAL, "%s: the sum needs the workspace", what);
    if ((((uintptr_t)x | (uintptr_t)Wm | (uintptr_t)Ws | (uintptr_t)Wl) & 15) != 0)
        return fail(LIPVQ_EINVAL, "%s: x and the weights must be 16-byte aligned", what);
    GmmArgs a{x, Wm, Ws, Wl, bm, bs, bl, (log_prob || lp_sum) ? actions : nullptr, {nullptr}, {nullptr}, log_prob, pre, mean, scale, logits,
              lp_sum ? (float*)workspace : nullptr, nullptr, N, bstride, T, E, M, A, 0, 0, scale_mode, min_std};
    if (int rc = gmm_launch("gmm_head_kernel", a, st, matmul)) return rc;
    if (!lp_sum) return LIPVQ_OK;
    hipLaunchKernelGGL(gmm_sum_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, (N + GMM_ROWS - 1) / GMM_ROWS, lp_sum);
    return check_launch("gmm_sum_kernel");
}

static int gmm_sample(const char* what, const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws,
                      const float* bs, const float* Wl, const float* bl, const float* u, const float* eps, float* action, int64_t N,
                      int T, int E, int M, int A, int scale_mode, float min_std, int matmul, void* stream) {
    if (int rc = gmm_check(what, N, T, E, M, A, scale_mode, bstride)) return rc;
    if (int rc = lq_head_matmul_check(what, matmul, E)) return rc;
    if (N == 0) return LIPVQ_OK;
    if (!x || !Wm || !bm || !Ws || !bs || !Wl || !bl || !u || !eps || !action) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if ((((uintptr_t)x | (uintptr_t)Wm | (uintptr_t)Ws | (uintptr_t)Wl) & 15) != 0)
        return fail(LIPVQ_EINVAL, "%s: x and the weights must be 16-byte aligned", what);
    GmmArgs a{x, Wm, Ws, Wl, bm, bs, bl, nullptr, {u}, {eps}, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, action,
              N, bstride, T, E, M, A, 0, 0, scale_mode, min_std};
    return gmm_launch("gmm_head_kernel (sample)", a, (hipStream_t)stream, matmul);
}

static int gmm_sample_draw(const char* what, const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws,
                           const float* bs, const float* Wl, const float* bl, const int64_t* snap, const int64_t* streams, float* action,
                           int64_t N, int T, int E, int M, int A, int scale_mode, float min_std, int matmul, void* stream) {
    if (int rc = gmm_check(what, N, T, E, M, A, scale_mode, bstride)) return rc;
    if (int rc = lq_head_matmul_check(what, matmul, E)) return rc;
    if (N == 0) return LIPVQ_OK;
    if (!x || !Wm || !bm || !Ws || !bs || !Wl || !bl || !snap || !action) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if ((((uintptr_t)x | (uintptr_t)Wm | (uintptr_t)Ws | (uintptr_t)Wl) & 15) != 0)
        return fail(LIPVQ_EINVAL, "%s: x and the weights must be 16-byte aligned", what);
    GmmArgs a{x, Wm, Ws, Wl, bm, bs, bl, nullptr, {nullptr}, {nullptr}, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, action,
              N, bstride, T, E, M, A, 0, 0, scale_mode, min_std};
    a.snap = snap;
    a.streams = streams;
    return gmm_launch("gmm_head_kernel (sample, drawn)", a, (hipStream_t)stream, matmul, true);
}

extern "C" {

size_t lipvq_gmm_workspace_bytes(int64_t N) {
    if (N <= 0) return 0;
    return (size_t)((N + GMM_ROWS - 1) / GMM_ROWS) * sizeof(float);
}

int lipvq_gmm_head_f32(const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws, const float* bs,
                       const float* Wl, const float* bl, const float* actions, float* log_prob, float* pre, float* mean,
                       float* scale, float* logits, float* lp_sum, void* workspace, int64_t N, int T, int E, int M, int A,
                       int scale_mode, float min_std, void* stream) {
    return gmm_forward("lipvq_gmm_head_f32", x, bstride, Wm, bm, Ws, bs, Wl, bl, actions, log_prob, pre, mean, scale, logits,
                       lp_sum, workspace, N, T, E, M, A, scale_mode, min_std, LIPVQ_MATMUL_FP32, stream);
}

int lipvq_gmm_head_mp_f32(const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws, const float* bs,
                          const float* Wl, const float* bl, const float* actions, float* log_prob, float* pre, float* mean,
                          float* scale, float* logits, float* lp_sum, void* workspace, int64_t N, int T, int E, int M, int A,
                          int scale_mode, float min_std, int matmul, void* stream) {
    return gmm_forward("lipvq_gmm_head_mp_f32", x, bstride, Wm, bm, Ws, bs, Wl, bl, actions, log_prob, pre, mean, scale,
                       logits, lp_sum, workspace, N, T, E, M, A, scale_mode, min_std, matmul, stream);
}

int lipvq_gmm_sample_f32(const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws, const float* bs,
                         const float* Wl, const float* bl, const float* u, const float* eps, float* action, int64_t N, int T,
                         int E, int M, int A, int scale_mode, float min_std, void* stream) {
    return gmm_sample("lipvq_gmm_sample_f32", x, bstride, Wm, bm, Ws, bs, Wl, bl, u, eps, action, N, T, E, M, A, scale_mode,
                      min_std, LIPVQ_MATMUL_FP32, stream);
}

int lipvq_gmm_sample_mp_f32(const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws, const float* bs,
                            const float* Wl, const float* bl, const float* u, const float* eps, float* action, int64_t N, int T,
                            int E, int M, int A, int scale_mode, float min_std, int matmul, void* stream) {
    return gmm_sample("lipvq_gmm_sample_mp_f32", x, bstride, Wm, bm, Ws, bs, Wl, bl, u, eps, action, N, T, E, M, A, scale_mode,
                      min_std, matmul, stream);
}

int lipvq_gmm_sample_draw_f32(const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws, const float* bs,
                              const float* Wl, const float* bl, const int64_t* snap, const int64_t* streams, float* action, int64_t N,
                              int T, int E, int M, int A, int scale_mode, float min_std, void* stream) {
    return gmm_sample_draw("lipvq_gmm_sample_draw_f32", x, bstride, Wm, bm, Ws, bs, Wl, bl, snap, streams, action, N, T, E, M,
                           A, scale_mode, min_std, LIPVQ_MATMUL_FP32, stream);
}

int lipvq_gmm_sample_draw_mp_f32(const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws, const float* bs,
                                 const float* Wl, const float* bl, const int64_t* snap, const int64_t* streams, float* action, int64_t N,
                                 int T, int E, int M, int A, int scale_mode, float min_std, int matmul, void* stream) {
    return gmm_sample_draw("lipvq_gmm_sample_draw_mp_f32", x, bstride, Wm, bm, Ws, bs, Wl, bl, snap, streams, action, N, T, E,
                           M, A, scale_mode, min_std, matmul, stream);
}

static int gmm_noise_args(const char* what, int64_t B, int T, int A) {
    if (B < 0 || T <= 0) return fail(LIPVQ_EINVAL, "%s: bad sizes B=%lld T=%d", what, (long long)B, T);
    if (A < 1 || A > GMM_MAXA) return fail(LIPVQ_EUNSUPPORTED, "%s: ac_dim A=%d (1..%d)", what, A, GMM_MAXA);
    if (B > 0x7fffffffLL * 8 / T) return fail(LIPVQ_EUNSUPPORTED, "%s: B=%lld T=%d is too large a field for one launch", what, (long long)B, T);
    return LIPVQ_OK;
}

int lipvq_gmm_noise_f32(const int64_t* snap, const int64_t* streams, float* u, float* eps, int64_t B, int T, int A, void* stream) {
    if (int rc = gmm_noise_args("lipvq_gmm_noise_f32", B, T, A)) return rc;
    if (B == 0) return LIPVQ_OK;
    if (!snap || !u || !eps) return fail(LIPVQ_EINVAL, "lipvq_gmm_noise_f32: null pointer");
    const int64_t rows = B * T, items = rows * ((A + 3) / 4 + 1);
    hipLaunchKernelGGL(gmm_noise_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, snap, streams, u, eps,
                       rows, T, A);
    return check_launch("gmm_noise_kernel");
}

// the same two fields from the header on the host: no GPU call
int lipvq_gmm_noise_host(uint64_t seed, uint64_t step, const int64_t* streams, int64_t B, int T, int A, float* u, float* eps) {
    if (int rc = gmm_noise_args("lipvq_gmm_noise_host", B, T, A)) return rc;
    if (B == 0) return LIPVQ_OK;
    if (!u || !eps) return fail(LIPVQ_EINVAL, "lipvq_gmm_noise_host: null pointer");
    const lq_dropout dr = lq_sample_make(seed, step);
    for (int64_t row = 0; row < B * T; ++row) {
        const uint32_t rw = lq_sample_row(streams, row, T);
        u[row] = lq_sample_u(dr, rw);
        for (int g = 0; 4 * g < A; ++g) {
            const lq_philox4 r = lq_sample_eps_draw(dr, rw, (uint32_t)g);
            for (int k = 0; k < 4 && 4 * g + k < A; ++k) eps[row * A + 4 * g + k] = lq_normal_icdf(lq_sample_open(r.w[k]));
        }
    }
    return LIPVQ_OK;
}

int lipvq_normal_icdf_host(const uint32_t* words, float* out, int64_t n) {
    if (n < 0) return fail(LIPVQ_EINVAL, "lipvq_normal_icdf_host: n=%lld", (long long)n);
    if (n == 0) return LIPVQ_OK;
    if (!words || !out) return fail(LIPVQ_EINVAL, "lipvq_normal_icdf_host: null pointer");
    for (int64_t i = 0; i < n; ++i) out[i] = lq_normal_icdf(lq_sample_open(words[i]));
    return LIPVQ_OK;
}

int lipvq_gmm_head_bwd_f32(const float* pre, const float* actions, const float* g, const float* gsum, float* gpre, int64_t N,
                           int M, int A, int scale_mode, float min_std, void* stream) {
    if (int rc = gmm_check("lipvq_gmm_head_bwd_f32", N, 1, 4, M, A, scale_mode, 0)) return rc;
    if (N == 0) return LIPVQ_OK;
    if (!pre || !actions || !gpre || (!g && !gsum)) return fail(LIPVQ_EINVAL, "lipvq_gmm_head_bwd_f32: null pointer");
    const int P = M * (2 * A + 1), PS = P | 1;
    GmmBwdArgs a{pre, actions, g, gsum, gpre, N, M, A, P, PS, scale_mode, min_std};
    const size_t lds = (size_t)(GMM_ROWS * PS + 2 * GMM_ROWS * (GMM_MAXM + 1)) * sizeof(float);
    static LqLdsReserve reserved;
    if (lds > 64 * 1024)
        if (int rc = lipvq_reserve_lds(reserved, (const void*)gmm_head_bwd_kernel, lds, "gmm_head_bwd_kernel")) return rc;
    hipLaunchKernelGGL(gmm_head_bwd_kernel, dim3((unsigned)((N + GMM_ROWS - 1) / GMM_ROWS)), dim3(256), lds, (hipStream_t)stream, a);
    return check_launch("gmm_head_bwd_kernel");
}

int lipvq_gmm_params_bwd_f32(const float* pre, const float* gmean, const float* gscale, const float* glogits, float* gpre,
                             int64_t N, int M, int A, int scale_mode, void* stream) {
    if (int rc = gmm_check("lipvq_gmm_params_bwd_f32", N, 1, 4, M, A, scale_mode, 0)) return rc;
    if (N == 0) return LIPVQ_OK;
    if (!pre || !gpre) return fail(LIPVQ_EINVAL, "lipvq_gmm_params_bwd_f32: null pointer");
    const size_t total = (size_t)N * M * (2 * A + 1);
    size_t grid = (total + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(gmm_params_bwd_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, pre, gmean, gscale, glogits,
                       gpre, N, M, A, scale_mode);
    return check_launch("gmm_params_bwd_kernel");
}

}  // extern "C"
