// lipvq_action_head.hip -- the deterministic policy's output head: what the reference's ICLTransformer (algo.gmm.enabled = False,
// config/icl_config.py:63) runs on the backbone output: the ObservationDecoder's one Linear `action` (robomimic/models/
// obs_nets.py:747-771 with output_shapes = action (ac_dim,), policy_nets.py:1683-1690), tanh (policy_nets.py:1728-1731) and the three
// losses of ICL._compute_losses (algo/icl.py:174-202): MSELoss, SmoothL1Loss, cosine_loss on the first three components
// (utils/loss_utils.py:11-23), and their weighted sum (icl_config.py:43-45).
//
// MI355X design.  lipvq_gmm.hip's simpler sibling: the same product stage (lipvq_head_product.h: 32 rows and all A <= 64 columns
// per workgroup, the k-ordered fp32-MFMA chain from the bias, the reduction over E never split -- the same bits as
// lipvq_linear_act_f32), the accumulators in an LDS tile [32][A | 1], and an epilogue on that tile: tanh in place, then one
// thread per row forms the row's three loss terms.  Per-workgroup partial sums (32 rows, in row order) go to a workspace and a
// one-workgroup launch adds them in a fixed order and writes the four losses: no float atomics, the same bits on every run.
// The backward (action_head_bwd_kernel) is elementwise over the saved pre-activations; the upstream gradient of the four losses
// is read on the device.
// The _mp entry point picks the product stage: LIPVQ_MATMUL_BF16 / _BF16X3 run it on the bf16 matrix pipe with the bits of
// lipvq_linear_act_bf16 / _bf16x3 (lq_head_product_bf16); the epilogue is the same code.
// ABI: include/lipvq.h.
#include <math.h>

#include "lipvq_common.h"
#include "lipvq_head_product.h"

#define AH_MAXA 64
#define AH_MAXE 1024
#define AH_COS_EPS 1e-8f                              // nn.CosineSimilarity's eps
#define AH_NT 1                                       // A <= 64: two column tiles at the most, waves 0 and 1
#define AH_KC 32
#define AH_DEPTH 4                                    // chunks in flight: few workgroups walk E alone, so the loads' latency decides
#define AH_DEPTHB 4                                   // the same for the bf16 stage's chunks of 32

struct ActionHeadArgs {
    const float* x; const float* W; const float* b; const float* target;
    float* actions; float* pre; float* partial;
    int64_t N, bstride;
    int T, E, A, PS;
};

struct ActionHeadCols {
    const float* W; const float* b;
    int A, E;
    __device__ __forceinline__ float bias(int c) const { return c < A ? b[c] : 0.0f; }
    __device__ __forceinline__ const float* wrow(int c) const { return c < A ? W + (size_t)c * E : nullptr; }
};

// SmoothL1Loss with beta = 1 and its derivative
__device__ __forceinline__ float ah_smoothl1(float d) {
    const float z = fabsf(d);
    return z < 1.0f ? (0.5f * d) * d : z - 0.5f;
}
__device__ __forceinline__ float ah_smoothl1_grad(float d) {
    return d <= -1.0f ? -1.0f : (d >= 1.0f ? 1.0f : d);             // (a NaN fails both tests and stays a NaN, as in torch)
}

// nn.CosineSimilarity over 3 components (fewer: padded with zeros, which add nothing), each norm clamped on its own:
// sim = sum_c (p_c / max(|p|, eps)) (t_c / max(|t|, eps)).  pn, tn receive the normalised vectors; returns sim;
// np_out = max(|p|, eps), clamped = |p| <= eps.
__device__ __forceinline__ float ah_cos_sim(const float (&p)[3], const float (&t)[3], float (&pn)[3], float (&tn)[3], float& np_out,
                                            bool& clamped) {
    float pp = 0.0f, tt = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) { pp += p[c] * p[c]; tt += t[c] * t[c]; }
    const float np = sqrtf(pp), nt = sqrtf(tt);
    clamped = np <= AH_COS_EPS;                                      // (false for a NaN norm: its sim, a NaN, reaches every d sim / d p_c)
    np_out = fmaxf(np, AH_COS_EPS);
    const float ntc = fmaxf(nt, AH_COS_EPS);
    float sim = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pn[c] = p[c] / np_out;
        tn[c] = t[c] / ntc;
        sim += pn[c] * tn[c];
    }
    return sim;
}

// dynamic LDS: max(staging [32 + 128][33] (MP: the bf16 images), tile [32][PS]) floats, then 3 x 32 row results
template <int MP>
__global__ __launch_bounds__(256) void action_head_kernel(const ActionHeadArgs a, int side_off) {
    extern __shared__ __attribute__((aligned(16))) float ah_lds[];
    float* pt = ah_lds;                                             // [32][PS], after the product
    float* s_row = ah_lds + side_off;                               // [3][32]
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * HEAD_ROWS;
    const int A = a.A, PS = a.PS;
    lq_head_product_mp<MP, AH_NT, AH_KC, AH_DEPTH, AH_DEPTHB>(ah_lds, a.x, a.bstride, a.N, a.T, a.E, A, PS, ActionHeadCols{a.W, a.b, A, a.E});
    const int live = (int)((a.N - row0 < HEAD_ROWS) ? (a.N - row0) : HEAD_ROWS);          // rows of this tile that exist
    if (a.pre) {
        float* dst = a.pre + (size_t)row0 * A;
        for (int i = tid; i < live * A; i += 256) dst[i] = pt[(i / A) * PS + (i % A)];
    }
    // y = tanh(pre), in place: an item reads and writes its own element
    for (int i = tid; i < live * A; i += 256) {
        float* p = pt + (i / A) * PS + (i % A);
        const float y = tanhf(*p);
        *p = y;
        if (a.actions) a.actions[(size_t)row0 * A + i] = y;
    }
    if (!a.partial) return;                                         // uniform
    __syncthreads();
    if (tid < HEAD_ROWS) {
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
        if (tid < live) {
            const float* y = pt + tid * PS;
            const float* t = a.target + (size_t)(row0 + tid) * A;
            for (int c = 0; c < A; ++c) {
                const float d = y[c] - t[c];
                s0 += d * d;
                s1 += ah_smoothl1(d);
            }
            const int C = A < 3 ? A : 3;
            float p3[3], t3[3], pn[3], tn[3], np;
            bool clamped;
#pragma unroll
            for (int c = 0; c < 3; ++c) { p3[c] = c < C ? y[c] : 0.0f; t3[c] = c < C ? t[c] : 0.0f; }
            s2 = 1.0f - ah_cos_sim(p3, t3, pn, tn, np, clamped);
        }
        s_row[tid] = s0;
        s_row[HEAD_ROWS + tid] = s1;
        s_row[2 * HEAD_ROWS + tid] = s2;
    }
    __syncthreads();
    if (tid < 3) {
        float s = 0.0f;
        for (int r = 0; r < HEAD_ROWS; ++r) s += s_row[tid * HEAD_ROWS + r];      // row order
        a.partial[(size_t)blockIdx.x * 3 + tid] = s;
    }
}

// The three sums of the per-workgroup partial sums [n][3] in a fixed order (thread t: partials t, t + 256, ...; then a fixed
// tree), then losses = (l2, l1, cos, action).  The partials of the cosine term hold sum (1 - sim): cos = that sum / N.
__global__ __launch_bounds__(256) void action_head_sum_kernel(const float* __restrict__ partial, int64_t n, float* __restrict__ losses,
                                                              int64_t N, int A, float w2, float w1, float wc) {
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = tid; i < n; i += 256)
        for (int k = 0; k < 3; ++k) s[k] += (double)partial[i * 3 + k];
    for (int k = 0; k < 3; ++k) red[k][tid] = s[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off)
            for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        const double na = (double)N * (double)A;
        const float l2 = (float)(red[0][0] / na), l1 = (float)(red[1][0] / na), lc = (float)(red[2][0] / (double)N);
        losses[0] = l2;
        losses[1] = l1;
        losses[2] = lc;
        losses[3] = (w2 * l2 + w1 * l1) + wc * lc;                  // sum([w2 l2, w1 l1, wc cos]) in fp32, left to right (icl.py:195-200)
    }
}

// ---------------------------------------------------------------------------------------------------
// backward: gpre [N][A] = (the gradient of the four losses with respect to y = tanh(pre), + gy) (1 - y^2), one item per element.
// The effective coefficients of the three terms are g[0] + g[3] w2, g[1] + g[3] w1, g[2] + g[3] wc, from the device tensor g[4].
//   d sim / d p_c = t^_c / n_p                         if |p| <= eps (the clamped norm is a constant)
//                 = (t^_c - sim p^_c) / n_p            otherwise        (p^ = p / n_p, t^ = t / n_t, n = max(|.|, eps))
// which is t_c / (n_p n_t) - [|p| > eps] sim p_c / |p|^2 without the cancellation of two large terms.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void action_head_bwd_kernel(const float* __restrict__ pre, const float* __restrict__ target,
                                                              const float* __restrict__ g, const float* __restrict__ gy,
                                                              float* __restrict__ gpre, int64_t N, int A, float w2, float w1, float wc) {
    const size_t total = (size_t)N * A;
    const int C = A < 3 ? A : 3;
    float k2 = 0.0f, k1 = 0.0f, kc = 0.0f;
    if (g) {
        const float g3 = g[3];
        k2 = g[0] + g3 * w2;
        k1 = g[1] + g3 * w1;
        kc = g[2] + g3 * wc;
    }
    const float na = (float)N * (float)A, nn = (float)N;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t n = e / A;
        const int c = (int)(e - n * A);
        const float y = tanhf(pre[e]);
        float v = gy ? gy[e] : 0.0f;
        if (g) {
            const float d = y - target[e];
            v += k2 * ((2.0f * d) / na) + k1 * (ah_smoothl1_grad(d) / na);
            if (c < C) {
                float p3[3], t3[3], pn[3], tn[3], np;
                bool clamped;
#pragma unroll
                for (int j = 0; j < 3; ++j) { p3[j] = j < C ? tanhf(pre[n * A + j]) : 0.0f; t3[j] = j < C ? target[n * A + j] : 0.0f; }
                const float sim = ah_cos_sim(p3, t3, pn, tn, np, clamped);
                float ds = 0.0f;
#pragma unroll
                for (int j = 0; j < 3; ++j)                         // a select, not an indexed register array
                    if (j == c) ds = (clamped ? tn[j] : tn[j] - sim * pn[j]) / np;
                v += kc * (-ds / nn);
            }
        }
        gpre[e] = v * (1.0f - y * y);
    }
}

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------
static int ah_check(const char* what, int64_t N, int T, int E, int A, int64_t bstride) {
    if (N < 0 || T <= 0 || E <= 0 || bstride < 0)
        return fail(LIPVQ_EINVAL, "%s: bad sizes N=%lld T=%d E=%d bstride=%lld", what, (long long)N, T, E, (long long)bstride);
    if (A < 1 || A > AH_MAXA) return fail(LIPVQ_EUNSUPPORTED, "%s: ac_dim A=%d (1..%d)", what, A, AH_MAXA);
    if (E > AH_MAXE || (E & 3) != 0) return fail(LIPVQ_EUNSUPPORTED, "%s: E=%d (a multiple of 4, <= %d)", what, E, AH_MAXE);
    if ((bstride & 3) != 0) return fail(LIPVQ_EINVAL, "%s: the batch stride must be a multiple of 4 floats", what);
    if ((N + HEAD_ROWS - 1) / HEAD_ROWS > 0x7fffffffLL / 3) return fail(LIPVQ_EUNSUPPORTED, "%s: N=%lld", what, (long long)N);
    return LIPVQ_OK;
}

static int ah_forward(const char* what, const float* x, int64_t bstride, const float* W, const float* b, const float* target,
                      float* actions, float* pre, float* losses, void* workspace, int64_t N, int T, int E, int A, float w2, float w1,
                      float wc, int matmul, void* stream) {
    if (int rc = ah_check(what, N, T, E, A, bstride)) return rc;
    if (int rc = lq_head_matmul_check(what, matmul, E)) return rc;
    if (N == 0) return LIPVQ_OK;
    if (!x || !W || !b) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if (losses && !target) return fail(LIPVQ_EINVAL, "%s: the losses need a target", what);
    if (losses && !workspace) return fail(LIPVQ_EINVAL, "%s: the losses need the workspace", what);
    if ((((uintptr_t)x | (uintptr_t)W) & 15) != 0) return fail(LIPVQ_EINVAL, "%s: x and the weight must be 16-byte aligned", what);
    hipStream_t st = (hipStream_t)stream;
    const int PS = A | 1;                                           // odd row stride: the items of a wave differ in the row
    ActionHeadArgs a{x, W, b, losses ? target : nullptr, actions, pre, losses ? (float*)workspace : nullptr, N, bstride, T, E, A, PS};
    const int stage = matmul == LIPVQ_MATMUL_FP32 ? lq_head_stage_floats(AH_NT, AH_KC) : lq_head_stage_floats_bf16(AH_NT, matmul == LIPVQ_MATMUL_BF16X3);
    const int tile = HEAD_ROWS * PS;
    const int side_off = stage > tile ? stage : tile;
    const size_t lds = (size_t)(side_off + 3 * HEAD_ROWS) * sizeof(float);          // 21.5 KB (bf16: 13, bf16x3: 25.5)
    const int64_t tiles = (N + HEAD_ROWS - 1) / HEAD_ROWS;
    if (matmul == LIPVQ_MATMUL_FP32) hipLaunchKernelGGL(action_head_kernel<LIPVQ_MATMUL_FP32>, dim3((unsigned)tiles), dim3(256), lds, st, a, side_off);
    else if (matmul == LIPVQ_MATMUL_BF16) hipLaunchKernelGGL(action_head_kernel<LIPVQ_MATMUL_BF16>, dim3((unsigned)tiles), dim3(256), lds, st, a, side_off);
    else hipLaunchKernelGGL(action_head_kernel<LIPVQ_MATMUL_BF16X3>, dim3((unsigned)tiles), dim3(256), lds, st, a, side_off);
    if (int rc = check_launch("action_head_kernel")) return rc;
    if (!losses) return LIPVQ_OK;
    hipLaunchKernelGGL(action_head_sum_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, tiles, losses, N, A, w2, w1, wc);
    return check_launch("action_head_sum_kernel");
}

extern "C" {

size_t lipvq_action_head_workspace_bytes(int64_t N) {
    if (N <= 0) return 0;
    return (size_t)((N + HEAD_ROWS - 1) / HEAD_ROWS) * 3 * sizeof(float);
}

int lipvq_action_head_f32(const float* x, int64_t bstride, const float* W, const float* b, const float* target, float* actions,
                          float* pre, float* losses, void* workspace, int64_t N, int T, int E, int A, float w2, float w1,
                          float wc, void* stream) {
    return ah_forward("lipvq_action_head_f32", x, bstride, W, b, target, actions, pre, losses, workspace, N, T, E, A, w2, w1, wc,
                      LIPVQ_MATMUL_FP32, stream);
}

int lipvq_action_head_mp_f32(const float* x, int64_t bstride, const float* W, const float* b, const float* target, float* actions,
                             float* pre, float* losses, void* workspace, int64_t N, int T, int E, int A, float w2, float w1,
                             float wc, int matmul, void* stream) {
    return ah_forward("lipvq_action_head_mp_f32", x, bstride, W, b, target, actions, pre, losses, workspace, N, T, E, A, w2, w1, wc,
                      matmul, stream);
}

int lipvq_action_head_bwd_f32(const float* pre, const float* target, const float* g, const float* gy, float* gpre, int64_t N,
                              int A, float w2, float w1, float wc, void* stream) {
    if (int rc = ah_check("lipvq_action_head_bwd_f32", N, 1, 4, A, 0)) return rc;
    if (N == 0) return LIPVQ_OK;
    if (!pre || !gpre || (!g && !gy)) return fail(LIPVQ_EINVAL, "lipvq_action_head_bwd_f32: null pointer");
    if (g && !target) return fail(LIPVQ_EINVAL, "lipvq_action_head_bwd_f32: the losses' gradient needs the target");
    const size_t total = (size_t)N * A;
    size_t grid = (total + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(action_head_bwd_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, pre, target, g, gy, gpre, N, A,
                       w2, w1, wc);
    return check_launch("action_head_bwd_kernel");
}

}  // extern "C"
