// lipvq_xf.hip -- the pieces of the DEFAULT action branch (reference robomimic/models/obs_nets.py:1244-1260, the `else` of the
// tokenizer switch: spectral-norm MLP + a 4-layer post-norm nn.TransformerEncoder attending over the flattened batch + Linear)
// that the tokenizer library did not have yet:
//   spectral_kernel        torch.nn.utils.spectral_norm's power iteration, sigma and W / sigma for one small weight matrix
//   spectral_bwd_kernel    backward of W -> W / sigma(W)  (u, v are constants, as in torch)
//   attention_kernel       softmax(Q K^T / sqrt(dh)) V per head on an UNBATCHED sequence [S][3D] (the reference hands the
//                          encoder a 2-D [B*T][D] tensor: every action of the batch attends to every other), fp32, online softmax
//   attention_bwd_q/kv     its backward (probabilities recomputed from the saved log-sum-exp)
// The Linears run on the existing lipvq_linear_act_f32 / lipvq_wgrad_f32, the post-norm residual y = LayerNorm(a + b) * w + bias
// and its backward on lipvq_gpt_layernorm_f32 / lipvq_gpt_layernorm_bwd_f32 (lipvq_gpt.hip) with s = NULL, gres = NULL.
// All sizes here are small (S = B*T rows of a training step, D <= 256): the kernels are written for launch latency and
// occupancy of a few workgroups, not for a roofline.
//   in-kernel dropout      the three attention kernels' <DH, true> instances draw the attention-probability decisions themselves
//                          (lipvq_rng.h) where the <DH, false> ones read keep bytes: same lanes, same order, same bits
// ABI: include/lipvq.h ("default action branch", "in-kernel dropout for the embedding stage and the default action branch").  Tolerance against torch: 1e-5 of each tensor's scale (tests/test_gpu_default.py).
#include "lipvq_common.h"
#include "lipvq_rng.h"

// ---------------------------------------------------------------------------------------------------
// spectral norm (torch/nn/utils/spectral_norm.py compute_weight): W [J][K] = weight_orig, u [J], v [K]
//   training:  v = normalize(W^T u), u = normalize(W v)   (one iteration, eps = 1e-12: x / max(|x|, eps)), written back
//   always:    sigma = u . (W v);  Wsn = W / sigma
// One workgroup; every reduction is a sequential fp32 chain in index order (deterministic; J, K <= 256).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spectral_kernel(const float* __restrict__ W, float* __restrict__ u, float* __restrict__ v,
                                                       float* __restrict__ Wsn, float* __restrict__ sigma_out, int J, int K,
                                                       int do_iter, float eps) {
    __shared__ float su[256], sv[256], sw[256];
    __shared__ float s_norm;
    const int tid = threadIdx.x;
    if (tid < J) su[tid] = u[tid];
    if (tid < K) sv[tid] = v[tid];
    __syncthreads();
    if (do_iter) {
        if (tid < K) {
            float a = 0.0f;
            for (int j = 0; j < J; ++j) a = lq_fma(W[(size_t)j * K + tid], su[j], a);
            sw[tid] = a;
        }
        __syncthreads();
        if (tid == 0) {
            float n2 = 0.0f;
            for (int k = 0; k < K; ++k) n2 = lq_fma(sw[k], sw[k], n2);
            const float n = lq_sqrt(n2);
            s_norm = n > eps ? n : eps;
        }
        __syncthreads();
        if (tid < K) { sv[tid] = sw[tid] / s_norm; v[tid] = sv[tid]; }
        __syncthreads();
    }
    if (tid < J) {                                   // (W v)[j]
        float a = 0.0f;
        for (int k = 0; k < K; ++k) a = lq_fma(W[(size_t)tid * K + k], sv[k], a);
        sw[tid] = a;
    }
    __syncthreads();
    if (do_iter) {
        if (tid == 0) {
            float n2 = 0.0f;
            for (int j = 0; j < J; ++j) n2 = lq_fma(sw[j], sw[j], n2);
            const float n = lq_sqrt(n2);
            s_norm = n > eps ? n : eps;
        }
        __syncthreads();
        if (tid < J) { su[tid] = sw[tid] / s_norm; u[tid] = su[tid]; }
        __syncthreads();
    }
    if (tid == 0) {
        float s = 0.0f;
        for (int j = 0; j < J; ++j) s = lq_fma(su[j], sw[j], s);
        s_norm = s;
        *sigma_out = s;
    }
    __syncthreads();
    const float sg = s_norm;
    for (int i = tid; i < J * K; i += 256) Wsn[i] = W[i] / sg;
}

extern "C" int lipvq_spectral_norm_f32(const float* W, float* u, float* v, float* Wsn, float* sigma, int J, int K,
                                       int do_power_iteration, float eps, void* stream) {
    if (!W || !u || !v || !Wsn || !sigma) return fail(LIPVQ_EINVAL, "spectral_norm: null pointer");
    if (J <= 0 || K <= 0 || J > 256 || K > 256) return fail(LIPVQ_EUNSUPPORTED, "spectral_norm: J=%d K=%d (1..256)", J, K);
    hipLaunchKernelGGL(spectral_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, W, u, v, Wsn, sigma, J, K,
                       do_power_iteration, eps);
    return check_launch("spectral_norm");
}

// Wsn = W / sigma with sigma = u^T W v, u and v constants:  gW = (gWsn - <gWsn, Wsn> u v^T) / sigma
__global__ __launch_bounds__(256) void spectral_bwd_kernel(const float* __restrict__ gWsn, const float* __restrict__ Wsn,
                                                           const float* __restrict__ u, const float* __restrict__ v,
                                                           const float* __restrict__ sigma, float* __restrict__ gW, int J, int K) {
    __shared__ double part[256];
    const int tid = threadIdx.x;
    double a = 0.0;
    for (int i = tid; i < J * K; i += 256) a += (double)gWsn[i] * (double)Wsn[i];
    part[tid] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    const float dot = (float)part[0];
    const float sg = *sigma;
    for (int i = tid; i < J * K; i += 256) {
        const int j = i / K, k = i - j * K;
        gW[i] = (gWsn[i] - dot * u[j] * v[k]) / sg;
    }
}

extern "C" int lipvq_spectral_norm_bwd_f32(const float* gWsn, const float* Wsn, const float* u, const float* v, const float* sigma,
                                           float* gW, int J, int K, void* stream) {
    if (!gWsn || !Wsn || !u || !v || !sigma || !gW) return fail(LIPVQ_EINVAL, "spectral_norm_bwd: null pointer");
    if (J <= 0 || K <= 0) return fail(LIPVQ_EINVAL, "spectral_norm_bwd: bad sizes");
    hipLaunchKernelGGL(spectral_bwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, gWsn, Wsn, u, v, sigma, gW, J, K);
    return check_launch("spectral_norm_bwd");
}

// ---------------------------------------------------------------------------------------------------
// attention over an unbatched sequence.  qkv [S][3D]: q = columns [0, D), k = [D, 2D), v = [2D, 3D); head h owns columns
// [h dh, (h+1) dh) of each.  Workgroup = 16 queries x 16 key lanes of one head: lane p of a query takes keys p, p+16, ... of a
// 64-key LDS tile, keeps an online softmax (m, l, acc[dh]); the 16 partials are merged by xor-shuffles at the end.
// keep [H][S][S] bytes (1 = keep) + inv_keep = 1 / (1 - p): the attention-probability dropout of nn.MultiheadAttention in
// training mode (NULL in eval); the normaliser uses every key, the value sum only the kept ones.
// A score is a float64 fma chain and stays float64 until its maximum is subtracted: an fp32 chain is off by ~1e-4 at |s| ~ 500
// (q, k sixteen times unit-normal), which moves the weights of two nearly tied keys by as much; exp, l and the value sum are fp32.
// ---------------------------------------------------------------------------------------------------
#define XF_DH 32
#define XF_QB 16
#define XF_KT 64
__device__ __forceinline__ float xf_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }

// the size and keep_prob checks shared by the forward and the backward entry point
static int attention_args(const char* what, const unsigned char* keep, float keep_prob, int64_t S, int D, int H) {
    if (S <= 0 || D <= 0 || H <= 0 || D % H != 0 || D / H > XF_DH)
        return fail(LIPVQ_EUNSUPPORTED, "%s: S=%lld D=%d H=%d (head width 1..%d)", what, (long long)S, D, H, XF_DH);
    if (S > 65535LL * XF_QB || (keep && !(keep_prob > 0.0f))) return fail(LIPVQ_EINVAL, "%s: bad S / keep_prob", what);
    return 0;
}

// the head width padded to 8, 16 or 32 columns (compile-time loops: the reference's 8 heads give 8 at D = 64, 26 at D = 208)
template <typename F>
static void xf_for_width(int dh, F&& f) { lq_dispatch<8, 16, 32>(dh <= 8 ? 8 : dh <= 16 ? 16 : 32, f); }

// PHILOX instances (forward, bwd_q): the decisions of one query `row` for the 64 keys of the tile at k0, bit n = key k0 + n.
// The tile's 16 draws (4 columns each) are shared by the query's 16 key lanes: lane p runs draw k0 / 4 + p and the lanes OR
// their nibbles together.  Every lane of the wave must call it (k0 is uniform); lane p then tests bits p, p + 16, p + 32, p + 48.
__device__ __forceinline__ uint64_t xf_keep_tile_q(lq_dropout d, uint32_t row, int k0, int p) {
    const uint32_t nib = lq_dropout_keep4(d, row, (uint32_t)(k0 >> 2) + (uint32_t)p) << (4 * (p & 7));
    uint32_t lo = p < 8 ? nib : 0u, hi = p < 8 ? 0u : nib;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        lo |= (uint32_t)__shfl_xor((int)lo, off, 64);
        hi |= (uint32_t)__shfl_xor((int)hi, off, 64);
    }
    return ((uint64_t)hi << 32) | lo;
}

template <int DH, bool PHILOX>
__global__ __launch_bounds__(256) void attention_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse,
                                                        const unsigned char* __restrict__ keep, float inv_keep, lq_dropout_src src,
                                                        int S, int D, int H) {
    __shared__ float sk[XF_KT][DH + 1], svv[XF_KT][DH + 1];
    const int dh = D / H, h = blockIdx.y;
    const int tid = threadIdx.x, qi = tid >> 4, p = tid & 15;
    const int q = blockIdx.x * XF_QB + qi;
    const int qc = q < S ? q : S - 1;
    const float scale = 1.0f / lq_sqrt((float)dh);
    double qr[DH];
    float acc[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) {
        qr[d] = d < dh ? (double)qkv[(size_t)qc * 3 * D + h * dh + d] * scale : 0.0;
        acc[d] = 0.0f;
    }
    double m = -INFINITY;
    float l = 0.0f;
    lq_dropout dr = {};
    if constexpr (PHILOX) dr = lq_dropout_load(src);
    for (int k0 = 0; k0 < S; k0 += XF_KT) {
        uint64_t kb = 0;
        if constexpr (PHILOX) kb = xf_keep_tile_q(dr, (uint32_t)((size_t)h * S + qc), k0, p);
        __syncthreads();
        for (int i = tid; i < XF_KT * DH; i += 256) {
            const int j = i / DH, d = i - j * DH;
            const int kj = k0 + j < S ? k0 + j : S - 1;
            sk[j][d] = d < dh ? qkv[(size_t)kj * 3 * D + D + h * dh + d] : 0.0f;            // (columns past the head width: zeros)
            svv[j][d] = d < dh ? qkv[(size_t)kj * 3 * D + 2 * D + h * dh + d] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < XF_KT / 16; ++jj) {
            const int j = p + 16 * jj;
            if (k0 + j < S) {
                double s = 0.0;
#pragma unroll
                for (int d = 0; d < DH; ++d)
                    s = fma(qr[d], (double)sk[j][d], s);
                const double mn = fmax(m, s);
                const float c = xf_exp((float)(m - mn)), e = xf_exp((float)(s - mn));
                l = lq_fma(l, c, e);
                float w;
                if constexpr (PHILOX) w = ((kb >> j) & 1u) ? e * inv_keep : 0.0f;
                else w = keep ? (keep[((size_t)h * S + qc) * S + k0 + j] ? e * inv_keep : 0.0f) : e;
#pragma unroll
                for (int d = 0; d < DH; ++d)
                    acc[d] = lq_fma(acc[d], c, w * svv[j][d]);
                m = mn;
            }
        }
    }
    // merge the 16 key lanes of the query (lanes qi*16 .. qi*16+15 of the workgroup: 16 consecutive lanes of one wave)
    double mall = m;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) mall = fmax(mall, __shfl_xor(mall, off, 64));
    const float c = (m == -INFINITY) ? 0.0f : xf_exp((float)(m - mall));
    l *= c;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) l += __shfl_xor(l, off, 64);
#pragma unroll
    for (int d = 0; d < DH; ++d) {
        float a = acc[d] * c;
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) a += __shfl_xor(a, off, 64);
        acc[d] = a;
    }
    if (q < S) {
        const float inv = 1.0f / l;
        for (int d = p; d < dh; d += 16) out[(size_t)q * D + h * dh + d] = acc[d] * inv;       // (acc[d] is the same in all 16 lanes)
        if (p == 0) lse[(size_t)h * S + q] = (float)(mall + (double)__logf(l));
    }
}

extern "C" int lipvq_attention_f32(const float* qkv, float* out, float* lse, const unsigned char* keep, float keep_prob,
                                   int64_t S, int D, int H, void* stream) {
    if (!qkv || !out || !lse) return fail(LIPVQ_EINVAL, "attention: null pointer");
    if (int rc = attention_args("attention", keep, keep_prob, S, D, H)) return rc;
    xf_for_width(D / H, [&](auto w) {
        hipLaunchKernelGGL((attention_kernel<w(), false>), dim3((unsigned)((S + XF_QB - 1) / XF_QB), H), dim3(256), 0, (hipStream_t)stream,
                           qkv, out, lse, keep, keep ? 1.0f / keep_prob : 1.0f, lq_dropout_src{}, (int)S, D, H);
    });
    return check_launch("attention");
}

extern "C" int lipvq_attention_drop_f32(const float* qkv, float* out, float* lse, const int64_t* snap, uint32_t site, double p,
                                        int64_t S, int D, int H, void* stream) {
    if (int rc = attention_args("attention_drop", nullptr, 1.0f, S, D, H)) return rc;
    if (int rc = lq_dropout_check("attention_drop", snap, p, (int64_t)H * S)) return rc;
    if (!qkv || !out || !lse) return fail(LIPVQ_EINVAL, "attention_drop: null pointer");
    const lq_dropout_src src = lq_dropout_src_make(snap, site, p);
    xf_for_width(D / H, [&](auto w) {
        hipLaunchKernelGGL((attention_kernel<w(), true>), dim3((unsigned)((S + XF_QB - 1) / XF_QB), H), dim3(256), 0, (hipStream_t)stream,
                           qkv, out, lse, nullptr, src.inv_keep, src, (int)S, D, H);
    });
    return check_launch("attention_drop");
}

// Backward.  delta[h][i] = sum_d dO[i][hd] O[i][hd];  P_ij = exp(s_ij - lse_i);  dP_ij = (keep_ij / keep_prob) dO_i . V_j;
// dS_ij = P_ij (dP_ij - delta_i);  dQ_i = scale sum_j dS_ij K_j;  dK_j = scale sum_i dS_ij Q_i;  dV_j = sum_i (keep_ij/keep_prob) P_ij dO_i.
// attention_bwd_q: workgroup = 16 queries x 16 key lanes (as the forward) -> dQ;  attention_bwd_kv: 16 keys x 16 query lanes -> dK, dV.
template <int DH, bool PHILOX>
__global__ __launch_bounds__(256) void attention_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                              const float* __restrict__ go, const float* __restrict__ lse,
                                                              float* __restrict__ gqkv, float* __restrict__ delta,
                                                              const unsigned char* __restrict__ keep, float inv_keep,
                                                              lq_dropout_src src, int S, int D, int H) {
    __shared__ float sk[XF_KT][DH + 1], svv[XF_KT][DH + 1];
    const int dh = D / H, h = blockIdx.y;
    const int tid = threadIdx.x, qi = tid >> 4, p = tid & 15;
    const int q = blockIdx.x * XF_QB + qi;
    const int qc = q < S ? q : S - 1;
    const float scale = 1.0f / lq_sqrt((float)dh);
    float qr[DH], gor[DH], acc[DH];
    float dl = 0.0f;
#pragma unroll
    for (int d = 0; d < DH; ++d) {
        qr[d] = d < dh ? qkv[(size_t)qc * 3 * D + h * dh + d] * scale : 0.0f;
        gor[d] = d < dh ? go[(size_t)qc * D + h * dh + d] : 0.0f;
        if (d < dh) dl = lq_fma(gor[d], o[(size_t)qc * D + h * dh + d], dl);
        acc[d] = 0.0f;
    }
    const float ls = lse[(size_t)h * S + qc];
    if (p == 0 && q < S) delta[(size_t)h * S + q] = dl;
    lq_dropout dr = {};
    if constexpr (PHILOX) dr = lq_dropout_load(src);
    for (int k0 = 0; k0 < S; k0 += XF_KT) {
        uint64_t kb = 0;
        if constexpr (PHILOX) kb = xf_keep_tile_q(dr, (uint32_t)((size_t)h * S + qc), k0, p);
        __syncthreads();
        for (int i = tid; i < XF_KT * DH; i += 256) {
            const int j = i / DH, d = i - j * DH;
            const int kj = k0 + j < S ? k0 + j : S - 1;
            sk[j][d] = d < dh ? qkv[(size_t)kj * 3 * D + D + h * dh + d] : 0.0f;
            svv[j][d] = d < dh ? qkv[(size_t)kj * 3 * D + 2 * D + h * dh + d] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < XF_KT / 16; ++jj) {
            const int j = p + 16 * jj;
            if (k0 + j < S) {
                double s = 0.0;
                float dp = 0.0f;
#pragma unroll
                for (int d = 0; d < DH; ++d)
                    { s = fma((double)qr[d], (double)sk[j][d], s); dp = lq_fma(gor[d], svv[j][d], dp); }
                const float pr = xf_exp((float)(s - (double)ls));
                if constexpr (PHILOX) dp = ((kb >> j) & 1u) ? dp * inv_keep : 0.0f;
                else if (keep) dp = keep[((size_t)h * S + qc) * S + k0 + j] ? dp * inv_keep : 0.0f;
                const float ds = pr * (dp - dl) * scale;
#pragma unroll
                for (int d = 0; d < DH; ++d)
                    acc[d] = lq_fma(ds, sk[j][d], acc[d]);
            }
        }
    }
#pragma unroll
    for (int d = 0; d < DH; ++d) {
        float a = acc[d];
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) a += __shfl_xor(a, off, 64);
        acc[d] = a;
    }
    if (q < S)
        for (int d = p; d < dh; d += 16) gqkv[(size_t)q * 3 * D + h * dh + d] = acc[d];
}

// PHILOX: the roles are swapped -- the workgroup's 16 keys are 4 draws wide and a tile has 64 queries: 256 draws, one per thread
// (query tid >> 2 of the tile, columns 4 (tid & 3) .. + 3 of the 16 keys), left in LDS as nibbles with the tile's other operands.
template <int DH, bool PHILOX>
__global__ __launch_bounds__(256) void attention_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ go,
                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                               float* __restrict__ gqkv, const unsigned char* __restrict__ keep,
                                                               float inv_keep, lq_dropout_src src, int S, int D, int H) {
    __shared__ float sq[XF_KT][DH + 1], sg[XF_KT][DH + 1];
    __shared__ float sl[XF_KT], sd[XF_KT];
    __shared__ unsigned char sb[PHILOX ? XF_KT : 1][4];
    const int dh = D / H, h = blockIdx.y;
    const int tid = threadIdx.x, ki = tid >> 4, p = tid & 15;
    const int k = blockIdx.x * XF_QB + ki;
    const int kc = k < S ? k : S - 1;
    const float scale = 1.0f / lq_sqrt((float)dh);
    float kr[DH], vr[DH], ak[DH], av[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) {
        kr[d] = d < dh ? qkv[(size_t)kc * 3 * D + D + h * dh + d] : 0.0f;
        vr[d] = d < dh ? qkv[(size_t)kc * 3 * D + 2 * D + h * dh + d] : 0.0f;
        ak[d] = 0.0f; av[d] = 0.0f;
    }
    lq_dropout dr = {};
    if constexpr (PHILOX) dr = lq_dropout_load(src);
    for (int q0 = 0; q0 < S; q0 += XF_KT) {
        __syncthreads();
        for (int i = tid; i < XF_KT * DH; i += 256) {
            const int j = i / DH, d = i - j * DH;
            const int qj = q0 + j < S ? q0 + j : S - 1;
            sq[j][d] = d < dh ? qkv[(size_t)qj * 3 * D + h * dh + d] * scale : 0.0f;
            sg[j][d] = d < dh ? go[(size_t)qj * D + h * dh + d] : 0.0f;
        }
        if (tid < XF_KT) {
            const int qj = q0 + tid < S ? q0 + tid : S - 1;
            sl[tid] = lse[(size_t)h * S + qj];
            sd[tid] = delta[(size_t)h * S + qj];
        }
        if constexpr (PHILOX) {
            const int j = tid >> 2, qj = q0 + j < S ? q0 + j : S - 1;
            sb[j][tid & 3] = (unsigned char)lq_dropout_keep4(dr, (uint32_t)((size_t)h * S + qj), (uint32_t)(4 * blockIdx.x + (tid & 3)));
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < XF_KT / 16; ++jj) {
            const int j = p + 16 * jj;
            if (q0 + j < S) {
                double s = 0.0;
                float dp = 0.0f;
#pragma unroll
                for (int d = 0; d < DH; ++d)
                    { s = fma((double)sq[j][d], (double)kr[d], s); dp = lq_fma(sg[j][d], vr[d], dp); }
                const float pr = xf_exp((float)(s - (double)sl[j]));
                float kp = 1.0f;
                if constexpr (PHILOX) kp = ((sb[j][ki >> 2] >> (ki & 3)) & 1u) ? inv_keep : 0.0f;
                else if (keep) kp = keep[((size_t)h * S + q0 + j) * S + kc] ? inv_keep : 0.0f;
                const float ds = pr * (dp * kp - sd[j]);          // (the forward's q was pre-scaled: dK_j = sum_i dS_ij (scale Q_i))
                const float pv = pr * kp;
#pragma unroll
                for (int d = 0; d < DH; ++d)
                    { ak[d] = lq_fma(ds, sq[j][d], ak[d]); av[d] = lq_fma(pv, sg[j][d], av[d]); }
            }
        }
    }
#pragma unroll
    for (int d = 0; d < DH; ++d) {
        float a = ak[d], b = av[d];
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) { a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64); }
        ak[d] = a; av[d] = b;
    }
    if (k < S)
        for (int d = p; d < dh; d += 16) {
            gqkv[(size_t)k * 3 * D + D + h * dh + d] = ak[d];
            gqkv[(size_t)k * 3 * D + 2 * D + h * dh + d] = av[d];
        }
}

extern "C" int lipvq_attention_bwd_f32(const float* qkv, const float* out, const float* gout, const float* lse, float* gqkv,
                                       float* delta, const unsigned char* keep, float keep_prob, int64_t S, int D, int H, void* stream) {
    if (!qkv || !out || !gout || !lse || !gqkv || !delta) return fail(LIPVQ_EINVAL, "attention_bwd: null pointer");
    if (int rc = attention_args("attention_bwd", keep, keep_prob, S, D, H)) return rc;
    const dim3 grid((unsigned)((S + XF_QB - 1) / XF_QB), H);
    const float ik = keep ? 1.0f / keep_prob : 1.0f;
    xf_for_width(D / H, [&](auto w) {
        hipLaunchKernelGGL((attention_bwd_q_kernel<w(), false>), grid, dim3(256), 0, (hipStream_t)stream, qkv, out, gout, lse, gqkv, delta,
                           keep, ik, lq_dropout_src{}, (int)S, D, H);
        hipLaunchKernelGGL((attention_bwd_kv_kernel<w(), false>), grid, dim3(256), 0, (hipStream_t)stream, qkv, gout, lse, delta, gqkv,
                           keep, ik, lq_dropout_src{}, (int)S, D, H);
    });
    return check_launch("attention_bwd");
}

extern "C" int lipvq_attention_bwd_drop_f32(const float* qkv, const float* out, const float* gout, const float* lse, float* gqkv,
                                            float* delta, const int64_t* snap, uint32_t site, double p, int64_t S, int D, int H,
                                            void* stream) {
    if (int rc = attention_args("attention_bwd_drop", nullptr, 1.0f, S, D, H)) return rc;
    if (int rc = lq_dropout_check("attention_bwd_drop", snap, p, (int64_t)H * S)) return rc;
    if (!qkv || !out || !gout || !lse || !gqkv || !delta) return fail(LIPVQ_EINVAL, "attention_bwd_drop: null pointer");
    const dim3 grid((unsigned)((S + XF_QB - 1) / XF_QB), H);
    const lq_dropout_src src = lq_dropout_src_make(snap, site, p);
    xf_for_width(D / H, [&](auto w) {
        hipLaunchKernelGGL((attention_bwd_q_kernel<w(), true>), grid, dim3(256), 0, (hipStream_t)stream, qkv, out, gout, lse, gqkv, delta,
                           nullptr, src.inv_keep, src, (int)S, D, H);
        hipLaunchKernelGGL((attention_bwd_kv_kernel<w(), true>), grid, dim3(256), 0, (hipStream_t)stream, qkv, gout, lse, delta, gqkv,
                           nullptr, src.inv_keep, src, (int)S, D, H);
    });
    return check_launch("attention_bwd_drop");
}
