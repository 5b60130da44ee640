// lipvq_optim.hip -- the policy's parameter update (reference robomimic/utils/torch_utils.py:196-234 backprop_for_loss:
// clip_grad_norm_ over the whole parameter list, a Python loop of p.grad.norm(2).pow(2).item() -- one host synchronisation per
// parameter --, then optim.Adam.step(); robomimic/algo/icl.py:215-226 calls it every iteration) without a host synchronisation:
//
//   lipvq_grad_sumsq_f32   sum of squares of a gradient LIST, each tensor into 64 fixed double slots (one per workgroup)
//   lipvq_clip_coef_f64    the slots summed in a fixed order -> stats = [total_norm, clip_coef, sumsq, sumsq_clipped] on the device
//   lipvq_grad_scale_f32   g *= (float)clip_coef for a list (the stand-alone clip_grad_norm_)
//   lipvq_adam_f32         Adam (coupled L2) or AdamW for a list, reading the coefficient and the learning rate on the device
//
// Every element is squared in double (a 24 x 24-bit product is exact there: nothing overflows at 1e15 or underflows at 1e-30)
// and summed in double; there are no atomics, and which elements meet in which slot depends on the list and the sizes alone,
// so two runs give the same bits.  All four are bandwidth bound: float4 loads where the layout allows, plain stores.
#include "lipvq_common.h"
#include "lipvq_optim.h"

#define LQ_SUMSQ_SLOTS 64          // workgroups, and so partial sums, per tensor

struct GradListArgs {
    float* g[LIPVQ_ADAMW_MAX];
    long long n[LIPVQ_ADAMW_MAX];
};

// Sum over the 256 threads of a workgroup in a fixed order (shuffles inside each wave, then the four waves left to right); every
// thread returns the sum.
__device__ __forceinline__ double lq_block_sum256(double s) {
    __shared__ double part[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// A tensor of n floats at any 4-byte alignment as  head (0..3 floats up to the next 16-byte boundary) | nv float4 | tail (0..3).
struct LqSplit16 {
    long long head, nv, tail0, ntail;
};
__device__ __forceinline__ LqSplit16 lq_split16(const float* g, long long n) {
    LqSplit16 s;
    s.head = (long long)(((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) >> 2);
    if (s.head > n) s.head = n;
    s.nv = (n - s.head) >> 2;
    s.tail0 = s.head + 4 * s.nv;
    s.ntail = n - s.tail0;
    return s;
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(GradListArgs a, double* __restrict__ slots) {
    const int t = blockIdx.y;
    const float* __restrict__ g = a.g[t];
    const LqSplit16 sp = lq_split16(g, a.n[t]);
    const float4* __restrict__ gv = (const float4*)(g + sp.head);
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < sp.nv; i += (long long)LQ_SUMSQ_SLOTS * 256) {
        const float4 q = gv[i];
        s += (double)q.x * (double)q.x;
        s += (double)q.y * (double)q.y;
        s += (double)q.z * (double)q.z;
        s += (double)q.w * (double)q.w;
    }
    if (blockIdx.x == 0) {                                  // the at most 3 + 3 floats around the float4 body, one thread each
        const long long k = threadIdx.x;
        if (k < sp.head) {
            const double x = (double)g[k];
            s += x * x;
        } else if (k - sp.head < sp.ntail) {
            const double x = (double)g[sp.tail0 + (k - sp.head)];
            s += x * x;
        }
    }
    s = lq_block_sum256(s);
    if (threadIdx.x == 0) slots[(long long)t * LQ_SUMSQ_SLOTS + blockIdx.x] = s;
}

// torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False): coef = clamp(max_norm / (norm + 1e-6), max = 1); a NaN norm gives a
// NaN coefficient (the comparison below is false), an infinite one 0.
__global__ __launch_bounds__(256) void clip_coef_kernel(const double* __restrict__ slots, long long nslots, double max_norm,
                                                        double* __restrict__ stats) {
    double s = 0.0;
    for (long long i = threadIdx.x; i < nslots; i += 256) s += slots[i];
    s = lq_block_sum256(s);
    if (threadIdx.x == 0) {
        const double norm = sqrt(s);
        double coef = max_norm / (norm + 1e-6);
        if (coef > 1.0) coef = 1.0;
        stats[0] = norm;
        stats[1] = coef;
        stats[2] = s;
        stats[3] = coef * coef * s;
    }
}

__global__ __launch_bounds__(256) void grad_scale_kernel(GradListArgs a, const double* __restrict__ stats) {
    const int t = blockIdx.y;
    float* g = a.g[t];
    const float c = (float)stats[1];
    const LqSplit16 sp = lq_split16(g, a.n[t]);
    float4* gv = (float4*)(g + sp.head);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < sp.nv; i += (long long)gridDim.x * 256) {
        float4 q = gv[i];
        q.x *= c; q.y *= c; q.z *= c; q.w *= c;
        gv[i] = q;
    }
    if (blockIdx.x == 0) {
        const long long k = threadIdx.x;
        if (k < sp.head) g[k] *= c;
        else if (k - sp.head < sp.ntail) g[sp.tail0 + (k - sp.head)] *= c;
    }
}

// adamw_kernel's element arithmetic (lipvq_bwd.hip) with three additions, each uniform over the launch:
//   CLIP       g' = g * (float)clip_coef, rounded to fp32 once -- the value torch's mul_ would have stored; g itself is not written
//   !DECOUPLED torch.optim.Adam's L2 term: g' = g' + wd p in fp32 before the moments (skipped when wd == 0, as torch skips
//              it), and no p *= 1 - lr wd
//   lr_dev     the step size and the decay factor formed from the device scalar: a scheduler's fill_ reaches a captured graph
template <bool DECOUPLED, bool CLIP>
__global__ __launch_bounds__(256) void adam_kernel(AdamwArgs a, float lr, float decay, double wd, const float* __restrict__ lr_dev,
                                                   const double* __restrict__ stats, float omb1, float beta2, float omb2, float eps,
                                                   const float* __restrict__ bc) {
    const int t = blockIdx.y;
    float* __restrict__ p = a.p[t];
    const float* __restrict__ g = a.g[t];
    float* __restrict__ m = a.m[t];
    float* __restrict__ v = a.v[t];
    const long long n = a.n[t];
    if (lr_dev) {
        lr = lr_dev[0];
        decay = (float)(1.0 - (double)lr * wd);
    }
    const float wdf = (float)wd;
    const float coef = CLIP ? (float)stats[1] : 1.0f;
    const float step_size = lr / bc[2 * t], bc2s = bc[2 * t + 1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float gi = g[i];
        if (CLIP) gi = gi * coef;
        float pi = p[i];
        if (DECOUPLED) pi = pi * decay;
        else if (wdf != 0.0f) gi = gi + wdf * pi;
        const float mi = m[i] + (gi - m[i]) * omb1;
        const float vi = v[i] * beta2 + omb2 * gi * gi;
        m[i] = mi;
        v[i] = vi;
        pi = pi - step_size * (mi / (lq_sqrt(vi) / bc2s + eps));
        p[i] = pi;
    }
}

static int grad_list(const char* what, float* const* grads, const int64_t* numels, int count, GradListArgs& a, long long& nmax) {
    if (!grads || !numels) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if (count <= 0 || count > LIPVQ_ADAMW_MAX) return fail(LIPVQ_EINVAL, "%s: %d tensors (1..%d per call)", what, count, LIPVQ_ADAMW_MAX);
    nmax = 0;
    for (int i = 0; i < count; ++i) {
        if (!grads[i] || numels[i] <= 0) return fail(LIPVQ_EINVAL, "%s: tensor %d has a null pointer or no elements", what, i);
        a.g[i] = grads[i];
        a.n[i] = numels[i];
        if (numels[i] > nmax) nmax = numels[i];
    }
    return LIPVQ_OK;
}

extern "C" size_t lipvq_grad_sumsq_workspace_bytes(int64_t tensors) {
    return tensors <= 0 ? 0 : (size_t)tensors * LQ_SUMSQ_SLOTS * sizeof(double);
}

extern "C" int lipvq_grad_sumsq_f32(const float* const* grads, const int64_t* numels, int count, int64_t first, int64_t tensors,
                                    void* workspace, void* stream) {
    GradListArgs a;
    long long nmax;
    int rc = grad_list("grad_sumsq", (float* const*)grads, numels, count, a, nmax);
    if (rc) return rc;
    if (!workspace) return fail(LIPVQ_EINVAL, "grad_sumsq: no workspace");
    if (first < 0 || first + count > tensors)
        return fail(LIPVQ_EINVAL, "grad_sumsq: tensors %lld..%lld of a workspace for %lld", (long long)first, (long long)first + count - 1,
                    (long long)tensors);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(LQ_SUMSQ_SLOTS, count), dim3(256), 0, (hipStream_t)stream, a,
                       (double*)workspace + first * LQ_SUMSQ_SLOTS);
    return check_launch("grad_sumsq");
}

extern "C" int lipvq_clip_coef_f64(const void* workspace, int64_t tensors, double max_norm, double* stats, void* stream) {
    if (!workspace) return fail(LIPVQ_EINVAL, "clip_coef: no workspace");
    if (!stats) return fail(LIPVQ_EINVAL, "clip_coef: null pointer");
    if (tensors <= 0) return fail(LIPVQ_EINVAL, "clip_coef: %lld tensors", (long long)tensors);
    if (!(max_norm >= 0.0)) return fail(LIPVQ_EINVAL, "clip_coef: max_norm = %g (>= 0; +inf reports only)", max_norm);
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace,
                       (long long)tensors * LQ_SUMSQ_SLOTS, max_norm, stats);
    return check_launch("clip_coef");
}

extern "C" int lipvq_grad_scale_f32(float* const* grads, const int64_t* numels, int count, const double* stats, void* stream) {
    GradListArgs a;
    long long nmax;
    int rc = grad_list("grad_scale", grads, numels, count, a, nmax);
    if (rc) return rc;
    if (!stats) return fail(LIPVQ_EINVAL, "grad_scale: null pointer");
    long long gx = (nmax + 4095) / 4096;
    if (gx > 256) gx = 256;
    hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)gx, count), dim3(256), 0, (hipStream_t)stream, a, stats);
    return check_launch("grad_scale");
}

extern "C" int lipvq_adam_f32(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                              float* const* steps, const int64_t* numels, int count, double lr, double beta1, double beta2, double eps,
                              double weight_decay, int decoupled, const float* lr_dev, const double* stats, void* workspace,
                              void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !steps || !numels) return fail(LIPVQ_EINVAL, "adam: null pointer");
    if (!workspace) return fail(LIPVQ_EINVAL, "adam: no workspace");
    if (count <= 0 || count > LIPVQ_ADAMW_MAX) return fail(LIPVQ_EINVAL, "adam: %d tensors (1..%d per call)", count, LIPVQ_ADAMW_MAX);
    if (decoupled != 0 && decoupled != 1) return fail(LIPVQ_EINVAL, "adam: decoupled = %d (0: Adam's L2, 1: AdamW)", decoupled);
    AdamwArgs a;
    long long nmax = 0;
    for (int i = 0; i < count; ++i) {
        if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || !steps[i] || numels[i] <= 0)
            return fail(LIPVQ_EINVAL, "adam: tensor %d has a null pointer or no elements", i);
        a.p[i] = params[i]; a.g[i] = grads[i]; a.m[i] = exp_avg[i]; a.v[i] = exp_avg_sq[i]; a.step[i] = steps[i];
        a.n[i] = numels[i];
        if (numels[i] > nmax) nmax = numels[i];
    }
    a.count = count;
    hipStream_t st = (hipStream_t)stream;
    lipvq_adamw_launch_steps(a, beta1, beta2, (float*)workspace, st);
    long long gx = (nmax + 1023) / 1024;
    if (gx > 256) gx = 256;
    const dim3 grid((unsigned)gx, count), block(256);
    // the same host-side constants as lipvq_adamw_f32: formed in double, rounded to fp32 once
    const float lrf = (float)lr, decay = (float)(1.0 - lr * weight_decay), omb1 = (float)(1.0 - beta1), b2 = (float)beta2,
                omb2 = (float)(1.0 - beta2), epsf = (float)eps;
    const float* bc = (const float*)workspace;
#define LQ_ADAM_LAUNCH(D, C) \
    hipLaunchKernelGGL((adam_kernel<D, C>), grid, block, 0, st, a, lrf, decay, weight_decay, lr_dev, stats, omb1, b2, omb2, epsf, bc)
    if (decoupled) { if (stats) LQ_ADAM_LAUNCH(true, true); else LQ_ADAM_LAUNCH(true, false); }
    else           { if (stats) LQ_ADAM_LAUNCH(false, true); else LQ_ADAM_LAUNCH(false, false); }
#undef LQ_ADAM_LAUNCH
    return check_launch("adam");
}
