// lipvq_misc.hip -- error plumbing, Lipschitz normalisation, straight-through value, mse reductions
// ABI and reference citations: include/lipvq.h.  Arithmetic contract: lipvq_math.h.
#include <stdlib.h>

#include "lipvq_common.h"

#undef fail
#undef check_launch
// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int lipvq_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int lipvq_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lipvq_fail(LIPVQ_EHIP, "%s: %s", what, hipGetErrorString(e));
    return LIPVQ_OK;
}

// ------------------------------------------------------------------------------------------
// options (include/lipvq.h): process-global, set EXPLICITLY through the ABI.  The shipped library reads no environment
// variable (round 3's thirteen getenv sites meant a stray variable silently changed the product's speed).  For one-off runs the
// Python binding forwards LIPVQ_<NAME> variables through lipvq_set_option when LIPVQ_DEV_KNOBS=1 (_capi.py).
// ------------------------------------------------------------------------------------------
static const char* const g_opt_names[] = {"screen_mode", "tok_shape", "tok_ze_rows", "tok_inplace", "tok_defer_ze", "tok_nt_ze"};
constexpr int kNumOpts = (int)(sizeof(g_opt_names) / sizeof(g_opt_names[0]));
static char g_opt_vals[kNumOpts][32];
static bool g_opt_set[kNumOpts];

static int opt_index(const char* name) {          // "screen_mode" or "LIPVQ_SCREEN_MODE"
    if (!name) return -1;
    if (!strncmp(name, "LIPVQ_", 6)) name += 6;
    for (int i = 0; i < kNumOpts; ++i) {
        const char* a = g_opt_names[i];
        const char* b = name;
        while (*a && *b && (*a == *b || *a == (*b | 0x20))) { ++a; ++b; }
        if (!*a && !*b) return i;
    }
    return -1;
}

const char* lq_knob(const char* name) {
    const int i = opt_index(name);
    if (i >= 0 && g_opt_set[i]) return g_opt_vals[i];
    return nullptr;
}

extern "C" int lipvq_set_option(const char* name, const char* value) {
    const int i = opt_index(name);
    if (i < 0) return lipvq_fail(LIPVQ_EINVAL, "set_option: unknown option '%s'", name ? name : "(null)");
    if (!value) { g_opt_set[i] = false; return LIPVQ_OK; }
    if (strlen(value) >= sizeof(g_opt_vals[i])) return lipvq_fail(LIPVQ_EINVAL, "set_option: value too long");
    strcpy(g_opt_vals[i], value);
    g_opt_set[i] = true;
    return LIPVQ_OK;
}

extern "C" const char* lipvq_get_option(const char* name) {
    const int i = opt_index(name);
    return (i >= 0 && g_opt_set[i]) ? g_opt_vals[i] : nullptr;
}

extern "C" int lipvq_abi_version(void) { return LIPVQ_ABI_VERSION; }
extern "C" const char* lipvq_last_error(void) { return g_err; }

#define fail lipvq_fail
#define check_launch lipvq_check_launch

// ------------------------------------------------------------------------------------------
// v5:6-12  Lipschitz normalisation
// ------------------------------------------------------------------------------------------
// 16 rows per workgroup: the rows are staged in LDS with coalesced loads, 16 threads then sum one row each IN INDEX ORDER
// (the canonical `s = s + |w[j]|` chain the oracle restates), all threads write Wn back coalesced.  (One thread per row
// straight from global memory walked 128 strided, dependent loads: 26 us per call at D = 208 -- more than either MLP launch
// of a training step.)
#define LIPS_ROWS 16
#define LIPS_HMAX 256
__global__ __launch_bounds__(256) void lipschitz_scale_kernel(const float* __restrict__ W, const float* __restrict__ ci,
                                                              float* __restrict__ scale, float* __restrict__ Wn, int D, int H) {
    __shared__ float ws[LIPS_ROWS][LIPS_HMAX + 1];
    __shared__ float s_sc[LIPS_ROWS];
    const int tid = threadIdx.x, r0 = blockIdx.x * LIPS_ROWS;
    for (int i = tid; i < LIPS_ROWS * H; i += 256) {
        const int r = i / H, j = i - r * H;
        ws[r][j] = (r0 + r < D) ? W[(size_t)(r0 + r) * H + j] : 0.0f;
    }
    __syncthreads();
    if (tid < LIPS_ROWS && r0 + tid < D) {
        float s = 0.0f;
        for (int j = 0; j < H; ++j) s = s + lq_abs(ws[tid][j]);
        float sc = lq_softplus(ci[r0 + tid]) / s;
        if (!(sc < 1.0f)) sc = 1.0f;
        s_sc[tid] = sc;
        if (scale) scale[r0 + tid] = sc;
    }
    __syncthreads();
    if (Wn)
        for (int i = tid; i < LIPS_ROWS * H; i += 256) {
            const int r = i / H, j = i - r * H;
            if (r0 + r < D) Wn[(size_t)(r0 + r) * H + j] = ws[r][j] * s_sc[r];
        }
}

extern "C" int lipvq_lipschitz_scale_f32(const float* W, const float* ci, float* scale, float* Wn,
                                         int D, int H, void* stream) {
    if (!W || !ci || D <= 0 || H <= 0) return fail(LIPVQ_EINVAL, "lipschitz_scale: bad argument");
    if (H > LIPS_HMAX) return fail(LIPVQ_EUNSUPPORTED, "lipschitz_scale: H=%d > %d", H, LIPS_HMAX);
    hipLaunchKernelGGL(lipschitz_scale_kernel, dim3((D + LIPS_ROWS - 1) / LIPS_ROWS), dim3(256), 0, (hipStream_t)stream,
                       W, ci, scale, Wn, D, H);
    return check_launch("lipschitz_scale");
}

// ------------------------------------------------------------------------------------------
// vq:74 straight-through value
// ------------------------------------------------------------------------------------------
__global__ void ste_kernel(const float* __restrict__ ze, const float* __restrict__ zq,
                           float* __restrict__ out, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = ze[i] + (zq[i] - ze[i]);
}

extern "C" int lipvq_ste_f32(const float* ze, const float* zq, float* out, int64_t n_elem, void* stream) {
    if (n_elem < 0) return fail(LIPVQ_EINVAL, "ste: n < 0");
    if (n_elem == 0) return LIPVQ_OK;
    if (!ze || !zq || !out) return fail(LIPVQ_EINVAL, "ste: null pointer");
    int64_t blocks = (n_elem + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(ste_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ze, zq, out, n_elem);
    return check_launch("ste");
}

// ------------------------------------------------------------------------------------------
// F.mse_loss pair: deterministic two-pass reduction in double
// ------------------------------------------------------------------------------------------
#define MSE_BLOCKS 2048

__device__ __forceinline__ double block_sum(double v, double* sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (l == 0) sh[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
    __syncthreads();
    return t;
}

// One launch for both pairs (blockIdx.y).  16-byte loads, two float4 pairs in flight per thread and four independent double
// accumulators (the first version -- one dword pair per iteration into one accumulator, one launch per pair -- read the
// 268 MB latent pair of a 524 288-row batch at 1.8 TB/s); the head up to the first aligned element and the tail are scalar.
__global__ __launch_bounds__(256) void mse_partial_kernel(const float* __restrict__ a0, const float* __restrict__ b0, int64_t n0,
                                                          const float* __restrict__ a1, const float* __restrict__ b1, int64_t n1,
                                                          double* __restrict__ partial) {
    __shared__ double sh[4];
    const float* __restrict__ a = blockIdx.y ? a1 : a0;
    const float* __restrict__ b = blockIdx.y ? b1 : b0;
    const int64_t n = blockIdx.y ? n1 : n0;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    auto sq = [](float x, float y) { const double d = (double)x - (double)y; return d * d; };
    const bool vec = ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0;
    const int64_t n4 = vec ? n / 4 : 0;
    const float4* __restrict__ a4 = reinterpret_cast<const float4*>(a);
    const float4* __restrict__ b4 = reinterpret_cast<const float4*>(b);
    int64_t i = tid;
    for (; i + nth < n4; i += 2 * nth) {
        const float4 x = a4[i], y = b4[i], u = a4[i + nth], v = b4[i + nth];
        s0 += sq(x.x, y.x); s1 += sq(x.y, y.y); s2 += sq(x.z, y.z); s3 += sq(x.w, y.w);
        s0 += sq(u.x, v.x); s1 += sq(u.y, v.y); s2 += sq(u.z, v.z); s3 += sq(u.w, v.w);
    }
    if (i < n4) {
        const float4 x = a4[i], y = b4[i];
        s0 += sq(x.x, y.x); s1 += sq(x.y, y.y); s2 += sq(x.z, y.z); s3 += sq(x.w, y.w);
    }
    for (int64_t j = 4 * n4 + tid; j < n; j += nth) s0 += sq(a[j], b[j]);
    const double t = block_sum((s0 + s1) + (s2 + s3), sh);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// out[0], out[1] = the two means; with `loss` also the tokenizer's loss from them in the reference's fp32 association
// (LIPVQ_LOSS_LLFQ: (m0 + w m1) + w m1, backbone_lfqvae_v5.py:83;  LIPVQ_LOSS_VQ: m0 + (m1 + w m1), backbone.py:50-51,69-71) --
// three tiny torch kernels per training step otherwise.
__global__ __launch_bounds__(256) void mse_final_kernel(const double* __restrict__ partial, int64_t nx, int64_t nz,
                                                        float* __restrict__ out, float* __restrict__ loss, float w, int form) {
    __shared__ double sh[4];
    float m[2] = {0.0f, 0.0f};
    for (int which = 0; which < 2; ++which) {
        double acc = 0.0;
        for (int i = threadIdx.x; i < MSE_BLOCKS; i += blockDim.x) acc += partial[which * MSE_BLOCKS + i];
        const double t = block_sum(acc, sh);
        m[which] = (float)(t / (double)(which == 0 ? nx : nz));
        if (threadIdx.x == 0) out[which] = m[which];
    }
    if (loss && threadIdx.x == 0) {
        const float q = w * m[1];
        *loss = form == LIPVQ_LOSS_VQ ? m[0] + (m[1] + q) : (m[0] + q) + q;
    }
}

extern "C" size_t lipvq_mse_workspace_bytes(void) { return 2 * MSE_BLOCKS * sizeof(double); }

static int mse_pair_launch(const float* xr, const float* x, int64_t nx, const float* zq, const float* ze, int64_t nz, float* out,
                           float* loss, float w, int form, void* workspace, void* stream, const char* who) {
    if (!xr || !x || !zq || !ze || !out || !workspace || nx <= 0 || nz <= 0) return fail(LIPVQ_EINVAL, "%s: bad argument", who);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(mse_partial_kernel, dim3(MSE_BLOCKS, 2), dim3(256), 0, st, xr, x, nx, zq, ze, nz, part);
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, st, part, nx, nz, out, loss, w, form);
    return check_launch(who);
}

int lipvq_mse_finish(const double* partial, int64_t nx, int64_t nz, float* out, float* loss, float w, int form, void* stream) {
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, nx, nz, out, loss, w, form);
    return check_launch("mse_finish");
}

extern "C" int lipvq_mse_pair_f32(const float* xr, const float* x, int64_t nx, const float* zq,
                                  const float* ze, int64_t nz, float* out2, void* workspace, void* stream) {
    return mse_pair_launch(xr, x, nx, zq, ze, nz, out2, nullptr, 0.0f, 0, workspace, stream, "mse_pair");
}

extern "C" int lipvq_mse_pair_loss_f32(const float* xr, const float* x, int64_t nx, const float* zq, const float* ze, int64_t nz,
                                       float* out3, float w, int form, void* workspace, void* stream) {
    if (form != LIPVQ_LOSS_LLFQ && form != LIPVQ_LOSS_VQ) return fail(LIPVQ_EINVAL, "mse_pair_loss: unknown loss form %d", form);
    return mse_pair_launch(xr, x, nx, zq, ze, nz, out3, out3 ? out3 + 2 : nullptr, w, form, workspace, stream, "mse_pair_loss");
}


int lipvq_reserve_lds(LqLdsReserve& r, const void* kernel, size_t bytes, const char* what) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(LIPVQ_EHIP, "%s: no current device", what);
    const bool tracked = dev >= 0 && dev < LqLdsReserve::kMaxDev;
    if (tracked && bytes <= r.got[dev].load(std::memory_order_acquire)) return LIPVQ_OK;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail(LIPVQ_EHIP, "%s: cannot reserve %zu B of LDS: %s", what, bytes, hipGetErrorString(e));
    if (tracked) {
        size_t cur = r.got[dev].load(std::memory_order_relaxed);
        while (cur < bytes && !r.got[dev].compare_exchange_weak(cur, bytes, std::memory_order_release)) {}
    }
    return LIPVQ_OK;
}
