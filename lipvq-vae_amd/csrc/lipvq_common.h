// lipvq_common.h -- shared by every translation unit of the gfx950 tokenizer library.
#ifndef LIPVQ_COMMON_H_
#define LIPVQ_COMMON_H_
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/lipvq.h"
#include "lipvq_math.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Dynamic-LDS reservation of a kernel (hipFuncAttributeMaxDynamicSharedMemorySize): the attribute belongs to the (function,
// device) pair, so the "already raised to" bookkeeping is kept PER DEVICE and in atomics -- a process that drives several
// GPUs, or several host threads, must not launch with more LDS than the current device has been told about.  (The first
// version kept one `static size_t` per kernel: per process, unsynchronised.)  The attribute call costs ~10 us of host
// time, hence the bookkeeping; a lost race only repeats the call.
#ifdef __cplusplus
#include <atomic>
struct LqLdsReserve {
    static constexpr int kMaxDev = 64;
    std::atomic<size_t> got[kMaxDev];
};
int lipvq_reserve_lds(LqLdsReserve& r, const void* kernel, size_t bytes, const char* what);

// A runtime value as a compile-time constant (a latent width, a distance rule picking a template instance): calls
// f(std::integral_constant<int, V>{}) for the V of the list that equals v and returns true, or calls nothing and returns false.
#include <type_traits>
template <typename F>
static inline bool lq_dispatch(int, F&&) { return false; }
template <int V, int... Vs, typename F>
static inline bool lq_dispatch(int v, F&& f) {
    if (v == V) { f(std::integral_constant<int, V>{}); return true; }
    return lq_dispatch<Vs...>(v, f);
}
#endif

#if defined(__HIPCC__)
// Workgroup barrier that does NOT drain vector-memory operations: this wave's LDS accesses are done (lgkmcnt(0)), then
// s_barrier.  __syncthreads() makes hipcc wait vmcnt(0) first, i.e. for every global load / LDS-DMA still in flight --
// which defeats any prefetch that is meant to stay in flight across the barrier.  Global data is waited for where it is
// consumed (hipcc's own counted vmcnt for ordinary loads; lq_wait_vmcnt for LDS-DMA).
__device__ __forceinline__ void lq_wg_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
#endif

#if defined(__HIPCC__)
// usage[k] += 1 for every lane with `active`, with duplicates inside the wave combined first: when many rows map
// to few codes (the reference's default initialisation maps EVERY row to one code) per-row atomics on one address
// serialise chip-wide (measured: 1.7 ms instead of 0.57 ms for a 524 288-row batch with 32 codes).  Up to four
// leader rounds (each: the first active lane's code, a ballot of the lanes that share it, ONE atomic of the count)
// then plain atomics for whatever is left (the typical well-spread case pays four cheap rounds).
__device__ __forceinline__ void lq_usage_add(unsigned long long* __restrict__ usage, int k, bool active) {
#pragma unroll 1
    for (int round = 0; round < 4; ++round) {
        const unsigned long long act = __ballot(active);
        if (act == 0ull) return;                                   // wave-uniform
        const int leader = __ffsll((long long)act) - 1;
        const int kl = __shfl(k, leader, 64);
        const unsigned long long same = __ballot(active && k == kl);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&usage[kl], (unsigned long long)__popcll(same));
        active = active && k != kl;
    }
    if (active) atomicAdd(&usage[k], 1ull);
}

// torch.argmin's first minimum over (value, code) pairs: (v, k) takes (ov, ok) if ov is smaller, or equal with a lower code.
// LQ_WAVE_MIN applies it across the lanes of a wave that differ in lane bits OFF0 and up (OFF0 = 1: all 64 lanes; 4 or 8: per
// lane class mod OFF0); every lane ends with its class's result.  Macros, not functions: hipcc simplifies an inline function's
// body before it inlines it, and the fused tokenize kernel (lq_lists_row) then compiled to different code; a macro expands to
// the statements the kernels had.  Arguments are evaluated more than once: pass variables.
#define LQ_TAKE_MIN(v, k, ov, ok) { if ((ov) < (v) || ((ov) == (v) && (ok) < (k))) { (v) = (ov); (k) = (ok); } }
#define LQ_WAVE_MIN(v, k, OFF0)                                                                                   \
    _Pragma("unroll") for (int lq_off = (OFF0); lq_off < 64; lq_off <<= 1) {                                      \
        const float lq_ov = __shfl_xor(v, lq_off, 64);                                                            \
        const int lq_ok = __shfl_xor(k, lq_off, 64);                                                              \
        LQ_TAKE_MIN(v, k, lq_ov, lq_ok);                                                                          \
    }
#endif

// measurement / test knobs: ONE place reads them (lipvq_misc.hip)
const char* lq_knob(const char* name);

// error plumbing (defined in lipvq_misc.hip)
int lipvq_fail(int code, const char* fmt, ...);
int lipvq_check_launch(const char* what);
// lipvq_misc.hip: the second pass of the mean-squared-error pair over 2 x 2048 double partial sums (what lipvq_mse_pair_loss_f32
// runs after its own first pass; lipvq_mlp3_loss_f32's first pass is the decoder kernel itself)
int lipvq_mse_finish(const double* partial, int64_t nx, int64_t nz, float* out, float* loss, float w, int form, void* stream);
#define fail lipvq_fail
#define check_launch lipvq_check_launch

// what every entry point of the in-kernel dropout source refuses (include/lipvq.h, "in-kernel dropout"): 0 < p < 1, a snap to
// read, and a field whose rows fit the 32-bit counter word
static inline int lq_dropout_check_p(const char* what, double p) {
    if (!(p > 0.0 && p < 1.0)) return fail(LIPVQ_EINVAL, "%s: dropout p=%g (0 < p < 1)", what, p);
    return 0;
}
static inline int lq_dropout_check(const char* what, const void* snap, double p, int64_t rows) {
    if (int rc = lq_dropout_check_p(what, p)) return rc;
    if (rows >= (1LL << 32)) return fail(LIPVQ_EUNSUPPORTED, "%s: %lld rows of decisions (< 2^32)", what, (long long)rows);
    if (!snap) return fail(LIPVQ_EINVAL, "%s: null snap", what);
    return 0;
}

__host__ __device__ static inline float lq_act_apply(float v, int act) {
    switch (act) {
        case LIPVQ_ACT_GELU: return lq_gelu(v);
        case LIPVQ_ACT_SIGMOID: return lq_sigmoid(v);
        case LIPVQ_ACT_RELU: return v <= 0.0f ? 0.0f : v;            // torch.relu: a NaN stays a NaN
        default: return v;
    }
}

// d act(v) / d v evaluated at the pre-activation v
__host__ __device__ static inline float lq_act_grad(float v, int act) {
    switch (act) {
#if defined(__HIP_DEVICE_COMPILE__)
        case LIPVQ_ACT_GELU: return lq_gelu_grad_dev(v);          // straight-line form (lipvq_math.h), 2e-7 from lq_gelu_grad
#else
        case LIPVQ_ACT_GELU: return lq_gelu_grad(v);
#endif
        case LIPVQ_ACT_SIGMOID: { const float s = lq_sigmoid(v); return s * (1.0f - s); }
        case LIPVQ_ACT_RELU: return v <= 0.0f ? 0.0f : 1.0f;          // torch's threshold_backward: the gradient passes at a NaN
        default: return 1.0f;
    }
}

// g * d act(pre) / d pre, as torch's backward functions form it: ReLU SELECTS (threshold_backward: 0 where pre <= 0 whatever g is,
// g itself -- a NaN or an infinity included -- elsewhere, also at a NaN pre); the others multiply, so a non-finite g stays non-finite
__host__ __device__ static inline float lq_act_bwd(float g, float pre, int act) {
    if (act == LIPVQ_ACT_RELU) return pre <= 0.0f ? 0.0f : g;
    return g * lq_act_grad(pre, act);
}
#endif
