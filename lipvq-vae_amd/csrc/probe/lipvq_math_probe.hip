// lipvq_math_probe.hip -- TEST SUPPORT, not part of the shipped ABI (include/lipvq.h does not know it).
//
// Runs the canonical arithmetic of lipvq_math.h / lipvq_rng.h on the device one fp32 bit pattern at a time, so that the suite can
// walk every input there is (tests/test_gpu_math_exhaustive.py, through tests/math_probe.py).  Built by csrc/Makefile with the
// library's own FLAGS into lipvq-vae_amd/_lipvq_probe.so: it sees the arithmetic the library sees.  Three kinds of entry point:
//   lq_probe_map   out[i] = f(in[i])                                          (device against host, bit for bit)
//   lq_probe_same  two forms of one function on every pattern of a range      (count of differing patterns, the lowest of them)
//   lq_probe_err   one function against a float64 reference formed on the device from ROCm's double exp / erf / log1p / sqrt
//   lq_probe_ref   that float64 reference itself, for the host to hold against numpy / scipy
// Every kernel is a grid-stride loop over the counts it is given, takes a stream, and reports through a small result array with
// atomicAdd / atomicMax / atomicMin on global memory (one set per thread, after its loop).  Pointers are device pointers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../lipvq_math.h"
#include "../lipvq_rng.h"

namespace {

constexpr int kThreads = 256, kBlocks = 4096;
constexpr uint32_t kGold = 0x9E3779B9u;
typedef unsigned long long u64;

// the result array of lq_probe_same and lq_probe_err: LQ_PROBE_NRES u64 words
enum { R_BAD = 0,      // same: patterns whose two forms differ           err: patterns whose class differs from the reference
       R_WHERE = 1,    // same: the lowest such pattern (~0: none)        err: (bits of the max error as float, rounded up) << 32 | a pattern that attains it
       R_SKIPPED = 2,  // patterns of the range outside the function's domain
       R_DONE = 3,     // patterns evaluated (R_SKIPPED + R_DONE = count)
       R_AUX = 4,      // four counters of the pair's own (the division sweep: see P_DIV)
       LQ_PROBE_NRES = 8 };

// An empty asm statement the value passes through: the compiler cannot see across it.  Without it LLVM may rewrite one form into
// the other before it is compared (packed into scalar ops, (float)((double)a / (double)b) into a / b -- a legal fold).
__device__ __forceinline__ void opaque(lq_v2f& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void opaque(float& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void opaque(double& v) { asm volatile("" : "+v"(v)); }

__device__ __forceinline__ bool is_nan(float a) { return a != a; }
__device__ __forceinline__ bool finite_bits(uint32_t p) { return (p & 0x7f800000u) != 0x7f800000u; }
// == on the bits; two NaNs count as equal
__device__ __forceinline__ bool same_bits(float a, float b) { return lq_f2u(a) == lq_f2u(b) || (is_nan(a) && is_nan(b)); }
__device__ __forceinline__ uint32_t fmix32(uint32_t h) {        // MurmurHash3's finaliser: a bijection of the 32-bit words
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// ---- map -------------------------------------------------------------------------------------------------------------------------
enum { F_EXP = 0, F_ERF, F_GELU, F_SIGMOID, F_SOFTPLUS, F_GELU_GRAD, F_LOG_GE1, F_SQRT, F_GELU_POLY, F_GELU_TAIL,   // 0..9: lq_ref_math_probe's numbers
       F_GELU_GRAD_DEV, F_ICDF_WORD, F_COUNT };

template <int FN>
__device__ __forceinline__ float map_fn(uint32_t p) {
    const float x = lq_u2f(p);
    if constexpr (FN == F_EXP) return lq_expf(x);
    if constexpr (FN == F_ERF) return lq_erff(x);
    if constexpr (FN == F_GELU) return lq_gelu(x);
    if constexpr (FN == F_SIGMOID) return lq_sigmoid(x);
    if constexpr (FN == F_SOFTPLUS) return lq_softplus(x);
    if constexpr (FN == F_GELU_GRAD) return lq_gelu_grad(x);
    if constexpr (FN == F_LOG_GE1) return lq_logf_ge1(x);
    if constexpr (FN == F_SQRT) return lq_sqrt(x);
    if constexpr (FN == F_GELU_POLY) return lq_gelu_poly(x);
    if constexpr (FN == F_GELU_TAIL) return lq_gelu_tail(x);
    if constexpr (FN == F_GELU_GRAD_DEV) return lq_gelu_grad_dev(x);
    if constexpr (FN == F_ICDF_WORD) return lq_normal_icdf(lq_sample_open(p));
    return x;
}

template <int FN>
__global__ __launch_bounds__(kThreads) void map_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) out[i] = lq_f2u(map_fn<FN>(in[i]));
}

// ---- the float64 references ------------------------------------------------------------------------------------------------------
enum { D_EXP = 0, D_ERF, D_LOG1P, D_SQRT, D_COUNT };

template <int FN>
__global__ __launch_bounds__(kThreads) void ref_kernel(const uint32_t* __restrict__ in, double* __restrict__ out, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const double x = (double)lq_u2f(in[i]);
        double r;
        if constexpr (FN == D_EXP) r = exp(x);
        if constexpr (FN == D_ERF) r = erf(x);
        if constexpr (FN == D_LOG1P) r = log1p(x);
        if constexpr (FN == D_SQRT) r = sqrt(x);
        out[i] = r;
    }
}

// ---- same ------------------------------------------------------------------------------------------------------------------------
enum { P_GELU2 = 0,      // lq_gelu_poly2, either lane                      against lq_gelu_poly           every pattern
       P_GELU2X4,        // lq_gelu_poly2xN<4>, each of the 8 positions     against lq_gelu_poly           every pattern
       P_SIG2,           // lq_sigmoid2_finite, either lane                 against lq_sigmoid             finite patterns
       P_SIG2X4,         // lq_sigmoid2_finite_xN<4>, each of 8 positions   against lq_sigmoid             finite patterns
       P_RCP2,           // lq_rcp2_ge1(d), either lane                     against 1.0f / d               [0x3F800000, 0x7E800000)
       P_SIG_EXP,        // lq_sigmoid(x)                                   against 1 / (1 + lq_expf(-x))  |x| <= 87
       P_GRAD_TAIL,      // lq_gelu_grad_dev                                against lq_gelu_grad           !(x * x < 18)
       P_NONFINITE,      // lq_nonfinite_acc2(x, 0), either lane            +-0 if x is finite, else NaN   every pattern
       P_SQRT,           // lq_sqrt(x)                                      against (float)sqrt((double)x) x >= 0 and NaN
       P_DIV,            // a / b, both hashed from the counter             against (float)((double)a / (double)b)
       P_RCP_1PE,        // 1.0f / (1.0f + e)                               the same in double             e normal, below 2^126
       P_COUNT };

// Element k of the values that travel with pattern p through a packed form: k = 0 is p itself, the others differ from it and from
// each other, so a result that comes back from the wrong chain is a mismatch.  Folded into the form's domain.
enum { DOM_ALL, DOM_FINITE, DOM_RCP };
template <int DOM>
__device__ __forceinline__ uint32_t companion(uint32_t p, uint32_t k) {
    uint32_t c = p + k * kGold;
    if (k == 0) return c;
    if constexpr (DOM == DOM_FINITE) { if (!finite_bits(c)) c &= ~0x00800000u; }
    if constexpr (DOM == DOM_RCP) c = 0x3F800000u + c % 0x3F000000u;
    return c;
}

enum { ST_OK = 0, ST_BAD = 1, ST_SKIP = 2 };

// a one-pair form FORM against the scalar SCALAR with p in lane 0, then in lane 1
template <int DOM, typename FORM, typename SCALAR>
__device__ __forceinline__ int check_pair(uint32_t p, FORM form, SCALAR scalar) {
    const uint32_t c = companion<DOM>(p, 1);
    const float rp = scalar(lq_u2f(p)), rc = scalar(lq_u2f(c));
    bool bad = false;
#pragma unroll
    for (int lane = 0; lane < 2; ++lane) {
        lq_v2f x = lane == 0 ? (lq_v2f){lq_u2f(p), lq_u2f(c)} : (lq_v2f){lq_u2f(c), lq_u2f(p)};
        opaque(x);
        lq_v2f y = form(x);
        opaque(y);
        bad |= !same_bits(lane == 0 ? y.x : y.y, rp) || !same_bits(lane == 0 ? y.y : y.x, rc);
    }
    return bad ? ST_BAD : ST_OK;
}

// a four-pair lockstep form against the scalar with p in each of the eight positions
template <int DOM, typename FORM, typename SCALAR>
__device__ __forceinline__ int check_x4(uint32_t p, FORM form, SCALAR scalar) {
    bool bad = false;
#pragma unroll 1
    for (uint32_t k = 0; k < 8; ++k) {
        lq_v2f x[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            x[j] = (lq_v2f){lq_u2f(companion<DOM>(p, (2 * j - k) & 7u)), lq_u2f(companion<DOM>(p, (2 * j + 1 - k) & 7u))};
            opaque(x[j]);
        }
        form(x);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            opaque(x[j]);
            bad |= !same_bits(x[j].x, scalar(lq_u2f(companion<DOM>(p, (2 * j - k) & 7u))));
            bad |= !same_bits(x[j].y, scalar(lq_u2f(companion<DOM>(p, (2 * j + 1 - k) & 7u))));
        }
    }
    return bad ? ST_BAD : ST_OK;
}

template <int PAIR>
__device__ __forceinline__ int check(u64 i, [[maybe_unused]] u64 (&aux)[4]) {
    const uint32_t p = (uint32_t)i;
    [[maybe_unused]] const float x = lq_u2f(p);
    if constexpr (PAIR == P_GELU2)
        return check_pair<DOM_ALL>(p, [](lq_v2f v) { return lq_gelu_poly2(v); }, [](float v) { return lq_gelu_poly(v); });
    if constexpr (PAIR == P_GELU2X4)
        return check_x4<DOM_ALL>(p, [](lq_v2f (&v)[4]) { lq_gelu_poly2xN<4>(v); }, [](float v) { return lq_gelu_poly(v); });
    if constexpr (PAIR == P_SIG2) {
        if (!finite_bits(p)) return ST_SKIP;
        return check_pair<DOM_FINITE>(p, [](lq_v2f v) { return lq_sigmoid2_finite(v); }, [](float v) { return lq_sigmoid(v); });
    }
    if constexpr (PAIR == P_SIG2X4) {
        if (!finite_bits(p)) return ST_SKIP;
        return check_x4<DOM_FINITE>(p, [](lq_v2f (&v)[4]) { lq_sigmoid2_finite_xN<4>(v); }, [](float v) { return lq_sigmoid(v); });
    }
    if constexpr (PAIR == P_RCP2) {
        if (p < 0x3F800000u || p >= 0x7E800000u) return ST_SKIP;
        return check_pair<DOM_RCP>(p, [](lq_v2f v) { return lq_rcp2_ge1(v); }, [](float v) { return 1.0f / v; });
    }
    if constexpr (PAIR == P_SIG_EXP) {
        if (!(lq_abs(x) <= 87.0f)) return ST_SKIP;
        float a = x, b = x;
        opaque(a); opaque(b);
        return same_bits(lq_sigmoid(a), 1.0f / (1.0f + lq_expf(-b))) ? ST_OK : ST_BAD;
    }
    if constexpr (PAIR == P_GRAD_TAIL) {
        if (x * x < 18.0f) return ST_SKIP;
        float a = x, b = x;
        opaque(a); opaque(b);
        return same_bits(lq_gelu_grad_dev(a), lq_gelu_grad(b)) ? ST_OK : ST_BAD;
    }
    if constexpr (PAIR == P_NONFINITE) {
        const uint32_t c = companion<DOM_FINITE>(p, 1);
        bool bad = false;
#pragma unroll
        for (int lane = 0; lane < 2; ++lane) {
            lq_v2f v = lane == 0 ? (lq_v2f){x, lq_u2f(c)} : (lq_v2f){lq_u2f(c), x};
            lq_v2f chk = {0.0f, 0.0f};
            opaque(v); opaque(chk);
            lq_v2f y = lq_nonfinite_acc2(v, chk);
            opaque(y);
            const float yp = lane == 0 ? y.x : y.y, yc = lane == 0 ? y.y : y.x;
            bad |= finite_bits(p) ? (lq_f2u(yp) & 0x7fffffffu) != 0u : !is_nan(yp);
            bad |= (lq_f2u(yc) & 0x7fffffffu) != 0u;
        }
        return bad ? ST_BAD : ST_OK;
    }
    if constexpr (PAIR == P_SQRT) {
        if (!(x >= 0.0f) && !is_nan(x)) return ST_SKIP;
        double d = (double)x;
        opaque(d);
        return same_bits(lq_sqrt(x), (float)sqrt(d)) ? ST_OK : ST_BAD;
    }
    if constexpr (PAIR == P_DIV) {
        // both operands hashed from the counter: every class occurs at its share of the bit patterns (1/256 denormal, 1/256 inf or NaN)
        const uint32_t pa = fmix32(p ^ 0x2545F491u), pb = fmix32(p + kGold);
        const float a = lq_u2f(pa), b = lq_u2f(pb);
        double da = (double)a, db = (double)b;
        opaque(da); opaque(db);
        const float got = a / b;
        aux[0] += ((pa & 0x7f800000u) == 0u && (pa & 0x007fffffu) != 0u) || ((pb & 0x7f800000u) == 0u && (pb & 0x007fffffu) != 0u);
        aux[1] += !finite_bits(pa) || !finite_bits(pb);
        aux[2] += (lq_f2u(got) & 0x7f800000u) == 0u && (lq_f2u(got) & 0x007fffffu) != 0u;      // a denormal quotient
        aux[3] += is_nan(got);
        return same_bits(got, (float)(da / db)) ? ST_OK : ST_BAD;
    }
    if constexpr (PAIR == P_RCP_1PE) {
        if (p < 0x00800000u || p >= 0x7E800000u) return ST_SKIP;
        const float d = 1.0f + x;
        double dd = (double)d;
        opaque(dd);
        return same_bits(1.0f / d, (float)(1.0 / dd)) ? ST_OK : ST_BAD;
    }
    return ST_SKIP;
}

__global__ void init_kernel(u64* res, u64 where0) {
    const int t = threadIdx.x;
    if (t < LQ_PROBE_NRES) res[t] = (t == R_WHERE) ? where0 : 0ull;
}

template <int PAIR>
__global__ __launch_bounds__(kThreads) void same_kernel(u64 first, u64 count, u64* __restrict__ res) {
    const u64 stride = (u64)gridDim.x * kThreads;
    u64 bad = 0, where = ~0ull, skipped = 0, done = 0, aux[4] = {0, 0, 0, 0};
    for (u64 k = (u64)blockIdx.x * kThreads + threadIdx.x; k < count; k += stride) {
        const u64 i = first + k;
        const int st = check<PAIR>(i, aux);
        if (st == ST_SKIP) { ++skipped; continue; }
        ++done;
        if (st == ST_BAD) { ++bad; where = i < where ? i : where; }
    }
    if (bad) { atomicAdd(&res[R_BAD], bad); atomicMin(&res[R_WHERE], where); }
    if (skipped) atomicAdd(&res[R_SKIPPED], skipped);
    if (done) atomicAdd(&res[R_DONE], done);
#pragma unroll
    for (int a = 0; a < 4; ++a)
        if (aux[a]) atomicAdd(&res[R_AUX + a], aux[a]);
}

// ---- err -------------------------------------------------------------------------------------------------------------------------
enum { E_EXP_NORMAL = 0,   // lq_expf, ulp, where the true result is a normal fp32 number
       E_EXP_DENORMAL,     // lq_expf, absolute in units of 2^-149, where the true result is below FLT_MIN
       E_ERF,              // absolute, finite patterns
       E_GELU,             // absolute, finite patterns
       E_GELU_GRAD,        // absolute, finite patterns
       E_SIGMOID,          // ulp, where the reference exceeds 1e-30
       E_SOFTPLUS,         // ulp, where the reference exceeds 1e-30
       E_LOG_GE1,          // ulp, finite u >= 1
       E_GRAD_DEV,         // |lq_gelu_grad_dev - lq_gelu_grad| (no float64 here), where x * x < 18
       E_GRAD_DEV64,       // lq_gelu_grad_dev against float64, absolute, where x * x < 18 (elsewhere it is lq_gelu_grad: E_GELU_GRAD)
       E_COUNT };

constexpr double kFltMin = 1.17549435082228750797e-38, kFltMax = 3.40282346638528859812e+38;

// the distance from |(float)ref| to the next fp32 number away from zero (numpy's spacing), 2^-149 in the denormal range
__device__ __forceinline__ double ulp_of(double ref) {
    const uint32_t e = (lq_f2u((float)ref) >> 23) & 0xffu;
    return __longlong_as_double((long long)((e == 0 ? 1u : e) + 1023u - 150u) << 52);
}

// one pattern: the error (>= 0), or ST_SKIP; cls is set where the result's class differs from the reference's.
// sign_floor: the sign of a non-zero result is held against the reference's only where |reference| exceeds it (0 for the functions
// measured in ulp; the absolute limit for those measured absolutely, whose sign near a zero crossing the limit does not decide).
template <int FN>
__device__ __forceinline__ int err_one(uint32_t p, double sign_floor, double& err, bool& cls) {
    const float x = lq_u2f(p);
    const double xd = (double)x;
    float got = 0.0f;
    double ref = 0.0;
    bool measured = false, in_ulp = false, inf_allowed = false;
    if constexpr (FN == E_EXP_NORMAL || FN == E_EXP_DENORMAL) {
        got = lq_expf(x);
        ref = exp(xd);
        const bool normal = ref >= kFltMin && ref <= kFltMax;
        measured = FN == E_EXP_NORMAL ? normal : ref < kFltMin;
        in_ulp = true;                                 /* below FLT_MIN an ulp is 2^-149: the absolute error in that unit */
        inf_allowed = ref > kFltMax;                   /* the header: exp stays finite (x is clamped to 88.72283) */
    }
    if constexpr (FN == E_ERF) { got = lq_erff(x); ref = erf(xd); measured = finite_bits(p); in_ulp = false; }
    if constexpr (FN == E_GELU) {
        got = lq_gelu(x); ref = 0.5 * xd * (1.0 + erf(xd * 0.70710678118654752440)); measured = finite_bits(p); in_ulp = false;
    }
    if constexpr (FN == E_GELU_GRAD) {
        got = lq_gelu_grad(x);
        ref = 0.5 * (1.0 + erf(xd * 0.70710678118654752440)) + xd * exp(-0.5 * xd * xd) * 0.39894228040143267794;
        measured = finite_bits(p); in_ulp = false;
    }
    if constexpr (FN == E_SIGMOID) { got = lq_sigmoid(x); ref = 1.0 / (1.0 + exp(-xd)); measured = ref > 1e-30; in_ulp = true; }
    if constexpr (FN == E_SOFTPLUS) {
        got = lq_softplus(x); ref = x > 20.0f ? xd : log1p(exp(xd)); measured = ref > 1e-30; in_ulp = true;
    }
    if constexpr (FN == E_LOG_GE1) {
        if (!(x >= 1.0f) || !finite_bits(p)) return ST_SKIP;
        got = lq_logf_ge1(x); ref = log1p(xd - 1.0); measured = true; in_ulp = true;
    }
    if constexpr (FN == E_GRAD_DEV64) {
        if (!(x * x < 18.0f)) return ST_SKIP;
        got = lq_gelu_grad_dev(x);
        ref = 0.5 * (1.0 + erf(xd * 0.70710678118654752440)) + xd * exp(-0.5 * xd * xd) * 0.39894228040143267794;
        measured = true; in_ulp = false;
    }
    if constexpr (FN == E_GRAD_DEV) {
        if (!(x * x < 18.0f)) return ST_SKIP;
        float a = x, b = x;
        opaque(a); opaque(b);
        got = lq_gelu_grad_dev(a); ref = (double)lq_gelu_grad(b); measured = true; in_ulp = false;
    }
    const double gd = (double)got;
    const bool got_nan = is_nan(got), ref_nan = ref != ref;
    const bool got_inf = !got_nan && !finite_bits(lq_f2u(got)), ref_inf = !ref_nan && fabs(ref) > kFltMax;
    cls = got_nan != ref_nan;
    if (!got_nan && !ref_nan) {
        if (got_inf != ref_inf && !inf_allowed) cls = true;
        if (got != 0.0f && fabs(ref) > sign_floor && ((gd < 0.0) != (ref < 0.0))) cls = true;
    }
    if (!measured || got_nan || ref_nan || got_inf || ref_inf) return ST_SKIP;
    err = fabs(gd - ref);
    if (in_ulp) err = err / ulp_of(ref);
    return ST_OK;
}

template <int FN>
__global__ __launch_bounds__(kThreads) void err_kernel(u64 first, u64 count, double sign_floor, u64* __restrict__ res) {
    const u64 stride = (u64)gridDim.x * kThreads;
    u64 bad = 0, best = 0, skipped = 0, done = 0;
    for (u64 k = (u64)blockIdx.x * kThreads + threadIdx.x; k < count; k += stride) {
        const uint32_t p = (uint32_t)(first + k);
        double err = 0.0;
        bool cls = false;
        const int st = err_one<FN>(p, sign_floor, err, cls);
        bad += cls;
        if (st == ST_SKIP) { ++skipped; continue; }
        ++done;
        // a non-negative float's bits order as it does: the larger error wins, then the larger pattern
        const u64 packed = ((u64)lq_f2u(__double2float_ru(err)) << 32) | p;
        best = packed > best ? packed : best;
    }
    if (bad) atomicAdd(&res[R_BAD], bad);
    if (best) atomicMax(&res[R_WHERE], best);
    if (skipped) atomicAdd(&res[R_SKIPPED], skipped);
    if (done) atomicAdd(&res[R_DONE], done);
}

inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -2; }
inline int blocks_for(u64 n) { const u64 b = (n + kThreads - 1) / kThreads; return (int)(b < 1 ? 1 : (b > (u64)kBlocks ? (u64)kBlocks : b)); }

template <int... I>
struct Seq {};
template <int N, int... I>
struct MakeSeq : MakeSeq<N - 1, N - 1, I...> {};
template <int... I>
struct MakeSeq<0, I...> { typedef Seq<I...> type; };

template <int... FN>
int launch_map(Seq<FN...>, int fn, const uint32_t* in, uint32_t* out, int64_t n, hipStream_t s) {
    int hit = 0;
    ((fn == FN ? (map_kernel<FN><<<dim3(blocks_for((u64)n)), dim3(kThreads), 0, s>>>(in, out, n), hit = 1) : 0), ...);
    return hit;
}
template <int... FN>
int launch_ref(Seq<FN...>, int fn, const uint32_t* in, double* out, int64_t n, hipStream_t s) {
    int hit = 0;
    ((fn == FN ? (ref_kernel<FN><<<dim3(blocks_for((u64)n)), dim3(kThreads), 0, s>>>(in, out, n), hit = 1) : 0), ...);
    return hit;
}
template <int... PAIR>
int launch_same(Seq<PAIR...>, int pair, u64 first, u64 count, u64* res, hipStream_t s) {
    int hit = 0;
    ((pair == PAIR ? (same_kernel<PAIR><<<dim3(blocks_for(count)), dim3(kThreads), 0, s>>>(first, count, res), hit = 1) : 0), ...);
    return hit;
}
template <int... FN>
int launch_err(Seq<FN...>, int fn, u64 first, u64 count, double sign_floor, u64* res, hipStream_t s) {
    int hit = 0;
    ((fn == FN ? (err_kernel<FN><<<dim3(blocks_for(count)), dim3(kThreads), 0, s>>>(first, count, sign_floor, res), hit = 1) : 0), ...);
    return hit;
}

}  // namespace

// Every entry point returns 0, -1 for a bad argument, -2 if the launch failed.  `stream` is a hipStream_t (NULL: the default stream);
// nothing here synchronises.
extern "C" {

__attribute__((visibility("default"))) int lq_probe_nres(void) { return LQ_PROBE_NRES; }

// out[i] = bits of f(the float whose bits are in[i]), i < n; fn: F_* above (0..9 are lq_ref_math_probe's numbers)
__attribute__((visibility("default"))) int lq_probe_map(int fn, const uint32_t* in, uint32_t* out, int64_t n, void* stream) {
    if (n < 0 || fn < 0 || fn >= F_COUNT || (n > 0 && (!in || !out))) return -1;
    if (n == 0) return 0;
    if (!launch_map(MakeSeq<F_COUNT>::type(), fn, in, out, n, (hipStream_t)stream)) return -1;
    return launched();
}

// out[i] = ROCm's float64 exp / erf / log1p / sqrt (fn: D_* above) of the float whose bits are in[i], i < n
__attribute__((visibility("default"))) int lq_probe_ref(int fn, const uint32_t* in, double* out, int64_t n, void* stream) {
    if (n < 0 || fn < 0 || fn >= D_COUNT || (n > 0 && (!in || !out))) return -1;
    if (n == 0) return 0;
    if (!launch_ref(MakeSeq<D_COUNT>::type(), fn, in, out, n, (hipStream_t)stream)) return -1;
    return launched();
}

// the patterns (for P_DIV: the counters) first .. first + count - 1, first + count <= 2^32; res: LQ_PROBE_NRES words, written here
__attribute__((visibility("default"))) int lq_probe_same(int pair, uint64_t first, uint64_t count, uint64_t* res, void* stream) {
    if (pair < 0 || pair >= P_COUNT || !res || first > (1ull << 32) || count > (1ull << 32) - first) return -1;
    hipLaunchKernelGGL(init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (u64*)res, ~0ull);
    if (count && !launch_same(MakeSeq<P_COUNT>::type(), pair, (u64)first, (u64)count, (u64*)res, (hipStream_t)stream)) return -1;
    return launched();
}

__attribute__((visibility("default"))) int lq_probe_err(int fn, uint64_t first, uint64_t count, double sign_floor, uint64_t* res, void* stream) {
    if (fn < 0 || fn >= E_COUNT || !res || first > (1ull << 32) || count > (1ull << 32) - first || !(sign_floor >= 0.0)) return -1;
    hipLaunchKernelGGL(init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (u64*)res, 0ull);
    if (count && !launch_err(MakeSeq<E_COUNT>::type(), fn, (u64)first, (u64)count, sign_floor, (u64*)res, (hipStream_t)stream)) return -1;
    return launched();
}

}  // extern "C"
