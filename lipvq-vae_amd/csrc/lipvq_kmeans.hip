// lipvq_kmeans.hip -- opt-in extension (not reference behaviour): D^2 sampling for k-means++ seeding and dead-code revival,
// and the Lloyd means.  ABI and the sampling rule: include/lipvq.h.  Arithmetic contract: lipvq_math.h.
//
// Every row n carries d[n], its tokenizer comparison value to the nearest code written so far (lq_sqdist8 + lq_sqrt for
// LIPVQ_DIST_NORM, lq_sqdist32 for LIPVQ_DIST_SQSUM: what oracle.distances returns).  Its weight w = d^2 (norm) or d (sum)
// is exact in fp64 and becomes the integer q = floor(ldexp(w, e)), with e fixed once so that N ldexp(w_max, e) <= 2^62: the
// sums of q are exact and associative, so the block partials below meet any sequential cumsum bit for bit.
//
// One centre = two launches, both with fixed arguments (the whole loop is graph-capturable; nothing is read back):
//   km_pick_kernel  one workgroup: Q = sum of the block partials, r = min(Q - 1, floor(u Q)), the block and then the row whose
//                   running sum first exceeds r; the row is copied into the code, bit for bit.  Q == 0 stops the loop.
//   km_pass_kernel  one lane per row: d = min(d, dist(z_n, new code)), q, one uint64 partial per 256-row block.
// Each pass reads [N, D] once.
#include <float.h>
#include <math.h>

#include <type_traits>

#include "lipvq_common.h"

#define KM_BLOCK 256              // rows per pass block = threads of a pass workgroup
#define KM_PICK 1024              // threads of the single pick workgroup

struct KmState {                  // workspace header (device); written by the one-workgroup kernels only
    int e;                        // scale exponent
    int stopped;                  // 1: a draw met Q == 0; nothing more is written
    int fresh;                    // 1: the last pick wrote a code that the next pass has to fold in
    int ndead;                    // revival: number of entries of the dead-code list
    long long last;               // row copied by the last pick
};

enum { KM_INIT_CODE = 0, KM_INIT_ROW = 1, KM_UPDATE = 2, KM_QSUM = 3 };

static inline size_t km_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline int64_t km_blocks(int64_t N) { return (N + KM_BLOCK - 1) / KM_BLOCK; }
// layout: [KmState | dead codes int32 [K] | d float [N] | partials uint64 [nb]]
static inline size_t km_off_dead() { return 256; }
static inline size_t km_off_d(int K) { return km_off_dead() + km_align((size_t)K * 4); }
static inline size_t km_off_part(int64_t N, int K) { return km_off_d(K) + km_align((size_t)N * 4); }

// the integer weight of a comparison value (non-finite values weigh 0)
__device__ __forceinline__ unsigned long long km_q(float v, int dist, int e) {
    if (!(v <= FLT_MAX)) return 0ull;
    const double w = dist == LIPVQ_DIST_NORM ? (double)v * (double)v : (double)v;
    return (unsigned long long)floor(ldexp(w, e));
}

// the tokenizer's comparison value of z against c.  DT > 0: the row is read into registers as float4s (16-byte aligned z,
// D = DT); DT = 0: any width, operands straight from memory
template <int DT, int DIST>
__device__ __forceinline__ float km_dist(const float* __restrict__ z, const float* c, int D) {
    if constexpr (DT > 0) {
        float zr[DT];
        const float4* z4 = reinterpret_cast<const float4*>(z);
#pragma unroll
        for (int i = 0; i < DT / 4; ++i) {
            const float4 v = z4[i];
            zr[4 * i + 0] = v.x; zr[4 * i + 1] = v.y; zr[4 * i + 2] = v.z; zr[4 * i + 3] = v.w;
        }
        return DIST == LIPVQ_DIST_NORM ? lq_sqrt(lq_sqdist8(zr, c, DT)) : lq_sqdist32(zr, c, DT);
    } else {
        return DIST == LIPVQ_DIST_NORM ? lq_sqrt(lq_sqdist8(z, c, D)) : lq_sqdist32(z, c, D);
    }
}

// 256-lane reduction (sum or max) of a uint64; every thread of the block must call it
template <bool MAX>
__device__ __forceinline__ unsigned long long km_block_reduce(unsigned long long v) {
    __shared__ unsigned long long s_red[KM_BLOCK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = MAX ? (o > v ? o : v) : v + o;
    }
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = s_red[0];
#pragma unroll
    for (int w = 1; w < KM_BLOCK / 64; ++w) v = MAX ? (s_red[w] > v ? s_red[w] : v) : v + s_red[w];
    return v;
}

// One lane per row.  KM_INIT_CODE: d = dist(z_n, codebook[idx[n]]) (an index outside [0, K) gives weight 0);
// KM_INIT_ROW: d = dist(z_n, z[last]); both leave the block's largest fp64 weight (its bits: w >= 0) in part[b].
// KM_UPDATE: d = min(d, dist(z_n, z[last])) after a pick that wrote a code; KM_QSUM: d as it is; both leave sum q in part[b].
template <int DT, int DIST, int MODE>
__global__ __launch_bounds__(KM_BLOCK) void km_pass_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                           const int64_t* __restrict__ cidx, KmState* st, float* __restrict__ d,
                                                           unsigned long long* __restrict__ part, int64_t N, int K, int D) {
    if (MODE == KM_UPDATE && (st->stopped || !st->fresh)) return;         // (uniform)
    __shared__ __attribute__((aligned(16))) float s_c[DT > 0 ? DT : 1];
    const int64_t n = (int64_t)blockIdx.x * KM_BLOCK + threadIdx.x;
    const bool valid = n < N;
    const int64_t row = valid ? n : N - 1;
    const float* zr = z + (size_t)row * D;
    float v;
    if (MODE == KM_QSUM) {
        v = d[row];
    } else if (MODE == KM_INIT_CODE) {
        const int64_t k = cidx[row];
        v = (k >= 0 && k < K) ? km_dist<DT, DIST>(zr, cb + (size_t)k * D, D) : 0.0f;
    } else {
        const float* c = z + (size_t)st->last * D;
        if constexpr (DT > 0) {                                           // the new code, staged once per block
            for (int i = threadIdx.x; i < DT; i += KM_BLOCK) s_c[i] = c[i];
            __syncthreads();
            c = s_c;
        }
        v = km_dist<DT, DIST>(zr, c, D);
        if (MODE == KM_UPDATE) {
            const float old = d[row];
            v = v < old ? v : old;
        }
    }
    if (valid && MODE != KM_QSUM) d[row] = v;
    if (MODE == KM_INIT_CODE || MODE == KM_INIT_ROW) {
        const double w = !(v <= FLT_MAX) ? 0.0 : (DIST == LIPVQ_DIST_NORM ? (double)v * (double)v : (double)v);
        const unsigned long long m = km_block_reduce<true>(valid ? (unsigned long long)__double_as_longlong(w) : 0ull);
        if (threadIdx.x == 0) part[blockIdx.x] = m;
    } else {
        const unsigned long long s = km_block_reduce<false>(valid ? km_q(v, DIST, st->e) : 0ull);
        if (threadIdx.x == 0) part[blockIdx.x] = s;
    }
}

// e = the largest integer with N ldexp(w_max, e) <= 2^62 (fp64 arithmetic), from the block maxima of KM_INIT_*; 0 if w_max = 0
__global__ __launch_bounds__(KM_PICK) void km_scale_kernel(KmState* st, const unsigned long long* __restrict__ part, int64_t nb,
                                                           int64_t N) {
    __shared__ unsigned long long s_m[KM_PICK];
    unsigned long long m = 0ull;
    for (int64_t b = threadIdx.x; b < nb; b += KM_PICK) m = part[b] > m ? part[b] : m;
    s_m[threadIdx.x] = m;
    __syncthreads();
    for (int s = KM_PICK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && s_m[threadIdx.x + s] > s_m[threadIdx.x]) s_m[threadIdx.x] = s_m[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double wmax = __longlong_as_double((long long)s_m[0]);
    int e = 0;
    if (wmax > 0.0) {
        const double lim = 4611686018427387904.0;                          // 2^62
        const double dn = (double)N;
        int x;
        frexp(wmax, &x);                                                   // wmax < 2^x
        int lg = 0;
        while (lg < 63 && (1ll << lg) < N) ++lg;                           // N <= 2^lg
        e = 62 - x - lg;                                                   // holds: N wmax 2^e < 2^62
        while (dn * ldexp(wmax, e + 1) <= lim) ++e;
    }
    st->e = e;
}

// The seed's first centre, or the revival's dead-code list; both clear picks.
__global__ __launch_bounds__(KM_PICK) void km_start_kernel(const float* __restrict__ z, float* __restrict__ cb,
                                                           const double* __restrict__ draws, const int64_t* __restrict__ counts,
                                                           int64_t threshold, KmState* st, int* __restrict__ dead,
                                                           int64_t* __restrict__ picks, int64_t* __restrict__ written, int64_t N,
                                                           int K, int D, int revive) {
    __shared__ long long s_pre[KM_PICK];
    const int tid = threadIdx.x;
    for (int k = tid; k < K; k += KM_PICK) picks[k] = -1;
    if (!revive) {
        double f = floor(draws[0] * (double)N);
        long long r = (f >= 0.0 && f < (double)N) ? (long long)f : (f < 0.0 ? 0 : N - 1);
        for (int i = tid; i < D; i += KM_PICK) cb[i] = z[(size_t)r * D + i];
        if (tid == 0) {
            picks[0] = r;
            *written = 1;
            st->e = 0; st->stopped = 0; st->fresh = 1; st->ndead = 0; st->last = r;
        }
        return;
    }
    // dead codes in ascending order: per-thread chunk counts, an exclusive scan, then the writes
    const int chunk = (K + KM_PICK - 1) / KM_PICK;
    const int lo = tid * chunk < K ? tid * chunk : K, hi = lo + chunk < K ? lo + chunk : K;
    long long c = 0;
    for (int k = lo; k < hi; ++k) c += counts[k] < threshold;
    s_pre[tid] = c;
    __syncthreads();
    for (int s = 1; s < KM_PICK; s <<= 1) {
        const long long t = tid >= s ? s_pre[tid - s] : 0;
        __syncthreads();
        s_pre[tid] += t;
        __syncthreads();
    }
    int o = (int)(s_pre[tid] - c);
    for (int k = lo; k < hi; ++k)
        if (counts[k] < threshold) dead[o++] = k;
    if (tid == 0) {
        *written = 0;
        st->e = 0; st->stopped = 0; st->fresh = 0; st->ndead = (int)s_pre[KM_PICK - 1]; st->last = 0;
    }
}

// One draw.  Seeding: code `step` with draws[step].  Revival: the step-th dead code k with draws[k].
template <int DIST>
__global__ __launch_bounds__(KM_PICK) void km_pick_kernel(const float* __restrict__ z, float* __restrict__ cb,
                                                          const double* __restrict__ draws, KmState* st,
                                                          const int* __restrict__ dead, const float* __restrict__ d,
                                                          const unsigned long long* __restrict__ part, int64_t* __restrict__ picks,
                                                          int64_t* __restrict__ written, int64_t N, int64_t nb, int D, int step,
                                                          int revive) {
    __shared__ unsigned long long s_pre[KM_PICK];
    __shared__ long long s_blk, s_row;
    __shared__ unsigned long long s_rb;
    __shared__ int s_go, s_code, s_e;
    const int tid = threadIdx.x;
    if (tid == 0) {
        int go = !st->stopped;
        int code = step;
        if (go && revive) {
            go = step < st->ndead;
            code = go ? dead[step] : 0;
        }
        if (!go) st->fresh = 0;
        s_go = go; s_code = code; s_e = st->e;
        s_blk = -1; s_row = -1;
    }
    __syncthreads();
    if (!s_go) return;
    const int code = s_code, e = s_e;
    // Q and the block: each thread sums a contiguous chunk of the partials, an inclusive scan over the threads
    const int64_t chunk = (nb + KM_PICK - 1) / KM_PICK;
    const int64_t lo = (int64_t)tid * chunk < nb ? (int64_t)tid * chunk : nb;
    const int64_t hi = lo + chunk < nb ? lo + chunk : nb;
    unsigned long long s = 0ull;
    for (int64_t b = lo; b < hi; ++b) s += part[b];
    s_pre[tid] = s;
    __syncthreads();
    for (int o = 1; o < KM_PICK; o <<= 1) {
        const unsigned long long t = tid >= o ? s_pre[tid - o] : 0ull;
        __syncthreads();
        s_pre[tid] += t;
        __syncthreads();
    }
    const unsigned long long Q = s_pre[KM_PICK - 1];
    if (Q == 0ull) {                                                       // no row left that differs from every code
        if (tid == 0) { st->stopped = 1; st->fresh = 0; }
        return;
    }
    const double f = floor(draws[code] * (double)Q);
    unsigned long long r = f >= 0.0 ? (unsigned long long)f : 0ull;
    if (!(f < (double)Q) || r > Q - 1ull) r = Q - 1ull;
    const unsigned long long excl = s_pre[tid] - s;
    if (s > 0ull && excl <= r && r < s_pre[tid]) {                         // exactly one thread
        unsigned long long acc = excl;
        for (int64_t b = lo; b < hi; ++b) {
            if (r < acc + part[b]) { s_blk = b; s_rb = r - acc; break; }
            acc += part[b];
        }
    }
    __syncthreads();
    const int64_t blk = s_blk;
    const unsigned long long rb = s_rb;
    // the row inside the block: an inclusive scan of its (at most 256) weights
    const int64_t row = blk * KM_BLOCK + tid;
    const unsigned long long q = (tid < KM_BLOCK && row < N) ? km_q(d[row], DIST, e) : 0ull;
    __syncthreads();
    s_pre[tid] = q;
    __syncthreads();
    for (int o = 1; o < KM_BLOCK; o <<= 1) {
        const unsigned long long t = (tid < KM_BLOCK && tid >= o) ? s_pre[tid - o] : 0ull;
        __syncthreads();
        if (tid < KM_BLOCK) s_pre[tid] += t;
        __syncthreads();
    }
    if (tid < KM_BLOCK && q > 0ull && s_pre[tid] - q <= rb && rb < s_pre[tid]) s_row = row;
    __syncthreads();
    const int64_t n = s_row;
    if (n < 0) {                                                           // unreachable: the partials and the rows agree
        if (tid == 0) { st->stopped = 1; st->fresh = 0; }
        return;
    }
    for (int i = tid; i < D; i += KM_PICK) cb[(size_t)code * D + i] = z[(size_t)n * D + i];
    if (tid == 0) {
        picks[code] = n;
        *written += 1;
        st->last = n;
        st->fresh = 1;
    }
}

// codebook[k] = sums[k] / (float)counts[k] where counts[k] > 0 (IEEE division)
__global__ __launch_bounds__(256) void km_means_kernel(float* __restrict__ cb, const float* __restrict__ sums,
                                                       const int64_t* __restrict__ counts, int64_t total, int D) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t c = counts[i / D];
    if (c > 0) cb[i] = sums[i] / (float)c;
}

// ---- launch plumbing ----------------------------------------------------------------------------------------------------------

template <int DT, int DIST>
static void km_pass(int mode, const float* z, const float* cb, const int64_t* cidx, KmState* st, float* d, unsigned long long* part,
                    int64_t N, int K, int D, hipStream_t s) {
    const dim3 g((unsigned)km_blocks(N)), b(KM_BLOCK);
    switch (mode) {
        case KM_INIT_CODE: hipLaunchKernelGGL((km_pass_kernel<DT, DIST, KM_INIT_CODE>), g, b, 0, s, z, cb, cidx, st, d, part, N, K, D); break;
        case KM_INIT_ROW: hipLaunchKernelGGL((km_pass_kernel<DT, DIST, KM_INIT_ROW>), g, b, 0, s, z, cb, cidx, st, d, part, N, K, D); break;
        case KM_UPDATE: hipLaunchKernelGGL((km_pass_kernel<DT, DIST, KM_UPDATE>), g, b, 0, s, z, cb, cidx, st, d, part, N, K, D); break;
        default: hipLaunchKernelGGL((km_pass_kernel<0, DIST, KM_QSUM>), g, b, 0, s, z, cb, cidx, st, d, part, N, K, D); break;
    }
}

template <int DIST>
static void km_pass_any(int mode, const float* z, const float* cb, const int64_t* cidx, KmState* st, float* d,
                        unsigned long long* part, int64_t N, int K, int D, hipStream_t s) {
    const bool aligned = ((uintptr_t)z & 15) == 0;
    if (aligned && mode != KM_QSUM &&
        lq_dispatch<32, 64, 128, 208>(D, [&](auto dt) { km_pass<dt(), DIST>(mode, z, cb, cidx, st, d, part, N, K, D, s); }))
        return;
    km_pass<0, DIST>(mode, z, cb, cidx, st, d, part, N, K, D, s);
}

static int km_check(const char* what, const float* z, const float* cb, const double* draws, const int64_t* picks,
                    const int64_t* written, const void* ws, int64_t N, int K, int D, int dist) {
    if (N < 1 || K < 1 || D < 1) return fail(LIPVQ_EINVAL, "%s: bad sizes N=%lld K=%d D=%d", what, (long long)N, K, D);
    if (!z || !cb || !draws || !picks || !written || !ws) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if (dist != LIPVQ_DIST_NORM && dist != LIPVQ_DIST_SQSUM) return fail(LIPVQ_EINVAL, "%s: unknown distance rule %d", what, dist);
    if (km_blocks(N) > 2147483647LL) return fail(LIPVQ_EUNSUPPORTED, "%s: N too large", what);
    if (((uintptr_t)ws & 7) != 0) return fail(LIPVQ_EINVAL, "%s: workspace must be 8-byte aligned", what);
    return LIPVQ_OK;
}

extern "C" size_t lipvq_kmeans_workspace_bytes(int64_t N, int K) {
    if (N < 1 || K < 1) return 0;
    return km_off_part(N, K) + (size_t)km_blocks(N) * 8;
}

template <int DIST>
static void km_draw_loop(const float* z, float* cb, const double* draws, KmState* st, int* dead, float* d, unsigned long long* part,
                         int64_t* picks, int64_t* written, int64_t N, int K, int D, int first, int revive, hipStream_t s) {
    const int64_t nb = km_blocks(N);
    for (int step = first; step < K; ++step) {
        hipLaunchKernelGGL(km_pick_kernel<DIST>, dim3(1), dim3(KM_PICK), 0, s, z, cb, draws, st, dead, d, part, picks, written, N, nb,
                           D, step, revive);
        if (step + 1 < K) km_pass_any<DIST>(KM_UPDATE, z, cb, nullptr, st, d, part, N, K, D, s);
    }
}

extern "C" int lipvq_kmeans_seed_f32(const float* z, float* codebook, const double* draws, int64_t* picks, int64_t* written,
                                     void* workspace, int64_t N, int K, int D, int dist, void* stream) {
    const int rc = km_check("kmeans_seed", z, codebook, draws, picks, written, workspace, N, K, D, dist);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    KmState* st = (KmState*)ws;
    int* dead = (int*)(ws + km_off_dead());
    float* d = (float*)(ws + km_off_d(K));
    unsigned long long* part = (unsigned long long*)(ws + km_off_part(N, K));
    const int64_t nb = km_blocks(N);
    hipLaunchKernelGGL(km_start_kernel, dim3(1), dim3(KM_PICK), 0, s, z, codebook, draws, nullptr, (int64_t)0, st, dead, picks,
                       written, N, K, D, 0);
    if (K > 1) {
        auto run = [&](auto tag) {
            constexpr int DIST = decltype(tag)::value;
            km_pass_any<DIST>(KM_INIT_ROW, z, codebook, nullptr, st, d, part, N, K, D, s);
            hipLaunchKernelGGL(km_scale_kernel, dim3(1), dim3(KM_PICK), 0, s, st, part, nb, N);
            km_pass_any<DIST>(KM_QSUM, z, codebook, nullptr, st, d, part, N, K, D, s);
            km_draw_loop<DIST>(z, codebook, draws, st, dead, d, part, picks, written, N, K, D, 1, 0, s);
        };
        if (dist == LIPVQ_DIST_NORM) run(std::integral_constant<int, LIPVQ_DIST_NORM>());
        else run(std::integral_constant<int, LIPVQ_DIST_SQSUM>());
    }
    return check_launch("kmeans_seed");
}

extern "C" int lipvq_kmeans_revive_f32(const float* z, float* codebook, const int64_t* idx, const int64_t* counts, int64_t threshold,
                                       const double* draws, int64_t* picks, int64_t* written, void* workspace, int64_t N, int K,
                                       int D, int dist, int max_codes, void* stream) {
    const int rc = km_check("kmeans_revive", z, codebook, draws, picks, written, workspace, N, K, D, dist);
    if (rc) return rc;
    if (!idx || !counts) return fail(LIPVQ_EINVAL, "kmeans_revive: null pointer");
    if (max_codes < 0) return fail(LIPVQ_EINVAL, "kmeans_revive: max_codes must be >= 0");
    const int steps = max_codes < K ? max_codes : K;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    KmState* st = (KmState*)ws;
    int* dead = (int*)(ws + km_off_dead());
    float* d = (float*)(ws + km_off_d(K));
    unsigned long long* part = (unsigned long long*)(ws + km_off_part(N, K));
    const int64_t nb = km_blocks(N);
    hipLaunchKernelGGL(km_start_kernel, dim3(1), dim3(KM_PICK), 0, s, z, codebook, draws, counts, threshold, st, dead, picks, written,
                       N, K, D, 1);
    if (steps > 0) {
        auto run = [&](auto tag) {
            constexpr int DIST = decltype(tag)::value;
            km_pass_any<DIST>(KM_INIT_CODE, z, codebook, idx, st, d, part, N, K, D, s);
            hipLaunchKernelGGL(km_scale_kernel, dim3(1), dim3(KM_PICK), 0, s, st, part, nb, N);
            km_pass_any<DIST>(KM_QSUM, z, codebook, nullptr, st, d, part, N, K, D, s);
            km_draw_loop<DIST>(z, codebook, draws, st, dead, d, part, picks, written, N, steps, D, 0, 1, s);
        };
        if (dist == LIPVQ_DIST_NORM) run(std::integral_constant<int, LIPVQ_DIST_NORM>());
        else run(std::integral_constant<int, LIPVQ_DIST_SQSUM>());
    }
    return check_launch("kmeans_revive");
}

extern "C" int lipvq_kmeans_means_f32(float* codebook, const float* sums, const int64_t* counts, int K, int D, void* stream) {
    if (K < 1 || D < 1) return fail(LIPVQ_EINVAL, "kmeans_means: bad sizes K=%d D=%d", K, D);
    if (!codebook || !sums || !counts) return fail(LIPVQ_EINVAL, "kmeans_means: null pointer");
    const int64_t total = (int64_t)K * D;
    hipLaunchKernelGGL(km_means_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codebook, sums,
                       counts, total, D);
    return check_launch("kmeans_means");
}
