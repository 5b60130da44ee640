// lipvq_nearest.hip -- nearest-code search (distance + first-minimum argmin + gather)
// ABI and reference citations: include/lipvq.h.  Arithmetic contract: lipvq_math.h.
#include "lipvq_common.h"

// ------------------------------------------------------------------------------------------
// nearest code: exact direct-difference distance, first-minimum argmin, gather
// ------------------------------------------------------------------------------------------
// One lane owns one latent row (its D floats live in registers); the workgroup streams the
// codebook through LDS in tiles and every lane reads the SAME code element (LDS broadcast).
// The distance is accumulated in the oracle's order (lq_sqdist8 / lq_sqdist32), so the result
// is bit-identical to torch's CPU kernels for D % 8 == 0.
template <int DCH, int DIST>
__global__ __launch_bounds__(256) void nearest_direct_kernel(
    const float* __restrict__ z, const float* __restrict__ cb, int64_t* __restrict__ idx,
    float* __restrict__ zq, unsigned long long* __restrict__ usage, float* __restrict__ best_out, int64_t N, int K,
    int KT) {
    constexpr int D = DCH * 8;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = slot < N;
    const int64_t row = valid ? slot : N - 1;

    float zr[D];
    {
        const float4* z4 = reinterpret_cast<const float4*>(z + (size_t)row * D);
#pragma unroll
        for (int i = 0; i < D / 4; ++i) {
            float4 v = z4[i];
            zr[4 * i + 0] = v.x; zr[4 * i + 1] = v.y; zr[4 * i + 2] = v.z; zr[4 * i + 3] = v.w;
        }
    }
    float best_v = INFINITY;   // compared value (sqrt for DIST_NORM)
    float best_s = INFINITY;   // its square (DIST_NORM) -- a cheap necessary test before the sqrt
    int best_k = 0;

    for (int k0 = 0; k0 < K; k0 += KT) {
        const int kt = (K - k0 < KT) ? (K - k0) : KT;
        __syncthreads();
        {
            const float4* src = reinterpret_cast<const float4*>(cb + (size_t)k0 * D);
            float4* dst = reinterpret_cast<float4*>(lds);
            const int n4 = kt * (D / 4);
            for (int i = threadIdx.x; i < n4; i += blockDim.x) dst[i] = src[i];
        }
        __syncthreads();
        for (int kk = 0; kk < kt; ++kk) {
            const float4* c4 = reinterpret_cast<const float4*>(lds + (size_t)kk * D);
            float s;
            if (DIST == LIPVQ_DIST_NORM) {
                s = lq_norm8_row<DCH>(zr, c4);
                if (s < best_s) {
                    const float v = lq_sqrt(s);
                    if (v < best_v) { best_v = v; best_s = s; best_k = k0 + kk; }
                }
            } else {
                s = lq_sq32_row<DCH>(zr, c4);
                if (s < best_v) { best_v = s; best_k = k0 + kk; }
            }
        }
    }
    // (per-row atomics on one address serialise chip-wide when the codes collapse -- the reference's default initialisation
    // does that: 6.5 ms for a 524 288-row VQVAE batch; lq_usage_add combines a wave's duplicates first)
    if (usage) lq_usage_add(usage, best_k, valid);
    if (!valid) return;
    idx[row] = (int64_t)best_k;
    if (best_out) best_out[row] = best_v;
    if (zq) {
        const float4* src = reinterpret_cast<const float4*>(cb + (size_t)best_k * D);
        float4* dst = reinterpret_cast<float4*>(zq + (size_t)row * D);
#pragma unroll
        for (int i = 0; i < D / 4; ++i) dst[i] = src[i];
    }
}

// Any D (including D % 8 != 0): one lane per row, operands straight from global memory.
__global__ void nearest_generic_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                       int64_t* __restrict__ idx, float* __restrict__ zq,
                                       unsigned long long* __restrict__ usage,
                                       float* __restrict__ best_out, int64_t N, int K, int D, int dist) {
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = slot < N;
    const int64_t row = valid ? slot : N - 1;
    const float* zr = z + (size_t)row * D;
    float best_v = INFINITY;
    int best_k = 0;
    for (int k = 0; k < K; ++k) {
        const float* c = cb + (size_t)k * D;
        float v = (dist == LIPVQ_DIST_NORM) ? lq_sqrt(lq_sqdist8(zr, c, D)) : lq_sqdist32(zr, c, D);
        if (v < best_v) { best_v = v; best_k = k; }
    }
    if (usage) lq_usage_add(usage, best_k, valid);
    if (!valid) return;
    idx[row] = (int64_t)best_k;
    if (best_out) best_out[row] = best_v;
    if (zq)
        for (int d = 0; d < D; ++d) zq[(size_t)row * D + d] = cb[(size_t)best_k * D + d];
}

template <int DCH>
static int launch_nearest_direct(const float* z, const float* cb, int64_t* idx, float* zq,
                                 int64_t* usage, float* best, int64_t N, int K, int dist,
                                 hipStream_t st) {
    constexpr int D = DCH * 8;
    int KT = 8192 / D;                     // 32 KiB of LDS per codebook tile
    if (KT > K) KT = K;
    size_t lds = (size_t)KT * D * sizeof(float);
    unsigned blocks = (unsigned)((N + 255) / 256);
    lq_dispatch<LIPVQ_DIST_NORM, LIPVQ_DIST_SQSUM>(dist, [&](auto rule) {
        hipLaunchKernelGGL((nearest_direct_kernel<DCH, rule()>), dim3(blocks), dim3(256), lds, st, z, cb, idx, zq,
                           (unsigned long long*)usage, best, N, K, KT);
    });
    return check_launch("nearest_direct");
}

// Widths 209 ... 512 (the range of the wide screening instances): the row no longer fits the registers nearest_direct_kernel keeps
// it in.  A workgroup takes NW_ROWS rows (2 per wave) and streams the codebook through LDS in groups of 64 codes, row stride D + 1
// floats (nearest_small_kernel's layout: the column reads of the scoring loop hit 32 different banks): lane = code, the row read as
// LDS broadcasts, torch's orders through lq_sqdist8 / lq_sqdist32.  A group's minimum (smallest value, the lower code among equal
// values) replaces the running one only when strictly smaller: the first minimum, as nearest_direct_kernel's scan.  A NaN or an
// infinite distance never wins (the scan's `v < best`).  DT: 256, 384, 512 at compile time (the loops unroll), 0 = any width.
#define NW_ROWS 8
#define NW_CODES 64
static inline size_t nearest_wide_lds_bytes(int D) { return ((size_t)NW_ROWS * D + (size_t)NW_CODES * (D + 1)) * sizeof(float); }

template <int DIST, int DT>
__global__ __launch_bounds__(256) void nearest_wide_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                           int64_t* __restrict__ idx, float* __restrict__ zq,
                                                           unsigned long long* __restrict__ usage, float* __restrict__ best_out,
                                                           int64_t N, int K, int D_rt) {
    extern __shared__ __attribute__((aligned(16))) float nw_lds[];
    constexpr int RPW = NW_ROWS / 4;
    const int D = DT ? DT : D_rt;
    const int LD = D + 1;
    float* s_z = nw_lds;                                  // [NW_ROWS][D]
    float* s_cb = nw_lds + NW_ROWS * D;                   // [NW_CODES][D + 1]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * NW_ROWS;
    for (int i = tid; i < NW_ROWS * D; i += 256) {
        const int r = i / D, d = i - r * D;
        int64_t row = r0 + r;
        row = row < N ? row : N - 1;
        s_z[i] = z[(size_t)row * D + d];
    }
    float best_v[RPW];
    int best_k[RPW];
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) { best_v[rr] = INFINITY; best_k[rr] = 0; }
    for (int k0 = 0; k0 < K; k0 += NW_CODES) {
        __syncthreads();                                  // the previous group's readers are done (first pass: s_z is written)
        for (int i = tid; i < NW_CODES * D; i += 256) {
            const int c = i / D, d = i - c * D;
            const int k = k0 + c;
            s_cb[c * LD + d] = k < K ? cb[(size_t)k * D + d] : 0.0f;
        }
        __syncthreads();
        const int k = k0 + lane;
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const float* zr = s_z + (w * RPW + rr) * D;
            float v = INFINITY;
            int kk = k < K ? k : K - 1;
            if (k < K) {
                const float* c = s_cb + lane * LD;
                const float t = (DIST == LIPVQ_DIST_NORM) ? lq_sqrt(lq_sqdist8(zr, c, D)) : lq_sqdist32(zr, c, D);
                if (t < INFINITY) v = t;
            }
            LQ_WAVE_MIN(v, kk, 1);
            if (v < best_v[rr]) { best_v[rr] = v; best_k[rr] = kk; }
        }
    }
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
        const int64_t row = r0 + w * RPW + rr;
        if (row >= N) continue;                           // (wave-uniform)
        const int bk = best_k[rr];
        if (lane == 0) {
            idx[row] = (int64_t)bk;
            if (best_out) best_out[row] = best_v[rr];
            if (usage) atomicAdd(&usage[bk], 1ull);
        }
        if (zq)
            for (int d = lane; d < D; d += 64) zq[(size_t)row * D + d] = cb[(size_t)bk * D + d];
    }
}

static int launch_nearest_wide(const float* z, const float* cb, int64_t* idx, float* zq, int64_t* usage, float* best,
                               int64_t N, int K, int D, int dist, hipStream_t st) {
    const size_t lds = nearest_wide_lds_bytes(D);
    const unsigned blocks = (unsigned)((N + NW_ROWS - 1) / NW_ROWS);
    int rc = LIPVQ_OK;
    auto go = [&](auto dt) {                              // (dt = the compile-time width, 0: any)
        lq_dispatch<LIPVQ_DIST_NORM, LIPVQ_DIST_SQSUM>(dist, [&](auto rule) {
            static LqLdsReserve reserved;                 // per kernel instance: one per instantiation of this lambda
            auto kfn = nearest_wide_kernel<rule(), dt()>;
            if (lds > 64 * 1024) {
                rc = lipvq_reserve_lds(reserved, (const void*)kfn, lds, "nearest_wide");
                if (rc) return;
            }
            hipLaunchKernelGGL(kfn, dim3(blocks), dim3(256), lds, st, z, cb, idx, zq, (unsigned long long*)usage, best, N, K, D);
        });
    };
    if (!lq_dispatch<256, 384, 512>(D, go)) go(std::integral_constant<int, 0>{});
    if (rc) return rc;
    return check_launch("nearest_wide");
}

extern "C" int lipvq_nearest_f32(const float* z, const float* codebook, int64_t* idx, float* zq,
                                 int64_t* usage, float* best, int64_t N, int K, int D, int dist,
                                 void* stream) {
    if (N < 0 || K <= 0 || D <= 0) return fail(LIPVQ_EINVAL, "nearest: bad sizes N=%lld K=%d D=%d", (long long)N, K, D);
    if (N == 0) return LIPVQ_OK;
    if (!z || !codebook || !idx) return fail(LIPVQ_EINVAL, "nearest: null pointer");
    if (dist != LIPVQ_DIST_NORM && dist != LIPVQ_DIST_SQSUM) return fail(LIPVQ_EINVAL, "nearest: unknown distance rule %d", dist);
    if (N > 2147483647LL * 64) return fail(LIPVQ_EUNSUPPORTED, "nearest: N too large");
    hipStream_t st = (hipStream_t)stream;
    const bool aligned = (((uintptr_t)z | (uintptr_t)codebook | (uintptr_t)zq) & 15) == 0;
    int rc = LIPVQ_OK;
    if (aligned && lq_dispatch<32, 64, 128, 208>(D, [&](auto d) { rc = launch_nearest_direct<d() / 8>(z, codebook, idx, zq, usage, best, N, K, dist, st); }))
        return rc;
    // 209 ... 512: LDS-staged (scalar staging: any alignment); the generic kernel is left to other widths
    if (D > 208 && D <= 512) {
        if ((N + NW_ROWS - 1) / NW_ROWS > 2147483647LL) return fail(LIPVQ_EUNSUPPORTED, "nearest: N too large");
        return launch_nearest_wide(z, codebook, idx, zq, usage, best, N, K, D, dist, st);
    }
    hipLaunchKernelGGL(nearest_generic_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, z, codebook,
                       idx, zq, (unsigned long long*)usage, best, N, K, D, dist);
    return check_launch("nearest_generic");
}

