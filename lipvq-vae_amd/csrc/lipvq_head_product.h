// lipvq_head_product.h -- the product stage of the policy's output heads (lipvq_gmm.hip, lipvq_action_head.hip): the head's
// Linears as ONE [rows, E] x [E, P] product on the fp32 MFMA with linear_kernel's k-ordered chain started from the bias
// (lipvq_embed.hip; the same bits as lipvq_linear_act_f32).  A workgroup of 256 threads owns HEAD_ROWS = 32 rows and ALL P
// columns (wave w takes column tiles w, w + 4, ...), because the epilogues need whole rows: the accumulators end in an LDS tile
// [32][PS].  Input row n = (b, t) = (n / T, n % T) is read at x + b bstride + t E: the last T positions of a [B, 3T, E] backbone
// output are addressed in place.
#ifndef LIPVQ_HEAD_PRODUCT_H_
#define LIPVQ_HEAD_PRODUCT_H_
#include "lipvq_common.h"

#define HEAD_ROWS 32

// floats of staging the product needs at the start of the workgroup's dynamic LDS (the tile [32][PS] takes the same place after it)
static inline int lq_head_stage_floats(int NT, int KC) { return (HEAD_ROWS + 128 * NT) * (KC + 1); }

#if defined(__HIPCC__)
// NT = column tiles per wave (P <= 128 NT), KC = input features staged per step, DEPTH = chunks of KC features whose loads are
// in flight ahead of the MFMAs (1: the next chunk alone; the chunks are multiplied in k order whatever the depth).
//   A operand: lane (m = lane & 31, kh = lane >> 5) = x[row0 + m][k0 + 2s + kh]
//   B operand: lane (n = lane & 31, kh)             = W[column][k0 + 2s + kh]
//   D[m][n]  : col n = lane & 31, row m = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
// Cols names the columns: cols.bias(c) is column c's bias (0 for c >= P), cols.wrow(c) its weight row [E] (nullptr for c >= P),
// so that several Linears are one product without their parameters ever being concatenated.
// lds: max(staging [32 + 128 NT][KC + 1], tile [32][PS]) floats.  On return (after a barrier) lds holds the tile: the row tile's
// P pre-activations, row r at lds + r PS; rows past N hold the bias chain of a zero input.
template <int NT, int KC, int DEPTH, typename Cols>
__device__ __forceinline__ void lq_head_product(float* lds, const float* x, int64_t bstride, int64_t N, int T, int E, int P, int PS,
                                                const Cols& cols) {
    constexpr int WROWS = 128 * NT, KS = KC + 1, KC4 = KC / 4;
    constexpr int WV = WROWS * KC4 / 256, WSTEP = 256 / KC4;      // float4 per thread and step; weight rows between two of them
    float* xs = lds;                                                // [32][KS]
    float* ws = lds + HEAD_ROWS * KS;                               // [WROWS][KS]
    float* pt = lds;                                                // [32][PS], after the product
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * HEAD_ROWS;

    f32x16 acc[NT];
    bool tile_ok[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int c = (j * 4 + wave) * 32 + li;
        tile_ok[j] = (j * 4 + wave) * 32 < P;                      // wave-uniform
        const float b0 = cols.bias(c);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = b0;
    }
    // staging: thread -> (row sr (+ WSTEP i), 4 consecutive features at sk)
    const int sr = tid / KC4, sk = 4 * (tid % KC4);
    const float* xp = nullptr;
    if (sr < HEAD_ROWS && row0 + sr < N) {
        const int64_t n = row0 + sr, b = n / T;
        xp = x + b * bstride + (n - b * T) * (int64_t)E;
    }
    const float* wp[WV];
#pragma unroll
    for (int i = 0; i < WV; ++i) wp[i] = cols.wrow(sr + WSTEP * i);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 xr[DEPTH], wr[DEPTH][WV];                               // DEPTH chunks in flight (indexed by unrolled constants: registers)
    auto fetch = [&](float4& xv, float4 (&wv)[WV], int k0) {
        const bool kin = k0 + sk < E;                               // E is a multiple of 4
        xv = (xp && kin) ? *reinterpret_cast<const float4*>(xp + k0 + sk) : zero4;
#pragma unroll
        for (int i = 0; i < WV; ++i) wv[i] = (wp[i] && kin) ? *reinterpret_cast<const float4*>(wp[i] + k0 + sk) : zero4;
    };
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) fetch(xr[d], wr[d], d * KC);
    for (int kb = 0; kb < E; kb += DEPTH * KC) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            const int k0 = kb + d * KC;
            if (k0 < E) {                                           // uniform
                if (sr < HEAD_ROWS) {
                    float* xd = xs + sr * KS + sk;
                    xd[0] = xr[d].x; xd[1] = xr[d].y; xd[2] = xr[d].z; xd[3] = xr[d].w;
                }
#pragma unroll
                for (int i = 0; i < WV; ++i) {
                    float* wd = ws + (sr + WSTEP * i) * KS + sk;
                    wd[0] = wr[d][i].x; wd[1] = wr[d][i].y; wd[2] = wr[d][i].z; wd[3] = wr[d][i].w;
                }
                __syncthreads();
                if (k0 + DEPTH * KC < E) fetch(xr[d], wr[d], k0 + DEPTH * KC);      // uniform; in flight during the next DEPTH chunks' MFMAs
                const int kend = (E - k0 < KC) ? ((E - k0) >> 1) : (KC / 2);
                for (int s = 0; s < kend; ++s) {
                    const float av = xs[li * KS + 2 * s + kh];
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        if (tile_ok[j]) {
                            const float bv = ws[((j * 4 + wave) * 32 + li) * KS + 2 * s + kh];
                            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j], 0, 0, 0);
                        }
                }
                __syncthreads();
            }
        }
    }
    // the row tile's P pre-activations -> LDS (the staging buffers are dead: every wave has passed the loop's last barrier)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int c = (j * 4 + wave) * 32 + li;
        if (c < P) {
#pragma unroll
            for (int r = 0; r < 16; ++r) pt[((r & 3) + 8 * (r >> 2) + 4 * kh) * PS + c] = acc[j][r];
        }
    }
    __syncthreads();
}
#endif

#endif
