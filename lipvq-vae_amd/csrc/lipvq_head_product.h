// lipvq_head_product.h -- the product stage of the policy's output heads (lipvq_gmm.hip, lipvq_action_head.hip): the head's
// Linears as ONE [rows, E] x [E, P] product on the fp32 MFMA with linear_kernel's k-ordered chain started from the bias
// (lipvq_embed.hip; the same bits as lipvq_linear_act_f32).  A workgroup of 256 threads owns HEAD_ROWS = 32 rows and ALL P
// columns (wave w takes column tiles w, w + 4, ...), because the epilogues need whole rows: the accumulators end in an LDS tile
// [32][PS].  Input row n = (b, t) = (n / T, n % T) is read at x + b bstride + t E: the last T positions of a [B, 3T, E] backbone
// output are addressed in place.
#ifndef LIPVQ_HEAD_PRODUCT_H_
#define LIPVQ_HEAD_PRODUCT_H_
#include "lipvq_common.h"
#include "lipvq_bf16_stage.h"

#define HEAD_ROWS 32

// floats of staging the product needs at the start of the workgroup's dynamic LDS (the tile [32][PS] takes the same place after it)
static inline int lq_head_stage_floats(int NT, int KC) { return (HEAD_ROWS + 128 * NT) * (KC + 1); }

// the same for lq_head_product_bf16: bf16 images [32 + 128 NT][40] (80-byte rows), a hi and a lo image in the split mode
static inline int lq_head_stage_floats_bf16(int NT, bool split) { return (split ? 2 : 1) * (HEAD_ROWS + 128 * NT) * 20; }

// the precision of a head's product: a bad mode is LIPVQ_EINVAL, a bf16 mode needs E % 8 == 0 (sizes: before any pointer)
static inline int lq_head_matmul_check(const char* what, int matmul, int E) {
    if (matmul < LIPVQ_MATMUL_FP32 || matmul > LIPVQ_MATMUL_BF16X3) return fail(LIPVQ_EINVAL, "%s: bad matmul precision %d", what, matmul);
    if (matmul != LIPVQ_MATMUL_FP32 && (E & 7) != 0)
        return fail(LIPVQ_EUNSUPPORTED, "%s: the bf16 modes need E=%d to be a multiple of 8", what, E);
    return LIPVQ_OK;
}

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
// The same stage on the bf16 matrix pipe: the arithmetic of lipvq_linear_act_bf16 (SPLIT: lipvq_linear_act_bf16x3), bit for bit
// (include/lipvq.h).  Operands are rounded to bf16, nearest even, as they are staged (gb_stage8; SPLIT: a hi and a lo image);
// accumulators start at 0; per accumulator tile ONE chain of v_mfma_f32_32x32x16_bf16 over k-steps of 16 in ascending order --
// SPLIT: a_lo b_hi, a_hi b_lo, a_hi b_hi per step -- with gemm_bf16_kernel's lane assignment:
//   A operand: lane (m = lane & 31, kh = lane >> 5) = x[row0 + m][k0 + 8 kh .. + 7]
//   B operand: lane (n = lane & 31, kh)             = W[column][k0 + 8 kh .. + 7]
// and the bias is added once, in fp32, after the chain.  Reduction elements past E (E % 8 == 0; the chain runs over whole
// steps of 32, as the gemm's does), rows past N and columns past P are zeros.  The reduction is never split across waves.
// Staging is the fp32 stage's scheme: DEPTH chunks of 32 features in flight in registers, one LDS buffer, two barriers a
// chunk; an LDS row is 80 bytes (64 of data + 16 of padding), so the 16-byte fragment reads of 16 consecutive rows fall on 16
// different 16-byte slots of the 256-byte bank row.  A thread stages chunks of 8 floats: chunk c = (row c >> 2, features
// 8 (c & 3) ..); x has 128 of them (threads 0..127), the weights 512 NT (2 NT per thread).
// lds: max(images, tile [32][PS]); images = lq_head_stage_floats_bf16(NT, SPLIT) floats.  On return: as lq_head_product.
template <int NT, bool SPLIT, int DEPTH, typename Cols>
__device__ __forceinline__ void lq_head_product_bf16(float* lds, const float* x, int64_t bstride, int64_t N, int T, int E, int P, int PS,
                                                     const Cols& cols) {
    constexpr int WROWS = 128 * NT, WV = 2 * NT, IM = SPLIT ? 2 : 1;
    unsigned short* xs = reinterpret_cast<unsigned short*>(lds);     // [IM][32][GB_LDK]
    unsigned short* ws = xs + IM * HEAD_ROWS * GB_LDK;               // [IM][WROWS][GB_LDK]
    float* pt = lds;                                                // [32][PS], after the product
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * HEAD_ROWS;

    f32x16 acc[NT];
    bool tile_ok[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        tile_ok[j] = (j * 4 + wave) * 32 < P;                      // wave-uniform
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    }
    // staging: thread -> (row sr (+ 64 i), 8 consecutive features at sk).  A line that does not exist is loaded from a valid
    // address and masked to zero (gb_keep): no load depends on a branch, nothing outside the tensors is read.
    const int sr = tid >> 2, sk = 8 * (tid & 3);
    const float* xp = x;
    uint32_t xm = 0u;
    if (sr < HEAD_ROWS && row0 + sr < N) {
        const int64_t n = row0 + sr, b = n / T;
        xp = x + b * bstride + (n - b * T) * (int64_t)E;
        xm = 0xffffffffu;
    }
    const float* wp[WV];
    uint32_t wm[WV];
#pragma unroll
    for (int i = 0; i < WV; ++i) {
        const float* p = cols.wrow(sr + 64 * i);
        wm[i] = p ? 0xffffffffu : 0u;
        wp[i] = p ? p : cols.wrow(0);                              // column 0 exists: P >= 1
    }
    lq_f32x4 xr[DEPTH][2], wr[DEPTH][WV][2];                       // DEPTH chunks in flight (indexed by unrolled constants: registers)
    auto fetch = [&](lq_f32x4 (&xv)[2], lq_f32x4 (&wv)[WV][2], int k0) {
        const bool kin = k0 + sk < E;                               // E is a multiple of 8: 8 floats are in or out together
        const int ko = kin ? k0 + sk : 0;
        const uint32_t km = kin ? 0xffffffffu : 0u;
        if (tid < 4 * HEAD_ROWS) {                                  // waves 0 and 1
            const lq_f32x4* p = reinterpret_cast<const lq_f32x4*>(xp + ko);
            xv[0] = gb_keep(p[0], xm & km);
            xv[1] = gb_keep(p[1], xm & km);
        }
#pragma unroll
        for (int i = 0; i < WV; ++i) {
            const lq_f32x4* p = reinterpret_cast<const lq_f32x4*>(wp[i] + ko);
            wv[i][0] = gb_keep(p[0], wm[i] & km);
            wv[i][1] = gb_keep(p[1], wm[i] & km);
        }
    };
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) fetch(xr[d], wr[d], d * GB_BK);
    const unsigned short* cA = xs + li * GB_LDK + kh * 8;
    const unsigned short* cB = ws + (wave * 32 + li) * GB_LDK + kh * 8;
    for (int kb = 0; kb < E; kb += DEPTH * GB_BK) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            const int k0 = kb + d * GB_BK;
            if (k0 < E) {                                           // uniform
                if (tid < 4 * HEAD_ROWS)
                    gb_stage8<SPLIT>(xs + sr * GB_LDK + sk, HEAD_ROWS * GB_LDK, xr[d][0].x, xr[d][0].y, xr[d][0].z, xr[d][0].w,
                                     xr[d][1].x, xr[d][1].y, xr[d][1].z, xr[d][1].w);
#pragma unroll
                for (int i = 0; i < WV; ++i)
                    gb_stage8<SPLIT>(ws + (sr + 64 * i) * GB_LDK + sk, WROWS * GB_LDK, wr[d][i][0].x, wr[d][i][0].y, wr[d][i][0].z,
                                     wr[d][i][0].w, wr[d][i][1].x, wr[d][i][1].y, wr[d][i][1].z, wr[d][i][1].w);
                __syncthreads();
                if (k0 + DEPTH * GB_BK < E) fetch(xr[d], wr[d], k0 + DEPTH * GB_BK);      // uniform; in flight during the next DEPTH chunks' MFMAs
#pragma unroll
                for (int s = 0; s < 2; ++s) {                       // both k-steps of 16, also where the second is all padding (the gemm's chain)
                    const lq_bf16x8 fa = __builtin_bit_cast(lq_bf16x8, *reinterpret_cast<const lq_u32x4*>(cA + s * 16));
                    lq_bf16x8 fb[NT];
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        fb[j] = __builtin_bit_cast(lq_bf16x8, *reinterpret_cast<const lq_u32x4*>(cB + j * 128 * GB_LDK + s * 16));
                    if constexpr (SPLIT) {
                        const lq_bf16x8 la = __builtin_bit_cast(lq_bf16x8, *reinterpret_cast<const lq_u32x4*>(cA + HEAD_ROWS * GB_LDK + s * 16));
                        lq_bf16x8 lb[NT];
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            lb[j] = __builtin_bit_cast(lq_bf16x8, *reinterpret_cast<const lq_u32x4*>(cB + (WROWS + j * 128) * GB_LDK + s * 16));
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            if (tile_ok[j]) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(la, fb[j], acc[j], 0, 0, 0);
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            if (tile_ok[j]) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, lb[j], acc[j], 0, 0, 0);
                    }
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        if (tile_ok[j]) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb[j], acc[j], 0, 0, 0);
                }
                __syncthreads();
            }
        }
    }
    // the row tile's P pre-activations, + bias in fp32, -> LDS (the images are dead: every wave has passed the loop's last barrier)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int c = (j * 4 + wave) * 32 + li;
        if (c < P) {
            const float b0 = cols.bias(c);
#pragma unroll
            for (int r = 0; r < 16; ++r) pt[((r & 3) + 8 * (r >> 2) + 4 * kh) * PS + c] = acc[j][r] + b0;
        }
    }
    __syncthreads();
}

// The stage by its precision (LIPVQ_MATMUL_*): the fp32 chain with its (KC, DEPTH), or the bf16 chain with DEPTHB.
template <int MP, int NT, int KC, int DEPTH, int DEPTHB, typename Cols>
__device__ __forceinline__ void lq_head_product_mp(float* lds, const float* x, int64_t bstride, int64_t N, int T, int E, int P, int PS,
                                                   const Cols& cols) {
    if constexpr (MP == LIPVQ_MATMUL_FP32) lq_head_product<NT, KC, DEPTH>(lds, x, bstride, N, T, E, P, PS, cols);
    else lq_head_product_bf16<NT, MP == LIPVQ_MATMUL_BF16X3, DEPTHB>(lds, x, bstride, N, T, E, P, PS, cols);
}
#endif

#endif
