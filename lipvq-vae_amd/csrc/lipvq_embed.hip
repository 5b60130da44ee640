// lipvq_embed.hip -- the step right after the tokenizer: the reference's
// ICLTransformer.input_embedding() + the interleave of (context_obs, context_actions, obs)
// (reference robomimic/models/obs_nets.py:2525-2543 and :2580-2596):
//     e = LayerNorm(Linear(z_latent) + time_embedding[t])          dropout is the caller's (identity in eval), or decided here:
//                                                                  the DROP instances, lipvq_rng.h, field row = the output row
//     transformer_embeddings[b, 2t] = e(context_obs), [b, 2t+1] = e(context_actions), [b, 2T+t] = e(obs)
//
// MI355X design.  For the LipVQ tokenizer z_latent[n] IS codebook[idx[n]] (v5:47,84), so
//     Linear(z_latent)[n] = (codebook . W^T + b)[idx[n]]
// and the Linear over N rows collapses into a [K][E] table computed once per parameter update
// (linear_kernel, fp32 MFMA, k-ordered chain from the bias = the canonical Linear).  The per-action work
// is then a gather of one table row + the time embedding + LayerNorm, written straight into its interleaved
// slot of the [B][3T][E] transformer input: one launch (embed_rows_kernel), HBM-write bound
// (4 E bytes per action; the table and the time embeddings stay in L2), and z_latent itself never
// exists in HBM -- the tokenizer hands over 8-byte indices.  Rows that are not codebook rows (the
// observation streams, the VQVAE's straight-through value) take linear_kernel over their N rows and
// then the same embed_rows_kernel with idx = NULL.
//
// Canonical LayerNorm (shared with oracle/lipvq_oracle.c, bit for bit): a row is owned by 16 lanes, lane l holding the
// float4 groups q = l, l+16, ...;  lane sums run in that order and the 16 lane sums are combined by a butterfly with
// partners l^1, l^2, l^7, l^15 (four DPP adds).  The row is centred twice:  mean0 = s*(1/E), d = v-mean0,
// rest = sum(d)*(1/E) (same lane order and butterfly), d = d-rest;  var = sum(d^2)*(1/E) (fmaf chain, same order),
// rstd = 1/sqrt(var+eps), y = fmaf(d*rstd, w, b);  stats = (mean0+rest, rstd).  One centring is not enough: fl(1/E) is
// inexact unless E is a power of two, so the mean of a constant row comes out an ulp off and rstd = 1/sqrt(eps) = 316
// multiplies the residue (1e-4 of max|y| on rows of 3.0 at E = 252; tests/test_gpu_embed_edges.py).  stats keeps the
// corrected mean, from which the backward kernels rebuild xhat = (v - mean) * rstd in one step.
// In-kernel dropout (include/lipvq.h, "in-kernel dropout for the embedding stage and the default action branch"): linear_kernel
// and linear_big_kernel take DROP as a template parameter (y = act(pre) * m in the epilogue), embed_rows_kernel and its two
// backward kernels likewise (out * m, gout * m); the plain instances are the kernels they were.
// ABI: include/lipvq.h.
#include <stdlib.h>

#include "lipvq_common.h"
#include "lipvq_rng.h"

// ---------------------------------------------------------------------------------------------------
// y[N][E] = x[N][Kin] . W[E][Kin]^T + b      (nn.Linear; obs_nets.py:2536 `embed_encoder`)
// WG = 4 waves; tile = 32 rows x 128 columns, one 32x32 MFMA tile per wave; K staged 32 at a time.
//   A operand: lane (m = lane & 31, kh = lane >> 5) = x[row0 + m][k0 + 2s + kh]
//   B operand: lane (n = lane & 31, kh)             = W[e0 + n][k0 + 2s + kh]
//   D[m][n]  : col n = lane & 31, row m = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
// ---------------------------------------------------------------------------------------------------
#define LIN_ROWS 32
#define LIN_KC 64

// DROP epilogue (lipvq_linear_act_drop_f32): the decisions of one 32 x 32 result tile for the lane's column `ecol`, bit r = the
// row of accumulator register r (row_of(r) = tile row0 + (r & 3) + 8 (r >> 2) + 4 kh).  The four lanes of a quad share
// ecol >> 2 and kh, hence all sixteen draws (one per r); lane q = lane & 3 runs those of r = q, q + 4, q + 8, q + 12 and the quad
// exchanges the nibbles: four draws per lane and tile.  Every lane of the wave must call it.
__device__ __forceinline__ uint32_t lin_keep_tile(lq_dropout d, int64_t row0, int kh, int ecol, int lane) {
    const int q = lane & 3;
    uint32_t mine = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int r = q + 4 * t;
        mine |= lq_dropout_keep4(d, (uint32_t)(row0 + (r & 3) + 8 * (r >> 2) + 4 * kh), (uint32_t)(ecol >> 2)) << (4 * t);
    }
    uint32_t bits = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint32_t m = (uint32_t)__shfl((int)mine, (lane & ~3) | s, 64);          // lane s of the quad: r = s + 4 t at bits 4 t .. 4 t + 3
#pragma unroll
        for (int t = 0; t < 4; ++t) bits |= ((m >> (4 * t + q)) & 1u) << (s + 4 * t);
    }
    return bits;
}

template <bool DROP>
__global__ __launch_bounds__(256) void linear_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                     const float* __restrict__ bias, float* __restrict__ y,
                                                     float* __restrict__ pre, int act, lq_dropout_src src, int64_t N, int Kin, int E) {
    __shared__ float xs[LIN_ROWS][LIN_KC + 1];
    __shared__ float ws[128][LIN_KC + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * LIN_ROWS;
    const int e0 = blockIdx.y * 128;
    const int ecol = e0 + wave * 32 + li;
    const bool tile_ok = (e0 + wave * 32) < E;          // wave-uniform; a ragged last tile computes on zero rows of W
    f32x16 acc;
    const float b0 = (ecol < E && bias) ? bias[ecol] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = b0;
    // Chunks of LIN_KC = 64 input features, the NEXT chunk's global loads in flight (registers) while the current one is
    // multiplied.  The first version (32-feature chunks, loads issued after the barrier that ended the previous chunk) paid one
    // L2 round trip per chunk: 30 us per call at N = 80, Kin = 208 -- 80 % of the default action branch's forward.
    constexpr int XV = LIN_ROWS * LIN_KC / 256, WV = 128 * LIN_KC / 256;       // floats per thread and chunk
    float xr[XV], wr[WV];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            const int f = tid + 256 * i, r = f / LIN_KC, k = f % LIN_KC;
            const int64_t row = row0 + r;
            xr[i] = (row < N && k0 + k < Kin) ? x[(size_t)row * Kin + k0 + k] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < WV; ++i) {
            const int f = tid + 256 * i, r = f / LIN_KC, k = f % LIN_KC;
            const int e = e0 + r;
            wr[i] = (e < E && k0 + k < Kin) ? W[(size_t)e * Kin + k0 + k] : 0.0f;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < Kin; k0 += LIN_KC) {
#pragma unroll
        for (int i = 0; i < XV; ++i) { const int f = tid + 256 * i; xs[f / LIN_KC][f % LIN_KC] = xr[i]; }
#pragma unroll
        for (int i = 0; i < WV; ++i) { const int f = tid + 256 * i; ws[f / LIN_KC][f % LIN_KC] = wr[i]; }
        __syncthreads();
        if (k0 + LIN_KC < Kin) fetch(k0 + LIN_KC);          // uniform
        if (tile_ok) {
            const int kend = (Kin - k0 < LIN_KC) ? ((Kin - k0 + 1) >> 1) : (LIN_KC / 2);
            for (int s = 0; s < kend; ++s) {
                const float a = xs[li][2 * s + kh];
                const float b = ws[wave * 32 + li][2 * s + kh];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    uint32_t kb = 0;
    if constexpr (DROP) kb = lin_keep_tile(lq_dropout_load(src), row0, kh, ecol, lane);      // (before any lane leaves)
    if (ecol >= E) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (row < N) {
            if (pre) pre[(size_t)row * E + ecol] = acc[r];
            if constexpr (DROP) y[(size_t)row * E + ecol] = lq_act_apply(acc[r], act) * (((kb >> r) & 1u) ? src.inv_keep : 0.0f);
            else y[(size_t)row * E + ecol] = lq_act_apply(acc[r], act);
        }
    }
}

// Large-N variant of linear_kernel: 128 x 128 (or 256 x 64) tile per workgroup, each of the 4 waves owns 64 x 64 (2 x 2 MFMA tiles, so
// every LDS operand feeds two MFMAs), K staged 32 at a time with the next chunk's global loads in flight (registers)
// while the current chunk is multiplied.  Same k-ordered chains as linear_kernel: bit-identical results.
#define LINB_KC 32

// WR x WC waves, each owning a 64 x 64 block: (2, 2) = 128 x 128 tile; (4, 1) = 256 x 64 tile for narrow outputs (E <= 64)
template <int WR, int WC, bool DROP>
__global__ __launch_bounds__(256) void linear_big_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                         const float* __restrict__ bias, float* __restrict__ y,
                                                         float* __restrict__ pre, int act, lq_dropout_src src, int64_t N, int Kin, int E) {
    constexpr int TR = 64 * WR, TC = 64 * WC;
    __shared__ float xs[TR][LINB_KC + 1];
    __shared__ float ws[TC][LINB_KC + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int wr = wave / WC, wc = wave % WC;
    const int64_t row0 = (int64_t)blockIdx.x * TR;
    const int e0 = blockIdx.y * TC;
    f32x16 acc[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ecol = e0 + (2 * wc + j) * 32 + li;
        const float b0 = (ecol < E && bias) ? bias[ecol] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = b0;
    }
    // staging: thread -> (row r = tid >> 3 (+32 i), 4 consecutive k at 4 (tid & 7)): 128 B per row and instruction
    float4 xr[2 * WR], wrg[2 * WC];
    const int sr = tid >> 3, sk = 4 * (tid & 7);
    auto fetch = [&](int k0) {
        const bool kin = k0 + sk < Kin;                          // Kin is a multiple of 4 on this path
#pragma unroll
        for (int i = 0; i < 2 * WR; ++i) {
            const int64_t row = row0 + sr + 32 * i;
            xr[i] = (row < N && kin) ? *reinterpret_cast<const float4*>(x + (size_t)row * Kin + k0 + sk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < 2 * WC; ++i) {
            const int e = e0 + sr + 32 * i;
            wrg[i] = (e < E && kin) ? *reinterpret_cast<const float4*>(W + (size_t)e * Kin + k0 + sk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < Kin; k0 += LINB_KC) {
#pragma unroll
        for (int i = 0; i < 2 * WR; ++i) {
            float* xd = &xs[sr + 32 * i][sk];
            xd[0] = xr[i].x; xd[1] = xr[i].y; xd[2] = xr[i].z; xd[3] = xr[i].w;
        }
#pragma unroll
        for (int i = 0; i < 2 * WC; ++i) {
            float* wd = &ws[sr + 32 * i][sk];
            wd[0] = wrg[i].x; wd[1] = wrg[i].y; wd[2] = wrg[i].z; wd[3] = wrg[i].w;
        }
        __syncthreads();
        if (k0 + LINB_KC < Kin) fetch(k0 + LINB_KC);            // in flight during the MFMAs below
        const int kend = (Kin - k0 < LINB_KC) ? ((Kin - k0 + 1) >> 1) : (LINB_KC / 2);
        for (int s2 = 0; s2 < kend; ++s2) {
            const int k = 2 * s2 + kh;
            const float a0 = xs[(2 * wr) * 32 + li][k], a1 = xs[(2 * wr + 1) * 32 + li][k];
            const float b0 = ws[(2 * wc) * 32 + li][k], b1 = ws[(2 * wc + 1) * 32 + li][k];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    lq_dropout dr = {};
    if constexpr (DROP) dr = lq_dropout_load(src);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ecol = e0 + (2 * wc + j) * 32 + li;
            uint32_t kb = 0;
            if constexpr (DROP) kb = lin_keep_tile(dr, row0 + (2 * wr + i) * 32, kh, ecol, lane);      // (all lanes: before the column test)
            if (ecol >= E) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = row0 + (2 * wr + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (row < N) {
                    if (pre) pre[(size_t)row * E + ecol] = acc[i][j][r];
                    if constexpr (DROP) y[(size_t)row * E + ecol] = lq_act_apply(acc[i][j][r], act) * (((kb >> r) & 1u) ? src.inv_keep : 0.0f);
                    else y[(size_t)row * E + ecol] = lq_act_apply(acc[i][j][r], act);
                }
            }
        }
}

// ---------------------------------------------------------------------------------------------------
// out[slot(n)][:] = LayerNorm(src[idx ? idx[n] : n][:] + pos[n % T][:])
// 16 lanes own one row (4 rows per wavefront step): the per-row work that every lane repeats (the two reductions --
// four DPP adds each --, the reciprocal square root, address arithmetic) is shared by four rows per instruction, which
// is what keeps the VALU under the store stream.  NJ = float4 groups per lane (16 NJ >= E / 4).
// A workgroup takes 16*chunk consecutive rows per grid-stride step (step r: wave w, lane group g -> row n0 + 16 r + 4 w + g),
// so its stores sweep one contiguous span of the output; each wave fetches its indices for all steps with one vector
// load; ln_w / ln_b sit in LDS; the [T][E] time table is read through the vector L1 (20 KiB at the reference's T = 10).
// ---------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float lq_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

// all-reduce over the 16 lanes of a DPP row; partner order l^1, l^2, l^7, l^15 (the oracle's row_allsum)
__device__ __forceinline__ float lq_row_allsum(float s) {
    s = s + lq_dpp<0xB1>(s);        // quad_perm [1,0,3,2]
    s = s + lq_dpp<0x4E>(s);        // quad_perm [2,3,0,1]
    s = s + lq_dpp<0x141>(s);       // row_half_mirror
    s = s + lq_dpp<0x140>(s);       // row_mirror
    return s;
}

// 64-lane butterfly (backward kernel only; no canonical order attached)
__device__ __forceinline__ float lq_wave_allsum(float s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
    return s;
}

struct EmbedRowsArgs {
    const float* src;
    const int64_t* idx;
    const float* pos;
    const float* ln_w;
    const float* ln_b;
    float* out;
    float* stats;
    int64_t N, src_rows, out_bstride, out_tstride, out_offset;
    int T, E, chunk;
    float eps;
    lq_dropout_src drop;       // DROP instances: out = LayerNorm(...) * m, field row = the OUTPUT row of the slot, col = e
};

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define EMB_CHUNK 16        // most steps per workgroup item (4 indices per step and wave: 64 lanes fetch 16 steps)

template <int NJ, bool DROP>
__global__ __launch_bounds__(256) void embed_rows_kernel(const EmbedRowsArgs a) {
    extern __shared__ float4 emb_lds[];                      // [ln_w: E4][ln_b: E4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, l = lane & 15;
    const int E4 = a.E >> 2;
    float4* sw = emb_lds;
    float4* sb = sw + E4;
    for (int q = tid; q < E4; q += 256) {
        sw[q] = reinterpret_cast<const float4*>(a.ln_w)[q];
        sb[q] = reinterpret_cast<const float4*>(a.ln_b)[q];
    }
    __syncthreads();
    const float invE = 1.0f / (float)a.E;
    const float qnan = __builtin_nanf("");
    const int q16 = 16 / a.T, r16 = 16 - q16 * a.T;
    const int64_t per_item = 16 * (int64_t)a.chunk;
    lq_dropout dr = {};
    if constexpr (DROP) dr = lq_dropout_load(a.drop);
    for (int64_t n0 = (int64_t)blockIdx.x * per_item; n0 < a.N; n0 += (int64_t)gridDim.x * per_item) {
        // this wave's indices for all steps of the item in one vector load: lane (r = lane >> 2, g = lane & 3)
        int64_t kv = n0 + (lane >> 2) * 16 + wave * 4 + (lane & 3);
        if (a.idx && kv < a.N && (lane >> 2) < a.chunk) kv = a.idx[kv];
        int64_t n = n0 + wave * 4 + g;
        int64_t b = n / a.T;
        int t = (int)(n - b * a.T);
        for (int r = 0; r < a.chunk; ++r) {
            const bool live = n < a.N;
            const int64_t k = __shfl(kv, 4 * r + g, 64);
            const bool ok = k >= 0 && k < a.src_rows;          // a bad index poisons its row instead of faulting
            const float4* srow = reinterpret_cast<const float4*>(a.src + (size_t)((ok && live) ? k : 0) * a.E);
            const float4* prow = a.pos ? reinterpret_cast<const float4*>(a.pos + (size_t)(live ? t : 0) * a.E) : nullptr;
            float4 v[NJ];
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int q = l + 16 * j;
                if (q < E4) {
                    float4 c = srow[q];
                    if (a.pos) {
                        const float4 p = prow[q];
                        c.x = c.x + p.x; c.y = c.y + p.y; c.z = c.z + p.z; c.w = c.w + p.w;
                    }
                    v[j] = c;
                    s = s + c.x; s = s + c.y; s = s + c.z; s = s + c.w;
                }
            }
            // Centre twice.  fl(1/E) is inexact for most E and the fp32 sum of a row around 1000 is ulps of 1000 E off, so the
            // first mean misses by up to ~1e-4 -- which rstd = 316 blows up on a constant row.  v - mean0 is exact for values
            // within a factor 2 of the mean: the mean of the centred values is that miss, to fp32 accuracy at ITS size.
            const float mean0 = lq_row_allsum(s) * invE;
            float rs = 0.0f;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (l + 16 * j < E4) {
                    float4 d = v[j];
                    d.x = d.x - mean0; d.y = d.y - mean0; d.z = d.z - mean0; d.w = d.w - mean0;
                    v[j] = d;
                    rs = rs + d.x; rs = rs + d.y; rs = rs + d.z; rs = rs + d.w;
                }
            const float rest = lq_row_allsum(rs) * invE;
            const float mean = mean0 + rest;                   // what stats keeps
            float ss = 0.0f;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (l + 16 * j < E4) {
                    float4 d = v[j];
                    d.x = d.x - rest; d.y = d.y - rest; d.z = d.z - rest; d.w = d.w - rest;
                    v[j] = d;
                    ss = lq_fma(d.x, d.x, ss); ss = lq_fma(d.y, d.y, ss);
                    ss = lq_fma(d.z, d.z, ss); ss = lq_fma(d.w, d.w, ss);
                }
            const float var = lq_row_allsum(ss) * invE;
            const float rstd = 1.0f / lq_sqrt(var + a.eps);
            const size_t slot = (size_t)(b * a.out_bstride + t * a.out_tstride + a.out_offset);
            float4* orow = reinterpret_cast<float4*>(a.out + slot);
            uint32_t orow_n = 0;                                 // the output row b S + s of the slot (host: strides and offset are multiples of E)
            if constexpr (DROP) orow_n = (uint32_t)(slot / (size_t)a.E);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int q = l + 16 * j;
                if (q < E4 && live) {
                    const float4 w = sw[q], bb = sb[q];
                    f32x4 o;
                    o.x = lq_fma(v[j].x * rstd, w.x, bb.x);
                    o.y = lq_fma(v[j].y * rstd, w.y, bb.y);
                    o.z = lq_fma(v[j].z * rstd, w.z, bb.z);
                    o.w = lq_fma(v[j].w * rstd, w.w, bb.w);
                    if constexpr (DROP) {                        // lane's float4 = columns 4 q .. 4 q + 3: one draw
                        const uint32_t kb = lq_dropout_keep4(dr, orow_n, (uint32_t)q);
                        o.x *= (kb & 1u) ? dr.inv_keep : 0.0f; o.y *= (kb & 2u) ? dr.inv_keep : 0.0f;
                        o.z *= (kb & 4u) ? dr.inv_keep : 0.0f; o.w *= (kb & 8u) ? dr.inv_keep : 0.0f;
                    }
                    if (!ok) o = f32x4{qnan, qnan, qnan, qnan};
                    __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(orow + q));   // written once, read by a later launch
                }
            }
            if (a.stats && live && l == 0) {
                a.stats[2 * n] = ok ? mean : qnan;
                a.stats[2 * n + 1] = ok ? rstd : qnan;
            }
            n += 16;
            t += r16;
            b += q16;
            if (t >= a.T) { t -= a.T; ++b; }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Backward of embed_rows_kernel.  gout is addressed like out.  Per row:
//   xhat = (src[k] + pos[t] - mean) * rstd,  gh = gout * w,
//   gv   = rstd * (gh - mean_e(gh) - xhat * mean_e(gh * xhat))
//   g_src[k] += gv (atomic; = gradient of the table / of the dense pre-LayerNorm rows),  g_pos[t] += gv,
//   g_lnw += gout * xhat,  g_lnb += gout   (kept in registers across the wave's rows, flushed once).
// ---------------------------------------------------------------------------------------------------
struct EmbedBwdArgs {
    const float* gout;
    const float* src;
    const int64_t* idx;
    const float* pos;
    const float* stats;
    const float* ln_w;
    float* g_src;
    float* g_pos;
    float* g_lnw;
    float* g_lnb;
    int64_t N, src_rows, out_bstride, out_tstride, out_offset;
    int T, E;
    float* gv;                 // large batches: the rows' gradients are written here (and scattered by a second pass), not added atomically
    int64_t* idx_clean;        // ... with the indices made safe for that pass (a row with a bad index: code 0, zero gradient)
    lq_dropout_src drop;       // DROP instances: gout is read as gout * m, m regenerated from the forward's field
    float* part;               // gv kernel, fixed-order route: workgroup w leaves its (g_pos, g_lnw, g_lnb) sums at part[w][3][E] and
                               // embed_param_reduce_kernel adds them in workgroup order -- no atomics, the same bits every run
};

// gout * m for the float4 at columns 4 q .. 4 q + 3 of the output row that holds float offset `slot`
__device__ __forceinline__ float4 emb_drop4(float4 g, lq_dropout dr, size_t slot, int E, int q) {
    const uint32_t kb = lq_dropout_keep4(dr, (uint32_t)(slot / (size_t)E), (uint32_t)q);
    g.x *= (kb & 1u) ? dr.inv_keep : 0.0f; g.y *= (kb & 2u) ? dr.inv_keep : 0.0f;
    g.z *= (kb & 4u) ? dr.inv_keep : 0.0f; g.w *= (kb & 8u) ? dr.inv_keep : 0.0f;
    return g;
}

// Large batches (lipvq_embed_rows_bwd_ws_f32).  The kernel above adds every row's E-float gradient to its table row AND to its
// time-embedding row with fp32 atomics: 2 N E atomics, the time-embedding ones onto T E addresses -- 8.7 ms at the metric's
// batch (N = 524 280, E = 512, T = 10), 55 ms when the codes collapse onto one table row.  Here a wave owns ONE time step t and
// walks batches b, b + W, ...: the time-embedding gradient stays in registers and costs one flush per wave; the row gradient is
// written once (gv [N][E]) and summed per code by the counting-sort scatter (lipvq_scatter.hip): no atomics on the table either.
template <int NJ, bool DROP>
__global__ __launch_bounds__(256) void embed_rows_bwd_gv_kernel(const EmbedBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int E4 = a.E >> 2;
    const float fE = (float)a.E;
    lq_dropout dr = {};
    if constexpr (DROP) dr = lq_dropout_load(a.drop);
    float4 w[NJ], aw[NJ], ab[NJ], ap[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int q = lane + 64 * j;
        aw[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        ab[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        ap[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        w[j] = q < E4 ? reinterpret_cast<const float4*>(a.ln_w)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __shared__ float4 red[3][4][64 * NJ];                      // the four waves' (ap, aw, ab) before ONE wave flushes them
    const int wave = threadIdx.x >> 6;
    const int64_t gpt = gridDim.x / a.T;                       // workgroups per time step (host: >= 1)
    if ((int64_t)blockIdx.x >= gpt * a.T) return;              // (whole workgroups: no barrier is skipped by part of one)
    const int t = (int)(blockIdx.x % a.T);                     // the four waves of a workgroup share the time step
    const int64_t wpt = gpt * 4;
    const int64_t B = (a.N + a.T - 1) / a.T;
    const float4* prow = a.pos ? reinterpret_cast<const float4*>(a.pos + (size_t)t * a.E) : nullptr;
    for (int64_t b = (int64_t)(blockIdx.x / a.T) * 4 + wave; b < B; b += wpt) {
        const int64_t n = b * a.T + t;
        if (n >= a.N) break;                                   // (wave-uniform)
        const int64_t k = a.idx ? a.idx[n] : n;
        const bool ok = k >= 0 && k < a.src_rows;
        float4* gvrow = a.gv ? reinterpret_cast<float4*>(a.gv + (size_t)n * a.E) : nullptr;
        if (a.idx_clean && lane == 0) a.idx_clean[n] = ok ? k : 0;
        if (!ok) {                                             // wave-uniform: a poisoned row contributes nothing
            if (gvrow) {
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    if (lane + 64 * j < E4) gvrow[lane + 64 * j] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            continue;
        }
        const float mean = a.stats[2 * n], rstd = a.stats[2 * n + 1];
        const float4* srow = reinterpret_cast<const float4*>(a.src + (size_t)k * a.E);
        const size_t slot = (size_t)(b * a.out_bstride + t * a.out_tstride + a.out_offset);
        const float4* grow = reinterpret_cast<const float4*>(a.gout + slot);
        float4 xh[NJ], gh[NJ];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int q = lane + 64 * j;
            if (q < E4) {
                float4 c = srow[q];
                if (prow) {
                    const float4 p = prow[q];
                    c.x = c.x + p.x; c.y = c.y + p.y; c.z = c.z + p.z; c.w = c.w + p.w;
                }
                c.x = (c.x - mean) * rstd; c.y = (c.y - mean) * rstd;
                c.z = (c.z - mean) * rstd; c.w = (c.w - mean) * rstd;
                float4 g = grow[q];
                if constexpr (DROP) g = emb_drop4(g, dr, slot, a.E, q);
                aw[j].x += g.x * c.x; aw[j].y += g.y * c.y; aw[j].z += g.z * c.z; aw[j].w += g.w * c.w;
                ab[j].x += g.x; ab[j].y += g.y; ab[j].z += g.z; ab[j].w += g.w;
                float4 h;
                h.x = g.x * w[j].x; h.y = g.y * w[j].y; h.z = g.z * w[j].z; h.w = g.w * w[j].w;
                s1 += (h.x + h.y) + (h.z + h.w);
                s2 += (h.x * c.x + h.y * c.y) + (h.z * c.z + h.w * c.w);
                xh[j] = c;
                gh[j] = h;
            }
        }
        const float c1 = lq_wave_allsum(s1) / fE, c2 = lq_wave_allsum(s2) / fE;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int q = lane + 64 * j;
            if (q < E4) {
                float4 gv;
                gv.x = rstd * (gh[j].x - c1 - xh[j].x * c2);
                gv.y = rstd * (gh[j].y - c1 - xh[j].y * c2);
                gv.z = rstd * (gh[j].z - c1 - xh[j].z * c2);
                gv.w = rstd * (gh[j].w - c1 - xh[j].w * c2);
                if (gvrow) gvrow[q] = gv;
                ap[j].x += gv.x; ap[j].y += gv.y; ap[j].z += gv.z; ap[j].w += gv.w;
            }
        }
    }
    // one flush per WORKGROUP (every flush is 3 E atomics onto 2 E + T E addresses: with one per wave of an 8 192-wave grid the
    // flushes cost more than the rows -- 1.15 ms for the whole launch)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        red[0][wave][lane + 64 * j] = ap[j];
        red[1][wave][lane + 64 * j] = aw[j];
        red[2][wave][lane + 64 * j] = ab[j];
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int q = lane + 64 * j;
        if (q < E4) {
            float4 sp = red[0][0][q], sw = red[1][0][q], sb = red[2][0][q];
#pragma unroll
            for (int u = 1; u < 4; ++u) {
                const float4 p = red[0][u][q], ww = red[1][u][q], bb = red[2][u][q];
                sp.x += p.x; sp.y += p.y; sp.z += p.z; sp.w += p.w;
                sw.x += ww.x; sw.y += ww.y; sw.z += ww.z; sw.w += ww.w;
                sb.x += bb.x; sb.y += bb.y; sb.z += bb.z; sb.w += bb.w;
            }
            if (a.part) {                                      // (uniform) fixed-order route: one partial row triple per workgroup
                float4* d = reinterpret_cast<float4*>(a.part + (size_t)blockIdx.x * 3 * a.E);
                d[q] = sp; d[E4 + q] = sw; d[2 * E4 + q] = sb;
                continue;
            }
            if (a.g_pos) {
                float* d = a.g_pos + (size_t)t * a.E + 4 * q;
                atomicAdd(d + 0, sp.x); atomicAdd(d + 1, sp.y); atomicAdd(d + 2, sp.z); atomicAdd(d + 3, sp.w);
            }
            if (a.g_lnw) {
                float* d = a.g_lnw + 4 * q;
                atomicAdd(d + 0, sw.x); atomicAdd(d + 1, sw.y); atomicAdd(d + 2, sw.z); atomicAdd(d + 3, sw.w);
            }
            if (a.g_lnb) {
                float* d = a.g_lnb + 4 * q;
                atomicAdd(d + 0, sb.x); atomicAdd(d + 1, sb.y); atomicAdd(d + 2, sb.z); atomicAdd(d + 3, sb.w);
            }
        }
    }
}

// The second pass of the fixed-order route.  part [nwg][3][E]: workgroup w = i T + t of embed_rows_bwd_gv_kernel (time step t, i-th
// of the gpt workgroups of that step).  Item (which, q), owned by 16 lanes: which < T adds the gpt partial sums of time step `which`
// to g_pos, which == T / T + 1 all nwg partial sums to g_lnw / g_lnb.  Lane k of the 16 adds partials k, k + 16, ... in ascending
// order, the 16 lane sums are combined by a fixed xor butterfly, lane 0 writes: one order, one writer per address.
__global__ __launch_bounds__(256) void embed_param_reduce_kernel(const float* __restrict__ part, int nwg, int T, int E,
                                                                 float* __restrict__ g_pos, float* __restrict__ g_lnw,
                                                                 float* __restrict__ g_lnb) {
    const int E4 = E >> 2;
    const int gid = blockIdx.x * 256 + threadIdx.x, item = gid >> 4, k = gid & 15;
    if (item >= (T + 2) * E4) return;                              // (whole 16-lane groups)
    const int which = item / E4, q = item - which * E4;
    float* dst = which < T ? g_pos : (which == T ? g_lnw : g_lnb);
    if (!dst) return;
    const int kind = which < T ? 0 : which - T + 1;
    const int count = which < T ? nwg / T : nwg, stride = which < T ? T : 1, base = which < T ? which : 0;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int j = k; j < count; j += 16) {
        const float4 v = reinterpret_cast<const float4*>(part + ((size_t)(base + j * stride) * 3 + kind) * E)[q];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        s.x += __shfl_xor(s.x, off, 64); s.y += __shfl_xor(s.y, off, 64);
        s.z += __shfl_xor(s.z, off, 64); s.w += __shfl_xor(s.w, off, 64);
    }
    if (k != 0) return;
    float4* d = reinterpret_cast<float4*>(dst + (which < T ? (size_t)which * E : 0)) + q;
    float4 o = *d;
    o.x += s.x; o.y += s.y; o.z += s.z; o.w += s.w;
    *d = o;
}

template <int NJ, bool DROP>
__global__ __launch_bounds__(256) void embed_rows_bwd_kernel(const EmbedBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int E4 = a.E >> 2;
    const float fE = (float)a.E;
    lq_dropout dr = {};
    if constexpr (DROP) dr = lq_dropout_load(a.drop);
    float4 w[NJ], aw[NJ], ab[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int q = lane + 64 * j;
        aw[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        ab[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < E4) w[j] = reinterpret_cast<const float4*>(a.ln_w)[q];
    }
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t n = wave0; n < a.N; n += nwaves) {
        const int64_t k = a.idx ? a.idx[n] : n;
        if (k < 0 || k >= a.src_rows) continue;          // wave-uniform
        const int64_t b = n / a.T;
        const int t = (int)(n - b * a.T);
        const float mean = a.stats[2 * n], rstd = a.stats[2 * n + 1];
        const float4* srow = reinterpret_cast<const float4*>(a.src + (size_t)k * a.E);
        const float4* prow = a.pos ? reinterpret_cast<const float4*>(a.pos + (size_t)t * a.E) : nullptr;
        const size_t slot = (size_t)(b * a.out_bstride + t * a.out_tstride + a.out_offset);
        const float4* grow = reinterpret_cast<const float4*>(a.gout + slot);
        float4 xh[NJ], gh[NJ];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int q = lane + 64 * j;
            if (q < E4) {
                float4 c = srow[q];
                if (prow) {
                    const float4 p = prow[q];
                    c.x = c.x + p.x; c.y = c.y + p.y; c.z = c.z + p.z; c.w = c.w + p.w;
                }
                c.x = (c.x - mean) * rstd; c.y = (c.y - mean) * rstd;
                c.z = (c.z - mean) * rstd; c.w = (c.w - mean) * rstd;
                float4 g = grow[q];
                if constexpr (DROP) g = emb_drop4(g, dr, slot, a.E, q);
                aw[j].x += g.x * c.x; aw[j].y += g.y * c.y; aw[j].z += g.z * c.z; aw[j].w += g.w * c.w;
                ab[j].x += g.x; ab[j].y += g.y; ab[j].z += g.z; ab[j].w += g.w;
                float4 h;
                h.x = g.x * w[j].x; h.y = g.y * w[j].y; h.z = g.z * w[j].z; h.w = g.w * w[j].w;
                s1 += (h.x + h.y) + (h.z + h.w);
                s2 += (h.x * c.x + h.y * c.y) + (h.z * c.z + h.w * c.w);
                xh[j] = c;
                gh[j] = h;
            }
        }
        const float c1 = lq_wave_allsum(s1) / fE, c2 = lq_wave_allsum(s2) / fE;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int q = lane + 64 * j;
            if (q < E4) {
                float4 gv;
                gv.x = rstd * (gh[j].x - c1 - xh[j].x * c2);
                gv.y = rstd * (gh[j].y - c1 - xh[j].y * c2);
                gv.z = rstd * (gh[j].z - c1 - xh[j].z * c2);
                gv.w = rstd * (gh[j].w - c1 - xh[j].w * c2);
                if (a.g_src) {
                    float* d = a.g_src + (size_t)k * a.E + 4 * q;
                    if (a.idx) {
                        atomicAdd(d + 0, gv.x); atomicAdd(d + 1, gv.y); atomicAdd(d + 2, gv.z); atomicAdd(d + 3, gv.w);
                    } else {                                  // one row, one writer
                        reinterpret_cast<float4*>(d)[0] = gv;
                    }
                }
                if (a.g_pos) {
                    float* d = a.g_pos + (size_t)t * a.E + 4 * q;
                    atomicAdd(d + 0, gv.x); atomicAdd(d + 1, gv.y); atomicAdd(d + 2, gv.z); atomicAdd(d + 3, gv.w);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int q = lane + 64 * j;
        if (q < E4) {
            if (a.g_lnw) {
                float* d = a.g_lnw + 4 * q;
                atomicAdd(d + 0, aw[j].x); atomicAdd(d + 1, aw[j].y); atomicAdd(d + 2, aw[j].z); atomicAdd(d + 3, aw[j].w);
            }
            if (a.g_lnb) {
                float* d = a.g_lnb + 4 * q;
                atomicAdd(d + 0, ab[j].x); atomicAdd(d + 1, ab[j].y); atomicAdd(d + 2, ab[j].z); atomicAdd(d + 3, ab[j].w);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------
static int embed_grid(int64_t rows_per_wg_step, int64_t N) {
    int64_t g = (N + rows_per_wg_step - 1) / rows_per_wg_step;
#define LQ_EMB_GRID 2048
    if (g > LQ_EMB_GRID) g = LQ_EMB_GRID;              // 8 workgroups per CU, grid-stride beyond
    if (g < 1) g = 1;
    return (int)g;
}

// small batches (a training step) spread 16 rows per workgroup; large ones up to 16 * EMB_CHUNK consecutive rows
static int embed_chunk(int64_t N) {
    const int64_t c = N / (16 * 2048);
    return c < 1 ? 1 : (c > EMB_CHUNK ? EMB_CHUNK : (int)c);
}

static int embed_check(const char* what, int64_t N, int T, int E, int64_t src_rows, int64_t bstride, int64_t tstride,
                       int64_t offset) {
    if (N < 0 || T <= 0 || src_rows <= 0) return fail(LIPVQ_EINVAL, "%s: bad sizes N=%lld T=%d src_rows=%lld", what,
                                                      (long long)N, T, (long long)src_rows);
    if (E <= 0 || (E & 3) || E > 1024) return fail(LIPVQ_EUNSUPPORTED, "%s: E=%d (need a multiple of 4, <= 1024)", what, E);
    if ((bstride & 3) || (tstride & 3) || (offset & 3) || bstride < 0 || tstride < 0 || offset < 0)
        return fail(LIPVQ_EINVAL, "%s: output strides/offset must be non-negative multiples of 4 floats", what);
    return LIPVQ_OK;
}

// one launch for lipvq_linear_act_f32 (snap == NULL) and lipvq_linear_act_drop_f32: the same kernel choice for both
static int linear_act_launch(const char* what, const float* x, const float* W, const float* b, float* y, float* pre,
                             const int64_t* snap, uint32_t site, double p, int64_t N, int Kin, int E, int act, void* stream) {
    if (!x || !W || !y) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if (N < 0 || Kin <= 0 || E <= 0) return fail(LIPVQ_EINVAL, "%s: bad sizes", what);
    if (act < LIPVQ_ACT_NONE || act > LIPVQ_ACT_RELU) return fail(LIPVQ_EINVAL, "%s: bad activation %d", what, act);
    if (N == 0) return LIPVQ_OK;
    const int64_t gx = (N + LIN_ROWS - 1) / LIN_ROWS;
    if (gx > 0x7fffffffLL) return fail(LIPVQ_EUNSUPPORTED, "%s: N too large", what);
    const lq_dropout_src src = snap ? lq_dropout_src_make(snap, site, p) : lq_dropout_src{};
#define LQ_LIN_BIG_MIN 512          // workgroups of the 128 x 128 tiling needed before it pays (2 per CU)
    const bool narrow = E <= 64;                                  // 256 x 64 tiles instead of 128 x 128
    const int TR = narrow ? 256 : 128, TC = narrow ? 64 : 128;
    const int64_t big_wgs = ((N + TR - 1) / TR) * ((E + TC - 1) / TC);
    if (big_wgs >= LQ_LIN_BIG_MIN && (Kin & 3) == 0) {
        dim3 grid((unsigned)((N + TR - 1) / TR), (unsigned)((E + TC - 1) / TC));
        lq_dispatch<0, 1>(snap ? 1 : 0, [&](auto drop) {
            constexpr bool DROP = decltype(drop)::value != 0;
            if (narrow)
                hipLaunchKernelGGL((linear_big_kernel<4, 1, DROP>), grid, dim3(256), 0, (hipStream_t)stream, x, W, b, y, pre, act, src, N, Kin, E);
            else
                hipLaunchKernelGGL((linear_big_kernel<2, 2, DROP>), grid, dim3(256), 0, (hipStream_t)stream, x, W, b, y, pre, act, src, N, Kin, E);
        });
        return check_launch("linear_big_kernel");
    }
    dim3 grid((unsigned)gx, (unsigned)((E + 127) / 128));
    if (snap)
        hipLaunchKernelGGL(linear_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, W, b, y, pre, act, src, N, Kin, E);
    else
        hipLaunchKernelGGL(linear_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, W, b, y, pre, act, src, N, Kin, E);
    return check_launch("linear_kernel");
}

// the in-kernel source of an embed_rows call: the field row is the output row of a slot, so the slots must be whole rows of E
// floats, and the last output row must fit the 32-bit counter word
static int embed_drop_check(const char* what, const int64_t* snap, double p, int64_t N, int T, int E, int64_t bstride, int64_t tstride,
                            int64_t offset) {
    if (E <= 0 || T <= 0 || N < 0) return fail(LIPVQ_EINVAL, "%s: bad sizes", what);
    if (bstride % E || tstride % E || offset % E || bstride < 0 || tstride < 0 || offset < 0)
        return fail(LIPVQ_EINVAL, "%s: output strides/offset must be multiples of E under the in-kernel dropout source", what);
    const int64_t B = (N + T - 1) / T;
    const int64_t rows = N == 0 ? 0 : ((B - 1) * bstride + (int64_t)(T - 1) * tstride + offset) / E + 1;
    return lq_dropout_check(what, snap, p, rows);
}

// one forward launch for lipvq_embed_rows_f32 (drop == NULL) and lipvq_embed_rows_drop_f32
static int embed_rows_launch(const char* what, const float* src, const int64_t* idx, const float* pos, const float* ln_w,
                             const float* ln_b, float eps, float* out, float* stats, const lq_dropout_src* drop, int64_t N, int T,
                             int E, int64_t src_rows, int64_t out_batch_stride, int64_t out_t_stride, int64_t out_offset,
                             void* stream) {
    if (!src || !ln_w || !ln_b || !out) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    const int rc = embed_check(what, N, T, E, src_rows, out_batch_stride, out_t_stride, out_offset);
    if (rc) return rc;
    if (!idx && src_rows < N) return fail(LIPVQ_EINVAL, "%s: src has fewer rows than N", what);
    if (N == 0) return LIPVQ_OK;
    const int chunk = embed_chunk(N);
    EmbedRowsArgs a{src, idx, pos, ln_w, ln_b, out, stats, N, src_rows, out_batch_stride, out_t_stride, out_offset, T, E,
                    chunk, eps, drop ? *drop : lq_dropout_src{}};
    const dim3 grid(embed_grid(16 * chunk, N)), block(256);
    const size_t lds = (size_t)2 * E * sizeof(float);       // ln_w, ln_b
    hipStream_t st = (hipStream_t)stream;
    const int nj = (E / 4 + 15) / 16;
    lq_dispatch<0, 1>(drop ? 1 : 0, [&](auto dsel) {
        constexpr bool DROP = decltype(dsel)::value != 0;
        if (nj <= 2) hipLaunchKernelGGL((embed_rows_kernel<2, DROP>), grid, block, lds, st, a);
        else if (nj <= 4) hipLaunchKernelGGL((embed_rows_kernel<4, DROP>), grid, block, lds, st, a);
        else if (nj <= 8) hipLaunchKernelGGL((embed_rows_kernel<8, DROP>), grid, block, lds, st, a);
        else hipLaunchKernelGGL((embed_rows_kernel<16, DROP>), grid, block, lds, st, a);
    });
    return check_launch("embed_rows_kernel");
}

// the two backward launches, shared by the plain and the _drop entry points (drop == NULL: plain)
static int embed_rows_bwd_launch(const char* what, const float* gout, const float* src, const int64_t* idx, const float* pos,
                                 const float* stats, const float* ln_w, float* g_src, float* g_pos, float* g_lnw, float* g_lnb,
                                 const lq_dropout_src* drop, int64_t N, int T, int E, int64_t src_rows, int64_t out_batch_stride,
                                 int64_t out_t_stride, int64_t out_offset, void* stream) {
    if (!gout || !src || !stats || !ln_w) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    const int rc = embed_check(what, N, T, E, src_rows, out_batch_stride, out_t_stride, out_offset);
    if (rc) return rc;
    if (!idx && src_rows < N) return fail(LIPVQ_EINVAL, "%s: src has fewer rows than N", what);
    if (N == 0) return LIPVQ_OK;
    EmbedBwdArgs a{gout, src, idx, pos, stats, ln_w, g_src, g_pos, g_lnw, g_lnb, N, src_rows,
                   out_batch_stride, out_t_stride, out_offset, T, E, nullptr, nullptr, drop ? *drop : lq_dropout_src{}, nullptr};
    int g = embed_grid(4, N);
    if (g > 512) g = 512;                 // fewer waves = fewer final flushes of the LayerNorm gradients
    const dim3 grid(g), block(256);
    hipStream_t st = (hipStream_t)stream;
    lq_dispatch<0, 1>(drop ? 1 : 0, [&](auto dsel) {
        constexpr bool DROP = decltype(dsel)::value != 0;
        switch ((E + 255) / 256) {
            case 1: hipLaunchKernelGGL((embed_rows_bwd_kernel<1, DROP>), grid, block, 0, st, a); break;
            case 2: hipLaunchKernelGGL((embed_rows_bwd_kernel<2, DROP>), grid, block, 0, st, a); break;
            case 3: hipLaunchKernelGGL((embed_rows_bwd_kernel<3, DROP>), grid, block, 0, st, a); break;
            default: hipLaunchKernelGGL((embed_rows_bwd_kernel<4, DROP>), grid, block, 0, st, a); break;
        }
    });
    return check_launch("embed_rows_bwd_kernel");
}

static int embed_rows_bwd_ws_launch(const char* what, const float* gout, const float* src, const int64_t* idx, const float* pos,
                                    const float* stats, const float* ln_w, float* g_src, float* g_pos, float* g_lnw, float* g_lnb,
                                    void* workspace, const lq_dropout_src* drop, int64_t N, int T, int E, int64_t src_rows,
                                    int64_t out_batch_stride, int64_t out_t_stride, int64_t out_offset, void* stream) {
    if (!gout || !src || !stats || !ln_w || (idx && !workspace)) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    const int rc = embed_check(what, N, T, E, src_rows, out_batch_stride, out_t_stride, out_offset);
    if (rc) return rc;
    if (!idx && src_rows < N) return fail(LIPVQ_EINVAL, "%s: src has fewer rows than N", what);
    const bool okay = idx ? lipvq_embed_rows_bwd_ws_supported(N, T, E, src_rows) != 0 : (N >= 32768 && T <= 1024);
    if (!okay)
        return fail(LIPVQ_EUNSUPPORTED, "%s: N=%lld T=%d E=%d src_rows=%lld outside the supported range", what,
                    (long long)N, T, E, (long long)src_rows);
    const size_t gvb = ((size_t)N * E * sizeof(float) + 255) & ~(size_t)255, icb = ((size_t)N * sizeof(int64_t) + 255) & ~(size_t)255;
    // dense rows (idx == NULL): row n of g_src has one writer -- the row gradients ARE g_src, nothing to scatter
    float* gv = !g_src ? nullptr : (idx ? (float*)workspace : g_src);
    int64_t* idx_clean = (g_src && idx) ? (int64_t*)((char*)workspace + gvb) : nullptr;
    EmbedBwdArgs a{gout, src, idx, pos, stats, ln_w, g_src, g_pos, g_lnw, g_lnb, N, src_rows,
                   out_batch_stride, out_t_stride, out_offset, T, E, gv, idx_clean, drop ? *drop : lq_dropout_src{}, nullptr};
    const dim3 grid(1024 < T ? T : 1024), block(256);          // >= one workgroup per time step (T <= 1024)
    hipStream_t st = (hipStream_t)stream;
    lq_dispatch<0, 1>(drop ? 1 : 0, [&](auto dsel) {
        constexpr bool DROP = decltype(dsel)::value != 0;
        switch ((E + 255) / 256) {
            case 1: hipLaunchKernelGGL((embed_rows_bwd_gv_kernel<1, DROP>), grid, block, 0, st, a); break;
            case 2: hipLaunchKernelGGL((embed_rows_bwd_gv_kernel<2, DROP>), grid, block, 0, st, a); break;
            case 3: hipLaunchKernelGGL((embed_rows_bwd_gv_kernel<3, DROP>), grid, block, 0, st, a); break;
            default: hipLaunchKernelGGL((embed_rows_bwd_gv_kernel<4, DROP>), grid, block, 0, st, a); break;
        }
    });
    if (int e = check_launch("embed_rows_bwd_gv_kernel")) return e;
    if (!g_src || !idx) return LIPVQ_OK;
    return lipvq_scatter_add_sorted_f32(gv, idx_clean, g_src, (char*)workspace + gvb + icb, N, (int)src_rows, E, 0, stream);
}

// The fixed-order backward (lipvq_embed_rows_bwd_det_f32): the gv kernel at any N with its flush sent to partial sums, the
// second pass, and for indexed rows a table scatter without atomics.  workspace: [part][gv][idx_clean][sorted-scatter workspace].
static int embed_det_groups(int64_t N, int T) {                    // workgroups per time step
    const int64_t B = (N + T - 1) / T;
    int64_t g = (B + 3) / 4, cap = 1024 / T;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}
// Indexed rows the counting-sort scatter does not take (N < 32768, or more than 16384 table rows).  The row-order scatter has
// one workgroup per table row scan all N indices once per 256 columns: src_rows * N * ceil(E / 256) index reads, microseconds at
// a training step and out of proportion for a large table or a mid-size batch.  Up to LQ_EMB_DET_SCAN_MAX reads it is taken
// (the table gradient then repeats bit for bit too); beyond, the table rows are added with the fp32 atomics of
// lipvq_scatter_add_f32, as lipvq_embed_rows_bwd_f32 adds them -- g_pos, g_lnw and g_lnb keep their fixed order either way.
#define LQ_EMB_DET_SCAN_MAX (1LL << 24)
static bool embed_det_row_order_scatter(int64_t N, int64_t src_rows, int E) {
    return src_rows * N * ((E + 255) / 256) <= LQ_EMB_DET_SCAN_MAX;
}

static size_t embed_det_part_bytes(int64_t N, int T, int E) {
    return (((size_t)embed_det_groups(N, T) * T * 3 * E * sizeof(float)) + 255) & ~(size_t)255;
}

static int embed_rows_bwd_det_launch(const char* what, const float* gout, const float* src, const int64_t* idx, const float* pos,
                                     const float* stats, const float* ln_w, float* g_src, float* g_pos, float* g_lnw, float* g_lnb,
                                     void* workspace, const lq_dropout_src* drop, int64_t N, int T, int E, int64_t src_rows,
                                     int64_t out_batch_stride, int64_t out_t_stride, int64_t out_offset, void* stream) {
    if (!gout || !src || !stats || !ln_w || !workspace) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    const int rc = embed_check(what, N, T, E, src_rows, out_batch_stride, out_t_stride, out_offset);
    if (rc) return rc;
    if (!idx && src_rows < N) return fail(LIPVQ_EINVAL, "%s: src has fewer rows than N", what);
    if (T > 1024 || (idx && src_rows > 0x7fffffffLL)) return fail(LIPVQ_EUNSUPPORTED, "%s: T=%d src_rows=%lld", what, T, (long long)src_rows);
    if ((((uintptr_t)g_pos | (uintptr_t)g_lnw | (uintptr_t)g_lnb | (uintptr_t)workspace) & 15) != 0)
        return fail(LIPVQ_EINVAL, "%s: g_pos / g_lnw / g_lnb / workspace must be 16-byte aligned", what);
    if (N == 0) return LIPVQ_OK;
    const size_t pb = embed_det_part_bytes(N, T, E);
    const size_t gvb = ((size_t)N * E * sizeof(float) + 255) & ~(size_t)255, icb = ((size_t)N * sizeof(int64_t) + 255) & ~(size_t)255;
    float* part = (float*)workspace;
    float* gv = !g_src ? nullptr : (idx ? (float*)((char*)workspace + pb) : g_src);
    int64_t* idx_clean = (g_src && idx) ? (int64_t*)((char*)workspace + pb + gvb) : nullptr;
    EmbedBwdArgs a{gout, src, idx, pos, stats, ln_w, g_src, g_pos, g_lnw, g_lnb, N, src_rows,
                   out_batch_stride, out_t_stride, out_offset, T, E, gv, idx_clean, drop ? *drop : lq_dropout_src{}, part};
    const int nwg = embed_det_groups(N, T) * T;
    const dim3 grid(nwg), block(256);
    hipStream_t st = (hipStream_t)stream;
    lq_dispatch<0, 1>(drop ? 1 : 0, [&](auto dsel) {
        constexpr bool DROP = decltype(dsel)::value != 0;
        switch ((E + 255) / 256) {
            case 1: hipLaunchKernelGGL((embed_rows_bwd_gv_kernel<1, DROP>), grid, block, 0, st, a); break;
            case 2: hipLaunchKernelGGL((embed_rows_bwd_gv_kernel<2, DROP>), grid, block, 0, st, a); break;
            case 3: hipLaunchKernelGGL((embed_rows_bwd_gv_kernel<3, DROP>), grid, block, 0, st, a); break;
            default: hipLaunchKernelGGL((embed_rows_bwd_gv_kernel<4, DROP>), grid, block, 0, st, a); break;
        }
    });
    if (int e = check_launch("embed_rows_bwd_gv_kernel")) return e;
    if (g_pos || g_lnw || g_lnb) {
        const int items = (T + 2) * (E >> 2);
        hipLaunchKernelGGL(embed_param_reduce_kernel, dim3((items + 15) / 16), block, 0, st, part, nwg, T, E, g_pos, g_lnw, g_lnb);
        if (int e = check_launch("embed_param_reduce_kernel")) return e;
    }
    if (!g_src || !idx) return LIPVQ_OK;
    if (lipvq_scatter_add_sorted_supported(N, (int)src_rows, E))
        return lipvq_scatter_add_sorted_f32(gv, idx_clean, g_src, (char*)workspace + pb + gvb + icb, N, (int)src_rows, E, 0, stream);
    if (embed_det_row_order_scatter(N, src_rows, E)) return lipvq_scatter_add_det_f32(gv, idx_clean, g_src, N, (int)src_rows, E, stream);
    return lipvq_scatter_add_f32(gv, idx_clean, g_src, N, (int)src_rows, E, stream);
}

extern "C" {

size_t lipvq_embed_rows_bwd_det_workspace_bytes(int64_t N, int T, int E, int64_t src_rows, int indexed) {
    if (N <= 0 || T <= 0 || T > 1024 || E <= 0 || src_rows <= 0) return 0;
    size_t b = embed_det_part_bytes(N, T, E);
    if (indexed) {
        b += (((size_t)N * E * sizeof(float) + 255) & ~(size_t)255) + (((size_t)N * sizeof(int64_t) + 255) & ~(size_t)255);
        if (src_rows <= 0x7fffffffLL && lipvq_scatter_add_sorted_supported(N, (int)src_rows, E))
            b += lipvq_scatter_add_sorted_workspace_bytes(N, (int)src_rows, E);
    }
    return b;
}

int lipvq_embed_rows_bwd_det_f32(const float* gout, const float* src, const int64_t* idx, const float* pos, const float* stats,
                                 const float* ln_w, float* g_src, float* g_pos, float* g_lnw, float* g_lnb, void* workspace,
                                 const int64_t* snap, uint32_t site, double p, int64_t N, int T, int E, int64_t src_rows,
                                 int64_t out_batch_stride, int64_t out_t_stride, int64_t out_offset, void* stream) {
    if (!snap)
        return embed_rows_bwd_det_launch("lipvq_embed_rows_bwd_det_f32", gout, src, idx, pos, stats, ln_w, g_src, g_pos, g_lnw, g_lnb,
                                         workspace, nullptr, N, T, E, src_rows, out_batch_stride, out_t_stride, out_offset, stream);
    if (int rc = embed_drop_check("lipvq_embed_rows_bwd_det_f32", snap, p, N, T, E, out_batch_stride, out_t_stride, out_offset)) return rc;
    const lq_dropout_src drop = lq_dropout_src_make(snap, site, p);
    return embed_rows_bwd_det_launch("lipvq_embed_rows_bwd_det_f32", gout, src, idx, pos, stats, ln_w, g_src, g_pos, g_lnw, g_lnb,
                                     workspace, &drop, N, T, E, src_rows, out_batch_stride, out_t_stride, out_offset, stream);
}

int lipvq_linear_act_f32(const float* x, const float* W, const float* b, float* y, float* pre, int64_t N, int Kin,
                         int E, int act, void* stream) {
    return linear_act_launch("lipvq_linear_act_f32", x, W, b, y, pre, nullptr, 0, 0.0, N, Kin, E, act, stream);
}

int lipvq_linear_act_drop_f32(const float* x, const float* W, const float* b, float* y, float* pre, const int64_t* snap,
                              uint32_t site, double p, int64_t N, int Kin, int E, int act, void* stream) {
    if (int rc = lq_dropout_check("lipvq_linear_act_drop_f32", snap, p, N)) return rc;
    return linear_act_launch("lipvq_linear_act_drop_f32", x, W, b, y, pre, snap, site, p, N, Kin, E, act, stream);
}

int lipvq_linear_f32(const float* x, const float* W, const float* b, float* y, int64_t N, int Kin, int E,
                     void* stream) {
    return lipvq_linear_act_f32(x, W, b, y, nullptr, N, Kin, E, LIPVQ_ACT_NONE, stream);
}

int lipvq_embed_rows_f32(const float* src, const int64_t* idx, const float* pos, const float* ln_w, const float* ln_b,
                         float eps, float* out, float* stats, int64_t N, int T, int E, int64_t src_rows,
                         int64_t out_batch_stride, int64_t out_t_stride, int64_t out_offset, void* stream) {
    return embed_rows_launch("lipvq_embed_rows_f32", src, idx, pos, ln_w, ln_b, eps, out, stats, nullptr, N, T, E, src_rows,
                             out_batch_stride, out_t_stride, out_offset, stream);
}

int lipvq_embed_rows_drop_f32(const float* src, const int64_t* idx, const float* pos, const float* ln_w, const float* ln_b,
                              float eps, float* out, float* stats, const int64_t* snap, uint32_t site, double p, int64_t N, int T,
                              int E, int64_t src_rows, int64_t out_batch_stride, int64_t out_t_stride, int64_t out_offset,
                              void* stream) {
    if (int rc = embed_drop_check("lipvq_embed_rows_drop_f32", snap, p, N, T, E, out_batch_stride, out_t_stride, out_offset)) return rc;
    const lq_dropout_src drop = lq_dropout_src_make(snap, site, p);
    return embed_rows_launch("lipvq_embed_rows_drop_f32", src, idx, pos, ln_w, ln_b, eps, out, stats, &drop, N, T, E, src_rows,
                             out_batch_stride, out_t_stride, out_offset, stream);
}

int lipvq_embed_rows_bwd_f32(const float* gout, const float* src, const int64_t* idx, const float* pos,
                             const float* stats, const float* ln_w, float* g_src, float* g_pos, float* g_lnw,
                             float* g_lnb, int64_t N, int T, int E, int64_t src_rows, int64_t out_batch_stride,
                             int64_t out_t_stride, int64_t out_offset, void* stream) {
    return embed_rows_bwd_launch("lipvq_embed_rows_bwd_f32", gout, src, idx, pos, stats, ln_w, g_src, g_pos, g_lnw, g_lnb, nullptr, N, T,
                                 E, src_rows, out_batch_stride, out_t_stride, out_offset, stream);
}

int lipvq_embed_rows_bwd_drop_f32(const float* gout, const float* src, const int64_t* idx, const float* pos, const float* stats,
                                  const float* ln_w, float* g_src, float* g_pos, float* g_lnw, float* g_lnb, const int64_t* snap,
                                  uint32_t site, double p, int64_t N, int T, int E, int64_t src_rows, int64_t out_batch_stride,
                                  int64_t out_t_stride, int64_t out_offset, void* stream) {
    if (int rc = embed_drop_check("lipvq_embed_rows_bwd_drop_f32", snap, p, N, T, E, out_batch_stride, out_t_stride, out_offset)) return rc;
    const lq_dropout_src drop = lq_dropout_src_make(snap, site, p);
    return embed_rows_bwd_launch("lipvq_embed_rows_bwd_drop_f32", gout, src, idx, pos, stats, ln_w, g_src, g_pos, g_lnw, g_lnb, &drop, N,
                                 T, E, src_rows, out_batch_stride, out_t_stride, out_offset, stream);
}

// Large batches of indexed rows: no atomics on the table or the time embedding (embed_rows_bwd_gv_kernel + the counting-sort
// scatter).  workspace: gv [N][E] floats, the sanitised indices [N], then the scatter's own workspace.
int lipvq_embed_rows_bwd_ws_supported(int64_t N, int T, int E, int64_t src_rows) {
    return N >= 32768 && T >= 1 && T <= 1024 && E >= 4 && (E & 3) == 0 && E <= 1024 && src_rows <= 16384 &&
           lipvq_scatter_add_sorted_supported(N, (int)src_rows, E);
}

size_t lipvq_embed_rows_bwd_workspace_bytes(int64_t N, int T, int E, int64_t src_rows) {
    if (!lipvq_embed_rows_bwd_ws_supported(N, T, E, src_rows)) return 0;
    const size_t gv = ((size_t)N * E * sizeof(float) + 255) & ~(size_t)255, ic = ((size_t)N * sizeof(int64_t) + 255) & ~(size_t)255;
    return gv + ic + lipvq_scatter_add_sorted_workspace_bytes(N, (int)src_rows, E);
}

int lipvq_embed_rows_bwd_ws_f32(const float* gout, const float* src, const int64_t* idx, const float* pos, const float* stats,
                                const float* ln_w, float* g_src, float* g_pos, float* g_lnw, float* g_lnb, void* workspace,
                                int64_t N, int T, int E, int64_t src_rows, int64_t out_batch_stride, int64_t out_t_stride,
                                int64_t out_offset, void* stream) {
    return embed_rows_bwd_ws_launch("lipvq_embed_rows_bwd_ws_f32", gout, src, idx, pos, stats, ln_w, g_src, g_pos, g_lnw, g_lnb,
                                    workspace, nullptr, N, T, E, src_rows, out_batch_stride, out_t_stride, out_offset, stream);
}

int lipvq_embed_rows_bwd_ws_drop_f32(const float* gout, const float* src, const int64_t* idx, const float* pos, const float* stats,
                                     const float* ln_w, float* g_src, float* g_pos, float* g_lnw, float* g_lnb, void* workspace,
                                     const int64_t* snap, uint32_t site, double p, int64_t N, int T, int E, int64_t src_rows,
                                     int64_t out_batch_stride, int64_t out_t_stride, int64_t out_offset, void* stream) {
    if (int rc = embed_drop_check("lipvq_embed_rows_bwd_ws_drop_f32", snap, p, N, T, E, out_batch_stride, out_t_stride, out_offset)) return rc;
    const lq_dropout_src drop = lq_dropout_src_make(snap, site, p);
    return embed_rows_bwd_ws_launch("lipvq_embed_rows_bwd_ws_drop_f32", gout, src, idx, pos, stats, ln_w, g_src, g_pos, g_lnw, g_lnb,
                                    workspace, &drop, N, T, E, src_rows, out_batch_stride, out_t_stride, out_offset, stream);
}

}  // extern "C"
