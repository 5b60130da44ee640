// lipvq_gpt.hip -- what the ICRT transformer backbone (reference robomimic/models/transformers.py:80-439, GPT_Backbone: pre-norm
// blocks of causal multi-head self-attention and a GELU MLP over the [B][3T][E] tensor of ICLInputEmbedding) needs beyond the
// Linears of lipvq_linear_act_f32 / lipvq_wgrad_f32:
//   gpt_attention_kernel        softmax(mask(Q K^T / sqrt(dh))) V for every (batch, head) in one launch, head width 16 / 32 / 64,
//                               sequence 1..128, fp32 MFMA (v_mfma_f32_32x32x2_f32) for both products, exact two-pass softmax
//   gpt_attention_prefix_kernel the same forward for Lq new tokens over P cached prefix keys plus their own (P + Lq <= 128): the
//                               rollout step behind a prompt cache, bit-equal to rows P.. of the kernel above (eval only)
//   gpt_attention_bwd_q/kv      its backward in two passes (probabilities recomputed from the saved log-sum-exp), no atomics
//   gpt_layernorm_kernel        s = a + b, y = LayerNorm(s) w + bias in one pass (pre-norm: the residual stream AND the next
//                               sub-layer's input), rows of E <= 1024 floats
//   gpt_layernorm_bwd_kernel    gradient of s with the stream's own incoming gradient folded in; gw / gb through per-workgroup
//                               partial sums and a fixed-order second pass (bit-reproducible)
//   in-kernel dropout           the attention kernels' mask source is a template parameter (none / keep bytes / Philox draws,
//                               lipvq_rng.h); gpt_layernorm_kernel<true> and gpt_layernorm_bwd_kernel<true> drop the added branch;
//                               each is handed one lq_dropout_src (the state and the keep-field entry points: lipvq_rng.hip)
// ABI: include/lipvq.h ("the transformer backbone", "in-kernel dropout").  Tolerances: tests/test_gpu_gpt.py; the dropout forms
// are held to the keep-byte forms bit for bit: tests/test_gpu_gpt_dropout.py.
//
// Attention layout.  One WAVE owns one (batch, head, 32-query tile); workgroups are single waves and use no LDS, so a step of
// B = 8 sequences spreads its 64 (b, h) pairs over 64 compute units and a large batch fills the chip with independent waves.
// Scores are evaluated TRANSPOSED, S^T = K Q^T: keys are the MFMA A operand (32 keys x 2 d), queries the B operand (2 d x 32
// queries), so the 32x32 result has the QUERY on the lane (col = lane & 31) and 16 keys in the lane's registers: the softmax
// over keys is a loop over registers plus one exchange with lane ^ 32.  The keys are handed to the MFMA in the row order
// gpt_perm, chosen so that register g of lane half hf holds key 2 g + hf of the tile -- exactly the B-operand layout of the
// second product O^T = V^T P^T (k-step g takes keys 2 g and 2 g + 1), which therefore reads the probabilities straight from the
// accumulator registers.  Both products are fmaf chains in ascending k (d for the scores, key for the values).
#include "lipvq_common.h"
#include "lipvq_rng.h"

#define GPT_MAXL 128
#define GPT_MAXE 1024

// row r of a 32x32x2 MFMA result sits in register (r & 3) + 4 (r >> 3) of lane half (r >> 2) & 1; the A operand's row r is
// loaded from tile element gpt_perm(r) = 2 register + half, so that (register g, half hf) carries element 2 g + hf
__device__ __forceinline__ int gpt_perm(int r) { return 2 * ((r & 3) + 4 * (r >> 3)) + ((r >> 2) & 1); }

// elements 2 s + hf (s = 0 .. DH/2 - 1) of one head row: the lane's share of an A or B operand over the head width
template <int DH>
__device__ __forceinline__ void gpt_load_half(const float* __restrict__ row, int hf, float (&r)[DH / 2]) {
#pragma unroll
    for (int t = 0; t < DH / 4; ++t) {
        const float4 v = *reinterpret_cast<const float4*>(row + 4 * t);
        r[2 * t] = hf ? v.y : v.x;
        r[2 * t + 1] = hf ? v.w : v.z;
    }
}

template <int DH>
__device__ __forceinline__ f32x16 gpt_dot(const float (&a)[DH / 2], const float (&b)[DH / 2]) {
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
    return acc;
}

// the transposed [d][row] result tiles of a wave -> rows of DH floats at dst + row stride `ld` (lane = row, 4 consecutive d per store)
template <int DH, int DT>
__device__ __forceinline__ void gpt_store_t(float* __restrict__ dst, const f32x16 (&o)[DT], int hf, float mul) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d0 = 32 * dt + 8 * g4 + 4 * hf;
            if (d0 < DH)
                *reinterpret_cast<float4*>(dst + d0) =
                    make_float4(o[dt][4 * g4] * mul, o[dt][4 * g4 + 1] * mul, o[dt][4 * g4 + 2] * mul, o[dt][4 * g4 + 3] * mul);
        }
}

// Where the attention-probability dropout decisions come from: a compile-time choice of every attention instance.
//   GPT_MASK_NONE    no dropout (eval, p = 0)
//   GPT_MASK_BYTES   keep [B][H][L][L] bytes drawn by the caller (torch's generator)
//   GPT_MASK_PHILOX  drawn here (lipvq_rng.h): row = (b H + h) L + i, col = j -- the layout of the keep bytes -- of `site`
enum { GPT_MASK_NONE = 0, GPT_MASK_BYTES = 1, GPT_MASK_PHILOX = 2 };

// Query on the lane (forward, bwd_q): bit n of the result = the decision for key 32 kt + n of the lane's query `row`; the lane's
// register g holds key 2 g + hf.  The tile's eight draws (columns 32 kt + 4 q .. + 3, q = 0 .. 7) are the same for the two lanes
// of a query, so lane half hf runs draws 4 hf .. 4 hf + 3 and the halves exchange their 16 decisions: four draws per lane and
// tile.  Every lane of the wave must call it (kt is wave-uniform).
__device__ __forceinline__ uint32_t gpt_keep_tile_q(lq_dropout d, uint32_t row, int kt, int hf) {
    uint32_t mine = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) mine |= lq_dropout_keep4(d, row, (uint32_t)(8 * kt + 4 * hf + t)) << (4 * t);
    const uint32_t other = (uint32_t)__shfl_xor((int)mine, 32, 64);
    return hf ? (other | (mine << 16)) : (mine | (other << 16));
}

// Key on the lane (bwd_kv): the lane's key is column j, register g holds query row0 + 2 g + hf (clamped to L - 1 as the loads are).
// The four lanes of a quad share j >> 2 and hf, hence all sixteen draws (one per g); lane q = lane & 3 of the quad runs those of
// g = q, q + 4, q + 8, q + 12 and the quad exchanges the decisions.  Bit g of the result = the decision for (query of g, key j).
__device__ __forceinline__ uint32_t gpt_keep_tile_kv(lq_dropout d, size_t bhL, int qt, int L, int j, int lane, int hf) {
    const int q = lane & 3;
    uint32_t mine = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int i = qt * 32 + 2 * (q + 4 * t) + hf, ic = i < L ? i : L - 1;
        mine |= lq_dropout_keep4(d, (uint32_t)(bhL + ic), (uint32_t)(j >> 2)) << (4 * t);
    }
    uint32_t bits = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint32_t m = (uint32_t)__shfl((int)mine, (lane & ~3) | s, 64);          // lane s of the quad: g = s + 4 t at bits 4 t .. 4 t + 3
#pragma unroll
        for (int t = 0; t < 4; ++t) bits |= ((m >> (4 * t + q)) & 1u) << (s + 4 * t);
    }
    return bits;
}

// (the Philox source arrives as the three words of an lq_dropout_src, not as the struct the other kernels take: with the struct
// the PHILOX instances load their arguments in another grouping and end two SGPRs off the figures on record, LABNOTES)
template <int DH, int NKT, int MASK>
__global__ __launch_bounds__(64) void gpt_attention_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse,
                                                           const unsigned char* __restrict__ keep, float inv_keep,
                                                           const int64_t* __restrict__ snap, uint32_t site, uint32_t thr, int L, int E,
                                                           int H, int causal) {
    constexpr int DT = DH > 32 ? DH / 32 : 1;
    const int lane = threadIdx.x, c = lane & 31, hf = lane >> 5;
    const int qt = blockIdx.x % NKT;
    const size_t bh = blockIdx.x / NKT;
    const int h = (int)(bh % H);
    const size_t b = bh / H;
    const float* __restrict__ base = qkv + b * (size_t)L * 3 * E + (size_t)h * DH;
    const int i = qt * 32 + c, ic = i < L ? i : L - 1;
    const float scale = 1.0f / lq_sqrt((float)DH);
    const int kt_end = causal ? qt + 1 : NKT;                       // (wave-uniform)
    float q[DH / 2];
    gpt_load_half<DH>(base + (size_t)ic * 3 * E, hf, q);
    f32x16 s[NKT];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        if (kt < kt_end) {
            const int jr = kt * 32 + gpt_perm(c), jrc = jr < L ? jr : L - 1;
            float k[DH / 2];
            gpt_load_half<DH>(base + (size_t)jrc * 3 * E + E, hf, k);
            const f32x16 acc = gpt_dot<DH>(k, q);
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int j = kt * 32 + 2 * g + hf;
                const bool ok = j < L && (!causal || j <= i);
                const float v = ok ? acc[g] * scale : -INFINITY;
                s[kt][g] = v;
                m = fmaxf(m, v);
            }
        }
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));                            // (key 0 is open to every query: m is finite)
    float l = 0.0f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        if (kt < kt_end) {
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const float e = lq_expf(s[kt][g] - m);             // (masked: exp(-inf) = 0)
                s[kt][g] = e;
                l += e;
            }
        }
    }
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    f32x16 o[DT] = {};
    lq_dropout dr = {};
    if constexpr (MASK == GPT_MASK_PHILOX) dr = lq_dropout_load(lq_dropout_src{snap, site, thr, inv_keep});
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        if (kt < kt_end) {
            uint32_t kb = 0;
            if constexpr (MASK == GPT_MASK_PHILOX) kb = gpt_keep_tile_q(dr, (uint32_t)(bh * L + ic), kt, hf);
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int j = kt * 32 + 2 * g + hf, jc = j < L ? j : L - 1;
                float p = s[kt][g] * inv;
                if constexpr (MASK == GPT_MASK_BYTES) p = keep[(bh * L + ic) * L + jc] ? p * inv_keep : 0.0f;
                if constexpr (MASK == GPT_MASK_PHILOX) p = ((kb >> (2 * g + hf)) & 1u) ? p * inv_keep : 0.0f;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const float a = (DH >= 32 || c < DH) ? base[(size_t)jc * 3 * E + 2 * E + 32 * dt + c] : 0.0f;
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p, o[dt], 0, 0, 0);
                }
            }
        }
    }
    if (i < L) {
        gpt_store_t<DH, DT>(out + (b * L + i) * (size_t)E + (size_t)h * DH, o, hf, 1.0f);
        // (l >= 1: the row maximum contributes exp(0); a NaN l -- a score that is a NaN or +inf -- stays a NaN: lq_logf_ge1 works on
        // the bits and would return a number)
        if (hf == 0) lse[bh * L + i] = m + (l == l ? lq_logf_ge1(l) : l);
    }
}

// Causal attention of Lq NEW tokens over P cached prefix keys plus their own: the rollout step of a prompted policy, whose
// prompt's keys and values are constants of the evaluation.  prefix [Bp][P][3E] is the qkv tensor of a prefill, read in place
// (K at + E, V at + 2 E; pstride = 0 shares one prompt among all sequences); qkv [B][Lq][3E] and out [B][Lq][E] hold the new
// tokens alone.  One wave per (b, h, 32-query tile of the new tokens).  Key tiles are tiles of the CONCATENATED key index
// j = 0 .. P + Lq - 1 (j < P: prefix row j, else new row j - P), so query iq meets its keys in the tiles, registers and lane
// halves in which gpt_attention_kernel hands them to row P + iq of the concatenated tensor, and both products are the same
// chains: every output row carries that kernel's bits.  (A wave may run more trailing tiles for a row than that kernel does:
// they are masked whole, add exp(-inf) = 0 to the sum and a 0 * v product to the value chain, and change nothing.)
template <int DH, int NKT>
__global__ __launch_bounds__(64) void gpt_attention_prefix_kernel(const float* __restrict__ prefix, const float* __restrict__ qkv,
                                                                  float* __restrict__ out, size_t pstride, int P, int Lq, int E, int H,
                                                                  int NQT) {
    constexpr int DT = DH > 32 ? DH / 32 : 1;
    const int lane = threadIdx.x, c = lane & 31, hf = lane >> 5;
    const int qt = blockIdx.x % NQT;
    const size_t bh = blockIdx.x / NQT;
    const int h = (int)(bh % H);
    const size_t b = bh / H;
    const int L = P + Lq;
    const float* __restrict__ pbase = prefix + b * pstride + (size_t)h * DH;             // (read for j < P only: may be NULL when P = 0)
    const float* __restrict__ nbase = qkv + b * (size_t)Lq * 3 * E + (size_t)h * DH;
    const int i = qt * 32 + c, ic = i < Lq ? i : Lq - 1;
    const float scale = 1.0f / lq_sqrt((float)DH);
    const int q_end = Lq < 32 * (qt + 1) ? Lq : 32 * (qt + 1);
    const int kt_end = (P + q_end + 31) / 32;                       // (wave-uniform, <= NKT)
    float q[DH / 2];
    gpt_load_half<DH>(nbase + (size_t)ic * 3 * E, hf, q);
    f32x16 s[NKT];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        if (kt < kt_end) {
            const int jr = kt * 32 + gpt_perm(c), jrc = jr < L ? jr : L - 1;
            const float* __restrict__ krow = jrc < P ? pbase + (size_t)jrc * 3 * E : nbase + (size_t)(jrc - P) * 3 * E;
            float k[DH / 2];
            gpt_load_half<DH>(krow + E, hf, k);
            const f32x16 acc = gpt_dot<DH>(k, q);
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int j = kt * 32 + 2 * g + hf;
                const bool ok = j < L && j <= P + i;
                const float v = ok ? acc[g] * scale : -INFINITY;
                s[kt][g] = v;
                m = fmaxf(m, v);
            }
        }
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));                            // (key 0 is open to every query: m is finite)
    float l = 0.0f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        if (kt < kt_end) {
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const float e = lq_expf(s[kt][g] - m);             // (masked: exp(-inf) = 0)
                s[kt][g] = e;
                l += e;
            }
        }
    }
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    f32x16 o[DT] = {};
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        if (kt < kt_end) {
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int j = kt * 32 + 2 * g + hf, jc = j < L ? j : L - 1;
                const float* __restrict__ vrow = jc < P ? pbase + (size_t)jc * 3 * E : nbase + (size_t)(jc - P) * 3 * E;
                const float p = s[kt][g] * inv;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const float a = (DH >= 32 || c < DH) ? vrow[2 * E + 32 * dt + c] : 0.0f;
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p, o[dt], 0, 0, 0);
                }
            }
        }
    }
    if (i < Lq) gpt_store_t<DH, DT>(out + (b * Lq + i) * (size_t)E + (size_t)h * DH, o, hf, 1.0f);
}

// Backward.  delta[i] = sum_d dO[i][d] O[i][d];  P_ij = exp(s_ij - lse_i);  dP_ij = (keep_ij / keep_prob) dO_i . V_j;
// dS_ij = P_ij (dP_ij - delta_i);  dQ_i = scale sum_j dS_ij K_j;  dK_j = scale sum_i dS_ij Q_i;  dV_j = sum_i (keep_ij / keep_prob) P_ij dO_i.
// gpt_attention_bwd_q: wave = (b, h, 32 queries), loops over key tiles -> dQ, delta.  gpt_attention_bwd_kv: wave = (b, h, 32 keys),
// loops over query tiles -> dK, dV.  The same transposed-score layout as the forward: the lane owns the row the wave reduces INTO.
// The two close a dropped position differently -- bwd_q by a select on keep, bwd_kv by the factor kp = 0 -- and so differ where
// dO . V is not finite at a dropped position (LABNOTES, "GPT attention: dispatch and zeroing shared"): do not merge the two treatments.
template <int DH, int MASK>
__global__ __launch_bounds__(64) void gpt_attention_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                                 const float* __restrict__ go, const float* __restrict__ lse,
                                                                 float* __restrict__ gqkv, float* __restrict__ delta,
                                                                 const unsigned char* __restrict__ keep, float inv_keep,
                                                                 lq_dropout_src src, int L, int E, int H, int causal, int NT) {
    constexpr int DT = DH > 32 ? DH / 32 : 1;
    const int lane = threadIdx.x, c = lane & 31, hf = lane >> 5;
    const int qt = blockIdx.x % NT;
    const size_t bh = blockIdx.x / NT;
    const int h = (int)(bh % H);
    const size_t b = bh / H;
    const float* __restrict__ base = qkv + b * (size_t)L * 3 * E + (size_t)h * DH;
    const int i = qt * 32 + c, ic = i < L ? i : L - 1;
    const float scale = 1.0f / lq_sqrt((float)DH);
    const int kt_end = causal ? qt + 1 : NT;
    float q[DH / 2], gor[DH / 2];
    gpt_load_half<DH>(base + (size_t)ic * 3 * E, hf, q);
    gpt_load_half<DH>(go + (b * L + ic) * (size_t)E + (size_t)h * DH, hf, gor);
    float dl = 0.0f;
    {
        float orow[DH / 2];
        gpt_load_half<DH>(o + (b * L + ic) * (size_t)E + (size_t)h * DH, hf, orow);
#pragma unroll
        for (int t = 0; t < DH / 2; ++t) dl = lq_fma(gor[t], orow[t], dl);
    }
    dl += __shfl_xor(dl, 32, 64);
    const float ls = lse[bh * L + ic];
    if (hf == 0 && i < L) delta[bh * L + i] = dl;
    f32x16 dq[DT] = {};
    lq_dropout dr = {};
    if constexpr (MASK == GPT_MASK_PHILOX) dr = lq_dropout_load(src);
#pragma unroll 1
    for (int kt = 0; kt < kt_end; ++kt) {
        const int jr = kt * 32 + gpt_perm(c), jrc = jr < L ? jr : L - 1;
        uint32_t kb = 0;
        if constexpr (MASK == GPT_MASK_PHILOX) kb = gpt_keep_tile_q(dr, (uint32_t)(bh * L + ic), kt, hf);
        f32x16 sa, pa;
        {
            float k[DH / 2];
            gpt_load_half<DH>(base + (size_t)jrc * 3 * E + E, hf, k);
            sa = gpt_dot<DH>(k, q);
        }
        {
            float v[DH / 2];
            gpt_load_half<DH>(base + (size_t)jrc * 3 * E + 2 * E, hf, v);
            pa = gpt_dot<DH>(v, gor);
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int j = kt * 32 + 2 * g + hf, jc = j < L ? j : L - 1;
            const bool ok = j < L && (!causal || j <= i);
            const float p = ok ? lq_expf(sa[g] * scale - ls) : 0.0f;
            float dp = pa[g];
            if constexpr (MASK == GPT_MASK_BYTES) dp = keep[(bh * L + ic) * L + jc] ? dp * inv_keep : 0.0f;
            if constexpr (MASK == GPT_MASK_PHILOX) dp = ((kb >> (2 * g + hf)) & 1u) ? dp * inv_keep : 0.0f;
            sa[g] = ok ? p * (dp - dl) : 0.0f;                      // (a select: 0 * (a NaN dp or delta) would be a NaN)
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int j = kt * 32 + 2 * g + hf, jc = j < L ? j : L - 1;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const float a = (DH >= 32 || c < DH) ? base[(size_t)jc * 3 * E + E + 32 * dt + c] : 0.0f;
                dq[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sa[g], dq[dt], 0, 0, 0);
            }
        }
    }
    if (i < L) gpt_store_t<DH, DT>(gqkv + (b * L + i) * (size_t)3 * E + (size_t)h * DH, dq, hf, scale);
}

template <int DH, int MASK>
__global__ __launch_bounds__(64) void gpt_attention_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ go,
                                                                  const float* __restrict__ lse, const float* __restrict__ delta,
                                                                  float* __restrict__ gqkv, const unsigned char* __restrict__ keep,
                                                                  float inv_keep, lq_dropout_src src, int L, int E, int H, int causal,
                                                                  int NT) {
    constexpr int DT = DH > 32 ? DH / 32 : 1;
    const int lane = threadIdx.x, c = lane & 31, hf = lane >> 5;
    const int kt = blockIdx.x % NT;
    const size_t bh = blockIdx.x / NT;
    const int h = (int)(bh % H);
    const size_t b = bh / H;
    const float* __restrict__ base = qkv + b * (size_t)L * 3 * E + (size_t)h * DH;
    const float* __restrict__ gbase = go + b * (size_t)L * E + (size_t)h * DH;
    const int j = kt * 32 + c, jc = j < L ? j : L - 1;
    const float scale = 1.0f / lq_sqrt((float)DH);
    float k[DH / 2], v[DH / 2];
    gpt_load_half<DH>(base + (size_t)jc * 3 * E + E, hf, k);
    gpt_load_half<DH>(base + (size_t)jc * 3 * E + 2 * E, hf, v);
    f32x16 dk[DT], dv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { dk[dt] = f32x16{}; dv[dt] = f32x16{}; }
    lq_dropout dr = {};
    if constexpr (MASK == GPT_MASK_PHILOX) dr = lq_dropout_load(src);
#pragma unroll 1
    for (int qt = causal ? kt : 0; qt < NT; ++qt) {
        const int ir = qt * 32 + gpt_perm(c), irc = ir < L ? ir : L - 1;
        uint32_t kb = 0;
        if constexpr (MASK == GPT_MASK_PHILOX) kb = gpt_keep_tile_kv(dr, bh * L, qt, L, j, lane, hf);
        f32x16 sa, pa;
        {
            float q[DH / 2];
            gpt_load_half<DH>(base + (size_t)irc * 3 * E, hf, q);
            sa = gpt_dot<DH>(q, k);
        }
        {
            float g[DH / 2];
            gpt_load_half<DH>(gbase + (size_t)irc * E, hf, g);
            pa = gpt_dot<DH>(g, v);
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int i = qt * 32 + 2 * g + hf, ic = i < L ? i : L - 1;
            const bool ok = i < L && j < L && (!causal || j <= i);
            const float p = ok ? lq_expf(sa[g] * scale - lse[bh * L + ic]) : 0.0f;
            float kp = 1.0f;
            if constexpr (MASK == GPT_MASK_BYTES) kp = keep[(bh * L + ic) * L + jc] ? inv_keep : 0.0f;
            if constexpr (MASK == GPT_MASK_PHILOX) kp = ((kb >> g) & 1u) ? inv_keep : 0.0f;
            // a closed position is closed by a select: 0 * (the NaN delta of a query row that is not finite) would put that row into
            // the gradient of every key behind it
            sa[g] = ok ? p * (pa[g] * kp - delta[bh * L + ic]) : 0.0f;
            pa[g] = p * kp;
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int i = qt * 32 + 2 * g + hf, ic = i < L ? i : L - 1;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const bool col = DH >= 32 || c < DH;
                const float ag = col ? gbase[(size_t)ic * E + 32 * dt + c] : 0.0f;
                const float aq = col ? base[(size_t)ic * 3 * E + 32 * dt + c] : 0.0f;
                dv[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ag, pa[g], dv[dt], 0, 0, 0);
                dk[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq, sa[g], dk[dt], 0, 0, 0);
            }
        }
    }
    if (j < L) {
        float* __restrict__ dst = gqkv + (b * L + j) * (size_t)3 * E + (size_t)h * DH;
        gpt_store_t<DH, DT>(dst + E, dk, hf, scale);
        gpt_store_t<DH, DT>(dst + 2 * E, dv, hf, 1.0f);
    }
}

static int gpt_attention_args(const char* what, int64_t B, int L, int E, int H, const void* keep, float keep_prob, bool* empty) {
    if (B < 0 || L < 0 || E <= 0 || H <= 0 || E % H != 0) return fail(LIPVQ_EINVAL, "%s: B=%lld L=%d E=%d H=%d", what, (long long)B, L, E, H);
    const int dh = E / H;
    if (dh != 16 && dh != 32 && dh != 64) return fail(LIPVQ_EUNSUPPORTED, "%s: head width E/H=%d (16, 32 or 64)", what, dh);
    if (L > GPT_MAXL) return fail(LIPVQ_EUNSUPPORTED, "%s: sequence length L=%d (1..%d)", what, L, GPT_MAXL);
    if (keep && !(keep_prob > 0.0f)) return fail(LIPVQ_EINVAL, "%s: keep_prob=%g with a keep mask", what, (double)keep_prob);
    *empty = B == 0 || L == 0;
    if (!*empty && B * H * ((L + 31) / 32) > 0x7fffffffLL) return fail(LIPVQ_EUNSUPPORTED, "%s: B=%lld is too many (b, h) pairs for one launch", what, (long long)B);
    return 0;
}

// the instances: f(DH) for the head width, f(DH, NKT) for a forward over nkt = 1 .. 4 key tiles (what gpt_attention_args let through)
template <typename F>
static void gpt_for_width(int dh, F&& f) { lq_dispatch<16, 32, 64>(dh, f); }
template <typename F>
static void gpt_for_forward(int dh, int nkt, F&& f) {
    gpt_for_width(dh, [&](auto d) { lq_dispatch<1, 2, 3, 4>(nkt, [&](auto n) { f(d, n); }); });
}

// the mask source of a launch: src.snap -> PHILOX (inv_keep is src's), keep -> BYTES (inv_keep = 1 / keep_prob), neither -> NONE
static int gpt_mask_of(const unsigned char* keep, lq_dropout_src src) { return src.snap ? GPT_MASK_PHILOX : keep ? GPT_MASK_BYTES : GPT_MASK_NONE; }

// one forward launch for the three mask sources
static int gpt_attention_launch(const char* what, const float* qkv, float* out, float* lse, const unsigned char* keep, float inv_keep,
                                lq_dropout_src src, int64_t B, int L, int E, int H, int causal, void* stream) {
    if (!qkv || !out || !lse) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if ((((uintptr_t)qkv | (uintptr_t)out) & 15) != 0) return fail(LIPVQ_EINVAL, "%s: qkv / out must be 16-byte aligned", what);
    const int NT = (L + 31) / 32;
    lq_dispatch<GPT_MASK_NONE, GPT_MASK_BYTES, GPT_MASK_PHILOX>(gpt_mask_of(keep, src), [&](auto m) {
        gpt_for_forward(E / H, NT, [&](auto d, auto n) {
            hipLaunchKernelGGL((gpt_attention_kernel<d(), n(), decltype(m)::value>), dim3((unsigned)(B * H * NT)), dim3(64), 0, (hipStream_t)stream, qkv,
                               out, lse, keep, inv_keep, src.snap, src.site, src.thr, L, E, H, causal);
        });
    });
    return check_launch(what);
}

extern "C" int lipvq_gpt_attention_f32(const float* qkv, float* out, float* lse, const unsigned char* keep, float keep_prob,
                                       int64_t B, int L, int E, int H, int causal, void* stream) {
    bool empty = false;
    if (int rc = gpt_attention_args("gpt_attention", B, L, E, H, keep, keep_prob, &empty)) return rc;
    if (empty) return 0;
    return gpt_attention_launch("gpt_attention", qkv, out, lse, keep, keep ? 1.0f / keep_prob : 1.0f, lq_dropout_src{}, B, L, E, H, causal,
                                stream);
}

extern "C" int lipvq_gpt_attention_drop_f32(const float* qkv, float* out, float* lse, const int64_t* snap, uint32_t site, double p,
                                            int64_t B, int L, int E, int H, int causal, void* stream) {
    bool empty = false;
    if (int rc = gpt_attention_args("gpt_attention_drop", B, L, E, H, nullptr, 1.0f, &empty)) return rc;
    if (int rc = lq_dropout_check("gpt_attention_drop", snap, p, B * H * (int64_t)L)) return rc;
    if (empty) return 0;
    const lq_dropout_src src = lq_dropout_src_make(snap, site, p);
    return gpt_attention_launch("gpt_attention_drop", qkv, out, lse, nullptr, src.inv_keep, src, B, L, E, H, causal, stream);
}

extern "C" int lipvq_gpt_attention_prefix_f32(const float* prefix_qkv, const float* qkv, float* out, int64_t B, int64_t Bp, int P,
                                              int Lq, int E, int H, void* stream) {
    if (P < 0 || Lq < 0) return fail(LIPVQ_EINVAL, "gpt_attention_prefix: P=%d Lq=%d", P, Lq);
    if (P + (int64_t)Lq > GPT_MAXL)
        return fail(LIPVQ_EUNSUPPORTED, "gpt_attention_prefix: P + Lq = %d + %d keys (<= %d)", P, Lq, GPT_MAXL);
    bool empty = false;
    if (int rc = gpt_attention_args("gpt_attention_prefix", B, Lq, E, H, nullptr, 1.0f, &empty)) return rc;
    if (Bp != B && Bp != 1)
        return fail(LIPVQ_EINVAL, "gpt_attention_prefix: Bp=%lld prompts for B=%lld sequences (B, or 1 shared by all)", (long long)Bp, (long long)B);
    if (empty) return 0;
    if (!qkv || !out || (P > 0 && !prefix_qkv)) return fail(LIPVQ_EINVAL, "gpt_attention_prefix: null pointer");
    if ((((uintptr_t)prefix_qkv | (uintptr_t)qkv | (uintptr_t)out) & 15) != 0)
        return fail(LIPVQ_EINVAL, "gpt_attention_prefix: prefix_qkv / qkv / out must be 16-byte aligned");
    const int NQT = (Lq + 31) / 32;
    const size_t pstride = Bp == 1 ? 0 : (size_t)P * 3 * E;
    gpt_for_forward(E / H, (P + Lq + 31) / 32, [&](auto d, auto n) {
        hipLaunchKernelGGL((gpt_attention_prefix_kernel<d(), n()>), dim3((unsigned)(B * H * NQT)), dim3(64), 0, (hipStream_t)stream,
                           prefix_qkv, qkv, out, pstride, P, Lq, E, H, NQT);
    });
    return check_launch("gpt_attention_prefix");
}

static int gpt_attention_bwd_launch(const char* what, const float* qkv, const float* out, const float* gout, const float* lse,
                                    float* gqkv, float* delta, const unsigned char* keep, float ik, lq_dropout_src src, int64_t B,
                                    int L, int E, int H, int causal, void* stream) {
    if (!qkv || !out || !gout || !lse || !gqkv || !delta) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if ((((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)gout | (uintptr_t)gqkv) & 15) != 0)
        return fail(LIPVQ_EINVAL, "%s: qkv / out / gout / gqkv must be 16-byte aligned", what);
    const int NT = (L + 31) / 32;
    const dim3 grid((unsigned)(B * H * NT));
    lq_dispatch<GPT_MASK_NONE, GPT_MASK_BYTES, GPT_MASK_PHILOX>(gpt_mask_of(keep, src), [&](auto m) {
        gpt_for_width(E / H, [&](auto d) {
            hipLaunchKernelGGL((gpt_attention_bwd_q_kernel<d(), decltype(m)::value>), grid, dim3(64), 0, (hipStream_t)stream, qkv, out, gout,
                               lse, gqkv, delta, keep, ik, src, L, E, H, causal, NT);
            hipLaunchKernelGGL((gpt_attention_bwd_kv_kernel<d(), decltype(m)::value>), grid, dim3(64), 0, (hipStream_t)stream, qkv, gout, lse,
                               delta, gqkv, keep, ik, src, L, E, H, causal, NT);
        });
    });
    return check_launch(what);
}

extern "C" int lipvq_gpt_attention_bwd_f32(const float* qkv, const float* out, const float* gout, const float* lse, float* gqkv,
                                           float* delta, const unsigned char* keep, float keep_prob, int64_t B, int L, int E, int H,
                                           int causal, void* stream) {
    bool empty = false;
    if (int rc = gpt_attention_args("gpt_attention_bwd", B, L, E, H, keep, keep_prob, &empty)) return rc;
    if (empty) return 0;
    return gpt_attention_bwd_launch("gpt_attention_bwd", qkv, out, gout, lse, gqkv, delta, keep, keep ? 1.0f / keep_prob : 1.0f,
                                    lq_dropout_src{}, B, L, E, H, causal, stream);
}

extern "C" int lipvq_gpt_attention_bwd_drop_f32(const float* qkv, const float* out, const float* gout, const float* lse, float* gqkv,
                                                float* delta, const int64_t* snap, uint32_t site, double p, int64_t B, int L, int E,
                                                int H, int causal, void* stream) {
    bool empty = false;
    if (int rc = gpt_attention_args("gpt_attention_bwd_drop", B, L, E, H, nullptr, 1.0f, &empty)) return rc;
    if (int rc = lq_dropout_check("gpt_attention_bwd_drop", snap, p, B * H * (int64_t)L)) return rc;
    if (empty) return 0;
    const lq_dropout_src src = lq_dropout_src_make(snap, site, p);
    return gpt_attention_bwd_launch("gpt_attention_bwd_drop", qkv, out, gout, lse, gqkv, delta, nullptr, src.inv_keep, src, B, L, E, H,
                                    causal, stream);
}

// ---------------------------------------------------------------------------------------------------
// s = a + b;  y = LayerNorm(s) * w + bias over rows of E <= 1024 floats, E % 4 == 0: one wave per row, up to four float4 per
// lane, two-pass moments in registers (the mean in two steps, see the kernel).  With s_out == NULL this is the post-norm residual of the default action branch.
// ---------------------------------------------------------------------------------------------------
// DROP: s = a + drop(b), the branch's dropout decided here -- field (row, col = e) of `site`; a lane's float4 is columns
// 4 e4 .. 4 e4 + 3 of its row, i.e. exactly one draw.  A dropped element is b * 0 and a kept one b * inv_keep, the product torch's
// dropout forms (a NaN or an infinity of the branch stays one either way).
template <bool DROP>
__global__ __launch_bounds__(256) void gpt_layernorm_kernel(const float4* __restrict__ a, const float4* __restrict__ b,
                                                            const float4* __restrict__ w, const float4* __restrict__ bias, float eps,
                                                            float4* __restrict__ s_out, float4* __restrict__ y, float4* __restrict__ xhat,
                                                            float* __restrict__ rstd, lq_dropout_src src, int64_t N, int E) {
    const int lane = threadIdx.x & 63, E4 = E >> 2;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const size_t r0 = (size_t)row * E4;
    lq_dropout dr = {};
    if constexpr (DROP) dr = lq_dropout_load(src);
    const float inv_keep = dr.inv_keep;
    float4 x[4];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = lane + 64 * i;
        x[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (e < E4) {
            x[i] = a[r0 + e];
            if constexpr (DROP) {
                const float4 t = b[r0 + e];
                const uint32_t kb = lq_dropout_keep4(dr, (uint32_t)row, (uint32_t)e);
                x[i].x += t.x * ((kb & 1u) ? inv_keep : 0.0f); x[i].y += t.y * ((kb & 2u) ? inv_keep : 0.0f);
                x[i].z += t.z * ((kb & 4u) ? inv_keep : 0.0f); x[i].w += t.w * ((kb & 8u) ? inv_keep : 0.0f);
            } else if (b) { const float4 t = b[r0 + e]; x[i].x += t.x; x[i].y += t.y; x[i].z += t.z; x[i].w += t.w; }
            if (s_out) s_out[r0 + e] = x[i];
            s += (x[i].x + x[i].y) + (x[i].z + x[i].w);
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
    // Centre twice.  The fp32 sum of a row around 1000 is off by ulps of E * 1000, its mean by ~1e-4: as large as the row's own
    // spread allows unnoticed.  x - mean is exact for values within a factor 2 of the mean, so the mean of the centred values is
    // that error, to fp32 accuracy at ITS size, and comes off too (0 for a row the first mean already centres).
    const float mean = s / (float)E;
    float r = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (lane + 64 * i < E4) {
            x[i].x -= mean; x[i].y -= mean; x[i].z -= mean; x[i].w -= mean;
            r += (x[i].x + x[i].y) + (x[i].z + x[i].w);
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) r += __shfl_xor(r, off, 64);
    const float rest = r / (float)E;
    float v = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (lane + 64 * i < E4) {
            x[i].x -= rest; x[i].y -= rest; x[i].z -= rest; x[i].w -= rest;
            v = lq_fma(x[i].x, x[i].x, v); v = lq_fma(x[i].y, x[i].y, v); v = lq_fma(x[i].z, x[i].z, v); v = lq_fma(x[i].w, x[i].w, v);
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    const float rs = 1.0f / lq_sqrt(v / (float)E + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = lane + 64 * i;
        if (e < E4) {
            const float4 xh = make_float4(x[i].x * rs, x[i].y * rs, x[i].z * rs, x[i].w * rs);
            if (xhat) xhat[r0 + e] = xh;
            const float4 ww = w[e], bb = bias[e];
            y[r0 + e] = make_float4(lq_fma(xh.x, ww.x, bb.x), lq_fma(xh.y, ww.y, bb.y), lq_fma(xh.z, ww.z, bb.z), lq_fma(xh.w, ww.w, bb.w));
        }
    }
    if (rstd && lane == 0) rstd[row] = rs;
}

static int gpt_layernorm_launch(const char* what, const float* a, const float* b, const float* w, const float* bias, float eps, float* s,
                                float* y, float* xhat, float* rstd, lq_dropout_src src, int64_t N, int E, void* stream) {
    if (N < 0 || E <= 0) return fail(LIPVQ_EINVAL, "%s: N=%lld E=%d", what, (long long)N, E);
    if (E > GPT_MAXE || (E & 3) != 0) return fail(LIPVQ_EUNSUPPORTED, "%s: E=%d (a multiple of 4, <= %d)", what, E, GPT_MAXE);
    if (N == 0) return 0;
    if (!a || !w || !bias || !y || (src.snap && !b)) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)s | (uintptr_t)y | (uintptr_t)xhat) & 15) != 0)
        return fail(LIPVQ_EINVAL, "%s: pointers must be 16-byte aligned", what);
    if ((N + 3) / 4 > 0x7fffffffLL) return fail(LIPVQ_EUNSUPPORTED, "%s: N=%lld", what, (long long)N);
    const dim3 grid((unsigned)((N + 3) / 4));
    if (src.snap)
        hipLaunchKernelGGL(gpt_layernorm_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const float4*)a, (const float4*)b,
                           (const float4*)w, (const float4*)bias, eps, (float4*)s, (float4*)y, (float4*)xhat, rstd, src, N, E);
    else
        hipLaunchKernelGGL(gpt_layernorm_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const float4*)a, (const float4*)b,
                           (const float4*)w, (const float4*)bias, eps, (float4*)s, (float4*)y, (float4*)xhat, rstd, src, N, E);
    return check_launch(what);
}

extern "C" int lipvq_gpt_layernorm_f32(const float* a, const float* b, const float* w, const float* bias, float eps, float* s,
                                       float* y, float* xhat, float* rstd, int64_t N, int E, void* stream) {
    return gpt_layernorm_launch("gpt_layernorm", a, b, w, bias, eps, s, y, xhat, rstd, lq_dropout_src{}, N, E, stream);
}

extern "C" int lipvq_gpt_layernorm_drop_f32(const float* a, const float* b, const float* w, const float* bias, float eps,
                                            const int64_t* snap, uint32_t site, double p, float* s, float* y, float* xhat, float* rstd,
                                            int64_t N, int E, void* stream) {
    if (int rc = lq_dropout_check("gpt_layernorm_drop", snap, p, N)) return rc;
    return gpt_layernorm_launch("gpt_layernorm_drop", a, b, w, bias, eps, s, y, xhat, rstd, lq_dropout_src_make(snap, site, p), N, E, stream);
}

// gs = rstd (g w - mean(g w) - xhat mean(g w xhat)) + gres;  gw = sum_rows g xhat;  gb = sum_rows g.
// Pass 1: a workgroup takes rows_per_block rows (wave w the rows w, w + 4, ...), keeps its column sums in registers, adds the four
// waves in LDS in wave order and writes ONE partial row pair to part [nblk][2][E].  Pass 2 adds the partials of a column in
// block order (four interleaved chains, then ((0 + 1) + 2) + 3).  No atomics: the same bits every run.
#define GPT_LN_MAXBLK 512
static inline int gpt_ln_rows_per_block(int64_t N) {
    int64_t rpb = (N + GPT_LN_MAXBLK - 1) / GPT_LN_MAXBLK;
    rpb = (rpb + 3) / 4 * 4;
    return (int)(rpb < 4 ? 4 : rpb);
}

// DROP: the forward was s = a + drop(b); gs is the gradient of a, and gbr = gs * (kept ? inv_keep : 0), the branch's, is written
// by the same pass from the regenerated decisions of `site` (the field gpt_layernorm_kernel<true> drew).
template <bool DROP>
__global__ __launch_bounds__(256) void gpt_layernorm_bwd_kernel(const float4* __restrict__ gy, const float4* __restrict__ xhat,
                                                                const float* __restrict__ rstd, const float4* __restrict__ w,
                                                                const float4* __restrict__ gres, float4* __restrict__ gs,
                                                                float4* __restrict__ gbr, float* __restrict__ part, lq_dropout_src src,
                                                                int64_t N, int E, int rows_per_block) {
    __shared__ float s_gw[4][GPT_MAXE], s_gb[4][GPT_MAXE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, E4 = E >> 2;
    lq_dropout dr = {};
    if constexpr (DROP) dr = lq_dropout_load(src);
    const float inv_keep = dr.inv_keep;
    float4 pgw[4], pgb[4], ww[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        pgw[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        pgb[i] = pgw[i];
        ww[i] = lane + 64 * i < E4 ? w[lane + 64 * i] : pgw[i];
    }
    const int64_t rbeg = (int64_t)blockIdx.x * rows_per_block;
    int64_t rend = rbeg + rows_per_block;
    if (rend > N) rend = N;
    for (int64_t row = rbeg + wv; row < rend; row += 4) {
        const size_t r0 = (size_t)row * E4;
        float4 g[4], xh[4];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = lane + 64 * i;
            g[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            xh[i] = g[i];
            if (e < E4) {
                g[i] = gy[r0 + e];
                xh[i] = xhat[r0 + e];
                pgw[i].x = lq_fma(g[i].x, xh[i].x, pgw[i].x); pgw[i].y = lq_fma(g[i].y, xh[i].y, pgw[i].y);
                pgw[i].z = lq_fma(g[i].z, xh[i].z, pgw[i].z); pgw[i].w = lq_fma(g[i].w, xh[i].w, pgw[i].w);
                pgb[i].x += g[i].x; pgb[i].y += g[i].y; pgb[i].z += g[i].z; pgb[i].w += g[i].w;
                g[i].x *= ww[i].x; g[i].y *= ww[i].y; g[i].z *= ww[i].z; g[i].w *= ww[i].w;
                s1 += (g[i].x + g[i].y) + (g[i].z + g[i].w);
                s2 = lq_fma(g[i].x, xh[i].x, s2); s2 = lq_fma(g[i].y, xh[i].y, s2);
                s2 = lq_fma(g[i].z, xh[i].z, s2); s2 = lq_fma(g[i].w, xh[i].w, s2);
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { s1 += __shfl_xor(s1, off, 64); s2 += __shfl_xor(s2, off, 64); }
        const float m1 = s1 / (float)E, m2 = s2 / (float)E, rs = rstd[row];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = lane + 64 * i;
            if (e < E4) {
                float4 r = make_float4(rs * (g[i].x - m1 - xh[i].x * m2), rs * (g[i].y - m1 - xh[i].y * m2),
                                       rs * (g[i].z - m1 - xh[i].z * m2), rs * (g[i].w - m1 - xh[i].w * m2));
                if (gres) { const float4 t = gres[r0 + e]; r.x += t.x; r.y += t.y; r.z += t.z; r.w += t.w; }
                gs[r0 + e] = r;
                if constexpr (DROP) {
                    const uint32_t kb = lq_dropout_keep4(dr, (uint32_t)row, (uint32_t)e);
                    gbr[r0 + e] = make_float4(r.x * ((kb & 1u) ? inv_keep : 0.0f), r.y * ((kb & 2u) ? inv_keep : 0.0f),
                                              r.z * ((kb & 4u) ? inv_keep : 0.0f), r.w * ((kb & 8u) ? inv_keep : 0.0f));
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = 4 * (lane + 64 * i);
        if (e < E) {
            s_gw[wv][e] = pgw[i].x; s_gw[wv][e + 1] = pgw[i].y; s_gw[wv][e + 2] = pgw[i].z; s_gw[wv][e + 3] = pgw[i].w;
            s_gb[wv][e] = pgb[i].x; s_gb[wv][e + 1] = pgb[i].y; s_gb[wv][e + 2] = pgb[i].z; s_gb[wv][e + 3] = pgb[i].w;
        }
    }
    __syncthreads();
    float* __restrict__ p = part + (size_t)blockIdx.x * 2 * E;
    for (int e = threadIdx.x; e < E; e += 256) {
        p[e] = ((s_gw[0][e] + s_gw[1][e]) + s_gw[2][e]) + s_gw[3][e];
        p[E + e] = ((s_gb[0][e] + s_gb[1][e]) + s_gb[2][e]) + s_gb[3][e];
    }
}

// grid (ceil(E / 64), 2): 64 columns x 4 chains per workgroup; y = 0 -> gw, y = 1 -> gb
__global__ __launch_bounds__(256) void gpt_layernorm_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ gw,
                                                                       float* __restrict__ gb, int nblk, int E) {
    __shared__ float s_p[4][64];
    const int col = threadIdx.x & 63, ch = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + col, which = blockIdx.y;
    float acc = 0.0f;
    if (e < E)
        for (int k = ch; k < nblk; k += 4) acc += part[((size_t)k * 2 + which) * E + e];
    s_p[ch][col] = acc;
    __syncthreads();
    if (ch == 0 && e < E) (which ? gb : gw)[e] = ((s_p[0][col] + s_p[1][col]) + s_p[2][col]) + s_p[3][col];
}

extern "C" size_t lipvq_gpt_layernorm_bwd_workspace_bytes(int64_t N, int E) {
    if (N <= 0 || E <= 0) return 0;
    const int rpb = gpt_ln_rows_per_block(N);
    return (size_t)((N + rpb - 1) / rpb) * 2 * (size_t)E * sizeof(float);
}

static int gpt_layernorm_bwd_launch(const char* what, const float* gy, const float* xhat, const float* rstd, const float* w,
                                    const float* gres, float* gs, float* gbr, float* gw, float* gb, void* workspace,
                                    lq_dropout_src src, int64_t N, int E, void* stream) {
    if (N < 0 || E <= 0) return fail(LIPVQ_EINVAL, "%s: N=%lld E=%d", what, (long long)N, E);
    if (E > GPT_MAXE || (E & 3) != 0) return fail(LIPVQ_EUNSUPPORTED, "%s: E=%d (a multiple of 4, <= %d)", what, E, GPT_MAXE);
    if (!gw || !gb) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {                                       // no rows: the parameter gradients are zero
        if (hipMemsetAsync(gw, 0, (size_t)E * sizeof(float), st) != hipSuccess || hipMemsetAsync(gb, 0, (size_t)E * sizeof(float), st) != hipSuccess)
            return fail(LIPVQ_EHIP, "%s: memset failed", what);
        return 0;
    }
    if (!gy || !xhat || !rstd || !w || !gs || !workspace || (src.snap && !gbr)) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if ((((uintptr_t)gy | (uintptr_t)xhat | (uintptr_t)w | (uintptr_t)gres | (uintptr_t)gs | (uintptr_t)gbr) & 15) != 0)
        return fail(LIPVQ_EINVAL, "%s: pointers must be 16-byte aligned", what);
    const int rpb = gpt_ln_rows_per_block(N);
    const int nblk = (int)((N + rpb - 1) / rpb);
    if (src.snap)
        hipLaunchKernelGGL(gpt_layernorm_bwd_kernel<true>, dim3(nblk), dim3(256), 0, st, (const float4*)gy, (const float4*)xhat, rstd,
                           (const float4*)w, (const float4*)gres, (float4*)gs, (float4*)gbr, (float*)workspace, src, N, E, rpb);
    else
        hipLaunchKernelGGL(gpt_layernorm_bwd_kernel<false>, dim3(nblk), dim3(256), 0, st, (const float4*)gy, (const float4*)xhat, rstd,
                           (const float4*)w, (const float4*)gres, (float4*)gs, (float4*)nullptr, (float*)workspace, src, N, E, rpb);
    hipLaunchKernelGGL(gpt_layernorm_bwd_reduce_kernel, dim3((E + 63) / 64, 2), dim3(256), 0, st, (const float*)workspace, gw, gb, nblk, E);
    return check_launch(what);
}

extern "C" int lipvq_gpt_layernorm_bwd_f32(const float* gy, const float* xhat, const float* rstd, const float* w, const float* gres,
                                           float* gs, float* gw, float* gb, void* workspace, int64_t N, int E, void* stream) {
    return gpt_layernorm_bwd_launch("gpt_layernorm_bwd", gy, xhat, rstd, w, gres, gs, nullptr, gw, gb, workspace, lq_dropout_src{}, N, E, stream);
}

extern "C" int lipvq_gpt_layernorm_bwd_drop_f32(const float* gy, const float* xhat, const float* rstd, const float* w, const float* gres,
                                                const int64_t* snap, uint32_t site, double p, float* gs, float* gbranch, float* gw,
                                                float* gb, void* workspace, int64_t N, int E, void* stream) {
    if (int rc = lq_dropout_check("gpt_layernorm_bwd_drop", snap, p, N)) return rc;
    return gpt_layernorm_bwd_launch("gpt_layernorm_bwd_drop", gy, xhat, rstd, w, gres, gs, gbranch, gw, gb, workspace,
                                    lq_dropout_src_make(snap, site, p), N, E, stream);
}
