// lipvq_gemm_bf16.hip -- the opt-in bf16 matrix-pipe mode of the transformer's Linears (lipvq-vae_amd/gpt.py,
// GPTBackbone.set_matmul_precision("bf16")): forward, input gradient and weight gradient of one nn.Linear.
//
// Arithmetic contract (stated in include/lipvq.h): operands are fp32 in memory and stay so; every operand element is rounded
// to bf16 with round-to-nearest-even (v_cvt_pk_bf16_f32) on its way into LDS, products are accumulated in fp32 by
// v_mfma_f32_32x32x16_bf16, and everything after the accumulator -- bias, GELU, the sums over row chunks, the bias gradient --
// is fp32 (the GELU is lq_act_apply, the function of lipvq_linear_act_f32).  No float atomics: the same bits on every run.
//
// One tile core serves the three layouts.  It computes C[i][c] = sum_k A(i, k) B(k, c) for a BM x BN tile of C with a
// workgroup of WM x WN waves, each wave owning RM x RN MFMA tiles of 32 x 32.  Per step of BK = 32 along the reduction the
// workgroup stages a [BM][32] image of A and a [BN][32] image of B in LDS as bf16, REDUCTION INDEX CONTIGUOUS (rows of 80
// bytes: 64 of data + 16 of padding, so the 16-byte fragment reads of 16 consecutive rows fall on 16 different 16-byte slots
// of the 256-byte bank row), two buffers: the global loads of step t + 1 are issued before the MFMAs of step t and written
// to the other buffer after them, one barrier per step.  What differs between the layouts is only how an operand lies in
// memory:
//   reduction index contiguous (x and W of the forward, g of the input gradient): a thread loads 8 consecutive floats and
//       writes 8 bf16 (16 bytes) to the image;
//   reduction index strided (W of the input gradient, read AS STORED; g and x of the weight gradient): a thread loads a
//       float4 of 4 consecutive columns from each of 8 consecutive reduction rows -- coalesced along the columns -- and so
//       holds, per column, the 8 reduction-consecutive values of one 16-byte LDS write: the transpose happens in registers.
// Out-of-range rows, columns and reduction steps are loaded from a clamped (valid) address and replaced by zero, so no
// load depends on a branch and nothing outside the tensors is read; stores are masked.
//
// The bf16x3 mode (set_matmul_precision("bf16x3"), the lipvq_*_bf16x3 entry points) is the same kernel with SPLIT = true:
// every operand element v is staged as TWO bf16 numbers, hi = rne(v) and lo = rne(v - hi) (the subtraction is exact in fp32;
// lo = 0 where hi is not finite), formed from the staged fp32 registers at store time into a hi image and a lo image of the
// same layout (LDS doubles, loads and staging registers do not grow), and every MFMA of the plain mode becomes three into
// the same accumulator, in the fixed order a_lo b_hi, a_hi b_lo, a_hi b_hi.  The epilogue is the plain mode's.
#include "lipvq_common.h"
#include "lipvq_bf16_stage.h"   // gb_pk, gb_pk_lo, gb_stage8, gb_keep, GB_BK, GB_LDK: shared with the heads' product stage

namespace {

struct GemmArgs {
    const float* A;       // forward: x [M][R]; input gradient: g [M][R]; weight gradient: g [R][M]
    const float* B;       // forward: W [Nc][R]; input gradient: W [R][Nc]; weight gradient: x [R][Nc]
    const float* bias;    // forward only, may be NULL
    float* C;             // [M][Nc]; weight gradient: the workspace, one [M][Nc] slab per row chunk
    float* pre;           // forward only, may be NULL
    float* gbp;           // weight gradient: [chunks][M] partial column sums of g
    int64_t M;            // rows of C
    int Nc;               // columns of C
    int64_t R;            // reduction length
    int64_t chunk;        // weight gradient: reduction rows per blockIdx.z
    int act;
};

// Staging registers of an operand whose reduction index is contiguous in memory: P[row][k], leading dimension ld.
// SPLIT: store() writes the lo image BR rows behind the hi image.
template <int BR, int NT, bool SPLIT>
struct ContigStage {
    static constexpr int CH = BR * 4, PER = CH / NT;                 // chunks of 8 floats in a [BR][32] tile, per thread
    static_assert(CH % NT == 0, "every thread stages the same number of chunks");
    lq_f32x4 v[PER][2];
    __device__ __forceinline__ void load(const float* __restrict__ P, int64_t ld, int64_t rows, int64_t r0, int64_t k0,
                                         int64_t kend, int tid) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = tid + i * NT;
            const int64_t row = r0 + (c >> 2), k = k0 + (c & 3) * 8;
            const bool ok = row < rows && k < kend;                                  // kend % 8 == 0: 8 floats are in or out together
            const lq_f32x4* p = reinterpret_cast<const lq_f32x4*>(P + (size_t)(ok ? row : 0) * ld + (ok ? k : 0));
            const uint32_t m = ok ? 0xffffffffu : 0u;
            v[i][0] = gb_keep(p[0], m);
            v[i][1] = gb_keep(p[1], m);
        }
    }
    __device__ __forceinline__ void store(unsigned short* __restrict__ s, int tid) const {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = tid + i * NT;
            gb_stage8<SPLIT>(s + (c >> 2) * GB_LDK + (c & 3) * 8, BR * GB_LDK, v[i][0].x, v[i][0].y, v[i][0].z, v[i][0].w,
                             v[i][1].x, v[i][1].y, v[i][1].z, v[i][1].w);
        }
    }
};

// Staging registers of an operand whose reduction index is the ROW index in memory: P[k][col], leading dimension ld.  A unit
// is 8 reduction rows x 4 columns; the threads OFF .. OFF + units - 1 own one each (OFF lets the two operands of the weight
// gradient use different threads of the workgroup).  SUM: also keep the fp32 column sums of what was loaded (the bias gradient).
template <int BR, int NT, int OFF, bool SUM, bool SPLIT>
struct StridedStage {
    static constexpr int CG = BR / 4, UN = 4 * CG;
    static_assert(OFF + UN <= NT, "one unit per thread");
    lq_f32x4 v[8];
    lq_f32x4 sum;
    __device__ __forceinline__ void init() { sum = (lq_f32x4){0.f, 0.f, 0.f, 0.f}; }
    __device__ __forceinline__ void load(const float* __restrict__ P, int64_t ld, int64_t cols, int64_t c0, int64_t k0,
                                         int64_t kend, int tid) {
        const int u = tid - OFF;
        if (u >= 0 && u < UN) {                                                       // wave-uniform when UN and OFF are multiples of 64
            const int64_t c = c0 + (u % CG) * 4;
            const bool cok = c < cols;                                               // cols % 4 == 0: a float4 is in or out
            const float* base = P + (cok ? c : 0);
            const int64_t kb = k0 + (u / CG) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int64_t kk = kb + j;
                const uint32_t m = (cok && kk < kend) ? 0xffffffffu : 0u;
                v[j] = gb_keep(*reinterpret_cast<const lq_f32x4*>(base + (size_t)(kk < kend ? kk : kend - 1) * ld), m);
            }
        }
    }
    __device__ __forceinline__ void store(unsigned short* __restrict__ s, int tid) {
        const int u = tid - OFF;
        if (u >= 0 && u < UN) {
            unsigned short* d = s + ((u % CG) * 4) * GB_LDK + (u / CG) * 8;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                gb_stage8<SPLIT>(d + e * GB_LDK, BR * GB_LDK, v[0][e], v[1][e], v[2][e], v[3][e], v[4][e], v[5][e], v[6][e], v[7][e]);
            if (SUM) sum += ((((((v[0] + v[1]) + v[2]) + v[3]) + v[4]) + v[5]) + v[6]) + v[7];   // rows in ascending order
        }
    }
};

template <bool STRIDED, int BR, int NT, int OFF, bool SUM, bool SPLIT>
struct StageOf { typedef ContigStage<BR, NT, SPLIT> type; };
template <int BR, int NT, int OFF, bool SUM, bool SPLIT>
struct StageOf<true, BR, NT, OFF, SUM, SPLIT> { typedef StridedStage<BR, NT, OFF, SUM, SPLIT> type; };

// A wave's RM x RN accumulator tiles to memory.  C/D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2)
// + 4 (lane >> 5); row0 / col0 already hold the lane's part.  FWD: + bias, the pre-activation, the activation (ACT = -1: a.act).
template <int RM, int RN, bool FWD, int ACT>
__device__ __forceinline__ void gb_store_tile(const f32x16 (&acc)[RM][RN], const GemmArgs& a, float* __restrict__ C, int64_t row0,
                                              int64_t col0) {
#pragma unroll
    for (int m = 0; m < RM; ++m)
#pragma unroll
        for (int n = 0; n < RN; ++n) {
            const int64_t col = col0 + n * 32;
            if (col >= a.Nc) continue;
            const float bv = (FWD && a.bias) ? a.bias[col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = row0 + m * 32 + (r & 3) + 8 * (r >> 2);
                if (row >= a.M) continue;
                const size_t o = (size_t)row * a.Nc + col;
                float val = acc[m][n][r];
                if (FWD) {
                    if (a.bias) val = val + bv;
                    if (a.pre) a.pre[o] = val;
                    val = lq_act_apply(val, ACT < 0 ? a.act : ACT);
                }
                C[o] = val;
            }
        }
}

// AS / BS: the operand's reduction index is strided in memory.  (false, false) forward, (false, true) input gradient,
// (true, true) weight gradient.  SPLIT: the bf16x3 mode -- an operand buffer is a hi image followed by a lo image (IM = 2
// images), 80 KiB of LDS at the 128 tile, and a k-step is three MFMAs per accumulator tile.
template <int WM, int WN, int RM, int RN, bool AS, bool BS, bool SPLIT>
__global__ __launch_bounds__(64 * WM * WN) void gemm_bf16_kernel(const GemmArgs a) {
    constexpr int NT = 64 * WM * WN, BM = 32 * WM * RM, BN = 32 * WN * RN, IM = SPLIT ? 2 : 1;
    constexpr bool FWD = !AS && !BS, WGRAD = AS && BS;
    constexpr int BOFF = (WGRAD && BM + BN <= NT) ? BM : 0;                           // A units: threads [0, BM); B units: the next BN
    constexpr int ABUF = IM * BM * GB_LDK, BBUF = IM * BN * GB_LDK;                   // one buffer of an operand, in bf16
    __shared__ __attribute__((aligned(16))) unsigned short lds[2 * (ABUF + BBUF)];
    static_assert(!WGRAD || sizeof(lds) >= 4 * BM * sizeof(float), "the bias-gradient reduce reuses the LDS");
    unsigned short* const sA = lds;
    unsigned short* const sB = lds + 2 * ABUF;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid / WN, wn = wid % WN;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    const int64_t col0 = (int64_t)blockIdx.y * BN;
    const int64_t kbeg = WGRAD ? (int64_t)blockIdx.z * a.chunk : 0;
    const int64_t kend = WGRAD ? (kbeg + a.chunk < a.R ? kbeg + a.chunk : a.R) : a.R;
    const int T = (int)((kend - kbeg + GB_BK - 1) / GB_BK);
    const int64_t lda = AS ? a.M : a.R, ldb = BS ? (int64_t)a.Nc : a.R;

    typename StageOf<AS, BM, NT, 0, WGRAD, SPLIT>::type stA;
    typename StageOf<BS, BN, NT, BOFF, false, SPLIT>::type stB;
    if constexpr (AS) stA.init();

    f32x16 acc[RM][RN];
#pragma unroll
    for (int m = 0; m < RM; ++m)
#pragma unroll
        for (int n = 0; n < RN; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;

    stA.load(a.A, lda, a.M, row0, kbeg, kend, tid);
    stB.load(a.B, ldb, a.Nc, col0, kbeg, kend, tid);
    stA.store(sA, tid);
    stB.store(sB, tid);
    __syncthreads();

    const int fr = lane & 31, fh = lane >> 5;
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        if (t + 1 < T) {
            const int64_t k0 = kbeg + (int64_t)(t + 1) * GB_BK;
            stA.load(a.A, lda, a.M, row0, k0, kend, tid);
            stB.load(a.B, ldb, a.Nc, col0, k0, kend, tid);
        }
        const unsigned short* cA = sA + cur * ABUF + (wm * RM * 32 + fr) * GB_LDK + fh * 8;
        const unsigned short* cB = sB + cur * BBUF + (wn * RN * 32 + fr) * GB_LDK + fh * 8;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            lq_bf16x8 fa[RM], fb[RN];
#pragma unroll
            for (int m = 0; m < RM; ++m)
                fa[m] = __builtin_bit_cast(lq_bf16x8, *reinterpret_cast<const lq_u32x4*>(cA + m * 32 * GB_LDK + s * 16));
#pragma unroll
            for (int n = 0; n < RN; ++n)
                fb[n] = __builtin_bit_cast(lq_bf16x8, *reinterpret_cast<const lq_u32x4*>(cB + n * 32 * GB_LDK + s * 16));
            if constexpr (SPLIT) {
                // the two cross terms first, then hi x hi: per accumulator tile the same three-step chain at every tile
                // instance; the term is the outer loop, so consecutive MFMAs write different accumulators where RM RN > 1
                lq_bf16x8 la[RM], lb[RN];
#pragma unroll
                for (int m = 0; m < RM; ++m)
                    la[m] = __builtin_bit_cast(lq_bf16x8, *reinterpret_cast<const lq_u32x4*>(cA + (BM + m * 32) * GB_LDK + s * 16));
#pragma unroll
                for (int n = 0; n < RN; ++n)
                    lb[n] = __builtin_bit_cast(lq_bf16x8, *reinterpret_cast<const lq_u32x4*>(cB + (BN + n * 32) * GB_LDK + s * 16));
#pragma unroll
                for (int m = 0; m < RM; ++m)
#pragma unroll
                    for (int n = 0; n < RN; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(la[m], fb[n], acc[m][n], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < RM; ++m)
#pragma unroll
                    for (int n = 0; n < RN; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[m], lb[n], acc[m][n], 0, 0, 0);
            }
#pragma unroll
            for (int m = 0; m < RM; ++m)
#pragma unroll
                for (int n = 0; n < RN; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[m], fb[n], acc[m][n], 0, 0, 0);
        }
        if (t + 1 < T) {
            stA.store(sA + (cur ^ 1) * ABUF, tid);
            stB.store(sB + (cur ^ 1) * BBUF, tid);
        }
        __syncthreads();
    }

    float* const C = WGRAD ? a.C + (size_t)blockIdx.z * (size_t)a.M * a.Nc : a.C;
    const int64_t wrow0 = row0 + wm * RM * 32 + 4 * fh, wcol0 = col0 + wn * RN * 32 + fr;
    if (!FWD || a.act == LIPVQ_ACT_NONE) gb_store_tile<RM, RN, FWD, LIPVQ_ACT_NONE>(acc, a, C, wrow0, wcol0);
    else if (a.act == LIPVQ_ACT_GELU) gb_store_tile<RM, RN, FWD, LIPVQ_ACT_GELU>(acc, a, C, wrow0, wcol0);
    else gb_store_tile<RM, RN, FWD, -1>(acc, a, C, wrow0, wcol0);

    if constexpr (WGRAD) {
        // bias gradient of this chunk: the four 8-row groups of every step were summed per thread; add the groups in order
        if (blockIdx.y == 0) {                                                       // (the last barrier of the loop freed the LDS)
            float* red = reinterpret_cast<float*>(lds);                              // [4][BM]
            constexpr int CG = BM / 4;
            if (tid < 4 * CG) {
                float* d = red + (tid / CG) * BM + (tid % CG) * 4;
                d[0] = stA.sum.x; d[1] = stA.sum.y; d[2] = stA.sum.z; d[3] = stA.sum.w;
            }
            __syncthreads();
            for (int c = tid; c < BM; c += NT)
                if (row0 + c < a.M)
                    a.gbp[(size_t)blockIdx.z * a.M + row0 + c] = ((red[c] + red[BM + c]) + red[2 * BM + c]) + red[3 * BM + c];
        }
    }
}

// gW = the chunk slabs added in chunk order, gb likewise: one thread per element, the same order on every run
__global__ __launch_bounds__(256) void wgrad_bf16_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gW,
                                                                 float* __restrict__ gb, int64_t JK, int J, int nch) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = JK + (gb ? J : 0);
    if (i >= total) return;
    const bool w = i < JK;
    const float* p = w ? ws + i : ws + (size_t)nch * JK + (i - JK);
    const int64_t step = w ? JK : J;
    float s = p[0];
    for (int c = 1; c < nch; ++c) s = s + p[(size_t)c * step];
    if (w) gW[i] = s; else gb[i - JK] = s;
}

// Tile choice from the shape alone (lipvq_gemm_bf16_tile below, the rule of include/lipvq.h): 128 x 128 (2 x 2 waves of
// 64 x 64) once that gives the chip a workgroup per CU, else 64 x 64 (2 x 2 waves of 32 x 32), else one wave per 32 x 32 tile
// (the 240-row step shape: 8 x 16 .. 8 x 64 workgroups).
template <bool AS, bool BS, bool SPLIT>
static int launch_gemm(const char* what, const GemmArgs& a, int64_t nchunks, hipStream_t st) {
    const int t = lipvq_gemm_bf16_tile(a.M, a.Nc, nchunks);
    const int64_t gx = (a.M + t - 1) / t, gy = (a.Nc + t - 1) / t;
    if (gx > 0x7fffffffLL || gy > 65535 || nchunks > 65535) return fail(LIPVQ_EUNSUPPORTED, "%s: too large", what);
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)nchunks);
    if (t == 128) hipLaunchKernelGGL((gemm_bf16_kernel<2, 2, 2, 2, AS, BS, SPLIT>), grid, dim3(256), 0, st, a);
    else if (t == 64) hipLaunchKernelGGL((gemm_bf16_kernel<2, 2, 1, 1, AS, BS, SPLIT>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((gemm_bf16_kernel<1, 1, 1, 1, AS, BS, SPLIT>), grid, dim3(64), 0, st, a);
    return check_launch(what);
}

static int gemm_dims(const char* what, int64_t N, int J, int K) {
    if (N < 0 || J <= 0 || K <= 0) return fail(LIPVQ_EINVAL, "%s: bad sizes N=%lld J=%d K=%d", what, (long long)N, J, K);
    if ((J & 7) || (K & 7))
        return fail(LIPVQ_EUNSUPPORTED, "%s: input width %d and output width %d must be multiples of 8", what, K, J);
    return LIPVQ_OK;
}

static bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

// rows per chunk of the weight gradient: a function of (N, J, K) only (the formula of include/lipvq.h)
static int64_t wgrad_chunk(int64_t N, int J, int K) {
    const int64_t tiles = (int64_t)((J + 127) / 128) * ((K + 127) / 128);
    const int64_t want = tiles >= 1024 ? 1 : 1024 / tiles;
    const int64_t per = (N + want - 1) / want;
    const int64_t chunk = (per + 31) / 32 * 32;
    return chunk < 64 ? 64 : chunk;
}

template <bool SPLIT>
static int linear_act(const char* what, const float* x, const float* W, const float* b, float* y, float* pre, int64_t N, int Kin, int E,
                      int act, void* stream) {
    const int rc = gemm_dims(what, N, E, Kin);
    if (rc) return rc;
    if (act < LIPVQ_ACT_NONE || act > LIPVQ_ACT_RELU) return fail(LIPVQ_EINVAL, "%s: bad activation %d", what, act);
    if (N == 0) return LIPVQ_OK;
    if (!x || !W || !y) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if (misaligned(x) || misaligned(W)) return fail(LIPVQ_EINVAL, "%s: x and W must be 16-byte aligned", what);
    GemmArgs a = {x, W, b, y, pre, nullptr, N, E, Kin, Kin, act};
    return launch_gemm<false, false, SPLIT>(what, a, 1, (hipStream_t)stream);
}

template <bool SPLIT>
static int linear_nn(const char* what, const float* g, const float* W, float* gx, int64_t N, int J, int K, void* stream) {
    const int rc = gemm_dims(what, N, J, K);
    if (rc) return rc;
    if (N == 0) return LIPVQ_OK;
    if (!g || !W || !gx) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if (misaligned(g) || misaligned(W)) return fail(LIPVQ_EINVAL, "%s: g and W must be 16-byte aligned", what);
    GemmArgs a = {g, W, nullptr, gx, nullptr, nullptr, N, K, J, J, LIPVQ_ACT_NONE};
    return launch_gemm<false, true, SPLIT>(what, a, 1, (hipStream_t)stream);
}

template <bool SPLIT>
static int wgrad(const char* what, const float* G, const float* H, float* gW, float* gb, void* workspace, int64_t N, int J, int K,
                 void* stream) {
    const int rc = gemm_dims(what, N, J, K);
    if (rc) return rc;
    if (N == 0) return LIPVQ_OK;
    if (!G || !H || !gW || !workspace) return fail(LIPVQ_EINVAL, "%s: null pointer", what);
    if (misaligned(G) || misaligned(H) || misaligned(workspace))
        return fail(LIPVQ_EINVAL, "%s: G, H and the workspace must be 16-byte aligned", what);
    const int64_t chunk = wgrad_chunk(N, J, K), nch = (N + chunk - 1) / chunk;
    const int64_t JK = (int64_t)J * K;
    float* ws = static_cast<float*>(workspace);
    GemmArgs a = {G, H, nullptr, ws, nullptr, ws + (size_t)nch * JK, J, K, N, chunk, LIPVQ_ACT_NONE};
    const int lrc = launch_gemm<true, true, SPLIT>(what, a, nch, (hipStream_t)stream);
    if (lrc) return lrc;
    const int64_t total = JK + (gb ? J : 0);
    hipLaunchKernelGGL(wgrad_bf16_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws,
                       gW, gb, JK, J, (int)nch);
    return check_launch("wgrad_bf16_reduce_kernel");
}

}  // namespace

extern "C" {

int lipvq_gemm_bf16_tile(int64_t M, int Nc, int64_t chunks) {
    if (M <= 0 || Nc <= 0 || chunks <= 0) return 0;
    auto wgs = [&](int64_t t) { return ((M + t - 1) / t) * ((Nc + t - 1) / t) * chunks; };
    return wgs(128) >= 256 ? 128 : (wgs(64) >= 256 ? 64 : 32);
}

size_t lipvq_wgrad_bf16_workspace_bytes(int64_t N, int J, int K) {
    if (N <= 0 || J <= 0 || K <= 0) return 0;
    const int64_t chunk = wgrad_chunk(N, J, K);
    return (size_t)((N + chunk - 1) / chunk) * ((size_t)J * K + J) * sizeof(float);
}

int lipvq_linear_act_bf16(const float* x, const float* W, const float* b, float* y, float* pre, int64_t N, int Kin, int E,
                          int act, void* stream) {
    return linear_act<false>("lipvq_linear_act_bf16", x, W, b, y, pre, N, Kin, E, act, stream);
}

int lipvq_linear_act_bf16x3(const float* x, const float* W, const float* b, float* y, float* pre, int64_t N, int Kin, int E,
                            int act, void* stream) {
    return linear_act<true>("lipvq_linear_act_bf16x3", x, W, b, y, pre, N, Kin, E, act, stream);
}

int lipvq_linear_nn_bf16(const float* g, const float* W, float* gx, int64_t N, int J, int K, void* stream) {
    return linear_nn<false>("lipvq_linear_nn_bf16", g, W, gx, N, J, K, stream);
}

int lipvq_linear_nn_bf16x3(const float* g, const float* W, float* gx, int64_t N, int J, int K, void* stream) {
    return linear_nn<true>("lipvq_linear_nn_bf16x3", g, W, gx, N, J, K, stream);
}

int lipvq_wgrad_bf16(const float* G, const float* H, float* gW, float* gb, void* workspace, int64_t N, int J, int K,
                     void* stream) {
    return wgrad<false>("lipvq_wgrad_bf16", G, H, gW, gb, workspace, N, J, K, stream);
}

int lipvq_wgrad_bf16x3(const float* G, const float* H, float* gW, float* gb, void* workspace, int64_t N, int J, int K,
                       void* stream) {
    return wgrad<true>("lipvq_wgrad_bf16x3", G, H, gW, gb, workspace, N, J, K, stream);
}

}  // extern "C"
