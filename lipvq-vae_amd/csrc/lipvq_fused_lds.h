// lipvq_fused_lds.h -- the LDS of one workgroup of the fused tokenize launch (lipvq_fused.hip), described ONCE: the host sizes the
// launch with it and the kernel takes its pointers from it.  Includable from a stand-alone host program.
#pragma once
#include "lipvq_screen.h"

// LDS budget: the D = 128 instance holds 105 KB of weights, so its codebook stages are one tile deep
#define FUSED_HIST_MAX 2048
#define FUSED_LDS_MAX ((size_t)160 * 1024)
// stage ring of the fused kernel (LDS left beside the encoder weights): S <= 4: four buffers of two/four tiles; S = 8: the
// weights take 98 KB, three buffers of one tile
// The Lipschitz layer's weights are STREAMED through the stage ring (instead of living in LDS) from this many k-steps on:
// 13 (D = 208) has no choice -- 112 KB of A operands; for 8 (D = 128) it is a trade measured in round 3: 64 KB of LDS go from
// a phase that is a twentieth of the work at K = 8192 to the codebook ring of the phase that is the rest.
// (LQ_STREAM2_MIN_S = 9 lives in lipvq_screen.h: it also sizes the streamed weights' region of the workspace)
#define LQ_RING8_TC 1
#define LQ_RING8_NB 3
#define LQ_RING13_NB 3
constexpr int fused_ring_tc(int S) { return (S <= 2) ? 4 : (S <= 4) ? 2 : (S == 8) ? LQ_RING8_TC : 1; }
constexpr int fused_ring_nb(int S) { return (S <= 4) ? 4 : (S == 8) ? LQ_RING8_NB : LQ_RING13_NB; }
#define LQ_COARSE_TC_WIDE 2       /* tiles per stage of the one-product S = 8 instance */
// S = 8 (cfg3): 1.610 -> 1.555 ms, same box.  Not S = 13: with two tiles per stage that instance runs 10 ms instead of 0.9 (its
// 26-k-step stage body no longer fits the registers it has left beside 104 of row fragments) -- profiles/r04_f_coarse_ring_ab.txt
constexpr int fused_ring_tc_coarse(int S) { return S == 8 ? LQ_COARSE_TC_WIDE * fused_ring_tc(S) : fused_ring_tc(S); }

// [ P0 | B0 | P1 | B1 | P2 | B2 | mu ] (floats), then the stage ring, then the usage histogram (bytes).  A is the fan-in, 1 .. 64
// (tokenize_shape_fits asks nothing else).  FAST: the three weight blocks are fp16 MFMA fragments, [T][k-steps of 16][64 lanes][8 halfs].
template <int S, bool FAST>
struct FusedLds {
    static constexpr int T0 = 2, T1 = 4, T2 = (S + 1) / 2;          // 32-feature tiles per layer; S odd (D = 208): the last one is half used
    static constexpr int S1 = 16 * T0, S2 = 16 * T1;                // k-steps (pairs) of layers 1 and 2
    // STREAM2: the Lipschitz layer's weights (T2 x 16 KB of fp32 MFMA A operands: 112 KB at D = 208) do not fit beside the stage
    // ring, so they are streamed, one 16 KB output-tile slab at a time, through that ring -- which is idle during the encoder
    // phase -- by the same LDS-DMA + counted-vmcnt mechanism as the codebook (all eight waves work on the same tile).
    static constexpr bool STREAM2 = !FAST && S >= LQ_STREAM2_MIN_S;

    // The stage ring + its dummy KiB of the instance that runs the three-product (fine) or the one-product (coarse) screen.  The
    // one-product screen stages hi-only tiles (half the bytes): twice the tiles per stage in the same LDS at S = 8.
    static constexpr size_t RING_FINE = lq_ring_bytes<S, fused_ring_tc(S), fused_ring_nb(S)>();
    static constexpr size_t RING_COARSE = (size_t)fused_ring_nb(S) * ScreenCfg<S, fused_ring_tc_coarse(S), true>::STAGE_BYTES + 1024;
    // what a launch RESERVES: one size for both screens' instances, the larger ring, rounded to 64
    static constexpr size_t RING_BYTES = ((RING_FINE > RING_COARSE ? RING_FINE : RING_COARSE) + 63) & ~(size_t)63;
    // what an instance USES, and behind which its histogram starts: its own ring or the fine one, whichever is larger.  (At S = 8
    // the coarse ring is 768 bytes larger than the fine one, so the three-product instance's histogram starts that much in front
    // of the reservation's end of ring -- inside it; moving it to RING_BYTES would change that kernel's code.)
    template <bool COARSE>
    static constexpr size_t stages_bytes() { return COARSE && RING_COARSE > RING_FINE ? RING_COARSE : RING_FINE; }
    // the streamed layer-2 slabs' three buffers (either screen): 16 KB slabs at the fine ring's stage stride
    static constexpr size_t SLAB_STRIDE = ScreenCfg<S, fused_ring_tc(S), false>::STAGE_BYTES;
    static constexpr int SLAB_BYTES = (S2 / 4) * 1024;              // one output tile's A operands: 16 KB
    static_assert(!STREAM2 || (SLAB_BYTES <= SLAB_STRIDE && 3 * SLAB_STRIDE <= RING_FINE), "slabs ride in the stage ring");
    // per-wave private slice of the (idle) ring: the decision's transposes (LQ_DECIDE_BYTES) and the z_q copy's staging (GP KiB)
    template <int WAVES, bool COARSE>
    static constexpr size_t wslice() { return (stages_bytes<COARSE>() >= (size_t)WAVES * 8192) ? 8192 : LQ_DECIDE_BYTES; }
    template <int WAVES, bool COARSE, bool KEEPZ>
    static constexpr bool slices_fit() {
        static_assert(stages_bytes<COARSE>() >= (size_t)WAVES * LQ_DECIDE_BYTES, "the decision's per-wave transposes live in the stage ring");
        static_assert(LQ_DECIDE_BYTES >= 4096 && wslice<WAVES, COARSE>() >= LQ_DECIDE_BYTES, "a slice holds the transposes and four staged KiB");
        static_assert(!KEEPZ || wslice<WAVES, COARSE>() >= LQ_DECIDE_BYTES + 64 * S, "KEEPZ: one z_e row behind the decision scratch");
        static_assert(!STREAM2 || SLAB_BYTES % (1024 * WAVES) == 0, "slabs ride in the stage ring");
        return true;
    }

    // The blocks in order, in floats.  Only layer 0's depends on the fan-in: k0 groups of k-steps (parity: S0q groups of four
    // fp32 k-steps, [T0][S0q][64][4]; FAST: S0h fp16 k-steps of 16), 256 floats per group and tile.
    // k0 is what the kernel calls S0q (= (packed_layout(A, ..).S0 + 3) / 4, S0 = (A + 1) / 2) in the parity instances and S0h in the
    // fast ones: the prologue fills and layer 0 reads the block with those, so the three must stay the same expression of A.
    int k0;
    static constexpr int N_B0 = 32 * T0, N_P1 = FAST ? T1 * (2 * T0) * 256 : T1 * (S1 / 4) * 256;       // [32*T0], [T1][S1/4][64][4]
    static constexpr int N_B1 = 32 * T1, N_P2 = FAST ? T2 * (2 * T1) * 256 : STREAM2 ? 0 : T2 * (S2 / 4) * 256;   // [32*T1], [T2][S2/4][64][4]
    static constexpr int N_B2 = 32 * T2, N_MU = 16 * S;                                                  // [32*T2], [16*S]
    __host__ __device__ explicit FusedLds(int A) : k0(FAST ? (A + 15) / 16 : ((A + 1) / 2 + 3) / 4) {}
    template <typename I>
    __host__ __device__ I n_P0() const { return (I)T0 * k0 * 256; }
    // where an instance's histogram starts, in bytes behind the start of the ring
    template <bool COARSE>
    static constexpr size_t hist_in_ring() { return (stages_bytes<COARSE>() + 63) & ~(size_t)63; }
    // what the host reserves: the same blocks, the ring of either screen
    __host__ __device__ size_t bytes_nohist() const {
        return (n_P0<size_t>() + N_B0 + N_P1 + N_B1 + N_P2 + N_B2 + N_MU) * sizeof(float) + RING_BYTES;
    }
    // the per-workgroup usage histogram: codebooks of up to FUSED_HIST_MAX codes, where the LDS has room for it
    __host__ __device__ static bool hist_fits(int A, int K) {
        return K <= FUSED_HIST_MAX && FusedLds(A).bytes_nohist() + (size_t)K * 4 <= FUSED_LDS_MAX;
    }
    __host__ __device__ static size_t bytes(int A, int K) { return FusedLds(A).bytes_nohist() + (hist_fits(A, K) ? (size_t)K * 4 : 0); }
};
