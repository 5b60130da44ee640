/* lipvq.h -- C ABI of the MI355X (gfx950) LipVQ-VAE action-tokenizer library.
 *
 * The reference is pure Python/PyTorch: its "FFI" for this path is the set of stock torch ops
 * that LLFQVAE_V4.forward / VQVAE.forward issue (reference files, relative to /root/reference:
 *   v5 = robomimic/models/vq_vae/backbone_lfqvae_v5.py,  vq = robomimic/models/vq_vae/backbone.py).
 * Each entry point below replaces one group of those ops with one hand-written HIP launch and
 * cites the lines it replaces.  The reference-side binding (a ctypes stub called from a
 * torch.autograd.Function) is shown in INTEGRATION.md and implemented in
 * lipvq-vae_amd/_capi.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch allocates); the library
 *     never frees, retains or reallocates it.  Tensors are row-major contiguous fp32 unless a
 *     parameter says otherwise; indices and usage counts are int64 (torch.long).
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *     Work is only enqueued; no entry point synchronises the device.
 *   - return value: 0 on success, a negative LIPVQ_E* code otherwise; lipvq_last_error()
 *     returns a thread-local message.  Nothing throws across the ABI.
 *   - stateless and re-entrant; one process per GPU.
 *   - arithmetic: "canonical fp32" (lipvq-vae_amd/csrc/lipvq_math.h): every forward tensor is
 *     bit-identical to oracle/lipvq_oracle.c on the same inputs.  That includes denormals -- nothing is
 *     flushed, neither by the vector ALU nor by the fp32 MFMA chains of the three-layer stacks, operands
 *     and results alike (measured on gfx950: tests/test_gpu_mlp3_edges.py) -- and NaN / infinite
 *     inputs, which stay in their own row.
 */
#ifndef LIPVQ_H_
#define LIPVQ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIPVQ_ABI_VERSION 1

enum { LIPVQ_OK = 0, LIPVQ_EINVAL = -1, LIPVQ_EUNSUPPORTED = -2, LIPVQ_EHIP = -3 };

/* activation codes of lipvq_mlp3_* */
enum { LIPVQ_ACT_NONE = 0, LIPVQ_ACT_GELU = 1, LIPVQ_ACT_SIGMOID = 2, LIPVQ_ACT_RELU = 3 };

/* distance rules of lipvq_nearest_f32 */
enum {
    LIPVQ_DIST_NORM = 0,  /* v5:43-46  torch.norm(.., dim=-1) then argmin (compares square roots) */
    LIPVQ_DIST_SQSUM = 1  /* vq:58-63  (..).pow(2).sum(-1) then argmin */
};

int lipvq_abi_version(void);
const char* lipvq_last_error(void);

/* Options: process-global switches for tests and measurements, set EXPLICITLY -- the library reads no environment variable.
 * Results are identical under every setting (the parity suites run both screens and every kernel shape); only speed changes.
 * value = NULL restores the default.  Unknown name: LIPVQ_EINVAL.  Read per launch.
 *   screen_mode       "coarse" | "fine": force the one-product / three-product screen (default: the shape's measured winner,
 *                     lipvq_screen_is_coarse)
 *   tok_shape         "w8rg1" | "w4rg1": 8 or 4 waves per workgroup of the fused launch (default: 4 up to 32 768 rows in
 *                     the parity mode, else 8)
 *   tok_ze_rows       batch size up to which a fused launch stores z_e for its exact stage when nothing else asks for it
 *   tok_inplace       "0" | "1": the fused launch never / whenever possible lets its waves decide their uncertified rows in place
 *                     instead of listing them for a second kernel (default: whenever possible = K <= 2048 under the three-product
 *                     screen; a parity launch of a latent width <= 64 whose caller wants no z_e then stores none)
 *   tok_defer_ze, tok_nt_ze   "0" | "1": the fused launch's two device-dependent schedule choices (the last z_e tile's stores issued
 *                     behind the screen's first stage copies; z_e rows stored nontemporal) -- overrides the defaults (0, 1) and
 *                     whatever lipvq_tokenize_tune_f32 found for the device */
int lipvq_set_option(const char* name, const char* value);
const char* lipvq_get_option(const char* name);        /* NULL = default */

/* v5:6-12 normalization():  scale[i] = min(1, softplus(ci[i]) / sum_j |W[i][j]|),  Wn = W * scale.
 * W [D][H], ci [D]; scale [D] and Wn [D][H] are outputs (either may be NULL). */
int lipvq_lipschitz_scale_f32(const float* W, const float* ci, float* scale, float* Wn, int D, int H,
                              void* stream);

/* A three-layer perceptron y = act2(L2(act1(L1(act0(L0(x)))))) with nn.Linear weights
 * W_l [J_l][K_l] -- the shape of every MLP stack on the path:
 *   v5:54-59 + v5:22-24   encoder + Lipschitz layer   (A -> 64 -> hidden -> D; gelu, gelu, sigmoid; W2 = Wn)
 *   v5:62-68              decoder + to_output         (D -> 64 -> hidden -> A; gelu, gelu, none)
 *   vq:17-24 / vq:25-32   ReLU encoder / decoder      (relu x3)
 * The weights are first re-laid out into MFMA A-operand order by lipvq_mlp3_pack_f32 (once
 * per parameter update); `packed` needs lipvq_mlp3_packed_floats() floats.
 * J0 and J1 must be multiples of 32 (<= 256); K0 and J2 are free. */
size_t lipvq_mlp3_packed_floats(int K0, int J0, int J1, int J2);
int lipvq_mlp3_pack_f32(const float* W0, const float* b0, const float* W1, const float* b1,
                        const float* W2, const float* b2, float* packed, int K0, int J0, int J1,
                        int J2, void* stream);
/* x [N][K0], or, when gather_idx != NULL, row n of the input is table x[gather_idx[n]] (the
 * codebook gather of v5:47 fused into the decoder's first layer).  y [N][J2].  pre0/pre1/pre2
 * (each may be NULL) receive the pre-activations [N][J_l] that the backward pass needs. */
int lipvq_mlp3_f32(const float* x, const int64_t* gather_idx, const float* packed, float* y,
                   float* pre0, float* pre1, float* pre2, int64_t N, int K0, int J0, int J1, int J2,
                   int act0, int act1, int act2, void* stream);

/* v5:37-48 LFQQuantizer.forward / vq:55-66 VQVAE.quantize (distance + argmin + gather):
 *   idx[n] = first k minimising dist(z[n], codebook[k]);  zq[n] = codebook[idx[n]];
 *   usage[k] += number of rows mapped to k (usage may be NULL; it is NOT zeroed here).
 * z [N][D], codebook [K][D], idx [N] int64, zq [N][D] (may be NULL), best [N] (may be NULL)
 * receives the winning compared value.  Never materialises [N][K] or [N][K][D]. */
int lipvq_nearest_f32(const float* z, const float* codebook, int64_t* idx, float* zq,
                      int64_t* usage, float* best, int64_t N, int K, int D, int dist, void* stream);

/* vq:74 straight-through value  out = z_e + (z_q - z_e)  (fp32, as torch rounds it). */
int lipvq_ste_f32(const float* ze, const float* zq, float* out, int64_t n_elem, void* stream);

/* v5:79-81 / vq:50,69-70  F.mse_loss pair:  out[0] = mean((xr-x)^2) over nx elements,
 * out[1] = mean((zq-ze)^2) over nz elements.  workspace: lipvq_mse_workspace_bytes() bytes. */
size_t lipvq_mse_workspace_bytes(void);
int lipvq_mse_pair_f32(const float* xr, const float* x, int64_t nx, const float* zq, const float* ze,
                       int64_t nz, float* out2, void* workspace, void* stream);

/* The same two means in out3[0], out3[1], plus out3[2] = the tokenizer's loss built from them on the device in the
 * reference's fp32 association:  LIPVQ_LOSS_LLFQ  (m0 + w m1) + w m1   (backbone_lfqvae_v5.py:83, w = 0.25)
 *                                LIPVQ_LOSS_VQ    m0 + (m1 + w m1)     (backbone.py:50-51, 69-71, w = commitment_cost). */
#define LIPVQ_LOSS_LLFQ 0
#define LIPVQ_LOSS_VQ 1
int lipvq_mse_pair_loss_f32(const float* xr, const float* x, int64_t nx, const float* zq, const float* ze, int64_t nz,
                            float* out3, float w, int form, void* workspace, void* stream);


/* ---- nearest code, fast path: MFMA screening + exact re-scoring (same results as
 *      lipvq_nearest_f32(.., LIPVQ_DIST_NORM); design: lipvq-vae_amd/csrc/lipvq_screen.hip) ------ */

/* Per-codebook preparation (centred, fp16 hi/lo split, MFMA fragment order, |e|^2, bounds).
 * Redo it whenever the codebook changes.  prep: lipvq_nearest_prep_bytes(K, D) bytes. */
size_t lipvq_nearest_prep_bytes(int K, int D);
int lipvq_nearest_prepare_f32(const float* codebook, void* prep, int K, int D, void* stream);
int lipvq_nearest_screened_supported(int K, int D);          /* 1 for any D in 1 ... 512 (widths other than 32 / 64 / 128 / 208 /
                                                               * 256 / 384 / 512 run the next larger instance on zero-padded
                                                               * columns; above 208 a three-product screen only) */
size_t lipvq_nearest_workspace_bytes(int64_t N);
/* The screen comes in two strengths with identical results: three fp16 products per algorithmic product (22-bit operands; a
 * fraction of a percent of the rows left to the exact kernel) or ONE (11-bit operands, a third of the matrix work, lower-bound
 * bookkeeping; 10-40 % of the rows left to the exact stage with their two or three candidates each).  The library picks per
 * shape (the one-product screen from K = 4096 on, and from K = 1024 on for 64 < D <= 208; never for D > 208); this query tells which one
 * a call with (K, D) would run now (environment LIPVQ_SCREEN_MODE=coarse|fine overrides: a measurement knob). */
int lipvq_screen_is_coarse(int K, int D);
/* idx / zq / usage exactly as lipvq_nearest_f32.  After the call the first int of `workspace`
 * holds how many rows were decided by the exact kernel (the rest were certified by the screen). */
int lipvq_nearest_screened_f32(const float* z, const float* codebook, const void* prep, int64_t* idx, float* zq,
                               int64_t* usage, void* workspace, int64_t N, int K, int D, void* stream);
/* Same contract again (idx / zq / usage as lipvq_nearest_f32 with LIPVQ_DIST_NORM) with every row decided by the exact
 * re-scoring kernel: needs no prepared codebook.  For batches of a few thousand rows (training steps, where the codebook
 * changes every step).  Any D (tuned instances for 32 / 64 / 128 / 208, a generic kernel otherwise). */
int lipvq_nearest_rows_f32(const float* z, const float* codebook, int64_t* idx, float* zq, int64_t* usage, int64_t N,
                           int K, int D, void* stream);

/* The same decision for SMALL batches (the reference's training step and rollouts: B*T = 1 ... a few hundred rows) with the
 * whole chip busy: a workgroup scores 4 rows against 64 codes staged in LDS, the grid is (row groups) x (code groups), a row's
 * partial minima meet behind a counter.  dist: LIPVQ_DIST_NORM | LIPVQ_DIST_SQSUM.  Identical idx / zq / usage.
 * lipvq_nearest_small_supported: N <= 4096, D a multiple of 4 up to 512.
 * workspace: lipvq_nearest_small_workspace_bytes(N, K) bytes, 16-byte aligned, ZERO on entry; the call leaves it zero (one
 * zero-filled buffer serves every later call on a stream, whatever its shape). */
int lipvq_nearest_small_supported(int64_t N, int K, int D);
size_t lipvq_nearest_small_workspace_bytes(int64_t N, int K);
int lipvq_nearest_small_f32(const float* z, const float* codebook, int64_t* idx, float* zq, int64_t* usage, void* workspace,
                            int64_t N, int K, int D, int dist, void* stream);
/* The plain VQVAE's quantizer (reference robomimic/models/vq_vae/backbone.py:55-63: `(z_e.unsqueeze(1) - E).pow(2).sum(-1)`,
 * argmin) through the same two routes: idx / zq / usage exactly as lipvq_nearest_f32(.., LIPVQ_DIST_SQSUM).  The screen is the
 * same certified MFMA screen (its margin covers the sum rule's rounding too); uncertified rows are decided by the exact kernel in
 * torch's cascade-sum order, first minimum.  prep / workspace as for lipvq_nearest_screened_f32.  D in 1 ... 512. */
int lipvq_vq_nearest_screened_f32(const float* z, const float* codebook, const void* prep, int64_t* idx, float* zq,
                                  int64_t* usage, void* workspace, int64_t N, int K, int D, void* stream);
int lipvq_vq_nearest_rows_f32(const float* z, const float* codebook, int64_t* idx, float* zq, int64_t* usage, int64_t N,
                              int K, int D, void* stream);
/* Test hook: also dumps the approximate distances d~ [N][Kpad] (Kpad = K rounded up to 32) and takes
 * the error-bound factor gamma from the caller. */
int lipvq_screen_debug_f32(const float* z, const float* codebook, const void* prep, int64_t* idx, float* zq,
                           int64_t* usage, void* workspace, float* dtilde, float gamma, int64_t N, int K, int D,
                           void* stream);

/* ---- the metric's path in one launch: encode + quantize (v5:71-74), lipvq-vae_amd/csrc/lipvq_fused.hip ---- */

/* x [N][A] -> idx [N], zq [N][D] (may be NULL), usage [K] (may be NULL, accumulated), ze_out [N][D] (may be
 * NULL).  Same results as lipvq_mlp3_f32(gelu, gelu, sigmoid) followed by lipvq_nearest_f32(LIPVQ_DIST_NORM);
 * z_e stays in registers.  packed = lipvq_mlp3_pack_f32 of the encoder stack (A -> J0 -> J1 -> D, W2 already
 * Lipschitz-normalised); prep = lipvq_nearest_prepare_f32 of the codebook.  Supported: J0 = 64, J1 = 128
 * (the reference's widths), D in {32, 64, 128, 208} (208 = the width the reference itself runs, v5:89-92 / obs_nets.py:1225-1227:
 * its 112 KB of Lipschitz-layer weights are streamed through LDS), A <= 64 (D = 128, whose layer 2 stays in LDS: A <= 40).  raw6 = host array of the six device pointers {W0, b0, W1, b1,
 * W2 (normalised), b2}: the exact kernel re-encodes the few uncertified rows from x with them, so z_e is written to
 * HBM only when ze_out is given.  After the call the first int of `workspace` holds the number of rows the screen left to an
 * exact decision.  WORKSPACE CONTRACT (round 4): the first 64 bytes are a header whose counters are zero between calls -- zero a
 * fresh workspace ONCE with lipvq_tokenize_workspace_init (or a 64-byte memset); every lipvq_tokenize_* / lipvq_vq_tokenize_*
 * call leaves them at zero (its last kernel does that: no fill launch per call), and one that returns an error re-zeroes the
 * header.  One workspace serves one stream at a time.  Shapes that run the one-product screen (lipvq_screen_is_coarse) leave 10-20 % of the rows to the exact stage,
 * which then reads z_e rows: z_e is written to ze_out if given, else to a scratch inside the workspace -- which is why
 * lipvq_tokenize_workspace_bytes(N, D) always includes N x D floats (plus 72 bytes of row / candidate lists per row). */
int lipvq_tokenize_supported(int A, int J0, int J1, int D, int K);
int lipvq_tokenize_fast_supported(int A, int J0, int J1, int D, int K);      /* lipvq_tokenize_fast_f32: D in {32, 64, 128} */
size_t lipvq_tokenize_workspace_bytes(int64_t N, int D);
int lipvq_tokenize_workspace_init(void* workspace, void* stream);
int lipvq_tokenize_f32(const float* x, const float* packed, const float* const* raw6, const float* codebook,
                       const void* prep, int64_t* idx, float* zq, int64_t* usage, float* ze_out, void* workspace,
                       int64_t N, int A, int J0, int J1, int D, int K, void* stream);
/* MI355X devices hold different clocks under the same kernel, and two schedule choices of the fused launch (identical results) win
 * on some devices and lose on others (profiles/r04_i_clock_ab.txt).  This call measures the four combinations with the caller's
 * own arguments (those of lipvq_tokenize_f32) -- each warmed, then `launches` back-to-back calls between HIP events, two alternating
 * rounds, minimum per combination -- and keeps the fastest as the current device's setting for every later lipvq_tokenize_* call of
 * the process.  SYNCHRONOUS (waits for the stream), not capturable; every launch writes idx / zq / ze_out and accumulates into usage
 * as lipvq_tokenize_f32 does.  choice (may be NULL): defer_ze | nt_ze << 1; ms4 (may be NULL): ms per launch of the four.
 * Latent widths above 64 have no such choice (their instances fix both): the call returns at once with choice = -1.
 * A launch that stores no z_e at all has none either (width <= 64, at most 2048 codes under the three-product screen, ze_out NULL:
 * its rows are decided in place from registers): the one launch is timed once, ms4 carries that time four times, choice is the
 * library default and the device's setting stays as it was. */
int lipvq_tokenize_tune_f32(const float* x, const float* packed, const float* const* raw6, const float* codebook,
                            const void* prep, int64_t* idx, float* zq, int64_t* usage, float* ze_out, void* workspace,
                            int64_t N, int A, int J0, int J1, int D, int K, void* stream, int launches, int* choice, float* ms4);
/* The forward half of a training step in the same launch: lipvq_tokenize_f32 that also stores what autograd saves for
 * the backward of v5:71-74 -- z_e [N][D] and the pre-activations pre0 [N][J0], pre1 [N][J1], pre2 [N][D] (all required,
 * 16-byte aligned), bit-identical to lipvq_mlp3_f32(x, .., pre0, pre1, pre2). */
int lipvq_tokenize_train_f32(const float* x, const float* packed, const float* const* raw6, const float* codebook,
                             const void* prep, int64_t* idx, float* zq, int64_t* usage, float* ze_out, float* pre0,
                             float* pre1, float* pre2, void* workspace, int64_t N, int A, int J0, int J1, int D, int K,
                             void* stream);

/* The plain VQVAE's encode + quantize in ONE launch (reference robomimic/models/vq_vae/backbone.py:40-66: encoder = three
 * Linear + ReLU, `(z_e.unsqueeze(1) - E).pow(2).sum(-1)`, argmin, embedding lookup): the same persistent kernel with ReLU
 * activations and a per-row fp16 scale (a ReLU latent is unbounded).  packed = lipvq_mlp3_pack_f32 of the encoder (plain weights),
 * prep = lipvq_nearest_prepare_f32 of the embedding table, ze_out [N][D] REQUIRED (the straight-through value of vq:74 and the
 * exact stage read it).  Same results as lipvq_mlp3_f32(relu, relu, relu) + lipvq_nearest_f32(LIPVQ_DIST_SQSUM).  Shapes as
 * lipvq_tokenize_supported; workspace lipvq_tokenize_workspace_bytes(N, D). */
int lipvq_vq_tokenize_f32(const float* x, const float* packed, const float* codebook, const void* prep, int64_t* idx,
                          float* zq, int64_t* usage, float* ze_out, void* workspace, int64_t N, int A, int J0, int J1, int D,
                          int K, void* stream);
/* The same launch as the forward half of a VQVAE training step: also stores the three pre-activations pre0 [N][J0], pre1 [N][J1],
 * pre2 [N][D] (16-byte aligned) that lipvq_mlp3_bwd_f32 consumes -- bit for bit what lipvq_mlp3_f32 would save. */
int lipvq_vq_tokenize_train_f32(const float* x, const float* packed, const float* codebook, const void* prep, int64_t* idx,
                                float* zq, int64_t* usage, float* ze_out, float* pre0, float* pre1, float* pre2, void* workspace,
                                int64_t N, int A, int J0, int J1, int D, int K, void* stream);

/* ---- fast mode (opt-in): the encoder's three GEMMs on fp16 MFMAs with fp32 accumulation -- the half-precision
 * encoder of BASELINE.json's config 2 / SURVEY section 7.  NOT bit-identical to lipvq_tokenize_f32: a fraction of a
 * percent of the indices differ, always between near-equidistant codes (the flip rate is reported by bench.py and
 * bounded in tests/test_gpu_fast.py); z_q rows are exact codebook rows; the quantizer (screen + exact re-scoring) is the
 * parity one, applied to the fp16-encoder z_e; rows the screen cannot certify are decided by the exact kernel from the
 * fp32 encoder.  packed16: lipvq_mlp3_pack_f16_f32 of {W0, W1, W2 (normalised)} (lipvq_mlp3_packed_f16_bytes() bytes,
 * 16-byte aligned); `packed` still supplies the fp32 biases.  Same shapes as lipvq_tokenize_supported(). */
size_t lipvq_mlp3_packed_f16_bytes(int A, int J0, int J1, int D);
int lipvq_mlp3_pack_f16_f32(const float* W0, const float* W1, const float* W2, void* packed16, int A, int J0, int J1,
                            int D, void* stream);
int lipvq_tokenize_fast_f32(const float* x, const float* packed, const void* packed16, const float* const* raw6,
                            const float* codebook, const void* prep, int64_t* idx, float* zq, int64_t* usage,
                            void* workspace, int64_t N, int A, int J0, int J1, int D, int K, void* stream);

/* ---- backward (what autograd derives from v5:70-84 / vq:38-76) --------------------------- */

/* Backward-data of lipvq_mlp3_f32.  gy [N][J2] = dL/dy.  pre0/pre1/pre2 are the saved
 * pre-activations (pre2 may be NULL when act2 is the identity).  packed_bwd holds the transposed
 * weights (lipvq_mlp3_pack_bwd_f32; lipvq_mlp3_packed_bwd_floats() floats).  Outputs:
 *   g2 [N][J2] = gy * act2'(pre2)      (may be NULL; equal to gy when act2 is the identity)
 *   g1 [N][J1], g0 [N][J0]             dL/d(pre-activation) of layers 1 and 0
 *   gx [N][K0] = dL/dx                 (may be NULL: the last GEMM is then skipped) */
size_t lipvq_mlp3_packed_bwd_floats(int K0, int J0, int J1, int J2);
int lipvq_mlp3_pack_bwd_f32(const float* W0, const float* W1, const float* W2, float* packed, int K0,
                            int J0, int J1, int J2, void* stream);
/* Two stacks' backward packs in one launch (small training steps are launch-count bound). */
int lipvq_mlp3_pack_bwd2_f32(const float* aW0, const float* aW1, const float* aW2, float* a_packed, int aK0, int aJ0, int aJ1,
                             int aJ2, const float* bW0, const float* bW1, const float* bW2, float* b_packed, int bK0, int bJ0,
                             int bJ1, int bJ2, void* stream);
int lipvq_mlp3_bwd_f32(const float* gy, const float* pre0, const float* pre1, const float* pre2,
                       const float* packed_bwd, float* g2, float* g1, float* g0, float* gx, int64_t N,
                       int K0, int J0, int J1, int J2, int act0, int act1, int act2, void* stream);

/* lipvq_mlp3_f32 with the tokenizer's loss folded in (the decoder of backbone_lfqvae_v5.py:76-83 at large batches): besides y
 * and the saved pre-activations,
 *   out3[0] = mean((y - target)^2)            target [N][J2]   (the reconstruction error)
 *   out3[1] = mean((input rows - latent)^2)   latent [N][K0]   (input rows = x, or x[gather_idx[n]]: z_q against z_e)
 *   out3[2] = the loss, as lipvq_mse_pair_loss_f32 forms it from the two means (w, form)
 * summed in double by the kernel itself -- no second pass over the operands.  workspace: lipvq_mse_workspace_bytes().
 * ste_out [N][K0], optional: the stack then runs on latent + (input rows - latent) -- the plain VQVAE's straight-through value
 * z_e + (z_q - z_e).detach() of backbone.py:74, lipvq_ste_f32's two roundings -- and stores it there (out3[1] stays the mean over
 * the rows as given: z_q against z_e).
 * Large batches on the reference's hidden widths only: lipvq_mlp3_loss_supported() (LIPVQ_EUNSUPPORTED otherwise). */
int lipvq_mlp3_loss_supported(int64_t N, int K0, int J0, int J1, int J2);
int lipvq_mlp3_loss_f32(const float* x, const int64_t* gather_idx, const float* packed, float* y, float* pre0, float* pre1,
                        float* pre2, int64_t N, int K0, int J0, int J1, int J2, int act0, int act1, int act2,
                        const float* target, const float* latent, float* ste_out, float* out3, float w, int form,
                        void* workspace, void* stream);

/* The same chain with the VQ losses' gradient terms folded in (what autograd derives from backbone_lfqvae_v5.py:79-83 /
 * backbone.py:69-74 next to the stack's own backward; three lipvq_scaled_diff_f32 launches per step otherwise):
 *   in_b  != NULL:  gy := (in_alpha  * *gscale) * (act2(pre2) - B)   -- gy is not read; act2(pre2) is the forward's own output
 *                                                                       (z_e), re-evaluated from the saved pre-activation
 *   out_a != NULL:  gx := (out_alpha * *gscale) * (A - B) + gx
 * (one of the two per launch) with A / B the rows of out_a / in_b / out_b, [N][K0] ([N][J2] for in_b) floats, or -- when the
 * matching index vector is given -- rows of a table picked by it (z_q = codebook[idx] without materialising it).  gscale: device scalar or NULL (= 1).
 * Same numbers as lipvq_scaled_diff_f32 followed by lipvq_mlp3_bwd_f32.  Large batches on the reference's hidden widths
 * only: ask lipvq_mlp3_bwd_vq_supported() first (LIPVQ_EUNSUPPORTED otherwise). */
int lipvq_mlp3_bwd_vq_supported(int64_t N, int K0, int J0, int J1, int J2);
int lipvq_mlp3_bwd_vq_f32(const float* gy, const float* pre0, const float* pre1, const float* pre2,
                          const float* packed_bwd, float* g2, float* g1, float* g0, float* gx, int64_t N,
                          int K0, int J0, int J1, int J2, int act0, int act1, int act2,
                          const float* in_b, const int64_t* in_b_idx, float in_alpha, const float* out_a, const int64_t* out_a_idx, const float* out_b,
                          const int64_t* out_b_idx, float out_alpha, const float* gscale, void* stream);

/* Weight/bias gradient of one Linear layer:  gW [J][Kd] = G^T . act(H),  gb [J] = column sums of G.
 * G [N][J] = dL/d(pre-activation); H [N][Kd] = the layer's input, given as a saved pre-activation
 * plus the activation code h_act to re-apply (LIPVQ_ACT_NONE for raw inputs), or, with hidx,
 * rows H[hidx[n]] of a table (the codebook gather).  workspace: lipvq_wgrad_workspace_bytes(). */
size_t lipvq_wgrad_workspace_bytes(int64_t N, int J, int Kd);
int lipvq_wgrad_f32(const float* G, const float* H, const int64_t* hidx, int h_act, float* gW, float* gb,
                    void* workspace, int64_t N, int J, int Kd, void* stream);

/* Codebook gradient: gC[idx[n]] += g[n]  (the index_add_ behind v5:47 / vq:66).  gC [K][D] must be
 * zeroed by the caller.  Uses float atomics: the last bits may differ between runs. */
int lipvq_scatter_add_f32(const float* g, const int64_t* idx, float* gC, int64_t N, int K, int D,
                          void* stream);

/* The same sum, deterministically: rows are added in ascending row order per code (no atomics), so repeated runs give
 * bit-identical gradients (what torch.use_deterministic_algorithms(True) asks of index_add_).  gC is accumulated into. */
int lipvq_scatter_add_det_f32(const float* g, const int64_t* idx, float* gC, int64_t N, int K, int D, void* stream);

/* The same sum for a large batch without floating-point atomics (csrc/lipvq_scatter.hip): rows are counting-sorted by code
 * (stable), then
 *   sequential = 0: every code's rows are summed in segments of 256 rows in row order and the segment sums added in segment
 *                   order.  The order depends on (idx, N) only: repeated runs give bit-identical results;
 *   sequential = 1: one chain per (code, column) over ALL its rows in ascending row order -- the order of
 *                   lipvq_scatter_add_det_f32 and of torch's deterministic index_add_, bit for bit (a hot code is one long chain).
 * gC is accumulated into.  lipvq_scatter_add_sorted_supported: N >= 32768, K <= 16384.
 * workspace: lipvq_scatter_add_sorted_workspace_bytes() (0 when unsupported). */
int lipvq_scatter_add_sorted_supported(int64_t N, int K, int D);
size_t lipvq_scatter_add_sorted_workspace_bytes(int64_t N, int K, int D);
int lipvq_scatter_add_sorted_f32(const float* g, const int64_t* idx, float* gC, void* workspace, int64_t N, int K, int D,
                                 int sequential, void* stream);
/* The same scatter with the rows formed inside the summing kernel instead of read (the codebook gradient of a training step,
 * backbone_lfqvae_v5.py:81-83 / backbone.py:69-70, without its [N][D] intermediate):
 *   row n contributes  (alpha * *gscale) * (table[idx[n]] - ze[n])  (+ g[n] when g is not NULL)
 * with the roundings of lipvq_scaled_diff_f32; gscale: device scalar or NULL (= 1).  Same support, workspace and orders. */
int lipvq_scatter_add_sorted_vq_f32(const float* g, const float* ze, const float* table, float alpha, const float* gscale,
                                    const int64_t* idx, float* gC, void* workspace, int64_t N, int K, int D, int sequential,
                                    void* stream);

/* Backward of lipvq_lipschitz_scale_f32: gWn [D][H] -> gW [D][H], gci [D]. */
int lipvq_lipschitz_bwd_f32(const float* W, const float* ci, const float* gWn, float* gW, float* gci, int D,
                            int H, void* stream);

/* out = alpha * (gscale ? *gscale : 1) * (a - b) + (c ? c : 0): the d mse / d input terms of
 * v5:79-81 with the upstream gradient of the loss read from device memory (no host sync). */
int lipvq_scaled_diff_f32(const float* a, const float* b, const float* c, float alpha, const float* gscale,
                          float* out, int64_t n, void* stream);

/* ---- the step after the tokenizer: input embedding + interleave, lipvq-vae_amd/csrc/lipvq_embed.hip ----
 * ob = robomimic/models/obs_nets.py.  ob:2525-2543 input_embedding():
 *     e = embed_drop(embed_ln(embed_encoder(inputs) + time_embeddings))
 * ob:2580-2596: stack/view/cat of the three streams into transformer_embeddings [B][3T][E]
 *     (context_obs at 2t, context_actions at 2t+1, obs at 2T+t).
 * Dropout (ob:2541) is left to the caller: identity in eval, torch's own RNG in training. */

/* ob:2536  y [N][E] = x [N][Kin] . W [E][Kin]^T + b [E] (b may be NULL) -- the canonical Linear (one k-ordered fmaf
 * chain per output, fp32 MFMA).  Used (i) once per parameter update on the codebook
 * (x = codebook, N = K) to build the [K][E] table that replaces the Linear over the tokenizer's output rows, since
 * z_latent[n] = codebook[idx[n]] (v5:47,84); (ii) on rows that are not codebook rows (observation streams). */
int lipvq_linear_f32(const float* x, const float* W, const float* b, float* y, int64_t N, int Kin, int E,
                     void* stream);

/* ob:2537-2540 + ob:2584-2596  For n = b*T + t (n < N):
 *     out[b*out_batch_stride + t*out_t_stride + out_offset + e] =
 *         LayerNorm_e(src[idx ? idx[n] : n][e] + (pos ? pos[t][e] : 0)) * ln_w[e] + ln_b[e]
 * src [src_rows][E] is the table (idx = the tokenizer's int64 indices) or dense pre-LayerNorm rows (idx NULL).
 * pos [T][E] is the time embedding the reference adds (ob:2485-2523: nn.Parameter [1][T][E], nn.Embedding rows 0..T-1
 * or the sinusoidal table).  The strides/offset (in floats, multiples of 4) place each row directly in its interleaved
 * slot: context_actions use (3T*E, 2E, E), context_obs (3T*E, 2E, 0), obs (3T*E, E, 2T*E).  stats [N][2] (may be
 * NULL) receives (mean, rstd) for the backward.  E: multiple of 4, <= 1024.  An index outside [0, src_rows) yields a
 * NaN row (no fault). */
int lipvq_embed_rows_f32(const float* src, const int64_t* idx, const float* pos, const float* ln_w, const float* ln_b,
                         float eps, float* out, float* stats, int64_t N, int T, int E, int64_t src_rows,
                         int64_t out_batch_stride, int64_t out_t_stride, int64_t out_offset, void* stream);

/* Backward of lipvq_embed_rows_f32 (what autograd derives from ob:2536-2540).  gout is addressed like out.
 * ACCUMULATES (caller zero-fills): g_src [src_rows][E] (gradient of the table rows; with idx NULL it is written, not
 * accumulated), g_pos [T][E], g_lnw [E], g_lnb [E]; any of them may be NULL.  The Linear's own gradients follow from
 * g_src with lipvq_wgrad_f32 (g_src^T . codebook) and lipvq_linear_f32 (g_src . W). */
int lipvq_embed_rows_bwd_f32(const float* gout, const float* src, const int64_t* idx, const float* pos,
                             const float* stats, const float* ln_w, float* g_src, float* g_pos, float* g_lnw,
                             float* g_lnb, int64_t N, int T, int E, int64_t src_rows, int64_t out_batch_stride,
                             int64_t out_t_stride, int64_t out_offset, void* stream);

/* The same backward for a large batch of INDEXED rows without atomics on the table or the time embedding: a wave owns one time
 * step (its time-embedding gradient stays in registers), the rows' gradients are written once and summed per table row by the
 * counting-sort scatter (lipvq_scatter_add_sorted_f32): reproducible, and independent of how the indices are distributed
 * (the atomic kernel: 8.7 ms at N = 524 280, E = 512, T = 10; 55 ms when every row picks the same table row).  idx == NULL
 * (dense rows, N >= 32768): the row gradients are g_src itself, workspace may be NULL.  workspace: lipvq_embed_rows_bwd_workspace_bytes() (0 = unsupported: N < 32768 or more than 16384 table rows). */
int lipvq_embed_rows_bwd_ws_supported(int64_t N, int T, int E, int64_t src_rows);
size_t lipvq_embed_rows_bwd_workspace_bytes(int64_t N, int T, int E, int64_t src_rows);
int lipvq_embed_rows_bwd_ws_f32(const float* gout, const float* src, const int64_t* idx, const float* pos, const float* stats,
                                const float* ln_w, float* g_src, float* g_pos, float* g_lnw, float* g_lnb, void* workspace,
                                int64_t N, int T, int E, int64_t src_rows, int64_t out_batch_stride, int64_t out_t_stride,
                                int64_t out_offset, void* stream);

/* The same backward with the sums in a fixed order, for any N >= 1 (T <= 1024): no floating-point atomics, so repeated runs
 * give bit-identical g_pos, g_lnw, g_lnb and (but for the one case named below) g_src.  A wave owns one time step as in _ws; each workgroup leaves
 * its partial (g_pos, g_lnw, g_lnb) sums in the workspace and a second launch adds them in workgroup order (one writer per
 * address); indexed rows are summed per table row by lipvq_scatter_add_sorted_f32 where it is supported, else by
 * lipvq_scatter_add_det_f32 while src_rows * N * ceil(E / 256) <= 2^24 (its cost in index reads), else by lipvq_scatter_add_f32:
 * the one case in which g_src, and only g_src, is added with atomics, as lipvq_embed_rows_bwd_f32 adds it.  The outputs are accumulated into as above and g_pos / g_lnw / g_lnb must be 16-byte aligned.
 * snap != NULL: gout is read as gout * m of the in-kernel dropout source (site, p; see "in-kernel dropout for the embedding
 * stage"), snap == NULL: plain.  workspace: lipvq_embed_rows_bwd_det_workspace_bytes(N, T, E, src_rows, idx != NULL) bytes.
 * This is the route the Python module takes. */
size_t lipvq_embed_rows_bwd_det_workspace_bytes(int64_t N, int T, int E, int64_t src_rows, int indexed);
int lipvq_embed_rows_bwd_det_f32(const float* gout, const float* src, const int64_t* idx, const float* pos, const float* stats,
                                 const float* ln_w, float* g_src, float* g_pos, float* g_lnw, float* g_lnb, void* workspace,
                                 const int64_t* snap, uint32_t site, double p, int64_t N, int T, int E, int64_t src_rows,
                                 int64_t out_batch_stride, int64_t out_t_stride, int64_t out_offset, void* stream);

/* lipvq_linear_f32 with an activation epilogue: y = act(x . W^T + b); pre (may be NULL) receives the pre-activation
 * for the backward.  bin:29-30 (second Linear + GELU of AdaptiveBinActionEmbedding.output_layer). */
int lipvq_linear_act_f32(const float* x, const float* W, const float* b, float* y, float* pre, int64_t N, int Kin,
                         int E, int act, void* stream);

/* ---- the sibling tokenizer behind `bin_enabled` (obs_nets.py:1214-1217): AdaptiveBinActionEmbedding,
 *      bin = robomimic/models/bin_action/backbone.py; lipvq-vae_amd/csrc/lipvq_bin.hip ---- */

/* bin:37-40 update_running_stats(): running_min[i] = min(running_min[i], min_n actions[n][i]), running_max likewise,
 * updated IN PLACE (actions [N][A], buffers [A]). */
int lipvq_bin_minmax_f32(const float* actions, float* running_min, float* running_max, int64_t N, int A, void* stream);

/* bin:42-66 compute_bins() + discretize(): bins[i][n] = clamp(bucketize(actions[n][i], linspace(running_min[i],
 * running_max[i], num_bins + 1)) - 1, 0, num_bins - 1).  bins is int64 [A][N] (dimension-major: each dimension's
 * indices are contiguous; the reference's [N][A] stack is its transpose).  Bit-exact restatement of torch's linspace
 * rounding and lower-bound search.  A * (num_bins + 1) <= 4096. */
int lipvq_bin_discretize_f32(const float* actions, const float* running_min, const float* running_max, int64_t* bins,
                             int64_t N, int A, int num_bins, void* stream);

/* bin:42-53 compute_bins() alone: boundaries [A][num_bins + 1] = linspace(running_min[i], running_max[i], num_bins + 1). */
int lipvq_bin_boundaries_f32(const float* running_min, const float* running_max, float* boundaries, int A, int num_bins,
                             void* stream);

/* bin:77-86 embeddings + cat + output_layer[0..1]:  pre1[n][j] = b1[j] + sum_i P[i][bins[i][n]][j], h = gelu(pre1).
 * P [A][num_bins][H] = per-dimension product of the embedding table with its 64-column block of the first Linear's
 * weight (lipvq_linear_f32(emb_i, W1[:, 64 i : 64 i + 64], NULL)), rebuilt when a parameter changes.  h [N][H];
 * pre1 [N][H] may be NULL. */
int lipvq_bin_hidden_f32(const int64_t* bins, const float* P, const float* b1, float* h, float* pre1, int64_t N, int A,
                         int num_bins, int H, void* stream);

/* out = g * act'(pre), elementwise over n floats (backward of the GELUs of bin:28,30). */
int lipvq_act_bwd_f32(const float* g, const float* pre, float* out, int64_t n, int act, void* stream);

/* ---- the DEFAULT action branch (obs_nets.py:1244-1260, the `else` of the tokenizer switch; ob = robomimic/models/obs_nets.py):
 *      nn.Sequential(spectral_norm(Linear(A,64)), GELU, spectral_norm(Linear(64,128)), GELU, spectral_norm(Linear(128,D)),
 *                    nn.TransformerEncoder(TransformerEncoderLayer(d_model=D, nhead=8, dim_feedforward=256, activation="gelu"), 4),
 *                    Linear(D,D))
 *      called on the 2-D [B*T][A] action tensor (ob:1344), i.e. the encoder sees ONE unbatched sequence of S = B*T actions.
 *      Linears: lipvq_linear_act_f32 / lipvq_wgrad_f32 above.  lipvq-vae_amd/csrc/lipvq_xf.hip, lipvq-vae_amd/default_branch.py ---- */

/* ob:1253-1257 torch.nn.utils.spectral_norm (torch/nn/utils/spectral_norm.py compute_weight), W [J][K] = weight_orig,
 * u [J] = weight_u, v [K] = weight_v.  do_power_iteration (module.training): v = normalize(W^T u), u = normalize(W v)
 * (x / max(|x|, eps), one iteration) written back in place.  Always: sigma[0] = u . (W v), Wsn = W / sigma.  J, K <= 256. */
int lipvq_spectral_norm_f32(const float* W, float* u, float* v, float* Wsn, float* sigma, int J, int K,
                            int do_power_iteration, float eps, void* stream);
/* Backward of W -> Wsn with u, v held constant (as torch does):  gW = (gWsn - <gWsn, Wsn> u v^T) / sigma. */
int lipvq_spectral_norm_bwd_f32(const float* gWsn, const float* Wsn, const float* u, const float* v, const float* sigma,
                                float* gW, int J, int K, void* stream);

/* ob:1245-1258 nn.MultiheadAttention inside TransformerEncoderLayer on an unbatched sequence: qkv [S][3D] = in_proj(x)
 * (q | k | v column blocks; head h owns columns [h D/H, (h+1) D/H) of each), out [S][D] = concat_h softmax(Q_h K_h^T /
 * sqrt(D/H)) V_h, lse [H][S] = log-sum-exp of the scaled scores (for the backward).  keep [H][S][S] bytes (may be NULL):
 * the attention-probability dropout mask of training mode, kept entries scaled by 1 / keep_prob.  D/H <= 32. */
int lipvq_attention_f32(const float* qkv, float* out, float* lse, const unsigned char* keep, float keep_prob, int64_t S,
                        int D, int H, void* stream);
/* Its backward: gqkv [S][3D] from gout [S][D]; delta [H][S] is scratch. */
int lipvq_attention_bwd_f32(const float* qkv, const float* out, const float* gout, const float* lse, float* gqkv,
                            float* delta, const unsigned char* keep, float keep_prob, int64_t S, int D, int H, void* stream);

/* ob:1245 post-norm residual of TransformerEncoderLayer (norm_first = False), y = LayerNorm(a + b) * w + bias, and its backward:
 * lipvq_gpt_layernorm_f32 with s = NULL and lipvq_gpt_layernorm_bwd_f32 with gres = NULL, declared with the backbone below
 * (D is a multiple of 8 here, so every row width is a multiple of 4; those entry points want a, b, w, bias and the gradient
 * rows 16-byte aligned and answer LIPVQ_EINVAL otherwise -- a LayerNorm parameter that is a view into a flat buffer must start
 * at a multiple of 4 floats). */

/* ---- the transformer backbone (tf = robomimic/models/transformers.py; tf:321-440 GPT_Backbone, built at obs_nets.py:2453-2463
 *      with embed_dim 512, 8 heads, 6 layers, context 3 T = 30): pre-norm blocks x + attn(ln1(x)), x + mlp(ln2(x)), then output_ln.
 *      Linears: lipvq_linear_act_f32 / lipvq_wgrad_f32 above.  lipvq-vae_amd/csrc/lipvq_gpt.hip, lipvq-vae_amd/gpt.py ---- */

/* tf:173-201 SelfAttention.forward between the qkv Linear and the output Linear, for all B sequences and H heads in ONE launch:
 * qkv [B][L][3E] = q | k | v column blocks (tf:174 chunk), head h owns columns [h E/H, (h+1) E/H) of each (tf:175-177);
 * att = (q k^T) / sqrt(E/H) (tf:184); with causal != 0 key j is open to query i only for j <= i (tf:146-151, :189 masked_fill),
 * otherwise every key; softmax over keys (tf:190); out [B][L][E] = att v already in the layout of tf:201 (heads concatenated);
 * lse [B][H][L] = log-sum-exp of the masked scaled scores (for the backward).  keep [B][H][L][L] bytes (may be NULL): the
 * attn_dropout mask of training mode (tf:195), kept probabilities scaled by 1 / keep_prob, as in lipvq_attention_f32.
 * E/H is 16, 32 or 64; L <= 128 (longer: LIPVQ_EUNSUPPORTED); B == 0 or L == 0 is a no-op.  qkv and out 16-byte aligned. */
int lipvq_gpt_attention_f32(const float* qkv, float* out, float* lse, const unsigned char* keep, float keep_prob, int64_t B,
                            int L, int E, int H, int causal, void* stream);
/* The same causal forward for Lq NEW tokens behind P cached ones (a rollout step of a prompted policy: the prompt's keys and
 * values do not change during an evaluation).  prefix_qkv [Bp][P][3E] is the qkv tensor of the prefix as the qkv Linear wrote
 * it (q | k | v; only k and v are read), Bp == B or Bp == 1 (one prompt shared by every sequence); qkv [B][Lq][3E] and
 * out [B][Lq][E] hold the new tokens alone.  Query iq is open to all P prefix keys and to the new keys jq <= iq.  out is, bit
 * for bit, rows P .. P + Lq - 1 of lipvq_gpt_attention_f32 (causal, keep = NULL) on the concatenation [prefix | new] along L.
 * Forward only: no dropout mask, no lse.  E/H is 16, 32 or 64; 0 <= P, 0 <= Lq, P + Lq <= 128 (longer: LIPVQ_EUNSUPPORTED);
 * Bp other than B or 1: LIPVQ_EINVAL; B == 0 or Lq == 0 is a no-op; P == 0 (prefix_qkv may be NULL) is plain causal attention.
 * prefix_qkv, qkv and out 16-byte aligned. */
int lipvq_gpt_attention_prefix_f32(const float* prefix_qkv, const float* qkv, float* out, int64_t B, int64_t Bp, int P, int Lq,
                                   int E, int H, void* stream);
/* Its backward: gqkv [B][L][3E] from gout [B][L][E] and the forward's out, lse; delta [B][H][L] is scratch.  Two launches, no
 * atomics: the same bits on every run. */
int lipvq_gpt_attention_bwd_f32(const float* qkv, const float* out, const float* gout, const float* lse, float* gqkv,
                                float* delta, const unsigned char* keep, float keep_prob, int64_t B, int L, int E, int H,
                                int causal, void* stream);

/* The residual add and the LayerNorm that follows it, in one pass over rows of E floats (E % 4 == 0, E <= 1024), for both
 * modules: s = a + b (b may be NULL: s = a), y = LayerNorm(s) * w + bias.  The backbone (tf:300-301, :439) keeps s, the `x + ...`
 * of its pre-norm residual stream, and y is the next ln1 / ln2 / output_ln; the default branch's post-norm residual (ob:1245) passes
 * s = NULL and carries y on.  s [N][E] may be NULL (not stored); xhat [N][E] and rstd [N] (either may be NULL) are saved for the
 * backward.  N == 0: no-op. */
int lipvq_gpt_layernorm_f32(const float* a, const float* b, const float* w, const float* bias, float eps, float* s, float* y,
                            float* xhat, float* rstd, int64_t N, int E, void* stream);
/* Its backward: gs [N][E] = the LayerNorm's gradient with respect to s PLUS gres [N][E] (the residual stream's own incoming
 * gradient; NULL where nothing but the LayerNorm reads s, as in the default branch) -- the gradient of both a and b; gw [E],
 * gb [E] are WRITTEN, not accumulated: per-workgroup partial sums added in a fixed order, so the bits repeat from run to run.
 * workspace: lipvq_gpt_layernorm_bwd_workspace_bytes(N, E) bytes, any contents. */
size_t lipvq_gpt_layernorm_bwd_workspace_bytes(int64_t N, int E);
int lipvq_gpt_layernorm_bwd_f32(const float* gy, const float* xhat, const float* rstd, const float* w, const float* gres,
                                float* gs, float* gw, float* gb, void* workspace, int64_t N, int E, void* stream);

/* ---- in-kernel dropout for the backbone (GPTBackbone.set_dropout_source("kernel")): the three dropout sites of a block
 *      (tf:195 attn_dropout, tf:205 and tf:289 the two block-output dropouts) decided INSIDE the kernels that touch those elements.
 *      No mask tensor exists: every decision is a pure function of (seed, step, site, row, col), and the backward regenerates it.
 *      lipvq-vae_amd/csrc/lipvq_rng.h (generator and mapping, one header for device and host), lipvq-vae_amd/csrc/lipvq_gpt.hip (the
 *      backbone's kernels), lipvq-vae_amd/csrc/lipvq_rng.hip (lipvq_dropout_begin and the keep fields, shared by every module).
 *
 *      The mapping (the contract).  A site is a 2-D field of decisions.  With Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57,
 *      Weyl constants 0x9E3779B9 / 0xBB67AE85, 10 rounds; the Random123 known answers hold), the decision for element (row, col) is
 *          word  col & 3  of  philox(counter = (col >> 2, row, site, step & 0xffffffff), key = (seed & 0xffffffff, seed >> 32)).
 *      The element is KEPT iff word >= thr, thr = (uint32) floor(p * 2^32) formed in double, for 0 < p < 1; a kept element is
 *      multiplied by inv_keep = 1.0f / (float)(1.0 - p) -- the factor the keep-byte entry points form from keep_prob = 1 - p, so
 *      the two paths agree in bits for the same decisions.  rows >= 2^32: LIPVQ_EUNSUPPORTED.  p outside (0, 1): LIPVQ_EINVAL
 *      (no dropout is the caller's choice of the plain entry point).  Only the low 32 bits of `step` enter the counter: a
 *      (seed, site) pair's fields repeat after 2^32 steps.
 *      Fields.  Attention probabilities: row = (b H + h) L + i, col = j (the layout of the keep bytes [B][H][L][L]).  A branch of
 *      the residual stream: row = the row of [N][E], col = e.  GPTBackbone uses site 4 layer + 0 for a block's attention
 *      probabilities, 4 layer + 1 for its attention-output branch and 4 layer + 2 for its MLP branch.
 *
 *      State.  `state` is a device int64[2] = (seed, step).  lipvq_dropout_begin (one thread) copies it to `snap` (another device
 *      int64[2]) and stores step + 1 back.  Every dropout kernel of one forward call and of its backward reads that snap: a
 *      captured graph advances on every replay without the host, and a backward sees its own forward's step however many forwards
 *      ran in between. ---- */
int lipvq_dropout_begin(int64_t* state, int64_t* snap, void* stream);
/* The decisions of one site as bytes, out [rows][cols] = 1 kept / 0 dropped: what the kernels below decide, for tests and for
 * users who want to see a mask.  _u8 runs on the device from a snap; _host is the same header code on the host from (seed, step)
 * and makes no GPU call.  rows == 0 or cols == 0: no-op.  cols <= 2^32. */
int lipvq_dropout_keep_u8(const int64_t* snap, uint32_t site, int64_t rows, int64_t cols, double p, unsigned char* out, void* stream);
int lipvq_dropout_keep_host(uint64_t seed, uint64_t step, uint32_t site, int64_t rows, int64_t cols, double p, unsigned char* out);
/* lipvq_gpt_attention_f32 / _bwd_f32 with the attention-probability decisions of `site` drawn in the kernel (B H L < 2^32 rows):
 * the bits of the keep-byte form given the bytes of lipvq_dropout_keep_u8(snap, site, B H L, L, p) and keep_prob = (float)(1 - p).
 * A query row all of whose keys are dropped has a zero output row and its lse unchanged. */
int lipvq_gpt_attention_drop_f32(const float* qkv, float* out, float* lse, const int64_t* snap, uint32_t site, double p, int64_t B,
                                 int L, int E, int H, int causal, void* stream);
int lipvq_gpt_attention_bwd_drop_f32(const float* qkv, const float* out, const float* gout, const float* lse, float* gqkv,
                                     float* delta, const int64_t* snap, uint32_t site, double p, int64_t B, int L, int E, int H,
                                     int causal, void* stream);
/* lipvq_gpt_layernorm_f32 with the branch's dropout inside: s = a + b * m, m = inv_keep where (row, e) of `site` is kept and 0
 * where it is dropped (the product torch's dropout forms), y = LayerNorm(s) * w + bias.  b is required. */
int lipvq_gpt_layernorm_drop_f32(const float* a, const float* b, const float* w, const float* bias, float eps, const int64_t* snap,
                                 uint32_t site, double p, float* s, float* y, float* xhat, float* rstd, int64_t N, int E, void* stream);
/* Its backward.  With dropout on b the gradients of a and b differ: gs [N][E] is lipvq_gpt_layernorm_bwd_f32's (the gradient of
 * a), gbranch [N][E] = gs * m (the gradient of b) is written by the same launch from the regenerated decisions. */
int lipvq_gpt_layernorm_bwd_drop_f32(const float* gy, const float* xhat, const float* rstd, const float* w, const float* gres,
                                     const int64_t* snap, uint32_t site, double p, float* gs, float* gbranch, float* gw, float* gb,
                                     void* workspace, int64_t N, int E, void* stream);

/* ---- in-kernel dropout for the embedding stage and the default action branch (ICLInputEmbedding / DefaultActionNetwork
 *      .set_dropout_source("kernel")).  Generator, threshold, inv_keep, snap and the refusals (p outside (0, 1): LIPVQ_EINVAL;
 *      rows >= 2^32: LIPVQ_EUNSUPPORTED) are those of the section above; only the SITES are new.  The site is one 32-bit counter
 *      word, and the two modules take theirs from ranges the backbone's 4 layer + {0, 1, 2} cannot reach:
 *          LIPVQ_DROPOUT_SITE_EMBED              the dropout after the embedding LayerNorm.  Field: row = the OUTPUT row b S + s
 *                                                of the call's [B][S][E] result (S = 3T for forward, 2T for prompt_embedding, T
 *                                                for input_embedding*), col = e.
 *          LIPVQ_DROPOUT_SITE_DEFAULT + 4 layer + k   encoder layer `layer` of the default action branch:
 *              k = 0  attention probabilities, row = h S + q, col = key (the layout of the keep bytes [H][S][S])
 *              k = 1  dropout1, the attention-output branch: row of [S][D], col = d
 *              k = 2  dropout2, the FFN-output branch: the same field
 *              k = 3  dropout between linear1's GELU and linear2: row of [S][FF], col = f
 *      The site word enters every draw, so two modules whose states hold equal (seed, step) still draw unrelated fields. ---- */
#define LIPVQ_DROPOUT_SITE_EMBED 0x40000000u
#define LIPVQ_DROPOUT_SITE_DEFAULT 0x80000000u
/* lipvq_attention_f32 / _bwd_f32 with the attention-probability decisions of `site` drawn in the kernels (H S < 2^32 rows): the
 * bits of the keep-byte form given the bytes of lipvq_dropout_keep_u8(snap, site, H S, S, p) and keep_prob = (float)(1 - p),
 * for every head-width instance.  A query row all of whose keys are dropped has a zero output row and its lse unchanged. */
int lipvq_attention_drop_f32(const float* qkv, float* out, float* lse, const int64_t* snap, uint32_t site, double p, int64_t S,
                             int D, int H, void* stream);
int lipvq_attention_bwd_drop_f32(const float* qkv, const float* out, const float* gout, const float* lse, float* gqkv,
                                 float* delta, const int64_t* snap, uint32_t site, double p, int64_t S, int D, int H, void* stream);
/* lipvq_linear_act_f32 whose stored y is act(pre) * m, m = inv_keep where (row, col) of `site` is kept and 0 where it is dropped
 * (a product: a NaN at a dropped position stays a NaN).  pre is the plain pre-activation.  Same kernel choice, same chains. */
int lipvq_linear_act_drop_f32(const float* x, const float* W, const float* b, float* y, float* pre, const int64_t* snap,
                              uint32_t site, double p, int64_t N, int Kin, int E, int act, void* stream);
/* The first step of its backward in one launch: out [rows][cols] = lipvq_act_bwd_f32 of (g * m) at pre, m regenerated from
 * (snap, site, p).  act == LIPVQ_ACT_NONE gives g * m. */
int lipvq_act_bwd_drop_f32(const float* g, const float* pre, float* out, const int64_t* snap, uint32_t site, double p,
                           int64_t rows, int64_t cols, int act, void* stream);
/* lipvq_embed_rows_f32 that stores LayerNorm(...) * m.  The field row is the OUTPUT row of the slot,
 * (b out_batch_stride + t out_t_stride + out_offset) / E -- not the stream's own row number --, so the streams of one result
 * share one field; the strides and the offset must be multiples of E (LIPVQ_EINVAL).  stats stay the pre-dropout statistics. */
int lipvq_embed_rows_drop_f32(const float* src, const int64_t* idx, const float* pos, const float* ln_w, const float* ln_b,
                              float eps, float* out, float* stats, const int64_t* snap, uint32_t site, double p, int64_t N, int T,
                              int E, int64_t src_rows, int64_t out_batch_stride, int64_t out_t_stride, int64_t out_offset,
                              void* stream);
/* lipvq_embed_rows_bwd_f32 / _bwd_ws_f32 reading gout * m from the regenerated decisions (the same field, the same limits). */
int lipvq_embed_rows_bwd_drop_f32(const float* gout, const float* src, const int64_t* idx, const float* pos, const float* stats,
                                  const float* ln_w, float* g_src, float* g_pos, float* g_lnw, float* g_lnb, const int64_t* snap,
                                  uint32_t site, double p, int64_t N, int T, int E, int64_t src_rows, int64_t out_batch_stride,
                                  int64_t out_t_stride, int64_t out_offset, void* stream);
int lipvq_embed_rows_bwd_ws_drop_f32(const float* gout, const float* src, const int64_t* idx, const float* pos, const float* stats,
                                     const float* ln_w, float* g_src, float* g_pos, float* g_lnw, float* g_lnb, void* workspace,
                                     const int64_t* snap, uint32_t site, double p, int64_t N, int T, int E, int64_t src_rows,
                                     int64_t out_batch_stride, int64_t out_t_stride, int64_t out_offset, void* stream);

/* ---- the backbone's opt-in bf16 matrix-pipe mode (GPTBackbone.set_matmul_precision("bf16")): the three products of one
 *      nn.Linear on the bf16 MFMAs.  lipvq-vae_amd/csrc/lipvq_gemm_bf16.hip.
 *      Rounding rule: every tensor is fp32 in memory, as for the _f32 entry points; each element of the two MATRIX operands of
 *      a product is rounded to bf16 with round-to-nearest-even as it is read (nothing is truncated, nothing is stored as bf16).
 *      Accumulation: the bf16 x bf16 products are exact in fp32 and are accumulated in fp32 (v_mfma_f32_32x32x16_bf16); bias,
 *      activation, the sums over row chunks and the bias gradient are fp32 and never see a rounded operand.
 *      Determinism: no float atomics; the summation order depends on the shape alone, never on the device, its CU count or
 *      the launch's timing, so repeated calls give bit-identical results.  A row of y or gx has one chain over the reduction
 *      in the same order at every tile (lipvq_gemm_bf16_tile), so its bits depend neither on its position nor on the number
 *      of rows or output columns of the launch (tests/test_gpu_gemm_bf16_tiles.py compares the three tiles bit for bit).
 *      Special values: the rounding is IEEE -- ties to even, -0 stays -0, denormal operands are kept, NaN and +-Inf pass and
 *      reach only their own row (or column) of the result -- and it can OVERFLOW: an |element| from the bit pattern 0x7f7f8000
 *      (about 3.396e38) up, FLT_MAX among them, rounds to +-Inf in bf16, so an output is +-Inf or NaN here where the _f32
 *      entry point's is finite.
 *      Shapes: any N >= 0 (N == 0: no-op, returns 0); both Linear widths must be multiples of 8, else LIPVQ_EUNSUPPORTED.
 *      Input tensors (and the workspace) 16-byte aligned, else LIPVQ_EINVAL; outputs need no alignment.  Sizes are checked
 *      before pointers, pointers before any launch. ---- */

/* y [N][E] = act(x [N][Kin] . W [E][Kin]^T + b): lipvq_linear_act_f32 in the bf16 mode.  b may be NULL; pre (may be NULL)
 * receives the fp32 pre-activation; the activation is the fp32 function lipvq_linear_act_f32 applies (for GELU: the one whose
 * derivative lipvq_act_bwd_f32 evaluates at pre). */
int lipvq_linear_act_bf16(const float* x, const float* W, const float* b, float* y, float* pre, int64_t N, int Kin, int E,
                          int act, void* stream);
/* gx [N][K] = g [N][J] . W [J][K]: the input gradient of the Linear above with W read AS STORED (no transposed copy). */
int lipvq_linear_nn_bf16(const float* g, const float* W, float* gx, int64_t N, int J, int K, void* stream);
/* gW [J][K] = G [N][J]^T . H [N][K] (both rounded to bf16), gb [J] (may be NULL) = column sums of the UNROUNDED fp32 G.
 * The N rows are cut into chunks of
 *     chunk = max(64, 32 ceil(ceil(N / want) / 32)) rows,  want = max(1, floor(1024 / (ceil(J / 128) ceil(K / 128)))),
 * one launch writes every chunk's partial gW and gb into the workspace and a second adds them in chunk order;
 * lipvq_wgrad_bf16_workspace_bytes = ceil(N / chunk) (J K + J) 4 bytes (0 for N <= 0), a function of (N, J, K) only. */
size_t lipvq_wgrad_bf16_workspace_bytes(int64_t N, int J, int K);
/* The tile of the launch that computes an [M][Nc] result in `chunks` row chunks (1 for the forward and the input gradient;
 * ceil(N / chunk) for the weight gradient, whose result is gW: M = J, Nc = K), chosen from the shape alone:
 *     128 (128 x 128, 2 x 2 waves of 64 x 64) when the 128^2-grid (x row chunks), ceil(M / 128) ceil(Nc / 128) chunks, has
 *         >= 256 workgroups,
 *     64 (64 x 64, 2 x 2 waves of 32 x 32) else, if the 64^2-grid has >= 256,
 *     32 (32 x 32, one wave) else.
 * lipvq_linear_act_bf16, lipvq_linear_nn_bf16 and lipvq_wgrad_bf16 take their tile from this function.  Returns 0 for a non-positive argument.  Pure host
 * arithmetic: launches nothing, needs no device. */
int lipvq_gemm_bf16_tile(int64_t M, int Nc, int64_t chunks);
int lipvq_wgrad_bf16(const float* G, const float* H, float* gW, float* gb, void* workspace, int64_t N, int J, int K,
                     void* stream);

/* ---- the bf16x3 mode (GPTBackbone.set_matmul_precision("bf16x3"), what torch calls "bfloat16_3x"): the same three products
 *      with every fp32 operand element SPLIT into two bf16 numbers and three matrix-pipe products per fp32 product.  The same
 *      kernels (lipvq-vae_amd/csrc/lipvq_gemm_bf16.hip, SPLIT = true), arguments, validation, error codes, tile rule
 *      (lipvq_gemm_bf16_tile), chunk rule and workspace (lipvq_wgrad_bf16_workspace_bytes) as the _bf16 entry points above.
 *      Split: for an operand element v,  hi = bf16_rne(v),  lo = bf16_rne(v - float(hi));  the subtraction is exact in fp32;
 *      where hi is not finite, lo = 0.
 *      Product: C = sum_k (a_lo b_hi + a_hi b_lo + a_hi b_hi).  Each k-step of 16 of v_mfma_f32_32x32x16_bf16 runs three
 *      MFMAs into the same fp32 accumulator IN THIS ORDER -- a_lo b_hi, then a_hi b_lo, then a_hi b_hi -- at every tile
 *      instance, k-steps ascending, so a row's bits depend neither on its position nor on the tile it lands in, as above.
 *      Everything after the accumulator is fp32 and is the _bf16 code: bias, pre-activation, activation, the chunk-ordered
 *      reduce of the weight gradient; gb is the fp32 column sums of the UNROUNDED g.  No float atomics: results repeat bit
 *      for bit.
 *      Bound, for operand elements that are 0 or of normal magnitude with no bf16 overflow:
 *          |v - hi| <= 2^-8 |v|,   |v - hi - lo| <= 2^-16 |v|,   |lo| <= 2^-8 (1 + 2^-8) |v|,
 *      so the dropped a_lo b_lo term and the two residuals give  |a b - (three terms)| <= 3 2^-16 (1 + 2^-7) |a| |b|  per
 *      product, against 2^-8 (1 + 2^-9) |a| |b| in the bf16 mode; the fp32 accumulation of the 3 L terms of a reduction of
 *      length L adds at most (3 L + 1) 2^-24 sum(|a_hi b_hi| + |a_hi b_lo| + |a_lo b_hi|) under any-order round to nearest.
 *      Limits: an |element| >= (2 - 2^-8) 2^127 (bit pattern 0x7f7f8000 up, FLT_MAX among them) rounds to +-Inf as in the bf16
 *      mode; such an element, or a non-finite one, makes the outputs of its own line (its row of A or its column of B)
 *      non-finite -- NaN or +-Inf is not specified, because Inf x (lo = 0) is NaN -- and changes nothing outside that line.
 *      fp32-denormal operand elements keep only the bf16 mode's guarantee (their lo may be lost).  Both Linear widths must be
 *      multiples of 8. ---- */
int lipvq_linear_act_bf16x3(const float* x, const float* W, const float* b, float* y, float* pre, int64_t N, int Kin, int E,
                            int act, void* stream);
int lipvq_linear_nn_bf16x3(const float* g, const float* W, float* gx, int64_t N, int J, int K, void* stream);
int lipvq_wgrad_bf16x3(const float* G, const float* H, float* gW, float* gb, void* workspace, int64_t N, int J, int K,
                       void* stream);

/* ---- the policy's GMM output head (pn = robomimic/models/policy_nets.py; ob:747-771 ObservationDecoder's three Linears
 *      mean | scale | logits, pn:2545-2575 tanh / softplus + min_std / MixtureSameFamily, icl.py:947 log_prob, icl.py:966 the NLL,
 *      pn:2599 sample).  lipvq-vae_amd/csrc/lipvq_gmm.hip, lipvq-vae_amd/gmm.py.
 *      M = num_modes (1..16), A = ac_dim (1..64), P = M (2 A + 1) <= 512 columns mean [M][A] | scale [M][A] | logits [M];
 *      E % 4 == 0, E <= 1024; outside these limits: LIPVQ_EUNSUPPORTED.  Row n = (b, t) = (n / T, n % T) of the input is read at
 *      x + b bstride + t E floats (bstride % 4 == 0, x 16-byte aligned): the last T positions of a [B][3T][E] backbone output are
 *      x = out + 2 T E, bstride = 3 T E; a dense [N][E] input is T = N.  N == 0: no-op. ---- */
enum { LIPVQ_GMM_SOFTPLUS = 0, LIPVQ_GMM_EXP = 1, LIPVQ_GMM_LOW_NOISE = 2 };

/* One launch: pre = x W^T + b for the three Linears (Wm, Ws [M A][E], Wl [M][E]; the k-ordered fp32 chain of
 * lipvq_linear_act_f32, started from the bias), then per mode m and component a
 *     mu = tanh(pre_mean),  sigma = softplus(pre_scale) + min_std  (F.softplus: beta 1, identity above 20; LIPVQ_GMM_EXP:
 *     exp(pre_scale) + min_std; LIPVQ_GMM_LOW_NOISE: 1e-4, pn:2557),  l_m = sum_a [-(x_a - mu)^2 / (2 sigma^2) - log sigma - log(2 pi)/2],
 *     log_prob = logsumexp_m(log_softmax(logits)_m + l_m)          (both max-subtracted)
 * Every output may be NULL (not computed / not stored): log_prob [N] (needs actions [N][A]); pre [N][P] (kept for the backward);
 * mean [N][M][A], scale [N][M][A], logits [N][M] (raw) for a distribution object; lp_sum [1] = sum_n log_prob[n], formed from
 * per-workgroup partial sums in `workspace` (lipvq_gmm_workspace_bytes(N) bytes, any contents) by a second, one-workgroup launch
 * in a fixed order: no float atomics, the same bits on every run. */
size_t lipvq_gmm_workspace_bytes(int64_t N);
int lipvq_gmm_head_f32(const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws, const float* bs,
                       const float* Wl, const float* bl, const float* actions, float* log_prob, float* pre, float* mean,
                       float* scale, float* logits, float* lp_sum, void* workspace, int64_t N, int T, int E, int M, int A,
                       int scale_mode, float min_std, void* stream);
/* Its backward, one launch, no atomics: gpre [N][P] from the saved pre, the actions and the rows' upstream gradient
 * g[n] + gsum[0] (g [N] = gradient of log_prob, gsum [1] = gradient of lp_sum; either may be NULL, not both).  With the
 * responsibilities r_m = softmax_m(log pi_m + l_m):  d/dlogit_m = g (r_m - pi_m),  d/dpre_mean = g r_m (x - mu) / sigma^2 (1 - mu^2),
 * d/dpre_scale = g r_m ((x - mu)^2 / sigma^3 - 1 / sigma) sigma'  (sigma' = sigmoid(p), 1 above 20; exp(p); 0 in low-noise mode).
 * The Linear gradients are lipvq_wgrad_f32 (G = gpre) and lipvq_linear_act_f32 (gpre times the stacked weights). */
int lipvq_gmm_head_bwd_f32(const float* pre, const float* actions, const float* g, const float* gsum, float* gpre, int64_t N,
                           int M, int A, int scale_mode, float min_std, void* stream);
/* Backward of the mean / scale / logits outputs: gpre [N][P] = gmean (1 - tanh(pre)^2) | gscale sigma' | glogits (a NULL
 * gradient counts as zeros). */
int lipvq_gmm_params_bwd_f32(const float* pre, const float* gmean, const float* gscale, const float* glogits, float* gpre,
                             int64_t N, int M, int A, int scale_mode, void* stream);
/* pn:2599 .sample() in one launch (the forward's product and tile, another epilogue): the mode of row n is the first m with
 * u[n] < sum_{j <= m} softmax(logits)_j (the last mode if rounding leaves none), action [N][A] = mu_m + sigma_m eps[n][a].
 * u [N] uniform in [0, 1), eps [N][A] standard normal; no [N][M][A] tensor is formed. */
int lipvq_gmm_sample_f32(const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws, const float* bs,
                         const float* Wl, const float* bl, const float* u, const float* eps, float* action, int64_t N, int T,
                         int E, int M, int A, int scale_mode, float min_std, void* stream);

/* ---- in-kernel sampling (GMMActionHead.set_sample_source("kernel")): the sampling launch draws its uniform and its normals
 *      itself; no noise tensor exists and torch's generators are not touched.  lipvq-vae_amd/csrc/lipvq_rng.h (one header for
 *      device and host), lipvq-vae_amd/csrc/lipvq_gmm.hip.
 *
 *      The contract.  Generator, counter layout, key and state are those of "in-kernel dropout" above: the value for element
 *      (row, col) of a field comes from
 *          word  w = col & 3  of  philox(counter = (col >> 2, row, site, step & 0xffffffff), key = (seed & 0xffffffff, seed >> 32)),
 *      so one Philox call serves four neighbouring columns, and only the low 32 bits of `step` enter (step 2^32 + 1 draws what
 *      step 1 draws).
 *      Sites.  LIPVQ_SAMPLE_SITE_GMM = 0xC0000000 is the UNIFORM field: one column per row (col = 0, so word 0 of counter
 *      (0, row, site, step)).  LIPVQ_SAMPLE_SITE_GMM + 1 is the NORMAL field [rows][A]: col = the action component a.  Neither
 *      word is a dropout site (backbone 4 layer + {0, 1, 2} < 0x40000000, embedding 0x40000000, default branch 0x80000000 +
 *      4 layer + {0, 1, 2, 3} < 0xC0000000): a sampling state and a dropout state with equal (seed, step) draw unrelated fields.
 *      Row word.  Input row n = (b, t) = (n / T, n % T) of a [B][T] call draws at
 *          row = (uint32) (stream[b] T + t),
 *      `streams` a device int64[B] of per-environment stream ids that the kernel reads itself; streams == NULL means
 *      stream[b] = b.  The noise of an environment follows its id, not its batch position: a batch of ids (7, 3, 0) at one step
 *      draws, row for row, what three B = 1 calls with ids 7, 3 and 0 draw at that step.  The product is formed in unsigned 64-bit
 *      arithmetic and ONLY ITS LOW 32 BITS enter the counter: two (id, t) pairs with id T + t equal modulo 2^32 share their noise
 *      (ids below 2^32 / T never collide; a negative id counts as its two's-complement bit pattern).
 *      Uniform (the mode pick).   u = (float)(w >> 8) * 2^-24: in [0, 1), each value exact -- lipvq_gmm_sample_f32's `u`.
 *      Normal.   v = (float)(2 (w >> 9) + 1) * 2^-24: 2^23 values strictly inside (0, 1), each exact in fp32, symmetric about 1/2.
 *          eps = lq_normal_icdf(v) (lipvq_rng.h): Wichura's AS 241 PPND7 in fp32 with explicit fma, on min(v, 1 - v) and negated
 *          for v < 1/2: icdf(1 - v) == -icdf(v) in every bit, the result is finite for every word and non-decreasing in v, and
 *          device and host agree in every bit.  Within 2.4e-7 of the largest magnitude of the float64 inverse CDF over the whole
 *          grid.  TRUNCATION: |eps| <= icdf(1 - 2^-24) ~= 5.2947; the tail mass 2 Phi(-5.2947) ~= 1.2e-7 is never drawn.
 *          The evaluation, every operation one correctly rounded fp32 operation, fma(a, b, c) = a b + c rounded once, every
 *          constant the fp32 value nearest the decimal:
 *              w = v < 0.5 ? v : 1 - v;   q = 0.5 - w;
 *              q <= 0.425:  r = fma(-q, q, 0.180625)
 *                           n = fma(fma(fma(59.109374720, r, 159.29113202), r, 50.434271938), r, 3.3871327179)
 *                           d = fma(fma(fma(67.187563600, r, 78.757757664), r, 17.895169469), r, 1)
 *                           x = (q n) / d
 *              otherwise:   r = sqrt(L(1 / w)) - 1.6
 *                           n = fma(fma(fma(0.17023821103, r, 1.3067284816), r, 2.7568153900), r, 1.4234372777)
 *                           d = fma(fma(0.12021132975, r, 0.73700164250), r, 1);   x = n / d
 *              eps = v < 0.5 ? -x : x
 *          L(t) = log t for t >= 1 is lipvq_math.h's lq_logf_ge1: t = m 2^e, m in [1, 2) from the bit pattern; if
 *          m > 1.41421356237309504880 then m = 0.5 m, e = e + 1; s = (m - 1) / (m + 1); z = s s;
 *          p = fma(fma(fma(fma(0.19365468621253967, z, 0.2219124436378479), z, 0.28571757674217224), z, 0.3999999761581421), z,
 *          0.6666666865348816); lm = fma(s z, p, 2 s); L = fma(e, 0.693145751953125, fma(e, 1.42860682030941723e-6, lm)).
 *      Step.  `snap` is what one lipvq_dropout_begin launch on the module's sampling state (device int64[2] = seed, step) wrote:
 *      one such launch per sampling call hands it its (seed, step) and advances the step on the device, also in a captured graph. ---- */
#define LIPVQ_SAMPLE_SITE_GMM 0xC0000000u
/* lipvq_gmm_sample_f32 with u and eps drawn in the launch by the contract above (streams may be NULL): the bits of
 * lipvq_gmm_sample_f32 given the u and eps of lipvq_gmm_noise_f32(snap, streams, ..., N / T, T, A); streams holds one id per batch
 * entry, ceil(N / T) of them.  Same limits, same refusals, checked before any launch. */
int lipvq_gmm_sample_draw_f32(const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws, const float* bs,
                              const float* Wl, const float* bl, const int64_t* snap, const int64_t* streams, float* action, int64_t N,
                              int T, int E, int M, int A, int scale_mode, float min_std, void* stream);
/* The two fields written out, u [B T] and eps [B T][A]: what the launch above draws, for tests and for users who want to see the
 * noise.  _f32 runs on the device from a snap; _host is the same header code on the host from (seed, step) (streams then a host
 * pointer) and makes no GPU call.  B == 0: no-op.  A outside 1..64: LIPVQ_EUNSUPPORTED. */
int lipvq_gmm_noise_f32(const int64_t* snap, const int64_t* streams, float* u, float* eps, int64_t B, int T, int A, void* stream);
int lipvq_gmm_noise_host(uint64_t seed, uint64_t step, const int64_t* streams, int64_t B, int T, int A, float* u, float* eps);
/* out[i] = the normal that the raw 32-bit word words[i] maps to (v, then lq_normal_icdf), on the host. */
int lipvq_normal_icdf_host(const uint32_t* words, float* out, int64_t n);

/* ---- the deterministic policy's output head: what algo_factory (robomimic/algo/icl.py:41-75) builds when algo.gmm.enabled is
 *      False (config/icl_config.py:63, the default) -- ICLTransformer: the ObservationDecoder's one Linear `action`
 *      (obs_nets.py:747-771 with output_shapes = action (ac_dim,), pn:1683-1690), tanh (pn:1728-1731), and the losses of
 *      ICL._compute_losses (icl.py:174-202, weights icl_config.py:43-45): MSELoss, SmoothL1Loss (beta 1), cosine_loss on the first
 *      three components (utils/loss_utils.py:11-23) and their weighted sum.  lipvq-vae_amd/csrc/lipvq_action_head.hip,
 *      lipvq-vae_amd/action_head.py.
 *      A = ac_dim (1..64); E % 4 == 0, E <= 1024; outside these limits: LIPVQ_EUNSUPPORTED.  Rows are addressed as in the GMM
 *      head: row n = (b, t) = (n / T, n % T) at x + b bstride + t E floats (bstride % 4 == 0, x and W 16-byte aligned).
 *      Sizes are checked before pointers, pointers before any launch.  N == 0: no-op. ---- */

/* One launch: pre = x W^T + b (W [A][E]; the GMM head's product stage: the k-ordered fp32 chain of lipvq_linear_act_f32 started
 * from the bias, the reduction over E never split -- the same bits as lipvq_linear_act_f32), y = tanh(pre).  Every output may be
 * NULL: actions [N][A] = y; pre [N][A] (kept for the backward); losses [4] (needs target [N][A] and `workspace`,
 * lipvq_action_head_workspace_bytes(N) bytes, any contents) = with d = y - target, C = min(3, A), eps = 1e-8
 *     losses[0] = l2  = sum d^2 / (N A)
 *     losses[1] = l1  = sum smoothl1(d) / (N A)            smoothl1(d) = d^2 / 2 where |d| < 1, else |d| - 1/2
 *     losses[2] = cos = sum_n (1 - sim_n) / N               sim = sum_{c < C} (y_c / max(|y|, eps)) (target_c / max(|target|, eps)),
 *                                                           each norm over the first C components and clamped on its own
 *                                                           (torch's nn.CosineSimilarity): -mean(sim - 1)
 *     losses[3] = w2 l2 + w1 l1 + wc cos
 * formed from per-workgroup partial sums (three floats per 32 rows, rows in order) by a second, one-workgroup launch that adds
 * them in double in a fixed order: no float atomics, the same bits on every run. */
size_t lipvq_action_head_workspace_bytes(int64_t N);
int lipvq_action_head_f32(const float* x, int64_t bstride, const float* W, const float* b, const float* target, float* actions,
                          float* pre, float* losses, void* workspace, int64_t N, int T, int E, int A, float w2, float w1,
                          float wc, void* stream);
/* Its backward, one elementwise launch: gpre [N][A] = (gL + gy) (1 - y^2) with y = tanh(pre).  g [4] is the upstream gradient of
 * the four losses, a DEVICE tensor (needs target); with k2 = g[0] + g[3] w2, k1 = g[1] + g[3] w1, kc = g[2] + g[3] wc
 *     gL = k2 2 d / (N A) + k1 smoothl1'(d) / (N A) - [c < C] kc / N  d sim / d y_c        smoothl1'(d) = d inside the band, sign(d) outside
 *     d sim / d y_c = target_c / (n_y n_t) - [|y| > eps] sim y_c / |y|^2,   n = max(|.|, eps)
 * gy [N][A] is a gradient arriving at the `actions` output.  Either of g, gy may be NULL (counts as zeros), not both.
 * The Linear gradients are lipvq_wgrad_f32 (G = gpre) and lipvq_linear_act_f32 (gpre times the weight). */
int lipvq_action_head_bwd_f32(const float* pre, const float* target, const float* g, const float* gy, float* gpre, int64_t N,
                              int A, float w2, float w1, float wc, void* stream);

/* ---- the output heads' opt-in matrix-pipe modes (ActionHead / GMMActionHead.set_matmul_precision): the product stage of
 *      lipvq_action_head_f32, lipvq_gmm_head_f32, lipvq_gmm_sample_f32 and lipvq_gmm_sample_draw_f32 on the bf16 MFMAs.
 *      lipvq-vae_amd/csrc/lipvq_head_product.h (lq_head_product_bf16).  The _mp_f32 entry points below take the argument list of
 *      their _f32 namesake plus `matmul` before `stream`; LIPVQ_MATMUL_FP32 IS the _f32 entry point (which forwards with it):
 *      the same launches, the same bits.
 *      LIPVQ_MATMUL_BF16 / LIPVQ_MATMUL_BF16X3: the pre-activations [N][P] are, bit for bit, the first P columns of
 *      lipvq_linear_act_bf16 / lipvq_linear_act_bf16x3 (LIPVQ_ACT_NONE) on the dense rows of x and the head's weights and biases
 *      stacked in column order and extended with zero rows to a multiple of 8 (never formed: a column picks its row of its own
 *      Linear).  That is the contract of the two sections above: operands rounded to bf16, nearest even, as they are read (the
 *      split mode: hi and lo, lo = 0 where hi is not finite); accumulators start at 0; per output element ONE chain of
 *      v_mfma_f32_32x32x16_bf16 over k-steps of 16 in ascending order (split: a_lo b_hi, a_hi b_lo, a_hi b_hi per step), never
 *      split across waves; reduction elements past E and rows past N are zeros; the bias is added once, in fp32, after the chain
 *      (acc + bias -- the fp32 stage STARTS its chain from the bias).  A row's bits do not depend on N, on its position or on P.
 *      Everything after the pre-activations is the fp32 code of the _f32 entry point on the same values: tanh and the loss
 *      partial sums, the mixture's log_prob and its sum, mean / scale / logits, the inverse-CDF sample, the drawn sample.
 *      Special values and overflow as stated above: a NaN, an Inf or an |element| >= 0x7f7f8000 in a row of x makes that row's
 *      outputs non-finite (and what sums over the rows) and changes no other row.  The error bound of the split mode is the
 *      one of the bf16x3 section with a = x, b = W, L = E.
 *      Validation: the limits of the _f32 entry point; then a `matmul` outside the enum is LIPVQ_EINVAL and a bf16 mode with
 *      E % 8 != 0 is LIPVQ_EUNSUPPORTED; sizes are checked before pointers, pointers before any launch.
 *      The backward entry points are unchanged: they read the saved pre-activations.  In a bf16 mode the Linear gradients are
 *      lipvq_linear_nn_<mode> (gx = gpre times the stacked weights AS STORED) and lipvq_wgrad_<mode>, with gpre's columns and the
 *      stacked weight's rows extended with zeros to 8 ceil(P / 8) (zero lines add exact zeros) and the results cut. ---- */
enum { LIPVQ_MATMUL_FP32 = 0, LIPVQ_MATMUL_BF16 = 1, LIPVQ_MATMUL_BF16X3 = 2 };
int lipvq_action_head_mp_f32(const float* x, int64_t bstride, const float* W, const float* b, const float* target, float* actions,
                             float* pre, float* losses, void* workspace, int64_t N, int T, int E, int A, float w2, float w1,
                             float wc, int matmul, void* stream);
int lipvq_gmm_head_mp_f32(const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws, const float* bs,
                          const float* Wl, const float* bl, const float* actions, float* log_prob, float* pre, float* mean,
                          float* scale, float* logits, float* lp_sum, void* workspace, int64_t N, int T, int E, int M, int A,
                          int scale_mode, float min_std, int matmul, void* stream);
int lipvq_gmm_sample_mp_f32(const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws, const float* bs,
                            const float* Wl, const float* bl, const float* u, const float* eps, float* action, int64_t N, int T,
                            int E, int M, int A, int scale_mode, float min_std, int matmul, void* stream);
int lipvq_gmm_sample_draw_mp_f32(const float* x, int64_t bstride, const float* Wm, const float* bm, const float* Ws, const float* bs,
                                 const float* Wl, const float* bl, const int64_t* snap, const int64_t* streams, float* action, int64_t N,
                                 int T, int E, int M, int A, int scale_mode, float min_std, int matmul, void* stream);

/* icl.py:885-889, :970  optim.AdamW(vq_vae_model.parameters(), lr=1e-3, weight_decay=1e-4).step() for a LIST of tensors in
 * two launches (torch's foreach form is 8-10): params / grads / exp_avg / exp_avg_sq / steps are HOST arrays of `count`
 * DEVICE pointers (count <= 32), numels their element counts; steps[i] is a float32 device scalar (torch's capturable layout),
 * incremented here.  Standard AdamW (amsgrad off); the hyper-parameters are doubles (derived constants such as 1 - beta2 are
 * formed in double and rounded to fp32 once, as torch forms them).  workspace: lipvq_adamw_workspace_bytes() device bytes. */
size_t lipvq_adamw_workspace_bytes(void);
int lipvq_adamw_f32(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                    float* const* steps, const int64_t* numels, int count, double lr, double beta1, double beta2, double eps,
                    double weight_decay, void* workspace, void* stream);

/* torch_utils.py:196-234 backprop_for_loss (called at icl.py:215-226): clip_grad_norm_ over the whole parameter list, the sum of
 * p.grad.norm(2).pow(2) -- there one host synchronisation per parameter --, then optim.Adam.step() (icl_config.py:27,
 * torch_utils.py:108-113: Adam with L2, not AdamW).  Here without a host synchronisation; tensor lists as above (HOST arrays of
 * `count` <= 32 DEVICE pointers per call; a longer list takes several calls).
 *
 * Sum of squares: every element widened to double and squared (exact), summed in double into 64 slots per tensor, one per
 * workgroup, of a double workspace sized lipvq_grad_sumsq_workspace_bytes(tensors) for the WHOLE list of `tensors` gradients.  A
 * call covers list entries first ... first + count - 1 and writes their slots, all of them, so the workspace needs no
 * initialisation.  No atomics; which elements meet in which slot depends on the sizes (and each pointer's offset from a 16-byte
 * boundary) alone: the same bits on every run.  Any size >= 1, any 4-byte alignment; each gradient is read exactly once. */
size_t lipvq_grad_sumsq_workspace_bytes(int64_t tensors);
int lipvq_grad_sumsq_f32(const float* const* grads, const int64_t* numels, int count, int64_t first, int64_t tensors,
                         void* workspace, void* stream);
/* One small launch: sumsq = the slots of `tensors` gradients added in a fixed order, and the device record
 *     stats[0] = total_norm = sqrt(sumsq)           stats[1] = clip_coef = min(1, max_norm / (total_norm + 1e-6))
 *     stats[2] = sumsq                              stats[3] = sumsq_clipped = clip_coef^2 sumsq   (the reference's grad_norms)
 * -- torch.nn.utils.clip_grad_norm_ with error_if_nonfinite=False: a NaN norm gives a NaN coefficient, an infinite norm 0.
 * max_norm = +inf only reports (the coefficient is 1); negative or NaN: LIPVQ_EINVAL. */
int lipvq_clip_coef_f64(const void* workspace, int64_t tensors, double max_norm, double* stats, void* stream);
/* g *= (float)stats[1] in place for a list, the coefficient read on the device.  Always multiplies, as torch does (by 1.0f: exact). */
int lipvq_grad_scale_f32(float* const* grads, const int64_t* numels, int count, const double* stats, void* stream);
/* lipvq_adamw_f32's two launches (the same per-tensor step counters, the same bias-correction kernel, the same workspace) with
 *   decoupled  1: AdamW, the arithmetic of lipvq_adamw_f32 bit for bit.  0: torch.optim.Adam -- g' = g' + weight_decay p in fp32
 *              before the moments (not formed when weight_decay == 0), and no p *= 1 - lr weight_decay.
 *   lr_dev     NULL: the host double `lr` is used as in lipvq_adamw_f32.  Else a float32 device scalar read by the kernel (`lr`
 *              is ignored): a learning-rate schedule then reaches a step that was captured in a HIP graph.
 *   stats      NULL, or the record above: each gradient is read as g' = g (float)clip_coef, rounded to fp32 once -- the value
 *              lipvq_grad_scale_f32 would have stored; the gradient itself is left unscaled. */
int lipvq_adam_f32(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                   float* const* steps, const int64_t* numels, int count, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int decoupled, const float* lr_dev, const double* stats, void* workspace, void* stream);

/* ---- opt-in extension: EMA codebook update (not in the reference; named by BASELINE.json's north star) ----
 * cluster_size [K] and embed_sum [K][D] are the running statistics (updated in place), counts [K] int64 = this batch's
 * code usage (lipvq_nearest_f32 / lipvq_tokenize_f32 `usage`, summed over ranks), dw [K][D] = sum of the z_e rows mapped
 * to each code (lipvq_scatter_add_f32, summed over ranks).  Writes the new codebook:
 *     cluster_size = decay cluster_size + (1-decay) counts;  embed_sum = decay embed_sum + (1-decay) dw;
 *     n = sum cluster_size;  codebook[k] = embed_sum[k] / ((cluster_size[k] + eps) / (n + K eps) * n).
 * workspace: 8 bytes. */
int lipvq_ema_update_f32(float* cluster_size, float* embed_sum, const int64_t* counts, const float* dw, float* codebook,
                         float decay, float eps, int K, int D, void* workspace, void* stream);

/* ---- opt-in extension: data-dependent codebook initialisation and dead-code revival (not in the reference, whose own
 *      initialisation maps every row to one code: SURVEY 7; csrc/lipvq_kmeans.hip) ----
 * D^2 sampling.  Every row n of z [N][D] carries d[n], its comparison value under `dist` to the nearest code written so far
 * (LIPVQ_DIST_NORM: the norm of lq_sqdist8; LIPVQ_DIST_SQSUM: lq_sqdist32 -- what lipvq_nearest_f32 compares).  Its weight
 * w = d^2 (norm) or d (sum) is exact in fp64 and is turned into an integer q[n] = floor(ldexp(w, e)); e is fixed once, from the
 * first weights, as the largest integer with N ldexp(w_max, e) <= 2^62 (0 if w_max = 0), and rows whose d is not finite weigh 0.
 * A draw u in [0, 1) (fp64, from `draws`) picks, with Q = sum q and r = min(Q - 1, floor(u (double)Q)), the smallest n with
 * q[0] + ... + q[n] > r; row n is copied into the code bit for bit and every d[n] becomes min(d[n], dist(z[n], code)).
 * Q == 0 (no row differs from every code written) stops the draws: the remaining codes are left unchanged.
 * Outputs: picks [K] int64 (the row copied into code k, or -1), written [1] int64 (how many codes were written).
 * Nothing is read back to the host: a whole call can be captured in a HIP graph.  Two launches per code.
 * workspace: lipvq_kmeans_workspace_bytes(N, K) bytes, 8-byte aligned, any contents (the call initialises what it reads). */
size_t lipvq_kmeans_workspace_bytes(int64_t N, int K);
/* k-means++ seeding of codebook [K][D]: code 0 = row min(N - 1, floor(draws[0] N)), then code k (k = 1 ... K - 1) by the draw
 * draws[k].  draws [K] fp64. */
int lipvq_kmeans_seed_f32(const float* z, float* codebook, const double* draws, int64_t* picks, int64_t* written,
                          void* workspace, int64_t N, int K, int D, int dist, void* stream);
/* Dead-code revival.  d[n] starts as dist(z[n], codebook[idx[n]]) (idx [N] int64: each row's assigned code; an index outside
 * [0, K) weighs 0); the codes with counts[k] < threshold (counts [K] int64) are refilled in ascending code order, code k by the
 * draw draws[k] (draws [K] fp64), the first max_codes of them at most (pass K for all: launches grow with max_codes). */
int lipvq_kmeans_revive_f32(const float* z, float* codebook, const int64_t* idx, const int64_t* counts, int64_t threshold,
                            const double* draws, int64_t* picks, int64_t* written, void* workspace, int64_t N, int K, int D,
                            int dist, int max_codes, void* stream);
/* The Lloyd update: codebook[k] = sums[k] / (float)counts[k] (IEEE fp32 division) where counts[k] > 0, other codes untouched.
 * sums [K][D] = the per-code sums of the rows (lipvq_scatter_add_det_f32 / the sequential sorted route), counts [K] int64. */
int lipvq_kmeans_means_f32(float* codebook, const float* sums, const int64_t* counts, int K, int D, void* stream);

/* ---- multi-GPU: the path's only cross-GPU exchange (the reference is single-GPU,
 *      robomimic/utils/torch_utils.py:48-50, so there is no reference line to cite) ----
 * One process per GPU, rows sharded, parameters replicated.  Per batch the code-usage histogram (and, with the EMA
 * extension, the per-code sums) is summed over the ranks by RCCL over xGMI.  The library binds RCCL at run time
 * (dlopen of librccl.so.1 -- the copy PyTorch has already mapped when there is one, so both share one RCCL), hence the
 * tokenizer library itself loads on hosts without RCCL; these four entries then return LIPVQ_EUNSUPPORTED.
 *
 * lipvq_allreduce_counts takes ANY ncclComm_t (as void*): the application's own communicator, or one made by
 * lipvq_comm_init from a 128-byte unique id that rank 0 obtains with lipvq_comm_unique_id and hands to the other ranks
 * over any out-of-band channel (torch.distributed's store, a file, MPI).  In place, sum, enqueued on `stream`. */
#define LIPVQ_COMM_ID_BYTES 128
int lipvq_comm_unique_id(void* id128);
int lipvq_comm_init(void** comm, const void* id128, int rank, int world);
int lipvq_comm_destroy(void* comm);
int lipvq_allreduce_counts(int64_t* counts, int K, void* comm /* ncclComm_t */, void* stream);
/* the same for fp32 payloads (EMA per-code sums [K][D], flat data-parallel gradients) */
int lipvq_allreduce_f32(float* buf, int64_t n, void* comm /* ncclComm_t */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIPVQ_H_ */
