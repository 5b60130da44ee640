// lipvq_rng.hip -- the module-independent entry points of the in-kernel random source (lipvq_rng.h; ABI: include/lipvq.h,
// "in-kernel dropout"): the state every dropout and sampling module advances once per call, and the decisions of a site as
// bytes (tests, users; no kernel of the library reads them).
//   lipvq_dropout_begin      snap = the state's (seed, step) as it was, step += 1 on the device: one one-thread launch
//   lipvq_dropout_keep_u8    the keep field of (snap, site, p) as [rows][cols] bytes, drawn on the device
//   lipvq_dropout_keep_host  the same field from (seed, step) with the header's host code: no GPU call
// The backbone, the embedding stage, the default action branch and the GMM head all call them.
#include "lipvq_common.h"
#include "lipvq_rng.h"

__global__ void dropout_begin_kernel(int64_t* __restrict__ state, int64_t* __restrict__ snap) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t seed = state[0], step = state[1];
    snap[0] = seed;
    snap[1] = step;
    state[1] = (int64_t)((uint64_t)step + 1u);
}

extern "C" int lipvq_dropout_begin(int64_t* state, int64_t* snap, void* stream) {
    if (!state || !snap) return fail(LIPVQ_EINVAL, "dropout_begin: null pointer");
    if (state == snap) return fail(LIPVQ_EINVAL, "dropout_begin: snap must not be the state itself");
    hipLaunchKernelGGL(dropout_begin_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, snap);
    return check_launch("dropout_begin");
}

// p first, then the sizes; the callers test their pointers after it
static int keep_field_args(const char* what, int64_t rows, int64_t cols, double p) {
    if (int rc = lq_dropout_check_p(what, p)) return rc;
    if (rows < 0 || cols < 0) return fail(LIPVQ_EINVAL, "%s: rows=%lld cols=%lld", what, (long long)rows, (long long)cols);
    if (rows >= (1LL << 32) || cols > (1LL << 32)) return fail(LIPVQ_EUNSUPPORTED, "%s: rows=%lld (< 2^32) cols=%lld (<= 2^32)", what, (long long)rows, (long long)cols);
    return 0;
}

// one thread per draw: columns 4 c4 .. 4 c4 + 3 of one row (inv_keep is not used: the output is the decisions)
__global__ __launch_bounds__(256) void dropout_keep_kernel(const int64_t* __restrict__ snap, uint32_t site, uint32_t thr, int64_t rows,
                                                           int64_t cols, int64_t cols4, unsigned char* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * cols4) return;
    const int64_t row = t / cols4, c4 = t % cols4;
    const lq_dropout dr = lq_dropout_load(lq_dropout_src{snap, site, thr, 1.0f});
    const uint32_t kb = lq_dropout_keep4(dr, (uint32_t)row, (uint32_t)c4);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * c4 + k < cols) out[row * cols + 4 * c4 + k] = (unsigned char)((kb >> k) & 1u);
}

extern "C" int lipvq_dropout_keep_u8(const int64_t* snap, uint32_t site, int64_t rows, int64_t cols, double p, unsigned char* out,
                                     void* stream) {
    if (int rc = keep_field_args("dropout_keep", rows, cols, p)) return rc;
    if (rows == 0 || cols == 0) return 0;
    if (!snap || !out) return fail(LIPVQ_EINVAL, "dropout_keep: null pointer");
    const int64_t cols4 = (cols + 3) / 4;
    if (rows > (0x7fffffffLL * 256) / cols4) return fail(LIPVQ_EUNSUPPORTED, "dropout_keep: rows=%lld cols=%lld is too large a field for one launch", (long long)rows, (long long)cols);
    hipLaunchKernelGGL(dropout_keep_kernel, dim3((unsigned)((rows * cols4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, snap, site,
                       lq_dropout_thr(p), rows, cols, cols4, out);
    return check_launch("dropout_keep");
}

// the same field from the header on the host: no GPU call
extern "C" int lipvq_dropout_keep_host(uint64_t seed, uint64_t step, uint32_t site, int64_t rows, int64_t cols, double p,
                                       unsigned char* out) {
    if (int rc = keep_field_args("dropout_keep_host", rows, cols, p)) return rc;
    if (rows == 0 || cols == 0) return 0;
    if (!out) return fail(LIPVQ_EINVAL, "dropout_keep_host: null pointer");
    const lq_dropout dr = lq_dropout_make(seed, step, site, p);
    for (int64_t row = 0; row < rows; ++row)
        for (int64_t c4 = 0; 4 * c4 < cols; ++c4) {
            const uint32_t kb = lq_dropout_keep4(dr, (uint32_t)row, (uint32_t)c4);
            for (int k = 0; k < 4 && 4 * c4 + k < cols; ++k) out[row * cols + 4 * c4 + k] = (unsigned char)((kb >> k) & 1u);
        }
    return 0;
}
