// lipvq_bf16_stage.h -- how an fp32 operand element becomes bf16 on its way into LDS, for every kernel of the bf16 / bf16x3
// matrix-pipe modes (lipvq_gemm_bf16.hip, lipvq_head_product.h): ONE rounding and ONE split, so that the kernels agree bit for
// bit (include/lipvq.h, the bf16 and bf16x3 sections).
#ifndef LIPVQ_BF16_STAGE_H_
#define LIPVQ_BF16_STAGE_H_
#include "lipvq_common.h"

#if defined(__HIPCC__)
typedef __bf16 lq_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 lq_bf16x8 __attribute__((ext_vector_type(8)));
typedef float lq_f32x2 __attribute__((ext_vector_type(2)));
typedef float lq_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t lq_u32x4 __attribute__((ext_vector_type(4)));

constexpr int GB_BK = 32;                  // reduction elements per staged step (two 32x32x16 MFMA steps)
constexpr int GB_LDK = 40;                 // bf16 per LDS row: 32 + 8 of padding (80 bytes)

// two floats -> two bf16, round to nearest even (v_cvt_pk_bf16_f32), low half first
__device__ __forceinline__ uint32_t gb_pk(float lo, float hi) {
    const lq_f32x2 f = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, lq_bf16x2));
}

// The residuals of the pair that gb_pk(a, b) rounded to `hi`: bf16(v - float(hi)) -- exact subtraction, one more rounding --
// and 0 where hi is not finite (Inf - Inf and NaN must not reach the lo image: the line is non-finite through hi alone).
__device__ __forceinline__ uint32_t gb_pk_lo(float a, float b, uint32_t hi) {
    const float ha = __builtin_bit_cast(float, hi << 16), hb = __builtin_bit_cast(float, hi & 0xffff0000u);
    const float la = __builtin_fabsf(ha) < __builtin_inff() ? a - ha : 0.0f;
    const float lb = __builtin_fabsf(hb) < __builtin_inff() ? b - hb : 0.0f;
    return gb_pk(la, lb);
}

// One 16-byte LDS write of eight reduction-consecutive floats as bf16: the hi image at s and (SPLIT) the lo image at s + lo_off.
template <bool SPLIT>
__device__ __forceinline__ void gb_stage8(unsigned short* __restrict__ s, int lo_off, float a0, float a1, float a2, float a3,
                                          float a4, float a5, float a6, float a7) {
    lq_u32x4 w;
    w.x = gb_pk(a0, a1); w.y = gb_pk(a2, a3); w.z = gb_pk(a4, a5); w.w = gb_pk(a6, a7);
    *reinterpret_cast<lq_u32x4*>(s) = w;
    if constexpr (SPLIT) {
        lq_u32x4 l;
        l.x = gb_pk_lo(a0, a1, w.x); l.y = gb_pk_lo(a2, a3, w.y); l.z = gb_pk_lo(a4, a5, w.z); l.w = gb_pk_lo(a6, a7, w.w);
        *reinterpret_cast<lq_u32x4*>(s + lo_off) = l;
    }
}

// A loaded vector with its lanes kept (m = ~0) or zeroed (m = 0).  A bit mask, not a select: hipcc turns `ok ? loaded : 0` into
// a branch around the load and then waits for every load on its own.
__device__ __forceinline__ lq_f32x4 gb_keep(lq_f32x4 r, uint32_t m) {
    return __builtin_bit_cast(lq_f32x4, __builtin_bit_cast(lq_u32x4, r) & m);
}
#endif

#endif
