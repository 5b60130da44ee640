/* lipvq_rng.h -- the counter-based generator behind the in-kernel dropout and, at the end of the file, the GMM head's in-kernel
 * sampling noise (uniform, and normal by an fp32 inverse CDF).
 *
 * ONE definition of Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the
 * Random123 known answers hold: tests/test_dropout_host.py) and of the mapping from a dropout SITE to its draws, shared
 * verbatim by the gfx950 device code (hipcc) and by the host (plain g++ / gcc), the way lipvq_math.h is.  Integer arithmetic
 * only: both sides agree in every bit.  The entry points that belong to no module (lipvq_dropout_begin, the keep fields as bytes)
 * are in lipvq_rng.hip.
 *
 * The contract (include/lipvq.h, "in-kernel dropout", repeats it).  A site is a 2-D field of decisions; the decision for
 * element (row, col) is word  col & 3  of
 *     philox4x32_10(counter = (col >> 2, row, site, step & 0xffffffff), key = (seed & 0xffffffff, seed >> 32))
 * and the element is KEPT iff  word >= thr,  thr = (uint32) floor(p * 2^32) formed in double (0 < p < 1).  One draw decides
 * four neighbouring columns.  rows < 2^32.  Only the low 32 bits of the step enter: the field repeats after 2^32 steps.
 *
 * Sites.  The backbone uses 4 layer + {0, 1, 2}; the embedding stage LIPVQ_DROPOUT_SITE_EMBED (0x40000000) and the default action
 * branch LIPVQ_DROPOUT_SITE_DEFAULT (0x80000000) + 4 layer + {0, 1, 2, 3} (include/lipvq.h lists the fields).  The site is a
 * counter word of every draw: modules whose states hold equal (seed, step) draw unrelated fields.
 */
#ifndef LIPVQ_RNG_H_
#define LIPVQ_RNG_H_

#include "lipvq_math.h"

#define LQ_PHILOX_M0 0xD2511F53u
#define LQ_PHILOX_M1 0xCD9E8D57u
#define LQ_PHILOX_W0 0x9E3779B9u
#define LQ_PHILOX_W1 0xBB67AE85u

typedef struct { uint32_t w[4]; } lq_philox4;

LQ_HD uint32_t lq_mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

LQ_HD lq_philox4 lq_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = lq_mulhi32(LQ_PHILOX_M0, c0), lo0 = LQ_PHILOX_M0 * c0;
        const uint32_t hi1 = lq_mulhi32(LQ_PHILOX_M1, c2), lo1 = LQ_PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += LQ_PHILOX_W0;                 /* (the bump after the last round is unused) */
        k1 += LQ_PHILOX_W1;
    }
    lq_philox4 out;
    out.w[0] = c0; out.w[1] = c1; out.w[2] = c2; out.w[3] = c3;
    return out;
}

/* what every dropout kernel of one forward call and of its backward is handed: the (seed, step) pair lipvq_dropout_begin
 * wrote, the site, the threshold and the factor of a kept element */
typedef struct {
    uint32_t k0, k1, step, site, thr;
    float inv_keep;
} lq_dropout;

/* thr and inv_keep of a drop probability 0 < p < 1: inv_keep is what the keep-byte path forms from keep_prob = (float)(1 - p) */
LQ_HD uint32_t lq_dropout_thr(double p) { return (uint32_t)(p * 4294967296.0); }
LQ_HD float lq_dropout_inv_keep(double p) { return 1.0f / (float)(1.0 - p); }

LQ_HD lq_dropout lq_dropout_make(uint64_t seed, uint64_t step, uint32_t site, double p) {
    lq_dropout d;
    d.k0 = (uint32_t)(seed & 0xffffffffu);
    d.k1 = (uint32_t)(seed >> 32);
    d.step = (uint32_t)(step & 0xffffffffu);
    d.site = site;
    d.thr = lq_dropout_thr(p);
    d.inv_keep = lq_dropout_inv_keep(p);
    return d;
}

/* the draw that decides columns 4 col4 .. 4 col4 + 3 of `row` */
LQ_HD lq_philox4 lq_dropout_draw(lq_dropout d, uint32_t row, uint32_t col4) {
    return lq_philox4x32_10(col4, row, d.site, d.step, d.k0, d.k1);
}

/* what a host entry point hands a dropout kernel: the snap lipvq_dropout_begin wrote (read on the device), the site, and the
 * threshold and factor of p */
typedef struct {
    const int64_t* snap;
    uint32_t site, thr;
    float inv_keep;
} lq_dropout_src;

LQ_HD lq_dropout_src lq_dropout_src_make(const int64_t* snap, uint32_t site, double p) {
    lq_dropout_src s;
    s.snap = snap; s.site = site; s.thr = lq_dropout_thr(p); s.inv_keep = lq_dropout_inv_keep(p);
    return s;
}

LQ_HD lq_dropout lq_dropout_load(lq_dropout_src s) {
    const uint64_t seed = (uint64_t)s.snap[0], step = (uint64_t)s.snap[1];
    lq_dropout d;
    d.k0 = (uint32_t)(seed & 0xffffffffu); d.k1 = (uint32_t)(seed >> 32); d.step = (uint32_t)(step & 0xffffffffu);
    d.site = s.site; d.thr = s.thr; d.inv_keep = s.inv_keep;
    return d;
}

/* bit w = the decision of column 4 col4 + w (1: kept) */
LQ_HD uint32_t lq_dropout_keep4(lq_dropout d, uint32_t row, uint32_t col4) {
    const lq_philox4 r = lq_dropout_draw(d, row, col4);
    return (uint32_t)(r.w[0] >= d.thr) | ((uint32_t)(r.w[1] >= d.thr) << 1) | ((uint32_t)(r.w[2] >= d.thr) << 2) |
           ((uint32_t)(r.w[3] >= d.thr) << 3);
}

/* ---- in-kernel sampling: the GMM head's noise (include/lipvq.h, "in-kernel sampling", repeats this contract).
 *
 * Two fields per sampling call, drawn with the dropout counter and key:
 *     word  col & 3  of  philox4x32_10((col >> 2, row, site, step & 0xffffffff), (seed & 0xffffffff, seed >> 32)).
 * Sites.  LIPVQ_SAMPLE_SITE_GMM (0xC0000000) is the UNIFORM field, one column (col = 0) per row: the mode pick.
 * LIPVQ_SAMPLE_SITE_GMM + 1 is the NORMAL field [rows][A]: col = the action component.  Neither word is reachable by a dropout
 * site (backbone 4 layer + k, embedding 0x40000000, default branch 0x80000000 + 4 layer + k).
 * Row word.  Input row (b, t) of a [B][T] call draws at  row = (uint32)(stream[b] T + t),  stream an int64[B] of per-environment
 * ids read on the device (NULL: stream[b] = b, the batch position).  The product is formed in 64 bits and only its low 32 bits
 * enter the counter: ids whose stream T + t agree modulo 2^32 share their noise.
 * Uniform.  u = (float)(w >> 8) 2^-24: 2^24 values in [0, 1), each exact.
 * Normal.   v = (float)(2 (w >> 9) + 1) 2^-24: 2^23 values strictly inside (0, 1), each exact, symmetric about 1/2;
 *           eps = lq_normal_icdf(v).  The grid truncates the normal: |eps| <= icdf(1 - 2^-24) ~= 5.2948, and the tail mass
 *           2 Phi(-5.2948) ~= 1.2e-7 is never drawn.
 * Step.  One lipvq_dropout_begin launch per sampling call hands it its (seed, step) snap and advances the step. */
#define LQ_SAMPLE_SITE_GMM 0xC0000000u

LQ_HD float lq_sample_uniform(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }
LQ_HD float lq_sample_open(uint32_t w) { return (float)(2u * (w >> 9) + 1u) * 5.9604644775390625e-8f; }

/* Inverse of the standard normal CDF at v in (0, 1): Wichura's PPND7 (Algorithm AS 241, Appl. Statist. 37 (1988) 477-484),
 * the central rational in r = 0.180625 - q^2 for |v - 1/2| <= 0.425 and the rational in sqrt(-log min(v, 1 - v)) - 1.6 outside.
 * AS 241's third branch (sqrt(-log) > 5, v < 1.4e-11) is unreachable from the grid above (sqrt(-log 2^-24) = 4.08) and is left
 * out: a v below 2^-24 is evaluated by the second rational, finite for every positive float.  Evaluated on w = min(v, 1 - v) and
 * negated for v < 1/2, so icdf(1 - v) == -icdf(v) in every bit (1 - v is exact on the grid).  Only +, *, fma, / and lq_sqrt,
 * and lq_logf_ge1(1 / w): hipcc and gcc agree in every bit. */
LQ_HD float lq_normal_icdf(float v) {
    const float w = v < 0.5f ? v : 1.0f - v;
    const float q = 0.5f - w;                                   /* >= 0, exact on the grid */
    float x;
    if (q <= 0.425f) {
        const float r = lq_fma(-q, q, 0.180625f);
        float n = lq_fma(5.9109374720e+01f, r, 1.5929113202e+02f);
        n = lq_fma(n, r, 5.0434271938e+01f);
        n = lq_fma(n, r, 3.3871327179e+00f);
        float d = lq_fma(6.7187563600e+01f, r, 7.8757757664e+01f);
        d = lq_fma(d, r, 1.7895169469e+01f);
        d = lq_fma(d, r, 1.0f);
        x = q * n / d;
    } else {
        const float r = lq_sqrt(lq_logf_ge1(1.0f / w)) - 1.6f;
        float n = lq_fma(1.7023821103e-01f, r, 1.3067284816e+00f);
        n = lq_fma(n, r, 2.7568153900e+00f);
        n = lq_fma(n, r, 1.4234372777e+00f);
        float d = lq_fma(1.2021132975e-01f, r, 7.3700164250e-01f);
        d = lq_fma(d, r, 1.0f);
        x = n / d;
    }
    return v < 0.5f ? -x : x;
}

/* the (seed, step) of a sampling call: the key and step words of lq_dropout, its site the uniform field's */
LQ_HD lq_dropout lq_sample_make(uint64_t seed, uint64_t step) { return lq_dropout_make(seed, step, LQ_SAMPLE_SITE_GMM, 0.5); }

/* the same from the snap lipvq_dropout_begin wrote, read where the noise is drawn */
LQ_HD lq_dropout lq_sample_load(const int64_t* snap) { return lq_sample_make((uint64_t)snap[0], (uint64_t)snap[1]); }

/* the row word of input row n = b T + t (see above) */
LQ_HD uint32_t lq_sample_row(const int64_t* streams, int64_t n, int T) {
    const int64_t b = n / T, t = n - b * T;
    const uint64_t id = streams ? (uint64_t)streams[b] : (uint64_t)b;
    return (uint32_t)(id * (uint64_t)T + (uint64_t)t);
}

LQ_HD float lq_sample_u(lq_dropout d, uint32_t row) {
    return lq_sample_uniform(lq_philox4x32_10(0u, row, LQ_SAMPLE_SITE_GMM, d.step, d.k0, d.k1).w[0]);
}

/* the draw behind the normals of components 4 col4 .. 4 col4 + 3 of `row` */
LQ_HD lq_philox4 lq_sample_eps_draw(lq_dropout d, uint32_t row, uint32_t col4) {
    return lq_philox4x32_10(col4, row, LQ_SAMPLE_SITE_GMM + 1u, d.step, d.k0, d.k1);
}

#endif
