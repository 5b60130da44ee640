"""GPU: the canonical arithmetic of lipvq_math.h (and lq_normal_icdf of lipvq_rng.h) as the DEVICE build computes it, on every fp32
bit pattern there is.  Every `==` between a kernel and the C oracle elsewhere in the suite rests on three claims that are checked
here directly, through the probe library (csrc/probe/lipvq_math_probe.hip, math_probe.py):

A. hipcc and gcc produce the same bits from the header: every scalar function, device against host, on S and T (math_cases.py); the
   icdf on all 2^23 words of its grid.
B. the device-only forms (packed pairs, four pairs in lockstep, the bare reciprocal, the straight-line GELU') return the bits of the
   scalar forms: exhaustive sweeps, the pattern under test in every element position, the other positions holding other values.
C. the functions are as accurate as the project says, against a float64 reference formed on the device (first held against numpy and
   scipy); fp32 division and square root are correctly rounded; denormals are kept.

Every sweep is one launch and prints how many patterns it evaluated; that count is asserted to be the size of the domain."""
import numpy as np
import pytest

import math_cases as M
import math_probe as P

pytestmark = pytest.mark.gpu

ALL = 1 << 32
NONFINITE = 1 << 24                                        # both signs: 2^23 mantissas at exponent 0xFF
NAN = NONFINITE - 2
SQ18_OUT = int(M.u32(M.THRESHOLDS["gelu: x*x < 18, first outside, x > 0"]).reshape(-1)[0])     # |x| patterns below it: x*x < 18
_cache = {}


def _ST():
    if "ST" not in _cache:
        _cache["ST"] = np.concatenate([M.structured_set(), M.threshold_set()])
    return _cache["ST"]


def _report(bits, dev, host, what):
    """device bits == host bits; a NaN only has to be a NaN"""
    nan = np.isnan(M.f32(host))
    bad = np.flatnonzero((np.isnan(M.f32(dev)) != nan) | (~nan & (dev != host)))
    lines = [f"x = 0x{int(bits[i]):08X} ({M.f32(bits[i:i + 1])[0]!r}): device 0x{int(dev[i]):08X}, host 0x{int(host[i]):08X}" for i in bad[:8]]
    assert bad.size == 0, f"{what}: {bad.size} of {bits.size} inputs differ\n" + "\n".join(lines)


# ---- A. device and host produce the same bits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.FUNCTIONS))
def test_device_equals_host(oracle, name):
    fn, dom = M.FUNCTIONS[name]
    bits = _ST()[dom(_ST())]
    dev = P.map_bits(fn, bits)
    host = M.u32(oracle.math_probe(M.f32(bits), fn))
    print(f"\nlq_{name}: device against host on {bits.size} patterns of S and T")
    _report(bits, dev, host, f"lq_{name}")


def test_device_gelu_grad_dev_against_host_gelu_grad(oracle):
    """lq_gelu_grad_dev has no host form: outside x*x < 18 it IS lq_gelu_grad (the host's bits); inside, it stays within the limit
    of the exhaustive sweep (test_gelu_grad_dev_against_gelu_grad) of the host's lq_gelu_grad."""
    bits = _ST()
    dev = P.map_bits(P.F_GELU_GRAD_DEV, bits)
    host = M.u32(oracle.math_probe(M.f32(bits), 5))
    inside = M.FUNCTIONS["gelu_poly"][1](bits)
    _report(bits[~inside], dev[~inside], host[~inside], "lq_gelu_grad_dev outside x*x < 18")
    d = np.abs(M.f32(dev[inside]).astype(np.float64) - M.f32(host[inside]).astype(np.float64))
    print(f"\nlq_gelu_grad_dev - host lq_gelu_grad on {inside.sum()} patterns with x*x < 18: max {d.max():.4g} "
          f"at 0x{int(bits[inside][np.argmax(d)]):08X}")
    assert M.within("gelu_grad_dev - gelu_grad, abs", d.max())


def test_device_icdf_equals_host_on_its_whole_grid():
    from lipvq_vae_amd import ops
    words = np.arange(M.ICDF_GRID, dtype=np.uint32) << np.uint32(9)
    dev = P.map_bits(P.F_ICDF_WORD, words)
    host = M.u32(ops.normal_icdf_host(words).numpy())
    print(f"\nlq_normal_icdf(lq_sample_open(w)): device against host on all {words.size} grid words")
    assert np.isfinite(M.f32(host)).all()
    _report(words, dev, host, "lq_normal_icdf")
    low = P.map_bits(P.F_ICDF_WORD, M.icdf_threshold_words() | np.uint32(0x1FF))      # the low nine bits of a word do not enter
    assert np.array_equal(low, dev[M.icdf_threshold_words() >> np.uint32(9)])


# ---- B. device forms against the scalar forms ------------------------------------------------------------------------------------
def _same(pair, what, first, count, done):
    r = P.same(pair, first, count)
    print(f"\n{what}: {r['done']} patterns compared, {r['skipped']} outside the domain, {r['bad']} differ"
          + ("" if r["first_bad"] is None else f" (lowest 0x{r['first_bad']:08X})"))
    assert r["done"] == done, f"{what}: {r['done']} patterns compared, the domain holds {done}"
    assert r["bad"] == 0, f"{what}: {r['bad']} of {r['done']} patterns differ, the lowest 0x{r['first_bad']:08X}"
    return r


def test_gelu_poly2_both_lanes():
    _same(P.P_GELU2, "lq_gelu_poly2 (either lane) against lq_gelu_poly", 0, ALL, ALL)


def test_gelu_poly2x4_all_eight_positions():
    _same(P.P_GELU2X4, "lq_gelu_poly2xN<4> (each of 8 positions) against lq_gelu_poly", 0, ALL, ALL)


def test_sigmoid2_finite_both_lanes():
    _same(P.P_SIG2, "lq_sigmoid2_finite (either lane) against lq_sigmoid", 0, ALL, ALL - NONFINITE)


def test_sigmoid2_finite_x4_all_eight_positions():
    _same(P.P_SIG2X4, "lq_sigmoid2_finite_xN<4> (each of 8 positions) against lq_sigmoid", 0, ALL, ALL - NONFINITE)


def test_rcp2_ge1_is_ieee_division():
    n = M.RCP_END - M.RCP_FIRST
    _same(P.P_RCP2, "lq_rcp2_ge1(d) (either lane) against 1.0f / d on [1, 2^126)", M.RCP_FIRST, n, n)
    r = P.same(P.P_RCP2, 0, ALL)                       # the domain is the kernel's own, too: everything else is skipped
    assert r["done"] == n and r["bad"] == 0


def test_sigmoid_is_one_over_one_plus_exp():
    _same(P.P_SIG_EXP, "lq_sigmoid(x) against 1.0f / (1.0f + lq_expf(-x)) on |x| <= 87", 0, ALL, 2 * (M.BITS_87 + 1))


def test_gelu_grad_dev_against_gelu_grad():
    _same(P.P_GRAD_TAIL, "lq_gelu_grad_dev against lq_gelu_grad where !(x*x < 18)", 0, ALL, ALL - 2 * SQ18_OUT)
    key = "gelu_grad_dev - gelu_grad, abs"
    r = P.err(P.E_GRAD_DEV, 0, ALL)
    print(f"\n|lq_gelu_grad_dev - lq_gelu_grad| where x*x < 18: {r['done']} patterns, max {r['max']:.4g} at 0x{r['at']:08X} "
          f"(x = {M.f32([r['at']])[0]!r}); limit {M.LIMITS[key]}")
    assert r["done"] == 2 * SQ18_OUT and r["bad"] == 0
    assert M.within(key, r["max"]), (r["max"], hex(r["at"]))


def test_nonfinite_acc2():
    _same(P.P_NONFINITE, "lq_nonfinite_acc2(x, 0) (either lane): +-0 for finite x, NaN for inf and NaN", 0, ALL, ALL)


# ---- C. accuracy and IEEE properties ---------------------------------------------------------------------------------------------
def test_device_float64_reference_against_numpy_and_scipy():
    """The reference the sweeps below measure against is independent of the code under test and right: ROCm's double exp, erf and
    log1p on S agree with numpy / scipy to a relative 1e-14 (to 1e-14 DBL_MIN where the result is a denormal double, whose own
    spacing is coarser than 1e-14 of it)."""
    from scipy import special
    S = M.structured_set()
    with np.errstate(all="ignore"):
        xd = M.f32(S).astype(np.float64)
        for what, fn, want in (("exp", P.D_EXP, np.exp(xd)), ("erf", P.D_ERF, special.erf(xd)), ("log1p", P.D_LOG1P, np.log1p(xd)),
                               ("sqrt", P.D_SQRT, np.sqrt(xd))):
            got = P.ref64(fn, S)
            tol = 1e-14 * np.maximum(np.abs(want), 2.2250738585072014e-308)
            ok = (np.isnan(got) & np.isnan(want)) | (got == want) | (np.abs(got - want) <= tol)
            rel = np.abs(got - want) / np.abs(want)
            rel = rel[np.isfinite(rel) & (np.abs(want) >= 2.2250738585072014e-308)]
            print(f"\ndevice float64 {what} against numpy/scipy on {S.size} points: max relative difference {rel.max():.3g}, "
                  f"{(~ok).sum()} outside 1e-14")
            bad = np.flatnonzero(~ok)
            assert bad.size == 0, (what, [(hex(int(S[i])), got[i], want[i]) for i in bad[:5]])


_ERR = {
    "exp, ulp, true result normal": P.E_EXP_NORMAL, "exp, abs, true result denormal": P.E_EXP_DENORMAL, "erf, abs": P.E_ERF,
    "gelu, abs": P.E_GELU, "gelu_grad, abs": P.E_GELU_GRAD, "sigmoid, ulp": P.E_SIGMOID, "softplus, ulp": P.E_SOFTPLUS,
    "logf_ge1, ulp": P.E_LOG_GE1,
}


def _first_false(pred, sign):
    """how many of the patterns sign | k, k = 0 .. 0x7F800000 (zero out to the infinity), satisfy pred, which holds up to some
    magnitude and not beyond: a bisection on numpy's float64 reference, independent of the code under test"""
    assert pred(M.f32([sign | 0])[0])
    if pred(M.f32([sign | 0x7F800000])[0]):
        return 0x7F800001
    lo, hi = 0, 0x7F800000                       # pred holds at lo, fails at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(M.f32([sign | mid])[0]) else (lo, mid)
    return hi


def _domain_sizes():
    """the number of patterns each sweep measures, from where numpy's float64 reference crosses the bound of its domain"""
    if "sizes" not in _cache:
        normal = lambda x: M.FLT_MIN <= M.reference("exp", x) <= M.FLT_MAX
        exp_pos, exp_neg = _first_false(normal, 0), _first_false(normal, 0x80000000)
        sig_neg = _first_false(lambda x: M.reference("sigmoid", x) > 1e-30, 0x80000000)
        sp_neg = _first_false(lambda x: M.reference("softplus", x) > 1e-30, 0x80000000)
        _cache["sizes"] = {
            "exp, ulp, true result normal": exp_pos + exp_neg,
            "exp, abs, true result denormal": 0x7F800001 - exp_neg,            # the rest of the negative patterns, -inf included
            "erf, abs": ALL - NONFINITE, "gelu, abs": ALL - NONFINITE, "gelu_grad, abs": ALL - NONFINITE,
            "sigmoid, ulp": 0x7F800001 + sig_neg,                              # +0 .. +inf (the reference is 1 there)
            "softplus, ulp": 0x7F800000 + sp_neg,                              # +0 .. FLT_MAX: at +inf the reference is infinite
            "logf_ge1, ulp": 0x7F800000 - 0x3F800000,
        }
    return _cache["sizes"]


@pytest.mark.parametrize("key", list(_ERR))
def test_accuracy_against_float64(key):
    name = key.split(",")[0]
    r = P.err(_ERR[key], 0, ALL, M.SIGN_FLOOR.get(name, 0.0))
    worst = r["max"] * 2.0 ** -149 if "denormal" in key else r["max"]
    print(f"\nlq_{name} against float64, {key}: {r['done']} patterns measured, {r['skipped']} outside, max {worst:.6g} "
          f"at 0x{r['at']:08X} (x = {M.f32([r['at']])[0]!r}), {r['bad']} class mismatches; limit {M.LIMITS[key]}")
    assert r["bad"] == 0, f"{key}: {r['bad']} results whose class (NaN, sign, infinity) differs from the reference's"
    assert r["done"] == _domain_sizes()[key], f"{key}: {r['done']} patterns measured, the domain holds {_domain_sizes()[key]}"
    msg = f"{key}: {worst!r} at 0x{r['at']:08X} exceeds {M.LIMITS[key]}"
    if "denormal" in key:
        msg += " -- results in the denormal range are off by more than two denormal steps: are denormals flushed to zero?"
    assert M.within(key, worst), msg


def test_gelu_grad_dev_against_float64():
    """lq_gelu_grad_dev's own error on x*x < 18 (elsewhere it is lq_gelu_grad, swept above), under lq_gelu_grad's stated limit"""
    key = "gelu_grad, abs"
    r = P.err(P.E_GRAD_DEV64, 0, ALL, M.SIGN_FLOOR["gelu_grad"])
    print(f"\nlq_gelu_grad_dev against float64 where x*x < 18: {r['done']} patterns measured, max {r['max']:.6g} at 0x{r['at']:08X} "
          f"(x = {M.f32([r['at']])[0]!r}), {r['bad']} class mismatches; limit {M.LIMITS[key]}")
    assert r["done"] == 2 * SQ18_OUT and r["bad"] == 0
    assert M.within(key, r["max"]), (r["max"], hex(r["at"]))


def test_sqrt_is_correctly_rounded():
    done = 0x7F800001 + 1 + NAN                        # +0 .. +inf, -0, the NaNs of both signs
    _same(P.P_SQRT, "lq_sqrt(x) against (float)sqrt((double)x), x >= 0 (denormals included) and NaN", 0, ALL, done)


def test_division_is_correctly_rounded():
    n = 1 << 30
    r = _same(P.P_DIV, "a / b against (float)((double)a / (double)b), both hashed from a counter", 0, n, n)
    denormal_in, nonfinite_in, denormal_out, nan_out = r["aux"]
    print(f"  pairs with a denormal operand {denormal_in}, with an infinite or NaN operand {nonfinite_in}, denormal quotients "
          f"{denormal_out}, NaN quotients {nan_out}")
    # a class that 1/256 of the bit patterns belong to occurs in about n / 128 of the pairs
    assert denormal_in > n // 256 and nonfinite_in > n // 256 and denormal_out > 1000 and nan_out > n // 256
    m = 0x7E800000 - 0x00800000
    _same(P.P_RCP_1PE, "1.0f / (1.0f + e) against double, every normal e below 2^126 (the sigmoid's range and beyond)", 0, ALL, m)
