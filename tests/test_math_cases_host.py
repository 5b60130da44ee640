"""CPU: the case description of the canonical-math tests (math_cases.py) is what it claims, and the HOST build of lipvq_math.h keeps
on S and T the limits the device build is held to on every fp32 pattern (test_gpu_math_exhaustive.py).  float64 references: numpy and
scipy.  Each maximum is printed with the input that gives it (pytest -s)."""
import numpy as np
import pytest

import math_cases as M

_cache = {}


def _S():
    if "S" not in _cache:
        _cache["S"] = M.structured_set()
    return _cache["S"]


def _ST():
    if "ST" not in _cache:
        _cache["ST"] = np.concatenate([_S(), M.threshold_set()])
    return _cache["ST"]


def _host(oracle, name):
    """(patterns of S and T inside the function's domain, the host's result bits), computed once"""
    if name not in _cache:
        fn, dom = M.FUNCTIONS[name]
        bits = _ST()[dom(_ST())]
        _cache[name] = (bits, M.u32(oracle.math_probe(M.f32(bits), fn)))
    return _cache[name]


# ---- S and T ---------------------------------------------------------------------------------------------------------------------
def test_structured_set():
    S = _S().reshape(512, 1 << 15)
    assert S.size == 1 << 24
    assert np.array_equal(S >> np.uint32(23), np.broadcast_to(np.arange(512, dtype=np.uint32)[:, None], S.shape))
    mant = np.sort(S & np.uint32(0x007FFFFF), axis=1)
    assert (np.diff(mant.astype(np.int64), axis=1) > 0).all(), "a pattern occurs twice within a sign/exponent block"
    assert np.array_equal(mant[:, :1 << 13], np.broadcast_to(np.arange(1 << 13, dtype=np.uint32), (512, 1 << 13)))
    assert np.array_equal(mant[:, -(1 << 13):], np.broadcast_to(np.arange((1 << 23) - (1 << 13), 1 << 23, dtype=np.uint32), (512, 1 << 13)))
    mid = mant[:, 1 << 13:-(1 << 13)]
    assert mid.shape[1] == 1 << 14 and len(np.unique(mid[0])) == 1 << 14
    assert not np.array_equal(mid[0], mid[1]), "the drawn mantissas repeat from block to block"
    assert np.array_equal(_S(), M.structured_set()), "the draw is not reproducible"


def test_threshold_set(oracle):
    T = M.threshold_set()
    assert len(np.unique(T)) == len(T)
    for name, c in M.THRESHOLDS.items():
        b = int(M.u32(c).reshape(-1)[0])
        assert np.isin(np.arange(b - M.NEIGHBOURS, b + M.NEIGHBOURS + 1, dtype=np.int64).astype(np.uint32), T).all(), name
    assert np.isin(M.SPECIALS, T).all()
    nan = M.f32(M.SPECIALS)
    assert np.isnan(nan).sum() >= 6 and (M.SPECIALS[np.isnan(nan)] & np.uint32(0x00400000)).all(), "the NaNs are quiet ones"
    assert {int(s) >> 31 for s in M.SPECIALS[np.isnan(nan)]} == {0, 1}
    # each constant is the float its comparison flips at
    f = np.float32
    nxt = lambda v, to: np.nextafter(f(v), f(to))
    t = M.THRESHOLDS
    a_in, a_out = t["gelu: x*x < 18, last inside, x > 0"], t["gelu: x*x < 18, first outside, x > 0"]
    assert a_in * a_in < f(18) and not a_out * a_out < f(18) and nxt(a_in, np.inf) == a_out
    assert t["gelu: x*x < 18, last inside, x < 0"] == -a_in and t["gelu: x*x < 18, first outside, x < 0"] == -a_out
    assert t["exp: x > 88.72283 clamp"] == f(88.72283) and t["exp: x < -104 returns 0"] == f(-104)
    assert t["softplus: x <= 20"] == f(20) and t["erf: |x| < 3, x > 0"] == f(3) and t["erf: |x| < 4, x < 0"] == f(-4)
    # 1 + exp(x) == 1 starts inside the neighbourhood of -24 ln 2 (on the host's exp)
    nb = M.f32(M.neighbourhood(int(M.u32(t["softplus: 1 + exp(x) == 1"]).reshape(-1)[0])))
    one = (f(1) + oracle.math_probe(nb, 0)) == f(1)
    assert one.any() and not one.all()
    # the fold of lq_logf_ge1: the mantissa of sqrt 2, at two exponents
    m0, m10 = M.u32(t["logf_ge1: m > sqrt 2 fold, exponent 0"]).reshape(-1)[0], M.u32(t["logf_ge1: m > sqrt 2 fold, exponent 10"]).reshape(-1)[0]
    assert (m0 & 0x007FFFFF) == (m10 & 0x007FFFFF) and (m0 >> 23) == 127 and (m10 >> 23) == 137


def test_icdf_thresholds():
    th = M.icdf_thresholds()
    f = np.float32
    v = M.icdf_v
    assert v(th["icdf: v < 1/2, last"]) < f(0.5) <= v(th["icdf: v < 1/2, first past"])
    q = lambda k: f(0.5) - min(v(k), f(1) - v(k))
    assert q(th["icdf: q <= 0.425f, last tail (low)"]) > f(0.425) >= q(th["icdf: q <= 0.425f, first central (low)"])
    assert q(th["icdf: q <= 0.425f, last central (high)"]) <= f(0.425) < q(th["icdf: q <= 0.425f, first tail (high)"])
    w = M.icdf_threshold_words()
    assert len(np.unique(w)) == len(w) and not (w & np.uint32(0x1FF)).any()
    for name, k in th.items():
        assert np.isin((np.arange(k - M.NEIGHBOURS, k + M.NEIGHBOURS + 1) << 9).astype(np.uint32), w).all(), name


def test_every_branch_is_taken(oracle):
    """Every branch of every function of the two headers, named, is taken by at least one element of S and T (of the icdf's
    threshold words), judged by restating the comparison in fp32."""
    bits = _ST()
    x = M.f32(bits)
    f = np.float32
    with np.errstate(all="ignore"):
        nan, a, xx = np.isnan(x), np.abs(x), x * x
        e = oracle.math_probe(x, 0)
        u = f(1) + e
        mant = M.f32((bits & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000))
        ge1 = M.FUNCTIONS["logf_ge1"][1](bits)
        branches = {
            "exp: NaN returned": nan,
            "exp: x > 88.72283 clamped": x > f(88.72283),
            "exp: x < -104 gives 0": x < f(-104),
            "exp: main path, normal result": ~nan & (x <= f(88.72283)) & (x >= f(-87.3)),
            "exp: main path, denormal result": (x >= f(-104)) & (x < f(-87.4)),
            "erf: NaN returned": nan,
            "erf: |x| < 3 polynomial": a < f(3),
            "erf: 3 <= |x| < 4 through exp": (a >= f(3)) & (a < f(4)),
            "erf: |x| >= 4 gives +-1": a >= f(4),
            "gelu: x*x < 18 polynomial": xx < f(18),
            "gelu: tail, finite": ~(xx < f(18)) & ~nan & np.isfinite(x),
            "gelu: tail, NaN or inf": ~(xx < f(18)) & ~np.isfinite(x),
            "gelu_grad: erf polynomial branch": np.abs(x * f(0.70710678118654752440)) < f(3),
            "gelu_grad: erf exp branch": (np.abs(x * f(0.70710678118654752440)) >= f(3)) & (np.abs(x * f(0.70710678118654752440)) < f(4)),
            "gelu_grad: erf saturated, exp underflows to 0": f(-0.5) * xx < f(-104),
            "sigmoid: -x > 87 clamped": -x > f(87),
            "sigmoid: -x < -87 clamped": -x < f(-87),
            "sigmoid: unclamped": a <= f(87),
            "sigmoid: NaN falls through both clamps": nan,
            "softplus: !(x <= 20) returns x": ~(x <= f(20)) & ~nan,
            "softplus: NaN returns x": nan,
            "softplus: 1 + exp(x) == 1 returns exp(x)": (x <= f(20)) & (u == f(1)),
            "softplus: log1p path": (x <= f(20)) & (u != f(1)),
            "logf_ge1: m > sqrt 2 folded": ge1 & (mant > f(1.41421356237309504880)),
            "logf_ge1: m <= sqrt 2": ge1 & (mant <= f(1.41421356237309504880)),
            "logf_ge1: exponent 0": ge1 & ((bits >> np.uint32(23)) == 127),
            "logf_ge1: largest exponent": ge1 & ((bits >> np.uint32(23)) == 254),
            "sqrt: zero": a == 0, "sqrt: denormal": (x > 0) & (x < f(M.FLT_MIN)), "sqrt: normal": x >= f(M.FLT_MIN), "sqrt: NaN": nan,
        }
        w = M.icdf_threshold_words()
        v = M.icdf_v(w >> np.uint32(9))
        q = f(0.5) - np.where(v < f(0.5), v, f(1) - v)
        branches.update({
            "icdf: v < 1/2 (negated)": v < f(0.5), "icdf: v >= 1/2": v >= f(0.5),
            "icdf: central rational, v < 1/2": (q <= f(0.425)) & (v < f(0.5)), "icdf: central rational, v >= 1/2": (q <= f(0.425)) & (v >= f(0.5)),
            "icdf: tail rational, v < 1/2": (q > f(0.425)) & (v < f(0.5)), "icdf: tail rational, v >= 1/2": (q > f(0.425)) & (v >= f(0.5)),
        })
    missing = [name for name, m in branches.items() if not np.any(m)]
    assert not missing, missing


# ---- accuracy of the host build on S and T ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [k for k in M.LIMITS if not k.startswith("gelu_grad_dev")])
def test_host_accuracy(oracle, key):
    bits, got = _host(oracle, key.split(",")[0])
    worst, at, n, cls = M.measure(key, bits, got)
    print(f"\nhost, S and T: {key}: max {worst:.6g} at x = {M.f32([at])[0]!r} (0x{at:08X}), {n} patterns measured, "
          f"{cls} class mismatches, limit {M.LIMITS[key]}")
    assert n > 0 and cls == 0
    assert M.within(key, worst), (key, worst, hex(at))


def test_host_softplus_known_point(oracle):
    """the point that broke the earlier limit of 3 ulp is in S's range and is measured (3.13 ulp)"""
    x = np.array([-2.7698472], np.float32)
    worst, _, n, _ = M.measure("softplus, ulp", M.u32(x), M.u32(oracle.math_probe(x, 4)))
    print(f"\nhost: softplus at x = -2.7698472: {worst:.4f} ulp")
    assert n == 1 and 3.0 < worst <= M.LIMITS["softplus, ulp"]


def test_host_sqrt_is_correctly_rounded(oracle):
    bits, got = _host(oracle, "sqrt")
    with np.errstate(invalid="ignore"):
        want = np.sqrt(M.f32(bits).astype(np.float64)).astype(np.float32)      # rounding a double square root to fp32 is correctly rounded
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(M.f32(got)), nan) and np.array_equal(got[~nan], M.u32(want)[~nan])
    assert (M.f32(bits) < M.FLT_MIN).sum() > 1 << 14, "denormals are in the set"


# ---- identities the header states ------------------------------------------------------------------------------------------------
def test_host_sigmoid_is_one_over_one_plus_exp(oracle):
    bits, got = _host(oracle, "sigmoid")
    with np.errstate(invalid="ignore"):
        sel = np.abs(M.f32(bits)) <= np.float32(87.0)
    x = M.f32(bits[sel])
    want = np.float32(1.0) / (np.float32(1.0) + oracle.math_probe(-x, 0))
    bad = np.flatnonzero(got[sel] != M.u32(want))
    print(f"\nhost: lq_sigmoid against 1 / (1 + lq_expf(-x)) on {sel.sum()} points with |x| <= 87: {bad.size} mismatches")
    assert sel.sum() > 8_000_000 and bad.size == 0, [hex(int(b)) for b in bits[sel][bad[:8]]]


def test_host_gelu_is_its_two_branches(oracle):
    bits, got = _host(oracle, "gelu")
    inside = M.FUNCTIONS["gelu_poly"][1](bits)
    poly = M.u32(oracle.math_probe(M.f32(bits[inside]), 8))
    tail = oracle.math_probe(M.f32(bits[~inside]), 9)
    assert inside.sum() > 1 << 22 and (~inside).sum() > 1 << 22
    assert np.array_equal(got[inside], poly)
    g = M.f32(got[~inside])
    nan = np.isnan(tail)
    assert np.array_equal(np.isnan(g), nan) and np.array_equal(got[~inside][~nan], M.u32(tail)[~nan])


def test_host_special_values(oracle):
    f = np.float32
    p = lambda x, fn: oracle.math_probe(np.array(x, np.float32), fn)
    nans = M.f32(M.SPECIALS[np.isnan(M.f32(M.SPECIALS))])
    assert np.isnan(p(nans, 0)).all(), "exp(NaN) is NaN"
    top = p([88.72283], 0)[0]
    assert np.isfinite(top) and top > f(3.4e38), "exp(88.72283) is finite"
    assert (M.u32(p([np.inf, 1e30, 89.0], 0)) == M.u32([top])[0]).all(), "exp(+inf) = exp(88.72283)"
    below = np.nextafter(f(-104), f(-np.inf))
    assert M.u32(p([below, -1e30, -np.inf], 0)).tolist() == [0, 0, 0], "exp(x < -104) is +0"
    assert M.u32(p([np.inf, -np.inf, 4.0, -4.0], 1)).tolist() == M.u32(np.array([1, -1, 1, -1], f)).tolist(), "erf(+-inf) = +-1"
    assert M.u32(p([0.0, -0.0], 1)).tolist() == [0, 0x80000000], "erf keeps the sign of zero"
    assert np.isnan(p(nans, 1)).all()
    big = np.array([np.nextafter(f(20), f(np.inf)), 25.0, 1e30, np.inf], f)
    assert np.array_equal(M.u32(p(big, 4)), M.u32(big)), "softplus(x > 20) = x"
    assert np.isnan(p(nans, 3)).all(), "sigmoid(NaN) is NaN"
    assert np.isnan(p(nans, 4)).all() and np.isnan(p(nans, 2)).all() and np.isnan(p(nans, 5)).all() and np.isnan(p(nans, 9)).all()
    assert p([np.inf], 3)[0] == f(1) and 0 <= p([-np.inf], 3)[0] < f(2e-38), "sigmoid beyond the clamp: 1, or below 2e-38"
