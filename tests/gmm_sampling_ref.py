"""numpy restatement of the in-kernel sampling contract (include/lipvq.h, "in-kernel sampling") and the float64 moments of the
mixture the GMM head samples from.  Written from the header's text and tests/dropout_ref.py's Philox, not from csrc/lipvq_rng.h:
tests/test_gmm_sampling_host.py holds the library's host functions to it bit for bit -- u, and eps through an exact float32
restatement of the header's inverse CDF (fma32) -- and the transform to the float64 inverse CDF over the whole grid."""
import numpy as np
import torch

import dropout_ref
import gmm_ref

SITE_U = 0xC0000000                     # LIPVQ_SAMPLE_SITE_GMM: the uniform field, one column per row
SITE_EPS = SITE_U + 1                   # the normal field [rows][A]
MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF


def row_words(B, T, streams=None):
    """uint64 [B * T]: row = (uint32)(stream[b] T + t), the product taken modulo 2^64 first; streams None = arange(B)."""
    ids = list(range(B)) if streams is None else [int(s) for s in streams]
    assert len(ids) == B
    return np.array([(((s & MASK64) * T + t) & MASK64) & MASK32 for s in ids for t in range(T)], dtype=np.uint64)


def _key(seed):
    seed = int(seed) & MASK64
    return seed & MASK32, seed >> 32


def uniform_words(seed, step, B, T, streams=None):
    """uint32 [B * T]: word 0 of philox((0, row, SITE_U, step), key)."""
    return dropout_ref.philox4x32_10((0, row_words(B, T, streams), SITE_U, int(step) & MASK32), _key(seed))[0]


def normal_words(seed, step, B, T, A, streams=None):
    """uint32 [B * T, A]: word col & 3 of philox((col >> 2, row, SITE_EPS, step), key)."""
    row = row_words(B, T, streams)[:, None]
    col = np.arange(A, dtype=np.uint64)[None, :]
    words = dropout_ref.philox4x32_10((col >> np.uint64(2), row, SITE_EPS, int(step) & MASK32), _key(seed))
    pick = np.broadcast_to(col & np.uint64(3), (B * T, A)).astype(np.int64)
    return np.choose(pick, [np.broadcast_to(w, (B * T, A)) for w in words])


def uniform_of(words):
    """u = (w >> 8) 2^-24 as float32 (exact)."""
    return ((np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def open_of(words):
    """v = (2 (w >> 9) + 1) 2^-24 in float64 (exact there and in float32)."""
    return (2.0 * (np.asarray(words, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24


F32 = np.float32


def fma32(a, b, c):
    """float32 fused multiply-add, exactly: the product of two float32 is exact in float64; the float64 sum is rounded TO ODD
    (its rounding error comes from TwoSum), so the final rounding to float32 sees what the exact sum would show it."""
    a, b, c = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a * b
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, odd, s).astype(np.float32)


def logf_ge1(u):
    """The library's fp32 log of a finite float32 u >= 1 (csrc/lipvq_math.h lq_logf_ge1; include/lipvq.h spells it out)."""
    u = np.asarray(u, dtype=np.float32)
    b = u.view(np.uint32)
    e = (b >> np.uint32(23)).astype(np.int32) - 127
    m = ((b & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(np.float32)
    big = m > F32(1.41421356237309504880)
    m = np.where(big, F32(0.5) * m, m).astype(np.float32)
    e = e + big
    s = ((m - F32(1.0)) / (m + F32(1.0))).astype(np.float32)
    z = s * s
    r = np.full_like(s, F32(0.19365468621253967))
    for c in (0.2219124436378479, 0.28571757674217224, 0.3999999761581421, 0.6666666865348816):
        r = fma32(r, z, F32(c))
    lm = fma32(s * z, r, F32(2.0) * s)
    fe = e.astype(np.float32)
    return fma32(fe, F32(0.693145751953125), fma32(fe, F32(1.42860682030941723e-6), lm))


def normal_icdf32(v):
    """eps of the float32 grid point v, operation for operation as include/lipvq.h lists them (AS 241 PPND7 in fp32)."""
    v = np.asarray(v, dtype=np.float32)
    w = np.where(v < F32(0.5), v, F32(1.0) - v).astype(np.float32)
    q = (F32(0.5) - w).astype(np.float32)
    r = fma32(-q, q, F32(0.180625))
    n = fma32(F32(5.9109374720e+01), r, F32(1.5929113202e+02))
    n = fma32(n, r, F32(5.0434271938e+01))
    n = fma32(n, r, F32(3.3871327179e+00))
    d = fma32(F32(6.7187563600e+01), r, F32(7.8757757664e+01))
    d = fma32(d, r, F32(1.7895169469e+01))
    d = fma32(d, r, F32(1.0))
    centre = ((q * n).astype(np.float32) / d).astype(np.float32)
    wt = np.where(q <= F32(0.425), F32(0.25), w).astype(np.float32)       # (the tail formula is evaluated on tail arguments only)
    r = (np.sqrt(logf_ge1((F32(1.0) / wt).astype(np.float32))).astype(np.float32) - F32(1.6)).astype(np.float32)
    n = fma32(F32(1.7023821103e-01), r, F32(1.3067284816e+00))
    n = fma32(n, r, F32(2.7568153900e+00))
    n = fma32(n, r, F32(1.4234372777e+00))
    d = fma32(F32(1.2021132975e-01), r, F32(7.3700164250e-01))
    d = fma32(d, r, F32(1.0))
    tail = (n / d).astype(np.float32)
    x = np.where(q <= F32(0.425), centre, tail).astype(np.float32)
    return np.where(v < F32(0.5), -x, x).astype(np.float32)


def noise32(seed, step, B, T, A, streams=None):
    """(u float32 [B, T], eps float32 [B, T, A]): what lipvq_gmm_noise_* must write, bit for bit."""
    u = uniform_of(uniform_words(seed, step, B, T, streams)).reshape(B, T)
    v = open_of(normal_words(seed, step, B, T, A, streams)).astype(np.float32)
    return u, normal_icdf32(v).reshape(B, T, A)


def ndtri64(v):
    """float64 inverse normal CDF of v (a float64 array)."""
    return torch.special.ndtri(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))).numpy()


def noise(seed, step, B, T, A, streams=None):
    """(u float32 [B, T], v float64 [B, T, A], eps float64 [B, T, A]): the contract's uniform, the normal field's grid point and
    its float64 inverse CDF -- the ideal-grid reference of the library's fp32 eps."""
    u = uniform_of(uniform_words(seed, step, B, T, streams)).reshape(B, T)
    v = open_of(normal_words(seed, step, B, T, A, streams)).reshape(B, T, A)
    return u, v, ndtri64(v)


def std_normal_cdf(x):
    return 0.5 * torch.special.erfc(-torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)) / np.sqrt(2.0)).numpy()


def ks_distance(x):
    """Kolmogorov-Smirnov distance of the sample x (any shape) to the standard normal."""
    x = np.sort(np.asarray(x, dtype=np.float64).reshape(-1))
    n = x.size
    cdf = std_normal_cdf(x)
    return float(max((np.arange(1, n + 1) / n - cdf).max(), (cdf - np.arange(n) / n).max()))


def corr(a, b):
    """Sample correlation coefficient of two equally shaped arrays."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def chi2_quantile(df, prob=0.999):
    """The `prob` quantile of chi-squared with df degrees of freedom: bisection on the regularised lower incomplete gamma
    function P(df / 2, x / 2) in float64 (df = 2: -2 log(1 - prob) = 13.8155; df = 255: 330.52)."""
    a = torch.tensor(df / 2.0, dtype=torch.float64)
    lo, hi = 0.0, 10.0 * df + 100.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if float(torch.special.gammainc(a, torch.tensor(mid / 2.0, dtype=torch.float64))) < prob:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def chi2_uniform(u, buckets=256):
    """Pearson chi-squared of u in [0, 1) against `buckets` equal buckets."""
    counts = np.bincount(np.minimum((np.asarray(u, dtype=np.float64).reshape(-1) * buckets).astype(np.int64), buckets - 1), minlength=buckets)
    expect = counts.sum() / buckets
    return float(((counts - expect) ** 2 / expect).sum())


def mixture_moments(sd, feat, M, A, min_std=0.01, std_activation="softplus"):
    """float64 (pi [M], mu [M, A], sigma [M, A], mean [A], var [A], fourth central moment [A]) of the mixture at ONE feature row
    feat [E] (the head's state_dict in float64): per component a, x = mu_m + sigma_m eps with m ~ pi."""
    pm, ps, lg = gmm_ref.decoder(sd, feat.double().view(1, -1), M, A)
    mu, sg = gmm_ref.activate(pm, ps, min_std, std_activation)
    mu, sg, pi = mu[0], sg[0], torch.softmax(lg[0], -1)
    mean = (pi[:, None] * mu).sum(0)
    d = mu - mean
    var = (pi[:, None] * (sg ** 2 + d ** 2)).sum(0)
    m4 = (pi[:, None] * (d ** 4 + 6.0 * d ** 2 * sg ** 2 + 3.0 * sg ** 4)).sum(0)
    return pi.numpy(), mu.numpy(), sg.numpy(), mean.numpy(), var.numpy(), m4.numpy()


def modes_of(act, mu, sg, eps):
    """(modes [n], residual [n]): the mode whose mu_m + sigma_m eps reproduces each sampled row act [n, A] (float64), and how
    closely -- the picked mode read back from the kernel's own output."""
    act, eps = np.asarray(act, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    res = np.abs(act[:, None, :] - (mu[None] + sg[None] * eps[:, None, :])).max(-1)      # [n, M]
    return res.argmin(1), res.min(1)


def distribution_figures(act, modes, moments):
    """(z of the per-component sample means [A], z of the per-component sample variances [A], chi-squared of the mode counts):
    standard errors from the mixture's own float64 moments (mixture_moments)."""
    pi, _, _, mean, var, m4 = moments
    act = np.asarray(act, dtype=np.float64)
    n = act.shape[0]
    z_mean = (act.mean(0) - mean) / np.sqrt(var / n)
    z_var = (((act - mean) ** 2).mean(0) - var) / np.sqrt((m4 - var ** 2) / n)
    counts = np.bincount(np.asarray(modes), minlength=len(pi))
    chi2 = float(((counts - n * pi) ** 2 / (n * pi)).sum())
    return z_mean, z_var, chi2


def pick_modes(pi, u):
    """The inverse-CDF pick in float64: the first m with u < sum_{j <= m} pi_j, the last if none."""
    cdf = np.cumsum(np.asarray(pi, dtype=np.float64))
    return np.minimum((np.asarray(u, dtype=np.float64)[:, None] >= cdf[None, :]).sum(1), len(cdf) - 1)
