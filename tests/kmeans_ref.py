"""numpy restatement of the D^2 sampling rule of include/lipvq.h (lipvq_kmeans_*), for tests/test_*kmeans*.py.

Distances come from the CPU oracle (``CanonicalOracle.distances``: the tokenizers' comparison values), the integer weights from
np.ldexp / np.floor, the draws from a uint64 cumsum and searchsorted.  Sequential on purpose: it is the definition the GPU's
block-parallel sums have to meet bit for bit.
"""
from __future__ import annotations

import numpy as np

DIST_NORM, DIST_SQSUM = 0, 1
LIM = 2.0 ** 62


def weights(d, dist):
    """fp64 weights of comparison values d (d^2 for the norm rule, d for the sum rule; non-finite values weigh 0)."""
    d = np.asarray(d, np.float32).astype(np.float64)
    w = d * d if dist == DIST_NORM else d
    return np.where(np.isfinite(d), w, 0.0)


def scale_exponent(wmax, N):
    """The largest integer e with N ldexp(wmax, e) <= 2^62 in fp64 arithmetic (0 when wmax == 0)."""
    wmax = float(wmax)
    if wmax == 0.0:
        return 0
    _, x = np.frexp(wmax)
    lg = 0
    while (1 << lg) < N:
        lg += 1
    e = 62 - int(x) - lg
    assert float(N) * np.ldexp(wmax, e) <= LIM
    while float(N) * np.ldexp(wmax, e + 1) <= LIM:
        e += 1
    return e


def qweights(d, dist, e):
    return np.floor(np.ldexp(weights(d, dist), e)).astype(np.uint64)


def draw(q, u):
    """The row picked by draw u from integer weights q, or None when Q = sum q is 0."""
    c = np.cumsum(q, dtype=np.uint64)
    Q = c[-1]
    if Q == 0:
        return None
    r = np.uint64(np.floor(np.float64(u) * np.float64(Q)))
    r = min(Q - np.uint64(1), r)
    return int(np.searchsorted(c, r, side="right"))            # the smallest n with c[n] > r


def _dist_to(oracle, z, code, dist):
    return oracle.distances(z, code[None, :], dist)[:, 0]


def _draw_loop(oracle, z, cb, d, codes, draws, dist, e, picks):
    written = 0
    for k in codes:
        n = draw(qweights(d, dist, e), draws[k])
        if n is None:
            break
        cb[k] = z[n]
        picks[k] = n
        written += 1
        nd = _dist_to(oracle, z, cb[k], dist)
        d = np.where(nd < d, nd, d)
    return written


def seed(oracle, z, K, draws, dist, init=None):
    """(codebook, picks, written) of lipvq_kmeans_seed_f32."""
    z = np.ascontiguousarray(z, np.float32)
    N, D = z.shape
    cb = np.zeros((K, D), np.float32) if init is None else np.array(init, np.float32, copy=True)
    picks = np.full(K, -1, np.int64)
    r0 = min(N - 1, int(np.floor(np.float64(draws[0]) * np.float64(N))))
    cb[0] = z[r0]
    picks[0] = r0
    if K == 1:
        return cb, picks, 1
    d = _dist_to(oracle, z, cb[0], dist)
    e = scale_exponent(weights(d, dist).max(), N)
    return cb, picks, 1 + _draw_loop(oracle, z, cb, d, range(1, K), draws, dist, e, picks)


def revive(oracle, z, codebook, idx, counts, threshold, draws, dist, max_codes=None):
    """(codebook, picks, written) of lipvq_kmeans_revive_f32."""
    z = np.ascontiguousarray(z, np.float32)
    cb = np.array(codebook, np.float32, copy=True)
    K = cb.shape[0]
    picks = np.full(K, -1, np.int64)
    dead = [k for k in range(K) if counts[k] < threshold][: K if max_codes is None else max_codes]
    if not dead:
        return cb, picks, 0
    idx = np.asarray(idx, np.int64)
    inside = np.nonzero((idx >= 0) & (idx < K))[0]             # an index outside [0, K) weighs 0
    d = np.zeros(z.shape[0], np.float32)
    d[inside] = oracle.distances(z, cb, dist)[inside, idx[inside]]
    e = scale_exponent(weights(d, dist).max(), z.shape[0])
    return cb, picks, _draw_loop(oracle, z, cb, d, dead, draws, dist, e, picks)


def lloyd_step(oracle, z, codebook, draws, dist):
    """(codebook, idx, counts) of kmeans.lloyd_step: exact assignment, sequential fp32 sums, fp32 division, revival of the empty
    codes with threshold 1."""
    z = np.ascontiguousarray(z, np.float32)
    K = codebook.shape[0]
    idx, _, counts = oracle.nearest(z, codebook, dist)
    sums = np.zeros(codebook.shape, np.float32)
    np.add.at(sums, idx, z)                                    # unbuffered, in row order, fp32
    cb = np.array(codebook, np.float32, copy=True)
    live = counts > 0
    cb[live] = sums[live] / counts[live].astype(np.float32)[:, None]
    cb, _, _ = revive(oracle, z, cb, idx, counts, 1, draws, dist)
    return cb, idx, counts


# ---- inputs of the edge suites (tests/test_kmeans_host.py, tests/test_gpu_kmeans_edges.py) ------------------------------------

LAST = float(np.nextafter(1.0, 0.0))                           # the last double below 1
EDGE_DRAWS = np.array([0.0, 0.3, 0.6, LAST, 0.0, 0.5])


def scaled_rows(s, N=600, D=8, seed=0):
    """randn * s: s = 1e-22 puts every squared distance into the fp32 subnormals, 1e-30 makes all rows equal under both rules,
    1e15 / 1e18 push the scale exponent far below 0."""
    return (np.random.default_rng(seed).standard_normal((N, D)) * s).astype(np.float32)


def first_state(oracle, z, draws, dist):
    """(r0, d, e) after code 0 of a seeding: its row, every row's comparison value to it, the scale exponent."""
    N = z.shape[0]
    r0 = min(N - 1, int(np.floor(np.float64(draws[0]) * np.float64(N))))
    d = _dist_to(oracle, z, z[r0], dist)
    return r0, d, scale_exponent(weights(d, dist).max(), N)


def nonfinite_rows(N=600, D=8, seed=1):
    """Rows 3, 200 and 599 hold a NaN, an inf and 3e19 (whose squared difference overflows fp32): they weigh 0 for ever."""
    z = np.random.default_rng(seed).standard_normal((N, D)).astype(np.float32)
    z[3, 2], z[200, 0], z[N - 1, D - 1] = np.nan, np.inf, 3e19
    return z, (3, 200, N - 1)


def boundary_draws(q, n):
    """The two doubles next to c[n] / Q, c = cumsum(q): the draw below stops at row n, the one above at the next row that
    weighs something."""
    c = np.cumsum(q, dtype=np.uint64)
    u = np.float64(c[n]) / np.float64(c[-1])
    return float(np.nextafter(u, 0.0)), float(np.nextafter(u, 1.0))


def zero_run_rows(N=1500, D=8, seed=2, r0=100):
    """Rows 256..767 are copies of row r0: once r0 is a code, blocks 1 and 2 weigh nothing at all."""
    z = np.random.default_rng(seed).standard_normal((N, D)).astype(np.float32)
    z[256:768] = z[r0]
    return z, r0


ZERO_RUN_BOUNDARIES = (0, 99, 254, 255, 768, 1023, 1024, 1279, 1498)    # row 255: the next row that weighs something is 768
