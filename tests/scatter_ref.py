"""numpy restatement of the two sum orders of the counting-sort scatter-add (include/lipvq.h lipvq_scatter_add_sorted_f32,
lipvq_scatter_add_sorted_vq_f32, lipvq_scatter_add_det_f32), and the inputs of tests/test_gpu_scatter_edges.py.

sequential = 0: the rows of a code in ascending row order, cut into segments of 256; every segment one fp32 chain from +0.0f;
                gC[k] = ((gC0[k] + s_0) + s_1) + ... in segment order.
sequential = 1: one fp32 chain per code over all its rows in ascending row order, starting from gC0[k].
Row loops on purpose: np.sum adds pairwise.  tests/test_scatter_ref_host.py checks that the inputs built here can tell a wrong
row order, a wrong segment length and a wrong segment order from the right ones.
"""
from __future__ import annotations

import numpy as np

SEG = 256


def _per_code(idx, K):
    idx = np.asarray(idx, np.int64)
    order = np.argsort(idx, kind="stable")
    ends = np.cumsum(np.bincount(idx, minlength=K))
    return order, ends


def sorted_ref(g, idx, K, gC0=None, seg=SEG, mutate=None):
    """The sequential = 0 order.  mutate (host checks only): "reverse_rows" takes every code's rows in descending row order,
    "reverse_segments" adds every code's segment sums last to first."""
    g = np.ascontiguousarray(g, np.float32)
    D = g.shape[1]
    out = np.zeros((K, D), np.float32) if gC0 is None else np.array(gC0, np.float32, copy=True)
    order, ends = _per_code(idx, K)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in np.nonzero(np.diff(ends, prepend=0))[0]:
            rows = order[(ends[k - 1] if k else 0): ends[k]]
            if mutate == "reverse_rows":
                rows = rows[::-1]
            sums = []
            for s0 in range(0, len(rows), seg):
                s = np.zeros(D, np.float32)                    # +0.0f
                for n in rows[s0: s0 + seg]:
                    s += g[n]
                sums.append(s)
            if mutate == "reverse_segments":
                sums = sums[::-1]
            for s in sums:
                out[k] += s
    return out


def seq_ref(g, idx, K, gC0=None):
    """The sequential = 1 order (lipvq_scatter_add_det_f32, a sequential fp32 index_add_)."""
    g = np.ascontiguousarray(g, np.float32)
    out = np.zeros((K, g.shape[1]), np.float32) if gC0 is None else np.array(gC0, np.float32, copy=True)
    order, _ = _per_code(idx, K)
    idx = np.asarray(idx, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in order:                                        # per code: ascending row order
            out[idx[n]] += g[n]
    return out


def fold_rows(g, ze, table, idx, alpha, gscale):
    """The row values lipvq_scatter_add_sorted_vq_f32 forms, with its roundings: f = fp32(alpha * gscale) (alpha alone without
    gscale), d = f * (table[k] - ze[n]) as two rounded operations, then d + g[n] (d alone without g)."""
    ze, table = np.asarray(ze, np.float32), np.asarray(table, np.float32)
    f = np.float32(alpha) if gscale is None else np.float32(alpha) * np.float32(gscale)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = table[np.asarray(idx, np.int64)] - ze
        d = f * diff
        assert diff.dtype == np.float32 and d.dtype == np.float32
        return d if g is None else d + np.asarray(g, np.float32)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def code_bits_differ(a, b):
    """[K] bool: the codes of which at least one column differs in its bits."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) != b.view(np.uint32)).any(axis=1)


# ---- inputs -------------------------------------------------------------------------------------------------------------------

def wide_rows(rng, N, D):
    """randn * 10**U(-3, 3) per row: six decades of magnitudes, so that every change of order moves some column's bits."""
    return (rng.standard_normal((N, D)) * 10.0 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)


def idx_from_counts(rng, counts, N, hot):
    """[N] codes with exactly counts[k] rows of code k, code `hot` taking what is left, shuffled by a fixed permutation."""
    counts = np.array(counts, np.int64)
    assert counts.sum() <= N
    counts[hot] += N - counts.sum()
    idx = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    return idx[rng.permutation(N)], counts


ORDER_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 0, 1000)
ORDER_SEED = 1


def order_case(seed=ORDER_SEED, D=65, K=40):
    """N = 32768 + 13, K = 40 (or any K > 20): counts on both sides of the 16-row branch, FOLD's 32-row halves, the 64-row chunk
    and the 256-row segment; two empty codes; code 19 hot (most of the rest); the remainder spread at random over codes
    20..K-1."""
    rng = np.random.default_rng(seed)
    N, hot = 32768 + 13, 19
    counts = np.zeros(K, np.int64)
    counts[: len(ORDER_COUNTS)] = ORDER_COUNTS
    counts[20:] = rng.multinomial(3000, np.full(K - 20, 1.0 / (K - 20)))
    idx, counts = idx_from_counts(rng, counts, N, hot)
    g = wide_rows(rng, N, D)
    gC0 = wide_rows(rng, K, D)
    return g, idx, K, gC0, counts


COMBINE_SEGMENTS = (2, 15, 16, 17, 17)                         # the last one: 16 * 256 + 1 rows
COMBINE_SEED = 2


def combine_case(seed=COMBINE_SEED, D=65):
    """N = 32768 + 13, K = 12: codes 1..5 with exactly 2, 15, 16, 17 and 17 segments (the unrolled-by-16 combine loop and its
    tail), code 7 hot, the rest small."""
    rng = np.random.default_rng(seed)
    N, K, hot = 32768 + 13, 12, 7
    counts = np.zeros(K, np.int64)
    counts[1:6] = (2 * 256 - 3, 15 * 256, 16 * 256 - 100, 17 * 256, 16 * 256 + 1)
    counts[8:] = (40, 300, 0, 77)
    idx, counts = idx_from_counts(rng, counts, N, hot)
    g = wide_rows(rng, N, D)
    gC0 = wide_rows(rng, K, D)
    return g, idx, K, gC0, counts


def one_code_case(code, seed=3, D=5):
    """K = 2 with every row on one code, N = 32768 + 255: 129 segments."""
    rng = np.random.default_rng(seed + code)
    N = 32768 + 255
    return wide_rows(rng, N, D), np.full(N, code, np.int64), 2, wide_rows(rng, 2, D)


def block_rows(K):
    """Rows of a count / place block: 16, 4 or 2 waves of 512 rows, so that their K-int histograms fit the LDS."""
    return 8192 if K <= 2048 else (2048 if K <= 8192 else 1024)


def regime_case(K, N, seed=4, D=5):
    """Few used codes among K: 0 and K - 1, the neighbours of the code scan's thread, wave and 1024-code edges, and some at
    random; code K - 1 hot (most rows, >= 3 segments), code 0 two segments, the rest under 40 rows; all other codes empty
    (for K > 3)."""
    rng = np.random.default_rng(seed + K + N)
    edges = {1, 63, 64, 65, 511, 512, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 8191, 8192, K // 2, K - 2}
    used = sorted({k for k in edges if 0 < k < K - 1 and K > 3} | {int(k) for k in rng.integers(1, max(2, K - 1), 12) if K > 3})
    counts = np.zeros(K, np.int64)
    counts[0] = 300
    for k in used:
        counts[k] = rng.integers(1, 40)
    idx, counts = idx_from_counts(rng, counts, N, K - 1)
    idx[N - 1], idx[0] = idx[0], idx[N - 1]                     # (still a permutation of the same codes)
    return wide_rows(rng, N, D), idx, wide_rows(rng, K, D), counts
