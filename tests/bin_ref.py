"""References and seeded input builders for tests/test_gpu_bin_edges.py and tests/test_gpu_update_edges.py, held to their own
conditions on the CPU by tests/test_bin_ref_host.py.

Everything here is stock torch or numpy on the CPU, in float64 where a value is a yardstick and in fp32 where the reference class
itself (robomimic/models/bin_action/backbone.py, restated with the ops it calls) is the expected value bit for bit.  Nothing here
reads a file; every builder is seeded and returns the same arrays on every machine."""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
F32 = np.float32
INF, NAN = float("inf"), float("nan")


def rng_of(*key):
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(k) for k in key])))


# ---- A.1-A.3  bin_hidden --------------------------------------------------------------------------------------------------------

HIDDEN_WIDE = ((64, 5, 96), (65, 5, 96), (100, 5, 130), (128, 4, 64), (256, 2, 64), (128, 4, 96))        # (A, num_bins, H); the last: whole chunks, ragged slice
HIDDEN_WIDE_N = (5, 1000)
HIDDEN_LDS_EDGES = ((16, 20), (3, 107), (12, 50))                                         # A * num_bins = 320, 321, 600
HIDDEN_REFUSED = ((1, 601), (12, 64))
HIDDEN_RAGGED_A_NB = (7, 20)                                                               # A * num_bins = 140: slice width 128
HIDDEN_RAGGED_H = (1, 63, 64, 65, 128, 129, 224)
HIDDEN_RAGGED_N = (1, 3, 4, 5, 63, 64, 65)
HIDDEN_GRID_STRIDE = (32768 + 67, 32)                                                      # (N, H)


def hidden_case(A, nb, H, N, seed=0):
    """(bins [A, N] int64, P [A, nb, H] fp32, b1 [H] fp32): every bin of every dimension is used when N >= nb; P is O(1) with a
    few entries 1e3 times larger so that a row taken from the wrong dimension moves the sum far beyond rounding."""
    rng = rng_of(A, nb, H, N, seed, 1)
    bins = rng.integers(0, nb, (A, N)).astype(np.int64)
    bins[:, :min(N, nb)] = (np.arange(min(N, nb))[None, :] + np.arange(A)[:, None]) % nb
    P = rng.standard_normal((A, nb, H)).astype(F32)
    P[rng.integers(0, A, 8), rng.integers(0, nb, 8), rng.integers(0, H, 8)] *= F32(1e3)
    b1 = rng.standard_normal(H).astype(F32)
    return bins, P, b1


def hidden_f64(bins, P, b1):
    """(pre1 in float64, allowed |error| of the fp32 recursive sum b1 + P_0 + ... + P_{A-1}: (A + 1) u (|b1| + sum_i |P_i[bin_i]|))."""
    A = bins.shape[0]
    P64, rows = P.astype(np.float64), np.arange(A)[:, None]
    g = P64[rows, bins]                                                   # [A, N, H]
    pre = b1.astype(np.float64)[None] + g.sum(0)
    mag = np.abs(b1.astype(np.float64))[None] + np.abs(g).sum(0)
    return pre, (A + 1) * U32 * mag


# ---- A.4-A.5  bin_minmax ---------------------------------------------------------------------------------------------------------

MINMAX_A = (1, 7, 63, 64, 65, 255, 256)
MINMAX_N = (1, 2, 9, 4099)
MINMAX_START = ("inf", "finite")


def minmax_start(A, start):
    if start == "inf":
        return np.full(A, INF, F32), np.full(A, -INF, F32)
    lo, hi = np.full(A, -0.5, F32), np.full(A, 0.5, F32)
    lo[::3], hi[::3] = F32(-1e6), F32(1e6)                                # every third column: the batch leaves both unchanged
    return lo, hi


def minmax_case(A, N, seed=0):
    """x [N, A] fp32 with planted extremes: the largest value at flat index 0, the smallest at flat index N A - 1, and a second
    pair on either side of every 2048-element boundary the array has (flat 2047 | 2048, 4095 | 4096, ...)."""
    rng = rng_of(A, N, seed, 2)
    x = rng.standard_normal((N, A)).astype(F32)
    flat = x.reshape(-1)
    for b in range(2048, flat.size, 2048):
        flat[b - 1], flat[b] = F32(-50.0 - b % 97), F32(60.0 + b % 89)
    flat[0] = F32(1e5)
    flat[-1] = F32(-2e5)
    return x


def minmax_torch(x, rmin, rmax):
    """bin:37-40 with the stock ops on the CPU (NaN propagates through both)."""
    xt = torch.from_numpy(np.ascontiguousarray(x))
    lo = torch.minimum(torch.from_numpy(rmin.copy()), xt.min(dim=0)[0])
    hi = torch.maximum(torch.from_numpy(rmax.copy()), xt.max(dim=0)[0])
    return lo.numpy(), hi.numpy()


def same_floats(a, b, sign_of_zero=True):
    """Equal as floats with NaN in the same places (array_equal treats -0 and +0 as equal; with sign_of_zero the bits of the
    zeros are compared as well)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = np.array_equal(np.nan_to_num(a, nan=0.0, posinf=INF, neginf=-INF), np.nan_to_num(b, nan=0.0, posinf=INF, neginf=-INF))
    if ok and sign_of_zero:
        ok = np.array_equal(np.signbit(a) & (a == 0), np.signbit(b) & (b == 0))
    return bool(ok)


NAN_A = (1, 7, 65, 256)
NAN_N = (1, 9, 4099)


def nan_case(A, N, seed=0):
    """(x [N, A] with NaN planted in every third column, nan_cols, later [N, A] finite): a NaN in the first row, the last, or alone
    in the middle (by column), and wherever such a column meets either side of a 2048-element boundary of the flat array; the
    other columns stay clean."""
    rng = rng_of(A, N, seed, 3)
    x = rng.standard_normal((N, A)).astype(F32)
    nan_cols = list(range(0, A, 3))
    for j, c in enumerate(nan_cols):
        x[(0, N - 1, N // 2)[j % 3], c] = NAN
    flat = x.reshape(-1)
    for b in range(2048, flat.size, 2048):
        for f in (b - 1, b):
            if (f % A) % 3 == 0:
                flat[f] = NAN
    later = (3.0 * rng.standard_normal((N, A))).astype(F32)
    return x, nan_cols, later


# ---- A.6  boundaries / discretize on edge statistics ----------------------------------------------------------------------------

ONE_UP = float(np.nextafter(F32(1), F32(2)))
EDGE_STATS = ((-1.0, INF), (-INF, 2.0), (-INF, INF), (NAN, NAN), (0.0, 0.0), (-1e-45, 3e-39), (-3e38, 3e38), (2.0, 2.0),
              (1.0, ONE_UP), (-0.75, 1.25))
EDGE_SPECIALS = (NAN, INF, -INF, 0.0, -0.0, 1e-45, 3e38, -3e38)
EDGE_NB = (1, 2, 5, 20, 255)


def edge_stats():
    return np.array([s[0] for s in EDGE_STATS], F32), np.array([s[1] for s in EDGE_STATS], F32)


def torch_boundaries(rmin, rmax, nb):
    """[A, nb + 1]: torch.linspace per column on the CPU (bin:42-53)."""
    lo, hi = torch.from_numpy(np.ascontiguousarray(rmin)), torch.from_numpy(np.ascontiguousarray(rmax))
    return torch.stack([torch.linspace(lo[i], hi[i], nb + 1) for i in range(lo.numel())]).numpy()


def torch_bins(x, bd, nb):
    """[A, N] int64: bucketize + clamp per column on the CPU (bin:55-66) on given boundaries."""
    xt = torch.from_numpy(np.ascontiguousarray(x))
    return torch.stack([torch.clamp(torch.bucketize(xt[:, i].contiguous(), torch.from_numpy(bd[i].copy())) - 1, 0, nb - 1)
                        for i in range(x.shape[1])]).numpy()


def edge_values(nb):
    """x [3 (nb + 1) + len(EDGE_SPECIALS), A]: column i holds every boundary of column i, its two fp32 neighbours, and the specials."""
    bd = torch_boundaries(*edge_stats(), nb)
    up, down = np.nextafter(bd, F32(INF)), np.nextafter(bd, F32(-INF))
    sp = np.tile(np.array(EDGE_SPECIALS, F32)[None], (bd.shape[0], 1))
    return np.ascontiguousarray(np.concatenate([bd, up, down, sp], 1).T.astype(F32)), bd


# ---- B  gradients of the module ---------------------------------------------------------------------------------------------------

GRAD_SMALL = ((1, 1, 8, 1), (5, 3, 32, 5), (80, 12, 208, 20), (333, 7, 64, 20), (4097, 2, 16, 2), (200, 65, 16, 5))    # (N, A, D, nb)
GRAD_CONSTANT = (64, 3, 16, 5)                        # column 1 constant: every row in one bin of that dimension
GRAD_LARGE = ((32781, 3, 32, 20), (66000, 3, 32, 20), (66000, 2, 16, 2), (66000, 2, 16, 1))
GRAD_DETERMINISTIC = GRAD_LARGE[:2]
E2E = 2e-5
LARGE_FACTOR = 4.0


def grad_actions(N, A, nb, seed=0, constant_col=None):
    """x [N, A] fp32 in [-1, 1] with both ends present in every column; from 1000 rows on 95 % of a column's rows sit in the
    middle of one bin (the hot bin: tens of thousands of rows summed into one table row) and the rest cover every bin."""
    rng = rng_of(N, A, nb, seed, 4)
    x = rng.uniform(-1.0, 1.0, (N, A)).astype(F32)
    if N >= 1000:
        for c in range(A):
            hot_bin = (7 + 3 * c) % nb
            centre = -1.0 + (hot_bin + 0.5) * 2.0 / nb
            hot = rng.random(N) < 0.95
            x[hot, c] = (centre + rng.uniform(-0.3, 0.3, int(hot.sum())) / nb).astype(F32)
            edges = -1.0 + (np.arange(nb) + 0.5) * 2.0 / nb
            x[1:1 + nb, c] = edges.astype(F32)                             # one row in the middle of every bin
    if N >= 2:
        x[0], x[-1] = F32(-1.0), F32(1.0)
    if constant_col is not None:
        x[:, constant_col] = F32(0.375)
    return x


def module_state(A, D, nb, seed=0):
    """Seeded parameters keyed like AdaptiveBinActionEmbedding.state_dict() minus the two buffers (CPU fp32 tensors)."""
    from oracle import lipvq_oracle as O
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in O.make_bin_params(seed + 7 * A + D + nb, A, D, nb).items()}


def grad_upstream(N, D, seed=0):
    return rng_of(N, D, seed, 5).standard_normal((N, D)).astype(F32)


def stock_module_grads(sd, bins, R, dtype, scale=1.0):
    """Parameter gradients of scale * (out * R).sum() for the stock formulation (embedding gather, cat, Linear, GELU, Linear, GELU;
    bin:26-31, 77-86) in `dtype` on the CPU.  sd: the module's state_dict (CPU tensors), bins [N, A] int64.  Returns (out, grads)."""
    A = bins.shape[1]
    p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in sd.items() if not k.startswith("running_")}
    emb = torch.cat([F.embedding(bins[:, i], p[f"embedding_layers.{i}.weight"]) for i in range(A)], dim=-1)
    h = F.gelu(F.linear(emb, p["output_layer.0.weight"], p["output_layer.0.bias"]))
    out = F.gelu(F.linear(h, p["output_layer.2.weight"], p["output_layer.2.bias"]))
    (scale * (out * R.to(dtype)).sum()).backward()
    return out.detach(), {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in p.items()}


SCATTER_K = (1, 2, 5, 20)
SCATTER_D = (16, 96, 384)
SCATTER_N = (1000, 40000, 70001)


def scatter_case(N, K, D, seed=0):
    """(g [N, D] fp32, idx [N] int64): a third of the rows on code K - 1, every code used."""
    rng = rng_of(N, K, D, seed, 6)
    g = rng.standard_normal((N, D)).astype(F32)
    idx = rng.integers(0, K, N).astype(np.int64)
    idx[:N // 3] = K - 1
    idx[N // 3:N // 3 + K] = np.arange(K)
    return g, idx


def scatter_sequential_fp32(g, idx, K):
    """fp32 adds in ascending row order per code (what the sequential routes promise bit for bit)."""
    out = np.zeros((K, g.shape[1]), F32)
    for k in range(K):
        rows = g[idx == k]
        acc = np.zeros(g.shape[1], F32)
        for r in rows:
            acc = acc + r
        out[k] = acc
    return out


# ---- C  EMA ------------------------------------------------------------------------------------------------------------------

EMA_SHAPES = ((1, 7), (37, 5), (1024, 3), (1025, 33), (8192, 257))                         # (K, D)
EMA_STATES = ("typical", "fresh_zero", "first_step_third_dead", "decay0", "decay1", "one_live_code", "huge_counts", "tiny_clusters",
              "eps1")
EMA_NONFINITE = ("fresh_zero",)                       # n = 0: smoothed = eps / (K eps) * 0 = 0, codebook = 0 / 0


def ema_state(K, D, state, seed=0):
    """dict(cs [K], es [K, D], counts [K] int64, dw [K, D], decay, eps) in fp32 for one named state."""
    rng = rng_of(K, D, EMA_STATES.index(state), seed, 7)
    decay, eps = 0.97, 1e-5
    cs = rng.uniform(0.5, 40.0, K).astype(F32)
    es = (cs[:, None] * rng.uniform(0.0, 1.0, (K, D))).astype(F32)
    counts = rng.integers(0, 60, K).astype(np.int64)
    if state == "fresh_zero":
        cs[:], es[:], counts[:] = 0, 0, 0
    elif state == "first_step_third_dead":
        cs[:] = 0
        es = rng.uniform(0.0, 1.0, (K, D)).astype(F32)
        counts[::3] = 0
        counts[1 % K] = max(1, counts[1 % K])
    elif state == "decay0":
        decay = 0.0
        counts = np.maximum(counts, 1)
    elif state == "decay1":
        decay = 1.0
    elif state == "one_live_code":
        cs[:], counts[:] = 0, 0
        counts[K // 2] = 1000
    elif state == "huge_counts":
        counts = rng.integers(2 ** 24, 2 ** 26 + 1, K).astype(np.int64)
        counts[0], counts[-1] = 2 ** 24 + 1, 2 ** 26
    elif state == "tiny_clusters":
        cs = rng.uniform(1e-9, 9e-7, K).astype(F32)
        es = (cs[:, None] * rng.uniform(0.0, 1.0, (K, D))).astype(F32)
        counts[:] = 0
        decay = 0.5
    elif state == "eps1":
        eps = 1.0
    dw = (counts[:, None] * rng.uniform(0.0, 1.0, (K, D))).astype(F32)       # a sum of `counts` rows of a sigmoid's outputs
    return dict(cs=cs, es=es, counts=counts, dw=dw, decay=decay, eps=eps)


def ema_f64(s):
    """The rule in float64 from the fp32 state (decay and eps as the fp32 values the kernel receives)."""
    decay, eps = float(F32(s["decay"])), float(F32(s["eps"]))
    cs = decay * s["cs"].astype(np.float64) + (1.0 - decay) * s["counts"].astype(np.float64)
    es = decay * s["es"].astype(np.float64) + (1.0 - decay) * s["dw"].astype(np.float64)
    n = cs.sum()
    with np.errstate(all="ignore"):
        sm = (cs + eps) / (n + cs.size * eps) * n
        cb = es / sm[:, None]
    return cs, es, cb


def within_or_same_kind(got, want, rel=1e-5):
    """|got - want| <= rel (1 + |want|) where want is finite; elsewhere the same kind (NaN | +inf | -inf) in the same place."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    ok = np.abs(got[fin] - want[fin]) <= rel * (1.0 + np.abs(want[fin]))
    kind = np.array_equal(np.isnan(got[~fin]), np.isnan(want[~fin])) and np.array_equal(got[~fin][~np.isnan(got[~fin])],
                                                                                        want[~fin][~np.isnan(want[~fin])])
    return bool(np.isfinite(got[fin]).all() and ok.all() and kind)


# ---- C  AdamW ----------------------------------------------------------------------------------------------------------------

ADAMW_SIZES = (1, 255, 256, 257, 65537, 300001)
ADAMW_REGIMES = ("randn_decades", "zero", "tiny", "huge", "spike", "alternating")
ADAMW_STEPS = 6


def adamw_sizes(count, seed=0):
    """`count` sizes from ADAMW_SIZES: every size at least once, the two large ones at most twice each (memory and time)."""
    rng = rng_of(count, seed, 8)
    sizes = list(ADAMW_SIZES) + [65537, 300001] + [int(s) for s in rng.choice(ADAMW_SIZES[:4], count - 8)]
    rng.shuffle(sizes)
    return sizes


def adamw_params(sizes, scale, seed=0):
    rng = rng_of(len(sizes), seed, 9)
    return [(scale * rng.standard_normal(n)).astype(F32) for n in sizes]


def adamw_grad(regime, n, step, index, seed=0):
    """fp32 gradient [n] of parameter `index` at `step` (0-based) in one regime; None = no gradient on this step."""
    if index % 11 == 3 and step in (1, 4):
        return None
    rng = rng_of(ADAMW_REGIMES.index(regime), n, step, index, seed, 10)
    if regime == "randn_decades":
        return (rng.standard_normal(n) * 10.0 ** (step - 2)).astype(F32)
    if regime == "zero":
        return np.zeros(n, F32)
    if regime == "tiny":
        return np.full(n, 1e-30, F32) * np.where(rng.random(n) < 0.5, F32(-1), F32(1))
    if regime == "huge":                                  # 1e15^2 = 1e30 < 3.4e38: the square stays in fp32
        return np.full(n, 1e15, F32) * np.where(rng.random(n) < 0.5, F32(-1), F32(1))
    if regime == "spike":
        return (np.zeros(n, F32) if step != 3 else (100.0 * rng.standard_normal(n)).astype(F32))
    if regime == "alternating":
        return np.full(n, 1.0 if step % 2 == 0 else -1.0, F32)
    raise ValueError(regime)


# ---- C  loss reductions ----------------------------------------------------------------------------------------------------------

MSE_N = (1, 3, 4, 5, 1023, 2 ** 21 + 7, 3 * 2 ** 21 + 23)
STE_N = (1, 2048 * 256 + 1)


def mse_pair_case(nx, nz, seed=0, big=False):
    """(xr, x, zq, ze) fp32 1-D; with `big` a few differences of up to 1e19 (their squares, 1e38, still fit fp32 and double)."""
    rng = rng_of(nx, nz, seed, 11)
    xr, x = rng.standard_normal(nx).astype(F32), rng.standard_normal(nx).astype(F32)
    zq, ze = rng.uniform(0, 1, nz).astype(F32), rng.uniform(0, 1, nz).astype(F32)
    if big:
        xr[::max(1, nx // 7)] = F32(1e19)
        ze[nz // 2] = F32(-1e19)
    return xr, x, zq, ze


def mse_f64(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sum(d * d, dtype=np.float64) / d.size)
