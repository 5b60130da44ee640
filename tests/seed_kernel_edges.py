"""Input builders of the seed kernels' edge tests (tests/test_gpu_mlp3_edges.py, test_gpu_misc_edges.py,
test_gpu_nearest_edges.py).  Pure numpy, no torch.cuda: tests/test_seed_kernel_edges_host.py holds every builder to what it
claims on the CPU, against the canonical oracle, so that a failure on the GPU cannot come from an input that is not what its
name says.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

ACT_NONE, ACT_GELU, ACT_SIGMOID, ACT_RELU = 0, 1, 2, 3
MATH_H = Path(__file__).resolve().parent.parent / "lipvq-vae_amd" / "csrc" / "lipvq_math.h"
MSE_THREADS = 2048 * 256          # mse_partial_kernel's grid (csrc/lipvq_misc.hip): MSE_BLOCKS workgroups of 256 threads

F32 = np.float32
DENORM_MIN = np.float32(np.ldexp(1.0, -149))                      # smallest positive denormal
DENORM_MAX = np.nextafter(np.float32(np.ldexp(1.0, -126)), F32(0))   # largest denormal

# the planted row classes of special_rows, in planting order
SPECIAL_CLASSES = ("nan_row", "nan_elem", "pos_inf", "neg_inf", "pos_3e38", "neg_3e38", "denormal", "neg_zero")


def special_rows(N, K0, positions, rot=0, seed=0):
    """(x, planted, rows): x [N, K0] seeded standard-normal rows, `planted` a copy with one special row per entry of `rows`
    (dict row -> class).  Rows are `positions` (callers pass the 32-row tile seams 0, 31, 32, 63, 64 and N - 1) and, while a
    class is still missing, the rows next to the first and the last position; class c of SPECIAL_CLASSES goes to the
    (c + rot)-th of them, so every class is planted at least once and `rot` moves the classes over the seams."""
    rng = np.random.default_rng(1000003 * N + 101 * K0 + seed)
    x = (rng.standard_normal((N, K0)) * 1.5).astype(F32)
    where = []
    for p in list(positions) + [positions[0] + 1, positions[-1] - 1, positions[0] + 2, positions[-1] - 2]:
        if 0 <= p < N and p not in where:
            where.append(int(p))
        if len(where) >= len(SPECIAL_CLASSES) and len(where) >= len(positions):
            break
    planted = x.copy()
    rows = {}
    for i, r in enumerate(where):
        cls = SPECIAL_CLASSES[(i + rot) % len(SPECIAL_CLASSES)]
        rows[r] = cls
        if cls == "nan_row":
            planted[r] = np.nan
        elif cls == "nan_elem":
            planted[r, K0 // 2] = np.nan
        elif cls == "pos_inf":
            planted[r] = np.inf
        elif cls == "neg_inf":
            planted[r] = -np.inf
        elif cls == "pos_3e38":
            planted[r] = F32(3e38)
        elif cls == "neg_3e38":
            planted[r] = F32(-3e38)
        elif cls == "denormal":
            planted[r] = F32(1e-40)
        elif cls == "neg_zero":
            planted[r] = F32(-0.0)
    return x, planted, rows


# ---------------------------------------------------------------------------------------------------------------------------
# activation sweep: the branch constants are READ from lipvq_math.h
# ---------------------------------------------------------------------------------------------------------------------------
# functions whose comparisons decide a branch of an activation the stacks apply (lq_gelu calls lq_erff through lq_gelu_tail,
# lq_erff and lq_softplus call lq_expf)
BRANCHING_FUNCTIONS = ("lq_gelu", "lq_erff", "lq_sigmoid", "lq_expf", "lq_softplus", "lq_logf_ge1")
_CMP = re.compile(r"[<>]=?\s*(-?\d+\.\d*(?:[eE][-+]?\d+)?)f")


def _function_body(text, name):
    m = re.search(r"LQ_HD\s+float\s+" + re.escape(name) + r"\s*\(", text)
    if m is None:
        raise LookupError(f"{name} not found in {MATH_H.name}")
    i = text.index("{", m.end())
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
        if depth == 0:
            return text[i:j]


def branch_constants(text=None):
    """dict function -> sorted list of the float literals its comparisons (and ?: clamps) test against, from the header text."""
    text = MATH_H.read_text() if text is None else text
    return {fn: sorted({float(c) for c in _CMP.findall(_function_body(text, fn))}) for fn in BRANCHING_FUNCTIONS}


def _neighbours(c, k=3):
    out = [F32(c)]
    lo = hi = F32(c)
    for _ in range(k):
        lo = np.nextafter(lo, F32(-np.inf))
        hi = np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return out


def act_sweep(dense=4001):
    """fp32 arguments for the device-against-host activation comparison: a dense linspace(-30, 30); every constant c that a
    comparison in lipvq_math.h's activation functions tests, as +-c and -- because lq_gelu compares x * x and lq_erff is
    reached with x / sqrt 2 -- +-sqrt(c) and +-c sqrt 2, each with its three fp32 neighbours on either side; +-0, the smallest
    and the largest denormal, +-inf."""
    pts = list(np.linspace(-30.0, 30.0, dense).astype(F32))
    for consts in branch_constants().values():
        for c in consts:
            a = abs(c)
            for v in (a, np.sqrt(a), a * np.sqrt(2.0)):
                for s in (1.0, -1.0):
                    pts += _neighbours(F32(s * v))
    pts += [F32(0.0), F32(-0.0), DENORM_MIN, -DENORM_MIN, DENORM_MAX, -DENORM_MAX, F32(np.inf), F32(-np.inf)]
    return np.array(pts, F32)


def act_reference(oracle, x, act):
    """act(x) as the canonical oracle evaluates it (math_probe for gelu / sigmoid; ReLU is `v <= 0 ? 0 : v`)."""
    x = np.ascontiguousarray(x, F32)
    if act == ACT_GELU:
        return oracle.math_probe(x, 2)
    if act == ACT_SIGMOID:
        return oracle.math_probe(x, 3)
    if act == ACT_RELU:
        return np.where(x <= 0, F32(0.0), x).astype(F32)
    return x.copy()


def identity_stack(pos, act, J, K0=1):
    """(W0, b0, W1, b1, W2, b2, acts): a stack that routes input column 0 unchanged into output column 0 and applies `act` at
    layer `pos` only: W0[0, 0] = 1 and nothing else, W1 / W2 leading identities, zero biases.  J = (J0, J1, J2)."""
    J0, J1, J2 = J
    W0 = np.zeros((J0, K0), F32)
    W0[0, 0] = 1.0
    W1 = np.zeros((J1, J0), F32)
    W1[np.arange(min(J0, J1)), np.arange(min(J0, J1))] = 1.0
    W2 = np.zeros((J2, J1), F32)
    W2[np.arange(min(J1, J2)), np.arange(min(J1, J2))] = 1.0
    acts = [ACT_NONE] * 3
    acts[pos] = act
    return W0, np.zeros(J0, F32), W1, np.zeros(J1, F32), W2, np.zeros(J2, F32), tuple(acts)


def sweep_input(sweep, N, K0):
    """[N, K0] rows with the sweep in column 0 (repeated cyclically up to N rows) and zeros elsewhere."""
    x = np.zeros((N, K0), F32)
    x[:, 0] = np.resize(sweep, N)
    return x


# ---------------------------------------------------------------------------------------------------------------------------
# nearest search
# ---------------------------------------------------------------------------------------------------------------------------
def root_tie_pair(D, oracle, start=1.0625, max_steps=256):
    """(z [D], hi [D], lo [D]): two codes whose squared distances to z differ in fp32 (hi's is the larger) while their
    lq_sqrt values are equal.  With hi at the LOWER index, DIST_NORM must pick hi (first minimum of equal roots) and DIST_SQSUM
    lo.  Found by walking nextafter from `start` (squared distances 1 + a^2 in [2, 4): about a third of adjacent ones share a
    root) and decided by the oracle's own distances -- no fixed numbers."""
    z = np.zeros((1, D), F32)
    a = F32(start)
    for _ in range(max_steps):
        b = np.nextafter(a, F32(np.inf))
        cb = np.zeros((2, D), F32)
        cb[:, 0] = 1.0                                        # 1 + a^2: not a perfect square (sqrt(fl(a^2)) is always a)
        cb[0, D - 1], cb[1, D - 1] = b, a                     # index 0: the larger square
        s = oracle.distances(z, cb, 1)[0]
        v = oracle.distances(z, cb, 0)[0]
        if s[0] > s[1] and v[0] == v[1]:
            return z[0], cb[0], cb[1]
        a = b
    raise LookupError(f"no root tie within {max_steps} steps of {start}")


def mse_probe_positions(n, aligned, nth=MSE_THREADS):
    """Element indices where a one-hot difference probes mse_partial_kernel's loop seams.  Aligned operands: the ends, the last
    vector element and the first tail element, the first element of the second in-flight float4 and of the second pass.
    Misaligned operands run the scalar loop alone, whose seams are the passes of nth elements.  Clipped to [0, n)."""
    pos = [0, n - 1, 4 * (n // 4) - 1, 4 * (n // 4), 4 * nth - 1, 4 * nth, 8 * nth - 1, 8 * nth]
    if not aligned:
        pos += [nth - 1, nth, 2 * nth - 1, 2 * nth]
    return sorted({int(p) for p in pos if 0 <= p < n})


def ulp32(x):
    """Spacing of fp32 at |x| (x a finite fp32 value)."""
    x = np.abs(F32(x))
    return float(np.nextafter(x, F32(np.inf)) - x)


def mse_ref(a, b):
    """mean((a - b)^2) in exact float64 summation (math.fsum) of the float64 squares of the fp32 differences' widened operands."""
    import math
    d = a.astype(np.float64).ravel() - b.astype(np.float64).ravel()
    return math.fsum(d * d) / d.size
