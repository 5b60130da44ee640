"""Inputs of tests/test_gpu_tokenize_instances.py, built with numpy and the C oracle only (no GPU code), so that
tests/test_tokenize_cases_host.py can show on a machine without a GPU that every planted input is the case it claims to be and
that a wrong implementation of the property under test answers differently on it.

  * `instance()` restates the host-side rule of csrc/lipvq_fused.hip (tokenize_run / launch_tokenize): which of the fused
    launch's kernel instances a call runs.
  * `params()` / `scaled()` / `dead()` / `centred()`: models (oracle.make_params' trained regime, the numpy twin of
    bench.trained_like_) and their edge variants.
  * `planted()`: codebooks built from the oracle's z_e of the first N_PLANT input rows (families (a) - (d) of
    tests/test_gpu_tokenize_booking.py, restated for any width, and the half-used last tile of D = 208).
  * `nonfinite_inputs()`: the row set of test_gpu_tokenize_booking.py::test_nonfinite_rows_beside_ordinary_ones, beside ordinary
    rows and in a wave of its own.

Everything is computed once per key and must not be modified by its users."""
import numpy as np

from oracle import lipvq_oracle as O

CB_KEY = {"llfq": "quantizer.codebook", "vq": "embedding.weight"}
DIST = {"llfq": O.DIST_NORM, "vq": O.DIST_SQSUM}
RELU3 = (O.ACT_RELU, O.ACT_RELU, O.ACT_RELU)
VQ_ENC = ("encoder.0.weight", "encoder.0.bias", "encoder.2.weight", "encoder.2.bias", "encoder.4.weight", "encoder.4.bias")

N_EDGE = 256 + 37              # one full 8-wave row block, one full wave, one wave of five rows, six empty ones
N_PLANT = 64                   # the first two waves of rows carry the plants
LISTS_ALL_K = 2048             # csrc/lipvq_screen.h: LQ_LISTS_ALL_K
FUSED_WORKGROUPS = 256         # one persistent workgroup per CU (launch_tokenize_as)
SCALE_EXP_CLAMP = 60           # lq_scale_exp: k = 13 - floor(log2 max) clamped to [-60, 60]

_oracle = []
_cache = {}


def orc():
    if not _oracle:
        _oracle.append(O.CanonicalOracle())
    return _oracle[0]


def _once(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


# ---- which instance a call runs (csrc/lipvq_fused.hip: tokenize_run, launch_tokenize) ---------------------------------------------

def screen_S(D):
    s = (D + 15) // 16
    return 2 if s <= 2 else 4 if s <= 4 else 8 if s <= 8 else 13


def instance(variant, D, K, N, screen=None, shape=None, want_ze=False, want_pre=False, fast=False, inplace_opt=True):
    """The template arguments <S, FAST, TRAIN, WAVES, COARSE, VQ, KEEPZ> of the launch and the host-side modes that go with them.
    screen = "fine" | "coarse" | None (the size rule lq_screen_coarse_default); shape = "w8rg1" | "w4rg1" | None (tok_waves' size
    rule); want_ze: the caller passes a z_e buffer (the VQ and training entry points always do)."""
    S = screen_S(D)
    vq = variant == "vq"
    coarse = (K >= 4096 or (S >= 8 and K >= 1024)) if screen is None else screen == "coarse"
    coarse = coarse and not fast
    caller_ze = want_ze or want_pre or vq
    # (z_e goes to the workspace's scratch where the caller gives no buffer: always for a parity launch, up to 131 072 rows in fast mode)
    have_ze = caller_ze or coarse or not fast or N <= 131072
    inplace = have_ze and not coarse and K <= LISTS_ALL_K and inplace_opt
    ring = inplace and not caller_ze
    parity = not vq and not want_pre and not fast
    keepz = ring and parity and S <= 4
    if parity:
        waves = {"w8rg1": 8, "w4rg1": 4, None: 4 if N <= 4 * 32 * 256 else 8}[shape]
        if coarse and S < 8:
            waves = 8                                          # (the narrow one-product instances have the 8-wave shape only)
    else:
        waves = 8
    return dict(S=S, FAST=fast, TRAIN=want_pre, WAVES=waves, COARSE=coarse, VQ=vq, KEEPZ=keepz, inplace=inplace,
                ring=ring and not keepz, PACKF=S <= 4 or S > 8 or coarse, lap=FUSED_WORKGROUPS * waves * 32, unit=waves * 32)


# ---- models ------------------------------------------------------------------------------------------------------------------------

def params(variant, A, D, K):
    return _once(("params", variant, A, D, K),
                 lambda: O.make_params(31000 + 1000 * A + 7 * D + K + (500 if variant == "vq" else 0), A, D, K, variant=variant, oracle=orc()))


def with_codebook(variant, p, cb):
    q = dict(p)
    q[CB_KEY[variant]] = np.ascontiguousarray(cb, np.float32)
    return q


def inputs(seed, N, A, n_max=None):
    """the first N rows of one seeded array: a smaller launch's rows are a prefix of a larger one's"""
    full = _once(("x", seed, A, max(n_max or N_EDGE, N)), lambda: O.make_inputs(seed, max(n_max or N_EDGE, N), A))
    return full[:N]


def encode(variant, p, x, save_pre=False):
    if variant == "llfq":
        return orc().llfq_encode(p, x, save_pre=save_pre)
    return orc().mlp3(x, *[p[k] for k in VQ_ENC], RELU3, save_pre=save_pre)


def answers(key, variant, p, x):
    """the C oracle's answers of one (parameters, inputs) pair: dict(ze, pre, idx, zq, usage), computed once per key"""
    def build():
        ze, pre = encode(variant, p, x, save_pre=True)
        idx, zq, usage = orc().nearest(ze, p[CB_KEY[variant]], DIST[variant])
        return dict(ze=ze, pre=pre, idx=idx, zq=zq, usage=usage)
    return _once(("answers", key), build)


def near_tie_rows(variant, p, ze):
    """rows whose two smallest distances (the oracle's fp32 values) differ by less than 1e-6 of the smaller"""
    d = np.sort(orc().distances(ze, p[CB_KEY[variant]], DIST[variant]), axis=1)
    return (d[:, 1] - d[:, 0]) < 1e-6 * d[:, 0]


def two_best(ze_row, cb):
    """(best, second, d0, d1, d2) by float64 distances, first index first among equals"""
    d = ((cb.astype(np.float64) - ze_row.astype(np.float64)) ** 2).sum(axis=1)
    o = np.argsort(d, kind="stable")
    return int(o[0]), int(o[1]), d[o[0]], d[o[1]], d[o[2]]


# ---- planted codebooks ---------------------------------------------------------------------------------------------------------------

def ulp_up(z, j):
    e = z.copy()
    e[j] = np.nextafter(e[j], np.float32(np.inf))
    return e


def dup_upper_half(cb):
    """(d): code half + c becomes code c moved up by one ulp in coordinate c % D, for c < half = K // 2 (an odd K keeps its last code)"""
    cb = cb.copy()
    K, D = cb.shape
    half = K // 2
    c = np.arange(half)
    cb[half:2 * half] = cb[:half]
    cb[half + c, c % D] = np.nextafter(cb[c, c % D], np.float32(np.inf))
    return cb


def tile_pairs(ntiles):
    """consecutive tiles at the start, in the middle and at the end of the pass, and the first with the last"""
    return [(0, 1), (5, 6), (ntiles - 2, ntiles - 1), (0, ntiles - 1)]


def slots_same_lane(n, K, dup):
    """row n < N_PLANT -> (winner, runner-up): two codes of full tiles, in lane class n % 32 (dup, odd rows: the code of the later
    tile in lane class (n + 16) % 32 instead); rows n and n + 32 get disjoint tiles.  The exact copy of the row sits in the earlier
    tile for rows with (n // 4) % 2 == 0, in the later tile for the others."""
    t0, t1 = tile_pairs(K // 32)[(n if n < 32 else n + 2) % 4]
    k0, k1 = 32 * t0 + n % 32, 32 * t1 + n % 32
    if dup and n % 2 == 1:
        k1 = (k1 & ~31) | ((n + 16) % 32)
    return (k0, k1) if (n // 4) % 2 == 0 else (k1, k0)


def plant_same_lane(cb, ze, dup):
    """(a) / (c): per row an exact copy of its z_e and a copy one ulp away in its largest coordinate (dup: a second exact copy)"""
    cb = cb.copy()
    for n in range(N_PLANT):
        win, run = slots_same_lane(n, cb.shape[0], dup)
        cb[win] = ze[n]
        cb[run] = ze[n] if dup else ulp_up(ze[n], int(np.argmax(ze[n])))
    return cb


CORNER_ROWS = [0, 4, 27, 31]       # rows of a wave held by accumulator registers 0 and 15 in either half of the wave


def row_register(i):
    """row i of a wave's 32 -> (accumulator register, half of the wave) that hold it (lq_row_factors)"""
    return (i & 3) + 4 * (i >> 3), (i >> 2) & 1


def corner_slots(K):
    """(b): row -> code: the corner rows of wave 0 win in tile 0, those of wave 1 in the last full tile"""
    return {32 * w + i: 32 * tile + i for w, tile in ((0, 0), (1, K // 32 - 1)) for i in CORNER_ROWS}


def plant_corners(cb, ze):
    cb = cb.copy()
    for n, k in corner_slots(cb.shape[0]).items():
        cb[k] = ze[n]
    return cb


HALF_TILE_D = 208
HALF_TILE_LAST = slice(192, 208)   # the used half of the last 32-feature tile = the last (13th) k-step of the screen's chain
HALF_TILE_FIRST = slice(0, 16)     # the first k-step


def half_tile_slots(n):
    """row n < N_PLANT -> (code that differs from the row in features 192 .. 207 only, code that differs in 0 .. 15 only, the row's
    exact copy): the copy has the HIGHEST index, so a kernel that loses a k-step sees an exact tie and the first-index rule takes
    the wrong code"""
    return n, 64 + n, 128 + n


def plant_half_tile(cb, ze):
    """D = 208.  Even rows: steps of 1/4 (the screen separates the codes and certifies the row), odd rows: steps of 2^-7 (the row
    goes to an exact decision)."""
    assert cb.shape[1] == HALF_TILE_D and cb.shape[0] >= 192
    cb = cb.copy()
    for n in range(N_PLANT):
        last, first, win = half_tile_slots(n)
        step = np.float32(0.25 if n % 2 == 0 else 2.0 ** -7)
        cb[win] = ze[n]
        cb[last] = ze[n]
        cb[last, HALF_TILE_LAST] += step
        cb[first] = ze[n]
        cb[first, HALF_TILE_FIRST] += step
    return cb


PLANTS = {
    "plain": lambda cb, ze: cb,
    "same-lane": lambda cb, ze: plant_same_lane(cb, ze, dup=False),
    "dup": lambda cb, ze: plant_same_lane(cb, ze, dup=True),
    "corners": plant_corners,
    "upper-half": lambda cb, ze: dup_upper_half(cb),
    "half-tile": plant_half_tile,
}
X_SEED = 700
RAGGED_ROW = N_PLANT           # "dup" with K no multiple of 32: this row's exact copy is code K - 1


def planted(plant, A, D, K, variant="llfq"):
    """(parameters with the planted codebook, the N_EDGE input rows whose first N_PLANT carry the plants)"""
    def build():
        p = params(variant, A, D, K)
        x = inputs(X_SEED + D + A, N_EDGE, A)
        ze = encode(variant, p, x[:N_PLANT + 1])
        cb = PLANTS[plant](p[CB_KEY[variant]], ze)
        if K % 32 and plant == "dup":
            cb[K - 1] = ze[RAGGED_ROW]                     # the last code of a ragged last tile wins a row of its own
        return with_codebook(variant, p, cb), x
    return _once(("planted", plant, A, D, K, variant), build)


RING_K = 256


def ring_case(D, shape, fast=False, A=7):
    """(parameters, inputs, instance) of a launch whose workgroups 0 and 1 run a second row block: 256 workgroups x one block, one
    more full block and a ragged one of 37 rows; every code has a twin one ulp away, so no row of either lap can be certified"""
    probe = instance("llfq", D, RING_K, 1 << 17, shape=shape, fast=fast)
    N = probe["lap"] + probe["unit"] + 37
    p, _ = planted("upper-half", A, D, RING_K)
    x = inputs(X_SEED + 300 + D, N, A, n_max=65536 + 256 + 37)
    return p, x, instance("llfq", D, RING_K, N, shape=shape, fast=fast)


# ---- the plain VQVAE's edges -------------------------------------------------------------------------------------------------------

SCALE_EXPONENTS = (-20, -14, 0, 14, 20, 40)


def scaled(p, e):
    """the last encoder layer and the codebook times 2^e: z_e and the codes scale exactly, the distances by 2^(2e)"""
    q = dict(p)
    f = np.float32(2.0) ** np.float32(e)
    for k in ("encoder.4.weight", "encoder.4.bias", "embedding.weight"):
        q[k] = (p[k] * f).astype(np.float32)
        assert np.array_equal(q[k].astype(np.float64), p[k].astype(np.float64) * 2.0 ** e)
    return q


def dead(variant, p):
    """every encoder bias replaced by -|b|: a row of zeros dies in the first ReLU and z_e is exactly 0.  If the code nearest to the
    origin is code 0, codes 0 and 1 change places, so that an implementation that answers 0 for a row it cannot scale is told
    from the right one."""
    assert variant == "vq"
    q = dict(p)
    for k in ("encoder.0.bias", "encoder.2.bias", "encoder.4.bias"):
        q[k] = -np.abs(p[k])
    cb = p[CB_KEY[variant]].copy()
    if int(np.argmin((cb.astype(np.float64) ** 2).sum(axis=1))) == 0:
        cb[[0, 1]] = cb[[1, 0]]
    q[CB_KEY[variant]] = cb
    return q


def dead_inputs(A, all_zero=False):
    """N_EDGE rows; rows 1, 5, 30, 31 and 40 .. 47 of the first two waves are zeros among ordinary rows (all_zero: every row)"""
    x = inputs(X_SEED + 90 + A, N_EDGE, A).copy()
    rows = np.array([1, 5, 30, 31] + list(range(40, 48)))
    if all_zero:
        x[:] = 0.0
        rows = np.arange(N_EDGE)
    else:
        x[rows] = 0.0
    return x, rows


CENTRE = np.float32(0.5)
CENTRE_K = 64


def centred(variant, A, D):
    """every z_e row equal to the codebook's mean: 64 codes equal to c = 0.5 (a power-of-two count: the mean is exactly c) and an
    encoder that answers c for every row -- the VQVAE through W2 = 0, b2 = c, LLFQVAE_V4 through a zero hidden layer and a zero
    latent bias (sigmoid(0) = 0.5)"""
    def build():
        q = dict(params(variant, A, D, CENTRE_K))
        if variant == "vq":
            q["encoder.4.weight"] = np.zeros_like(q["encoder.4.weight"])
            q["encoder.4.bias"] = np.full_like(q["encoder.4.bias"], CENTRE)
        else:
            q["encoder.2.weight"] = np.zeros_like(q["encoder.2.weight"])
            q["encoder.2.bias"] = np.zeros_like(q["encoder.2.bias"])
            q["to_latent.b"] = np.zeros_like(q["to_latent.b"])
        q[CB_KEY[variant]] = np.full((CENTRE_K, D), CENTRE, np.float32)
        return q
    return _once(("centred", variant, A, D), build)


# ---- rows that are not finite ----------------------------------------------------------------------------------------------------------

def nonfinite_inputs(A):
    """(x, rows that hold a NaN, rows that hold an infinity, rows of +-1e30 / +-1e37): beside ordinary rows in waves 0, 1 and 2 and
    the last, ragged wave, and as a wave of their own (rows 96 .. 127)"""
    x = inputs(X_SEED + 800 + A, N_EDGE, A).copy()
    nan_rows, inf_rows, big_rows = [3, 40, 260], [9, 14, 70], [20, 25, 45, 50]
    x[3] = np.nan
    x[9] = np.inf
    x[14] = -np.inf
    x[20] = 1e30
    x[25] = -1e30
    x[45] = 1e37
    x[50] = -1e37
    x[40, min(2, A - 1)] = np.nan
    x[70, 0] = np.inf
    x[260] = np.nan
    kinds = [np.nan, np.inf, -np.inf, 1e30, -1e30, 1e37, -1e37]
    for i, r in enumerate(range(96, 128)):
        v = kinds[i % len(kinds)]
        x[r] = v
        (nan_rows if v != v else inf_rows if abs(v) == np.inf else big_rows).append(r)
    return x, np.array(sorted(nan_rows)), np.array(sorted(inf_rows)), np.array(sorted(big_rows))
