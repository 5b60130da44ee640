"""GPU: phase A of the fused tokenize launch (encoder GELUs, the Lipschitz layer's sigmoid, the fp16 split) against the C oracle, bit
for bit.  The lumped instances evaluate a tile's eight packed pairs four at a time in lockstep (lq_gelu_poly2xN,
lq_sigmoid2_finite_xN, tok_gelu_fixup_lumped); what that can break is WHICH value goes through WHICH chain and which branch a tile
takes, so besides the shape sweep the inputs here are planted, and every planted case is first asserted on the CPU, from the
oracle's pre-activations, to be the case it claims.

Register r of a lane's tile t holds feature 32 t + 2 r + h (h = lane half), so a packed pair (r, r + 1) is features f and f + 2; the
first pair of a tile is r = 0, the last r = 14.  Everything is compared with ==; only NaN is compared as "NaN" (the CPU's and the
GPU's default NaN differ in the sign bit)."""
import numpy as np
import pytest
import torch

from oracle import lipvq_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = ["w8rg1", "w4rg1"]
_params, _models, _refs = {}, {}, {}


def _p(oracle, A, D, K):
    if (A, D, K) not in _params:
        _params[(A, D, K)] = O.make_params(100 + A + D + K, A, D, K, regime="trained", oracle=oracle)
    return _params[(A, D, K)]


def _model(key, p, A, D, K):
    """The module on the GPU with the parameters p (built once per key, never modified)."""
    if key not in _models:
        from lipvq_vae_amd.tokenizer import LLFQVAE_V4
        m = LLFQVAE_V4(A, D, num_codes=K).cuda()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
        assert m.fused_shape()
        _models[key] = m
    return _models[key]


def _reference(oracle, key, p, x):
    """(z_e, pre-activations, idx, z_q) of the oracle, computed once per key."""
    if key not in _refs:
        ze, pre = oracle.llfq_encode(p, x, save_pre=True)
        idx, zq, _ = oracle.nearest(ze, p["quantizer.codebook"])
        _refs[key] = (ze, pre, idx, zq)
    return _refs[key]


def _same_bits(got, ref):
    """== on the bits, except that a NaN of the reference only has to be a NaN"""
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]))


def _check(model, x, ze_ref, idx_ref, zq_ref):
    """Both launches -- z_e kept in registers (want_ze=False) and stored -- against the oracle.  Rows whose z_e holds a NaN have no
    defined nearest code: there the two launches only have to agree with each other."""
    xt = torch.from_numpy(x).cuda()
    idx_k, zq_k, _ = model._tokenize_fused(xt, None, want_ze=False)
    idx_s, zq_s, ze_s = model._tokenize_fused(xt, None, want_ze=True)
    assert _same_bits(ze_s.cpu().numpy(), ze_ref)
    ok = ~np.isnan(ze_ref).any(axis=1)
    for idx, zq in ((idx_k, zq_k), (idx_s, zq_s)):
        assert np.array_equal(idx.cpu().numpy()[ok], idx_ref[ok])
        assert np.array_equal(zq.cpu().numpy()[ok].view(np.uint32), zq_ref[ok].view(np.uint32))
    assert torch.equal(idx_k, idx_s) and torch.equal(zq_k, zq_s)


# ---- the shape sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("K", [37, 256])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("A", [1, 7, 16])
@pytest.mark.parametrize("N", [1, 33, 293])
def test_shapes(oracle, lipvq_option, no_screen_monitor, N, A, D, K, shape):
    p = _p(oracle, A, D, K)
    x = O.make_inputs(N + A, N, A)
    ze, _, idx, zq = _reference(oracle, ("sweep", N, A, D, K), p, x)
    lipvq_option("tok_shape", shape)
    _check(_model(("sweep", A, D, K), p, A, D, K), x, ze, idx, zq)


# ---- planted rows ----------------------------------------------------------------------------------------------------------------
A_PL, K_PL, N_PL = 7, 256, 293


def _sq_ge18(v):
    """the kernel's own test, in fp32: !(v * v < 18)"""
    v = v.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return ~(v * v < np.float32(18.0))


def _one_of_pair(pre, r):
    """rows in which, for some tile and lane half, exactly ONE element of the packed pair (r, r + 1) has x^2 >= 18 and is finite"""
    J = pre.shape[1]
    f = np.array([32 * t + 2 * r + h for t in range(J // 32) for h in (0, 1)])
    big0, big1 = _sq_ge18(pre[:, f]), _sq_ge18(pre[:, f + 2])
    fin = np.isfinite(pre[:, f]) & np.isfinite(pre[:, f + 2])
    return ((big0 ^ big1) & fin).any(axis=1)


def _planted_rows(oracle, p, D):
    """x [N_PL][A_PL] of ordinary rows with planted ones among them, and a dict name -> row index.  The planted rows come from a
    seeded pool of scaled normal rows, picked by what the ORACLE says their pre-activations are."""
    rng = np.random.Generator(np.random.PCG64(4242 + D))
    # (the last three scales: finite inputs near the top of fp32, whose layer-2 sums overflow to an infinity of either sign)
    pool = np.concatenate([np.clip(s * rng.standard_normal((256, A_PL)), -3.3e38, 3.3e38).astype(np.float32)
                           for s in (4.0, 8.0, 16.0, 32.0, 64.0, 1e38, 1.5e38, 2e38)])
    assert np.isfinite(pool).all()
    _, pre = oracle.llfq_encode(p, pool, save_pre=True)
    fin_all = np.isfinite(pre[0]).all(axis=1) & np.isfinite(pre[1]).all(axis=1) & np.isfinite(pre[2]).all(axis=1)
    nonan2 = ~np.isnan(pre[2]).any(axis=1)
    picks = {
        "fixup0_first": _one_of_pair(pre[0], 0) & fin_all, "fixup0_last": _one_of_pair(pre[0], 14) & fin_all,
        "fixup1_first": _one_of_pair(pre[1], 0) & fin_all, "fixup1_last": _one_of_pair(pre[1], 14) & fin_all,
        "posinf2": np.isposinf(pre[2]).any(axis=1) & nonan2, "neginf2": np.isneginf(pre[2]).any(axis=1) & nonan2,
    }
    x = O.make_inputs(900 + D, N_PL, A_PL)
    # planted rows sit beside ordinary ones: wave 0 (rows 0-31), wave 1, the last wave of the first 8-wave block, the ragged tail
    slots = dict(fixup0_first=3, fixup0_last=37, fixup1_first=41, fixup1_last=250, posinf2=9, neginf2=50, nan=270, nan_tail=292)
    for name, mask in picks.items():
        assert mask.any(), f"the pool holds no row for {name}"
        x[slots[name]] = pool[np.flatnonzero(mask)[0]]
    x[slots["nan"]] = np.nan
    x[slots["nan_tail"], A_PL // 2] = np.nan
    return x, slots


@pytest.fixture(scope="module", params=[32, 64])
def planted(request, oracle):
    D = request.param
    p = _p(oracle, A_PL, D, K_PL)
    x, slots = _planted_rows(oracle, p, D)
    ze, pre, idx, zq = _reference(oracle, ("planted", D), p, x)
    return D, p, x, slots, ze, pre, idx, zq


def test_planted_rows_are_what_they_claim(planted):
    """CPU side of the planted launch (needs no GPU itself; it lives here so that the claim and the launch share one fixture)."""
    D, p, x, slots, ze, pre, idx, zq = planted
    for layer, r, name in ((0, 0, "fixup0_first"), (0, 14, "fixup0_last"), (1, 0, "fixup1_first"), (1, 14, "fixup1_last")):
        row = slots[name]
        assert _one_of_pair(pre[layer][row:row + 1], r)[0], name
        wave = slice(32 * (row // 32), 32 * (row // 32) + 32)
        others = np.delete(np.arange(wave.start, min(wave.stop, N_PL)), row - wave.start)
        # ... and the wave holds rows that stay on the polynomial in that layer
        assert (~_sq_ge18(pre[layer][others])).all(axis=1).any(), name
    assert np.isposinf(pre[2][slots["posinf2"]]).any() and not np.isnan(pre[2][slots["posinf2"]]).any()
    assert np.isneginf(pre[2][slots["neginf2"]]).any() and not np.isnan(pre[2][slots["neginf2"]]).any()
    assert np.isnan(pre[2][slots["nan"]]).all() and np.isnan(pre[2][slots["nan_tail"]]).any()
    for name in ("posinf2", "neginf2", "nan", "nan_tail"):              # ordinary rows in the same wave
        w0 = 32 * (slots[name] // 32)
        assert np.isfinite(pre[2][w0:w0 + 32]).all(axis=1).any(), name
    # a tile whose 16 values all differ (every tile of every layer of row 0, both lane halves): a pair swapped between two chains
    # cannot give the same tile
    for layer in range(3):
        J = pre[layer].shape[1]
        for t in range(J // 32):
            for h in (0, 1):
                assert np.unique(pre[layer][0, 32 * t + h:32 * t + 32:2]).size == 16, (layer, t, h)


@pytest.mark.parametrize("shape", SHAPES)
def test_planted_rows(planted, lipvq_option, no_screen_monitor, shape):
    """The fixup branch with its neighbour on the polynomial (first and last pair, both GELU layers), infinities and NaN into the
    sigmoid beside ordinary rows of the same wave, all in one launch."""
    D, p, x, slots, ze, pre, idx, zq = planted
    lipvq_option("tok_shape", shape)
    _check(_model(("planted", D), p, A_PL, D, K_PL), x, ze, idx, zq)


# ---- planted pre-activations: exact values --------------------------------------------------------------------------------------
A_EX, D_EX = 16, 64          # (fan-in 16: no padded k-step, whose + 0 * 0 would turn a -0 sum into +0)


def _largest_below_sqrt18():
    v = np.float32(np.sqrt(18.0))
    while not (v * v < np.float32(18.0)):
        v = np.nextafter(v, np.float32(0.0))
    assert not (np.nextafter(v, np.float32(9.0)) ** 2 < np.float32(18.0))
    return v


@pytest.fixture(scope="module")
def exact(oracle):
    """make_params' parameters with a few output features of layers 0 and 1 given zero weights (of a chosen sign) and a chosen bias:
    their pre-activation is that bias in every row.  Positive inputs, so that (-0) * x = -0 keeps a -0 bias a -0."""
    p = dict(_p(oracle, A_EX, D_EX, K_PL))
    v = _largest_below_sqrt18()
    plant = {}                       # (layer, feature) -> value
    for layer, (wk, bk) in enumerate((("encoder.0.weight", "encoder.0.bias"), ("encoder.2.weight", "encoder.2.bias"))):
        W, b = p[wk].copy(), p[bk].copy()
        base = 32 * layer            # layer 0: tile 0, layer 1: tile 1
        for f, val, wz in ((base + 0, v, 0.0), (base + 2, np.float32(0.0), 0.0), (base + 29, -v, 0.0), (base + 31, np.float32(-0.0), -0.0),
                           (base + 12, np.float32(-0.0), -0.0), (base + 14, v, 0.0)):
            W[f, :] = np.float32(wz)
            b[f] = val
            plant[(layer, f)] = val
        p[wk], p[bk] = W, b
    x = np.abs(O.make_inputs(77, N_PL, A_EX)) + np.float32(0.125)
    ze, pre, idx, zq = _reference(oracle, ("exact",), p, x)
    return p, x, plant, ze, pre, idx, zq


def test_exact_values_are_what_they_claim(exact):
    p, x, plant, ze, pre, idx, zq = exact
    for (layer, f), val in plant.items():
        col = pre[layer][:, f]
        if layer == 1 and val == 0 and np.signbit(val):
            # layer 1's inputs (GELU outputs) have both signs: (-0) * h is +0 for a negative h, and the sum then +0; rows where it
            # stayed -0 are not needed -- layer 0 has them
            assert (col == 0).all()
            continue
        assert np.array_equal(col.view(np.uint32), np.full(N_PL, val, np.float32).view(np.uint32)), (layer, f)
    v = _largest_below_sqrt18()
    assert v * v < np.float32(18.0) and not _sq_ge18(np.array([v, -v])).any()
    assert np.signbit(pre[0][:, 31]).all() and (pre[0][:, 31] == 0).all() and not np.signbit(pre[0][:, 2]).any()
    assert np.isfinite(ze).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_values(exact, lipvq_option, no_screen_monitor, shape):
    """+0, -0 and the largest |x| below sqrt(18), of either sign, in the first and the last pair of a tile and in the middle."""
    p, x, plant, ze, pre, idx, zq = exact
    lipvq_option("tok_shape", shape)
    _check(_model(("exact",), p, A_EX, D_EX, K_PL), x, ze, idx, zq)
