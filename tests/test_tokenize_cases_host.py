"""CPU: the inputs of tests/test_gpu_tokenize_instances.py (tests/tokenize_cases.py) are the cases they claim to be, shown with the
C oracle, and each separates a wrong implementation of the property under test from the right one -- so the GPU assertion can
fail.  Per planted input, the wrong variant:

  ring, second lap       the in-place decision reads the z_e row another row block left in the ring (row n decided from
                         z_e[n - lap]): another index on most rows of the second lap
  (a) same lane class    a near-tie resolved towards the earlier tile (the lane's second minimum lost): wrong where the winner sits
                         in the later tile
  (b) corners            a pass that loses its first / last tile: the winner is gone
  (c) duplicates         the later of two equal codes: not the first index
  (d) upper half         twins resolved towards the lower index: wrong where the oracle takes the upper twin
  half-used last tile    a chain that drops its last (or first) k-step sees an exact tie and the first index is the wrong code
  ragged last tile       a pass that stops at the last full tile loses code K - 1
  VQ, scales             fp16 fragments without the row's / the codebook's own power of two: overflow or underflow, other indices
  VQ, dead rows          a row that cannot be scaled answered with code 0: not the code nearest to the origin
  centring vector        any rule but "first index" among 64 equal distances
"""
import numpy as np
import pytest

import tokenize_cases as C

A = 7


def _argmin_first(ze, cb, cols=slice(None), codes=slice(None)):
    d = ((cb[codes, cols].astype(np.float64)[None] - ze[:, None, cols].astype(np.float64)) ** 2).sum(axis=2)
    return d.argmin(axis=1)


# ---- the restated selection rule ---------------------------------------------------------------------------------------------------

def test_the_instances_the_gpu_tests_name():
    i = C.instance("llfq", 128, 256, 32768 + 128 + 37, shape="w4rg1")
    assert (i["S"], i["WAVES"], i["COARSE"], i["KEEPZ"], i["ring"], i["inplace"], i["PACKF"]) == (8, 4, False, False, True, True, False)
    assert i["lap"] == 32768 and i["unit"] == 128
    i = C.instance("llfq", 128, 256, 65536 + 256 + 37, shape="w8rg1", want_ze=True)
    assert (i["WAVES"], i["ring"], i["inplace"]) == (8, False, True)
    i = C.instance("llfq", 128, 256, 300, shape="w8rg1", inplace_opt=False)
    assert (i["ring"], i["inplace"]) == (False, False)
    i = C.instance("llfq", 64, 256, 300)                                   # the narrow parity launch keeps z_e in registers: no ring
    assert i["KEEPZ"] and not i["ring"] and i["WAVES"] == 4
    i = C.instance("llfq", 32, 256, 65536 + 256 + 37, fast=True)           # ... the fast mode's does not
    assert (i["FAST"], i["WAVES"], i["ring"], i["KEEPZ"], i["COARSE"]) == (True, 8, True, False, False)
    assert not C.instance("llfq", 32, 256, 131073, fast=True)["ring"]
    i = C.instance("llfq", 208, 1024, 300, shape="w4rg1")                  # default screen of a wide latent from K = 1024: one product
    assert (i["S"], i["COARSE"], i["WAVES"], i["inplace"], i["PACKF"]) == (13, True, 4, False, True)
    i = C.instance("llfq", 128, 1024, 300, screen="fine", want_pre=True)
    assert (i["TRAIN"], i["WAVES"], i["inplace"], i["ring"], i["PACKF"]) == (True, 8, True, False, False)
    i = C.instance("llfq", 128, 2049, 300, shape="w4rg1")
    assert i["COARSE"] and i["WAVES"] == 4 and not i["inplace"]
    i = C.instance("vq", 32, 256, 300, shape="w4rg1")
    assert (i["VQ"], i["WAVES"], i["inplace"], i["ring"], i["COARSE"]) == (True, 8, True, False, False)
    assert C.instance("vq", 128, 1024, 300, screen="coarse", want_pre=True)["COARSE"]


def test_fan_ins_the_fused_launch_has_lds_for():
    """the pure host query: D = 128 (layer 2 resident in LDS) up to a fan-in of 40, every other width up to 64"""
    from lipvq_vae_amd import ops
    for D, last in ((32, 64), (64, 64), (128, 40), (208, 64)):
        assert ops.tokenize_supported(last, 64, 128, D, 256) and not ops.tokenize_supported(last + 1, 64, 128, D, 256), D
        assert ops.tokenize_supported(1, 64, 128, D, 256)
    assert not ops.tokenize_fast_supported(7, 64, 128, 208, 256) and ops.tokenize_fast_supported(64, 64, 128, 128, 256)


# ---- A: the ring's second lap ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,shape,fast", [(128, "w4rg1", False), (128, "w8rg1", False), (208, "w4rg1", False), (32, None, True)])
def test_ring_cases_have_near_ties_in_both_laps_and_a_stale_row_shows(D, shape, fast):
    p, x, inst = C.ring_case(D, shape, fast)
    N, lap, unit = x.shape[0], inst["lap"], inst["unit"]
    assert inst["ring"] and N == lap + unit + 37
    ref = C.answers(("ring", D, shape, fast), "llfq", p, x)
    tie = C.near_tie_rows("llfq", p, ref["ze"])
    # workgroup 0 runs rows [0, unit) and, in its second lap, [lap, lap + unit); workgroup 1's second block is the ragged one
    assert tie[:unit].all() and tie[lap:lap + unit].all() and tie[lap + unit:].all() and tie.all()
    # every code has a twin one ulp away, whatever z_e is (the fast mode's differs from the oracle's): no row can be certified
    cb = p[C.CB_KEY["llfq"]]
    half = cb.shape[0] // 2
    gap = (cb[half:].view(np.int32) - cb[:half].view(np.int32))
    assert ((gap != 0).sum(axis=1) == 1).all() and gap.max() == 1 and gap.min() == 0
    # the wrong ring: row n of the second lap decided from the row the first lap left in its slot
    stale = ref["idx"][:N - lap]
    differs = stale != ref["idx"][lap:]
    print(f"D={D} {shape}: {int(differs.sum())} of {N - lap} second-lap rows get another index from the first lap's z_e")
    assert differs.sum() > (N - lap) // 2


# ---- B / D: the planted families ----------------------------------------------------------------------------------------------------------

PLANT_SHAPES = [(128, 256), (128, 1024), (128, 2049), (208, 1024), (208, 2049)]


def _planted(plant, D, K):
    p, x = C.planted(plant, A, D, K)
    ref = C.answers(("planted", plant, A, D, K), "llfq", p, x)
    return p, x, ref, p[C.CB_KEY["llfq"]]


@pytest.mark.parametrize("D,K", [(128, 256), (128, 1024)])
def test_runner_up_in_the_winners_lane_class(D, K):
    p, x, ref, cb = _planted("same-lane", D, K)
    later = 0
    for n in range(C.N_PLANT):
        win, run = C.slots_same_lane(n, K, dup=False)
        b0, b1, d0, d1, d2 = C.two_best(ref["ze"][n], cb)
        assert (b0, b1) == (win, run) and ref["idx"][n] == win and d0 == 0.0 and 0.0 < d1 < 1e-12 < d2, (n, b0, b1, win, run, d0, d1, d2)
        assert win % 32 == run % 32 == n % 32
        assert np.abs(cb[win].view(np.int32) - cb[run].view(np.int32)).sum() == 1            # one ulp in one coordinate
        later += win > run                                                                      # (the wrong variant answers `run` here)
    tiles = {int(i) // 32 for i in ref["idx"][:C.N_PLANT]}
    assert 0 in tiles and K // 32 - 1 in tiles and later == C.N_PLANT // 2


@pytest.mark.parametrize("D,K", PLANT_SHAPES)
def test_exact_duplicates(D, K):
    p, x, ref, cb = _planted("dup", D, K)
    for n in range(C.N_PLANT):
        k0, k1 = C.slots_same_lane(n, K, dup=True)
        assert np.array_equal(cb[k0].view(np.int32), cb[k1].view(np.int32)) and np.array_equal(cb[k0], ref["ze"][n])
        assert (k0 % 32 == k1 % 32) == (n % 2 == 0)
        assert ref["idx"][n] == min(k0, k1) != max(k0, k1)
    if K % 32:
        # the ragged last tile holds one code, and it wins a row: a pass that ends at the last full tile answers otherwise
        r = C.RAGGED_ROW
        assert K - 1 == 32 * (K // 32) and ref["idx"][r] == K - 1
        assert _argmin_first(ref["ze"][r:r + 1], cb, codes=slice(0, K - 1))[0] != K - 1


@pytest.mark.parametrize("D,K", [(128, 256), (128, 1024), (208, 256), (208, 1024)])
def test_winner_at_the_corners(D, K):
    p, x, ref, cb = _planted("corners", D, K)
    assert sorted(C.row_register(i) for i in C.CORNER_ROWS) == [(0, 0), (0, 1), (15, 0), (15, 1)]
    want = C.corner_slots(K)
    assert {k // 32 for k in want.values()} == {0, K // 32 - 1} and len(want) == 8
    for n, k in want.items():
        b0, _, d0, d1, _ = C.two_best(ref["ze"][n], cb)
        assert b0 == k == ref["idx"][n] and d0 == 0.0 and d1 > 0.0, (n, k, b0, d0, d1)
        tile = slice(32 * (k // 32), 32 * (k // 32) + 32)
        lost = np.delete(np.arange(K), np.arange(K)[tile])
        assert lost[_argmin_first(ref["ze"][n:n + 1], cb[lost])[0]] != k                       # a pass without that tile


@pytest.mark.parametrize("D,K", PLANT_SHAPES)
def test_every_row_a_near_tie(D, K):
    p, x, ref, cb = _planted("upper-half", D, K)
    assert C.near_tie_rows("llfq", p, ref["ze"]).all()
    half = K // 2
    twin = np.where(ref["idx"] < half, ref["idx"] + half, ref["idx"] - half)
    assert (ref["idx"] < 2 * half).all()                                                        # (an odd K's last code wins nothing)
    d = C.orc().distances(ref["ze"], cb)
    n = np.arange(x.shape[0])
    assert (np.abs(d[n, twin] - d[n, ref["idx"]]) < 1e-6 * d[n, ref["idx"]]).all()
    assert (ref["idx"] >= half).sum() > 0                                                       # twins resolved downwards: wrong there


@pytest.mark.parametrize("K", [256, 1024])
def test_half_used_last_tile(K):
    D = C.HALF_TILE_D
    p, x, ref, cb = _planted("half-tile", D, K)
    ze = ref["ze"]
    for n in range(C.N_PLANT):
        last, first, win = C.half_tile_slots(n)
        assert last < first < win
        dl, df = cb[last] != cb[win], cb[first] != cb[win]
        assert dl[C.HALF_TILE_LAST].all() and dl.sum() == 16 and df[C.HALF_TILE_FIRST].all() and df.sum() == 16
        b0, _, d0, d1, _ = C.two_best(ze[n], cb)
        assert b0 == win == ref["idx"][n] and d0 == 0.0 and d1 > 0.0
    rows = ze[:C.N_PLANT]
    want = np.array([C.half_tile_slots(n) for n in range(C.N_PLANT)])
    # the chain without its last k-step (features 192 .. 207 dropped, or read from the tile's unused half, which holds zeros
    # for the row and for every code alike), and without its first
    assert np.array_equal(_argmin_first(rows, cb, cols=slice(0, 192)), want[:, 0])
    assert np.array_equal(_argmin_first(rows, cb, cols=slice(16, 208)), want[:, 1])
    assert np.array_equal(_argmin_first(rows, cb), want[:, 2])


# ---- F: the plain VQVAE's edges ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,K", [(32, 256), (128, 256), (32, 1024), (128, 1024)])
def test_vq_scale_sweep(D, K):
    p0 = C.params("vq", A, D, K)
    x = C.inputs(C.X_SEED + 60 + D, C.N_EDGE, A)
    ref0 = C.answers(("vq-scale", D, K, 0), "vq", p0, x)
    cb0 = p0[C.CB_KEY["vq"]]
    mu0 = cb0.astype(np.float64).mean(axis=0)
    amax = np.abs(ref0["ze"] - mu0).max(axis=1)
    emax = np.abs(2.0 * (cb0 - mu0)).max()
    assert amax.min() > 0
    broken = 0
    for e in C.SCALE_EXPONENTS:
        p = C.scaled(p0, e)
        ref = C.answers(("vq-scale", D, K, e), "vq", p, x)
        assert np.array_equal(ref["ze"].astype(np.float64), ref0["ze"].astype(np.float64) * 2.0 ** e)      # exact, no overflow
        assert np.isfinite(C.orc().distances(ref["ze"], p[C.CB_KEY["vq"]], C.DIST["vq"])).all()
        assert np.array_equal(ref["idx"], ref0["idx"]), e                                                   # every exponent is kept
        # inside lq_scale_exp's clamp on both sides: k = 13 - floor(log2 max) in [-60, 60] for every row and for the codebook
        for m in (amax.min(), amax.max(), emax):
            assert abs(13 - int(np.floor(np.log2(m * 2.0 ** e)))) < C.SCALE_EXP_CLAMP, (e, m)
        # the wrong variant: fp16 operands without their power of two
        with np.errstate(over="ignore", invalid="ignore"):
            z16 = (ref["ze"] - p[C.CB_KEY["vq"]].mean(axis=0)).astype(np.float16).astype(np.float64)
            c16 = (p[C.CB_KEY["vq"]] - p[C.CB_KEY["vq"]].mean(axis=0)).astype(np.float16).astype(np.float64)
            d16 = ((c16[None] - z16[:, None]) ** 2).sum(axis=2)
        wrong = np.where(np.isfinite(d16).all(axis=1), d16.argmin(axis=1), 0)
        if e in (-20, 20, 40):
            assert (wrong != ref["idx"]).any(), e
            broken += 1
    assert broken == 3


@pytest.mark.parametrize("D,K", [(32, 256), (128, 256), (32, 1024), (128, 1024)])
def test_vq_dead_rows(D, K):
    p = C.dead("vq", C.params("vq", A, D, K))
    for all_zero in (False, True):
        x, rows = C.dead_inputs(A, all_zero)
        ref = C.answers(("vq-dead", D, K, all_zero), "vq", p, x)
        assert (ref["ze"][rows] == 0.0).all() and (x[rows] == 0.0).all()
        is_dead = (ref["ze"] == 0.0).all(axis=1)                  # (with negative biases some ordinary rows die as well)
        live = np.flatnonzero(~is_dead)
        if not all_zero:
            assert set(rows // 32) == {0, 1} and {0, 1} <= set(live // 32)                       # dead and live rows share a wave
            assert live.size >= 32
        else:
            assert live.size == 0
        k0 = int(np.argmin((p[C.CB_KEY["vq"]].astype(np.float64) ** 2).sum(axis=1)))
        assert k0 != 0 and (ref["idx"][is_dead] == k0).all()                                    # "cannot scale it: code 0" is wrong


@pytest.mark.parametrize("variant", ["vq", "llfq"])
@pytest.mark.parametrize("D", [32, 128])
def test_rows_equal_to_the_centring_vector(variant, D):
    p = C.centred(variant, A, D)
    x = C.inputs(C.X_SEED + 70 + D, C.N_EDGE, A)
    ref = C.answers(("centred", variant, D), variant, p, x)
    cb = p[C.CB_KEY[variant]]
    mu = cb.sum(axis=0, dtype=np.float32) / np.float32(C.CENTRE_K)
    assert (mu == C.CENTRE).all() and (ref["ze"] == C.CENTRE).all() and ((ref["ze"] - mu) == 0.0).all()
    d = C.orc().distances(ref["ze"], cb, C.DIST[variant])
    assert (d == d[:, :1]).all()                                                                # 64 equal distances per row
    assert (ref["idx"] == 0).all() and ref["usage"][0] == x.shape[0]                            # the first index, nothing else


@pytest.mark.parametrize("variant", ["vq", "llfq"])
def test_nonfinite_rows(variant):
    D, K = 128, 256
    p = C.params(variant, A, D, K)
    x, nan_rows, inf_rows, big_rows = C.nonfinite_inputs(A)
    ref = C.answers(("nonfinite", variant, D, K), variant, p, x)
    fin = np.isfinite(ref["ze"]).all(axis=1)
    planted = np.concatenate([nan_rows, inf_rows, big_rows])
    assert np.unique(planted).size == planted.size == 10 + 32
    assert np.isin(np.flatnonzero(~fin), planted).all()                                         # at most the planted rows
    ordinary = np.setdiff1d(np.arange(x.shape[0]), planted)
    assert fin[ordinary].all() and np.isfinite(x[ordinary]).all()
    print(f"{variant}: non-finite z_e in {int((~fin)[nan_rows].sum())}/{nan_rows.size} NaN rows, {int((~fin)[inf_rows].sum())}/"
          f"{inf_rows.size} inf rows, {int((~fin)[big_rows].sum())}/{big_rows.size} rows of 1e30 / 1e37")
    if variant == "llfq":
        assert (~fin)[nan_rows].all()                                                           # GELU and sigmoid keep a NaN
    # beside ordinary rows of the same wave, and a wave of their own
    assert set(range(96, 128)) <= set(planted) and all(np.isin(np.arange(32 * w, 32 * w + 32), ordinary).any() for w in (0, 1, 2, 8))
