"""GPU: the bookkeeping of the screen loop at latent widths <= 64 (csrc/lipvq_screen.h: lq_pack_key, lq_track_one,
lq_track_after_mfma, and the stage loop of lq_screen_core, unrolled over one pass of the ring).  Which instruction books a value,
in which MFMA gap, and how the ring's addresses are formed is a schedule: per (row, lane class) the same values are booked in the
same order of tiles, so every answer is the oracle's and the unfused route's (mlp3 + exact all-pairs nearest), bit for bit, and
the number of rows the screen leaves to an exact decision (`last_exact_rows`) is a constant of the inputs.

  * 8 tiles (K = 37, 256: two stages at D = 32, four at D = 64 -- one pass of the ring, the peeled one) and 32 tiles (K = 1024:
    the ring wraps more than four times), rows 1, 33, 256 + 37, 2 * 256 + 37 under both workgroup shapes, a second row block per
    workgroup (the ring starts again), the launch without z_e and the storing one (stores in front of / behind the first copies);
  * K = 2304 (listed rows), K = 8192 under the three-product screen, and cfg3's widths (D = 128, K = 8192: the one-product
    screen, unpacked bookkeeping of an 8-k-step chain);
  * planted codebooks (built from the oracle's z_e on the CPU, each asserted there to be the case it is meant to be):
      (a) winner and runner-up one ulp apart in the SAME lane class (codes k and k + 32 j), in consecutive tiles, in the first and
          in the last tile, the winner in the earlier or in the later tile: the runner-up lives in the lane's m2 only;
      (b) the winner in tile 0 / the last tile for the rows of accumulator registers 0 and 15 in both halves of the wave;
      (c) exact duplicates of the winner (same lane class: the two keys differ in the tile bits only; another lane class: the
          decision's join sees them): never certified, the reference's first-index rule decides;
      (d) the upper half of the codebook one ulp from the lower half: every row a near-tie, `last_exact_rows` == N;
      (e) NaN, +-inf and +-1e30 input rows next to ordinary rows of the same wave.  torch.argmin of an all-NaN row is unspecified
          (csrc/lipvq_screen.hip), so a row whose z_e is not finite is compared with the unfused route and the storing instance, the
          finite rows with the oracle as everywhere else.

EXACT_ROWS holds `last_exact_rows` of four seeded launches as the build this schedule was changed from left them (commit 936cb6a,
measured on an MI355X with

    LIPVQ_HIP_LIBRARY=<that build's _lipvq_hip.so> python tests/test_gpu_tokenize_booking.py

which prints the dictionary; seeds: torch.manual_seed(2000 + K), bench.trained_like_(seed=K + 1), O.make_inputs(1900 + K, N, 7)).
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import lipvq_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

A = 7
SHAPES = ["w8rg1", "w4rg1"]
N_SECOND = {"w8rg1": 65536 + 256 + 37, "w4rg1": 32768 + 128 + 37}     # 256 workgroups x one row block, one more block, a ragged one
N_CONST = 65536 + 256 + 37

# (K, tok_shape) -> rows of the N_CONST-row launch left to an exact decision, D = 64 (module docstring); parent commit 936cb6a
EXACT_ROWS = {
    (256, "w8rg1"): 137,
    (256, "w4rg1"): 137,
    (1024, "w8rg1"): 230,
    (1024, "w4rg1"): 230,
}

_models = {}
_refs = {}
_oracle = []


def _orc():
    if not _oracle:
        _oracle.append(O.CanonicalOracle())
    return _oracle[0]


def _params(model):
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in model.state_dict().items()}


def _model(fan_in, D, K, tag="plain", codebook=None, seeds=None):
    """(model on the GPU, its parameters as numpy arrays): bench.trained_like_ parameters; `codebook(cb, p)` -> the codebook to
    use instead (planted cases).  Built once per (shape, tag), never modified afterwards."""
    key = (fan_in, D, K, tag)
    if key not in _models:
        import bench
        from lipvq_vae_amd.tokenizer import LLFQVAE_V4
        s_torch, s_like = seeds if seeds else (1000 + D, D)
        torch.manual_seed(s_torch)
        model = LLFQVAE_V4(fan_in, D, num_codes=K).cuda()
        bench.trained_like_(model, fan_in, seed=s_like)
        if codebook is not None:
            p = _params(model)
            cb = codebook(p["quantizer.codebook"].copy(), p)
            with torch.no_grad():
                model.quantizer.codebook.copy_(torch.from_numpy(cb).cuda())
        _models[key] = (model, _params(model))
    return _models[key]


def _reference(key, p, x):
    """the C oracle's (z_e, idx, usage) of one (parameters, inputs) pair: computed once, shared, never modified"""
    if key not in _refs:
        ze = _orc().llfq_encode(p, x)
        idx, _, usage = _orc().nearest(ze, p["quantizer.codebook"])
        _refs[key] = (ze, idx, usage)
    return _refs[key]


def _launch(model, xt):
    """model.tokenize (the caller wants no z_e) -> idx, zq, usage, rows decided by an exact stage"""
    model.reset_usage()
    idx, zq = model.tokenize(xt)
    return idx, zq, model.code_usage.clone(), int(model.last_exact_rows[0])


def _check(model, p, x, ref_key, set_option, storing=True):
    """The launch without z_e (twice: same answers, same number of uncertified rows), the unfused route and the storing instance
    (its last tile's stores in front of the screen and behind its first copies) against the oracle, everything with ==.  Rows whose
    z_e is not finite (module docstring, (e)) are held to the unfused route instead of the oracle.  -> rows left to an exact decision"""
    from lipvq_vae_amd import ops
    N = x.shape[0]
    xt = torch.from_numpy(x).cuda()
    cb = model.quantizer.codebook.detach()
    ze_ref, idx_ref, usage_ref = _reference(ref_key, p, x)
    fin = np.isfinite(ze_ref).all(axis=1)
    idx, zq, usage, exact = _launch(model, xt)
    idx2, zq2, usage2, exact2 = _launch(model, xt)
    print(f"N={N} A={x.shape[1]} D={model.latent_dim} K={model.num_codes}: exact rows {exact}, {exact2}; rows with a non-finite z_e {int((~fin).sum())}")
    assert np.array_equal(idx.cpu().numpy()[fin], idx_ref[fin])
    assert int(idx.min()) >= 0 and int(idx.max()) < model.num_codes
    assert torch.equal(zq, cb[idx])
    assert int(usage.sum()) == N
    if fin.all():
        assert np.array_equal(usage.cpu().numpy(), usage_ref)
    assert torch.equal(idx2, idx) and torch.equal(zq2, zq) and torch.equal(usage2, usage) and exact2 == exact
    # the unfused route
    ze_u = model.encode(xt)
    idx_u, zq_u, _ = ops.nearest(ze_u, cb, ops.DIST_NORM)
    assert np.array_equal(ze_u.cpu().numpy(), ze_ref, equal_nan=True)
    assert torch.equal(idx_u, idx) and torch.equal(zq_u, zq)
    if storing:
        for defer in ("0", "1"):
            set_option("tok_defer_ze", defer)
            idx_s, zq_s, ze_s = model._tokenize_fused(xt, None, want_ze=True)
            assert torch.equal(idx_s, idx) and torch.equal(zq_s, zq)
            assert np.array_equal(ze_s.cpu().numpy(), ze_ref, equal_nan=True)
    return exact


# ---- shapes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("K", [37, 256, 1024])
def test_tile_and_row_counts(lipvq_option, no_screen_monitor, K, D, shape):
    """8 and 32 tiles; one row, one row past a wave, a ragged second and third row block."""
    model, p = _model(A, D, K)
    lipvq_option("tok_shape", shape)
    for N in (1, 33, 256 + 37, 2 * 256 + 37):
        x = O.make_inputs(100 + K + D, 2 * 256 + 37, A)[:N]
        _check(model, p, x, ("counts", K, D, N), lipvq_option)


@pytest.mark.parametrize("shape", SHAPES)
def test_second_block_per_workgroup(lipvq_option, no_screen_monitor, shape):
    """256 workgroups, then one more full row block and a ragged one: workgroups 0 and 1 run the ring a second time."""
    D, K = 64, 256
    model, p = _model(A, D, K)
    lipvq_option("tok_shape", shape)
    N = N_SECOND[shape]
    x = O.make_inputs(410, N_SECOND["w8rg1"], A)[:N]
    _check(model, p, x, ("second", N), lipvq_option)


@pytest.mark.parametrize("shape", SHAPES)
def test_codebook_past_the_inplace_limit(lipvq_option, no_screen_monitor, shape):
    """K = 2304 > 2048: no in-place decisions -- the launch stores z_e and lists its uncertified rows."""
    D, K = 64, 2304
    model, p = _model(A, D, K)
    lipvq_option("tok_shape", shape)
    x = O.make_inputs(210, 2 * 256 + 37, A)
    _check(model, p, x, ("past", K, D), lipvq_option)


def test_large_codebook_under_the_three_product_screen(lipvq_option, no_screen_monitor):
    """K = 8192 with screen_mode = fine: 128 stages through the ring, 8 tile bits in the packed keys."""
    D, K = 64, 8192
    model, p = _model(A, D, K)
    lipvq_option("screen_mode", "fine")
    x = O.make_inputs(260, 2 * 256 + 37, A)
    _check(model, p, x, ("fine", K, D), lipvq_option)


def test_one_product_launch(lipvq_option, no_screen_monitor):
    """cfg3's widths: the one-product screen (an accumulator seeded per tile, one MFMA per k-step) and the unpacked bookkeeping."""
    D, K = 128, 8192
    model, p = _model(A, D, K)
    x = O.make_inputs(270, 2 * 256 + 37, A)
    _check(model, p, x, ("coarse", K, D), lipvq_option)


# ---- planted codebooks ---------------------------------------------------------------------------------------------------------

N_PLANT = 64            # two waves of rows, every one planted
PLANT_SHAPES = [(64, 1024), (32, 256)]


def _plant_inputs(D):
    return O.make_inputs(700 + D, N_PLANT, A)


def _ulp_up(z, j):
    e = z.copy()
    e[j] = np.nextafter(e[j], np.float32(2.0))
    return e


def _tile_pairs(ntiles):
    """consecutive tiles at the start, in the middle and at the end of the pass, and the first with the last"""
    return [(0, 1), (5, 6), (ntiles - 2, ntiles - 1), (0, ntiles - 1)]


def _slots_a(n, ntiles):
    """row n -> (code of the earlier tile, code of the later tile) in lane class n % 32; rows n and n + 32 get disjoint tiles"""
    t0, t1 = _tile_pairs(ntiles)[(n if n < 32 else n + 2) % 4]
    return 32 * t0 + n % 32, 32 * t1 + n % 32


def _plant_same_lane(D, K, dup):
    """(a) / (c): per row an exact copy of its z_e and, in the same lane class of another tile, a copy one ulp away in its largest
    coordinate (dup: an exact copy); the exact copy sits in the earlier tile for rows with (n // 4) % 2 == 0, in the later tile
    for the others.  dup, odd rows: the second copy goes to lane class (n + 16) % 32 instead."""
    x = _plant_inputs(D)

    def codebook(cb, p):
        ze = _orc().llfq_encode(p, x)
        for n in range(N_PLANT):
            k0, k1 = _slots_a(n, K // 32)
            if dup and n % 2 == 1:
                k1 = (k1 & ~31) | ((n + 16) % 32)
            win, run = (k0, k1) if (n // 4) % 2 == 0 else (k1, k0)
            cb[win] = ze[n]
            cb[run] = ze[n] if dup else _ulp_up(ze[n], int(np.argmax(ze[n])))
        return cb

    return x, codebook


def _two_best(ze_row, cb):
    d = ((cb.astype(np.float64) - ze_row.astype(np.float64)) ** 2).sum(axis=1)
    o = np.argsort(d, kind="stable")
    return int(o[0]), int(o[1]), d[o[0]], d[o[1]], d[o[2]]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("D,K", PLANT_SHAPES)
def test_runner_up_in_the_winners_lane_class(lipvq_option, no_screen_monitor, D, K, shape):
    """(a): the only trace of the runner-up is the lane's second minimum.  Every row is a near-tie: none may be certified."""
    x, codebook = _plant_same_lane(D, K, dup=False)
    model, p = _model(A, D, K, tag="same-lane", codebook=codebook)
    ze, idx_ref, _ = _reference(("same-lane", D, K), p, x)
    cb = p["quantizer.codebook"]
    for n in range(N_PLANT):
        k0, k1 = _slots_a(n, K // 32)
        win, run = (k0, k1) if (n // 4) % 2 == 0 else (k1, k0)
        b0, b1, d0, d1, d2 = _two_best(ze[n], cb)
        assert (b0, b1) == (win, run) and idx_ref[n] == win and d0 == 0.0 and 0.0 < d1 < 1e-12 < d2, (n, b0, b1, win, run, d0, d1, d2)
        assert win % 32 == run % 32 == n % 32
    tiles = {(int(i) // 32) for i in idx_ref}
    assert 0 in tiles and K // 32 - 1 in tiles
    lipvq_option("tok_shape", shape)
    exact = _check(model, p, x, ("same-lane", D, K), lipvq_option)
    assert exact == N_PLANT


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("D,K", PLANT_SHAPES)
def test_exact_duplicates(lipvq_option, no_screen_monitor, D, K, shape):
    """(c): two codes with the winner's bits -- in one lane class (keys equal up to the tile bits) on even rows, in two on odd rows.
    The reference takes the lower index; the screen may not certify either."""
    x, codebook = _plant_same_lane(D, K, dup=True)
    model, p = _model(A, D, K, tag="dup", codebook=codebook)
    ze, idx_ref, _ = _reference(("dup", D, K), p, x)
    cb = p["quantizer.codebook"]
    for n in range(N_PLANT):
        k0, k1 = _slots_a(n, K // 32)
        if n % 2 == 1:
            k1 = (k1 & ~31) | ((n + 16) % 32)
        assert np.array_equal(cb[k0].view(np.int32), cb[k1].view(np.int32)) and np.array_equal(cb[k0], ze[n])
        assert (k0 % 32 == k1 % 32) == (n % 2 == 0)
        assert idx_ref[n] == min(k0, k1), (n, idx_ref[n], k0, k1)
    lipvq_option("tok_shape", shape)
    exact = _check(model, p, x, ("dup", D, K), lipvq_option)
    assert exact == N_PLANT


def _row_register(i):
    """row i of a wave's 32 -> (accumulator register, half of the wave) that hold it (lq_row_factors)"""
    return (i & 3) + 4 * (i >> 3), (i >> 2) & 1


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("D,K", PLANT_SHAPES)
def test_winner_at_the_corners(lipvq_option, no_screen_monitor, D, K, shape):
    """(b): registers 0 and 15 (the first and the last element booked of a tile), both halves of the wave, the pass's first tile
    (booked against the +inf of "no tile yet") in wave 0 and its last tile (booked after the loop) in wave 1."""
    x = _plant_inputs(D)
    rows = [0, 4, 27, 31]
    assert sorted(_row_register(i) for i in rows) == [(0, 0), (0, 1), (15, 0), (15, 1)]
    want = {}
    for w, tile in ((0, 0), (1, K // 32 - 1)):
        for i in rows:
            want[32 * w + i] = 32 * tile + i

    def codebook(cb, p):
        ze = _orc().llfq_encode(p, x)
        for n, k in want.items():
            cb[k] = ze[n]
        return cb

    model, p = _model(A, D, K, tag="corners", codebook=codebook)
    ze, idx_ref, _ = _reference(("corners", D, K), p, x)
    for n, k in want.items():
        b0, _, d0, d1, _ = _two_best(ze[n], p["quantizer.codebook"])
        assert b0 == k == idx_ref[n] and d0 == 0.0 and d1 > 0.0, (n, k, b0, idx_ref[n], d0, d1)
    lipvq_option("tok_shape", shape)
    _check(model, p, x, ("corners", D, K), lipvq_option)


def _dup_upper_half(cb, p):
    """cb[c] for c >= K/2 becomes cb[c - K/2] moved by one ulp in coordinate c % D (tests/test_gpu_tokenize_keepz.py)"""
    K, D = cb.shape
    half = K // 2
    cb[half:] = cb[:half]
    j = np.arange(half) % D
    cb[half + np.arange(half), j] = np.nextafter(cb[np.arange(half), j], np.float32(2.0))
    return cb


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("D,K", PLANT_SHAPES)
def test_every_row_a_near_tie(lipvq_option, no_screen_monitor, D, K, shape):
    """(d): winner and runner-up K/2 codes apart (the same lane class, K/64 tiles apart) on every row of three row blocks."""
    model, p = _model(A, D, K, tag="upper-half", codebook=_dup_upper_half)
    N = 2 * 256 + 37
    x = O.make_inputs(40 + D, N, A)
    ze, _, _ = _reference(("upper-half", D, K), p, x)
    d = np.sort(_orc().distances(ze, p["quantizer.codebook"]), axis=1)
    assert ((d[:, 1] - d[:, 0]) < 1e-6 * d[:, 0]).all()
    lipvq_option("tok_shape", shape)
    exact = _check(model, p, x, ("upper-half", D, K), lipvq_option)
    assert exact == N


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("D,K", PLANT_SHAPES)
def test_nonfinite_rows_beside_ordinary_ones(lipvq_option, no_screen_monitor, D, K, shape):
    """(e): the keys of a row that is not sane are booked like any others (NaN and +-inf through and_or, med3, min), beside the
    rows of the same wave, whose answers they must not touch."""
    model, p = _model(A, D, K)
    N = 256 + 37
    x = O.make_inputs(800 + D, N, A)
    x[3] = np.nan
    x[9] = np.inf
    x[14] = -np.inf
    x[20] = 1e30
    x[25] = -1e30
    x[40, 2] = np.nan
    x[70, 0] = np.inf
    x[260] = np.nan
    lipvq_option("tok_shape", shape)
    ze, _, _ = _reference(("nonfinite", D, K), p, x)
    assert not np.isfinite(ze[3]).all() and np.isfinite(ze[4]).all()
    _check(model, p, x, ("nonfinite", D, K), lipvq_option)


# ---- the count of uncertified rows ---------------------------------------------------------------------------------------------

def _exact_rows_const(K, shape, set_option):
    """the two counts of the module docstring's launch, and its indices"""
    model, _ = _model(A, 64, K, tag="const", seeds=(2000 + K, K + 1))
    set_option("tok_shape", shape)
    xt = torch.from_numpy(O.make_inputs(1900 + K, N_CONST, A)).cuda()
    idx, _, _, e1 = _launch(model, xt)
    idx2, _, _, e2 = _launch(model, xt)
    assert torch.equal(idx, idx2)
    return e1, e2, idx, xt


@pytest.mark.parametrize("K,shape", sorted(EXACT_ROWS))
def test_uncertified_rows_are_the_parents(lipvq_option, no_screen_monitor, K, shape):
    """Every m1, m2 and packed key is the same bits as before, so the screen certifies the same rows."""
    from lipvq_vae_amd import ops
    e1, e2, idx, xt = _exact_rows_const(K, shape, lipvq_option)
    print(f"K={K} {shape}: exact rows {e1}, {e2}; recorded {EXACT_ROWS[(K, shape)]}")
    assert e1 == e2
    assert e1 == EXACT_ROWS[(K, shape)]
    model, _ = _model(A, 64, K, tag="const")
    idx_u, _, _ = ops.nearest(model.encode(xt), model.quantizer.codebook.detach(), ops.DIST_NORM, want_zq=False)
    assert torch.equal(idx_u, idx)


if __name__ == "__main__":
    # prints EXACT_ROWS for the library in use (module docstring)
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd import _capi
    from lipvq_vae_amd.tokenizer import _ScreenMonitor
    _ScreenMonitor.ENABLED = False
    print("library:", _capi._LIB_PATH)
    print("EXACT_ROWS = {")
    for (K_, shape_) in sorted(EXACT_ROWS):
        a_, b_, _, _ = _exact_rows_const(K_, shape_, _capi.set_option)
        assert a_ == b_, (a_, b_)
        print(f"    ({K_}, \"{shape_}\"): {a_},")
    print("}")
