"""CPU: tests/bin_ref.py held to the conditions its GPU users (tests/test_gpu_bin_edges.py, tests/test_gpu_update_edges.py) rely on:
every builder is seeded, the canonical oracle equals stock torch on every entry of the edge-value tables (NaN statistics included),
every boundary neighbour differs from its boundary, the large gradient shapes really have a hot bin, and the float64 references of
the update kernels are finite wherever the state table does not say otherwise."""
import numpy as np
import pytest
import torch

import bin_ref as B


def test_builders_are_seeded():
    for build in (lambda: B.hidden_case(65, 5, 96, 5), lambda: B.nan_case(7, 9), lambda: (B.minmax_case(63, 9),),
                  lambda: (B.grad_actions(1000, 3, 20),), lambda: B.scatter_case(1000, 5, 16), lambda: B.mse_pair_case(5, 3, big=True),
                  lambda: tuple(B.ema_state(37, 5, "typical")[k] for k in ("cs", "es", "counts", "dw")),
                  lambda: (B.adamw_grad("tiny", 255, 2, 0), np.array(B.adamw_sizes(33)))):
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(build(), build()))


# ---- A.1  the oracle's table sum at widths it had never been used at ---------------------------------------------------------------

@pytest.mark.parametrize("N", B.HIDDEN_WIDE_N)
@pytest.mark.parametrize("A,nb,H", B.HIDDEN_WIDE)
def test_oracle_hidden_within_the_recursive_summation_bound(oracle, A, nb, H, N):
    bins, P, b1 = B.hidden_case(A, nb, H, N)
    assert bins.min() == 0 and bins.max() == nb - 1
    _, pre = oracle.bin_hidden(bins, P, b1, save_pre=True)
    want, allowed = B.hidden_f64(bins, P, b1)
    assert np.all(np.abs(pre.astype(np.float64) - want) <= allowed)
    # a row of the wrong dimension would show: shifting the bins of dimension A - 1 moves the sum by far more than the bound
    if nb > 1:
        other = bins.copy()
        other[A - 1] = (other[A - 1] + 1) % nb
        moved = np.abs(B.hidden_f64(other, P, b1)[0] - want)
        assert np.median(moved / allowed) > 100.0


# ---- A.4 / A.5  min/max ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("start", B.MINMAX_START)
@pytest.mark.parametrize("N", B.MINMAX_N)
@pytest.mark.parametrize("A", B.MINMAX_A)
def test_oracle_minmax_equals_torch(oracle, A, N, start):
    x = B.minmax_case(A, N)
    lo0, hi0 = B.minmax_start(A, start)
    want = B.minmax_torch(x, lo0, hi0)
    got = oracle.bin_minmax(x, lo0, hi0)
    assert B.same_floats(got[0], want[0], sign_of_zero=False) and B.same_floats(got[1], want[1], sign_of_zero=False)
    flat = x.reshape(-1)
    assert flat[0] == x.max() and flat[-1] == x.min()                                   # the planted extremes are the extremes
    if start == "finite" and N > 1:
        assert np.array_equal(want[0][::3], lo0[::3]) and np.array_equal(want[1][::3], hi0[::3])     # left unchanged
        if A > 1:
            assert not np.array_equal(want[0], lo0)


@pytest.mark.parametrize("N", B.NAN_N)
@pytest.mark.parametrize("A", B.NAN_A)
def test_oracle_minmax_propagates_nan_like_torch(oracle, A, N):
    x, nan_cols, later = B.nan_case(A, N)
    assert np.array_equal(np.flatnonzero(np.isnan(x).any(0)), nan_cols)
    lo, hi = B.minmax_start(A, "inf")
    wlo, whi = B.minmax_torch(x, lo, hi)
    glo, ghi = oracle.bin_minmax(x, lo, hi)
    assert np.array_equal(np.flatnonzero(np.isnan(wlo)), nan_cols) and np.array_equal(np.flatnonzero(np.isnan(whi)), nan_cols)
    assert B.same_floats(glo, wlo, False) and B.same_floats(ghi, whi, False)
    wlo2, whi2 = B.minmax_torch(later, wlo, whi)                                        # NaN statistics stay NaN
    glo2, ghi2 = oracle.bin_minmax(later, glo, ghi)
    assert np.array_equal(np.flatnonzero(np.isnan(wlo2)), nan_cols)
    assert B.same_floats(glo2, wlo2, False) and B.same_floats(ghi2, whi2, False)


def test_the_issue_column():
    lo, hi = B.minmax_torch(np.array([[0.5], [np.nan], [-1.0], [2.0]], np.float32), np.array([np.inf], np.float32),
                            np.array([-np.inf], np.float32))
    assert np.isnan(lo[0]) and np.isnan(hi[0])


# ---- A.6  edge statistics and edge values ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb", B.EDGE_NB)
def test_oracle_equals_torch_on_the_edge_tables(oracle, nb):
    x, bd = B.edge_values(nb)
    lo, hi = B.edge_stats()
    bins, got_bd = oracle.bin_discretize(x, lo, hi, nb, want_boundaries=True)
    assert B.same_floats(got_bd, bd, sign_of_zero=False)
    assert np.array_equal(bins, B.torch_bins(x, bd, nb))
    assert x.shape == (3 * (nb + 1) + len(B.EDGE_SPECIALS), len(B.EDGE_STATS))
    # every neighbour of a finite boundary differs from it; of an infinite one, the inward neighbour does
    n = nb + 1
    b, up, down = x[:n].T, x[n:2 * n].T, x[2 * n:3 * n].T
    assert np.array_equal(b, bd, equal_nan=True)
    fin = np.isfinite(bd)
    assert fin.all(1).sum() >= 5 and np.all(up[fin] > bd[fin]) and np.all(down[fin] < bd[fin])
    assert np.all(down[bd == np.inf] < np.inf) and np.all(up[bd == -np.inf] > -np.inf)
    assert np.isnan(up[np.isnan(bd)]).all()


def test_discretize_limit_is_on_the_edge():
    assert 16 * (255 + 1) == 4096 and 16 * (256 + 1) > 4096


# ---- B  gradient shapes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,A,D,nb", B.GRAD_LARGE)
def test_large_gradient_shapes_have_a_hot_bin_and_no_empty_one(N, A, D, nb):
    x = B.grad_actions(N, A, nb)
    bd = B.torch_boundaries(x.min(0), x.max(0), nb)
    bins = B.torch_bins(x, bd, nb)
    for i in range(A):
        hist = np.bincount(bins[i], minlength=nb)
        assert hist.max() >= 30000 and hist.min() >= 1, (i, hist)


def test_constant_column_falls_in_one_bin():
    N, A, D, nb = B.GRAD_CONSTANT
    x = B.grad_actions(N, A, nb, constant_col=1)
    bins = B.torch_bins(x, B.torch_boundaries(x.min(0), x.max(0), nb), nb)
    assert len(np.unique(bins[1])) == 1 and len(np.unique(bins[0])) > 1


def test_stock_fp32_module_is_close_to_float64_at_the_small_shapes():
    """The ground under E2E for N <= 4097: the stock fp32 module's own distance from float64 (2.0e-6 at most when measured)."""
    worst = 0.0
    for N, A, D, nb in B.GRAD_SMALL + (B.GRAD_CONSTANT,):
        sd = B.module_state(A, D, nb)
        x = B.grad_actions(N, A, nb)
        bins = torch.from_numpy(B.torch_bins(x, B.torch_boundaries(x.min(0), x.max(0), nb), nb).T.copy())
        R = torch.from_numpy(B.grad_upstream(N, D))
        _, g64 = B.stock_module_grads(sd, bins, R, torch.float64)
        _, g32 = B.stock_module_grads(sd, bins, R, torch.float32)
        for k in g64:
            worst = max(worst, float((g32[k].double() - g64[k]).abs().max() / g64[k].abs().max().clamp(min=1e-300)))
    assert worst <= 0.25 * B.E2E, worst


@pytest.mark.parametrize("N", B.SCATTER_N[:1])
@pytest.mark.parametrize("K", B.SCATTER_K)
def test_scatter_case_uses_every_code(N, K):
    g, idx = B.scatter_case(N, K, 16)
    assert np.array_equal(np.unique(idx), np.arange(K)) and np.bincount(idx)[K - 1] >= N // 3
    want = B.scatter_sequential_fp32(g, idx, K)
    ref = torch.zeros(K, 16, dtype=torch.float64).index_add_(0, torch.from_numpy(idx), torch.from_numpy(g).double()).numpy()
    assert np.abs(want - ref).max() <= 2e-6 * np.abs(g).max() * np.sqrt(N)


# ---- C  update kernels -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("state", B.EMA_STATES)
@pytest.mark.parametrize("K,D", B.EMA_SHAPES)
def test_ema_reference_is_finite_where_the_table_says_and_the_oracle_follows_it(oracle, K, D, state):
    s = B.ema_state(K, D, state)
    want = B.ema_f64(s)
    if state in B.EMA_NONFINITE:
        assert np.isnan(want[2]).all() and np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    else:
        assert all(np.isfinite(w).all() for w in want)
    got = oracle.ema_update(s["cs"], s["es"], s["counts"], s["dw"], s["decay"], s["eps"])
    for g, w in zip(got, want):
        assert B.within_or_same_kind(g, w)
    if state == "first_step_third_dead":
        assert (s["counts"] == 0).sum() >= K // 3 and (s["counts"] > 0).any()
    if state == "huge_counts":
        assert s["counts"].min() >= 2 ** 24 and s["counts"].max() == 2 ** 26
    if state == "tiny_clusters":
        assert want[0].max() < 1e-6


@pytest.mark.parametrize("regime", B.ADAMW_REGIMES)
def test_adamw_regimes_keep_the_square_in_fp32_and_float64_finite(regime):
    sizes = [1, 257]
    for scale in (1.0, 1e4):
        ps = [torch.from_numpy(p).double().requires_grad_(True) for p in B.adamw_params(sizes, scale)]
        opt = torch.optim.AdamW(ps, lr=1e-3, weight_decay=1e-2)
        for step in range(B.ADAMW_STEPS):
            for i, p in enumerate(ps):
                g = B.adamw_grad(regime, p.numel(), step, i)
                assert g is None or np.isfinite(g * g).all()
                p.grad = None if g is None else torch.from_numpy(g).double()
            opt.step()
        assert all(torch.isfinite(p).all() for p in ps)
    assert any(B.adamw_grad(regime, 4, s, 3) is None for s in range(B.ADAMW_STEPS))          # step counts differ
    for count in (33, 65):
        sizes = B.adamw_sizes(count)
        assert len(sizes) == count and set(sizes) == set(B.ADAMW_SIZES) and sum(sizes) < 2_000_000


def test_mse_cases():
    xr, x, zq, ze = B.mse_pair_case(1023, 5, big=True)
    assert np.abs(xr - x).max() >= 9e18 and np.isfinite(B.mse_f64(xr, x)) and np.isfinite(B.mse_f64(zq, ze))
    assert B.MSE_N[-2] // 4 > 2048 * 256 and B.MSE_N[-1] // 4 > 3 * 2048 * 256                # the two-float4 loop runs
