"""CPU: argument validation of the k-means extension (lipvq_kmeans_* through _capi, the ops wrappers) and edge cases of the
numpy restatement of its sampling rule (tests/kmeans_ref.py).  No compute call reaches a GPU."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import kmeans_ref as R  # noqa: E402


class _FakeOracle:
    """distances() in fp32 with the plain formulas: enough for the edge cases below (exactly representable values)."""

    def distances(self, z, c, dist):
        diff = z[:, None, :].astype(np.float32) - c[None, :, :].astype(np.float32)
        s = (diff * diff).sum(-1, dtype=np.float32)
        return np.sqrt(s) if dist == R.DIST_NORM else s


def test_abi_validates_sizes_and_pointers():
    from lipvq_vae_amd import _capi
    lib = _capi.lib
    fake = ctypes.c_void_p(16)                                  # never dereferenced: every call below fails its checks first
    assert lib.lipvq_kmeans_workspace_bytes(0, 4) == 0
    assert lib.lipvq_kmeans_workspace_bytes(10, 0) == 0
    # header, dead-code list, d [N], one uint64 partial per 256 rows
    assert lib.lipvq_kmeans_workspace_bytes(1000, 300) == 256 + 1280 + 4096 + 4 * 8
    assert lib.lipvq_kmeans_seed_f32(fake, fake, fake, fake, fake, fake, 0, 4, 8, 0, None) < 0      # N < 1
    assert lib.lipvq_kmeans_seed_f32(fake, fake, fake, fake, fake, fake, 10, 0, 8, 0, None) < 0     # K < 1
    assert lib.lipvq_kmeans_seed_f32(fake, fake, fake, fake, fake, fake, 10, 4, 8, 7, None) < 0     # unknown rule
    assert lib.lipvq_kmeans_seed_f32(None, fake, fake, fake, fake, fake, 10, 4, 8, 0, None) < 0     # null z
    assert b"kmeans_seed" in lib.lipvq_last_error()
    assert lib.lipvq_kmeans_revive_f32(fake, fake, None, fake, 1, fake, fake, fake, fake, 10, 4, 8, 0, 4, None) < 0
    assert lib.lipvq_kmeans_revive_f32(fake, fake, fake, fake, 1, fake, fake, fake, fake, 10, 4, 8, 0, -1, None) < 0
    assert lib.lipvq_kmeans_means_f32(fake, fake, fake, 0, 8, None) < 0
    assert lib.lipvq_kmeans_means_f32(None, fake, fake, 4, 8, None) < 0
    with pytest.raises(RuntimeError, match="kmeans_means"):
        _capi.check(lib.lipvq_kmeans_means_f32(fake, fake, fake, 4, 0, None), "lipvq_kmeans_means_f32")


def test_ops_reject_cpu_tensors():
    from lipvq_vae_amd import ops
    z = torch.zeros(10, 4)
    draws = torch.zeros(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.kmeans_seed(z, 3, draws)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.kmeans_revive_(torch.zeros(3, 4), z, torch.zeros(10, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), 1, draws)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.kmeans_means_(torch.zeros(3, 4), torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64))


def test_scale_exponent_is_the_largest_that_fits():
    for wmax, N in ((1.0, 1), (1.0, 1000), (0.75, 524288), (3.0e-90, 7), (1.2e77, 2 ** 40), (2.0 ** 62, 1)):
        e = R.scale_exponent(wmax, N)
        assert N * np.ldexp(wmax, e) <= R.LIM < N * np.ldexp(wmax, e + 1)
    assert R.scale_exponent(0.0, 100) == 0


def test_draw_rule():
    q = np.array([0, 3, 0, 5, 2], np.uint64)                     # Q = 10: r 0..2 -> row 1, 3..7 -> row 3, 8..9 -> row 4
    assert R.draw(q, 0.0) == 1
    assert R.draw(q, 0.2999) == 1
    assert R.draw(q, 0.3) == 3
    assert R.draw(q, 0.7999) == 3
    assert R.draw(q, 0.8) == 4
    assert R.draw(q, np.nextafter(1.0, 0.0)) == 4               # r = min(Q - 1, floor(u Q))
    assert R.draw(np.zeros(4, np.uint64), 0.5) is None           # Q == 0: nothing left to draw


def test_seed_stops_when_no_distinct_row_is_left():
    z = np.array([[1, 2], [1, 2], [3, 4], [1, 2]], np.float32)  # two distinct rows
    init = np.full((5, 2), 7.0, np.float32)
    for dist in (R.DIST_NORM, R.DIST_SQSUM):
        cb, picks, written = R.seed(_FakeOracle(), z, 5, np.array([0.0, 0.5, 0.5, 0.5, 0.5]), dist, init=init)
        assert written == 2
        assert picks.tolist() == [0, 2, -1, -1, -1]
        assert np.array_equal(cb[:2], z[[0, 2]]) and np.all(cb[2:] == 7.0)


def test_seed_with_one_row():
    z = np.array([[0.5, -1.0, 2.0]], np.float32)
    cb, picks, written = R.seed(_FakeOracle(), z, 3, np.array([0.99, 0.1, 0.1]), R.DIST_NORM)
    assert written == 1 and picks.tolist() == [0, -1, -1]
    assert np.array_equal(cb[0], z[0]) and not cb[1:].any()


def test_revive_refills_dead_codes_in_order():
    z = np.array([[0, 0], [0, 0], [10, 0], [0, 3]], np.float32)
    cb = np.array([[0, 0], [5, 5], [6, 6]], np.float32)
    idx = np.array([0, 0, 0, 0])
    counts = np.array([4, 0, 0])
    # d = 0, 0, 10, 3 under the norm rule: weights 0, 0, 100, 9
    out, picks, written = R.revive(_FakeOracle(), z, cb, idx, counts, 1, np.array([0.0, 0.5, 0.0]), R.DIST_NORM)
    assert written == 2 and picks.tolist() == [-1, 2, 3]
    assert np.array_equal(out, np.array([[0, 0], [10, 0], [0, 3]], np.float32))
    _, picks1, _ = R.revive(_FakeOracle(), z, cb, idx, counts, 1, np.array([0.0, 0.5, 0.0]), R.DIST_NORM, max_codes=1)
    assert picks1.tolist() == [-1, 2, -1]
    _, picks0, written0 = R.revive(_FakeOracle(), z, cb, idx, np.array([4, 1, 1]), 1, np.zeros(3), R.DIST_NORM)
    assert written0 == 0 and (picks0 == -1).all()


# ---- edge inputs of tests/test_gpu_kmeans_edges.py, on the real oracle ----------------------------------------------------------

TINY = float(np.finfo(np.float32).tiny)


def _fits(wmax, N, e):
    return N * np.ldexp(wmax, e) <= R.LIM < N * np.ldexp(wmax, e + 1)


def test_revive_gives_rows_with_an_index_outside_the_codebook_no_weight():
    z = np.array([[0, 0], [9, 0], [10, 0], [0, 3], [0, 50]], np.float32)
    cb = np.array([[0, 0], [5, 5], [6, 6]], np.float32)
    counts = np.array([5, 0, 0])
    # rows 1 and 4 are the farthest from code 0, and their idx is -1 and K: they weigh 0 -> d = 0, 0, 10, 3, 0
    out, picks, written = R.revive(_FakeOracle(), z, cb, np.array([0, -1, 0, 0, 3]), counts, 1, np.array([0.0, 0.0, R.LAST]),
                                   R.DIST_NORM)
    assert written == 2 and picks.tolist() == [-1, 2, 3]
    _, picks_in, _ = R.revive(_FakeOracle(), z, cb, np.zeros(5, np.int64), counts, 1, np.array([0.0, 0.0, R.LAST]), R.DIST_NORM)
    assert picks_in.tolist() == [-1, 1, 4]                       # with every idx inside, those two rows are the ones drawn


def test_subnormal_comparison_values_under_the_sum_rule(oracle):
    z = R.scaled_rows(1e-22)
    _, d, e = R.first_state(oracle, z, R.EDGE_DRAWS, R.DIST_SQSUM)
    assert (d > 0).sum() == len(d) - 1 and (d[d > 0] < TINY).all()              # every non-zero d is subnormal
    assert e == 193 and e > 0 and _fits(R.weights(d, R.DIST_SQSUM).max(), len(d), e)
    _, picks, written = R.seed(oracle, z, 6, R.EDGE_DRAWS, R.DIST_SQSUM)
    assert written == 6 and len(set(picks.tolist())) == 6


def test_subnormal_squares_with_normal_roots_under_the_norm_rule(oracle):
    z = R.scaled_rows(1e-22)
    sq = R.first_state(oracle, z, R.EDGE_DRAWS, R.DIST_SQSUM)[1]
    _, d, e = R.first_state(oracle, z, R.EDGE_DRAWS, R.DIST_NORM)
    assert (sq[sq > 0] < TINY).all() and (d[d > 0] >= TINY).all() and (d > 0).sum() == len(d) - 1
    assert e > 0 and _fits(R.weights(d, R.DIST_NORM).max(), len(d), e)
    assert R.seed(oracle, z, 6, R.EDGE_DRAWS, R.DIST_NORM)[2] == 6


@pytest.mark.parametrize("dist", [R.DIST_NORM, R.DIST_SQSUM])
def test_rows_that_differ_below_fp32_resolution_stop_the_seeding(oracle, dist):
    z = R.scaled_rows(1e-30)
    assert len({r.tobytes() for r in z}) > 500                   # distinct rows, all at distance 0 from one another
    _, d, e = R.first_state(oracle, z, R.EDGE_DRAWS, dist)
    assert not d.any() and e == 0
    _, picks, written = R.seed(oracle, z, 6, R.EDGE_DRAWS, dist)
    assert written == 1 and picks.tolist() == [0, -1, -1, -1, -1, -1]


@pytest.mark.parametrize("s,want", [(1e15, -53), (1e18, -73)])
@pytest.mark.parametrize("dist", [R.DIST_NORM, R.DIST_SQSUM])
def test_large_rows_give_a_negative_scale_exponent(oracle, dist, s, want):
    z = R.scaled_rows(s)
    _, d, e = R.first_state(oracle, z, R.EDGE_DRAWS, dist)
    assert np.isfinite(d).all()
    assert e == want and e < 0 and _fits(R.weights(d, dist).max(), len(d), e)
    assert R.seed(oracle, z, 6, R.EDGE_DRAWS, dist)[2] == 6


@pytest.mark.parametrize("dist", [R.DIST_NORM, R.DIST_SQSUM])
def test_non_finite_rows(oracle, dist):
    z, bad = R.nonfinite_rows()
    _, d, _ = R.first_state(oracle, z, R.EDGE_DRAWS, dist)
    assert not np.isfinite(d[list(bad)]).any() and np.isfinite(np.delete(d, bad)).all()
    assert not R.weights(d, dist)[list(bad)].any()
    u = np.concatenate([R.EDGE_DRAWS, np.random.default_rng(3).random(58)])
    cb, picks, written = R.seed(oracle, z, 64, u, dist)
    assert written == 64 and not set(picks.tolist()) & set(bad) and np.isfinite(cb).all()
    # LAST stops at the last row that weighs something: 598, not the 3e19 row 599
    assert picks[3] == len(z) - 2
    z[0, 5] = np.nan                                             # code 0 is row 0: every distance is NaN, nothing weighs
    cb, picks, written = R.seed(oracle, z, 6, R.EDGE_DRAWS, dist)
    assert written == 1 and picks.tolist() == [0, -1, -1, -1, -1, -1] and not cb[1:].any()


@pytest.mark.parametrize("dist", [R.DIST_NORM, R.DIST_SQSUM])
def test_boundary_draws_stop_at_the_row_or_the_next_one_that_weighs(oracle, dist):
    """u = c[n] / Q is where row n ends.  Its two neighbouring doubles stop at n and at the next row with q > 0 -- over two
    zero-weight blocks for n = 255 -- or, as floor(u Q) is rounded in fp64 (Q is near 2^62), both on the same side; both
    outcomes occur, so an off-by-one in the block or row search picks another row somewhere in the set."""
    z, r0 = R.zero_run_rows()
    N = len(z)
    _, d, e = R.first_state(oracle, z, [(r0 + 0.5) / N], dist)
    q = R.qweights(d, dist, e)
    assert not q[256:768].any() and not q[r0] and np.count_nonzero(q) == N - 513
    below, above = [], []
    for n in R.ZERO_RUN_BOUNDARIES:
        nxt = n + 1 + int(np.nonzero(q[n + 1:])[0][0])
        lo, hi = R.boundary_draws(q, n)
        assert 0.0 <= lo < hi < 1.0
        a, b = R.draw(q, lo), R.draw(q, hi)
        assert a in (n, nxt) and b in (n, nxt) and a <= b
        below.append(a == n)
        above.append(b == nxt)
    assert R.draw(q, R.boundary_draws(q, 255)[1]) == 768
    assert sum(below) >= 5 and sum(above) >= 5
    assert not all(below) or not all(above)                      # the rounded product lands on either side
    assert R.draw(q, 0.0) == 0 and R.draw(q, R.LAST) == N - 1
