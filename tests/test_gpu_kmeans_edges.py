"""GPU: edge instances of the k-means extension (csrc/lipvq_kmeans.hip via ops.kmeans_seed / kmeans_revive_ / kmeans_means_)
against the numpy restatement of its sampling rule (tests/kmeans_ref.py) on the CPU oracle, bit for bit, as
test_gpu_kmeans.py::test_seed_is_exact does: picks, written, the codebook's bits, untouched codes equal to their initial contents.
Covered here and not there: the D = 128 register instance and the run-time-width instance taken when z is not 16-byte aligned,
N at 256-row block edges, more than 1024 pass blocks (the pick's per-thread chunk > 1), draws at 0 and at the last double below 1
across zero-weight rows and whole zero-weight blocks, draws next to a row's boundary, scale exponents far from 0, subnormal
comparison values, non-finite rows, the dead-code list scan with K > 1024, idx outside [0, K), threshold / max_codes extremes,
and the Lloyd division.  tests/test_kmeans_host.py checks on the CPU what these inputs are meant to reach."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import kmeans_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NORM, SQSUM = R.DIST_NORM, R.DIST_SQSUM
BOTH = pytest.mark.parametrize("dist", [NORM, SQSUM], ids=["norm", "sqsum"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _init(K, D, seed=7):
    return np.random.default_rng(seed).uniform(-1, 1, (K, D)).astype(np.float32)


def check_seed(oracle, z, K, u, dist, zt=None):
    """ops.kmeans_seed against R.seed; returns the reference (codebook, picks, written)."""
    from lipvq_vae_amd import ops
    init = _init(K, z.shape[1])
    cb, picks, written = ops.kmeans_seed(dev(z) if zt is None else zt, K, dev(np.asarray(u, np.float64)), dist, out=dev(init))
    ref_cb, ref_picks, ref_written = R.seed(oracle, z, K, u, dist, init=init)
    assert picks.cpu().numpy().tolist() == ref_picks.tolist()
    assert int(written.item()) == ref_written
    assert np.array_equal(_bits(cb.cpu().numpy()), _bits(ref_cb))
    assert np.array_equal(_bits(ref_cb[ref_picks < 0]), _bits(init[ref_picks < 0]))     # untouched codes
    return ref_cb, ref_picks, ref_written


def check_revive(oracle, z, cb0, idx, counts, threshold, u, dist, max_codes=None):
    from lipvq_vae_amd import ops
    cb = dev(cb0)
    picks, written = ops.kmeans_revive_(cb, dev(z), dev(np.asarray(idx, np.int64)), dev(np.asarray(counts, np.int64)), threshold,
                                        dev(np.asarray(u, np.float64)), dist, max_codes=max_codes)
    ref_cb, ref_picks, ref_written = R.revive(oracle, z, cb0, idx, counts, threshold, u, dist, max_codes=max_codes)
    assert picks.cpu().numpy().tolist() == ref_picks.tolist()
    assert int(written.item()) == ref_written
    assert np.array_equal(_bits(cb.cpu().numpy()), _bits(ref_cb))
    assert np.array_equal(_bits(ref_cb[ref_picks < 0]), _bits(np.asarray(cb0, np.float32)[ref_picks < 0]))
    return ref_cb, ref_picks, ref_written


def _rows(seed, N, D):
    return np.random.default_rng(seed).standard_normal((N, D)).astype(np.float32)


# ---- instances ----------------------------------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("D", [32, 128])
def test_register_instances(oracle, D, dist):
    """D = 32 and D = 128: rows read into registers as float4s; seeding (KM_INIT_ROW / KM_UPDATE) and revival (KM_INIT_CODE)."""
    N, K = 1000, 12
    z = _rows(D, N, D)
    u = np.random.default_rng(D + 1).random(K)
    _, picks, written = check_seed(oracle, z, K, u, dist)
    assert written == K
    cb0 = _init(K, D, seed=3)
    idx = oracle.nearest(z, cb0, dist)[0]
    counts = np.bincount(idx, minlength=K)
    threshold = int(np.sort(counts)[K // 2]) + 1
    _, _, written = check_revive(oracle, z, cb0, idx, counts, threshold, u, dist)
    assert written >= K // 2


@BOTH
def test_unaligned_rows_take_the_run_time_width_instance(oracle, dist):
    """z a contiguous view one float into its buffer: not 16-byte aligned, so the D = 64 register instance (float4 loads) must
    not be taken.  Bit-equal to the aligned call and to the restatement."""
    from lipvq_vae_amd import ops
    N, K, D = 1000, 12, 64
    z = _rows(64, N, D)
    buf = torch.empty(N * D + 1, device="cuda")
    zt = buf[1:].view(N, D)
    zt.copy_(dev(z))
    assert zt.is_contiguous() and zt.data_ptr() % 16 == 4 and dev(z).data_ptr() % 16 == 0
    u = np.random.default_rng(5).random(K)
    ref_cb, ref_picks, _ = check_seed(oracle, z, K, u, dist, zt=zt)
    cb, picks, _ = ops.kmeans_seed(dev(z), K, dev(u), dist)
    assert picks.cpu().numpy().tolist() == ref_picks.tolist() and np.array_equal(_bits(cb.cpu().numpy()), _bits(ref_cb))
    cb0 = _init(K, D, seed=3)
    idx = oracle.nearest(z, cb0, dist)[0]
    counts = np.bincount(idx, minlength=K)
    cbt = dev(cb0)
    picks, written = ops.kmeans_revive_(cbt, zt, dev(idx), dev(counts), int(counts.max()), dev(u), dist)
    ref_cb, ref_picks, ref_written = R.revive(oracle, z, cb0, idx, counts, int(counts.max()), u, dist)
    assert picks.cpu().numpy().tolist() == ref_picks.tolist()
    assert int(written.item()) == ref_written == (counts < counts.max()).sum()
    assert np.array_equal(_bits(cbt.cpu().numpy()), _bits(ref_cb))


# ---- N edges ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 512, 513])
def test_n_at_block_edges(oracle, N):
    """One pass block is 256 rows; lanes past N repeat row N - 1 and must weigh nothing.  The draws reach the last row."""
    K, D = 4, 8
    z = _rows(N, N, D)
    for dist in (NORM, SQSUM):
        for u in ([R.LAST, R.LAST, 0.0, 0.5], [0.0, R.LAST, R.LAST, 0.0], [0.5, 0.999, 0.001, R.LAST]):
            _, picks, written = check_seed(oracle, z, K, u, dist)
            assert written == min(N, K)
        assert check_seed(oracle, z, 1, [R.LAST], dist)[1].tolist() == [N - 1]                 # K = 1: no pass at all
        assert check_seed(oracle, z, 1, [0.0], dist)[1].tolist() == [0]
    assert check_seed(oracle, z, K, [0.0, R.LAST, 0.5, 0.5], NORM)[1][1] in (N - 1, -1)


@BOTH
@pytest.mark.parametrize("N", [1024 * 256 + 300, 2 * 1024 * 256 + 1])
def test_more_than_1024_pass_blocks(oracle, N, dist):
    """nb = 1026 and 2049: every pick thread sums a chunk of 2 and 3 block partials.  The first 300 and the last 700 rows are
    copies of row 0 = code 0: draw 0 must pass a whole zero-weight block and 44 rows, the last double below 1 must stop before
    the zero-weight tail (its last two blocks and more)."""
    D, K = 4, 6
    z = _rows(N % 1000, N, D)
    z[:300] = z[0]
    z[N - 700:] = z[0]
    u = [0.0, 0.0, R.LAST, 0.5, 0.25, 0.75]
    _, picks, written = check_seed(oracle, z, K, u, dist)
    assert written == K and picks[0] == 0 and picks[1] == 300 and picks[2] == N - 701


# ---- zero-weight runs and row boundaries ----------------------------------------------------------------------------------------

@BOTH
def test_boundary_draws_over_zero_weight_blocks(oracle, dist):
    """N = 1500, rows 256..767 copies of code 0's row: blocks 1 and 2 weigh nothing.  The two doubles next to each boundary row's
    end pick that row or the next one that weighs something (test_kmeans_host.py: both occur), row 255's the row 768."""
    z, r0 = R.zero_run_rows()
    N = len(z)
    u0 = (r0 + 0.5) / N
    _, d, e = R.first_state(oracle, z, [u0], dist)
    q = R.qweights(d, dist, e)
    zt = dev(z)
    seen = set()
    for n in R.ZERO_RUN_BOUNDARIES:
        for u in R.boundary_draws(q, n):
            _, picks, written = check_seed(oracle, z, 2, [u0, u], dist, zt=zt)
            assert written == 2 and picks[0] == r0
            seen.add((n, int(picks[1])))
    assert (255, 768) in seen and (255, 255) in seen
    for u in (0.0, R.LAST):
        _, picks, _ = check_seed(oracle, z, 2, [u0, u], dist, zt=zt)
        assert picks[1] == (0 if u == 0.0 else N - 1)
    u = np.concatenate([[u0], R.boundary_draws(q, 255), R.boundary_draws(q, 1023), [0.0, R.LAST, 0.5]])
    assert check_seed(oracle, z, len(u), u, dist, zt=zt)[2] == len(u)


# ---- magnitudes and non-finite rows ---------------------------------------------------------------------------------------------

def _revive_inputs(oracle, z, dist, K=6):
    cb0 = z[:: len(z) // K][:K].copy()
    finite = np.isfinite(z).all(axis=1) & (np.abs(z).max(axis=1) < 1e19)
    idx = np.zeros(len(z), np.int64)
    idx[finite] = oracle.nearest(z[finite], cb0, dist)[0]
    counts = np.bincount(idx, minlength=K)
    return cb0, idx, counts, int(np.sort(counts)[K // 2]) + 1


@BOTH
@pytest.mark.parametrize("s", [1e-22, 1e-30, 1e15, 1e18])
def test_magnitudes(oracle, s, dist):
    """randn * s.  1e-22: subnormal squared distances (lipvq_math.h: denormals kept, the root correctly rounded), e = 193;
    1e-30: every distance 0, only code 0 is written; 1e15, 1e18: e = -53, -73."""
    z = R.scaled_rows(s)
    _, _, e = R.first_state(oracle, z, R.EDGE_DRAWS, dist)
    assert e == {1e-22: 193, 1e-30: 0, 1e15: -53, 1e18: -73}[s]
    _, picks, written = check_seed(oracle, z, 6, R.EDGE_DRAWS, dist)
    assert written == (1 if s == 1e-30 else 6)
    cb0, idx, counts, threshold = _revive_inputs(oracle, z, dist)
    _, _, written = check_revive(oracle, z, cb0, idx, counts, threshold, R.EDGE_DRAWS, dist)
    assert written == (0 if s == 1e-30 else (counts < threshold).sum())


@BOTH
def test_non_finite_rows_weigh_nothing(oracle, dist):
    z, bad = R.nonfinite_rows()
    u = np.concatenate([R.EDGE_DRAWS, np.random.default_rng(3).random(58)])
    _, picks, written = check_seed(oracle, z, 64, u, dist)
    assert written == 64 and not set(picks.tolist()) & set(bad) and picks[3] == len(z) - 2
    cb0, idx, counts, threshold = _revive_inputs(oracle, z, dist)
    _, picks, written = check_revive(oracle, z, cb0, idx, counts, threshold, R.EDGE_DRAWS, dist)
    assert written > 0 and not set(picks.tolist()) & set(bad)
    z[0, 5] = np.nan                                            # code 0 is the NaN row: no row weighs anything
    _, picks, written = check_seed(oracle, z, 6, R.EDGE_DRAWS, dist)
    assert written == 1 and picks.tolist() == [0, -1, -1, -1, -1, -1]


# ---- revival ------------------------------------------------------------------------------------------------------------------

def _dead_codes(K, rng):
    """About 40 dead codes: 0, K - 1, both sides of the list scan's per-thread chunk edges and of its 64-thread wave edges."""
    chunk = -(-K // 1024)
    dead = {0, K - 1, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 64 * chunk - 1, 64 * chunk, 500 * chunk - 1,
            500 * chunk, 500 * chunk + 1, (K - 1) // chunk * chunk - 1, (K - 1) // chunk * chunk, K - 2}
    dead |= {int(k) for k in rng.integers(0, K, 26)}
    return chunk, np.array(sorted(k for k in dead if 0 <= k < K))


@BOTH
@pytest.mark.parametrize("K", [1025, 2500])
def test_revival_with_a_long_dead_code_list(oracle, K, dist):
    """K > 1024: every thread of the start kernel scans a chunk of 2 or 3 codes.  counts == threshold is alive; rows whose idx
    is -1 or K weigh nothing; max_codes cuts the list."""
    N, D = 3000, 8
    rng = np.random.default_rng(K)
    z = _rows(K, N, D)
    cb0 = _rows(K + 1, K, D)
    idx = rng.integers(0, K, N)
    idx[::7] = -1
    idx[3::11] = K
    chunk, dead = _dead_codes(K, rng)
    assert chunk == (2 if K == 1025 else 3) and 35 <= len(dead) <= 41
    counts = rng.integers(3, 50, K)                              # threshold 3: a count of 3 is alive
    counts[dead] = rng.integers(0, 3, len(dead))
    assert (counts == 3).any() and (counts == 2).any()
    u = rng.random(K)
    u[dead[0]], u[dead[1]], u[dead[-1]] = 0.0, R.LAST, R.LAST
    _, picks, written = check_revive(oracle, z, cb0, idx, counts, 3, u, dist)
    assert written == len(dead) and np.array_equal(np.nonzero(picks >= 0)[0], dead)
    outside = set(np.nonzero((idx < 0) | (idx >= K))[0].tolist())
    assert picks[dead[0]] not in outside                         # draw 0: rows 0 (idx -1) and 3 (idx K) weigh nothing
    _, picks, written = check_revive(oracle, z, cb0, idx, counts, 3, u, dist, max_codes=5)
    assert written == 5 and np.array_equal(np.nonzero(picks >= 0)[0], dead[:5])
    _, picks, written = check_revive(oracle, z, cb0, idx, counts, 3, u, dist, max_codes=0)
    assert written == 0 and (picks == -1).all()
    _, picks, written = check_revive(oracle, z, cb0, idx, counts, 0, u, dist)       # no count is below 0: no dead code
    assert written == 0 and (picks == -1).all()


@BOTH
def test_revival_extremes(oracle, dist):
    """K = 8: every code dead (threshold above every count); none dead; every row's idx outside the codebook (nothing weighs,
    nothing is written)."""
    N, K, D = 700, 8, 8
    rng = np.random.default_rng(12)
    z, cb0 = _rows(1, N, D), _rows(2, K, D)
    idx = rng.integers(0, K, N)
    counts = np.bincount(idx, minlength=K)
    u = np.array([0.0, R.LAST, 0.5, 0.25, 0.75, 0.1, R.LAST, 0.0])
    _, picks, written = check_revive(oracle, z, cb0, idx, counts, int(counts.max()) + 1, u, dist)
    assert written == K and (picks >= 0).all()
    assert check_revive(oracle, z, cb0, idx, counts, 2 ** 62, u, dist, max_codes=3)[2] == 3
    assert check_revive(oracle, z, cb0, idx, counts, int(counts.min()), u, dist)[2] == 0
    assert check_revive(oracle, z, cb0, idx, counts, -5, u, dist)[2] == 0
    idx_out = np.where(np.arange(N) % 2 == 0, -1, K)
    assert check_revive(oracle, z, cb0, idx_out, counts, int(counts.max()) + 1, u, dist)[2] == 0
    idx_one = idx_out.copy()
    idx_one[N - 1] = 3                                           # one row weighs: it is drawn whatever the draw, then Q = 0
    _, picks, written = check_revive(oracle, z, cb0, idx_one, counts, int(counts.max()) + 1, u, dist)
    assert written == 1 and picks[0] == N - 1


# ---- the Lloyd division ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,D,counts", [(3, 1, [0, 1, 2 ** 24 + 1]), (5, 51, [2 ** 24 + 1, 0, 1, 7, 0]), (1, 257, [2 ** 24 + 1]),
                                        (1, 257, [0]), (1, 257, [1])])
def test_means(K, D, counts):
    """codebook[k] = sums[k] / (float)counts[k]: counts 0 keeps the code's bytes (NaN payloads included), 2^24 + 1 rounds to
    2^24 as numpy's float32 does; sums hold inf and -0.0; K * D is no multiple of the 256-thread block."""
    from lipvq_vae_amd import ops
    rng = np.random.default_rng(K * D)
    sums = (rng.standard_normal((K, D)) * 10.0 ** rng.uniform(-3, 8, (K, D))).astype(np.float32)
    sums[:, 0] = -0.0
    sums[K - 1, D - 1] = np.inf
    sums[0, D // 2] = -np.inf if D > 1 else -0.0
    cb0 = rng.standard_normal((K, D)).astype(np.float32)
    cb0.view(np.uint32)[:, 0] = 0x7FC12345                        # a NaN with a payload
    cb0.view(np.uint32)[:, D - 1] = 0xFFA00001
    counts = np.array(counts, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where((counts > 0)[:, None], sums / counts.astype(np.float32)[:, None], cb0)
    want = want.astype(np.float32)
    want.view(np.uint32)[counts <= 0] = cb0.view(np.uint32)[counts <= 0]
    assert np.float32(2 ** 24 + 1) == np.float32(2 ** 24)
    cb = dev(cb0)
    assert np.array_equal(cb.cpu().numpy().view(np.uint32), cb0.view(np.uint32))          # the copy keeps the payloads
    ops.kmeans_means_(cb, dev(sums), dev(counts))
    got = cb.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    zero = (counts > 0) & (sums[:, 0] == 0)                       # -0.0 / c = -0.0
    assert (got[zero, 0].view(np.uint32) == 0x80000000).all()
