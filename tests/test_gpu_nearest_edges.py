"""GPU: exact nearest-code search (lipvq_nearest_f32, csrc/lipvq_nearest.hip) at the edges of its three kernels -- the direct
kernel (D in {32, 64, 128, 208}: rows in registers, the codebook through LDS in tiles of KT = 8192 / D codes), the LDS-staged
wide kernel (D = 209 ... 512, groups of 64 codes, zero pad codes) and the generic kernel (any other D, or misaligned operands).

idx, zq, best and usage are compared with the canonical oracle with ==; then lipvq_nearest_rows_f32 (route "rows") and, where
lipvq_nearest_small_supported, lipvq_nearest_small_f32 (route "small") must return the same idx / zq / usage on the same inputs.
usage starts at 2^33 + k everywhere: it is ACCUMULATED, in 64 bits, and grows by exactly N.
"""
import numpy as np
import pytest
import torch

import seed_kernel_edges as E
from oracle import lipvq_oracle as O

pytestmark = pytest.mark.gpu

DISTS = [O.DIST_NORM, O.DIST_SQSUM]
SENTINEL = -7777.25


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _prefill(K):
    return (2 ** 33 + np.arange(K)).astype(np.int64)


def _check(ops, oracle, z, cb, dist, what, routes=True):
    """lipvq_nearest_f32 against the oracle (idx, zq, best, usage), then the rows / small routes against the same answers.
    Returns the oracle's (idx, best)."""
    N, D = z.shape
    K = cb.shape[0]
    idx_ref, zq_ref, usage_ref, best_ref = oracle.nearest(z, cb, dist, want_best=True)
    assert usage_ref.sum() == N and np.array_equal(usage_ref, np.bincount(idx_ref, minlength=K))
    zd, cbd = dev(z), dev(cb)
    usage = dev(_prefill(K))
    idx, zq, best = ops.nearest(zd, cbd, dist, usage=usage, want_best=True)
    torch.cuda.synchronize()
    idx, zq, best, usage = idx.cpu().numpy(), zq.cpu().numpy(), best.cpu().numpy(), usage.cpu().numpy()
    bad = np.flatnonzero(idx != idx_ref)
    assert bad.size == 0, f"{what}: idx differs at rows {bad[:5].tolist()}: got {idx[bad[:5]].tolist()}, oracle {idx_ref[bad[:5]].tolist()}"
    assert np.array_equal(zq, zq_ref, equal_nan=bool(np.isnan(cb).any())), f"{what}: zq"
    assert np.array_equal(best, best_ref), f"{what}: best {best[:4]} oracle {best_ref[:4]}"
    assert int((usage - _prefill(K)).sum()) == N, f"{what}: usage grew by {int((usage - _prefill(K)).sum())}, not N = {N}"
    assert np.array_equal(usage - _prefill(K), usage_ref), f"{what}: usage"
    if routes:
        names = ["rows"] + (["small"] if ops.lib.lipvq_nearest_small_supported(N, K, D) else [])
        for route in names:
            u = dev(_prefill(K))
            i2, q2 = ops.nearest_rows(zd, cbd, usage=u, dist=dist, route=route)
            torch.cuda.synchronize()
            assert np.array_equal(i2.cpu().numpy(), idx_ref), f"{what}: route {route} idx"
            assert np.array_equal(q2.cpu().numpy(), zq_ref, equal_nan=bool(np.isnan(cb).any())), f"{what}: route {route} zq"
            assert np.array_equal(u.cpu().numpy() - _prefill(K), usage_ref), f"{what}: route {route} usage"
    return idx_ref, best_ref


# ---------------------------------------------------------------------------------------------------------------------------
# the direct kernel's codebook tile seam
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("kk", ["KT-1", "KT", "KT+1", "2KT+1"])
@pytest.mark.parametrize("D", [32, 64, 128, 208])
def test_direct_kernel_tile_seam(ops, oracle, D, kk, dist):
    """K around the LDS tile of KT = 8192 / D codes (one ragged tile, one whole tile, a one-code second tile, a one-code third
    tile); exact duplicate codes at (KT - 1, KT) -- the last code of one tile and the first of the next -- and at (0, K - 1),
    rows sitting exactly on them: the lower index wins (the scan's `v < best` must stay strict across the tile reload).  A row on
    the last code, alone in the ragged tile, has distance 0."""
    KT = 8192 // D
    K = {"KT-1": KT - 1, "KT": KT, "KT+1": KT + 1, "2KT+1": 2 * KT + 1}[kk]
    N = 70
    rng = np.random.default_rng(D * 7 + K)
    base = rng.uniform(0, 1, (K, D)).astype(np.float32)
    near = (base[rng.integers(0, K, N)] + 0.01 * rng.standard_normal((N, D))).astype(np.float32)
    for variant in ("seam", "ends"):
        cb, z = base.copy(), near.copy()
        if variant == "seam":
            if K > KT:
                cb[KT] = cb[KT - 1]
                z[0] = z[33] = z[N - 1] = cb[KT - 1]
            z[1] = cb[K - 1]                                  # the last code: in a ragged tile of its own for K = KT + 1, 2 KT + 1
            if K > 2 * KT:
                cb[2 * KT - 1] = cb[KT + 5]                   # a duplicate that ends the second tile
                z[2] = cb[KT + 5]
        else:
            cb[K - 1] = cb[0]
            z[0] = z[33] = z[N - 1] = cb[0]
            z[1] = cb[K - 2]
        idx, best = _check(ops, oracle, z, cb, dist, f"D={D} K={K} {variant}")
        if variant == "seam" and K > KT:
            assert idx[0] == idx[33] == idx[N - 1] == KT - 1 and best[0] == 0.0
        if variant == "seam":
            assert idx[1] == (KT - 1 if K == KT + 1 else K - 1) and best[1] == 0.0
        if variant == "ends":
            assert idx[0] == idx[33] == idx[N - 1] == 0 and idx[1] == K - 2 and best[0] == best[1] == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# the last block's clamped lanes and the wave-combined usage counts
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_wave", [1, 4, 5, 64])
@pytest.mark.parametrize("N", [1, 63, 65, 255, 256, 257])
def test_block_tail_and_usage(ops, oracle, N, per_wave):
    """Lanes past N re-read row N - 1 and must not count.  lq_usage_add combines a wave's equal codes in up to four leader
    rounds and finishes with single adds: waves holding one code, exactly four (all leader rounds, nothing left), exactly five
    (one code left for the single adds) and 64 distinct codes.  D = 32: direct kernel (256-row blocks), D = 7: generic kernel
    (64-row blocks), D = 256: the wide kernel's own per-row add."""
    K = 192
    for D in (32, 7, 256):
        rng = np.random.default_rng(N * 5 + per_wave + D)
        cb = rng.uniform(0, 1, (K, D)).astype(np.float32) + np.arange(K, dtype=np.float32)[:, None]     # far apart in every width
        n = np.arange(N)
        codes = ((n // 64) * per_wave + (n % per_wave)) % K          # wave w of 64 rows: codes w m ... w m + m - 1
        z = (cb[codes] + 0.001 * rng.standard_normal((N, D))).astype(np.float32)
        for dist in DISTS:
            idx, _ = _check(ops, oracle, z, cb, dist, f"N={N} D={D} {per_wave} codes per wave")
            assert np.array_equal(idx, codes)
            for w in range((N + 63) // 64):
                assert len(set(idx[64 * w:64 * w + 64])) == min(per_wave, N - 64 * w)


# ---------------------------------------------------------------------------------------------------------------------------
# two squares, one root
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 208, 256, 7])
def test_root_ties(ops, oracle, D):
    """Two codes whose squared distances differ by an fp32 ulp while their square roots are equal, the larger square at the lower
    index: torch.norm + argmin (DIST_NORM) compares the ROOTS and keeps the lower index, pow(2).sum + argmin (DIST_SQSUM)
    compares the squares and takes the higher.  Direct (32, 208), wide (256) and generic (7) kernels."""
    z1, hi, lo = E.root_tie_pair(D, oracle)
    K, N = 70, 5
    cb = np.full((K, D), 10.0, np.float32) + np.arange(K, dtype=np.float32)[:, None]
    cb[3], cb[66] = hi, lo                                        # (more than 64 codes apart: two groups of the wide kernel)
    z = np.repeat(z1[None], N, 0)
    idx, best = _check(ops, oracle, z, cb, O.DIST_NORM, f"root tie D={D} norm")
    assert (idx == 3).all()
    idx, best = _check(ops, oracle, z, cb, O.DIST_SQSUM, f"root tie D={D} sqsum")
    assert (idx == 66).all()
    cb[3], cb[66] = lo, hi                                        # the other way round both rules take the lower index
    for dist in DISTS:
        idx, _ = _check(ops, oracle, z, cb, dist, f"root tie D={D} swapped")
        assert (idx == 3).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the wide kernel: pad codes, NaN codes, overflowing rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("D", [209, 256, 300, 384, 512])
def test_wide_kernel_pad_codes_and_non_finite(ops, oracle, D, dist):
    """K % 64 != 0: the last group's pad codes are zeros in LDS, and only the `k < K` guard keeps them from winning an all-zero
    latent row (a pad code winning shows as best == 0).  A code holding one NaN element never wins (`v < best` is false), even
    for the row that sits on it.  A 3e38 row overflows every distance: code 0, best = +inf.  N = 1, 7, 9: one row, a partial and
    a second 8-row workgroup."""
    for K in (1, 63, 65, 127):
        for N in (1, 7, 9):
            rng = np.random.default_rng(D + K * 11 + N)
            cb = rng.uniform(0.5, 1.5, (K, D)).astype(np.float32)
            knan = K // 2
            on_nan = cb[knan].copy()
            if K > 1:
                cb[knan, D - 3] = np.nan
            kinds = {"zero": np.zeros(D, np.float32), "on_nan_code": on_nan, "3e38": np.full(D, 3e38, np.float32)}
            variants = [[k] for k in kinds] if N == 1 else [list(kinds)]
            for kinds_here in variants:
                z = rng.uniform(0.5, 1.5, (N, D)).astype(np.float32)
                rows = {}
                for i, k in enumerate(kinds_here):
                    r = (N - 1, 0, N // 2)[i] if N > 1 else 0
                    z[r] = kinds[k]
                    rows[k] = r
                idx, best = _check(ops, oracle, z, cb, dist, f"wide D={D} K={K} N={N} {kinds_here}")
                if "zero" in rows:
                    assert best[rows["zero"]] > 0.0 and idx[rows["zero"]] < K
                if "on_nan_code" in rows and K > 1:
                    assert idx[rows["on_nan_code"]] != knan
                if "3e38" in rows:
                    assert idx[rows["3e38"]] == 0 and best[rows["3e38"]] == np.inf
            # finite inputs of the same shape: all three routes
            zf = rng.uniform(0.5, 1.5, (N, D)).astype(np.float32)
            zf[0] = 0.0
            cbf = np.nan_to_num(cb, nan=1.0)
            _check(ops, oracle, zf, cbf, dist, f"wide D={D} K={K} N={N} finite")


# ---------------------------------------------------------------------------------------------------------------------------
# the generic kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("D", [1, 3, 7, 33, 203])
def test_generic_kernel_widths(ops, oracle, D, dist):
    N, K = 100, 37
    rng = np.random.default_rng(D)
    cb = rng.uniform(0, 1, (K, D)).astype(np.float32)
    cb[K - 1] = cb[2]
    z = (cb[rng.integers(0, K, N)] + 0.01 * rng.standard_normal((N, D))).astype(np.float32)
    z[0] = z[64] = z[N - 1] = cb[2]
    idx, _ = _check(ops, oracle, z, cb, dist, f"generic D={D}")
    assert idx[0] == idx[64] == idx[N - 1] == 2


def _lib_nearest(ops, z, cb, dist, N, K, D, zq=True, best=True, usage=True, offsets=(0, 0, 0)):
    """lipvq_nearest_f32 through the library on views that start offsets = (z, codebook, zq) floats into their allocations;
    returns (rc, idx, zq, best, usage - prefill), outputs between guard floats."""
    def at(a, off):
        buf = torch.full((a.size + off + 4,), SENTINEL, device="cuda")
        v = buf[off:off + a.size]
        v.copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
        return v
    zd, cbd = at(z, offsets[0]), at(cb, offsets[1])
    idxb = torch.full((N + 2,), -5, device="cuda", dtype=torch.int64)
    zqb = torch.full((N * D + 8,), SENTINEL, device="cuda")
    bestb = torch.full((N + 2,), SENTINEL, device="cuda")
    ub = dev(np.concatenate([[-9], _prefill(K), [-9]]).astype(np.int64))
    o = offsets[2] + (4 if offsets[2] == 0 else 0)                 # (zq aligned: start one 16-byte unit in, a guard unit before)
    rc = ops.lib.lipvq_nearest_f32(zd.data_ptr(), cbd.data_ptr(), idxb.data_ptr() + 8, zqb.data_ptr() + 4 * o if zq else None,
                                   ub.data_ptr() + 8 if usage else None, bestb.data_ptr() + 4 if best else None,
                                   N, K, D, dist, _stream())
    torch.cuda.synchronize()
    idxh, zqh, besth, uh = idxb.cpu().numpy(), zqb.cpu().numpy(), bestb.cpu().numpy(), ub.cpu().numpy()
    assert idxh[0] == idxh[-1] == -5 and besth[0] == besth[-1] == np.float32(SENTINEL) and uh[0] == uh[-1] == -9
    zq_region = zqh[o:o + N * D]
    assert (np.delete(zqh, np.s_[o:o + N * D]) == np.float32(SENTINEL)).all(), "zq: a float outside the N x D rows was written"
    if not zq:
        assert (zq_region == np.float32(SENTINEL)).all()
    if not best:
        assert (besth == np.float32(SENTINEL)).all()
    if not usage:
        assert np.array_equal(uh[1:-1], _prefill(K))
    return rc, idxh[1:-1], zq_region.reshape(N, D), besth[1:-1], uh[1:-1] - _prefill(K)


@pytest.mark.parametrize("dist", DISTS)
def test_misaligned_operands_take_the_generic_kernel(ops, oracle, dist):
    """D = 64 belongs to the direct kernel, whose float4 loads need z, codebook and zq 16-byte aligned: each of them one float
    off sends the call to the generic kernel -- the same idx / zq / best / usage as the aligned call and as the oracle."""
    N, K, D = 300, 129, 64
    rng = np.random.default_rng(dist)
    cb = rng.uniform(0, 1, (K, D)).astype(np.float32)
    cb[K - 1] = cb[1]
    z = (cb[rng.integers(0, K, N)] + 0.01 * rng.standard_normal((N, D))).astype(np.float32)
    z[0] = z[N - 1] = cb[1]
    idx_ref, zq_ref, usage_ref, best_ref = oracle.nearest(z, cb, dist, want_best=True)
    for offsets in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 2, 1)):
        rc, idx, zq, best, usage = _lib_nearest(ops, z, cb, dist, N, K, D, offsets=offsets)
        assert rc == 0, (offsets, ops.lib.lipvq_last_error())
        assert np.array_equal(idx, idx_ref) and np.array_equal(zq, zq_ref), offsets
        assert np.array_equal(best, best_ref) and np.array_equal(usage, usage_ref), offsets


# ---------------------------------------------------------------------------------------------------------------------------
# NULL outputs, N = 0
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 256, 7])
def test_null_outputs(ops, oracle, D):
    """zq, best and usage are optional, each on its own and all together, in the direct, wide and generic kernels; what is passed is
    written as before, what is not stays untouched.  N = 0 returns 0 and touches nothing."""
    N, K = 77, 70
    rng = np.random.default_rng(D)
    cb = rng.uniform(0, 1, (K, D)).astype(np.float32)
    z = (cb[rng.integers(0, K, N)] + 0.01 * rng.standard_normal((N, D))).astype(np.float32)
    for dist in DISTS:
        idx_ref, zq_ref, usage_ref, best_ref = oracle.nearest(z, cb, dist, want_best=True)
        for want in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            rc, idx, zq, best, usage = _lib_nearest(ops, z, cb, dist, N, K, D, zq=want[0], best=want[1], usage=want[2])
            assert rc == 0 and np.array_equal(idx, idx_ref), want
            if want[0]:
                assert np.array_equal(zq, zq_ref), want
            if want[1]:
                assert np.array_equal(best, best_ref), want
            if want[2]:
                assert np.array_equal(usage, usage_ref), want
    rc, idx, zq, best, usage = _lib_nearest(ops, z, cb, O.DIST_NORM, 0, K, D)
    assert rc == 0 and (usage == 0).all() and idx.size == 0
    assert ops.lib.lipvq_nearest_f32(None, None, None, None, None, None, 0, K, D, O.DIST_NORM, _stream()) == 0
