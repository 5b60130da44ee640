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
