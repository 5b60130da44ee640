"""GPU: the counting-sort scatter-add (csrc/lipvq_scatter.hip) and the scanning kernel (lipvq_scatter_add_det_f32) against the
numpy restatement of their two sum orders (tests/scatter_ref.py), bit for bit: the row order inside hot codes, the 256-row
segment, the order of the segment sums, "gC is accumulated into", the block shapes of the three K regimes, N at block edges, D at
64-column slice edges, the 16-row and 32-row branches, row 0 loaded by lanes past a segment's end and never added, signed zeros
and infinities, and the rows formed inside the summing kernel (lipvq_scatter_add_sorted_vq_f32).  Every comparison is on uint32
views; where the result is NaN by construction it is compared with isnan.  tests/test_scatter_ref_host.py shows on the CPU that
these inputs tell the wrong orders from the right one.  The C entry points are called directly (ops.scatter_add zero-fills gC)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import scatter_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

ROUTES = ("sorted", "sequential_sorted", "sequential_scan")


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ops, route, g, idx, K, gC0=None, fold=None):
    """gC0 (zeros when None) after the route has accumulated into it.  fold = (ze, table, alpha, gscale or None): the rows are
    formed in the kernel, g may be None."""
    idx = np.asarray(idx, np.int64)
    N = idx.shape[0]
    D = (g if g is not None else fold[0]).shape[1]
    assert idx.min() >= 0 and idx.max() < K                    # the kernels index LDS histograms with idx
    lib = ops.lib
    gt, it = (None if g is None else dev(np.asarray(g, np.float32))), dev(idx)
    out = torch.zeros(K, D, device="cuda") if gC0 is None else dev(np.asarray(gC0, np.float32))
    with ops._on(out.device):
        if route == "sequential_scan":
            assert fold is None
            ops.check(lib.lipvq_scatter_add_det_f32(ops._ptr(gt), ops._ptr(it), ops._ptr(out), N, K, D, ops._stream()), "det")
        else:
            assert lib.lipvq_scatter_add_sorted_supported(N, K, D)
            ws = torch.empty(lib.lipvq_scatter_add_sorted_workspace_bytes(N, K, D), device="cuda", dtype=torch.uint8)
            seq = {"sorted": 0, "sequential_sorted": 1}[route]
            if fold is None:
                ops.check(lib.lipvq_scatter_add_sorted_f32(ops._ptr(gt), ops._ptr(it), ops._ptr(out), ops._ptr(ws), N, K, D, seq,
                                                           ops._stream()), "sorted")
            else:
                ze, table, alpha, gscale = fold
                zt, tt = dev(np.asarray(ze, np.float32)), dev(np.asarray(table, np.float32))
                gs = None if gscale is None else dev(np.array([gscale], np.float32))
                ops.check(lib.lipvq_scatter_add_sorted_vq_f32(ops._ptr(gt), ops._ptr(zt), ops._ptr(tt), float(alpha), ops._ptr(gs),
                                                              ops._ptr(it), ops._ptr(out), ops._ptr(ws), N, K, D, seq,
                                                              ops._stream()), "sorted_vq")
    return out.cpu().numpy()


def ref(route, g, idx, K, gC0=None):
    return S.sorted_ref(g, idx, K, gC0) if route == "sorted" else S.seq_ref(g, idx, K, gC0)


def bad_codes(got, want):
    """The codes whose bits differ (for the assertion message)."""
    return np.nonzero(S.code_bits_differ(got, want))[0].tolist()


@pytest.fixture(scope="module")
def order():
    g, idx, K, gC0, counts = S.order_case()
    refs = {(r, z): ref(r, g, idx, K, None if z else gC0) for r in ("sorted", "sequential") for z in (True, False)}
    return dict(g=g, idx=idx, K=K, gC0=gC0, counts=counts, refs=refs)


@pytest.mark.parametrize("zero", [True, False], ids=["gC0=0", "gC0=random"])
@pytest.mark.parametrize("route", ROUTES)
def test_order(ops, order, route, zero):
    """N = 32768 + 13, K = 40, D = 65, counts 0, 1, 15..17, 31..33, 63..65, 255..257, 511..513, 1000 and one hot code, rows
    shuffled: the segment order on route sorted, one chain per code on the two sequential routes."""
    want = order["refs"]["sorted" if route == "sorted" else "sequential", zero]
    got = run(ops, route, order["g"], order["idx"], order["K"], None if zero else order["gC0"])
    assert S.bits_equal(got, want), bad_codes(got, want)
    if zero:                                                    # the wrapper: the same numbers from a zero-filled gC
        got = ops.scatter_add(dev(order["g"]), dev(order["idx"]), order["K"], route=route).cpu().numpy()
        assert S.bits_equal(got, want), bad_codes(got, want)


@pytest.mark.parametrize("zero", [True, False], ids=["gC0=0", "gC0=random"])
def test_combine_loop(ops, zero):
    """Codes of exactly 2, 15, 16, 17 segments and of 16 * 256 + 1 rows: the combine kernel's blocks of 16 and its tail."""
    g, idx, K, gC0, counts = S.combine_case()
    gC0 = None if zero else gC0
    want = S.sorted_ref(g, idx, K, gC0)
    got = run(ops, "sorted", g, idx, K, gC0)
    assert S.bits_equal(got, want), bad_codes(got, want)


@pytest.mark.parametrize("code", [1, 0])
def test_every_row_on_one_of_two_codes(ops, code):
    """K = 2, N = 32768 + 255: 129 segments on one code, the other keeps gC0."""
    g, idx, K, gC0 = S.one_code_case(code)
    for route in ("sorted", "sequential_sorted"):
        want = ref(route, g, idx, K, gC0)
        got = run(ops, route, g, idx, K, gC0)
        assert S.bits_equal(got, want), (route, bad_codes(got, want))
        assert S.bits_equal(got[1 - code], gC0[1 - code])


@pytest.mark.parametrize("edge", ["N=32768", "N=32769", "N=32768+block-1"])
@pytest.mark.parametrize("K", [2, 3, 2048, 2049, 8192, 8193, 16384])
def test_k_regimes(ops, K, edge):
    """The count / place block is 8192, 2048 or 1024 rows for K <= 2048, <= 8192, above; N on a block edge, one row past it and
    one row short of the next.  Codes 0 and K - 1 are used, most are empty and keep gC0 bit for bit."""
    N = {"N=32768": 32768, "N=32769": 32769, "N=32768+block-1": 32768 + S.block_rows(K) - 1}[edge]
    g, idx, gC0, counts = S.regime_case(K, N)
    assert counts[0] > 256 and counts[K - 1] >= 3 * 256 and (K <= 3 or (counts == 0).sum() > K - 40)
    for route in ("sorted", "sequential_sorted"):
        want = ref(route, g, idx, K, gC0)
        got = run(ops, route, g, idx, K, gC0)
        assert S.bits_equal(got, want), (route, bad_codes(got, want)[:10])
        assert S.bits_equal(got[counts == 0], gC0[counts == 0])


@pytest.mark.parametrize("D", [1, 63, 64, 65, 128, 129, 208])
def test_d_edges(ops, D):
    """One wave per 64-column slice: D on both sides of one, two and three slices."""
    g, idx, K, gC0, counts = S.order_case(seed=5, D=D, K=37)
    for route in ("sorted", "sequential_sorted"):
        want = ref(route, g, idx, K, gC0)
        got = run(ops, route, g, idx, K, gC0)
        assert S.bits_equal(got, want), (route, bad_codes(got, want))


def _fold_inputs(order, seed=6):
    rng = np.random.default_rng(seed)
    N, D = order["g"].shape
    return S.wide_rows(rng, N, D), S.wide_rows(rng, order["K"], D)


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("fold", [False, True], ids=["read", "fold"])
def test_row_zero_is_loaded_and_never_added(ops, order, fold, bad):
    """Lanes past a segment's end read perm as row 0, and the chunk loads that row for them.  With row 0 all NaN (all +inf) every
    code but its own equals the restatement and is finite -- the counts 1, 15, 17, 31, 33, 63, 65, 255, 257, ... all leave
    such lanes, on both sides of the 16-row branch and of FOLD's 32-row halves.  FOLD: the NaN sits in ze[0]."""
    g, idx, K, gC0 = order["g"].copy(), order["idx"], order["K"], order["gC0"]
    a = int(idx[0])
    others = np.arange(K) != a
    if fold:
        ze, table = _fold_inputs(order)
        ze[0] = bad
        rows = S.fold_rows(g, ze, table, idx, 0.37, None)
    else:
        g[0] = bad
        rows = g
    for route in ("sorted", "sequential_sorted"):
        want = ref(route, rows, idx, K, gC0)
        got = run(ops, route, g, idx, K, gC0, fold=(ze, table, 0.37, None) if fold else None)
        assert np.isfinite(want[others]).all() and not np.isfinite(want[a]).any()
        assert S.bits_equal(got[others], want[others]), (route, bad_codes(got[others], want[others]))
        assert np.isfinite(got[others]).all()
        if np.isnan(bad) or fold:                               # (f * (t - inf) is -inf: the chain may meet inf - inf)
            assert np.array_equal(np.isnan(got[a]), np.isnan(want[a])) and not np.isfinite(got[a]).any()
        else:
            assert S.bits_equal(got[a], want[a]) and (got[a] == np.inf).all()


@pytest.mark.parametrize("neg_zero_gc0", [False, True], ids=["gC0=+0", "gC0=-0"])
def test_special_values(ops, order, neg_zero_gc0):
    """A code whose only row is -0.0: the segment chain starts at +0.0, so the sorted route gives +0.0 whatever the sign of
    gC0's zero, the sequential chain keeps -0.0 + -0.0 = -0.0.  +inf rows give +inf, also from a code's second segment alone;
    +inf and -inf give NaN."""
    g, idx, K, counts = order["g"].copy(), order["idx"], order["K"], order["counts"]
    rows_of = lambda k: np.nonzero(idx == k)[0]                 # noqa: E731
    assert counts[1] == 1 and counts[2] == 15 and counts[3] == 16 and counts[13] == 257
    g[rows_of(1)] = -0.0
    g[rows_of(2)] = np.inf
    g[rows_of(3)] = np.inf
    g[rows_of(3)[7]] = -np.inf
    g[rows_of(13)[256]] = np.inf                                # the one row of the code's second segment
    gC0 = np.zeros((K, g.shape[1]), np.float32)
    if neg_zero_gc0:
        gC0[:] = -0.0
    for route in ROUTES:
        want = ref(route, g, idx, K, gC0)
        got = run(ops, route, g, idx, K, gC0)
        assert np.isnan(want[3]).all() and np.isnan(got[3]).all()
        keep = np.arange(K) != 3
        assert S.bits_equal(got[keep], want[keep]), (route, bad_codes(got[keep], want[keep]))
        assert (got[2] == np.inf).all() and (got[13] == np.inf).all()
        minus = neg_zero_gc0 and route != "sorted"
        assert (got[1].view(np.uint32) == (0x80000000 if minus else 0)).all()
        assert S.bits_equal(got[[0, 17]], gC0[[0, 17]])          # codes without rows: gC0's zero keeps its sign


@pytest.mark.parametrize("sequential", [0, 1])
@pytest.mark.parametrize("gscale", [None, 1.7], ids=["no-gscale", "gscale"])
@pytest.mark.parametrize("with_g", [True, False], ids=["g", "no-g"])
def test_rows_formed_in_the_kernel(ops, order, with_g, gscale, sequential):
    """lipvq_scatter_add_sorted_vq_f32 at the order test's shape: f = fp32(alpha * gscale), d = f * (table[k] - ze[n]) in two
    rounded operations, d + g[n] -- then the two orders, accumulated into a non-zero gC0.  Counts 31, 32, 33 and 63, 64, 65 sit
    on both sides of its 32-row halves."""
    idx, K, gC0 = order["idx"], order["K"], order["gC0"]
    g = order["g"] if with_g else None
    ze, table = _fold_inputs(order)
    route = "sequential_sorted" if sequential else "sorted"
    want = ref(route, S.fold_rows(g, ze, table, idx, 0.37, gscale), idx, K, gC0)
    got = run(ops, route, g, idx, K, gC0, fold=(ze, table, 0.37, gscale))
    assert S.bits_equal(got, want), bad_codes(got, want)


def test_wrapper_forms_rows_in_the_kernel_on_the_default_route(ops):
    """ops.scatter_add_vq, N = 65536 + 13: the non-deterministic route of a large batch is the segment order over formed rows."""
    rng = np.random.default_rng(8)
    N, K, D = 65536 + 13, 24, 33
    counts = np.zeros(K, np.int64)
    counts[:12] = (0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 700)
    idx, counts = S.idx_from_counts(rng, counts, N, 20)
    g, ze, table = S.wide_rows(rng, N, D), S.wide_rows(rng, N, D), S.wide_rows(rng, K, D)
    gs = np.float32(0.81)
    got = ops.scatter_add_vq(dev(g), dev(ze), dev(table), dev(idx), 0.37, gscale=dev(np.array(gs)), deterministic=False)
    want = S.sorted_ref(S.fold_rows(g, ze, table, idx, 0.37, gs), idx, K)
    assert S.bits_equal(got.cpu().numpy(), want), bad_codes(got.cpu().numpy(), want)
