"""GPU: the sibling `bin_enabled` tokenizer (csrc/lipvq_bin.hip, lipvq_vae_amd/binning.py) where tests/test_gpu_bin.py does not go:
action vectors wider than one wave (A > 64), the LDS sizing branches of lipvq_bin_hidden_f32 and its refusal, ragged row / column
counts inside guard bands, the min/max kernel at its block and column edges, NaN statistics, edge-value statistics and probe values
against stock torch, and the module's gradients against float64 autograd through every route of scatter_add with num_bins codes.

Yardsticks (tests/bin_ref.py, held to their conditions on the CPU by tests/test_bin_ref_host.py):
  * integers and statistics: the canonical oracle AND stock torch on the CPU, exactly (floats: equal, NaN in the same places);
  * the table sum: the oracle bit for bit, and the float64 sum within the recursive-summation bound (A + 1) u (|b1| + sum |P_i|);
  * gradients: float64 autograd of embedding gather, cat, Linear, GELU, Linear, GELU on the module's own bins, E2E = 2e-5 of a
    gradient's largest magnitude up to 4097 rows; from 32 781 rows on max(E2E, 4 x the stock fp32 CPU module's own error).

Which path a shape of bin_hidden reaches (SW = slice width; rows = A * num_bins):
  rows <= 320: SW = floor(20480 / rows / 64) * 64 (two workgroups per CU); 321 .. 600: SW = 64, one workgroup per CU, up to 150 KiB
  of LDS; 601 and up: refused with LIPVQ_EUNSUPPORTED.  A <= 64: one chunk of lane-held offsets per row step; A > 64: one per
  64 dimensions.  A workgroup step is 16 waves x 4 rows; rows are grid-strided over at most 512 workgroups (32 768 rows).

What these tests found when they were written: with the library before the per-chunk offsets and the NaN rule, every A > 64 case of
test_hidden_wide_action_vectors missed the summation bound by 2e4 .. 2.4e5 and every case of test_minmax_nan_parity failed.  A first
fix that formed the offsets inside a lane-strided column loop failed the (65, 5, 96), (100, 5, 130) and (200, 65, 16, 5) cases
(idle lanes of a ragged slice kept stale offsets) and passed (128, 4, 64) and (256, 2, 64): hence (128, 4, 96).  Used fractions of
the bounds on an MI355X: LABNOTES 4.4 (none above 0.42).
"""
import numpy as np
import pytest
import torch

import bin_ref as B
from fenced import _Fenced

pytestmark = pytest.mark.gpu

EUNSUPPORTED, EINVAL = -2, -1


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _capi():
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    return _capi.lib, _capi.check, lipvq_vae_amd.ops._stream


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def close(got, ref, allowed, name):
    """|got - ref| <= allowed elementwise (float64 on the CPU); prints the worst used fraction of the budget before asserting."""
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    err = (got - ref).abs()
    allowed = allowed if torch.is_tensor(allowed) else torch.full_like(err, float(allowed))
    frac = float((err / allowed.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{name}: max|err| {float(err.max()) if err.numel() else 0.0:.3e}, worst err/allowed {frac:.3f}")
    bad = err > allowed
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} elements over budget, worst err/allowed {frac:.3f}, "
                           f"first at {bad.nonzero()[0].tolist()}")
    return frac


# ---------------------------------------------------------------------------------------------------------------------------
# A.1  bin_hidden, wide A
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", B.HIDDEN_WIDE_N)
@pytest.mark.parametrize("A,nb,H", B.HIDDEN_WIDE)
def test_hidden_wide_action_vectors(oracle, ops, A, nb, H, N):
    """Dimensions 64 and up have a table row of their own: the oracle bit for bit, the float64 sum within the summation bound
    (before the offsets were formed per chunk of 64 dimensions, readlane(off, i) for i >= 64 wrapped to lane i - 64: A = 65 and up
    summed other dimensions' rows).  The last shape has whole chunks and a ragged slice (H = 96)."""
    bins, P, b1 = B.hidden_case(A, nb, H, N)
    h, pre = ops.bin_hidden(cuda(bins), cuda(P), cuda(b1), save_pre=True)
    h_ref, pre_ref = oracle.bin_hidden(bins, P, b1, save_pre=True)
    want, allowed = B.hidden_f64(bins, P, b1)
    frac = float((np.abs(host(pre).astype(np.float64) - want) / allowed).max())
    print(f"A={A} nb={nb} H={H} N={N}: worst |pre1 - float64| / bound {frac:.3f}")
    assert frac <= 1.0
    assert np.array_equal(host(pre), pre_ref) and np.array_equal(host(h), h_ref)
    assert np.array_equal(host(ops.bin_hidden(cuda(bins), cuda(P), cuda(b1))), h_ref)          # without pre1


# ---------------------------------------------------------------------------------------------------------------------------
# A.2  bin_hidden, LDS sizing edges
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("A,nb", B.HIDDEN_LDS_EDGES)
@pytest.mark.parametrize("H,N", [(96, 131), (64, 3)])
def test_hidden_lds_sizing_edges(oracle, ops, A, nb, H, N):
    bins, P, b1 = B.hidden_case(A, nb, H, N)
    h, pre = ops.bin_hidden(cuda(bins), cuda(P), cuda(b1), save_pre=True)
    h_ref, pre_ref = oracle.bin_hidden(bins, P, b1, save_pre=True)
    assert np.array_equal(host(pre), pre_ref) and np.array_equal(host(h), h_ref)


@pytest.mark.parametrize("A,nb", B.HIDDEN_REFUSED)
def test_hidden_refuses_more_than_600_table_rows(ops, A, nb):
    from lipvq_vae_amd._capi import LipvqLibraryError
    from lipvq_vae_amd.binning import AdaptiveBinActionEmbedding
    lib, _, stream = _capi()
    H, N = 64, 9
    bins, P, b1 = B.hidden_case(A, nb, H, N)
    tb, tP, tb1 = cuda(bins), cuda(P), cuda(b1)
    h, pre = _Fenced("h", N, H), _Fenced("pre1", N, H, offset_words=1)
    assert lib.lipvq_bin_hidden_f32(tb.data_ptr(), tP.data_ptr(), tb1.data_ptr(), h.ptr(), pre.ptr(), N, A, nb, H, stream()) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert h.untouched() and pre.untouched()
    with pytest.raises(LipvqLibraryError, match="status -2"):
        ops.bin_hidden(tb, tP, tb1)
    torch.manual_seed(A)
    m = AdaptiveBinActionEmbedding(A, 8, num_bins=nb).cuda()
    with pytest.raises(LipvqLibraryError, match="status -2"), torch.no_grad():
        m(torch.randn(N, A, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------------
# A.3  bin_hidden, ragged shapes inside guard bands
# ---------------------------------------------------------------------------------------------------------------------------

def _hidden_fenced(lib, stream, tb, tP, tb1, N, A, nb, H, with_pre, off):
    h = _Fenced("h", N, H, offset_words=off)
    pre = _Fenced("pre1", N, H, offset_words=off)
    rc = lib.lipvq_bin_hidden_f32(tb.data_ptr(), tP.data_ptr(), tb1.data_ptr(), h.ptr(), pre.ptr() if with_pre else None, N, A, nb, H, stream())
    assert rc == 0
    torch.cuda.synchronize()
    if not with_pre:
        assert pre.untouched()
    return h.check(), (pre.check() if with_pre else None)


@pytest.mark.parametrize("H", B.HIDDEN_RAGGED_H)
def test_hidden_ragged_rows_and_columns(oracle, H):
    lib, _, stream = _capi()
    A, nb = B.HIDDEN_RAGGED_A_NB
    assert A * nb == 140
    for N in B.HIDDEN_RAGGED_N:
        bins, P, b1 = B.hidden_case(A, nb, H, N)
        tb, tP, tb1 = cuda(bins), cuda(P), cuda(b1)
        h_ref, pre_ref = oracle.bin_hidden(bins, P, b1, save_pre=True)
        for with_pre in (True, False):
            for off in (0, 1):
                h, pre = _hidden_fenced(lib, stream, tb, tP, tb1, N, A, nb, H, with_pre, off)
                assert np.array_equal(host(h), h_ref), (N, with_pre, off)
                assert pre is None or np.array_equal(host(pre), pre_ref), (N, off)


def test_hidden_grid_stride(oracle):
    lib, _, stream = _capi()
    A, nb = B.HIDDEN_RAGGED_A_NB
    N, H = B.HIDDEN_GRID_STRIDE
    assert N > 512 * 16 * 4                                                    # more rows than one pass of the largest grid
    bins, P, b1 = B.hidden_case(A, nb, H, N)
    tb, tP, tb1 = cuda(bins), cuda(P), cuda(b1)
    h_ref, pre_ref = oracle.bin_hidden(bins, P, b1, save_pre=True)
    for with_pre, off in ((True, 1), (False, 0)):
        h, pre = _hidden_fenced(lib, stream, tb, tP, tb1, N, A, nb, H, with_pre, off)
        assert np.array_equal(host(h), h_ref) and (pre is None or np.array_equal(host(pre), pre_ref))


# ---------------------------------------------------------------------------------------------------------------------------
# A.4 / A.5  bin_minmax
# ---------------------------------------------------------------------------------------------------------------------------

def _minmax_fenced(lib, stream, x, lo0, hi0):
    N, A = x.shape
    lo, hi = _Fenced("running_min", A, offset_words=1), _Fenced("running_max", A)
    lo.t.copy_(cuda(lo0))
    hi.t.copy_(cuda(hi0))
    tx = cuda(x)
    assert lib.lipvq_bin_minmax_f32(tx.data_ptr(), lo.ptr(), hi.ptr(), N, A, stream()) == 0
    torch.cuda.synchronize()
    return host(lo.check()), host(hi.check())


@pytest.mark.parametrize("A", B.MINMAX_A)
def test_minmax_edges_equal_torch(oracle, A):
    """The sign of a zero statistic is not compared: it depends on the order in which +0 and -0 are visited and cannot move a
    boundary (fma(step, 0, -0.0) is +0)."""
    lib, _, stream = _capi()
    for N in B.MINMAX_N:
        x = B.minmax_case(A, N)
        for start in B.MINMAX_START:
            lo0, hi0 = B.minmax_start(A, start)
            wlo, whi = B.minmax_torch(x, lo0, hi0)
            lo, hi = _minmax_fenced(lib, stream, x, lo0, hi0)
            assert B.same_floats(lo, wlo, False) and B.same_floats(hi, whi, False), (N, start)
            olo, ohi = oracle.bin_minmax(x, lo0, hi0)
            assert B.same_floats(lo, olo, False) and B.same_floats(hi, ohi, False), (N, start)


def test_minmax_refuses_257_columns(ops):
    from lipvq_vae_amd._capi import LipvqLibraryError
    lib, _, stream = _capi()
    A, N = 257, 3
    x = cuda(B.minmax_case(A, N))
    lo, hi = _Fenced("running_min", A), _Fenced("running_max", A)
    assert lib.lipvq_bin_minmax_f32(x.data_ptr(), lo.ptr(), hi.ptr(), N, A, stream()) == EINVAL
    torch.cuda.synchronize()
    assert lo.untouched() and hi.untouched()
    with pytest.raises(LipvqLibraryError, match="status -1"):
        ops.bin_minmax(x, torch.zeros(A, device="cuda"), torch.zeros(A, device="cuda"))


@pytest.mark.parametrize("A", B.NAN_A)
def test_minmax_nan_parity(oracle, A):
    """A NaN anywhere in a column makes both statistics of that column NaN, they stay NaN over later finite batches, and the other
    columns are what they would have been (torch.minimum / maximum of Tensor.min / max on the CPU)."""
    lib, _, stream = _capi()
    for N in B.NAN_N:
        x, nan_cols, later = B.nan_case(A, N)
        lo0, hi0 = B.minmax_start(A, "inf")
        wlo, whi = B.minmax_torch(x, lo0, hi0)
        lo, hi = _minmax_fenced(lib, stream, x, lo0, hi0)
        assert np.array_equal(np.flatnonzero(np.isnan(lo)), nan_cols) and np.array_equal(np.flatnonzero(np.isnan(hi)), nan_cols), N
        assert B.same_floats(lo, wlo, False) and B.same_floats(hi, whi, False), N
        wlo2, whi2 = B.minmax_torch(later, wlo, whi)
        lo2, hi2 = _minmax_fenced(lib, stream, later, lo, hi)
        assert np.array_equal(np.flatnonzero(np.isnan(lo2)), nan_cols)
        assert B.same_floats(lo2, wlo2, False) and B.same_floats(hi2, whi2, False), N
        # a NaN batch on finite statistics
        flo, fhi = B.minmax_start(A, "finite")
        wlo3, whi3 = B.minmax_torch(x, flo, fhi)
        lo3, hi3 = _minmax_fenced(lib, stream, x, flo, fhi)
        assert B.same_floats(lo3, wlo3, False) and B.same_floats(hi3, whi3, False), N


def test_module_statistics_keep_a_nan(ops):
    from lipvq_vae_amd.binning import AdaptiveBinActionEmbedding
    torch.manual_seed(0)
    m = AdaptiveBinActionEmbedding(3, 8, num_bins=5).cuda()
    with torch.no_grad():
        m(torch.tensor([[0.5, 1.0, 0.0], [float("nan"), 2.0, 1.0], [-1.0, 3.0, 2.0], [2.0, 4.0, 3.0]], device="cuda"))
        m(torch.tensor([[0.5, 9.0, -7.0]], device="cuda"))
    lo, hi = m.running_min.tolist(), m.running_max.tolist()
    assert np.isnan(lo[0]) and np.isnan(hi[0]) and lo[1:] == [1.0, -7.0] and hi[1:] == [9.0, 3.0]


# ---------------------------------------------------------------------------------------------------------------------------
# A.6  discretize / boundaries on edge statistics and edge values
# ---------------------------------------------------------------------------------------------------------------------------

def _discretize_fenced(lib, stream, tx, tlo, thi, nb):
    N, A = tx.shape
    bins = _Fenced("bins", A, N, offset_words=2, dtype=torch.int64)
    bd = _Fenced("boundaries", A, nb + 1, offset_words=1)
    assert lib.lipvq_bin_discretize_f32(tx.data_ptr(), tlo.data_ptr(), thi.data_ptr(), bins.ptr(), N, A, nb, stream()) == 0
    assert lib.lipvq_bin_boundaries_f32(tlo.data_ptr(), thi.data_ptr(), bd.ptr(), A, nb, stream()) == 0
    torch.cuda.synchronize()
    return bins.check(), bd.check()


@pytest.mark.parametrize("nb", B.EDGE_NB)
def test_edge_statistics_and_values_equal_torch(oracle, nb):
    """Bins equal the CPU's torch.linspace -> bucketize -> clamp exactly and boundaries equal torch.linspace's as floats on the ten
    statistics columns of bin_ref.EDGE_STATS; on the device, where the reference class would run, bins equal torch.bucketize on
    our boundaries exactly, and our boundaries are within 2 ulp of max(|min|, |max|) of the device's torch.linspace on every column
    whose range max - min is finite (both evaluate start + step i, or its mirror, with at most two roundings; where the step
    itself is infinite or NaN there is no such statement, and the comparison is printed)."""
    lib, _, stream = _capi()
    x, want_bd = B.edge_values(nb)
    lo, hi = B.edge_stats()
    tx, tlo, thi = cuda(x), cuda(lo), cuda(hi)
    bins, bd = _discretize_fenced(lib, stream, tx, tlo, thi, nb)
    assert B.same_floats(host(bd), want_bd, sign_of_zero=False)
    assert np.array_equal(host(bins), B.torch_bins(x, want_bd, nb))
    o_bins, o_bd = oracle.bin_discretize(x, lo, hi, nb, want_boundaries=True)
    assert np.array_equal(host(bins), o_bins) and B.same_floats(host(bd), o_bd, sign_of_zero=False)
    # on the device
    A = len(lo)
    dev_bins = torch.stack([torch.clamp(torch.bucketize(tx[:, i].contiguous(), bd[i].contiguous()) - 1, 0, nb - 1) for i in range(A)])
    assert torch.equal(dev_bins, bins)
    dev_bd = host(torch.stack([torch.linspace(tlo[i], thi[i], nb + 1, device="cuda") for i in range(A)]))
    ours = host(bd)
    with np.errstate(all="ignore"):
        finite_range = np.isfinite(hi - lo)
    assert finite_range.sum() == 5
    for i in range(A):
        same = B.same_floats(ours[i], dev_bd[i], sign_of_zero=False)
        print(f"nb={nb} statistics {B.EDGE_STATS[i]}: device linspace {'bit-equal' if same else 'differs'}"
              + ("" if finite_range[i] else "  (no finite step: not asserted)"))
        if finite_range[i]:
            ulp = float(np.spacing(np.float32(max(abs(lo[i]), abs(hi[i])))))
            diff = np.abs(ours[i].astype(np.float64) - dev_bd[i].astype(np.float64))
            print(f"    max |ours - device| = {diff.max():.3e} = {diff.max() / ulp:.2f} ulp")
            assert np.all(diff <= 2.0 * ulp)


def test_discretize_limit(oracle, ops):
    from lipvq_vae_amd._capi import LipvqLibraryError
    lib, _, stream = _capi()
    A, N = 16, 301
    rng = B.rng_of(A, N, 12)
    x = rng.standard_normal((N, A)).astype(np.float32)
    lo, hi = x[:N // 2].min(0), x[:N // 2].max(0)                              # the other half clamps
    tx, tlo, thi = cuda(x), cuda(lo), cuda(hi)
    bins = _Fenced("bins", A, N, dtype=torch.int64)
    assert lib.lipvq_bin_discretize_f32(tx.data_ptr(), tlo.data_ptr(), thi.data_ptr(), bins.ptr(), N, A, 256, stream()) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert bins.untouched()
    with pytest.raises(LipvqLibraryError, match="status -2"):
        ops.bin_discretize(tx, tlo, thi, 256)
    got, bd = _discretize_fenced(lib, stream, tx, tlo, thi, 255)
    o_bins, o_bd = oracle.bin_discretize(x, lo, hi, 255, want_boundaries=True)
    assert np.array_equal(host(got), o_bins) and np.array_equal(host(bd), o_bd)
    assert int(got.min()) == 0 and int(got.max()) == 254


# ---------------------------------------------------------------------------------------------------------------------------
# B  gradients of the module against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------------

def _module(A, D, nb):
    from lipvq_vae_amd.binning import AdaptiveBinActionEmbedding
    sd = B.module_state(A, D, nb)
    m = AdaptiveBinActionEmbedding(A, D, num_bins=nb)
    full = dict(sd)
    full["running_min"], full["running_max"] = m.running_min.clone(), m.running_max.clone()
    m.load_state_dict(full, strict=True)
    return m.cuda(), sd


UPSTREAM = 3.5                        # the second backward's upstream gradient is UPSTREAM * R: .grad then holds (1 + UPSTREAM) x


def _run_gradients(N, A, D, nb, constant_col=None, large=False, tag=""):
    """One forward / backward with upstream R, checked; a second with upstream UPSTREAM * R accumulating into .grad, checked
    against (1 + UPSTREAM) x the reference.  Returns (the first run's gradients, the worst used fraction)."""
    m, sd = _module(A, D, nb)
    x = B.grad_actions(N, A, nb, constant_col=constant_col)
    R = torch.from_numpy(B.grad_upstream(N, D))
    tx, tR = cuda(x), R.cuda()
    out = m(tx)
    bins = m.last_bins.t().contiguous().cpu()
    assert np.array_equal(host(m.last_bins), B.torch_bins(x, B.torch_boundaries(x.min(0), x.max(0), nb), nb))
    out64, ref = B.stock_module_grads(sd, bins, R, torch.float64)
    bound = {k: B.E2E for k in ref}
    if large:
        _, g32 = B.stock_module_grads(sd, bins, R, torch.float32)
        for k in ref:
            dev = float((g32[k].double() - ref[k]).abs().max() / ref[k].abs().max().clamp(min=1e-300))
            bound[k] = max(B.E2E, B.LARGE_FACTOR * dev)
            print(f"{tag}{k}: stock fp32 CPU module's own error {dev:.3e} of max|ref|, bound {bound[k]:.3e}")
    close(out, out64, 1e-5 * (1.0 + out64.abs()), tag + "out")
    (out * tR).sum().backward()
    first = {k: p.grad.clone() for k, p in m.named_parameters()}
    assert set(first) == set(ref)
    worst = 0.0
    for k, g in first.items():
        worst = max(worst, close(g, ref[k], bound[k] * max(float(ref[k].abs().max()), 1e-300), f"{tag}{k}"))
    (UPSTREAM * (m(tx) * tR).sum()).backward()
    for k, p in m.named_parameters():
        total = (1.0 + UPSTREAM) * ref[k]
        worst = max(worst, close(p.grad, total, bound[k] * max(float(total.abs().max()), 1e-300), f"{tag}{k} (accumulated, upstream {UPSTREAM})"))
    return first, worst


@pytest.mark.parametrize("N,A,D,nb", B.GRAD_SMALL)
def test_gradients_against_float64_autograd(N, A, D, nb):
    _run_gradients(N, A, D, nb)


def test_gradients_with_a_constant_column():
    N, A, D, nb = B.GRAD_CONSTANT
    _run_gradients(N, A, D, nb, constant_col=1)


@pytest.mark.parametrize("N,A,D,nb", B.GRAD_LARGE)
def test_gradients_through_every_scatter_route(N, A, D, nb):
    """scatter_add with K = num_bins codes: LDS atomics (32 781 rows), the counting sort (66 000 rows, 20 and 2 codes) and, with one
    code, the LDS atomics again (the sort refuses K < 2).  Used fractions of the bound measured on an MI355X: see LABNOTES 4.4."""
    from lipvq_vae_amd._capi import lib
    assert bool(lib.lipvq_scatter_add_sorted_supported(N, nb, 32 * A)) == (nb >= 2)
    _, worst = _run_gradients(N, A, D, nb, large=True, tag=f"[{N},{A},{D},{nb}] ")
    print(f"[{N},{A},{D},{nb}] worst used fraction {worst:.3f}")


@pytest.mark.parametrize("N,A,D,nb", B.GRAD_DETERMINISTIC)
def test_gradients_are_bit_identical_in_deterministic_mode(N, A, D, nb):
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        a, wa = _run_gradients(N, A, D, nb, large=True, tag=f"det run 1 [{N},{nb}] ")
        b, wb = _run_gradients(N, A, D, nb, large=True, tag=f"det run 2 [{N},{nb}] ")
    finally:
        torch.use_deterministic_algorithms(prev)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    print(f"deterministic [{N},{A},{D},{nb}] worst used fraction {max(wa, wb):.3f}")


@pytest.mark.parametrize("N", B.SCATTER_N)
def test_scatter_add_with_few_codes(ops, N):
    """ops.scatter_add at K = num_bins-sized code counts (the scatter tests of tests/test_gpu_kernels.py start at 37 codes): the
    sequential routes equal the fp32 row-order loop bit for bit, the others the float64 index_add_ to 2e-6 of that test's scale."""
    for K in B.SCATTER_K:
        for D in B.SCATTER_D:
            g, idx = B.scatter_case(N, K, D)
            want = B.scatter_sequential_fp32(g, idx, K)
            gt, it = cuda(g), cuda(idx)
            sortable = bool(ops.lib.lipvq_scatter_add_sorted_supported(N, K, D))
            assert sortable == (N >= 32768 and K >= 2)
            seq = [ops.scatter_add(gt, it, K, deterministic=True), ops.scatter_add(gt, it, K, route="sequential_scan")]
            if sortable:
                seq.append(ops.scatter_add(gt, it, K, route="sequential_sorted"))
            for s in seq:
                assert np.array_equal(host(s), want), (K, D)
            ref = torch.zeros(K, D, dtype=torch.float64).index_add_(0, torch.from_numpy(idx), torch.from_numpy(g).double())
            counts = np.bincount(idx, minlength=K)
            scale = max(float(np.abs(g).max() * np.sqrt(max(1, counts.max()))), float(ref.abs().max()))
            others = [("default", ops.scatter_add(gt, it, K, deterministic=False)), ("atomics", ops.scatter_add(gt, it, K, route="atomics"))]
            if sortable:
                others.append(("sorted", ops.scatter_add(gt, it, K, route="sorted")))
            for name, o in others:
                err = float((o.cpu().double() - ref).abs().max())
                print(f"N={N} K={K} D={D} {name}: max|err| {err:.3e} = {err / (2e-6 * scale):.3f} of the bound")
                assert err <= 2e-6 * scale, (K, D, name)
