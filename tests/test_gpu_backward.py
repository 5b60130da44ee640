"""GPU: every backward kernel against the float64 reference of tests/backward_ref.py (stock torch ops and autograd on the CPU),
at the shapes where the dispatchers of csrc/lipvq_mlp.hip and csrc/lipvq_bwd.hip change kernel, tile count or path.

Tolerances are derived, not tuned (backward_ref.py has the expressions).  Every matrix product of the backward-data chain is
checked layer-locally -- g1 against the float64 product formed from the kernel's OWN g2, and so on -- so one comparison sees one
dot product and one activation derivative; the allowed error per element is
    2 dot_bound |act'| + |dot| delta_act + one fp32 ulp of the result.
On top of that one end-to-end comparison per case holds the whole chain to 2e-5 max|ref| (test_wgrad_against_float64's bound).
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import lipvq_oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import backward_ref as R  # noqa: E402
from backward_edge_cases import mlp3_inputs as _mlp3_inputs  # noqa: E402  (the draws, shared with tests/test_gpu_backward_extent.py)

pytestmark = pytest.mark.gpu

# delta_act: absolute error of the fp32 activation derivatives against the exact float64 forms, MEASURED on the CPU over the dense
# sweep of test_gelu_derivative_on_device_tracks_the_canonical_one plus the planted values (backward_ref.act_sweep / PLANTED,
# 200 016 points): oracle.math_probe(x, 5) = lq_gelu_grad gives 1.504e-7, s (1 - s) in fp32 from oracle.math_probe(x, 3) =
# lq_sigmoid gives 8.86e-8.  tests/test_oracle_backward.py::test_measured_constants_hold re-measures both on every CPU run.
GELU_GRAD_ABS_ERR = R.GELU_GRAD_ABS_ERR
SIGMOID_GRAD_ABS_ERR = R.SIGMOID_GRAD_ABS_ERR
# the device evaluates GELU' in a straight-line form; test_gelu_derivative_on_device_tracks_the_canonical_one holds it to this
# distance from lq_gelu_grad.  (The device's sigmoid is lq_sigmoid itself, bit for bit: no allowance.)
GELU_DEVICE_ALLOWANCE = R.GELU_DEVICE_ALLOWANCE
DELTA_ACT = R.DELTA_ACT          # (the values live in tests/backward_ref.py: tests/test_gpu_large_extent.py uses the same budget)
E2E = 2e-5                       # whole-chain bound relative to max|ref| (the project's existing bound)

ENC = (O.ACT_GELU, O.ACT_GELU, O.ACT_SIGMOID)          # LLFQVAE_V4's encoder
DEC = (O.ACT_GELU, O.ACT_GELU, O.ACT_NONE)             # its decoder: pre2 = None, g2 is gy
RELU3 = (O.ACT_RELU, O.ACT_RELU, O.ACT_RELU)           # the plain VQVAE's stacks
MIX = (O.ACT_RELU, O.ACT_SIGMOID, O.ACT_GELU)
LDS_N = 65536 + 45                                     # LQ_MLP3_LDS_ROWS + a ragged tile


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def dev(a):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.cuda()


def close(got, ref, allowed, name):
    """|got - ref| <= allowed elementwise (float64 on the CPU); prints the worst used fraction of the budget before asserting."""
    got = R.f64(got)
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    err = (got - ref).abs()
    allowed = allowed if torch.is_tensor(allowed) else torch.full_like(err, float(allowed))
    frac = float((err / allowed.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{name}: max|err| {float(err.max()) if err.numel() else 0.0:.3e}, worst err/allowed {frac:.3f}")
    bad = err > allowed
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} elements over budget, worst err/allowed {frac:.3f}, "
                           f"first at {bad.nonzero()[0].tolist()}")


def e2e(got, ref, name):
    close(got, ref, E2E * max(float(ref.abs().max()), 1e-300), name + " (end to end)")


# ---------------------------------------------------------------------------------------------------------------------------
# mlp3_bwd
# ---------------------------------------------------------------------------------------------------------------------------
# (N, K0, J0, J1, J2, acts, want_gx).  The backward chain runs J2 -> J1 -> J0 -> K0: its "input width" in launch_mlp3_wg /
# mlp3_lds_takes is the forward J2 and its plane is (2 ceil(J2 / 2) + J1 + J0) * 33 floats.
MLP3_CASES = []
# mlp3_wg_kernel<true, 1>: N < 4096 keeps one 32-row sub-tile per workgroup; single row, ragged and whole last tiles
for _n in (1, 31, 32, 33, 80, 500, 4095):
    MLP3_CASES += [(_n, 7, 64, 128, 64, ENC, False), (_n, 64, 64, 128, 7, DEC, True)]
# mlp3_wg_kernel<true, 2>: N >= 4096 and 2 * plane <= 80 KiB; whole, one-row and one-tile-plus-one-row last workgroups
for _n in (4096, 4097, 4160 + 1):
    MLP3_CASES += [(_n, 7, 64, 128, 64, ENC, True), (_n, 64, 64, 128, 7, DEC, True)]
MLP3_CASES += [
    (4097, 7, 64, 128, 64, RELU3, True),
    (4097, 12, 64, 128, 208, ENC, True),      # J2 = 208: 2 * plane = 103 KiB > 80 KiB keeps ONE sub-tile at N >= 4096
    (4097, 208, 64, 128, 12, DEC, True),      # forward K0 = 208: seven output tiles of the last link, two sub-tiles
    (4097, 9, 64, 128, 118, ENC, True),       # the widest J2 that still takes two sub-tiles (2 * plane = 81 840 <= 81 920)
    (4097, 9, 64, 128, 119, ENC, True),       # ... and the first that does not (odd: padded to 120)
    # mlp3_lds_kernel<.., true, 0>: N >= 65 536 and hidden (64, 128) or (128, 64)
    (LDS_N, 7, 64, 128, 64, ENC, False), (LDS_N, 7, 64, 128, 64, ENC, True), (LDS_N, 64, 64, 128, 7, DEC, True),
    (LDS_N, 7, 128, 64, 64, ENC, True), (LDS_N, 64, 128, 64, 7, RELU3, True), (LDS_N, 64, 128, 64, 7, RELU3, False),
    # other hidden pairs stay on mlp3_wg_kernel at that size (mlp3_lds_select has no instance)
    (LDS_N, 12, 96, 64, 37, MIX, True), (LDS_N, 12, 32, 32, 37, MIX, True),
    # fallback mlp3_kernel<.., true>: launch_mlp3_wg declines above 150 KiB of LDS: (2 ceil(J2 / 2) + 192) * 132 > 153 600 from
    # J2 = 971 on at hidden (64, 128) / (128, 64); J2 = 970 is the last shape of the workgroup kernel
    (70, 7, 64, 128, 971, ENC, True), (70, 7, 128, 64, 971, RELU3, False), (33, 7, 64, 128, 970, ENC, True),
    (40, 7, 32, 32, 1099, MIX, True),         # hidden (32, 32): (1100 + 64) * 132 > 153 600 -> mlp3_kernel<1, 1, true>
    (40, 7, 96, 64, 1003, MIX, True),         # hidden (96, 64): (1004 + 160) * 132 > 153 600 -> mlp3_kernel<2, 3, true>
    (80, 64, 64, 128, 7, DEC, False),         # want_gx = False on the identity-output stack
    (500, 7, 64, 128, 64, RELU3, True), (500, 64, 128, 64, 7, RELU3, True),
]
# hidden widths (T0, T1 of the unit loops in mlp3_wg_kernel: 1 ... 8 tiles per layer against 8 waves)
MLP3_CASES += [(333, 12, j0, j1, 37, MIX, True) for j0, j1 in ((32, 32), (64, 128), (128, 64), (96, 64), (192, 64), (256, 256), (64, 256))]
# forward K0: the last link's output width (ragged / odd stores, 16-byte vector stores only at K0 % 4 == 0)
MLP3_CASES += [(100, k0, 64, 128, 16, DEC, True) for k0 in (1, 3, 7, 12, 33, 64, 208, 209, 512)]
# forward J2: the chain's input width (odd widths exercise the (J2 + 1) / 2 k-pair padding of the staged gy)
MLP3_CASES += [(100, 9, 64, 128, j2, ENC, True) for j2 in (1, 5, 7, 12, 64, 208, 300, 512)]


def _check_chain(out, gy, pre, W0, W1, W2, acts, want_gx, zero_row, g2_checked=False):
    """Layer-local budgets from the kernel's own upstream gradients, the end-to-end bound, exact zeros."""
    g2, g1, g0, gx = out
    if not g2_checked:
        if acts[2] == O.ACT_NONE:
            assert torch.equal(g2.cpu(), gy.cpu())
        else:
            r, tol = R.elementwise_ref_and_budget(gy, pre[2], acts[2], DELTA_ACT[acts[2]])
            close(g2, r, tol, "g2")
    r, tol = R.layer_ref_and_budget(g2, W2, pre[1], acts[1], DELTA_ACT[acts[1]])
    close(g1, r, tol, "g1")
    r, tol = R.layer_ref_and_budget(g1, W1, pre[0], acts[0], DELTA_ACT[acts[0]])
    close(g0, r, tol, "g0")
    if want_gx:
        r, tol = R.layer_ref_and_budget(g0, W0, None, O.ACT_NONE, 0.0)
        close(gx, r, tol, "gx")
    else:
        assert gx is None
    if gy is not None:
        for got, rf, name in zip((g2, g1, g0, gx), R.mlp3_bwd_ref(gy, pre, W0, W1, W2, acts), ("g2", "g1", "g0", "gx")):
            if got is not None:
                e2e(got, rf, name)
    # exact zeros: ReLU' at +0.0 and -0.0 (torch's threshold_backward), and the row whose upstream gradient is all zero
    for got, p, act in ((g2, pre[2], acts[2]), (g1, pre[1], acts[1]), (g0, pre[0], acts[0])):
        if act == O.ACT_RELU:
            at0 = (p == 0).cpu()
            assert int(at0.sum()) >= 2 and bool((got.cpu()[at0] == 0).all()), "ReLU' at a pre-activation of exactly 0 must be 0"
    if zero_row is not None:
        for got in (g2, g1, g0, gx):
            if got is not None:
                assert bool((got[zero_row] == 0).all()), "a zero upstream row must give exactly zero gradients"


@pytest.mark.parametrize("N,K0,J0,J1,J2,acts,want_gx", MLP3_CASES)
def test_mlp3_bwd_against_float64(ops, N, K0, J0, J1, J2, acts, want_gx):
    W0, W1, W2, gy, pre, zero_row = _mlp3_inputs(N, K0, J0, J1, J2, acts, N * 131 + K0 * 17 + J0 + 3 * J1 + 7 * J2)
    pk = ops.mlp3_pack_bwd(dev(W0), dev(W1), dev(W2))
    gyd = dev(gy)
    out = ops.mlp3_bwd(gyd, [None if p is None else dev(p) for p in pre], pk, acts, want_gx=want_gx)
    torch.cuda.synchronize()
    if acts[2] == O.ACT_NONE:
        assert out[0] is gyd                                   # g2 aliases gy on an identity output layer
    _check_chain(out, gy, pre, W0, W1, W2, acts, want_gx, zero_row)


def test_mlp3_bwd_refuses_hidden_widths_without_a_fallback_instance(ops):
    """At J2 = 971 the workgroup kernel's plane exceeds 150 KiB for every hidden pair; (256, 256) has no mlp3_kernel instance:
    the library must answer LIPVQ_EUNSUPPORTED (-2) -- no crash, no silent return."""
    from lipvq_vae_amd._capi import LipvqLibraryError
    N, K0, J0, J1, J2 = 40, 7, 256, 256, 971
    W0, W1, W2, gy, pre, _ = _mlp3_inputs(N, K0, J0, J1, J2, ENC, 5)
    pk = ops.mlp3_pack_bwd(dev(W0), dev(W1), dev(W2))
    with pytest.raises(LipvqLibraryError, match=r"status -2.*no kernel instance"):
        ops.mlp3_bwd(dev(gy), [dev(p) for p in pre], pk, ENC, want_gx=True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("with_gscale", [True, False])
def test_mlp3_bwd_folded_input_term_against_float64(ops, with_gscale):
    """in_term (mlp3_lds_kernel<.., true, 1>): gy := alpha gscale (sigmoid(pre2) - B[idx]), at the encoder's shape."""
    N, K0, J0, J1, J2 = LDS_N, 7, 64, 128, 64
    W0, W1, W2, _, pre, _ = _mlp3_inputs(N, K0, J0, J1, J2, ENC, 77)
    g = torch.Generator().manual_seed(78)
    cb = torch.rand(300, J2, generator=g)
    idx = torch.randint(0, 300, (N,), generator=g)
    alpha, gs = 0.37, (torch.tensor([3.0]) if with_gscale else None)
    pk = ops.mlp3_pack_bwd(dev(W0), dev(W1), dev(W2))
    assert ops.mlp3_bwd_vq_supported(N, pk)
    out = ops.mlp3_bwd(None, [dev(p) for p in pre], pk, ENC, want_gx=False, in_term=(None, None, dev(cb), dev(idx), alpha),
                       gscale=None if gs is None else dev(gs))
    torch.cuda.synchronize()
    gy_ref = R.scaled_diff_ref(R.act_ref(pre[2], O.ACT_SIGMOID), cb[idx], alpha, gs)
    g2_ref = gy_ref * R.act_grad_ref(pre[2], O.ACT_SIGMOID)
    # fp32 forms f = alpha gscale, sigmoid (5 u relative, backward_ref.LIP_FUNC_REL), the difference, two products and sigma'
    s = R.act_ref(pre[2], O.ACT_SIGMOID)
    f = abs(alpha * (3.0 if with_gscale else 1.0))
    d_gy = f * (R.LIP_FUNC_REL * s + 3.0 * R.U32 * (s - R.f64(cb[idx])).abs())
    tol = d_gy * R.act_grad_ref(pre[2], O.ACT_SIGMOID) + gy_ref.abs() * (SIGMOID_GRAD_ABS_ERR + 2.0 * R.U32) + R.ulp32(g2_ref)
    close(out[0], g2_ref, tol, "g2 (folded input term)")
    _check_chain(out, None, pre, W0, W1, W2, ENC, False, None, g2_checked=True)
    chain = R.mlp3_bwd_ref(g2_ref, [pre[0], pre[1], None], W0, W1, W2, (ENC[0], ENC[1], O.ACT_NONE))
    e2e(out[0], g2_ref, "g2")
    e2e(out[1], chain[1], "g1")
    e2e(out[2], chain[2], "g0")


@pytest.mark.parametrize("with_gscale", [True, False])
def test_mlp3_bwd_folded_output_term_against_float64(ops, with_gscale):
    """out_term (mlp3_lds_kernel<.., true, 2>): gx += alpha gscale (A - B[idx]), at the plain VQVAE's decoder shape."""
    N, K0, J0, J1, J2 = LDS_N, 64, 128, 64, 7
    W0, W1, W2, gy, pre, zero_row = _mlp3_inputs(N, K0, J0, J1, J2, RELU3, 91)
    g = torch.Generator().manual_seed(92)
    ze = torch.rand(N, K0, generator=g)
    E = torch.rand(128, K0, generator=g)
    idx = torch.randint(0, 128, (N,), generator=g)
    alpha, gs = 0.011, (torch.tensor([3.0]) if with_gscale else None)
    pk = ops.mlp3_pack_bwd(dev(W0), dev(W1), dev(W2))
    assert ops.mlp3_bwd_vq_supported(N, pk)
    out = ops.mlp3_bwd(dev(gy), [dev(p) for p in pre], pk, RELU3, want_gx=True, out_term=(dev(ze), None, dev(E), dev(idx), alpha),
                       gscale=None if gs is None else dev(gs))
    torch.cuda.synchronize()
    g2, g1, g0, gx = out
    _check_chain((g2, g1, g0, None), gy, pre, W0, W1, W2, RELU3, False, None)
    term = R.scaled_diff_ref(ze, E[idx], alpha, gs)
    chain, tol = R.layer_ref_and_budget(g0, W0, None, O.ACT_NONE, 0.0)
    # the term's own roundings (f, the difference, the product) and the final sum
    close(gx, chain + term, tol + 3.0 * R.U32 * term.abs() + R.ulp32(chain + term), "gx (folded output term)")
    e2e(gx, R.mlp3_bwd_ref(gy, pre, W0, W1, W2, RELU3)[3] + term, "gx")


# ---------------------------------------------------------------------------------------------------------------------------
# lipschitz_bwd
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", R.LIPSCHITZ_H)
@pytest.mark.parametrize("D", R.LIPSCHITZ_D)
def test_lipschitz_bwd_against_float64(ops, D, H):
    """Both branches in one matrix, rows close to the switch, sign(0) entries, an all-zero row, ragged 16-row groups.
    Rows whose float64 ratio is within 4 H u of 1 would be left out (fp32 and float64 may disagree about the branch there): the
    seeded inputs leave out NO row for any (D, H) -- asserted here, and checked on the CPU with the reference alone by
    tests/test_oracle_backward.py::test_lipschitz_cases_leave_out_no_row."""
    W, ci, gWn, roles = R.lipschitz_case(D, H, 1000 * D + H)
    ref_gW, ref_gci, ratio = R.lipschitz_bwd_ref(W, ci, gWn)
    assert int(((ratio - 1.0).abs() <= R.lipschitz_band(H)).sum()) == 0
    active = ratio < 1.0
    gW, gci = ops.lipschitz_bwd(dev(W), dev(ci), dev(gWn))
    scale, _ = ops.lipschitz_scale(dev(W), dev(ci))
    torch.cuda.synchronize()
    gW, gci, scale = gW.cpu(), gci.cpu(), scale.cpu()
    assert torch.isfinite(gW).all() and torch.isfinite(gci).all()
    # the branch the forward kernel took == the branch the backward kernel took == the reference's, row for row
    assert torch.equal(scale < 1.0, active), "forward kernel and float64 disagree about the clamped rows"
    assert torch.equal(gci != 0, active), "backward kernel's clamped rows differ from the forward kernel's"
    d_gW, d_gci = R.lipschitz_budget(W, ci, gWn)
    close(gW[active], ref_gW[active], d_gW[active], "gW (clamped rows)")
    close(gci[active], ref_gci[active], d_gci[active], "gci (clamped rows)")
    assert torch.equal(gW[~active], torch.from_numpy(gWn)[~active]) and bool((gci[~active] == 0).all())       # scale is exactly 1
    if "zero_row" in roles:
        r = roles["zero_row"]
        assert not bool(active[r]) and torch.isinf(ratio[r]) and torch.equal(gW[r], torch.from_numpy(gWn[r])) and gci[r] == 0
    if "zero_entries" in roles:
        r = roles["zero_entries"]
        z = torch.from_numpy(W[r] == 0)
        assert bool(active[r]) and int(z.sum()) >= 2
        want = (torch.from_numpy(gWn[r]).double() * (torch.nn.functional.softplus(R.f64(ci[r:r + 1])) / R.f64(W[r]).abs().sum()))[z]
        close(gW[r][z], want, d_gW[r][z], "gW at exact-zero weights (sign(0) = 0: gWn * scale)")


def test_lipschitz_bwd_refuses_rows_wider_than_256(ops):
    from lipvq_vae_amd._capi import LipvqLibraryError
    W = torch.randn(8, 257, device="cuda")
    with pytest.raises(LipvqLibraryError, match=r"status -2"):
        ops.lipschitz_bwd(W, torch.ones(8, device="cuda"), torch.randn(8, 257, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------------
# act_bwd, scaled_diff
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [O.ACT_RELU, O.ACT_SIGMOID, O.ACT_NONE, O.ACT_GELU])
def test_act_bwd_against_float64(ops, act):
    """g * act'(pre) on the dense sweep plus ReLU' at +-0 and saturated sigmoid' / GELU' (+-9, +-40, +-100)."""
    x = np.concatenate([R.act_sweep(), R.PLANTED])
    g = torch.Generator().manual_seed(act)
    gin = torch.randn(x.size, 1, generator=g) * 3.0
    got = ops.act_bwd(dev(gin), dev(x.reshape(-1, 1)), act).cpu()
    ref, tol = R.elementwise_ref_and_budget(gin, x.reshape(-1, 1), act, DELTA_ACT[act])
    close(got, ref, tol, "act_bwd")
    if act == O.ACT_NONE:
        assert torch.equal(got, gin)
    if act == O.ACT_RELU:
        pos = torch.from_numpy(x.reshape(-1, 1) > 0)
        assert torch.equal(got[pos], gin[pos]) and bool((got[~pos] == 0).all())          # exactly 0 at +0.0 and -0.0


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048 * 256 + 3])
@pytest.mark.parametrize("with_c", [False, True])
@pytest.mark.parametrize("with_gscale", [False, True])
def test_scaled_diff_bit_exact_and_against_float64(ops, n, with_c, with_gscale):
    """alpha * gscale * (a - b) + c: the fp32 expression with product and sum rounded separately, bit for bit (n crosses the
    2048-block grid-stride cap), and within three roundings of the float64 value."""
    g = torch.Generator().manual_seed(n + 2 * with_c + with_gscale)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    c = torch.randn(n, generator=g) if with_c else None
    gs = torch.tensor(3.7) if with_gscale else None
    alpha = 2.0 / 7.0
    got = ops.scaled_diff(dev(a), dev(b), alpha, gscale=None if gs is None else dev(gs), c=None if c is None else dev(c)).cpu()
    want = R.scaled_diff_fp32(a, b, alpha, gs, c)
    assert torch.equal(got, want)
    ref = R.scaled_diff_ref(a, b, float(np.float32(alpha)), gs, c)
    term = ref if c is None else ref - R.f64(c)
    close(got, ref, 3.0 * R.U32 * term.abs() + R.ulp32(ref), "scaled_diff")


# ---------------------------------------------------------------------------------------------------------------------------
# wgrad
# ---------------------------------------------------------------------------------------------------------------------------
ONE_CHUNK = 128                  # wgrad_chunk_rows: N <= 128 is one chunk, written directly (no reduce launch); above, 64-row chunks
WGRAD_CASES = []
# both sides of the one-chunk `direct` path, at a two-tile x four-tile pair (wg5, 64-row blocks) and a ragged 7 x 4 one (32-row)
for _n in (1, 31, 33, 127, ONE_CHUNK, ONE_CHUNK + 1):
    WGRAD_CASES += [(_n, 128, 64, O.ACT_GELU, "plain"), (_n, 196, 100, O.ACT_NONE, "plain")]
WGRAD_CASES += [
    # tile counts {1, 2, 4, 7}^2 of wgrad_wg5_kernel at ragged widths
    (129, 196, 64, O.ACT_NONE, "plain"), (129, 64, 200, O.ACT_GELU, "plain"), (129, 224, 224, O.ACT_NONE, "plain"),
    (1000, 196, 128, O.ACT_GELU, "plain"), (1000, 128, 224, O.ACT_RELU, "plain"), (500, 224, 196, O.ACT_NONE, "plain"),
    (33, 100, 36, O.ACT_NONE, "plain"), (129, 36, 100, O.ACT_GELU, "plain"), (129, 200, 100, O.ACT_NONE, "plain"),
    (80, 64, 7, O.ACT_NONE, "plain"), (80, 7, 128, O.ACT_GELU, "plain"),                 # one-tile operands with odd rows (element loads)
    # J & 3 != 0 or Kd & 3 != 0 at more than one tile: leaves the wg5 family (wgrad_wg_kernel)
    (129, 66, 64, O.ACT_NONE, "plain"), (129, 64, 130, O.ACT_GELU, "plain"), (33, 130, 66, O.ACT_NONE, "plain"),
    (1000, 66, 130, O.ACT_NONE, "plain"),
    # tile counts without a wg5 instance: 3, 5, 6, 8 (8 rows: `wide`, column blocks of 128 through the four-tile instance)
    (129, 96, 64, O.ACT_NONE, "plain"), (129, 160, 64, O.ACT_GELU, "plain"), (129, 192, 64, O.ACT_NONE, "plain"),
    (129, 256, 64, O.ACT_NONE, "plain"), (129, 64, 96, O.ACT_GELU, "plain"), (129, 64, 160, O.ACT_NONE, "plain"),
    (129, 64, 192, O.ACT_RELU, "plain"), (129, 64, 256, O.ACT_NONE, "plain"),
    # wide gradient operands: J % 128 == 0 above 224 columns, and J = 320 (the per-tile wgrad_kernel)
    (129, 256, 32, O.ACT_NONE, "plain"), (129, 384, 64, O.ACT_NONE, "plain"), (129, 512, 64, O.ACT_GELU, "plain"),
    (33, 512, 128, O.ACT_NONE, "plain"), (1000, 384, 100, O.ACT_NONE, "plain"), (129, 320, 64, O.ACT_NONE, "plain"),
    (33, 320, 100, O.ACT_GELU, "plain"),
    # G and H as 4-byte-offset views of flat buffers: contiguous (ops._chk passes them on), not 16-byte aligned -> no float4 loads
    (129, 128, 64, O.ACT_GELU, "misaligned"), (129, 196, 100, O.ACT_NONE, "misaligned"), (33, 64, 128, O.ACT_NONE, "misaligned"),
    # hidx gather with repeated and unused table rows
    (129, 64, 64, O.ACT_NONE, "gather"), (33, 128, 7, O.ACT_NONE, "gather"), (1000, 196, 64, O.ACT_NONE, "gather"),
    (129, 128, 64, O.ACT_GELU, "nobias"), (33, 196, 64, O.ACT_NONE, "nobias"), (1000, 64, 128, O.ACT_GELU, "nobias"),
]


@pytest.mark.parametrize("N,J,Kd,act,mode", WGRAD_CASES)
def test_wgrad_dispatch_edges_against_float64(ops, N, J, Kd, act, mode):
    """The float64 reference and the bound of test_wgrad_against_float64, at the edges of lipvq_wgrad_f32's dispatcher."""
    g = torch.Generator().manual_seed(N * 1009 + J * 31 + Kd)
    hidx = None
    if mode == "misaligned":
        gbuf, hbuf = torch.randn(N * J + 1, generator=g).cuda(), torch.randn(N * Kd + 1, generator=g).cuda()
        G, H = gbuf[1:].view(N, J), hbuf[1:].view(N, Kd)
        assert G.is_contiguous() and H.is_contiguous() and G.data_ptr() % 16 == 4 and H.data_ptr() % 16 == 4
    else:
        G = torch.randn(N, J, generator=g).cuda()
        H = torch.randn(50 if mode == "gather" else N, Kd, generator=g).cuda()
        if mode == "gather":
            hidx = (torch.randint(0, 10, (N,), generator=g) * 3).cuda()            # rows 0, 3, ..., 27 repeat; the others are unused
    gW, gb = ops.wgrad(G, H, h_act=act, hidx=hidx, want_bias=mode != "nobias")
    torch.cuda.synchronize()
    refW, refb = R.wgrad_ref(G, H, act, hidx)
    close(gW, refW, E2E * float(refW.abs().max()), "gW")
    if mode == "nobias":
        assert gb is None
    else:
        close(gb, refb, E2E * max(float(refb.abs().max()), N ** 0.5), "gb")


# ---------------------------------------------------------------------------------------------------------------------------
# whole modules at training-step sizes
# ---------------------------------------------------------------------------------------------------------------------------
def _compare_module_grads(model, ref):
    for k, v in model.named_parameters():
        assert v.grad is not None, k
        close(v.grad, R.f64(ref[k]), E2E * max(1e-12, float(ref[k].abs().max())), k)


@pytest.mark.parametrize("N", R.MODULE_ROWS)
@pytest.mark.parametrize("A,D,K,hidden", R.MODULE_SHAPES)
def test_llfq_module_gradients_against_float64_autograd(oracle, A, D, K, hidden, N):
    """All 14 parameter gradients of 3 * loss at training-step batches, to_latent.ci with clamped and unclamped rows."""
    from lipvq_vae_amd.tokenizer import LLFQVAE_V4
    seed = N + D + hidden
    p = O.make_params(seed, A, D, K, hidden=hidden, oracle=oracle)
    p["to_latent.ci"] = R.mixed_ci(p["to_latent.W"], seed)
    ratio = R.lipschitz_bwd_ref(p["to_latent.W"], p["to_latent.ci"], np.zeros_like(p["to_latent.W"]))[2]
    assert int(((ratio - 1.0).abs() <= R.lipschitz_band(hidden)).sum()) == 0 and 0 < int((ratio < 1).sum()) < D
    model = LLFQVAE_V4(A, D, num_codes=K, hidden_dim=hidden).cuda()
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()})
    xt = torch.from_numpy(O.make_inputs(seed + 2, N, A)).cuda()
    _, loss = model(xt)
    (loss * 3.0).backward()
    _compare_module_grads(model, R.oracle_grads_cpu(model, xt, "llfq", 3.0))


@pytest.mark.parametrize("N", R.MODULE_ROWS)
@pytest.mark.parametrize("A,D,K,hidden", R.MODULE_SHAPES)
def test_vq_module_gradients_against_float64_autograd(A, D, K, hidden, N):
    """All 13 parameter gradients of 3 * loss of the plain VQVAE (its hidden widths are fixed: `hidden` only varies the seed).
    Parameters and inputs are drawn until no ReLU pre-activation of the float64 forward is within RELU_BAND of zero, where fp32 and
    float64 may sit on different sides of the kink (a property of the inputs, decided by the reference alone)."""
    from lipvq_vae_amd.tokenizer import VQVAE
    for attempt in range(50):
        torch.manual_seed(N + D + hidden + 1000 * attempt)
        model = VQVAE(A, D, num_embeddings=K).cuda()
        with torch.no_grad():
            model.embedding.weight.uniform_(0.0, 0.4)
        model.invalidate_caches()
        xt = torch.from_numpy(O.make_inputs(N + D + 100 * attempt, N, A)).cuda()
        _, loss = model(xt)
        ref, info = R.autograd_grads(dict(model.named_parameters()), xt, model.last_indices, "vq", 3.0,
                                     commitment_cost=float(model.commitment_cost))
        if info["relu_margin"] >= R.RELU_BAND:
            break
    else:
        pytest.fail("no draw without a ReLU pre-activation inside RELU_BAND")
    print(f"input draw {attempt}, smallest |ReLU pre-activation| {info['relu_margin']:.3e}")
    (loss * 3.0).backward()
    _compare_module_grads(model, ref)
