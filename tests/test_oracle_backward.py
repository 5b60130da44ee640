"""CPU: the C oracle's gradients (oracle/lipvq_oracle.c: lq_ref_lipschitz_bwd, lq_ref_mlp3_bwd and the whole-path llfq_grads /
vq_grads built from them) against the float64 reference of tests/backward_ref.py.  Several GPU tests compare the HIP kernels
with these oracle gradients, which were written from the same derivation as the kernels: this file pins them to stock torch
ops and autograd.  It also re-measures, on every run, the constants that tests/test_gpu_backward.py derives its budgets from.
No GPU is needed."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import lipvq_oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import backward_ref as R  # noqa: E402
import test_gpu_backward as G  # noqa: E402  (the named constants only; its tests carry the gpu marker)

E2E = 2e-5                       # relative to max|ref|: the project's bound for gradients (test_wgrad_against_float64)


def close(got, ref, allowed, name):
    got = R.f64(got)
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    err = (got - ref).abs()
    allowed = allowed if torch.is_tensor(allowed) else torch.full_like(err, float(allowed))
    bad = err > allowed
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} elements over budget, worst err/allowed "
                           f"{float((err / allowed.clamp(min=1e-300)).max()):.3f}")


def test_measured_constants_hold(oracle):
    """The two delta_act constants of tests/test_gpu_backward.py and backward_ref.LIP_FUNC_REL are what the canonical arithmetic
    measures against float64 on this machine -- not smaller (the budgets would be unsound) and not 10 % larger (they would be loose)."""
    x = np.concatenate([R.act_sweep(), R.PLANTED])
    gelu = float(np.abs(oracle.math_probe(x, 5).astype(np.float64) - R.act_grad_ref(x, R.ACT_GELU).numpy()).max())
    s = oracle.math_probe(x, 3)
    sig = float(np.abs((s * (np.float32(1.0) - s)).astype(np.float64) - R.act_grad_ref(x, R.ACT_SIGMOID).numpy()).max())
    print(f"lq_gelu_grad: {gelu:.4e}, s (1 - s) from lq_sigmoid: {sig:.4e}")
    assert gelu <= G.GELU_GRAD_ABS_ERR <= 1.1 * gelu
    assert sig <= G.SIGMOID_GRAD_ABS_ERR <= 1.1 * sig
    ci = np.linspace(-30, 88, 400001).astype(np.float32)
    c64 = torch.from_numpy(ci).double()
    for fn, exact in ((4, torch.nn.functional.softplus(c64)), (3, torch.sigmoid(c64))):
        rel = float(((torch.from_numpy(oracle.math_probe(ci, fn)).double() - exact).abs() / exact).max())
        assert rel <= R.LIP_FUNC_REL, (fn, rel / R.U32)


@pytest.mark.parametrize("H", R.LIPSCHITZ_H)
@pytest.mark.parametrize("D", R.LIPSCHITZ_D)
def test_lipschitz_cases_leave_out_no_row(D, H):
    """The condition of test_gpu_backward.py::test_lipschitz_bwd_against_float64, checked with the reference alone: no seeded row
    has a float64 ratio within 4 H u of 1, both branches occur from D = 15 on, the rows near the switch are where they should
    be, and the reference itself is finite (all-zero row included)."""
    W, ci, gWn, roles = R.lipschitz_case(D, H, 1000 * D + H)
    gW, gci, ratio = R.lipschitz_bwd_ref(W, ci, gWn)
    assert int(((ratio - 1.0).abs() <= R.lipschitz_band(H)).sum()) == 0
    assert torch.isfinite(gW).all() and torch.isfinite(gci).all()
    if D >= 15:
        assert 0 < int((ratio < 1).sum()) < D
        near = (ratio[roles["near"]] - 1.0).abs()
        assert float(near.max()) <= 1.1e-3 and float(near.min()) >= 1e-5 and float(near.min()) <= 1.3e-4
        assert int((ratio[roles["near"]] < 1).sum()) == 3


@pytest.mark.parametrize("H", R.LIPSCHITZ_H)
@pytest.mark.parametrize("D", R.LIPSCHITZ_D)
def test_oracle_lipschitz_bwd_against_float64(oracle, D, H):
    W, ci, gWn, roles = R.lipschitz_case(D, H, 1000 * D + H)
    ref_gW, ref_gci, ratio = R.lipschitz_bwd_ref(W, ci, gWn)
    active = ratio < 1.0
    gW, gci = (torch.from_numpy(a) for a in oracle.lipschitz_bwd(W, ci, gWn))
    scale, _ = oracle.lipschitz_scale(W, ci)
    assert torch.equal(torch.from_numpy(scale) < 1.0, active) and torch.equal(gci != 0, active)
    d_gW, d_gci = R.lipschitz_budget(W, ci, gWn)
    close(gW[active], ref_gW[active], d_gW[active], "gW")
    close(gci[active], ref_gci[active], d_gci[active], "gci")
    assert torch.equal(gW[~active], torch.from_numpy(gWn)[~active]) and bool((gci[~active] == 0).all())
    if "zero_row" in roles:
        assert not bool(active[roles["zero_row"]])


def _stack_case(N, K0, J0, J1, J2, acts, seed):
    g = torch.Generator().manual_seed(seed)
    W0 = torch.randn(J0, K0, generator=g) * 0.3
    W1 = torch.randn(J1, J0, generator=g) * 0.2
    W2 = torch.randn(J2, J1, generator=g) * 0.2
    x = torch.randn(N, K0, generator=g)
    gy = torch.randn(N, J2, generator=g)
    pre = [torch.randn(N, J, generator=g) * 2.0 for J in (J0, J1, J2)]
    for i, p in enumerate(pre):                                   # +-0 under ReLU, saturated GELU' / sigmoid'
        flat = p.view(-1)
        for k, v in enumerate(R.PLANTED):
            flat[(3 + i + 37 * k) % flat.numel()] = float(v)
    return W0, W1, W2, x, gy, pre


@pytest.mark.parametrize("N", [1, 31, 33, 80])
@pytest.mark.parametrize("K0,J0,J1,J2,acts", [
    (7, 64, 128, 64, (O.ACT_GELU, O.ACT_GELU, O.ACT_SIGMOID)), (37, 64, 128, 7, (O.ACT_GELU, O.ACT_GELU, O.ACT_NONE)),
    (7, 64, 128, 48, (O.ACT_RELU, O.ACT_RELU, O.ACT_RELU)), (12, 32, 96, 5, (O.ACT_RELU, O.ACT_SIGMOID, O.ACT_GELU)),
])
def test_oracle_mlp3_bwd_against_float64(oracle, N, K0, J0, J1, J2, acts):
    """lq_ref_mlp3_bwd (what llfq_grads / vq_grads are built from) at small batches, with pre-activations of exactly +-0 under
    ReLU and saturated ones under GELU / sigmoid."""
    W0, W1, W2, x, gy, pre = _stack_case(N, K0, J0, J1, J2, acts, N + K0 + J2)
    got = oracle.mlp3_bwd(x.numpy(), W0.numpy(), W1.numpy(), W2.numpy(), [p.numpy() for p in pre], gy.numpy(), acts)
    g2, g1, g0, gx = R.mlp3_bwd_ref(gy, pre, W0, W1, W2, acts)
    want = {"x": gx, "W2": g2.t() @ R.act_ref(pre[1], acts[1]), "b2": g2.sum(0), "W1": g1.t() @ R.act_ref(pre[0], acts[0]),
            "b1": g1.sum(0), "W0": g0.t() @ R.f64(x), "b0": g0.sum(0)}
    for k, ref in want.items():
        close(got[k], ref, E2E * max(float(ref.abs().max()), 1e-300), k)
    if acts[0] == O.ACT_RELU:          # (a ReLU' of 1 at +-0 would move b0 / W0 by a whole row's share: far outside the bound above)
        at0 = (pre[0] == 0)
        assert int(at0.sum()) >= 2 and bool((g0[at0] == 0).all())


@pytest.mark.parametrize("N", R.MODULE_ROWS)
@pytest.mark.parametrize("A,D,K,hidden", R.MODULE_SHAPES)
def test_oracle_llfq_grads_against_float64_autograd(oracle, A, D, K, hidden, N):
    seed = N + D + hidden
    p = O.make_params(seed, A, D, K, hidden=hidden, oracle=oracle)
    p["to_latent.ci"] = R.mixed_ci(p["to_latent.W"], seed)
    ratio = R.lipschitz_bwd_ref(p["to_latent.W"], p["to_latent.ci"], np.zeros_like(p["to_latent.W"]))[2]
    assert int(((ratio - 1.0).abs() <= R.lipschitz_band(hidden)).sum()) == 0 and 0 < int((ratio < 1).sum()) < D
    x = O.make_inputs(seed + 2, N, A)
    fwd = oracle.llfq_forward(p, x)
    got = oracle.llfq_grads(p, x, fwd=fwd)
    ref, _ = R.autograd_grads(p, x, fwd["indices"], "llfq", 1.0)
    assert set(got) == set(ref)
    for k in ref:
        close(got[k], ref[k], E2E * max(1e-12, float(ref[k].abs().max())), k)


@pytest.mark.parametrize("N", R.MODULE_ROWS)
@pytest.mark.parametrize("A,D,K,hidden", R.MODULE_SHAPES)
def test_oracle_vq_grads_against_float64_autograd(oracle, A, D, K, hidden, N):
    """Parameters and inputs are drawn until no ReLU pre-activation of the float64 forward is within RELU_BAND of zero (backward_ref.py)."""
    for attempt in range(50):
        p = O.make_params(N + D + hidden + 1000 * attempt, A, D, K, variant="vq", oracle=oracle)
        x = O.make_inputs(N + D + 100 * attempt, N, A)
        fwd = oracle.vq_forward(p, x)
        ref, info = R.autograd_grads(p, x, fwd["indices"], "vq", 1.0)
        if info["relu_margin"] >= R.RELU_BAND:
            break
    else:
        pytest.fail("no input draw without a ReLU pre-activation inside RELU_BAND")
    got = oracle.vq_grads(p, x, fwd=fwd)
    assert set(got) == set(ref)
    for k in ref:
        close(got[k], ref[k], E2E * max(1e-12, float(ref[k].abs().max())), k)
