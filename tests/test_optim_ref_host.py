"""CPU: the conditions of the policy update's yardsticks (tests/optim_ref.py), the library's argument refusals, and the loud
refusal of CPU parameters.  The GPU comparisons are tests/test_gpu_policy_update.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import bin_ref as B
import optim_ref as R

import lipvq_vae_amd  # noqa: F401
from lipvq_vae_amd import _capi, optim


def test_cases_clip_and_do_not_clip_and_stay_off_the_corner():
    """Over the steps, the cases of the GPU tests show clip_coef < 1 and clip_coef == 1, and the unclamped ratio is never within
    1e-3 of the corner at 1: a rounding difference between two implementations cannot flip the branch."""
    sizes = B.adamw_sizes(33)
    seen = set()
    for regime in R.CLIP_REGIMES:
        for max_norm in R.MAX_NORMS:
            for step in range(B.ADAMW_STEPS):
                ratio = R.clip_ratio(regime, sizes, step, max_norm)
                assert abs(ratio - 1.0) > 1e-3, (regime, max_norm, step, ratio)
                stats, _ = R.clip_yardstick(R.grads_at(regime, sizes, step), max_norm)
                # the two statements of the rule agree to what torch's own float64 sums can lose: numel additions of 2^-53 each
                for got, want in zip(R.stats_at(regime, sizes, step, max_norm), stats):
                    assert abs(got - want) <= sum(sizes) * R.EPS52 * abs(want)
                seen.add((regime, max_norm, stats[1] < 1.0))
    assert {s[2] for s in seen} == {True, False}
    for max_norm in R.MAX_NORMS:                                       # and each max_norm sees both
        assert {s[2] for s in seen if s[1] == max_norm} == {True, False}
    assert set(R.CLIP_REGIMES) == set(B.ADAMW_REGIMES)


def test_yardstick_reports_what_the_reference_loop_reports():
    grads = R.grads_at("randn_decades", B.adamw_sizes(33), 3)
    stats, clipped = R.clip_yardstick(grads, 1.0)
    assert stats[1] < 1.0 and abs(stats[3] - stats[1] ** 2 * stats[2]) <= sum(B.adamw_sizes(33)) * R.EPS52 * stats[3]
    assert abs(math.sqrt(stats[3]) - 1.0) < 1e-6                       # clipped to max_norm
    assert sum(g is None for g in R.grads_at("randn_decades", B.adamw_sizes(33), 1)) > 0
    s, n = R.sumsq_f64(grads)
    assert n == sum(B.adamw_sizes(33)) and abs(s - stats[2]) <= n * R.EPS52 * s


def test_library_refuses_bad_arguments_without_a_gpu():
    lib = _capi.lib
    one = (C.c_void_p * 1)(16)
    none = (C.c_void_p * 1)(None)
    n1, n0 = (C.c_int64 * 1)(4), (C.c_int64 * 1)(0)
    err = lambda: lib.lipvq_last_error()
    assert lib.lipvq_grad_sumsq_workspace_bytes(65) == 65 * 64 * 8 and lib.lipvq_grad_sumsq_workspace_bytes(0) == 0
    # sum of squares: null lists, count outside 1..32, an empty tensor, a null tensor, no workspace, slots outside the workspace
    assert lib.lipvq_grad_sumsq_f32(None, n1, 1, 0, 1, 16, None) == -1 and b"null" in err()
    assert lib.lipvq_grad_sumsq_f32(one, None, 1, 0, 1, 16, None) == -1
    assert lib.lipvq_grad_sumsq_f32(one, n1, 0, 0, 1, 16, None) == -1 and b"1..32" in err()
    assert lib.lipvq_grad_sumsq_f32(one, n1, 33, 0, 64, 16, None) == -1 and b"1..32" in err()
    assert lib.lipvq_grad_sumsq_f32(one, n0, 1, 0, 1, 16, None) == -1 and b"no elements" in err()
    assert lib.lipvq_grad_sumsq_f32(none, n1, 1, 0, 1, 16, None) == -1
    assert lib.lipvq_grad_sumsq_f32(one, n1, 1, 0, 1, None, None) == -1 and b"workspace" in err()
    assert lib.lipvq_grad_sumsq_f32(one, n1, 1, 1, 1, 16, None) == -1 and b"workspace" in err()
    assert lib.lipvq_grad_sumsq_f32(one, n1, 1, -1, 1, 16, None) == -1
    # coefficient: negative or NaN max_norm, no workspace, no stats
    assert lib.lipvq_clip_coef_f64(16, 1, -1.0, 16, None) == -1 and b"max_norm" in err()
    assert lib.lipvq_clip_coef_f64(16, 1, float("nan"), 16, None) == -1 and b"max_norm" in err()
    assert lib.lipvq_clip_coef_f64(None, 1, 1.0, 16, None) == -1 and b"workspace" in err()
    assert lib.lipvq_clip_coef_f64(16, 1, 1.0, None, None) == -1
    assert lib.lipvq_clip_coef_f64(16, 0, 1.0, 16, None) == -1
    # scale
    assert lib.lipvq_grad_scale_f32(None, n1, 1, 16, None) == -1
    assert lib.lipvq_grad_scale_f32(one, n1, 33, 16, None) == -1 and b"1..32" in err()
    assert lib.lipvq_grad_scale_f32(one, n0, 1, 16, None) == -1
    assert lib.lipvq_grad_scale_f32(one, n1, 1, None, None) == -1
    # Adam
    adam = lambda *a: lib.lipvq_adam_f32(*a)
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert adam(None, one, one, one, one, n1, 1, *hp, 0, None, None, 16, None) == -1 and b"null" in err()
    assert adam(one, one, one, one, one, None, 1, *hp, 0, None, None, 16, None) == -1
    assert adam(one, one, one, one, one, n1, 0, *hp, 0, None, None, 16, None) == -1 and b"1..32" in err()
    assert adam(one, one, one, one, one, n1, 33, *hp, 0, None, None, 16, None) == -1 and b"1..32" in err()
    assert adam(one, one, one, one, one, n0, 1, *hp, 0, None, None, 16, None) == -1 and b"no elements" in err()
    assert adam(one, none, one, one, one, n1, 1, *hp, 0, None, None, 16, None) == -1
    assert adam(one, one, one, one, one, n1, 1, *hp, 0, None, None, None, None) == -1 and b"workspace" in err()
    assert adam(one, one, one, one, one, n1, 1, *hp, 2, None, None, 16, None) == -1 and b"decoupled" in err()


@pytest.mark.parametrize("cls", ("Adam", "AdamW"))
def test_cpu_parameters_are_refused_at_step(cls):
    p = torch.nn.Parameter(torch.zeros(8))
    opt = getattr(optim, cls)([p], lr=1e-3, max_grad_norm=1.0)
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="CUDA"):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(8)) and len(opt.state[p]) == 0
    with pytest.raises(RuntimeError, match="CUDA"):
        optim.clip_grad_norm_([p], 1.0)
    assert torch.equal(p.grad, torch.ones(8))


def test_constructor_refusals_and_state_layout():
    p = torch.nn.Parameter(torch.zeros(8))
    for cls in (optim.Adam, optim.AdamW):
        with pytest.raises(ValueError):
            cls([p], amsgrad=True)
        with pytest.raises(ValueError):
            cls([p], maximize=True)
        with pytest.raises(ValueError):
            cls([p], max_grad_norm=-1.0)
        with pytest.raises(ValueError):
            cls([p], max_grad_norm=float("nan"))
        opt = cls([p])
        assert opt.max_grad_norm is None and opt.grad_stats is None and opt.param_groups[0]["capturable"] is True
    assert isinstance(optim.Adam([p]), torch.optim.Adam) and optim.Adam([p]).param_groups[0]["weight_decay"] == 0
    assert optim.AdamW([p]).param_groups[0]["weight_decay"] == 1e-2
    # state_dict() interchanges with a stock capturable Adam
    stock = torch.optim.Adam([p], capturable=True)
    ours = optim.Adam([p], lr=3e-4, weight_decay=1e-4)
    stock.load_state_dict(ours.state_dict())
    ours.load_state_dict(stock.state_dict())
    assert ours.param_groups[0]["lr"] == 3e-4
