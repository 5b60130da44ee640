"""CPU: the input classes and the yardstick of tests/xf_edge_inputs.py, at every class and shape tests/test_gpu_xf_edges.py uses.

Condition, not measurement: a bound of max(TOL, 4 x dev) only means something while dev is small, so here 4 x dev <= DEV_CAP
(2e-3) for every tensor of every case, and the plain-randn control stays at dev <= 1e-6.  And each generator must really
produce its edge: a 'peaked' case whose scores do not spread, or a 'constant' row that is not constant, would test nothing.
"""
import math

import numpy as np
import pytest
import torch

import xf_edge_inputs as X


def _check_dev(what, dev, control):
    for k, d in dev.items():
        assert np.isfinite(d), (what, k, d)
        assert X.REF_FACTOR * d <= X.DEV_CAP, (what, k, d)
        if control:
            assert d <= X.CONTROL_DEV, (what, k, d)


def _attention_edges(cls, case, B, L, H, dh, causal, drop):
    ref, sc = case["ref"], case["ref"]["scores"]
    finite = sc > -1e300
    assert all(torch.isfinite(case[k]).all() for k in ("qkv", "gout")) and all(torch.isfinite(ref[k]).all() for k in ("out", "gqkv", "lse", "delta"))
    spread = (sc.masked_fill(~finite, -1e300).amax(-1) - sc.masked_fill(~finite, 1e300).amin(-1)).max()
    if cls == "control":
        assert ref["score_max"] < 8.0
    if cls in ("peaked4", "peaked16") and L >= 31:
        assert spread > 40.0, spread
    if cls == "peaked16" and L >= 31:
        assert spread > 640.0, spread
    if cls == "offset":                                             # the scores sit around 16 sqrt(dh), not around 0
        assert sc[finite].mean() > 8.0 * math.sqrt(dh), sc[finite].mean()
    if cls == "uniform":
        assert ref["score_max"] == 0.0
    if cls == "dominant":
        p = torch.softmax(sc, -1)
        for b, h, i, j in X.dominant_pairs(B, L, H):
            assert j <= i and p[b, h, i, j] >= 1.0 - 2.0 ** -25, (b, h, i, j, float(p[b, h, i, j]))      # one-hot to fp32
    if cls == "far_apart" and L >= 31:                              # exp(s - m) of some open key is below the smallest fp32 denormal
        assert (sc.masked_fill(~finite, 0.0) - sc.amax(-1, keepdim=True)).min() < -104.0
    if drop:
        keep = case["keep"]
        for b, h, row, col in X.dropped_rows(B, L, H):
            assert keep[b, h, row].sum() == 0 and keep[b, h, :, col].sum() == 0
        assert L < 31 or 0.02 < keep.float().mean() < 0.2


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dh", X.GPT_DH)
def test_batched_attention_classes(dh, causal):
    B, H = X.GPT_B, X.GPT_H
    for L in X.GPT_L:
        for cls in X.ATTENTION_CLASSES:
            for drop in (False, True):
                case = X.attention_case(cls, B, L, H, dh, causal, drop)
                _check_dev(("gpt", cls, dh, L, causal, drop), case["dev"], cls == "control")
                _attention_edges(cls, case, B, L, H, dh, causal, drop)


@pytest.mark.parametrize("D,H", X.XF_DH_HEADS)
def test_unbatched_attention_classes(D, H):
    for S in X.XF_S:
        for cls in X.ATTENTION_CLASSES:
            for drop in (False, True):
                case = X.attention_case(cls, 1, S, H, D // H, False, drop)
                _check_dev(("xf", cls, D, H, S, drop), case["dev"], cls == "control")
                _attention_edges(cls, case, 1, S, H, D // H, False, drop)


def test_unbatched_reference_is_the_default_branch_tests_reference():
    """The unbatched yardstick runs gpt_ref.attention_ref on a batch of one; in float64 that is test_gpu_default._attention_ref."""
    from test_gpu_default import _attention_ref
    for (D, H), S in zip(X.XF_DH_HEADS, (17, 65, 15, 130)):
        for drop in (False, True):
            case = X.attention_case("peaked4", 1, S, H, D // H, False, drop)
            keep = case["keep"][0] if drop else None
            want = _attention_ref(case["qkv"][0].double(), H, keep, case["keep_prob"])
            assert X.rel(case["ref"]["out"][0], want) <= 1e-13


@pytest.mark.parametrize("E", X.LN_E)
def test_layernorm_classes(E):
    seen = set()
    for N in X.LN_N:
        for with_b, _, with_gres in X.LN_VARIANTS:
            for classes in X.layernorm_groups(N):
                case = X.layernorm_case(classes, N, E, with_b, with_gres)
                assert sorted((sl.start, sl.stop) for sl in case["rows"].values())[-1][1] == N
                for cls in classes:
                    seen.add(cls)
                    dev = {k: X.layernorm_dev(case, k, cls) for k in X.ROW_TENSORS}
                    _check_dev(("layernorm", cls, N, E, with_b, with_gres), dev, cls == "control")
                    _layernorm_edges(cls, case, E, with_b)
                _check_dev(("layernorm", classes, N, E), {k: X.layernorm_dev(case, k) for k in X.COLUMN_TENSORS}, False)
    assert seen == set(X.LAYERNORM_CLASSES)


def _layernorm_edges(cls, case, E, with_b):
    sl = case["rows"][cls]
    a, b = case["a"][sl], case["b"][sl] if with_b else None
    s = a + b if with_b else a                                      # fp32, what the kernel forms
    assert sl.stop > sl.start and torch.isfinite(s).all()
    mean, std = s.double().mean(-1), s.double().std(-1, unbiased=False)
    if cls == "control":
        assert (mean.abs() < 5.0).all() and (std > 0.05).all()
    if cls in ("plus100", "plus1000"):
        c = 100.0 if cls == "plus100" else (1000.0 if E > 4 else 200.0)
        assert ((mean - c).abs() < 5.0).all() and (std < 5.0).all()
    if cls == "tiny":
        assert (std ** 2 < X.LN_EPS).all() and (std > 0).all()
    if cls == "underflow":
        assert (s.double() ** 2 < 2.0 ** -126).all() and (s != 0).any()
    if cls == "huge":
        assert (s.double() ** 2).sum(-1).max() < 1e36 and s.abs().max() > 1e14
    if cls == "constant":
        assert (s == X.CONSTANT_VALUE).all()
        assert torch.equal(case["ref"]["xhat"][sl], torch.zeros_like(case["ref"]["xhat"][sl]))
    if cls == "onehot":
        assert ((s == X.ONEHOT_VALUE).sum(-1) == 1).all() and ((s == 0).sum(-1) == E - 1).all()
    if cls == "halves":
        assert (s.double().sum(-1) == 0).all() and (s.abs() == X.HALVES_VALUE).all()
    if cls == "cancel":
        assert s.abs().max() < 0.01
        if with_b:
            assert (a + b).abs().max() < 0.05 * a.abs().max()


def test_the_cap_decides_only_where_fp32_must_drift():
    """Where the bound leaves the fixed tolerances, it does so because of the inputs: the control class never moves it."""
    case = X.attention_case("control", X.GPT_B, 128, X.GPT_H, 64, True, False)
    assert X.bound(X.FWD_TOL, case["dev"]["out"]) == X.FWD_TOL and X.bound(X.BWD_TOL, case["dev"]["gqkv"]) == X.BWD_TOL
    case = X.layernorm_case(("control",), 5, 1024, True, True)
    assert all(X.bound(X.FWD_TOL, X.layernorm_dev(case, k, "control")) == X.FWD_TOL for k in X.ROW_TENSORS)
