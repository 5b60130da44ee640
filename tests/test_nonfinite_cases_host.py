"""CPU: the case file of the non-finite tracer tests (tests/nonfinite_cases.py) checked against itself -- the cones, the strict
restatements against stock torch on clean inputs, a judge that rejects a swallow, a leak and a one-ulp move and accepts the stock
fp32 restatement -- and the C oracle's ReLU stack against the torch restatement on rows that hold NaN / +-inf."""
import numpy as np
import pytest
import torch

import backward_ref as R
import nonfinite_cases as C
from oracle import lipvq_oracle as O

GROUPS = C.groups()
IDS = [g.name for g in GROUPS]


def _first(mask):
    return tuple(np.argwhere(mask)[0])


@pytest.mark.parametrize("group", GROUPS, ids=IDS)
def test_cones(group):
    for case in group.cases():
        a = case.analysis
        n_strict = n_outside = 0
        for k in a["strict"]:
            s, l = a["strict"][k], a["loose"][k]
            assert bool((l | ~s).all()), f"{case.name} {k}: the strict cone leaves the loose one"
            if not group.masked:
                assert torch.equal(s, l), f"{case.name} {k}: one formulation, two cones"
            n_strict += int(s.sum())
            n_outside += int((~l).sum())
        assert n_strict > 0, f"{case.name}: nothing inside the strict cone"
        assert n_outside > 0, f"{case.name}: nothing outside the loose cone"


@pytest.mark.parametrize("group", [g for g in GROUPS if g.op in ("gpt_attention", "gpt_attention_prefix")], ids=lambda g: g.name)
def test_attention_in_between_zone_is_one_batch_head_pair(group):
    """What stock torch's 0 * NaN reaches beyond the mathematical dependence lies inside the planted (b, h): <= 1 / (B H) of out."""
    B, H = C.GPT_ATT_B, C.GPT_ATT_H
    for case in group.cases():
        a = case.analysis
        for k in ("out", "gqkv"):
            if k not in a["strict"]:
                continue
            between = a["loose"][k] & ~a["strict"][k]
            assert int(between.sum()) <= between.numel() // (B * H), (case.name, k, int(between.sum()))
            if between.any() and k == "out":
                L, E = between.shape[1:]
                per = between.view(B, L, H, E // H).any(-1).any(1)           # [B, H]
                assert int(per.sum()) == 1, (case.name, per)


@pytest.mark.parametrize("group", [g for g in GROUPS if g.masked], ids=lambda g: g.name)
def test_strict_formulation_equals_stock_torch_on_clean_inputs(group):
    c = group.clean
    for k in c["strict"]:
        err = C.X.rel(c["strict"][k].numpy(), c["loose"][k].numpy())
        assert err <= 1e-12, (group.name, k, err)


def _wrong_outputs(case, got):
    """(swallow, leak, ulp): the accepted stock-fp32 result `got` with ONE element changed -- an in-cone non-finite value set to 0,
    an element outside the loose cone made NaN, the same element moved by one ulp; None where the case has no such element"""
    a = case.analysis
    swallow = leak = ulp = None
    for k in a["strict"]:
        nonfin = a["strict"][k] & ~a["ref_strict"][k].isfinite()
        if swallow is None and nonfin.any():
            swallow = {**got, k: got[k].clone()}
            swallow[k][_first(nonfin.numpy())] = 0.0
        outside = ~a["loose"][k]
        if leak is None and outside.any():
            i = _first(outside.numpy())
            leak, ulp = {**got, k: got[k].clone()}, {**got, k: got[k].clone()}
            leak[k][i] = float("nan")
            ulp[k][i] = torch.nextafter(got[k][i], torch.tensor(float("inf")))
    return swallow, leak, ulp


@pytest.mark.parametrize("group", GROUPS, ids=IDS)
def test_judge_accepts_stock_fp32_and_rejects_a_swallow_a_leak_and_an_ulp(group):
    seen = [0, 0, 0]
    cases = group.cases()
    if sum(v.numel() for v in group.clean["strict"].values()) > 1 << 20:
        cases = cases[:len(group.values)]              # (the large shapes: the first plant's values; the arithmetic is per element)
    for case in cases:
        got, clean_got = case.stock_fp32()
        assert C.judge(got, clean_got, case) == case.cone_sizes()
        for n, wrong in enumerate(_wrong_outputs(case, got)):
            if wrong is not None and not seen[n]:
                seen[n] += 1
                with pytest.raises(AssertionError):
                    C.judge(wrong, clean_got, case)
    assert all(seen), f"{group.name}: (swallow, leak, ulp) variants built: {seen}"


def test_judge_sign_of_infinity():
    group = [g for g in GROUPS if g.op == "linear" and g.params["act"] == R.ACT_NONE][0]
    case = [c for c in group.cases() if c.key == "b" and c.value_name == "+inf"][0]
    got, clean_got = case.stock_fp32()
    C.judge(got, clean_got, case)
    for value, ok in ((float("nan"), True), (float("-inf"), False), (3.0e38, False)):
        y = got["y"].clone()
        y[0, 128] = value
        if ok:
            C.judge({"y": y}, clean_got, case)
        else:
            with pytest.raises(AssertionError):
                C.judge({"y": y}, clean_got, case)


@pytest.fixture(scope="module")
def oracle():
    return O.CanonicalOracle()


@pytest.mark.parametrize("N", [70])
def test_oracle_relu_stack_has_the_restatements_finiteness_map(oracle, N):
    """The C oracle's mlp3 with the ReLU triple on rows that hold NaN / +-inf: forward (y and the pre-activations) and backward
    (the three layer gradients and gx) are finite exactly where the torch restatement is."""
    group = [g for g in C.groups("mlp3") if g.name == f"mlp3 N={N} relu"][0]
    acts = C.MLP3_TRIPLES["relu"]
    gy = torch.randn(N, C.MLP3_WIDTHS[3], generator=C._gen("oracle gy"))
    shown = 0
    for case in group.cases():
        t = case.planted()
        w = [t[k].numpy() for k in ("W0", "b0", "W1", "b1", "W2", "b2")]
        y, pre = oracle.mlp3(t["x"].numpy(), *w, acts, save_pre=True)
        t64 = C._to(t, torch.float64)
        x64 = t64["x"].clone().requires_grad_(True)
        ws = {k: t64[k].clone().requires_grad_(True) for k in ("W0", "W1", "W2")}
        ref = C.mlp3_ref({**t64, **ws, "x": x64}, False, acts)
        for r in (ref["pre0"], ref["pre1"], ref["pre2"]):
            r.retain_grad()
        (ref["y"] * gy.double()).sum().backward()
        for name, got in (("y", y), ("pre0", pre[0]), ("pre1", pre[1]), ("pre2", pre[2])):
            assert np.array_equal(np.isfinite(got), ref[name].detach().isfinite().numpy()), (case.name, name)
            assert np.array_equal(np.isnan(got), ref[name].detach().isnan().numpy()), (case.name, name)
        g = oracle.mlp3_bwd(t["x"].numpy(), w[0], w[2], w[4], pre, gy.numpy(), acts)
        want = {"W0": ws["W0"].grad, "W1": ws["W1"].grad, "W2": ws["W2"].grad, "x": x64.grad}
        assert set(want) <= set(g), sorted(g)
        for name, r in want.items():
            assert np.array_equal(np.isfinite(np.asarray(g[name])), r.isfinite().numpy()), (case.name, name)
        shown += int(not np.isfinite(y).all())
    assert shown >= 4                                   # (a NaN input reaches y: the ReLU does not swallow it)
