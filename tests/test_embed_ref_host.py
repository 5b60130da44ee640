"""CPU: the conditions of tests/embed_ref.py at every class and shape tests/test_gpu_embed_edges.py uses, and the CPU half of
that file's forward check -- the oracle's embedding LayerNorm (oracle/lipvq_oracle.c lq_ref_embed_rows, bit for bit the
kernel's) against float64.

Conditions, not measurements: REF_FACTOR x dev <= DEV_CAP for every tensor of every case (a bound of max(TOL, 4 x dev) only
means something while dev is small), the control class stays at dev <= 1e-6, the inputs are xf_edge_inputs.layernorm_case's,
and the float64 restatement is F.layer_norm autograd (dense rows) and a row-by-row loop (indices, bad indices, ragged N).

The oracle test failed before the LayerNorm centred twice, on exactly these (figures as fractions of the class's float64
max |y|): 'constant' (rows of 3.0) at E = 252 and 1020, N = 5 and 2053, with and without pos -- 6.1e-5 ... 9.8e-5 against
1e-5 (fl(1/E) is inexact, the mean one ulp off, rstd = 316 multiplies the residue) -- and 'plus100' at E = 132, N = 5 with
pos, 1.079e-5 against 1.016e-5.  Now the worst y is 0.29 of its bound.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import embed_ref as R
import xf_edge_inputs as X


def _check_dev(what, dev, control):
    for k, d in dev.items():
        assert np.isfinite(d), (what, k, d)
        assert X.REF_FACTOR * d <= X.DEV_CAP, (what, k, d)
        if control:
            assert d <= X.CONTROL_DEV, (what, k, d)


def _case_devs(case, classes, what):
    row_names = [k for k in R.ROW_OUT + R.ROW_SRC if case["ref"][k] is not None]
    for cls in classes:
        _check_dev(what + (cls,), {k: R.edge_dev(case, k, cls) for k in row_names}, cls == "control")
    _check_dev(what, {k: R.edge_dev(case, k) for k in R.COLUMNS}, False)


@pytest.mark.parametrize("E", R.EDGE_E)
def test_the_yardstick_holds_at_every_edge_case(E):
    seen = set()
    for N in R.EDGE_N:
        for route, with_pos in R.EDGE_ROUTES:
            for classes in X.layernorm_groups(N):
                case = R.edge_case(classes, N, E, route, with_pos)
                assert all(torch.isfinite(case[k]).all() for k in ("src", "w", "bias", "gout"))
                _case_devs(case, classes, ("edge", N, E, route, with_pos))
                seen.update(classes)
                if route == "indexed":                              # a permutation with repeats: a row used twice, a row never used
                    counts = torch.bincount(case["idx"], minlength=N)
                    assert counts.max() == 2 and counts.min() == 0 and int(case["idx"].min()) >= 0 and int(case["idx"].max()) < N
    assert seen == set(X.LAYERNORM_CLASSES)


@pytest.mark.parametrize("E", R.WS_EDGE_E)
def test_the_yardstick_holds_on_the_workspace_route(E):
    N, T = R.WS_EDGE_N, R.WS_EDGE_T
    assert N >= 32768 and N % T != 0
    (classes,) = X.layernorm_groups(N)
    assert classes == X.LAYERNORM_CLASSES
    _case_devs(R.edge_case(classes, N, E, "dense", False, T), classes, ("workspace edge", N, E))


@pytest.mark.parametrize("N,E,with_b", [(5, 132, True), (5, 8, False), (203, 260, True)])
def test_the_inputs_and_the_dense_results_are_layernorm_cases(N, E, with_b):
    """a -> src, b -> pos (B = 1, T = N), gy -> gout; y, rstd, gs -> g_src and g_pos, gw -> g_lnw, gb -> g_lnb."""
    for classes in X.layernorm_groups(N):
        lc = X.layernorm_case(classes, N, E, with_b, False)
        case = R.edge_case(classes, N, E, "dense", with_b)
        for mine, theirs in (("src", "a"), ("pos", "b"), ("w", "w"), ("bias", "bias"), ("gout", "gy")):
            assert (case[mine] is None and lc[theirs] is None) or torch.equal(case[mine], lc[theirs]), mine
        assert case["src_rows"] == lc["rows"]
        for run in ("ref", "f32"):
            tol = 1e-13 if run == "ref" else 0.0
            pairs = [("y", "y"), ("rstd", "rstd"), ("g_src", "gs"), ("g_lnw", "gw"), ("g_lnb", "gb")] + ([("g_pos", "gs")] if with_b else [])
            for mine, theirs in pairs:
                assert X.rel(case[run][mine], lc[run][theirs]) <= tol, (run, mine)


def test_the_restatement_row_by_row():
    """Indices with repeats and two bad ones, ragged N, pos by n % T: each row on its own through F.layer_norm, summed by hand."""
    N, T, K, E = 11, 4, 3, 12
    g = torch.Generator().manual_seed(3)
    table, pos = torch.randn(K, E, generator=g).double(), torch.randn(T, E, generator=g).double()
    w, bias, gout = torch.randn(E, generator=g).double(), torch.randn(E, generator=g).double(), torch.randn(N, E, generator=g).double()
    idx = torch.tensor([0, 2, 2, K, 1, 0, -1, 2, 1, 1, 0])
    got = R.embed_run(table, idx, pos, T, w, bias, gout, torch.float64)
    want = {"g_src": torch.zeros(K, E).double(), "g_pos": torch.zeros(T, E).double(), "g_lnw": torch.zeros(E).double(),
            "g_lnb": torch.zeros(E).double()}
    for n in range(N):
        k = int(idx[n])
        if not 0 <= k < K:
            assert torch.isnan(got["y"][n]).all() and torch.isnan(got["rstd"][n]) and torch.isnan(got["mean"][n])
            continue
        x = (table[k] + pos[n % T]).requires_grad_(True)
        ww, bb = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        y = F.layer_norm(x, (E,), ww, bb, X.LN_EPS)
        (y * gout[n]).sum().backward()
        assert X.rel(got["y"][n], y.detach()) <= 1e-13 and abs(float(got["mean"][n] - x.detach().mean())) <= 1e-13
        want["g_src"][k] += x.grad
        want["g_pos"][n % T] += x.grad
        want["g_lnw"] += ww.grad
        want["g_lnb"] += bb.grad
    for k, v in want.items():
        assert X.rel(got[k], v) <= 1e-13, k
    dense = R.embed_run(table[idx.clamp(0, K - 1)], None, None, T, w, bias, gout, torch.float64)
    assert dense["g_pos"] is None and torch.isfinite(dense["y"]).all()


def test_the_shape_lists_reach_what_they_are_there_for():
    chunk = {nt: R.embed_chunk(nt[0]) for nt in R.STEP_CASES}
    assert [chunk[nt] for nt in R.STEP_CASES] == [1, 2, 2, 3, 8, 16, 16, 2]
    per_pass = {nt: 2048 * 16 * c for nt, c in chunk.items()}       # rows of one grid-stride iteration
    assert per_pass[(40000, 10)] < 40000 and per_pass[(525061, 10)] < 525061
    assert 65573 % (16 * 2) and 525061 % (16 * 16) and 262793 % (16 * 8)          # a ragged last item with chunk > 1
    assert {(E + 255) // 256 for E in R.WIDE_E} == {2, 3, 4} and {(E + 255) // 256 for E in R.EDGE_E} == {1, 2, 3, 4}
    nj = {(E // 4 + 15) // 16 for E in R.EDGE_E}                     # the forward's instances: <= 2, <= 4, <= 8, <= 16 groups per lane
    assert {1, 2, 3, 4, 5, 8, 9, 16} <= nj
    assert R.WS_N >= 32768 and all(R.WS_N % T for _, T, _, _, _ in R.WS_CASES)


# ---------------------------------------------------------------------------------------------------
# the oracle's embedding LayerNorm against float64: the CPU half of the kernel's forward check
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", R.EDGE_E)
def test_oracle_layernorm_meets_the_forward_yardstick(oracle, E):
    results = []
    for N in R.EDGE_N:
        for with_pos in (True, False):
            for classes in X.layernorm_groups(N):
                case = R.edge_case(classes, N, E, "dense", with_pos)
                out = np.empty((1, N, E), np.float32)
                stats = oracle.embed_rows(case["src"].numpy(), None, None if case["pos"] is None else case["pos"].numpy(),
                                          case["w"].numpy(), case["bias"].numpy(), X.LN_EPS, out, N, N * E, E, 0, want_stats=True)
                got = {"y": out[0], "rstd": stats[:, 1]}
                for cls in classes:
                    for k in R.ROW_OUT:
                        results.append(X.report(f"oracle embed {cls} N={N} E={E} pos={with_pos} {k}", R.edge_err(case, k, got[k], cls),
                                                R.edge_dev(case, k, cls), X.FWD_TOL))
    failed = [(what, err, b) for what, err, b in results if not err <= b]
    assert not failed, failed
