"""CPU: the builders of tests/seed_kernel_edges.py produce what they claim, judged by the canonical oracle -- the
reference-side facts the GPU edge tests of the seed kernels rely on (row independence of the stack, the identity stack's
column 0, root ties, probe positions, the activation sweep's constants)."""
import re

import numpy as np
import pytest

import seed_kernel_edges as E
from oracle import lipvq_oracle as O

ENC = (O.ACT_GELU, O.ACT_GELU, O.ACT_SIGMOID)
RELU3 = (O.ACT_RELU, O.ACT_RELU, O.ACT_RELU)


def _stack(K0, J0, J1, J2, seed):
    rng = np.random.default_rng(seed)
    W0 = rng.standard_normal((J0, K0)).astype(np.float32) * 0.5
    W1 = rng.standard_normal((J1, J0)).astype(np.float32) * 0.2
    W2 = rng.standard_normal((J2, J1)).astype(np.float32) * 0.2
    b0, b1, b2 = (rng.standard_normal(J).astype(np.float32) for J in (J0, J1, J2))
    return W0, b0, W1, b1, W2, b2


@pytest.mark.parametrize("N", [70, 4097])
@pytest.mark.parametrize("acts", [ENC, RELU3])
def test_special_rows_plant_every_class_and_leave_the_other_rows_alone(oracle, N, acts):
    K0 = 7
    pos = (0, 31, 32, 63, 64, N - 1)
    for rot in (0, 3):
        x, planted, rows = E.special_rows(N, K0, pos, rot=rot)
        assert set(pos) <= set(rows) and set(rows.values()) == set(E.SPECIAL_CLASSES)
        keep = np.array([r not in rows for r in range(N)])
        assert np.isfinite(x).all() and np.array_equal(x[keep], planted[keep])
        for r, cls in rows.items():
            row = planted[r]
            want = {"nan_row": np.isnan(row).all(), "nan_elem": np.isnan(row).sum() == 1, "pos_inf": (row == np.inf).all(),
                    "neg_inf": (row == -np.inf).all(), "pos_3e38": (row == np.float32(3e38)).all(),
                    "neg_3e38": (row == np.float32(-3e38)).all(),
                    "denormal": ((row > 0) & (row < np.float32(2.0 ** -126))).all(),
                    "neg_zero": ((row == 0) & np.signbit(row)).all()}[cls]
            assert want, (r, cls)
        # every 32-row tile that holds a planted row also holds rows that are not (but a last tile of one or two rows)
        for t in {r // 32 for r in rows}:
            assert keep[32 * t:32 * t + 32].any() or N - 32 * t <= 2
        # reference-side row independence: the oracle's rows of the unplanted input, bit for bit
        w = _stack(K0, 64, 128, 37, 5)
        y0, pre0 = oracle.mlp3(x, *w, acts, save_pre=True)
        y1, pre1 = oracle.mlp3(planted, *w, acts, save_pre=True)
        for a, b in zip([y0] + pre0, [y1] + pre1):
            assert np.array_equal(a[keep].view(np.uint32), b[keep].view(np.uint32))
        # ... and the planted rows do change something (3e38 overflows the first layer's chain)
        r38 = [r for r, c in rows.items() if c == "pos_3e38"][0]
        assert not np.isfinite(pre1[0][r38]).all()


def test_act_sweep_reads_every_branch_constant_from_the_header():
    consts = E.branch_constants()
    for fn in ("lq_gelu", "lq_sigmoid", "lq_expf", "lq_softplus"):
        assert consts[fn], fn
    # a function of the header that compares against a float literal and is not swept: the list in seed_kernel_edges.py is stale
    text = E.MATH_H.read_text()
    for name in re.findall(r"LQ_HD\s+float\s+(\w+)\s*\(", text):
        body = E._function_body(text, name)
        if E._CMP.search(body):
            assert name in E.BRANCHING_FUNCTIONS, f"{name} branches on a float constant that act_sweep() does not cover"
    s = E.act_sweep()
    assert s.dtype == np.float32 and not np.isnan(s).any()
    have = set(s.view(np.uint32).tolist())
    for fn, cs in consts.items():
        for c in cs:
            for v in (c, -c):
                f = np.float32(v)
                nb = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
                for _ in range(2):
                    nb += [np.nextafter(nb[-2], np.float32(np.inf)), np.nextafter(nb[-1], np.float32(-np.inf))]
                assert {int(np.float32(q).view(np.uint32)) for q in nb} <= have, (fn, c)
    for v in (0.0, -0.0, 2.0 ** -149, -2.0 ** -149, np.inf, -np.inf, float(E.DENORM_MAX)):
        assert int(np.float32(v).view(np.uint32)) in have
    # both sides of lq_gelu's x * x < 18 hand-over are there
    sq = s.astype(np.float32) * s.astype(np.float32)
    near = np.abs(np.abs(s) - np.sqrt(18.0)) < 1e-5
    assert (sq[near] < 18.0).any() and (sq[near] >= 18.0).any()


@pytest.mark.parametrize("act", [O.ACT_GELU, O.ACT_SIGMOID, O.ACT_RELU, O.ACT_NONE])
@pytest.mark.parametrize("pos", [0, 1, 2])
@pytest.mark.parametrize("K0,J", [(1, (64, 128, 64)), (971, (64, 128, 5))])
def test_identity_stack_returns_the_activation_in_column_0(oracle, pos, act, K0, J):
    s = E.act_sweep()
    x = E.sweep_input(s, s.size, K0)
    *w, acts = E.identity_stack(pos, act, J, K0)
    assert acts[pos] == act and sum(a != O.ACT_NONE for a in acts) <= 1
    y = oracle.mlp3(x, *w, acts)
    fin = np.isfinite(s)
    assert np.array_equal(y[fin, 0], E.act_reference(oracle, s, act)[fin])
    # an infinite input meets the zero weights of layer 0 (0 * inf): NaN in every other feature and, one layer on, in column 0
    # (which a later ReLU turns into 0): for +-inf the answer is the oracle's stack, not the activation alone
    assert (~fin).sum() == 2
    if act != O.ACT_RELU:
        assert np.isnan(y[~fin, 0]).all()


@pytest.mark.parametrize("D", [32, 208, 256, 7])
def test_root_tie_pair_is_a_root_tie(oracle, D):
    z, hi, lo = E.root_tie_pair(D, oracle)
    cb = np.stack([hi, lo])
    s = oracle.distances(z[None], cb, O.DIST_SQSUM)[0]
    v = oracle.distances(z[None], cb, O.DIST_NORM)[0]
    assert s[0] > s[1] and v[0] == v[1]
    assert oracle.nearest(z[None], cb, O.DIST_NORM)[0][0] == 0
    assert oracle.nearest(z[None], cb, O.DIST_SQSUM)[0][0] == 1
    # with the pair the other way round both rules agree again
    assert oracle.nearest(z[None], cb[::-1].copy(), O.DIST_NORM)[0][0] == 0
    assert oracle.nearest(z[None], cb[::-1].copy(), O.DIST_SQSUM)[0][0] == 0


def test_mse_probe_positions():
    nth = E.MSE_THREADS
    assert nth == 524288
    assert E.mse_probe_positions(1, True) == [0]
    assert E.mse_probe_positions(5, True) == [0, 3, 4]
    assert E.mse_probe_positions(4 * nth, True) == [0, 4 * nth - 1]
    n = 8 * nth + 4003
    p = E.mse_probe_positions(n, True)
    assert p == sorted(set(p)) and all(0 <= q < n for q in p)
    assert {0, n - 1, 4 * (n // 4) - 1, 4 * (n // 4), 4 * nth - 1, 4 * nth, 8 * nth - 1, 8 * nth} == set(p)
    assert n % 4 == 3
    q = E.mse_probe_positions(n, False)
    assert set(p) < set(q) and {nth - 1, nth} <= set(q)


def test_mse_ref_and_ulp():
    a = np.array([1.0, 2.0, 3.0], np.float32)
    b = np.array([1.0, 0.0, 0.0], np.float32)
    assert E.mse_ref(a, b) == 13.0 / 3.0
    assert E.ulp32(1.0) == 2.0 ** -23 and E.ulp32(np.float32(3.0)) == 2.0 ** -22
