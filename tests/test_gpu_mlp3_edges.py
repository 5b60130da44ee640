"""GPU: the stand-alone three-layer stack (lipvq_mlp3_f32, csrc/lipvq_mlp.hip) at the edges of its dispatch and of fp32, every
forward tensor (y, pre0, pre1, pre2) against the canonical oracle with ==.

What runs here and nowhere else in the suite: the hidden widths 160 ... 256 of the header's "multiples of 32, <= 256"; both
sides of the one / two sub-tile switch of launch_mlp3_wg (N >= 4096 and 2 * plane <= 80 KiB); the one-wave-per-tile fallback
mlp3_kernel in the FORWARD direction (K0 >= 971 at hidden (64, 128)), with and without gather_idx; both sides of the 65 536-row
hand-over to mlp3_lds_kernel, and a misaligned packed buffer that must keep the workgroup kernel; outputs that start one
float into their allocation (the scalar side of lq_tile_store16) between guard floats; NaN / inf / 3e38 / denormal / -0.0 rows
at the seams of the 32-row MFMA tiles, with every other row bit-identical to the run without them; lq_gelu / lq_sigmoid / ReLU
on the device at every branch constant of lipvq_math.h; denormal pre-activations; lipvq_mlp3_pack_bwd2_f32 against two
lipvq_mlp3_pack_bwd_f32.

Left out: the fallback's grid-stride pass starts above 262 144 rows (2 048 workgroups x 4 waves x 32 rows); at K0 = 971 that is
a 1 GB input.

Denormals: lipvq_math.h says "denormals kept".  The fp32 MFMA chain on gfx950 keeps them -- inputs, products and sums in the
denormal range equal the oracle's bit for bit in all three kernels (test_denormal_products_equal_the_oracle).
"""
import numpy as np
import pytest
import torch

import seed_kernel_edges as E
from oracle import lipvq_oracle as O
from test_gpu_backward import _check_chain, _mlp3_inputs

pytestmark = pytest.mark.gpu

ENC = (O.ACT_GELU, O.ACT_GELU, O.ACT_SIGMOID)
RELU3 = (O.ACT_RELU, O.ACT_RELU, O.ACT_RELU)
MIX = (O.ACT_RELU, O.ACT_SIGMOID, O.ACT_GELU)
NONE3 = (O.ACT_NONE, O.ACT_NONE, O.ACT_NONE)
LDS_ROWS = 65536                       # LQ_MLP3_LDS_ROWS (csrc/lipvq_mlp.hip)
EUNSUPPORTED = -2                      # LIPVQ_EUNSUPPORTED (include/lipvq.h)
SENTINEL = -7777.25
NAMES = ("y", "pre0", "pre1", "pre2")


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                  # (a copy: the shared reference inputs are read-only)


def _stack(K0, J0, J1, J2, seed, s0=0.5):
    rng = np.random.default_rng(seed)
    W0 = rng.standard_normal((J0, K0)).astype(np.float32) * np.float32(s0)
    W1 = rng.standard_normal((J1, J0)).astype(np.float32) * np.float32(0.2)
    W2 = rng.standard_normal((J2, J1)).astype(np.float32) * np.float32(0.2)
    b0, b1, b2 = (rng.standard_normal(J).astype(np.float32) for J in (J0, J1, J2))
    return W0, b0, W1, b1, W2, b2


def _pack(ops, w):
    return ops.mlp3_pack(*(dev(a) for a in w))


def _run(ops, x, packed, acts, gather_idx=None):
    """[y, pre0, pre1, pre2] as numpy; the run without saved pre-activations must give the same y."""
    xd = dev(x)
    gi = None if gather_idx is None else dev(gather_idx)
    y, pre = ops.mlp3(xd, packed, acts, gather_idx=gi, save_pre=True)
    y2 = ops.mlp3(xd, packed, acts, gather_idx=gi)
    torch.cuda.synchronize()
    assert bool(((y2 == y) | (y2.isnan() & y.isnan())).all()), "y differs between save_pre = True and False"
    return [t.cpu().numpy() for t in [y] + pre]


def _ref(oracle, x, w, acts):
    y, pre = oracle.mlp3(x, *w, acts, save_pre=True)
    return [y] + pre


def _same(got, ref, what, equal_nan=False):
    for g, r, name in zip(got, ref, NAMES):
        assert g.shape == r.shape, (what, name)
        if not np.array_equal(g, r, equal_nan=equal_nan):
            bad = np.argwhere(~((g == r) | (np.isnan(g) & np.isnan(r) if equal_nan else False)))
            i = tuple(bad[0])
            raise AssertionError(f"{what} {name}: {len(bad)} mismatches, first at {list(i)}: got {g[i]!r}, oracle {r[i]!r}")


# ---------------------------------------------------------------------------------------------------------------------------
# hidden widths the header allows
# ---------------------------------------------------------------------------------------------------------------------------
WIDE_PAIRS = [(256, 256), (160, 224), (224, 160), (192, 32), (32, 256), (128, 160)]
# (128, 160) still fits two sub-tiles at N >= 4096: (8 + 288) * 132 * 2 = 78 144 <= 81 920; the wider pairs keep one
WIDTH_CASES = [(33, j0, j1) for j0, j1 in WIDE_PAIRS] + [(4097, 128, 160), (4097, 256, 256)]


@pytest.mark.parametrize("N,J0,J1", WIDTH_CASES)
def test_hidden_widths_forward(ops, oracle, N, J0, J1):
    K0, J2 = 7, 37
    w = _stack(K0, J0, J1, J2, J0 * 3 + J1)
    x = np.random.default_rng(N + J0).standard_normal((N, K0)).astype(np.float32)
    for acts in (ENC, MIX):
        _same(_run(ops, x, _pack(ops, w), acts), _ref(oracle, x, w, acts), f"hidden ({J0}, {J1}) N={N}")


@pytest.mark.parametrize("N,J0,J1", WIDTH_CASES)
def test_hidden_widths_backward(ops, N, J0, J1):
    """The same widths through lipvq_mlp3_bwd_f32, against the float64 reference and budgets of tests/backward_ref.py exactly as
    tests/test_gpu_backward.py applies them (_check_chain)."""
    K0, J2 = 7, 37
    W0, W1, W2, gy, pre, zero_row = _mlp3_inputs(N, K0, J0, J1, J2, MIX, N * 131 + J0 + 3 * J1)
    pk = ops.mlp3_pack_bwd(W0.cuda(), W1.cuda(), W2.cuda())
    out = ops.mlp3_bwd(gy.cuda(), [p.cuda() for p in pre], pk, MIX, want_gx=True)
    torch.cuda.synchronize()
    _check_chain(out, gy, pre, W0, W1, W2, MIX, True, zero_row)


# ---------------------------------------------------------------------------------------------------------------------------
# one / two sub-tiles per workgroup
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K0", [(4095, 7), (4096, 7), (4097, 7), (4097, 118), (4097, 119)])
def test_nsub_switch(ops, oracle, N, K0):
    """Hidden (64, 128): N = 4095 keeps one sub-tile, 4096 / 4097 take two (whole and one-row last workgroup); K0 = 118 is the
    widest input that still takes two ((118 + 192) * 132 * 2 = 81 840 <= 81 920), 119 is padded to 120 and keeps one."""
    w = _stack(K0, 64, 128, 64, K0 + N, s0=0.5 if K0 < 100 else 0.1)
    x = np.random.default_rng(N * 3 + K0).standard_normal((N, K0)).astype(np.float32)
    _same(_run(ops, x, _pack(ops, w), ENC), _ref(oracle, x, w, ENC), f"N={N} K0={K0}")


# ---------------------------------------------------------------------------------------------------------------------------
# the one-wave-per-tile fallback, forward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("K0,J0,J1,acts", [(970, 64, 128, ENC), (971, 64, 128, ENC), (971, 128, 64, RELU3), (1003, 96, 64, MIX)])
def test_forward_fallback_kernel(ops, oracle, K0, J0, J1, acts, gather):
    """launch_mlp3_wg declines above 150 KiB of LDS: (2 ceil(K0 / 2) + J0 + J1) * 132 > 153 600 from K0 = 971 on at hidden
    (64, 128) -- 970 is the last width of the workgroup kernel -- and from 1003 at (96, 64): mlp3_kernel<2, 4>, <4, 2>, <3, 2>."""
    N, J2 = 70, 12
    rng = np.random.default_rng(K0 + J0)
    w = _stack(K0, J0, J1, J2, K0 * 7 + J1, s0=0.05)
    if gather:
        table = rng.standard_normal((50, K0)).astype(np.float32)
        idx = rng.integers(0, 50, N).astype(np.int64)
        idx[0], idx[-1] = 49, 0
        got = _run(ops, table, _pack(ops, w), acts, gather_idx=idx)
        x = table[idx]
    else:
        x = rng.standard_normal((N, K0)).astype(np.float32)
        got = _run(ops, x, _pack(ops, w), acts)
    _same(got, _ref(oracle, x, w, acts), f"K0={K0} hidden ({J0}, {J1}) gather={gather}")


def test_forward_fallback_refuses_widths_without_an_instance(ops):
    """Hidden (160, 128) at K0 = 971: no workgroup plane, no mlp3_kernel<5, 4>: LIPVQ_EUNSUPPORTED, and y is not touched."""
    N, K0, J0, J1, J2 = 70, 971, 160, 128, 12
    pk = _pack(ops, _stack(K0, J0, J1, J2, 1))
    x = torch.zeros(N, K0, device="cuda")
    y = torch.full((N, J2), SENTINEL, device="cuda")
    rc = ops.lib.lipvq_mlp3_f32(x.data_ptr(), None, pk.buf.data_ptr(), y.data_ptr(), None, None, None, N, K0, J0, J1, J2,
                                *ENC, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED and b"no kernel instance" in ops.lib.lipvq_last_error()
    assert bool((y == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------
# hand-over to the LDS-resident kernel at 65 536 rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handover(oracle):
    """One seeded 65 536-row input of the encoder shape and the oracle's answer, shared (read-only) by the hand-over tests."""
    K0 = 7
    w = _stack(K0, 64, 128, 64, 99)
    x = (np.random.default_rng(17).standard_normal((LDS_ROWS, K0)) * 1.5).astype(np.float32)
    x[5] = 40.0
    ref = _ref(oracle, x, w, ENC)
    for a in [x] + ref:
        a.setflags(write=False)
    return w, x, ref


def test_lds_kernel_handover_at_65536_rows(ops, handover):
    """N = 65 535 (mlp3_wg_kernel, two sub-tiles) and N = 65 536 (mlp3_lds_kernel) on the same rows: both equal the oracle, hence
    each other on the first 65 535 rows -- asserted directly as well."""
    w, x, ref = handover
    pk = _pack(ops, w)
    below = _run(ops, x[:LDS_ROWS - 1], pk, ENC)
    at = _run(ops, x, pk, ENC)
    _same(below, [r[:LDS_ROWS - 1] for r in ref], "N=65535")
    _same(at, ref, "N=65536")
    for a, b, name in zip(below, at, NAMES):
        assert np.array_equal(a.view(np.uint32), b[:LDS_ROWS - 1].view(np.uint32)), name


def test_misaligned_packed_buffer_keeps_the_workgroup_kernel(ops, handover):
    """mlp3_lds_kernel copies the packed stack into LDS with 16-byte loads: a packed buffer that starts one float into its
    allocation fails launch_mlp3_lds's alignment test and runs mlp3_wg_kernel -- same bits."""
    w, x, ref = handover
    pk = _pack(ops, w)
    shifted = torch.empty(pk.buf.numel() + 1, device="cuda")[1:]
    shifted.copy_(pk.buf)
    assert shifted.data_ptr() % 16 == 4
    pk2 = type(pk)(shifted, pk.K0, pk.J0, pk.J1, pk.J2)
    got = _run(ops, x, pk2, ENC)
    _same(got, ref, "misaligned packed")
    for a, b, name in zip(got, _run(ops, x, pk, ENC), NAMES):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


def test_other_hidden_widths_stay_on_the_workgroup_kernel_above_65536_rows(ops, oracle):
    """Hidden (96, 64) has no mlp3_lds_kernel instance: N = 65 536 + 45 runs mlp3_wg_kernel with two sub-tiles."""
    N, K0, J2 = LDS_ROWS + 45, 12, 37
    w = _stack(K0, 96, 64, J2, 3)
    x = np.random.default_rng(4).standard_normal((N, K0)).astype(np.float32)
    _same(_run(ops, x, _pack(ops, w), MIX), _ref(oracle, x, w, MIX), "hidden (96, 64)")


# ---------------------------------------------------------------------------------------------------------------------------
# outputs that are not 16-byte aligned
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [45, 4097])
@pytest.mark.parametrize("J2", [1, 3, 5, 33, 63, 64, 65])
def test_misaligned_outputs_between_guards(ops, oracle, N, J2):
    """y, pre0, pre1, pre2 each start ONE float into an over-allocated buffer (the al16 == false side of lq_tile_store16:
    sixteen scalar stores per lane): values equal the oracle, the guard float on either side keeps its sentinel.  J2 = 64 and
    the hidden widths fail only the pointer test, the odd J2 the row-stride test as well."""
    K0, J0, J1 = 7, 64, 128
    w = _stack(K0, J0, J1, J2, J2 + N)
    x = np.random.default_rng(J2 * 5 + N).standard_normal((N, K0)).astype(np.float32)
    pk = _pack(ops, w)
    xd = dev(x)
    bufs = [torch.full((N * J + 2,), SENTINEL, device="cuda") for J in (J2, J0, J1, J2)]
    ptrs = [b.data_ptr() + 4 for b in bufs]
    assert all(p % 16 == 4 for p in ptrs)
    rc = ops.lib.lipvq_mlp3_f32(xd.data_ptr(), None, pk.buf.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ptrs[3], N, K0, J0, J1, J2,
                                *ENC, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, ops.lib.lipvq_last_error()
    got = []
    for b, J in zip(bufs, (J2, J0, J1, J2)):
        h = b.cpu().numpy()
        assert h[0] == np.float32(SENTINEL) and h[-1] == np.float32(SENTINEL), "a guard float was overwritten"
        got.append(h[1:-1].reshape(N, J))
    _same(got, _ref(oracle, x, w, ENC), f"misaligned outputs J2={J2}")


# ---------------------------------------------------------------------------------------------------------------------------
# special values and row independence
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acts,rot", [(ENC, 0), (RELU3, 3)])
@pytest.mark.parametrize("N", [70, 4097, LDS_ROWS + 45])
def test_special_rows_and_row_independence(ops, oracle, N, acts, rot):
    """NaN / inf / +-3e38 / denormal / -0.0 rows at rows 0, 31, 32, 63, 64, N - 1 (and their neighbours) of the 32-row MFMA tiles
    (N = 70: one sub-tile per workgroup, 4097: two, 65 581: mlp3_lds_kernel).  Every row equals the oracle (NaN == NaN in the
    planted rows only); every non-planted row is bit-identical to the oracle AND to the GPU run of the unplanted input."""
    K0 = 7
    x, planted, rows = E.special_rows(N, K0, (0, 31, 32, 63, 64, N - 1), rot=rot)
    w = _stack(K0, 64, 128, 37, 5)
    pk = _pack(ops, w)
    clean = _run(ops, x, pk, acts)
    got = _run(ops, planted, pk, acts)
    ref = _ref(oracle, planted, w, acts)
    keep = np.ones(N, bool)
    keep[list(rows)] = False
    assert keep.sum() == N - len(rows) and len(rows) >= 8
    for g, c, r, name in zip(got, clean, ref, NAMES):
        assert np.array_equal(g[keep].view(np.uint32), r[keep].view(np.uint32)), f"{name}: a non-planted row differs from the oracle"
        assert np.array_equal(g[keep].view(np.uint32), c[keep].view(np.uint32)), f"{name}: a planted row leaked into another row"
        assert np.isfinite(g[keep]).all(), name
    _same([g[~keep] for g in got], [r[~keep] for r in ref], f"planted rows {rows}", equal_nan=True)
    assert any(np.isnan(g[~keep]).any() for g in got) and any(np.isinf(g[~keep]).any() for g in got)


# ---------------------------------------------------------------------------------------------------------------------------
# the device's activations against the host's, at every branch constant
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    s = E.act_sweep()
    s.setflags(write=False)
    return s


@pytest.mark.parametrize("act", [O.ACT_GELU, O.ACT_SIGMOID, O.ACT_RELU, O.ACT_NONE])
@pytest.mark.parametrize("pos", [0, 1, 2])
@pytest.mark.parametrize("kernel", ["wg", "lds", "fallback"])
def test_activations_on_the_device(ops, oracle, sweep, kernel, pos, act):
    """identity_stack routes column 0 through the stack and applies `act` at layer `pos`: column 0 of y is lq_gelu / lq_sigmoid
    / ReLU of the sweep as the HOST evaluates it (oracle.math_probe) -- every threshold of lipvq_math.h with three neighbours
    on either side, +-0, denormals -- in mlp3_wg_kernel, mlp3_lds_kernel (sweep repeated up to 65 536 rows) and the fallback
    mlp3_kernel (K0 = 971).  For +-inf the zero weights give 0 * inf: there the answer is the oracle's stack."""
    K0, J = (971, (64, 128, 5)) if kernel == "fallback" else (7, (64, 128, 64))
    N = LDS_ROWS if kernel == "lds" else sweep.size
    assert sweep.size < LDS_ROWS and (kernel != "wg" or N >= 4096)
    *w, acts = E.identity_stack(pos, act, J, K0)
    got = _run(ops, E.sweep_input(sweep, N, K0), _pack(ops, w), acts)
    ref = _ref(oracle, E.sweep_input(sweep, sweep.size, K0), w, acts)
    ref = [np.resize(r, (N, r.shape[1])) if N != sweep.size else r for r in ref]      # (rows repeat with the sweep's period)
    _same(got, ref, f"{kernel} act {act} at layer {pos}", equal_nan=True)
    fin = np.isfinite(np.resize(sweep, N))
    assert np.array_equal(got[0][fin, 0], np.resize(E.act_reference(oracle, sweep, act), N)[fin])


# ---------------------------------------------------------------------------------------------------------------------------
# denormal pre-activations
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acts", [NONE3, (O.ACT_GELU, O.ACT_RELU, O.ACT_NONE)])
@pytest.mark.parametrize("kernel", ["wg", "lds", "fallback"])
def test_denormal_products_equal_the_oracle(ops, oracle, kernel, acts):
    """Inputs and layer-0 weights of magnitude 1e-20, denormal biases: every product, partial sum and pre-activation of the three
    layers is a denormal (or rounds to one).  lipvq_math.h's contract is "denormals kept": the fp32 MFMA chain must neither
    flush its operands nor its results -- equality with the oracle, which runs with denormals on."""
    K0, J = (971, (64, 128, 5)) if kernel == "fallback" else (7, (64, 128, 64))
    N = LDS_ROWS + 45 if kernel == "lds" else 70
    rng = np.random.default_rng(11)
    W0, b0, W1, b1, W2, b2 = _stack(K0, *J, 21, s0=1e-20 * (7.0 / K0) ** 0.5)     # (sums of K0 products stay near 3e-40)
    b0, b1, b2 = (b * np.float32(1e-41) for b in (b0, b1, b2))
    w = (W0, b0, W1, b1, W2, b2)
    x = (rng.standard_normal((N, K0)) * 1e-20).astype(np.float32)
    ref = _ref(oracle, x, w, acts)
    tiny = np.float32(2.0 ** -126)
    for r, name in zip(ref[1:], NAMES[1:]):                  # the case is what it claims: denormal, mostly non-zero pre-activations
        assert (np.abs(r) < tiny).all() and (r != 0).mean() > 0.9, name
    _same(_run(ops, x, _pack(ops, w), acts), ref, f"denormal {kernel}")


# ---------------------------------------------------------------------------------------------------------------------------
# two backward packings in one launch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [((7, 64, 128, 64), (64, 64, 128, 7)), ((12, 96, 64, 37), (37, 32, 256, 5)),
                                 ((208, 128, 64, 1), (1, 256, 32, 208))])
def test_pack_bwd2_equals_two_pack_bwd(ops, a, b):
    """(K0, J0, J1, J2) of two stacks: lipvq_mlp3_pack_bwd2_f32's two buffers equal two lipvq_mlp3_pack_bwd_f32 launches bit for
    bit (the encoder / decoder pair of the tokenizer, and pairs whose hidden widths differ per stack)."""
    g = torch.Generator(device="cuda").manual_seed(a[0] + b[0])
    Ws = [[torch.randn(s, device="cuda", generator=g) for s in ((J0, K0), (J1, J0), (J2, J1))] for K0, J0, J1, J2 in (a, b)]
    pa, pb = ops.mlp3_pack_bwd2(Ws[0], Ws[1])
    for got, W in ((pa, Ws[0]), (pb, Ws[1])):
        one = ops.mlp3_pack_bwd(*W)
        assert (got.K0, got.J0, got.J1, got.J2) == (one.K0, one.J0, one.J1, one.J2)
        assert torch.equal(got.buf.view(torch.int32), one.buf.view(torch.int32))
