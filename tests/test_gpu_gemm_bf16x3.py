"""GPU: the bf16x3 mode of the transformer's Linears (csrc/lipvq_gemm_bf16.hip with SPLIT = true; lipvq_linear_act_bf16x3 /
lipvq_linear_nn_bf16x3 / lipvq_wgrad_bf16x3; ops.linear_bf16x3 / linear_nn_bf16x3 / wgrad_bf16x3): forward (NT), input
gradient (NN) and weight gradient (TN), on the shapes of tests/test_gpu_gemm_bf16.py and on every row of
gemm_bf16_cases.INSTANCES, so every tile instance runs at its ragged edges.

References and bounds come from tests/gemm_bf16x3_ref.py, which tests/test_gemm_bf16x3_host.py pins on the CPU:
  1. float64 on the operands split exactly as the kernel splits them (s3), within TWICE the any-order round-to-nearest bound
     over the 3 L terms, (3 L + 1) 2^-24 R3 -- twice, because how the matrix pipe rounds inside a k-step is not documented;
  2. the exact product, within 3 2^-16 (1 + 2^-7) R_exact plus that accumulation bound; for reductions of at most 136 a plain
     bf16 product is outside this bound in more than 75 % of the elements (host test), so a kernel that drops or mis-stages
     lo cannot pass;
  3. exact witnesses: operands of 1 + 2^-9 (hi = 1, lo = 2^-9) give L (1 + 2^-8) in every output under torch.equal, with one
     operand so filled L (1 + 2^-9); all partial sums are exact in fp32 in any order, and a missing, doubled or swapped cross
     term gives another number (plain bf16: L).  For the weight gradient the reduced result is what is observable.
Every ratio is printed before it is asserted.  Measured on an MI355X: DESIGN.md section 4.6.1.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_bf16_cases as C
import gemm_bf16x3_ref as X

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_GELU = 0, 1
EPS = C.EPS


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


@pytest.fixture(scope="module")
def abi():
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    return _capi.lib, _capi.check, lipvq_vae_amd.ops._stream


def _product(ops, layout, x, W, g):
    """The layout's product of the mode, no bias, on the CPU."""
    if layout == "NT":
        return ops.linear_bf16x3(x.cuda(), W.cuda()).cpu()
    if layout == "NN":
        return ops.linear_nn_bf16x3(g.cuda(), W.cuda()).cpu()
    return ops.wgrad_bf16x3(g.cuda(), x.cuda(), want_bias=False)[0].cpu()


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2, 4: the split-operand reference, the exact product, gb
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.all_cases(), ids=X.case_id)
def test_against_split_reference_and_exact_product(ops, case):
    layout, N, K, J = case
    c, r = C.case(N, K, J), X.ref(layout, N, K, J)
    L, tag = r["L"], X.case_id(case)
    xc, Wc, gc = c["x"].cuda(), c["W"].cuda(), c["g"].cuda()
    outs = []                                                                    # (what, got, float64 offset)
    if layout == "NT":
        outs.append(("plain", ops.linear_bf16x3(xc, Wc), 0.0))
        y, pre = ops.linear_bf16x3(xc, Wc, c["b"].cuda(), act=ops.ACT_GELU, save_pre=True)
        outs.append(("bias gelu pre", pre, c["b"].double()))
        ref = F.gelu(pre.cpu().double())
        assert float((y.cpu().double() - ref).abs().max()) <= 1e-5 * max(1e-30, float(ref.abs().max())), tag
    elif layout == "NN":
        outs.append(("gx", ops.linear_nn_bf16x3(gc, Wc), 0.0))
    else:
        gW, gb = ops.wgrad_bf16x3(gc, xc)
        outs.append(("gW", gW, 0.0))
        assert gb.shape == (J,)
        e = (gb.cpu().double() - c["gb"]).abs()
        print(f"{tag} gb: error / (N 2^-24 sum|g|) = {float((e / (N * EPS * c['Rgb'])).max()):.3f}")
        assert bool((e <= N * EPS * c["Rgb"]).all()), tag
        gW2, none = ops.wgrad_bf16x3(gc, xc, want_bias=False)
        assert none is None and torch.equal(gW2, gW), tag
    for what, got, off in outs:
        assert got.shape == r["s3"].shape
        got = got.cpu().double()
        worst = C.ratio(f"{tag} {what}", got, r["s3"] + off, r["R3"], 3 * L)
        d = (got - (r["exact"] + off)).abs()
        bound = X.combined_bound(L, r["R_exact"], r["R3"])
        print(f"{tag} {what}: |got - exact| / combined bound = {float((d / bound.clamp_min(1e-300)).max()):.3f}, "
              f"|got - exact| / R_exact = {float((d / r['R_exact'].clamp_min(1e-300)).max()):.2e}")
        assert worst <= 2.0, (tag, what, worst)
        assert bool((d <= bound).all()), (tag, what)


# ---------------------------------------------------------------------------------------------------------------------------
# 3: exact witnesses at every instance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [(True, True), (True, False), (False, True)], ids=["both", "A", "B"])
@pytest.mark.parametrize("inst", C.INSTANCES, ids=lambda i: i.id)
def test_exact_witnesses(abi, ops, inst, fill):
    M, Nc, L, chunks = C.launch_dims(inst.layout, inst.N, inst.K, inst.J)
    assert abi[0].lipvq_gemm_bf16_tile(M, Nc, chunks) == inst.tile               # the instance under test is the stated one
    x, W, g = X.witness_operands(inst.layout, inst.N, inst.K, inst.J, *fill)
    got = _product(ops, inst.layout, x, W, g)
    want = torch.full((M, Nc), X.witness_value(L, *fill), dtype=torch.float32)
    assert float(want[0, 0]) == X.witness_value(L, *fill)                        # the value is an fp32 number
    if not torch.equal(got, want):
        vals = torch.unique(got)[:8].tolist()
        raise AssertionError(f"{inst.id} fill={fill}: expected {float(want[0, 0])!r} everywhere (plain bf16 would give {L}), "
                             f"got values {vals}")


# ---------------------------------------------------------------------------------------------------------------------------
# 5: guard bands and full coverage of the outputs, through the C ABI (the pattern of tests/test_gpu_gemm_bf16.py)
# ---------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FC0DEAD                   # a NaN with a payload: no arithmetic on finite inputs stores this word
PAD = 1024                              # words (4 KiB) of sentinel before and after every output


class _Fenced:
    """An fp32 output of `shape` in the middle of a sentinel-filled int32 buffer."""

    def __init__(self, what, *shape, offset_words=0):
        self.what, self.n = what, int(np.prod(shape))
        self.buf = torch.full((PAD + offset_words + self.n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.words = self.buf[PAD + offset_words:PAD + offset_words + self.n]
        self.t = self.words.view(torch.float32).view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        lo, hi = self.buf[:self.words.storage_offset()], self.buf[self.words.storage_offset() + self.n:]
        assert lo.numel() >= PAD and hi.numel() >= PAD
        assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), f"{self.what}: a word outside the output was written"
        assert not bool((self.words == SENTINEL).any()), f"{self.what}: an output word was never written"
        return self.t


def _forward(abi, x, W, b, act, with_pre):
    """lipvq_linear_act_bf16x3 into fenced outputs: (y, pre or None) on the CPU, every word written, no guard word touched."""
    lib, check, stream = abi
    (N, K), J = x.shape, W.shape[0]
    xc, Wc, bc = x.cuda(), W.cuda(), None if b is None else b.cuda()
    y, pre = _Fenced("y", N, J, offset_words=1), (_Fenced("pre", N, J, offset_words=3) if with_pre else None)
    check(lib.lipvq_linear_act_bf16x3(xc.data_ptr(), Wc.data_ptr(), None if bc is None else bc.data_ptr(), y.ptr(),
                                      None if pre is None else pre.ptr(), N, K, J, act, stream()), "lipvq_linear_act_bf16x3")
    torch.cuda.synchronize()
    return y.check().cpu(), (None if pre is None else pre.check().cpu())


def _input_gradient(abi, g, W):
    lib, check, stream = abi
    (N, J), K = g.shape, W.shape[1]
    gc, Wc = g.cuda(), W.cuda()
    gx = _Fenced("gx", N, K, offset_words=2)
    check(lib.lipvq_linear_nn_bf16x3(gc.data_ptr(), Wc.data_ptr(), gx.ptr(), N, J, K, stream()), "lipvq_linear_nn_bf16x3")
    torch.cuda.synchronize()
    return gx.check().cpu()


def _weight_gradient(abi, g, x):
    lib, check, stream = abi
    (N, J), K = g.shape, x.shape[1]
    gc, xc = g.cuda(), x.cuda()
    gW, gb = _Fenced("gW", J, K, offset_words=1), _Fenced("gb", J, offset_words=3)
    ws = torch.empty(lib.lipvq_wgrad_bf16_workspace_bytes(N, J, K), dtype=torch.uint8, device="cuda")
    check(lib.lipvq_wgrad_bf16x3(gc.data_ptr(), xc.data_ptr(), gW.ptr(), gb.ptr(), ws.data_ptr(), N, J, K, stream()),
          "lipvq_wgrad_bf16x3")
    torch.cuda.synchronize()
    return gW.check().cpu(), gb.check().cpu()


@pytest.mark.parametrize("K,J", [(72, 24), (512, 136)])
@pytest.mark.parametrize("N", [33, 130])
def test_kernels_write_their_outputs_and_nothing_else(abi, N, K, J):
    c = C.case(N, K, J)
    y, pre = _forward(abi, c["x"], c["W"], c["b"], ACT_GELU, True)
    r = X.ref("NT", N, K, J)
    assert C.ratio(f"fenced pre N={N} K={K} J={J}", pre, r["s3"] + c["b"].double(), r["R3"], 3 * K) <= 2.0
    assert float((y.double() - F.gelu(pre.double())).abs().max()) <= 1e-5 * float((r["s3"] + c["b"].double()).abs().max())
    r = X.ref("NN", N, K, J)
    assert C.ratio(f"fenced gx N={N} K={K} J={J}", _input_gradient(abi, c["g"], c["W"]), r["s3"], r["R3"], 3 * J) <= 2.0
    r = X.ref("TN", N, K, J)
    gW, gb = _weight_gradient(abi, c["g"], c["x"])
    assert C.ratio(f"fenced gW N={N} K={K} J={J}", gW, r["s3"], r["R3"], 3 * N) <= 2.0
    assert bool(((gb.double() - c["gb"]).abs() <= N * EPS * c["Rgb"]).all())


@pytest.mark.parametrize("N,K,J", [(240, 512, 1536), (4100, 64, 64)])
def test_results_repeat_bit_for_bit(ops, N, K, J):
    """(4100, 64, 64): 65 row chunks in the weight gradient, the last one of 4 rows."""
    torch.manual_seed(N + K + J)
    x, W, b, g = (torch.randn(N, K).cuda(), (torch.randn(J, K) / K ** 0.5).cuda(), torch.randn(J).cuda(), torch.randn(N, J).cuda())
    first = (ops.linear_bf16x3(x, W, b), ops.linear_nn_bf16x3(g, W), *ops.wgrad_bf16x3(g, x))
    again = (ops.linear_bf16x3(x, W, b), ops.linear_nn_bf16x3(g, W), *ops.wgrad_bf16x3(g, x))
    for what, p, q in zip(("y", "gx", "gW", "gb"), first, again):
        assert torch.equal(p, q), what
    s3, R3 = X.product3("TN", g.cpu(), x.cpu())                                  # and the chunks add up to the right thing
    assert bool(((first[2].cpu().double() - s3).abs() <= 2 * (3 * N + 1) * EPS * R3).all())
    assert not torch.equal(first[0], ops.linear_bf16(x, W, b))                  # and it is not the bf16 mode's product


# ---------------------------------------------------------------------------------------------------------------------------
# 6: a row does not depend on its position, on the number of rows of the launch or on the tile: bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [ACT_NONE, ACT_GELU], ids=["none", "gelu"])
def test_forward_rows_and_columns_across_tiles(abi, ops, act):
    tile = abi[0].lipvq_gemm_bf16_tile
    c = C.case(1921, 40, 2056)
    x, W, b = c["x"].cuda(), c["W"].cuda(), c["b"].cuda()
    N, J = x.shape[0], W.shape[0]
    full = ops.linear_bf16x3(x, W, b, act=act)
    assert tile(N, J, 1) == 128
    for r0 in (0, 127, 1888):                                                       # 33 rows: tile 32
        assert tile(33, J, 1) == 32
        part = x[r0:r0 + 33]
        assert part.is_contiguous() and part.data_ptr() % 16 == 0                  # a view: no copy is involved
        assert torch.equal(ops.linear_bf16x3(part, W, b, act=act), full[r0:r0 + 33]), r0
    assert tile(1001, J, 1) == 64
    assert torch.equal(ops.linear_bf16x3(x[:1001], W, b, act=act), full[:1001])
    for c0 in (0, 2032):                                                            # 24 rows of W: tile 32, the matching columns
        assert tile(N, 24, 1) == 32
        Wp, bp = W[c0:c0 + 24], b[c0:c0 + 24].contiguous()
        assert Wp.is_contiguous() and Wp.data_ptr() % 16 == 0
        assert torch.equal(ops.linear_bf16x3(x, Wp, bp, act=act), full[:, c0:c0 + 24]), c0


def test_input_gradient_rows_across_tiles(abi, ops):
    tile = abi[0].lipvq_gemm_bf16_tile
    c = C.case(1921, 2056, 40)
    g, W = c["g"].cuda(), c["W"].cuda()                                             # g [1921, 40], W [40, 2056]
    N, K = g.shape[0], W.shape[1]
    full = ops.linear_nn_bf16x3(g, W)
    assert (tile(N, K, 1), tile(1001, K, 1), tile(33, K, 1)) == (128, 64, 32)
    for r0 in (0, 127, 1888):
        part = g[r0:r0 + 33]
        assert part.is_contiguous() and part.data_ptr() % 16 == 0
        assert torch.equal(ops.linear_nn_bf16x3(part, W), full[r0:r0 + 33]), r0
    assert torch.equal(ops.linear_nn_bf16x3(g[:1001], W), full[:1001])


# ---------------------------------------------------------------------------------------------------------------------------
# 7: special values at the seams of the 128 tile
# ---------------------------------------------------------------------------------------------------------------------------
def _run(abi, layout, x, W, b, g):
    """dict name -> output on the CPU, through fenced outputs.  NT: bias + GELU + pre."""
    if layout == "NT":
        y, pre = _forward(abi, x, W, b, ACT_GELU, True)
        return dict(pre=pre, y=y)
    if layout == "NN":
        return dict(gx=_input_gradient(abi, g, W))
    gW, gb = _weight_gradient(abi, g, x)
    return dict(gW=gW, gb=gb)


_unplanted = {}


def _base_run(abi, layout):
    if layout not in _unplanted:
        _unplanted[layout] = _run(abi, layout, *C.special_base(layout))
    return _unplanted[layout]


NON_FINITE = ("nan_elem", "pos_inf_elem", "neg_inf_elem", "flt_max_elem")         # FLT_MAX rounds to +Inf in bf16


@pytest.mark.parametrize("which", [0, 1], ids=["first8", "last"])
@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
def test_special_values_stay_in_their_own_row_or_column(abi, layout, operand, which):
    """One special line per seam of the 128 tile (gemm_bf16_cases.plant): the single planted element sits in the first 8
    reduction indices, with the NaN on line 0 -- the address out-of-range loads of a reduction-contiguous operand are clamped
    to -- or at the LAST reduction index, the row out-of-range loads of a reduction-strided operand are clamped to."""
    N, K, J = C.SPECIAL_SHAPES[layout]
    R = C.launch_dims(layout, N, K, J)[2]
    rot, red = ((0, 3), (3, R - 1))[which]
    x, W, b, g = C.special_base(layout)
    A, B, axa, axb = C.operands(layout, x, W, g)
    if operand == "A":
        pA, where = C.plant(A, axa, red, rot, C.SPECIAL_CLASSES)
        pB = B
    else:
        pB, where = C.plant(B, axb, red, rot, C.SPECIAL_CLASSES)
        pA = A
    if which == 0:
        assert where[0] == "nan_elem"                                               # the NaN sits in the clamp target
    assert set(where.values()) >= set(NON_FINITE) | {"two126_elem", "neg_zero"}
    px, pW, pg = {"NT": (pA, pB, g), "NN": (x, pB, pA), "TN": (pB, W, pA)}[layout]
    want, R3 = X.product3(layout, pA, pB)
    exact, R_exact = X.product_exact(layout, pA, pB)
    if layout == "NT":
        want, exact = want + b.double(), exact + b.double()
    base, got = _base_run(abi, layout), _run(abi, layout, px, pW, b, pg)
    tag = f"{layout} operand {operand} rot={rot} red={red}"
    main = {"NT": "pre", "NN": "gx", "TN": "gW"}[layout]
    n = got[main].shape[0] if operand == "A" else got[main].shape[1]
    rest = torch.tensor([i for i in range(n) if i not in where])
    for name in ("pre", "y", "gx", "gW"):                                           # nothing outside the planted lines changes
        if name in got:
            same = (torch.equal(got[name][rest], base[name][rest]) if operand == "A"
                    else torch.equal(got[name][:, rest], base[name][:, rest]))
            assert same, f"{tag} {name}: a planted line reached an output that is not its own"
    out = got[main].double()
    lines = {pos: (out[pos] if operand == "A" else out[:, pos]) for pos in where}
    line_of = lambda t, pos: t[pos] if operand == "A" else t[:, pos]
    for pos, cls in where.items():
        line = lines[pos]
        if cls in NON_FINITE:                                                       # NaN or +-Inf: not specified which
            assert not bool(torch.isfinite(line).any()), (tag, pos, cls)
            assert not bool(torch.isfinite(line_of(want, pos)).any())
        elif cls == "neg_zero":
            zero = line_of(b.double().expand_as(out), pos) if layout == "NT" else torch.zeros_like(line)
            assert torch.equal(line, zero), (tag, pos, cls)                         # exact zeros plus bias
        else:
            assert bool(torch.isfinite(line).all()), (tag, pos, cls)
    fin = torch.isfinite(want)
    assert int((~fin).sum()) == sum(cls in NON_FINITE for cls in where.values()) * (out.numel() // n)
    e3 = (out - want).abs()[fin] / ((3 * R + 1) * EPS * R3[fin]).clamp_min(1e-300)
    ex = (out - exact).abs()[fin] / X.combined_bound(R, R_exact, R3)[fin].clamp_min(1e-300)
    print(f"{tag}: finite outputs, error / RN bound = {float(e3.max()):.3f}, |got - exact| / combined bound = {float(ex.max()):.3f}; "
          f"non-finite reference outputs: {int((~fin).sum())}")
    assert float(e3.max()) <= 2.0 and float(ex.max()) <= 1.0, tag
    if layout == "TN":                                                              # gb: fp32 sums of the UNROUNDED g
        if operand == "B":
            assert torch.equal(got["gb"], base["gb"]), tag                          # x does not enter gb
        else:
            assert torch.equal(got["gb"][rest], base["gb"][rest]), tag
            okb = C.agrees(got["gb"], pg.double().sum(0), N * EPS * pg.double().abs().sum(0))
            assert bool(okb.all()), f"{tag}: gb"
            for pos, cls in where.items():                                          # FLT_MAX stays finite in an fp32 sum
                assert bool(torch.isfinite(got["gb"][pos])) == (cls not in ("nan_elem", "pos_inf_elem", "neg_inf_elem")), (tag, pos, cls)
