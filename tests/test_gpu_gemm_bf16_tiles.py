"""GPU: every kernel instance of csrc/lipvq_gemm_bf16.hip -- three layouts (forward NT, input gradient NN, weight gradient TN)
at three tiles (32, 64, 128) -- at ragged edges, across tiles bit for bit, and on special values at the seams of the 128 tile.

Shapes, inputs and references come from tests/gemm_bf16_cases.py; tests/test_gemm_bf16_cases_host.py shows on the CPU that the
table reaches all nine instances (through lipvq_gemm_bf16_tile, which the launcher itself asks) and that every planted input
is what its name says.  The reference is torch float64 on the bf16-rounded operands and the bound the one of
tests/test_gpu_gemm_bf16.py: with R = sum |a^ b^| per output, error <= 2 (length + 1) 2^-24 R (twice any-order
round-to-nearest accumulation); gb within N 2^-24 sum |g| of the float64 column sums of the unrounded g.  Every ratio is
printed before it is asserted.  Kernels run through the C ABI into sentinel-fenced outputs at unaligned word offsets.

Measured on an MI355X: DESIGN.md section 4.6.1.
"""
import pytest
import torch
import torch.nn.functional as F

import gemm_bf16_cases as C
from fenced import _Fenced

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_GELU = 0, 1
EPS = C.EPS


@pytest.fixture(scope="module")
def abi():
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    return _capi.lib, _capi.check, lipvq_vae_amd.ops._stream


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _ptr(t):
    return None if t is None else t.data_ptr()


def _forward(abi, x, W, b, act, with_pre):
    """lipvq_linear_act_bf16 into fenced outputs: (y, pre or None) on the CPU, every word written, no guard word touched."""
    lib, check, stream = abi
    (N, K), J = x.shape, W.shape[0]
    xc, Wc, bc = x.cuda(), W.cuda(), None if b is None else b.cuda()
    y, pre = _Fenced("y", N, J, offset_words=1), (_Fenced("pre", N, J, offset_words=3) if with_pre else None)
    check(lib.lipvq_linear_act_bf16(xc.data_ptr(), Wc.data_ptr(), _ptr(bc), y.ptr(), None if pre is None else pre.ptr(),
                                    N, K, J, act, stream()), "lipvq_linear_act_bf16")
    torch.cuda.synchronize()
    return y.check().cpu(), (None if pre is None else pre.check().cpu())


def _input_gradient(abi, g, W):
    lib, check, stream = abi
    (N, J), K = g.shape, W.shape[1]
    gc, Wc = g.cuda(), W.cuda()
    gx = _Fenced("gx", N, K, offset_words=2)
    check(lib.lipvq_linear_nn_bf16(gc.data_ptr(), Wc.data_ptr(), gx.ptr(), N, J, K, stream()), "lipvq_linear_nn_bf16")
    torch.cuda.synchronize()
    return gx.check().cpu()


def _weight_gradient(abi, g, x, with_gb=True):
    lib, check, stream = abi
    (N, J), K = g.shape, x.shape[1]
    gc, xc = g.cuda(), x.cuda()
    gW, gb = _Fenced("gW", J, K, offset_words=1), (_Fenced("gb", J, offset_words=3) if with_gb else None)
    ws = torch.empty(lib.lipvq_wgrad_bf16_workspace_bytes(N, J, K), dtype=torch.uint8, device="cuda")
    check(lib.lipvq_wgrad_bf16(gc.data_ptr(), xc.data_ptr(), gW.ptr(), None if gb is None else gb.ptr(), ws.data_ptr(),
                               N, J, K, stream()), "lipvq_wgrad_bf16")
    torch.cuda.synchronize()
    return gW.check().cpu(), (None if gb is None else gb.check().cpu())


# ---------------------------------------------------------------------------------------------------------------------------
# every instance at ragged edges
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", C.INSTANCES, ids=lambda i: i.id)
def test_instance_at_ragged_edges(abi, inst):
    lib = abi[0]
    N, K, J = inst.N, inst.K, inst.J
    M, Nc, R, chunks = C.launch_dims(inst.layout, N, K, J)
    assert lib.lipvq_gemm_bf16_tile(M, Nc, chunks) == inst.tile                      # the instance under test is the stated one
    c = C.case(N, K, J)
    tag = f"{inst.layout} tile {inst.tile} N={N} K={K} J={J}"
    if inst.layout == "NT":
        y, pre = _forward(abi, c["x"], c["W"], c["b"], ACT_GELU, True)
        want = c["y"] + c["b"].double()
        worst = C.ratio(f"{tag} bias gelu pre", pre, want, c["Ry"], K)
        ref = F.gelu(pre.double())
        assert float((y.double() - ref).abs().max()) <= 1e-5 * float(want.abs().max()), tag
        y0, none = _forward(abi, c["x"], c["W"], None, ACT_NONE, False)
        assert none is None
        worst = max(worst, C.ratio(f"{tag} plain", y0, c["y"], c["Ry"], K))
    elif inst.layout == "NN":
        worst = C.ratio(tag, _input_gradient(abi, c["g"], c["W"]), c["gx"], c["Rgx"], J)
    else:
        gW, gb = _weight_gradient(abi, c["g"], c["x"])
        worst = C.ratio(f"{tag} gW", gW, c["gW"], c["RgW"], N)
        e = (gb.double() - c["gb"]).abs()
        print(f"{tag} gb: error / (N 2^-24 sum|g|) = {float((e / (N * EPS * c['Rgb'])).max()):.3f}")
        assert bool((e <= N * EPS * c["Rgb"]).all()), tag
        if (N, K, J) == (2801, 264, 136):                                           # gb = NULL: the same gW bits
            gW2, none = _weight_gradient(abi, c["g"], c["x"], with_gb=False)
            assert none is None and torch.equal(gW2, gW), tag
    print(f"INSTANCE {inst.id}: largest error / RN bound = {worst:.2e}")
    assert worst <= 2.0, (tag, worst)


# ---------------------------------------------------------------------------------------------------------------------------
# a row does not depend on its position, on the number of rows of the launch or on the tile: bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [ACT_NONE, ACT_GELU], ids=["none", "gelu"])
def test_forward_rows_and_columns_across_tiles(abi, ops, act):
    tile = abi[0].lipvq_gemm_bf16_tile
    c = C.case(1921, 40, 2056)
    x, W, b = c["x"].cuda(), c["W"].cuda(), c["b"].cuda()
    N, J = x.shape[0], W.shape[0]
    full = ops.linear_bf16(x, W, b, act=act)
    assert tile(N, J, 1) == 128
    for r0 in (0, 127, 1888):                                                       # 33 rows: tile 32
        assert tile(33, J, 1) == 32
        part = x[r0:r0 + 33]
        assert part.is_contiguous() and part.data_ptr() % 16 == 0                  # a view: no copy is involved
        assert torch.equal(ops.linear_bf16(part, W, b, act=act), full[r0:r0 + 33]), r0
    assert tile(1001, J, 1) == 64
    assert torch.equal(ops.linear_bf16(x[:1001], W, b, act=act), full[:1001])
    for c0 in (0, 2032):                                                            # 24 rows of W: tile 32, the matching columns
        assert tile(N, 24, 1) == 32
        Wp, bp = W[c0:c0 + 24], b[c0:c0 + 24].contiguous()
        assert Wp.is_contiguous() and Wp.data_ptr() % 16 == 0
        assert torch.equal(ops.linear_bf16(x, Wp, bp, act=act), full[:, c0:c0 + 24]), c0


def test_input_gradient_rows_across_tiles(abi, ops):
    tile = abi[0].lipvq_gemm_bf16_tile
    c = C.case(1921, 2056, 40)
    g, W = c["g"].cuda(), c["W"].cuda()                                             # g [1921, 40], W [40, 2056]
    N, K = g.shape[0], W.shape[1]
    full = ops.linear_nn_bf16(g, W)
    assert (tile(N, K, 1), tile(1001, K, 1), tile(33, K, 1)) == (128, 64, 32)
    for r0 in (0, 127, 1888):
        part = g[r0:r0 + 33]
        assert part.is_contiguous() and part.data_ptr() % 16 == 0
        assert torch.equal(ops.linear_nn_bf16(part, W), full[r0:r0 + 33]), r0
    assert torch.equal(ops.linear_nn_bf16(g[:1001], W), full[:1001])


def test_cached_backbone_equals_full_across_tiles_in_bf16_mode(abi):
    """B = 128 sequences of 64 tokens, E = 128: the full call's 8192 rows run the four Linears at tiles 64 / 64 / 128 / 64, the
    cached call's 1024 rows at 32 everywhere (asked of the entry point), and forward_cached == net(x)[:, P:] in bits."""
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gpt import GPTBackbone
    tile = abi[0].lipvq_gemm_bf16_tile
    E, L, B, P = 128, 64, 128, 56
    torch.manual_seed(7)
    net = GPTBackbone(embed_dim=E, context_length=L, causal=True, num_layers=1, num_heads=4, attn_dropout=0.0,
                      block_output_dropout=0.0).cuda().eval().set_matmul_precision("bf16")
    widths = [m.out_features for m in net.modules() if isinstance(m, torch.nn.Linear)]
    assert widths == [3 * E, E, 4 * E, E]
    assert [tile(B * L, w, 1) for w in widths] == [64, 64, 128, 64]
    assert [tile(B * (L - P), w, 1) for w in widths] == [32, 32, 32, 32]
    x = torch.randn(B, L, E).cuda()
    with torch.no_grad():
        full = net(x)
        out = net.forward_cached(x[:, P:], net.prefill(x[:, :P]))
    assert out.shape == (B, L - P, E) and bool(torch.isfinite(full).all())
    print(f"cached vs full bf16, 8192 / 1024 rows: max |difference| = {float((out - full[:, P:]).abs().max()):.3e}")
    assert torch.equal(out, full[:, P:])


# ---------------------------------------------------------------------------------------------------------------------------
# special values at the seams of the 128 tile
# ---------------------------------------------------------------------------------------------------------------------------
def _run(abi, layout, x, W, b, g, plain=False):
    """dict name -> output on the CPU.  NT: bias + GELU + pre (plain: no bias, no activation, no pre)."""
    if layout == "NT":
        if plain:
            return dict(y=_forward(abi, x, W, None, ACT_NONE, False)[0])
        y, pre = _forward(abi, x, W, b, ACT_GELU, True)
        return dict(pre=pre, y=y)
    if layout == "NN":
        return dict(gx=_input_gradient(abi, g, W))
    gW, gb = _weight_gradient(abi, g, x)
    return dict(gW=gW, gb=gb)


_unplanted = {}


def _base_run(abi, layout, plain=False):
    key = (layout, plain and layout == "NT")
    if key not in _unplanted:
        _unplanted[key] = _run(abi, layout, *C.special_base(layout), plain=plain)
    return _unplanted[key]


def _planted_inputs(layout, operand, red, rot, classes):
    """(x, W, b, g) with the layout's A or B operand planted, `where`, and the float64 (want, R) of the product."""
    x, W, b, g = C.special_base(layout)
    A, B, axa, axb = C.operands(layout, x, W, g)
    if operand == "A":
        pA, where = C.plant(A, axa, red, rot, classes, tie_signs=C.witness_signs(layout, B, True))
        pB = B
    else:
        pB, where = C.plant(B, axb, red, rot, classes, tie_signs=C.witness_signs(layout, A, False))
        pA = A
    want, Rsum = C.product64(layout, pA, pB)
    px, pW, pg = {"NT": (pA, pB, g), "NN": (x, pB, pA), "TN": (pB, W, pA)}[layout]
    return (px, pW, b, pg), where, want, Rsum


def _lines_equal(got, base, operand, where, what):
    """Everything outside the planted lines' own rows (A) or columns (B) of C has the bits of the unplanted run."""
    n = got.shape[0] if operand == "A" else got.shape[1]
    rest = torch.tensor([i for i in range(n) if i not in where])
    same = torch.equal(got[rest], base[rest]) if operand == "A" else torch.equal(got[:, rest], base[:, rest])
    assert same, f"{what}: a planted line reached an output that is not its own"


def _red_choices(layout):
    """Two places for the single planted element of a line: inside the first 8 reduction indices (with line 0 the address
    every out-of-range load of a reduction-contiguous operand is clamped to) and the LAST reduction index (the row every
    out-of-range load of a reduction-strided operand is clamped to; for the weight gradient a row of the ragged last chunk)."""
    R = C.launch_dims(layout, *C.SPECIAL_SHAPES[layout])[2]
    return ((0, 3), (3, R - 1))                                                     # (rot, red)


@pytest.mark.parametrize("which", [0, 1], ids=["first8", "last"])
@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
def test_special_values_stay_in_their_own_row_or_column(abi, layout, operand, which):
    rot, red = _red_choices(layout)[which]
    N, K, J = C.SPECIAL_SHAPES[layout]
    R = C.launch_dims(layout, N, K, J)[2]
    inputs, where, want, Rsum = _planted_inputs(layout, operand, red, rot, C.SPECIAL_CLASSES)
    if which == 0:
        assert where[0] == "nan_elem"                                               # the NaN sits in the clamp target
    base, got = _base_run(abi, layout), _run(abi, layout, *inputs)
    tag = f"{layout} operand {operand} rot={rot} red={red}"
    main = {"NT": "pre", "NN": "gx", "TN": "gW"}[layout]
    for name in ("pre", "y", "gx", "gW"):
        if name in got:
            _lines_equal(got[name], base[name], operand, where, f"{tag} {name}")
    if layout == "NT":
        want = want + inputs[2].double()
    bound = 2 * (R + 1) * EPS * Rsum
    ok = C.agrees(got[main], want, bound)
    fin = torch.isfinite(want)
    r = float(((got[main].double() - want).abs()[fin] / bound[fin].clamp_min(1e-300)).max()) / 2
    print(f"{tag}: finite outputs, error / RN bound = {r:.3f}; non-finite reference outputs: {int((~fin).sum())}")
    assert bool(ok.all()), f"{tag}: {int((~ok).sum())} outputs are not what IEEE arithmetic on the rounded operands gives"
    for pos, cls in where.items():                                                  # said once more, per class
        line = got[main][pos] if operand == "A" else got[main][:, pos]
        if cls == "nan_elem":
            assert bool(torch.isnan(line).all()), (tag, pos, cls)
        elif cls in ("pos_inf_elem", "neg_inf_elem", "flt_max_elem"):               # FLT_MAX rounds to +Inf in bf16
            assert bool(torch.isinf(line).all()), (tag, pos, cls)
        else:
            assert bool(torch.isfinite(line).all()), (tag, pos, cls)
    if layout == "TN":
        g = inputs[3]
        if operand == "B":
            assert torch.equal(got["gb"], base["gb"]), tag                          # x does not enter gb
        else:
            _lines_equal(got["gb"][:, None], base["gb"][:, None], "A", where, f"{tag} gb")
            okb = C.agrees(got["gb"], g.double().sum(0), N * EPS * g.double().abs().sum(0))
            assert bool(okb.all()), f"{tag}: gb"
            for pos, cls in where.items():                                          # gb sums the UNROUNDED g: FLT_MAX stays finite
                assert bool(torch.isfinite(got["gb"][pos])) == (cls not in ("nan_elem", "pos_inf_elem", "neg_inf_elem")), (tag, pos, cls)


@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
def test_fp32_denormal_inputs(abi, layout, operand):
    """Lines of 1e-40 and 2^-149 in turn (the bf16 denormal 2^-133 and 0 after rounding) at every seam, no bias.  Whether the
    convert and the bf16 matrix pipe keep or flush denormal operands is not documented; every other operand is below 1, so a
    flushed operand moves a product by less than 2^-126: the bound is the usual one plus 2^-126 per product.  The behaviour
    seen is printed (the accumulator path never flushes, so an output of exactly 0 means the OPERANDS were flushed)."""
    N, K, J = C.SPECIAL_SHAPES[layout]
    R = C.launch_dims(layout, N, K, J)[2]
    inputs, where, want, Rsum = _planted_inputs(layout, operand, 0, 0, ("denormal",))
    assert set(where.values()) == {"denormal"} and bool(torch.isfinite(want).all())
    base, got = _base_run(abi, layout, plain=True), _run(abi, layout, *inputs, plain=True)
    main = {"NT": "y", "NN": "gx", "TN": "gW"}[layout]
    tag = f"{layout} operand {operand} denormal lines"
    _lines_equal(got[main], base[main], operand, where, tag)
    bound = 2 * (R + 1) * EPS * Rsum + R * 2.0 ** -126
    err = (got[main].double() - want).abs()
    pos = sorted(where)
    lines, ref = (got[main][pos], want[pos]) if operand == "A" else (got[main][:, pos], want[:, pos])
    live = ref.abs() >= 2.0 ** -140                                                 # outputs whose exact value fp32 can hold
    zero = float((lines[live] == 0).float().mean())
    close = float(((lines.double() - ref).abs()[live] <= 2.0 ** -149 + 1e-3 * ref.abs()[live]).float().mean())
    seen = "KEPT" if close == 1.0 else ("FLUSHED to zero" if zero == 1.0 else "MIXED")
    print(f"{tag}: denormal operands {seen} ({int(live.sum())} outputs with a reference magnitude >= 2^-140: {zero:.3f} of them "
          f"exactly 0, {close:.3f} within 2^-149 + 0.1 % of the reference); largest error {float(err.max()):.3e}, "
          f"error / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), tag
    if layout == "TN" and operand == "A":                                           # gb: fp32 additions of the unrounded g
        g = inputs[3]
        eb = (got["gb"].double() - g.double().sum(0)).abs()
        print(f"{tag}: gb of the denormal columns {got['gb'][pos].tolist()} (float64: {g.double().sum(0)[pos].tolist()})")
        assert bool((eb <= N * EPS * g.double().abs().sum(0) + N * 2.0 ** -126).all()), f"{tag}: gb"
