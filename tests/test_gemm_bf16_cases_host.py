"""CPU: tests/gemm_bf16_cases.py against the library's own rules and against what its builders claim.  The instance table must
reach all nine (layout, tile) kernel instances of csrc/lipvq_gemm_bf16.hip -- asked of lipvq_gemm_bf16_tile, the function the
launcher itself takes its tile from -- with the ragged edges the table states; the special-value builders must plant what
their names say; the references must be finite wherever their operands are."""
import numpy as np
import pytest
import torch

import gemm_bf16_cases as C


@pytest.fixture(scope="module")
def lib():
    from lipvq_vae_amd import _capi
    return _capi.lib


@pytest.mark.parametrize("inst", C.INSTANCES, ids=lambda i: i.id)
def test_table_row_reaches_its_instance_with_its_ragged_edges(lib, inst):
    M, Nc, R, chunks = C.launch_dims(inst.layout, inst.N, inst.K, inst.J)
    assert lib.lipvq_gemm_bf16_tile(M, Nc, chunks) == inst.tile
    assert inst.K % 8 == 0 and inst.J % 8 == 0                                        # the kernels' own limit
    if inst.layout == "TN":                                                           # the header's formula is the library's
        assert lib.lipvq_wgrad_bf16_workspace_bytes(inst.N, inst.J, inst.K) == chunks * (inst.J * inst.K + inst.J) * 4
    props = C.ragged_properties(inst)
    assert inst.ragged, "a row that states nothing ragged"
    for key, want in inst.ragged.items():
        assert props[key] == want, (key, props[key], want)


def test_table_reaches_all_nine_instances():
    assert {(i.layout, i.tile) for i in C.INSTANCES} == {(l, t) for l in ("NT", "NN", "TN") for t in (32, 64, 128)}
    # and the paths only the 2 x 2-wave tiles have: a partial row tile and a column tile whose second wave column is out whole
    for layout in ("NT", "NN"):
        assert any(i.layout == layout and i.tile == 128 and C.ragged_properties(i)["wave_col_out"]
                   and C.ragged_properties(i)["rows_rem"] for i in C.INSTANCES)


def test_tile_rule_returns_zero_for_non_positive_arguments(lib):
    tile = lib.lipvq_gemm_bf16_tile
    assert tile(0, 64, 1) == 0 and tile(64, 0, 1) == 0 and tile(64, 64, 0) == 0 and tile(-5, 64, 1) == 0
    assert tile(1, 8, 1) == 32 and tile(2 ** 40, 8, 1) == 128


@pytest.mark.parametrize("Nc,chunks", [(2056, 1), (136, 1), (264, 3)])
def test_tile_rule_thresholds(lib, Nc, chunks):
    """The M at which the t^2-grid has exactly 255 and exactly 256 workgroups, found by walking M (no formula of the rule's
    own): they straddle the choice of tile t."""
    tile = lib.lipvq_gemm_bf16_tile
    for t in (128, 64):
        wgs = lambda M: C.ceil_div(M, t) * C.ceil_div(Nc, t) * chunks
        below = max((M for M in range(1, 40000) if wgs(M) <= 255), default=None)
        above = min((M for M in range(1, 40000) if wgs(M) >= 256), default=None)
        assert below is not None and above == below + 1 and wgs(below) < 256 <= wgs(above)
        if t == 128:
            assert tile(below, Nc, chunks) != 128 and tile(above, Nc, chunks) == 128
        else:                                               # (the 128 grid is far below 256 here: the 64 rule decides)
            assert tile(below, Nc, chunks) == 32 and tile(above, Nc, chunks) == 64
    # a grid of EXACTLY 255 and exactly 256 workgroups: Nc <= t, chunks = 1, so the grid is ceil(M / t)
    for t, other in ((128, 64), (64, 32)):
        assert tile(255 * t, t, 1) == other and tile(255 * t + 1, t, 1) == t
    assert tile(255 * 128, 128, 1) == 64                    # 255 at 128 is 510 at 64


def test_row_position_comparisons_cross_tiles(lib):
    """The shapes of the row-position tests use different kernel instances on their two sides."""
    tile = lib.lipvq_gemm_bf16_tile
    # NT: x [1921, 40] . W [2056, 40]^T and NN: g [1921, 40] . W [40, 2056] both have 2056 output columns
    assert (tile(1921, 2056, 1), tile(1001, 2056, 1), tile(33, 2056, 1)) == (128, 64, 32)
    assert tile(1921, 24, 1) == 32                                              # a 24-row slice of W
    rows = {8192: (64, 64, 128, 64), 1024: (32, 32, 32, 32)}                    # E = 128: qkv, output, fc1, fc2
    for n, want in rows.items():
        assert tuple(tile(n, Nc, 1) for Nc in (384, 128, 512, 128)) == want


# ---------------------------------------------------------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------------------------------------------------------
def _bits(v):
    return int(np.float32(v).view(np.uint32))


def test_rounding_facts_the_builders_rest_on():
    f = lambda v: float(torch.tensor([v], dtype=torch.float32).bfloat16().float())
    assert f(C.TIE_EVEN_DOWN) == 1.0 and f(-C.TIE_EVEN_DOWN) == -1.0                 # ties go to even: down here ...
    assert f(C.TIE_EVEN_UP) == 1.0 + 2.0 ** -6 and f(-C.TIE_EVEN_UP) == -(1.0 + 2.0 ** -6)   # ... and up here
    for v in (C.TIE_EVEN_DOWN, C.TIE_EVEN_UP):                                        # they ARE ties: exact in fp32, halfway
        assert float(np.float32(v)) == v and _bits(v) & 0xFFFF == 0x8000
    away = C.round_half_away(torch.tensor([C.TIE_EVEN_DOWN, C.TIE_EVEN_UP, -C.TIE_EVEN_DOWN, 1.0, -2.5], dtype=torch.float32))
    assert away.tolist() == [1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7), 1.0, -2.5]
    trunc = float(np.uint32(_bits(C.TIE_EVEN_UP) & 0xFFFF0000).view(np.float32))
    assert trunc == 1.0 + 2.0 ** -7 != f(C.TIE_EVEN_UP)                               # truncation misses the other tie
    assert C.FLT_MAX == float(np.finfo(np.float32).max) and f(C.FLT_MAX) == float("inf") and f(-C.FLT_MAX) == float("-inf")
    assert f(C.TWO126) == C.TWO126 and float(np.float32(C.TWO126)) == C.TWO126        # exact in both formats
    z = torch.tensor([-0.0], dtype=torch.float32).bfloat16().float()
    assert float(z) == 0.0 and bool(torch.signbit(z)[0])                              # -0 stays -0
    assert f(C.DENORMALS[0]) == 2.0 ** -133 and f(C.DENORMALS[1]) == 0.0              # a bf16 denormal; below half of the smallest
    assert 0 < float(np.float32(C.DENORMALS[0])) < 2.0 ** -126 and float(np.float32(C.DENORMALS[1])) == 2.0 ** -149


def test_seams_and_rotation():
    assert C.seam_positions(2056) == [0, 31, 32, 63, 64, 127, 128, 2055]
    assert C.seam_positions(136) == [0, 31, 32, 63, 64, 127, 128, 135] and C.seam_positions(40) == [0, 31, 32, 39]
    t = torch.zeros(300, 16)
    seen = set()
    for rot in range(len(C.SPECIAL_CLASSES)):
        _, where = C.plant(t, 0, 3, rot)
        assert list(where) == C.seam_positions(300)
        assert set(where.values()) == set(C.SPECIAL_CLASSES)                          # 8 seams, 7 classes: every class every time
        seen.add(where[0])
    assert seen == set(C.SPECIAL_CLASSES)                                             # ... and every class reaches seam 0
    assert C.plant(t, 0, 3, 0)[1][0] == "nan_elem"                                    # rot = 0: the NaN sits on the clamp target


@pytest.mark.parametrize("axis", [0, 1])
def test_plant_changes_the_named_lines_and_nothing_else(axis):
    torch.manual_seed(5)
    t = torch.randn(200, 136) / 8
    red = 3
    for classes in (C.SPECIAL_CLASSES, ("denormal",)):
        p, where = C.plant(t, axis, red, rot=2, classes=classes)
        assert p is not t and p.shape == t.shape and p.is_contiguous()
        lines, base = (p, t) if axis == 0 else (p.t(), t.t())
        untouched = [i for i in range(lines.shape[0]) if i not in where]
        assert torch.equal(lines[untouched], base[untouched])
        for pos, cls in where.items():
            line, was = lines[pos], base[pos]
            others = [k for k in range(line.numel()) if k != red]
            if cls.endswith("_elem"):
                assert torch.equal(line[others], was[others]), cls                   # one element changed
            v = float(line[red])
            if cls == "nan_elem":
                assert v != v
            elif cls == "pos_inf_elem":
                assert v == float("inf")
            elif cls == "neg_inf_elem":
                assert v == float("-inf")
            elif cls == "flt_max_elem":
                assert v == C.FLT_MAX and float(line[red].bfloat16()) == float("inf")
            elif cls == "two126_elem":
                assert v == 2.0 ** 126
            elif cls == "ties":
                assert set(line.tolist()) == {C.TIE_EVEN_DOWN, C.TIE_EVEN_UP, -C.TIE_EVEN_DOWN, -C.TIE_EVEN_UP}
                signs = torch.where(torch.arange(line.numel()) % 3 == 0, -1.0, 1.0)
                signed = C.tie_line(line.numel(), signs)
                assert torch.equal(signed.abs(), line.abs()) and torch.equal(torch.sign(signed), signs)
                assert set(line.bfloat16().float().tolist()) == {1.0, 1.0 + 2.0 ** -6, -1.0, -(1.0 + 2.0 ** -6)}
            elif cls == "neg_zero":
                assert bool((line == 0).all()) and bool(torch.signbit(line).all()) and bool(torch.signbit(line.bfloat16().float()).all())
            elif cls == "denormal":
                assert set(line.tolist()) == {float(np.float32(1e-40)), 2.0 ** -149}
                assert set(line.bfloat16().float().tolist()) == {2.0 ** -133, 0.0}


def _explicit(layout, A, B, line_axis_a, pos):
    """Row `pos` of C (the output line of A's line `pos`) by an explicit float64 sum over the reduction -- no BLAS."""
    Ar, Br = C.rb(A), C.rb(B)
    a = Ar[pos] if line_axis_a == 0 else Ar[:, pos]                                 # [R]
    Bk = Br.t() if layout == "NT" else Br                                          # [R, Nc]
    return (a[:, None] * Bk).sum(0)


@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
def test_special_references_are_ieee_and_overflow_nothing(layout):
    """Float64 on the rounded operands: finite wherever every operand of the output element is finite (no float64 overflow, no
    fp32 one either: below 2^127), NaN / +-Inf exactly where IEEE puts them -- checked against an explicit sum, not the BLAS --
    and every tie line distinguishes nearest-even from round-half-away by more than the kernels' bound."""
    x, W, b, g = C.special_base(layout)
    for t in (x, W, g):
        assert float(t.abs().max()) < 1.0                                             # 2^126 times any of these is finite in fp32
        assert float((t.bfloat16().float() != t).float().mean()) > 0.9
    A, B, axa, axb = C.operands(layout, x, W, g)
    R = C.launch_dims(layout, *C.SPECIAL_SHAPES[layout])[2]
    base, _ = C.product64(layout, A, B)
    assert bool(torch.isfinite(base).all())
    for rot, red in ((0, 3), (3, R - 1)):
        pa, where = C.plant(A, axa, red, rot, tie_signs=C.witness_signs(layout, B, True))
        got, Rsum = C.product64(layout, pa, B)
        planted = sorted(where)
        rest = [i for i in range(got.shape[0]) if i not in where]
        assert torch.equal(got[rest], base[rest])                                    # other rows of the REFERENCE do not move
        for pos, cls in where.items():
            row, want = got[pos], _explicit(layout, pa, B, axa, pos)
            bcol = (C.rb(B)[:, red] if layout == "NT" else C.rb(B)[red]) if cls.endswith("_elem") else None
            if cls == "nan_elem":
                assert bool(torch.isnan(row).all())
            elif cls in ("pos_inf_elem", "neg_inf_elem", "flt_max_elem"):
                sign = -1.0 if cls == "neg_inf_elem" else 1.0
                assert bool((bcol != 0).all()) and torch.equal(row, sign * torch.sign(bcol) * float("inf"))
            else:
                assert bool(torch.isfinite(row).all()) and float(row.abs().max()) < 2.0 ** 127
                assert bool(torch.isfinite(Rsum[pos]).all()) and float(Rsum[pos].max()) < 2.0 ** 127
                assert bool(((row - want).abs() <= 1e-12 * Rsum[pos]).all())
            if cls == "ties":
                line = pa[pos] if axa == 0 else pa[:, pos]
                away = C.round_half_away(line)
                Bk = C.rb(B).t() if layout == "NT" else C.rb(B)
                other = (away[:, None] * Bk).sum(0)
                bound = 2 * (R + 1) * C.EPS * Rsum[pos]
                far = ((other - row).abs() > 2 * bound)            # a result within `bound` of one is outside it of the other
                assert bool(far[C.WITNESS]), f"{layout}: round-half-away is within the bound of nearest-even"
                assert R > 100 or float(far.float().mean()) > 0.5            # a short reduction tells them apart nearly everywhere
        assert planted == C.seam_positions(got.shape[0])
    # B's lines feed the COLUMNS of C
    pb, where = C.plant(B, axb, 3, 0)
    got, _ = C.product64(layout, A, pb)
    rest = [i for i in range(got.shape[1]) if i not in where]
    assert torch.equal(got[:, rest], base[:, rest])
    for pos, cls in where.items():
        col = got[:, pos]
        if cls == "nan_elem":
            assert bool(torch.isnan(col).all())
        elif cls.endswith("inf_elem") or cls == "flt_max_elem":
            assert bool(torch.isinf(col).all())
        else:
            assert bool(torch.isfinite(col).all()) and float(col.abs().max()) < 2.0 ** 127


def test_agrees_tells_the_classes_apart():
    want = torch.tensor([1.0, float("inf"), float("-inf"), float("nan"), 2.0], dtype=torch.float64)
    bound = torch.full((5,), 0.5, dtype=torch.float64)
    assert C.agrees(torch.tensor([1.25, float("inf"), float("-inf"), float("nan"), 2.0]), want, bound).tolist() == [True] * 5
    bad = torch.tensor([1.75, float("-inf"), float("nan"), 0.0, float("inf")])
    assert C.agrees(bad, want, bound).tolist() == [False] * 5


def test_shared_case_is_cached_and_read_only_by_convention():
    a, b = C.case(33, 72, 24), C.case(33, 72, 24)
    assert a is b and a["y"].dtype == torch.float64 and a["y"].shape == (33, 24) and a["gW"].shape == (24, 72)
