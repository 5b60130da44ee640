"""Shapes, inputs and float64 references of the bf16 Linear tests (tests/test_gpu_gemm_bf16.py, test_gpu_gemm_bf16_tiles.py).
Pure numpy and torch on the CPU, no torch.cuda: tests/test_gemm_bf16_cases_host.py holds the instance table to the library's
tile and chunk rules and every builder to what its name says, so that a failure on the GPU cannot come from a shape that
misses its kernel instance or from an input that is not what it claims.

A product is C [M][Nc] = A . B over a reduction of length R; columns of the table are (N, K, J) with x [N, K], W [J, K],
g [N, J]:
    NT  forward          y  [N, J] = x . W^T   M = N, Nc = J, R = K   lines of A: rows of x,    lines of B: rows of W
    NN  input gradient   gx [N, K] = g . W     M = N, Nc = K, R = J   lines of A: rows of g,    lines of B: columns of W
    TN  weight gradient  gW [J, K] = g^T . x   M = J, Nc = K, R = N   lines of A: columns of g, lines of B: columns of x
A LINE of an operand is what feeds one row (A) or one column (B) of C and nothing else.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

EPS = 2.0 ** -24
FLT_MAX = float(torch.finfo(torch.float32).max)
BK = 32                                   # reduction elements per staged step (GB_BK of csrc/lipvq_gemm_bf16.hip)


def rb(t):
    """float64 of the operand rounded to bf16 (nearest even), as the kernels read it."""
    return t.bfloat16().double()


def ceil_div(a, b):
    return -(-a // b)


def header_chunk(N, J, K):
    """Rows per chunk of the weight gradient, as include/lipvq.h writes the rule."""
    want = max(1, 1024 // (ceil_div(J, 128) * ceil_div(K, 128)))
    return max(64, 32 * ceil_div(ceil_div(N, want), 32))


def launch_dims(layout, N, K, J):
    """(M, Nc, R, chunks) of the launch: the arguments of lipvq_gemm_bf16_tile and the reduction length."""
    if layout == "NT":
        return N, J, K, 1
    if layout == "NN":
        return N, K, J, 1
    assert layout == "TN"
    return J, K, N, ceil_div(N, header_chunk(N, J, K))


class Instance(NamedTuple):
    layout: str
    N: int
    K: int
    J: int
    tile: int
    ragged: dict            # property of ragged_properties -> the value the table states

    @property
    def id(self):
        return f"{self.layout}{self.tile}-{self.N}x{self.K}x{self.J}"


# (layout, N, K, J, tile, what is ragged): DESIGN.md 4.6.1; checked against the library by the host test
INSTANCES = (
    Instance("NT", 33, 40, 2056, 32, dict(rows_rem=1, cols_rem=8, steps=2, last_step=8)),
    Instance("NT", 1001, 72, 1032, 64, dict(rows_rem=41, cols_rem=8, steps=3, last_step=8)),
    Instance("NT", 1921, 40, 2056, 128, dict(row_tiles=16, rows_rem=1, col_tiles=17, cols_rem=8, wave_col_out=True)),
    Instance("NT", 20001, 136, 136, 128, dict(col_tiles=2, cols_rem=8, wave_col_out=True, steps=5, last_step=8)),
    Instance("NN", 97, 8, 24, 32, dict(Nc=8, R=24, steps=1, last_step=24, rows_rem=1)),
    Instance("NN", 1001, 1032, 72, 64, dict(rows_rem=41, cols_rem=8, steps=3, last_step=8)),
    Instance("NN", 1921, 2056, 40, 128, dict(row_tiles=16, rows_rem=1, col_tiles=17, cols_rem=8, wave_col_out=True)),
    Instance("TN", 70, 40, 24, 32, dict(chunk=64, chunks=2, last_chunk_rows=6, steps=1, last_step=6)),
    Instance("TN", 1001, 24, 1032, 64, dict(chunks=16, last_chunk_rows=41, steps=2, last_step=9)),
    Instance("TN", 2801, 264, 136, 128, dict(chunk=64, chunks=44, last_chunk_rows=49, rows_rem=8, cols_rem=8)),
    Instance("TN", 20001, 136, 136, 128, dict(chunk=96, chunks=209, last_chunk_rows=33, steps_per_chunk=3)),
    Instance("TN", 1921, 40, 2056, 128, dict(chunk=64, chunks=31, last_chunk_rows=1)),
)


def ragged_properties(inst):
    """What of the launch is ragged, from the shape and the STATED tile alone (the host test checks the tile).  rows_rem /
    cols_rem: rows and columns of C in the last, partial tile (0: none); wave_col_out: at a 2 x 2-wave tile the partial
    column tile is at most half a tile wide, so its second wave column is out of range whole; steps / last_step: 32-wide
    reduction steps of the (last) chunk and the width of the last one; steps_per_chunk: steps of a whole chunk."""
    M, Nc, R, chunks = launch_dims(inst.layout, inst.N, inst.K, inst.J)
    t = inst.tile
    chunk = header_chunk(inst.N, inst.J, inst.K) if inst.layout == "TN" else R
    last = R - (chunks - 1) * chunk
    return dict(M=M, Nc=Nc, R=R, chunk=chunk, chunks=chunks, last_chunk_rows=last,
                row_tiles=ceil_div(M, t), col_tiles=ceil_div(Nc, t), rows_rem=M % t, cols_rem=Nc % t,
                wave_col_out=t >= 64 and 0 < Nc % t <= t // 2,
                steps=ceil_div(last, BK), last_step=last - (ceil_div(last, BK) - 1) * BK, steps_per_chunk=ceil_div(chunk, BK))


# ---------------------------------------------------------------------------------------------------------------------------
# randn inputs and their references (shared, computed once, never modified)
# ---------------------------------------------------------------------------------------------------------------------------
_cases = {}


def case(N, K, J):
    """Inputs and float64 references of one shape.  y / gx / gW: the products of the bf16-ROUNDED operands with their
    R = sum |a^ b^| terms; y_exact: the product of the unrounded operands; gb: the column sums of the unrounded g."""
    key = (N, K, J)
    if key not in _cases:
        torch.manual_seed(10000 * N + 10 * K + J)
        x, W, b, g = torch.randn(N, K), torch.randn(J, K) / K ** 0.5, torch.randn(J), torch.randn(N, J)
        for t in (x, W, g):
            changed = float((t.bfloat16().float() != t).float().mean())
            assert changed > 0.9, f"only {changed:.2f} of the elements change under bf16 rounding"
        xr, Wr, gr = rb(x), rb(W), rb(g)
        c = dict(x=x, W=W, b=b, g=g)
        c["y"], c["Ry"] = xr @ Wr.t(), xr.abs() @ Wr.abs().t()                   # forward: reduction K
        c["y_exact"], c["Ry_exact"] = x.double() @ W.double().t(), x.double().abs() @ W.double().abs().t()
        c["gx"], c["Rgx"] = gr @ Wr, gr.abs() @ Wr.abs()                         # input gradient: reduction J
        c["gW"], c["RgW"] = gr.t() @ xr, gr.abs().t() @ xr.abs()                 # weight gradient: reduction N
        c["gb"], c["Rgb"] = g.double().sum(0), g.double().abs().sum(0)
        _cases[key] = c
    return _cases[key]


def ratio(what, got, want, R, length):
    """Largest |got - want| / ((length + 1) 2^-24 R): <= 1 is any-order round-to-nearest accumulation."""
    rn = (length + 1) * EPS * R
    r = float(((got.cpu().double() - want).abs() / rn.clamp_min(1e-300)).max())
    print(f"{what}: error / RN bound = {r:.3f}")
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# special values at the seams of the 128 tile
# ---------------------------------------------------------------------------------------------------------------------------
SPECIAL_SHAPES = {"NT": (1921, 40, 2056), "NN": (1921, 2056, 40), "TN": (2801, 264, 136)}      # (N, K, J)
SEAMS = (0, 31, 32, 63, 64, 127, 128, -1)                      # -1: the last index

TIE_EVEN_DOWN = 1.0 + 2.0 ** -8                                # halfway between 1 and 1 + 2^-7: nearest even is 1
TIE_EVEN_UP = 1.0 + 3.0 * 2.0 ** -8                            # halfway between 1 + 2^-7 and 1 + 2^-6: nearest even is 1 + 2^-6
TWO126 = 2.0 ** 126
DENORMALS = (1e-40, 2.0 ** -149)                               # rounds to the bf16 denormal 2^-133; rounds to 0

# Planted per line, in planting order.  *_elem classes change ONE element of the line (reduction index `red`), the others
# the whole line.  nan / +-inf: IEEE specials; flt_max rounds to +Inf in bf16, so it is one as well; ties: +-(1 + 2^-8) and
# +-(1 + 3 2^-8), which round-half-away and truncation both get wrong; two126: exact in bf16, finite in fp32 against |w| < 1.
SPECIAL_CLASSES = ("nan_elem", "pos_inf_elem", "neg_inf_elem", "flt_max_elem", "ties", "two126_elem", "neg_zero")


WITNESS = 5                                                    # the line of the OTHER operand a tie line takes its signs from


def tie_line(n, signs=None):
    """1 + 2^-8 and 1 + 3 2^-8 in turn; signs [n] (+-1): per element, default + + - - ...  Over a long reduction with random
    signs the two roundings differ by a random walk that the accumulation bound swallows; with the signs of the other operand's
    WITNESS line every term of that output element moves the same way, and the element tells the roundings apart."""
    v = torch.tensor([TIE_EVEN_DOWN, TIE_EVEN_UP], dtype=torch.float32).repeat(ceil_div(n, 2))[:n]
    if signs is None:
        signs = torch.tensor([1.0, 1.0, -1.0, -1.0]).repeat(ceil_div(n, 4))[:n]
    return v * torch.where(signs < 0, -1.0, 1.0).float()


def witness_signs(layout, other, other_is_b):
    """The signs of line WITNESS of the other operand along the reduction (`other_is_b`: it is the layout's B operand)."""
    axis = {"NT": (0, 0), "NN": (0, 1), "TN": (1, 1)}[layout][1 if other_is_b else 0]
    return torch.sign(other[WITNESS] if axis == 0 else other[:, WITNESS])


def denormal_line(n):
    v = torch.tensor(DENORMALS, dtype=torch.float32)
    return v.repeat(ceil_div(n, 2))[:n]


def round_half_away(t):
    """fp32 -> the bf16 grid with ties AWAY from zero (what a `+ 0x8000, truncate` convert does), as float64; finite input."""
    bits = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    out = ((bits + 0x8000) & 0xFFFF0000).to(torch.int64)
    out = torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32)
    return out.view(torch.float32).double()


def seam_positions(n):
    out = []
    for p in SEAMS:
        p = n - 1 if p < 0 else p
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


def plant(t, axis, red, rot=0, classes=SPECIAL_CLASSES, tie_signs=None):
    """(planted, where): a copy of t [rows, cols] with one special LINE per seam position; axis = 0: the lines are rows
    t[p, :], axis = 1: columns t[:, p]; `red`: the index along the line of the single element the *_elem classes change.
    tie_signs: the signs of the tie lines (tie_line).  where: dict position -> class; class c goes to the (c + rot)-th position, cyclically, as seed_kernel_edges.special_rows."""
    planted = t.clone()
    view = planted if axis == 0 else planted.t()                # view[p] is line p
    n = view.shape[1]
    where = {}
    for i, p in enumerate(seam_positions(view.shape[0])):
        cls = classes[(i + rot) % len(classes)]
        where[p] = cls
        if cls == "nan_elem":
            view[p, red] = float("nan")
        elif cls == "pos_inf_elem":
            view[p, red] = float("inf")
        elif cls == "neg_inf_elem":
            view[p, red] = float("-inf")
        elif cls == "flt_max_elem":
            view[p, red] = FLT_MAX
        elif cls == "two126_elem":
            view[p, red] = TWO126
        elif cls == "ties":
            view[p] = tie_line(n, tie_signs)
        elif cls == "neg_zero":
            view[p] = -0.0
        elif cls == "denormal":
            view[p] = denormal_line(n)
        else:
            raise ValueError(cls)
    return planted, where


_bases = {}


def special_base(layout):
    """(x, W, b, g) of SPECIAL_SHAPES[layout]: the randn tensors of case() with x and g scaled by 1/8 (exact), so that every
    element of every operand is below 1 in magnitude and a single 2^126 cannot overflow an fp32 sum."""
    if layout not in _bases:
        c = case(*SPECIAL_SHAPES[layout])
        _bases[layout] = (c["x"] / 8, c["W"], c["b"], c["g"] / 8)
    return _bases[layout]


def product64(layout, A, B):
    """(C, R) in float64 from the bf16-rounded operands; IEEE specials propagate as IEEE says."""
    Ar, Br = rb(A), rb(B)
    if layout == "NT":
        return Ar @ Br.t(), Ar.abs() @ Br.abs().t()
    if layout == "NN":
        return Ar @ Br, Ar.abs() @ Br.abs()
    return Ar.t() @ Br, Ar.abs().t() @ Br.abs()


def operands(layout, x, W, g):
    """(A, B, axis of A's lines, axis of B's lines) of the layout."""
    return {"NT": (x, W, 0, 0), "NN": (g, W, 0, 1), "TN": (g, x, 1, 1)}[layout]


def agrees(got, want, bound):
    """Elementwise: where `want` is finite, |got - want| <= bound; where it is +-Inf, got is the same Inf; where NaN, NaN."""
    got = got.double()
    fin = torch.isfinite(want)
    ok_fin = (got - want).abs() <= bound
    ok_inf = got == want
    ok_nan = torch.isnan(got)
    return torch.where(fin, ok_fin, torch.where(torch.isnan(want), ok_nan, ok_inf))
