"""Case builders for tests/test_gpu_backward_extent.py (and the draws tests/test_gpu_backward.py shares with it): exact-integer
weight-gradient operands, the three-layer backward's inputs, the maps of what one planted NaN / Inf must and must not reach, and
the parameter lists of the GPU file.  Pure numpy / CPU torch: nothing here touches the GPU or the library, and
tests/test_backward_edge_cases_host.py checks every builder on a machine without one.
"""
from __future__ import annotations

import functools

import torch

import backward_ref as R

ACT_NONE, ACT_GELU, ACT_SIGMOID, ACT_RELU = R.ACT_NONE, R.ACT_GELU, R.ACT_SIGMOID, R.ACT_RELU
ENC = (ACT_GELU, ACT_GELU, ACT_SIGMOID)                # LLFQVAE_V4's encoder
DEC = (ACT_GELU, ACT_GELU, ACT_NONE)                   # its decoder: pre2 = None, g2 is gy
RELU3 = (ACT_RELU, ACT_RELU, ACT_RELU)                 # the plain VQVAE's stacks
MIX = (ACT_RELU, ACT_SIGMOID, ACT_GELU)
LDS_ROWS = 65536                                       # LQ_MLP3_LDS_ROWS of csrc/lipvq_mlp.hip
LDS_N = LDS_ROWS + 45                                  # ... plus a ragged tile

# ---------------------------------------------------------------------------------------------------------------------------
# weight gradient: rows at which the chunking of csrc/lipvq_bwd.hip changes
# ---------------------------------------------------------------------------------------------------------------------------
WGRAD_GROUPS = 32                                      # WGR_GROUPS: chunk groups of wgrad_reduce_kernel


def wgrad_chunk_rows(N):
    """wgrad_chunk_rows of csrc/lipvq_bwd.hip, restated."""
    if N <= 128:
        return 128
    return 1024 if N >= 262144 else (256 if N >= 16384 else 64)


def wgrad_chunks(N):
    c = wgrad_chunk_rows(N)
    return (N + c - 1) // c


CHUNK_N = (
    128,              # `if (N <= 128) return 128`: the last one-chunk batch, written directly (no reduce launch)
    129,              # ... the first with 64-row chunks: 3 chunks (64 + 64 + 1) and the reduce
    64 * 31 + 1,      # 32 chunks: `for (; c < nchunks; c += WGR_GROUPS)` -- every one of the 32 groups sums exactly one chunk
    64 * 32,          # 32 chunks, the last one whole
    64 * 32 + 1,      # 33 chunks: group 0 sums two (c = 0, 32), the others one
    64 * 96,          # 96 chunks: `c + 3 * WGR_GROUPS < nchunks` holds for no group: the tail loop alone, three trips each
    64 * 96 + 1,      # 97 chunks: group 0 (0 + 96 < 97) takes ONE trip of the four-way unrolled loop, the other groups the tail loop
    64 * 97 + 1,      # 98 chunks: groups 0 and 1 take the unrolled trip
    16383,            # `N >= 16384 ? 256 : 64`: the last batch with 64-row chunks (256 of them, the last with 63 rows)
    16384,            # ... the first with 256-row chunks (64 chunks)
    16385,            # 65 chunks, the last with one row
    262143,           # `N >= 262144 ? 1024 : ...`: the last batch with 256-row chunks (1024 chunks: eight unrolled trips per group)
    262144,           # ... the first with 1024-row chunks (256 chunks)
    262145,           # 257 chunks, the last with one row: group 0 takes two unrolled trips and one tail step
)
EXACT_JK = ((32, 32), (64, 100))
GATHER_MAX_N = 16385
# (N, J, Kd, h_act, gather)
EXACT_SUM_CASES = [(n, j, k, act, gather) for n in CHUNK_N for j, k in EXACT_JK for act in (ACT_NONE, ACT_RELU)
                   for gather in (False, True) if not gather or n <= GATHER_MAX_N]


@functools.lru_cache(maxsize=2)
def integer_wgrad_case(N, J, Kd, seed, gather=False):
    """Operands whose weight gradient is exact in fp32 in ANY summation order: G in [-2, 2], H in [-3, 3], integers stored as
    fp32, so every product is an integer of magnitude <= 6 and every partial sum one of magnitude <= 6 N < 2^24.  Column 0 of
    both is 1: gb[0] == gW[0][0] == N counts every row exactly once.  With gather, H is a 50-row table and hidx picks rows
    0, 3, ..., 27 (repeated; the others unused, and filled with 1e30 so that a stray read shows).
    Returns a dict of CPU tensors: G [N, J], H ([N, Kd] or the table), hidx (or None), and the int64 references
    gW[act] = G^T act(H) for act in (ACT_NONE, ACT_RELU) and gb = column sums of G."""
    assert 6 * N < 2 ** 24, "partial sums must stay exactly representable in fp32"
    g = torch.Generator().manual_seed(seed)
    Gi = torch.randint(-2, 3, (N, J), generator=g)
    Gi[:, 0] = 1
    hidx = None
    if gather:
        table = torch.randint(-3, 4, (50, Kd), generator=g)
        table[:, 0] = 1
        hidx = torch.randint(0, 10, (N,), generator=g) * 3
        Hi = table[hidx]
        used = torch.zeros(50, dtype=torch.bool)
        used[::3][:10] = True
        H = table.float()
        H[~used] = 1e30
    else:
        Hi = torch.randint(-3, 4, (N, Kd), generator=g)
        Hi[:, 0] = 1
        H = Hi.float()
    Gt = Gi.t().contiguous()
    gW = {ACT_NONE: Gt @ Hi, ACT_RELU: Gt @ Hi.clamp(min=0)}
    return {"G": Gi.float(), "H": H, "hidx": hidx, "gW": gW, "gb": Gi.sum(0)}


# write extent: (J, Kd, family) at N in WGRAD_EXTENT_N -- 1, 33, 128: one chunk, the kernel's tile-shaped slab IS the result;
# 129: three chunks and the reduce
WGRAD_EXTENT_SHAPES = (
    (196, 100, "wg5 7x4 tiles, 32-row blocks, ragged both ways"), (7, 128, "wg5 1x4, element loads of G"),
    (64, 7, "wg5 2x1, element loads of H"), (224, 224, "wg5 7x7"),
    (66, 130, "wgrad_wg_kernel: J & 3 != 0 at more than one tile"),
    (320, 100, "wgrad_kernel: ten row tiles, one wave per tile"),
    (512, 64, "wide: four column blocks of 128, gridDim.y = 4"), (384, 32, "wide: gridDim.y = 3"),
)
WGRAD_EXTENT_N = (1, 33, 128, 129)
# (N, J, Kd, mode): plain | nobias (gb = NULL) | misaligned (G, H 4 bytes off) | offset_out (gW, gb, workspace 4 bytes off: every
# wgrad kernel stores its slab and wgrad_reduce_kernel its sums one element at a time, so no output alignment is assumed)
WGRAD_EXTENT_CASES = [(n, j, k, "plain") for j, k, _ in WGRAD_EXTENT_SHAPES for n in WGRAD_EXTENT_N]
WGRAD_EXTENT_CASES += [(128, 196, 100, "nobias"), (129, 196, 100, "nobias"), (129, 196, 100, "misaligned"), (33, 64, 128, "misaligned"),
                       (128, 196, 100, "offset_out"), (129, 66, 130, "offset_out"), (129, 512, 64, "offset_out")]

POISON_N = (100, 129, 4097)
POISON_JK = ((196, 100), (66, 130))


def poison_rows(N):
    """Row 0, the last row of a chunk, the first of the next, the last row of the batch (deduplicated, in range)."""
    c = wgrad_chunk_rows(N)
    rows = []
    for r in (0, min(c, N) - 1 if N > c else N // 2, min(c, N - 1), N - 1):
        if 0 <= r < N and r not in rows:
            rows.append(r)
    return rows


def wgrad_case(N, J, Kd, seed):
    """Random normal (G [N, J], H [N, Kd]) fp32 CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, J, generator=g), torch.randn(N, Kd, generator=g)


def wgrad_poison_map(G, H, n, h_act=ACT_NONE):
    """What the non-finite entries of row n of (G, H) must do to (gW, gb) = (G^T act(H), column sums of G), from the definition
    alone: every element of gW is a sum over the rows, and only row n's term G[n, j] act(H[n, k]) can be non-finite (every other
    operand is finite), so the element is NaN where that term is NaN, +-Inf where it is +-Inf, and otherwise does not depend on
    the planted value at all.  Returns float64 (classW [J, Kd], classb [J]): NaN / +Inf / -Inf where the output must be exactly
    that, 0 where it must keep the bits of the clean run."""
    g, h = R.f64(G[n]), R.act_ref(H[n], h_act)
    term = g[:, None] * h[None, :]
    classW = torch.where(torch.isfinite(term), torch.zeros_like(term), term)
    classb = torch.where(torch.isfinite(g), torch.zeros_like(g), g)
    return classW, classb


def assert_follows_poison_map(got, clean, cls, name):
    """got == cls where cls is NaN / +-Inf, got is bit-identical to clean elsewhere (CPU tensors)."""
    got, clean = got.detach().cpu(), clean.detach().cpu()
    hit = cls != 0                                              # NaN != 0 is True
    assert torch.equal(torch.isnan(got), torch.isnan(cls)), f"{name}: the NaN set differs from the map"
    inf = torch.isinf(cls)
    assert torch.equal(got[inf].double(), cls[inf]), f"{name}: the +-Inf elements differ from the map"
    assert torch.equal(got[~hit].view(torch.int32), clean[~hit].view(torch.int32)), f"{name}: an element outside the map changed"


# ---------------------------------------------------------------------------------------------------------------------------
# the three-layer backward
# ---------------------------------------------------------------------------------------------------------------------------
def plant(t, salt):
    """backward_ref.PLANTED (+-0, +-9, +-40, +-100) at scattered positions of a pre-activation tensor; returns the flat positions."""
    flat = t.view(-1)
    pos = [(salt + 37 * k) % flat.numel() for k in range(len(R.PLANTED))]
    for q, v in zip(pos, R.PLANTED):
        flat[q] = float(v)
    return pos


def mlp3_inputs(N, K0, J0, J1, J2, acts, seed):
    """(W0, W1, W2, gy, [pre0, pre1, pre2 or None], zero_row): the draws of tests/test_gpu_backward.py."""
    g = torch.Generator().manual_seed(seed)
    W0 = torch.randn(J0, K0, generator=g) * 0.3
    W1 = torch.randn(J1, J0, generator=g) * 0.2
    W2 = torch.randn(J2, J1, generator=g) * 0.2
    gy = torch.randn(N, J2, generator=g)
    pre = [torch.randn(N, J, generator=g) * 2.0 for J in (J0, J1, J2)]
    for i, p in enumerate(pre):
        plant(p, 3 + i)
    zero_row = N // 2 if N >= 3 else None                   # one row of all zeros in gy (its gradients must be exactly 0)
    if zero_row is not None:
        gy[zero_row] = 0.0
    if acts[2] == ACT_NONE:
        pre[2] = None
    return W0, W1, W2, gy, pre, zero_row


@functools.lru_cache(maxsize=2)
def mlp3_bwd_case(N, K0, J0, J1, J2, acts, seed=None):
    """mlp3_inputs as a dict, seeded from the shape (shared, read-only: tests clone what they change)."""
    seed = N * 131 + K0 * 17 + J0 + 3 * J1 + 7 * J2 if seed is None else seed
    W0, W1, W2, gy, pre, zero_row = mlp3_inputs(N, K0, J0, J1, J2, acts, seed)
    return {"W": (W0, W1, W2), "gy": gy, "pre": pre, "zero_row": zero_row, "acts": acts, "dims": (N, K0, J0, J1, J2)}


def mlp3_poison_map(case, row, col):
    """NaN planted at gy[row, col]: boolean (g2 [N, J2], g1 [N, J1], g0 [N, J0], gx [N, K0]) masks of the elements that must be
    NaN -- every other element must keep the bits of the clean run.  From the definition (backward_ref.mlp3_bwd_ref in float64):
    the chain works row by row, so only row `row` is evaluated with the planted value; all other rows are untouched by it."""
    N, K0, J0, J1, J2 = case["dims"]
    gy = case["gy"][row:row + 1].clone()
    gy[0, col] = float("nan")
    pre = [None if p is None else p[row:row + 1] for p in case["pre"]]
    out = R.mlp3_bwd_ref(gy, pre, *case["W"], case["acts"])
    masks = []
    for o, width in zip(out, (J2, J1, J0, K0)):
        m = torch.zeros(N, width, dtype=torch.bool)
        m[row] = torch.isnan(o[0])
        masks.append(m)
    return masks


# (name, (N, K0, J0, J1, J2, acts)): one case per kernel the comments of tests/test_gpu_backward.py::MLP3_CASES name
MLP3_KERNEL_CASES = {
    "wg1": (33, 7, 64, 128, 5, ENC),                     # mlp3_wg_kernel<true, 1>: N < 4096
    "wg2": (4097, 7, 64, 128, 64, ENC),                  # mlp3_wg_kernel<true, 2>: N >= 4096, 2 * plane <= 80 KiB
    "lds": (LDS_N, 7, 64, 128, 64, ENC),                 # mlp3_lds_kernel<2, 4, true, 0>
    "fallback": (70, 7, 64, 128, 971, ENC),              # mlp3_kernel<4, 2, true>: the chain's input plane exceeds 150 KiB
}
# (name, dims, mode): plain | no_g2 (identity output layer) | no_gx | offset_out (every output 4 bytes off a 16-byte boundary: all
# three kernels test pointer and row stride -- al16 in mlp3_wg_kernel / mlp3_lds_kernel -- before a 16-byte store, mlp3_kernel and the
# g2 store of mlp3_wg_kernel store single elements)
MLP3_EXTENT_CASES = [(f"wg1 K0={k0}", (33, k0, 64, 128, 5, ENC), "plain") for k0 in (1, 3, 7, 209)]
MLP3_EXTENT_CASES += [(k, MLP3_KERNEL_CASES[k], "plain") for k in ("wg2", "lds", "fallback")]
MLP3_EXTENT_CASES += [
    ("wg1 identity output, g2 given: a copy of gy", (33, 64, 64, 128, 7, DEC), "plain"),
    ("lds identity output, g2 given: a copy of gy", (LDS_N, 64, 64, 128, 7, DEC), "plain"),
    ("wg1 identity output, g2 = NULL", (33, 64, 64, 128, 7, DEC), "no_g2"), ("lds identity output, g2 = NULL", (LDS_N, 64, 64, 128, 7, DEC), "no_g2"),
    ("wg1 gx = NULL", (33, 7, 64, 128, 5, ENC), "no_gx"), ("lds gx = NULL", (LDS_N, 7, 64, 128, 64, ENC), "no_gx"),
    ("wg1 outputs 4 bytes off", (33, 64, 64, 128, 64, ENC), "offset_out"), ("wg2 outputs 4 bytes off", (4097, 64, 64, 128, 64, ENC), "offset_out"),
    ("lds outputs 4 bytes off", (LDS_N, 64, 64, 128, 64, ENC), "offset_out"), ("fallback outputs 4 bytes off", (70, 8, 64, 128, 972, ENC), "offset_out"),
]


def mlp3_isolation_rows(N):
    """First and last row of a 32-row tile, the first of the second sub-tile of a 64-row workgroup, the last row of the batch."""
    rows = []
    for r in (0, 31, 32, N - 1):
        if 0 <= r < N and r not in rows:
            rows.append(r)
    return rows


MLP3_ISOLATION_CASES = [("wg1", (70, 7, 64, 128, 5, ENC)), ("wg2", MLP3_KERNEL_CASES["wg2"]), ("lds", MLP3_KERNEL_CASES["lds"]),
                        ("fallback", MLP3_KERNEL_CASES["fallback"])]
MLP3_PERMUTATION_CASES = [(70, 7, 64, 128, 64, ENC), (4097, 7, 64, 128, 64, ENC), (LDS_N, 7, 64, 128, 64, ENC), (LDS_N, 64, 128, 64, 7, RELU3)]

# lipvq_mlp3_bwd_vq_f32: (term, A given as, B given as) -- the input term's A is always the forward's own output
VQ_FORMS = [("in", None, "rows"), ("in", None, "table"), ("out", "rows", "rows"), ("out", "rows", "table"),
            ("out", "table", "rows"), ("out", "table", "table")]
VQ_DIMS = {"in": (7, 64, 128, 64, ENC), "out": (64, 128, 64, 7, RELU3)}        # (K0, J0, J1, J2, acts): the two stacks that use it
VQ_TABLE_ROWS = 300


def vq_case(term, seed):
    """Weights, input rows and the difference term's operands for one lipvq_mlp3_bwd_vq_f32 case at N = LDS_ROWS (CPU fp32)."""
    K0, J0, J1, J2, acts = VQ_DIMS[term]
    N = LDS_ROWS
    g = torch.Generator().manual_seed(seed)
    case = {"dims": (N, K0, J0, J1, J2), "acts": acts,
            "W": (torch.randn(J0, K0, generator=g) * 0.3, torch.randn(J1, J0, generator=g) * 0.2, torch.randn(J2, J1, generator=g) * 0.2),
            "b": tuple(torch.randn(J, generator=g) * 0.1 for J in (J0, J1, J2)),
            "x": torch.randn(N, K0, generator=g), "gy": torch.randn(N, J2, generator=g)}
    width = J2 if term == "in" else K0
    for nm in ("a", "b_op"):
        case[nm + "_table"] = torch.rand(VQ_TABLE_ROWS, width, generator=g)
        case[nm + "_idx"] = torch.randint(0, VQ_TABLE_ROWS, (N,), generator=g)
    return case


# ---------------------------------------------------------------------------------------------------------------------------
# elementwise and small kernels: sizes on both sides of each block and grid-stride edge (constants of the kernels' launches)
# ---------------------------------------------------------------------------------------------------------------------------
ACT_BWD_BLOCK, ACT_BWD_PER_BLOCK, ACT_BWD_CAP = 256, 256 * 4, 4096       # lipvq_act_bwd_f32: stream_grid(n, 256 * 4, 4096) blocks of 256
ACT_BWD_N = (1, ACT_BWD_BLOCK - 1, ACT_BWD_BLOCK, ACT_BWD_BLOCK + 1, ACT_BWD_PER_BLOCK, ACT_BWD_PER_BLOCK + 1,
             ACT_BWD_PER_BLOCK * ACT_BWD_CAP, ACT_BWD_PER_BLOCK * ACT_BWD_CAP + 1, ACT_BWD_PER_BLOCK * ACT_BWD_CAP + ACT_BWD_BLOCK * ACT_BWD_CAP + 3)
SDIFF_BLOCK, SDIFF_CAP = 256, 2048                                       # lipvq_scaled_diff_f32: ceil(n / 256) blocks, at most 2048
SDIFF_N = (1, SDIFF_BLOCK - 1, SDIFF_BLOCK, SDIFF_BLOCK + 1, SDIFF_BLOCK * SDIFF_CAP, SDIFF_BLOCK * SDIFF_CAP + 1, 2 * SDIFF_BLOCK * SDIFF_CAP + 3)
LIPB_ROWS, LIPB_HMAX, LIPB_THREADS = 16, 256, 256                        # lipschitz_bwd_kernel: 16 rows a workgroup, 256 threads over 16 H
LIPB_DH = [(d, h) for d in (1, LIPB_ROWS - 1, LIPB_ROWS, LIPB_ROWS + 1, 2 * LIPB_ROWS + 1)
           for h in (1, LIPB_THREADS // LIPB_ROWS - 1, LIPB_THREADS // LIPB_ROWS, LIPB_THREADS // LIPB_ROWS + 1, LIPB_HMAX - 1, LIPB_HMAX)]

SPECTRAL_MAX = 256                                                       # lipvq_spectral_norm_f32: J, K <= 256
SPECTRAL_JK = ((1, 1), (1, 256), (256, 1), (255, 256), (256, 256), (64, 7))
SPECTRAL_REFUSED = ((SPECTRAL_MAX + 1, 8), (8, SPECTRAL_MAX + 1))
SPECTRAL_EPS = 1e-12


def spectral_case(J, K, seed, kind="random"):
    """Dict of fp32 CPU tensors W [J, K], u [J], v [K] (unit norm), gWsn [J, K].  kind: random | rank_one (W = p q^T: one power
    iteration lands on its singular vectors and sigma is |p| |q|, returned as sigma_exact in float64) | zero."""
    g = torch.Generator().manual_seed(seed)
    case = {"W": torch.randn(J, K, generator=g),
            "u": torch.nn.functional.normalize(torch.randn(J, generator=g), dim=0),
            "v": torch.nn.functional.normalize(torch.randn(K, generator=g), dim=0),
            "gWsn": torch.randn(J, K, generator=g)}
    if kind == "rank_one":
        p, q = torch.randn(J, generator=g).double() * 1.5, torch.randn(K, generator=g).double()
        case["W"] = torch.outer(p, q).float()
        case["sigma_exact"] = float(p.norm() * q.norm())
    elif kind == "zero":
        case["W"] = torch.zeros(J, K)
    return case


def spectral_ref_and_budget(W, u, v, training, eps=SPECTRAL_EPS):
    """float64 restatement of torch.nn.utils.spectral_norm's compute_weight (as tests/test_gpu_default.py::
    test_spectral_norm_and_backward) and the allowed |error| of an fp32 evaluation whose reductions are sequential fma chains.

    With u = 2^-24, gamma_L = backward_ref.gamma(L), a chain of length L over |x|.|y| errs by at most gamma_L |x|.|y| (dot_bound).
    Error propagation, first order, every input error carried through the exact float64 linear maps:
        d(W^T u)  = gamma_J |W|^T |u|                                                   (u as given: exact)
        n_v = |W^T u|:   d(n_v) <= |d(W^T u)|_2 + (gamma_K + 2 u) n_v                    (chain of squares, the root)
        d(v)      = d(W^T u) / n_v + |v| (d(n_v) / n_v + u)                             (the division)
        d(W v)    = gamma_K |W| |v| + |W| d(v)
        d(u)      likewise from d(W v) and n_u = |W v|
        d(sigma)  = gamma_J |u|.|Wv| + |u|.d(Wv) + d(u).|Wv|
        d(Wsn)    = |Wsn| (d(sigma) / |sigma| + u)                                      (one division)
    In eval mode d(v) = d(u) = 0.  Returns a dict of float64 refs and budgets."""
    Wd, ud, vd = R.f64(W), R.f64(u), R.f64(v)
    J, K = Wd.shape
    aW = Wd.abs()
    d_u, d_v = torch.zeros_like(ud), torch.zeros_like(vd)
    if training:
        wu = Wd.t() @ ud
        d_wu = R.gamma(J) * (aW.t() @ ud.abs())
        n = wu.norm()
        d_n = d_wu.norm() + (R.gamma(K) + 2 * R.U32) * n
        nc = n.clamp(min=eps)
        vd = wu / nc
        d_v = d_wu / nc + vd.abs() * (d_n / nc + R.U32)
    wv = Wd @ vd
    d_wv = R.gamma(K) * (aW @ vd.abs()) + aW @ d_v
    if training:
        n = wv.norm()
        d_n = d_wv.norm() + (R.gamma(J) + 2 * R.U32) * n
        nc = n.clamp(min=eps)
        ud = wv / nc
        d_u = d_wv / nc + ud.abs() * (d_n / nc + R.U32)
    sigma = torch.dot(ud, wv)
    d_sigma = R.gamma(J) * torch.dot(ud.abs(), wv.abs()) + torch.dot(ud.abs(), d_wv) + torch.dot(d_u, wv.abs()) + R.ulp32(sigma)
    Wsn = Wd / sigma
    d_Wsn = Wsn.abs() * (d_sigma / sigma.abs() + R.U32) + R.ulp32(Wsn)
    return {"u": ud, "v": vd, "sigma": sigma, "Wsn": Wsn, "d_u": d_u + R.ulp32(ud), "d_v": d_v + R.ulp32(vd), "d_sigma": d_sigma, "d_Wsn": d_Wsn}


def spectral_bwd_ref_and_budget(gWsn, Wsn, u, v, sigma):
    """gW = (gWsn - <gWsn, Wsn> u v^T) / sigma from the KERNEL's own (Wsn, u, v, sigma), in float64, and the allowed |error|: the
    inner product is summed in double and rounded once (u |dot|, and u sum|gWsn Wsn| for any order of the double sum's own 2^-53
    terms is far below that), then two products, one difference and one division in fp32."""
    g, Ws, ud, vd, sg = R.f64(gWsn), R.f64(Wsn), R.f64(u), R.f64(v), float(R.f64(sigma).reshape(-1)[0])
    dot = (g * Ws).sum()
    uv = torch.outer(ud, vd)
    ref = (g - dot * uv) / sg
    allowed = (R.U32 * dot.abs() * uv.abs() + 2 * R.U32 * (dot * uv).abs() + R.U32 * (g - dot * uv).abs()) / abs(sg) + R.U32 * ref.abs() + R.ulp32(ref)
    return ref, allowed


def value_class(t):
    """0 finite non-zero, 1 zero, 2 NaN, 3 +Inf, 4 -Inf, elementwise (int8 CPU tensor)."""
    t = t.detach().cpu().double()
    c = torch.zeros(t.shape, dtype=torch.int8)
    c[t == 0] = 1
    c[torch.isnan(t)] = 2
    c[t == float("inf")] = 3
    c[t == float("-inf")] = 4
    return c
