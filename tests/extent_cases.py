"""The large-extent cases of tests/test_gpu_large_extent.py, described once and checked without a GPU by
tests/test_extent_cases_host.py: one operand of every case crosses element offset 2^31 (byte offset 2^33), and with it element offset
2^30 = byte offset 2^32, the first address a 32-bit byte offset cannot reach.

Row count.  An operand [N, W] has N = 2^31 // W + 2 * 256 + 37 rows: the largest workgroup tile of the library is 256 rows, so
at least one complete tile of every kernel lies wholly past element 2^31, and the last tile is ragged (37 is odd and prime).

Windows.  Rows 0..63, 64 rows on each side of every boundary row (boundary // W), the last 101 rows.  The fine checks (float64
or the canonical oracle) read the window rows only; the whole-tensor checks compare bits on the device.

Exact-sum operands.  Reductions over rows are checked bit for bit: ``exact_rows`` gives integers |v| <= 8 (exact in bf16 too) on
the window rows, the operand is zero elsewhere; ``count`` operands are ones on EVERY row with r % 8 == 0.  The host test proves with
int64 arithmetic that the sum of the absolute values of all terms of every output element stays below 2^24: every partial sum in any
order is then an integer fp32 holds exactly, and the fp32 result must equal the int64 answer.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

B30, B31, B32 = 1 << 30, 1 << 31, 1 << 32
TILE_ROWS = 256                       # the largest row tile of any kernel of the library (linear_big_kernel<4, 1>)
CHUNK_ELEMS = 1 << 26                 # an extent the small-shape suite covers: the chunked calls stay at or below it
MEM_CAP = 48 << 30                    # declared device bytes of one case
EXACT = 1 << 24                       # integers below this are exact in fp32
FLAT_TAIL = 4099                      # flat kernels: 2^31 + 4099 and 2^32 + 4099 elements
FENCE_BYTES = 2 * 1024 * 4            # tests/fenced.py: PAD words of sentinel on each side


def rows_for(W, boundary=B31):
    return boundary // W + 2 * TILE_ROWS + 37


def windows(N, W, boundaries=(B30, B31)):
    """[(first row, end row)]: the head, 64 rows on each side of every boundary row, the last 101 rows."""
    out = [(0, 64)]
    for b in boundaries:
        r = b // W
        out.append((r - 64, r + 64))
    out.append((N - 101, N))
    return out


def window_rows(N, W, boundaries=(B30, B31)):
    """All window rows, ascending, as an int64 array."""
    return np.unique(np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in windows(N, W, boundaries)]))


def chunk_rows(W):
    """Rows of one chunked call: at most CHUNK_ELEMS elements, a multiple of the largest tile."""
    return max(TILE_ROWS, CHUNK_ELEMS // W // TILE_ROWS * TILE_ROWS)


def exact_values(rows, W, salt):
    """int64 [len(rows), W]: the integer in [-8, 8] at (row, col) of the exact-sum operand `salt` -- a closed form, so the device
    (torch, the same expression) and the host agree without copying anything."""
    r = np.asarray(rows, np.int64)[:, None]
    c = np.arange(W, dtype=np.int64)[None, :]
    return (r * 131 + c * 71 + salt * 29 + (r * c) % 7) % 17 - 8


def count_rows(N):
    """Rows of a count operand that hold ones: every row with r % 8 == 0."""
    return np.arange(0, N, 8, dtype=np.int64)


def scatter_code(rows, K):
    """The code of a row in the scatter cases: spread, a closed form."""
    r = np.asarray(rows, np.int64)
    return (r * 5 + r // 64 + 3) % K


@dataclass(frozen=True)
class Case:
    name: str                     # test id
    entry: str                    # the C entry point of the big call
    N: int                        # rows of the big operand
    W: int                        # its width in elements
    allocs: tuple                 # ((what, bytes), ...): every device allocation the test holds at its peak
    boundaries: tuple = (B30, B31)
    dims: tuple = ()              # the other sizes of the call, as the entry point takes them
    p: float = 0.0                # dropout probability (cases of the in-kernel source)

    @property
    def need(self):
        return sum(b for _, b in self.allocs)

    @property
    def elems(self):
        return self.N * self.W


F4 = 4
_CHUNK = 2 * CHUNK_ELEMS * F4 * 2            # chunk results and their comparison temporaries


def _big(N, W, n=1, item=F4, fenced=0):
    return n * N * W * item + fenced * FENCE_BYTES


def _linear_cases():
    N = rows_for(2048)
    out = []
    for tag, Kin in (("k8", 8), ("k6", 6)):          # Kin % 4 != 0 keeps the call on linear_kernel, Kin = 8 takes linear_big_kernel
        out.append(Case(f"linear_wide_out_{tag}", "lipvq_linear_act_f32", N, 2048,
                        (("x", _big(N, Kin)), ("y, pre (fenced)", _big(N, 2048, 2, fenced=2)), ("chunks", _CHUNK)), dims=(Kin, 2048)))
    out.append(Case("linear_wide_in", "lipvq_linear_act_f32", N, 2048,
                    (("x", _big(N, 2048)), ("y, pre (fenced)", _big(N, 8, 2, fenced=2)), ("chunks", _CHUNK)), dims=(2048, 8)))
    # the bf16 and bf16x3 matrix-pipe modes (one case each: the two modes run the same kernels, arguments and limits).  Their only
    # width rule is "a multiple of 8": the widest LEGAL width is unbounded, so the cases take the widest width the policy has (the MLP
    # hidden 4 E = 2048; a wider row only lowers N = 2^31 // W) against the narrowest legal one, 8
    out.append(Case("linear_pipe_wide_out", "lipvq_linear_act_bf16", N, 2048,
                    (("x", _big(N, 8)), ("y, pre (fenced)", _big(N, 2048, 2, fenced=2)), ("chunks", _CHUNK)), dims=(8, 2048)))
    out.append(Case("linear_pipe_wide_in", "lipvq_linear_act_bf16", N, 2048,
                    (("x", _big(N, 2048)), ("y, pre (fenced)", _big(N, 8, 2, fenced=2)), ("chunks", _CHUNK)), dims=(2048, 8)))
    out.append(Case("linear_nn_pipe", "lipvq_linear_nn_bf16", N, 2048,
                    (("g", _big(N, 2048)), ("gx (fenced)", _big(N, 8, fenced=1)), ("chunks", _CHUNK)), dims=(2048, 8)))
    out.append(Case("linear_drop", "lipvq_linear_act_drop_f32", N, 2048,
                    (("x", _big(N, 8)), ("y, pre (fenced)", _big(N, 2048, 2, fenced=2)), ("keep bytes", _big(N, 2048, item=1)), ("chunks", 2 * _CHUNK)),
                    dims=(8, 2048), p=0.3))
    out.append(Case("act_bwd_drop", "lipvq_act_bwd_drop_f32", N, 2048,
                    (("g, pre", _big(N, 2048, 2)), ("out (fenced)", _big(N, 2048, fenced=1)), ("keep bytes", _big(N, 2048, item=1)),
                     ("chunks", 2 * _CHUNK)), dims=(2048,), p=0.3))
    return out


def _keep_cases():
    N = rows_for(2048, B32)                      # bytes: the windows sit at byte 2^31 and byte 2^32
    return [Case("dropout_keep", "lipvq_dropout_keep_u8", N, 2048, (("field (fenced)", _big(N, 2048, item=1, fenced=1)), ("chunks", _CHUNK)),
                 boundaries=(B31, B32), dims=(2048,), p=0.25)]


def _layernorm_cases():
    N = rows_for(1024)
    return [Case("layernorm_b_s", "lipvq_gpt_layernorm_f32", N, 1024, (("a, b", _big(N, 1024, 2)), ("s, y (fenced)", _big(N, 1024, 2, fenced=2)),
                                                                       ("chunks", _CHUNK)), dims=(1024,)),
            Case("layernorm_save", "lipvq_gpt_layernorm_f32", N, 1024, (("a", _big(N, 1024)), ("y, xhat (fenced)", _big(N, 1024, 2, fenced=2)),
                                                                        ("rstd", N * F4), ("chunks", _CHUNK)), dims=(1024,)),
            Case("layernorm_drop", "lipvq_gpt_layernorm_drop_f32", N, 1024,
                 (("a, b", _big(N, 1024, 2)), ("y (fenced)", _big(N, 1024, fenced=1)), ("keep bytes", _big(N, 1024, item=1)), ("chunks", 2 * _CHUNK)),
                 dims=(1024,), p=0.2),
            Case("layernorm_bwd", "lipvq_gpt_layernorm_bwd_f32", N, 1024,
                 (("gy, xhat", _big(N, 1024, 2)), ("gs (fenced)", _big(N, 1024, fenced=1)), ("rstd", N * F4), ("chunks", _CHUNK)), dims=(1024,)),
            Case("layernorm_bwd_drop", "lipvq_gpt_layernorm_bwd_drop_f32", N, 1024,
                 (("gy, xhat", _big(N, 1024, 2)), ("gs, gbranch (fenced)", _big(N, 1024, 2, fenced=2)), ("rstd", N * F4),
                  ("keep bytes", _big(N, 1024, item=1)), ("chunks", 2 * _CHUNK)), dims=(1024,), p=0.2)]


EMBED_T, EMBED_E = 10, 1024


def _embed_cases():
    """The embedding stage's interleave (out [B][3 T][E], three calls fill every slot): B batches so that the output has at least
    rows_for(E) rows of E floats -- the largest slot lies past element 2^31.  N counts OUTPUT rows here; a call has B T input rows."""
    T, E = EMBED_T, EMBED_E
    B = -(-rows_for(E) // (3 * T))
    N = B * 3 * T
    return [Case("embed_rows", "lipvq_embed_rows_f32", N, E,
                 (("out (fenced)", _big(N, E, fenced=1)), ("dense rows", _big(B * T, E)), ("table, idx, stats", (1024 * E + 4 * B * T) * F4),
                  ("chunks", _CHUNK)), dims=(T, B)),
            # the backward on the same interleave: N counts rows of gout [B][3 T][E]
            Case("embed_rows_bwd", "lipvq_embed_rows_bwd_det_f32", N, E,
                 (("gout", _big(N, E)), ("dense rows, their gradient", _big(B * T, E, 2)), ("workspace (row gradients, partial sums, sort)", _big(B * T, E) + (256 << 20)),
                  ("table, its gradient, idx, stats", (2 * EMBED_K * E + 6 * B * T) * F4)), dims=(T, B))]


ATT_L, ATT_E = 128, 512


def _attention_cases():
    """qkv [B][L][3 E] past 2^31 elements: B whole sequences; N counts rows of 3 E floats.  H = 32 (head width 16): the keep bytes
    [B][H][L][L] pass 2^32 bytes as well; H = 8 (head width 64) runs without them.  The prefix form: 64 cached + 64 new tokens."""
    L, E = ATT_L, ATT_E
    W = 3 * E
    B = -(-rows_for(W) // L)
    N = B * L
    out, keep = _big(N, E), B * 32 * L * L
    B2 = -(-rows_for(W) // 64)
    N2 = B2 * 64
    return [Case("gpt_attention_dh16", "lipvq_gpt_attention_f32", N, W,
                 (("qkv", _big(N, W)), ("out, lse (fenced)", out + B * 32 * L * F4 + 2 * FENCE_BYTES), ("keep bytes", keep), ("gout", out),
                  ("gqkv, delta (fenced)", _big(N, W, fenced=2) + B * 32 * L * F4), ("the in-kernel source's out, lse, gqkv", out + B * 32 * L * F4 + _big(N, W)), ("chunks", 2 * _CHUNK)),
                 dims=(L, E, 32, B), p=0.1),
            Case("gpt_attention_dh64", "lipvq_gpt_attention_f32", N, W,
                 (("qkv", _big(N, W)), ("out, lse (fenced)", out + B * 8 * L * F4 + 2 * FENCE_BYTES), ("gout", out),
                  ("gqkv, delta (fenced)", _big(N, W, fenced=2) + B * 8 * L * F4), ("chunks", 2 * _CHUNK)), dims=(L, E, 8, B)),
            Case("gpt_attention_prefix", "lipvq_gpt_attention_prefix_f32", N2, W,
                 (("qkv, prefix_qkv", _big(N2, W, 2)), ("out (fenced)", _big(N2, E, fenced=1)), ("chunks", 2 * _CHUNK)), dims=(64, E, 32, B2))]


HEAD_M, HEAD_A = 2, 3


def _head_cases():
    """The policy's output heads on feats [N, 1024] (one sequence of N positions): every other operand has a few columns."""
    N = rows_for(1024)
    small = N * (HEAD_M * (2 * HEAD_A + 1) * 3 + 2 * HEAD_M * HEAD_A + HEAD_M + 6 * HEAD_A + 4) * F4
    return [Case("heads", "lipvq_gmm_head_f32", N, 1024, (("feats", _big(N, 1024)), ("per-row outputs, actions, noise", small), ("chunks", _CHUNK)),
                 dims=(HEAD_M, HEAD_A))]


BIN_A, BIN_NB = 7, 20


def _bin_cases():
    """The binning tokenizer: bin_discretize's [A][N] int64 output and bin_hidden's h [N, 256] past 2^31 elements."""
    Nd, Nh = rows_for(BIN_A), rows_for(256)
    return [Case("bin_discretize", "lipvq_bin_discretize_f32", Nd, BIN_A, (("actions", _big(Nd, BIN_A)), ("bins (int64)", _big(Nd, BIN_A, item=8)), ("chunks", _CHUNK)),
                 dims=(BIN_NB,)),
            Case("bin_hidden", "lipvq_bin_hidden_f32", Nh, 256, (("bins (int64)", _big(Nh, BIN_A, item=8)), ("h, pre (fenced)", _big(Nh, 256, 2, fenced=2)),
                                                                 ("chunks", _CHUNK)), dims=(BIN_NB,))]


EMBED_K = 1024


def embed_index(n):
    """The table row of input row n in the indexed embed_rows_bwd case: a closed form, spread over the EMBED_K rows."""
    n = np.asarray(n, np.int64)
    return (n * 7 + n // 13 + 5) % EMBED_K


def embed_bwd_expected(case, indexed):
    """The exact answer of lipvq_embed_rows_bwd_det_f32 on the exact-sum operands of the embed_rows case, as int64 NUMERATORS over
    E = 1024 (a power of two: the row means of the backward are dyadic, so every value of the kernel is numerator / 1024).
    gout [B][3 T][E] = exact_values(13) on the window OUTPUT rows, zero elsewhere; stats = (mean 0, rstd 1); ln_w = 1.
    indexed: slots b 3T + 2t + 1 (offset E, time stride 2 E), src = table exact_values(12) [EMBED_K] rows, pos = exact_values(14) // 4;
    dense:   slots b 3T + 2T + t (offset 2 T E, time stride E), src row n = exact_values(15) at n, no pos.
    Returns dict(rows n, gv [rows, E], g_pos [T, E], g_lnw, g_lnb, g_src (indexed: [EMBED_K, E]), bound = the largest sum of |term|
    numerators of any output element)."""
    T, B = case.dims
    E = case.W
    out_rows = window_rows(case.N, E)
    b, sl = out_rows // (3 * T), out_rows % (3 * T)
    if indexed:
        m = (sl < 2 * T) & (sl % 2 == 1)
        t = (sl[m] - 1) // 2
    else:
        m = sl >= 2 * T
        t = sl[m] - 2 * T
    n = b[m] * T + t
    g = exact_values(out_rows[m], E, 13)
    if indexed:
        xh = exact_values(embed_index(n), E, 12) + exact_values(t, E, 14) // 4
    else:
        xh = exact_values(n, E, 15)
    S1, S2 = g.sum(1, keepdims=True), (g * xh).sum(1, keepdims=True)
    gv = E * g - S1 - xh * S2
    g_pos, a_pos = np.zeros((T, E), np.int64), np.zeros((T, E), np.int64)
    np.add.at(g_pos, t, gv)
    np.add.at(a_pos, t, np.abs(gv))
    out = dict(n=n, t=t, gv=gv, g_pos=g_pos, g_lnw=(g * xh).sum(0) * E, g_lnb=g.sum(0) * E)
    bound = max(int(a_pos.max()), int(np.abs(g * xh).sum(0).max()) * E, int(np.abs(gv).max()),
                int((np.abs(E * g) + np.abs(S1) + np.abs(xh * S2)).max()))
    if indexed:
        g_src, a_src = np.zeros((EMBED_K, E), np.int64), np.zeros((EMBED_K, E), np.int64)
        np.add.at(g_src, embed_index(n), gv)
        np.add.at(a_src, embed_index(n), np.abs(gv))
        out["g_src"] = g_src
        bound = max(bound, int(a_src.max()))
    out["bound"] = bound
    return out


MLP_DIMS = (8, 128, 64, 256)          # K0, J0, J1, J2 of the mlp3 cases: the LDS-resident kernel takes it (and folds the losses)
MLP_DIMS_WG = (8, 32, 32, 256)        # hidden (32, 32): the workgroup-per-tile kernel at the same extent
TOK_DIMS = (7, 64, 128, 64)           # A, J0, J1, K of the tokenizer cases (latent width 208 = the case's W)
XF_S, XF_H, XF_D = 23200, 8, 64


def _tokenizer_cases():
    """Family C.  mlp3 / mlp3_bwd / mlp3_loss with y [N, 256]; the screened search and the fused launches with z [N, 208],
    N = 10.3 M; the default branch's unbatched attention whose keep bytes [H][S][S] pass 2^32 (N counts their rows, H S)."""
    N, Ns = rows_for(256), rows_for(208)
    K0, J0, J1, J2 = MLP_DIMS
    rows = lambda W: N * W * F4                                                                    # noqa: E731
    S, H, D = XF_S, XF_H, XF_D
    return [Case("mlp3", "lipvq_mlp3_f32", N, 256,
                 (("x, latent", 2 * rows(K0)), ("y, pre2 (fenced)", _big(N, 256, 2, fenced=2)), ("pre0, pre1", rows(J0) + rows(J1)),
                  ("target, the folded launch's y", 2 * rows(256)), ("chunks", 2 * _CHUNK)), dims=MLP_DIMS),
            Case("mlp3_wg", "lipvq_mlp3_f32", N, 256, (("x", rows(K0)), ("y (fenced)", _big(N, 256, fenced=1)), ("chunks", 2 * _CHUNK)), dims=MLP_DIMS_WG),
            Case("mlp3_bwd", "lipvq_mlp3_bwd_f32", N, 256,
                 (("gy", rows(256)), ("pre0, pre1", rows(J0) + rows(J1)), ("g0, g1, gx", rows(J0) + rows(J1) + rows(K0)), ("chunks", 2 * _CHUNK)),
                 dims=MLP_DIMS),
            Case("nearest_screened", "lipvq_nearest_screened_f32", Ns, 208,
                 (("z", _big(Ns, 208)), ("z_q", _big(Ns, 208)), ("idx, workspace", Ns * 8 + (1 << 30)), ("chunks", 2 * _CHUNK)), dims=(64, 208)),
            Case("tokenize", "lipvq_tokenize_f32", Ns, 208,
                 (("x", _big(Ns, TOK_DIMS[0])), ("z_q, z_e", _big(Ns, 208, 2)), ("idx", Ns * 8), ("workspace", _big(Ns, 208) + 80 * Ns + (1 << 20)),
                  ("chunks", 4 * _CHUNK)), dims=TOK_DIMS),
            Case("attention_unbatched", "lipvq_attention_f32", H * S, S,
                 (("keep bytes", H * S * S), ("float64 reference of one head: six [S, S] tensors at its peak", 6 * S * S * 8),
                  ("qkv, out, gout, gqkv, lse, delta, twice", 2 * (8 * S * D + 2 * H * S) * F4)), boundaries=(B31, B32), dims=(S, D, H), p=0.1)]


def _flat_cases():
    out = []
    for name, entry in (("ste", "lipvq_ste_f32"), ("scaled_diff", "lipvq_scaled_diff_f32"), ("act_bwd", "lipvq_act_bwd_f32")):
        for tag, n, bounds in (("2p31", B31 + FLAT_TAIL, (B30, B31)), ("2p32", B32 + FLAT_TAIL, (B30, B31, B32))):
            # the two inputs are two views of ONE buffer, SHIFT elements apart (both are only read): two operands, not three, so
            # that the 2^32 case stays inside the cap
            out.append(Case(f"{name}_{tag}", entry, n, 1, (("inputs (one buffer, two views)", (n + FLAT_SHIFT) * F4), ("out (fenced)", _big(n, 1, fenced=1)),
                                                           ("chunks", _CHUNK)), boundaries=bounds))
    return out


FLAT_SHIFT = 4 * 1031                 # elements between the two input views of a flat case (a multiple of 4: both stay 16-byte aligned)


def _reduction_cases():
    N = rows_for(2048)
    Ns = rows_for(208)
    Nm = rows_for(7)
    nf = B31 + FLAT_TAIL
    return [Case("wgrad_wide_g", "lipvq_wgrad_f32", N, 2048, (("G", _big(N, 2048)), ("H", _big(N, 8)), ("hidx", N * 8), ("workspace", 128 << 20)), dims=(2048, 8)),
            Case("wgrad_wide_h", "lipvq_wgrad_f32", N, 2048, (("H", _big(N, 2048)), ("G", _big(N, 8)), ("workspace", 128 << 20)), dims=(8, 2048)),
            Case("scatter_add", "lipvq_scatter_add_f32", Ns, 208, (("g", _big(Ns, 208)), ("idx", Ns * 8), ("workspace", 256 << 20)), dims=(64, 208)),
            Case("mse_pair", "lipvq_mse_pair_f32", nf, 1, (("xr, x", _big(nf, 1, 2)), ("small pair, workspace", 1 << 20))),
            Case("grad_norm", "lipvq_grad_sumsq_f32", nf, 1, (("gradient (fenced), its copy", _big(nf, 1, 2, fenced=1)), ("chunks", _CHUNK))),
            Case("nearest", "lipvq_nearest_rows_f32", Ns, 208, (("z", _big(Ns, 208)), ("z_q", _big(Ns, 208)), ("idx", Ns * 8), ("chunks", 2 * _CHUNK)), dims=(64, 208)),
            Case("adam_step", "lipvq_adam_f32", nf, 1, (("p, exp_avg, exp_avg_sq (fenced), grad", _big(nf, 1, 4, fenced=3)), ("chunks", 2 * _CHUNK))),
            Case("bin_minmax", "lipvq_bin_minmax_f32", Nm, 7, (("actions", _big(Nm, 7)),), dims=(7,))]


CASES = _linear_cases() + _keep_cases() + _layernorm_cases() + _embed_cases() + _attention_cases() + _head_cases() + _bin_cases() + _tokenizer_cases() + _flat_cases() + _reduction_cases()
BY_NAME = {c.name: c for c in CASES}

SCATTER_ROUTES = ("atomics", "sorted", "sequential_sorted", "sequential_scan")


# ---- legality: the library's own limits --------------------------------------------------------------------------------------

EINVAL, EUNSUPPORTED = -1, -2


def documented_limits(case):
    """[(the limit as include/lipvq.h and the entry point's argument checks state it, holds?)] for one case."""
    N, W = case.N, case.W
    e = case.entry
    if e in ("lipvq_linear_act_f32", "lipvq_linear_act_drop_f32"):
        out = [("ceil(N / 32) <= 2^31 - 1 (the row-tile grid)", (N + 31) // 32 <= 0x7fffffff)]
        if "drop" in e:
            out.append(("rows of decisions < 2^32", N < B32))
        return out
    if e in ("lipvq_linear_act_bf16", "lipvq_linear_nn_bf16"):
        return [("both Linear widths multiples of 8", all(d % 8 == 0 for d in case.dims)),
                ("ceil(N / 32) <= 2^31 - 1 row tiles, ceil(columns / 32) <= 65535", (N + 31) // 32 <= 0x7fffffff and (max(case.dims) + 31) // 32 <= 65535)]
    if e == "lipvq_act_bwd_drop_f32":
        return [("rows of decisions < 2^32", N < B32)]
    if e == "lipvq_dropout_keep_u8":
        c4 = (W + 3) // 4
        return [("rows < 2^32, cols <= 2^32", N < B32 and W <= B32), ("rows <= (2^31 - 1) * 256 / ceil(cols / 4): one launch", N <= (0x7fffffff * 256) // c4)]
    if e.startswith("lipvq_gpt_layernorm"):
        out = [("E a multiple of 4, <= 1024", W % 4 == 0 and W <= 1024), ("ceil(N / 4) <= 2^31 - 1", (N + 3) // 4 <= 0x7fffffff)]
        if "drop" in e:
            out.append(("rows of decisions < 2^32", N < B32))
        return out
    if e in ("lipvq_gpt_attention_f32", "lipvq_gpt_attention_prefix_f32"):
        L, E, H, B = case.dims
        keys = L if e == "lipvq_gpt_attention_f32" else 2 * L               # the prefix form: L cached + L new tokens
        return [("head width 16, 32 or 64", E % H == 0 and E // H in (16, 32, 64)), ("at most 128 keys", keys <= 128),
                ("B H ceil(L / 32) <= 2^31 - 1 workgroups", B * H * ((L + 31) // 32) <= 0x7fffffff),
                ("B H L rows of decisions < 2^32", B * H * L < B32), ("whole sequences", B * L == N)]
    if e == "lipvq_gmm_head_f32":                        # (lipvq_action_head_f32 on the same rows: its limit is the /3)
        M, A = case.dims
        return [("E a multiple of 4, <= 1024", W % 4 == 0 and W <= 1024), ("M <= 16, A <= 64, M (2 A + 1) <= 512", M <= 16 and A <= 64 and M * (2 * A + 1) <= 512),
                ("ceil(N / 32) <= (2^31 - 1) / 3 row tiles", (N + 31) // 32 <= 0x7fffffff // 3), ("T = N positions fit an int", N < B31)]
    if e in ("lipvq_embed_rows_f32", "lipvq_embed_rows_bwd_det_f32"):
        T, B = case.dims
        strides = (3 * T * W, 2 * W, W, 2 * T * W)                          # batch stride, the two time strides, the offsets used
        return [("E a multiple of 4, <= 1024", W % 4 == 0 and W <= 1024), ("strides and offsets non-negative multiples of 4 floats", all(v % 4 == 0 for v in strides)),
                ("the largest slot ends inside the output", (B - 1) * strides[0] + (T - 1) * strides[1] + W + W <= N * W)]
    if e in ("lipvq_ste_f32", "lipvq_scaled_diff_f32", "lipvq_act_bwd_f32", "lipvq_mse_pair_f32", "lipvq_grad_sumsq_f32", "lipvq_adam_f32"):
        return [("n >= 0 (grid-stride kernels: no upper limit below int64)", 0 <= N < 1 << 62)]
    if e == "lipvq_wgrad_f32":
        return [("N, J, Kd > 0; chunks of 1024 rows fit an int", N > 0 and (N + 1023) // 1024 <= 0x7fffffff)]
    if e == "lipvq_scatter_add_f32":
        return [("N >= 0, K > 0, D > 0", N >= 0), ("the counting sort: 32768 <= N < 2^31 - 65536", 32768 <= N < B31 - 65536)]
    if e == "lipvq_bin_discretize_f32":
        return [("A (num_bins + 1) <= 4096 boundaries", BIN_A * (case.dims[0] + 1) <= 4096)]
    if e == "lipvq_bin_hidden_f32":
        return [("A num_bins table rows leave a 64-column slice in 80 KiB of LDS", (80 * 1024 // 4) // (BIN_A * case.dims[0]) >= 64)]
    if e in ("lipvq_mlp3_f32", "lipvq_mlp3_bwd_f32"):
        K0, J0, J1, J2 = case.dims
        return [("hidden widths multiples of 32 in [32, 256]", all(j % 32 == 0 and 32 <= j <= 256 for j in (J0, J1))),
                ("ceil(N / 32) row tiles <= 2^31 - 1", (N + 31) // 32 <= 0x7fffffff), ("y is [N, 256]", J2 == W == 256)]
    if e in ("lipvq_nearest_screened_f32", "lipvq_tokenize_f32"):          # (lipvq_vq_tokenize_f32: the same checks)
        return [("N <= 2^31 - 1", N <= 0x7fffffff), ("latent width 208: a compile-time instance, 16-byte rows", W == 208)]
    if e == "lipvq_attention_f32":
        S, D, H = case.dims
        return [("head width D / H <= 32", D % H == 0 and D // H <= 32), ("S <= 65535 x 16 query blocks", S <= 65535 * 16),
                ("H S rows of decisions < 2^32", H * S < B32), ("the keep bytes pass 2^32", H * S * S > B32)]
    if e == "lipvq_nearest_rows_f32":                    # (lipvq_nearest_f32 on the same rows: N <= (2^31 - 1) 64)
        return [("N <= 2^31 - 1", N <= 0x7fffffff), ("D = 208: one of the compile-time widths, 16-byte rows", W == 208)]
    if e == "lipvq_bin_minmax_f32":
        return [("A <= 256", W <= 256)]
    raise KeyError(e)


def probe(case, lib):
    """The entry point's own argument checks with null pointers, where they run before the pointer test: the status must be the
    null-pointer refusal (EINVAL), not EUNSUPPORTED.  None where the pointer test comes first (documented_limits restates the limit)."""
    N, W, e, p = case.N, case.W, case.entry, case.p
    if e == "lipvq_linear_act_drop_f32":
        return lib.lipvq_linear_act_drop_f32(None, None, None, None, None, None, 7, p, N, case.dims[0], case.dims[1], 0, None)
    if e == "lipvq_linear_act_bf16":                     # (sizes are checked before pointers: include/lipvq.h)
        return [getattr(lib, e + sfx)(None, None, None, None, None, N, case.dims[0], case.dims[1], 1, None) for sfx in ("", "x3")]
    if e == "lipvq_linear_nn_bf16":
        return [getattr(lib, e + sfx)(None, None, None, N, case.dims[0], case.dims[1], None) for sfx in ("", "x3")]
    if e == "lipvq_gpt_attention_f32":
        L, E, H, B = case.dims
        rcs = [lib.lipvq_gpt_attention_f32(None, None, None, None, 1.0, B, L, E, H, 1, None),
               lib.lipvq_gpt_attention_bwd_f32(None, None, None, None, None, None, None, 1.0, B, L, E, H, 1, None)]
        if case.p:
            rcs += [lib.lipvq_gpt_attention_drop_f32(None, None, None, None, 7, case.p, B, L, E, H, 1, None),
                    lib.lipvq_gpt_attention_bwd_drop_f32(None, None, None, None, None, None, None, 7, case.p, B, L, E, H, 1, None)]
        return rcs
    if e == "lipvq_gpt_attention_prefix_f32":
        L, E, H, B = case.dims
        return lib.lipvq_gpt_attention_prefix_f32(None, None, None, B, B, L, L, E, H, None)
    if e == "lipvq_act_bwd_drop_f32":
        return lib.lipvq_act_bwd_drop_f32(None, None, None, None, 7, p, N, W, 1, None)
    if e == "lipvq_dropout_keep_u8":
        return lib.lipvq_dropout_keep_u8(None, 7, N, W, p, None, None)
    if e == "lipvq_gpt_layernorm_f32":
        return lib.lipvq_gpt_layernorm_f32(None, None, None, None, 1e-5, None, None, None, None, N, W, None)
    if e == "lipvq_gpt_layernorm_drop_f32":
        return lib.lipvq_gpt_layernorm_drop_f32(None, None, None, None, 1e-5, None, 7, p, None, None, None, None, N, W, None)
    if e == "lipvq_gpt_layernorm_bwd_f32":
        return lib.lipvq_gpt_layernorm_bwd_f32(None, None, None, None, None, None, None, None, None, N, W, None)
    if e == "lipvq_gpt_layernorm_bwd_drop_f32":
        return lib.lipvq_gpt_layernorm_bwd_drop_f32(None, None, None, None, None, None, 7, p, None, None, None, None, None, N, W, None)
    return None


# ---- exact sums: every term of every output element, in absolute value -------------------------------------------------------

def exact_sum_bounds():
    """{what: the largest sum over rows of |term| of any output element} of every exact-sum check of the GPU file, int64."""
    out = {}
    for name in ("wgrad_wide_g", "wgrad_wide_h"):
        c = BY_NAME[name]
        J, Kd = c.dims
        rows = window_rows(c.N, c.W)
        G, H = np.abs(exact_values(rows, J, 1)), np.abs(exact_values(rows, Kd, 2))
        ncount = len(count_rows(c.N))
        out[f"{name}: values x values"] = int((G.T @ H).max())
        out[f"{name}: gb of values"] = int(G.sum(0).max())
        out[f"{name}: count x count, gb of count"] = ncount
        cw = np.isin(rows, count_rows(c.N))
        out[f"{name}: count x values"] = int(max(G[cw].sum(0).max(), H[cw].sum(0).max()))
    c = BY_NAME["scatter_add"]
    rows = window_rows(c.N, c.W)
    out["scatter_add: values"] = int(np.abs(exact_values(rows, c.W, 3)).sum(0).max())            # (even if every row fell on one code)
    out["scatter_add: count"] = int(np.bincount(scatter_code(count_rows(c.N), c.dims[0])).max())
    c = BY_NAME["layernorm_bwd"]
    rows = window_rows(c.N, c.W)
    g, xh = np.abs(exact_values(rows, c.W, 4)), np.abs(exact_values(rows, c.W, 5))
    out["layernorm_bwd: gw"] = int((g * xh).sum(0).max())
    out["layernorm_bwd: gb"] = int(g.sum(0).max())
    return out


def grad_exact_sumsq(n, small):
    """int: the sum of squares of the gradient list of the grad_norm case -- exact_values on the windows of the big tensor (zero
    elsewhere) and `small` exact_values of a second tensor; the kernels sum in double (bound 2^53)."""
    rows = window_rows(n, 1, BY_NAME["grad_norm"].boundaries)
    a, b = exact_values(rows, 1, 10), exact_values(np.arange(small), 1, 11)
    return int((a * a).sum() + (b * b).sum())


def mse_exact_sum(n):
    """int: sum over the window elements of (xr - x)^2 of the mse case (both operands exact_values on the windows, zero elsewhere);
    the kernel sums in double, so the bound is 2^53, and the mean it stores is float32(sum / n)."""
    rows = window_rows(n, 1, BY_NAME["mse_pair"].boundaries)
    d = exact_values(rows, 1, 6) - exact_values(rows, 1, 7)
    return int((d * d).sum())


# ---- workspace sizes -----------------------------------------------------------------------------------------------------------

WORKSPACE_NS = (1 << 20, 1 << 24, B31 - 1, 1 << 33)


def _bf16_chunks(N, J, K):
    """ceil(N / chunk) of lipvq_wgrad_bf16 as include/lipvq.h states it."""
    want = max(1, 1024 // (-(-J // 128) * -(-K // 128)))
    chunk = max(64, 32 * -(-(-(-N // want)) // 32))
    return -(-N // chunk)


def workspace_exports():
    """[(export, widths, call(lib, N), floor(N) or None, zero_is_refusal)]: every lipvq_*_workspace_bytes of include/lipvq.h that
    takes N, at its narrowest and widest widths.  floor(N) = the bytes of the largest array the header says the workspace holds
    (None where the header names none); zero_is_refusal: the header documents 0 as "unsupported" for this export."""
    rows = []

    def add(name, widths, call, floor, zero_is_refusal=False):
        rows.append((name, widths, call, floor, zero_is_refusal))
    for J, Kd in ((1, 1), (2048, 2048)):
        add("lipvq_wgrad_workspace_bytes", (J, Kd), lambda lib, N, J=J, Kd=Kd: lib.lipvq_wgrad_workspace_bytes(N, J, Kd),
            lambda N, J=J, Kd=Kd: -(-N // 2048) * (J * Kd + J) * 4)                              # chunks of 64 ... 2048 rows
        add("lipvq_wgrad_bf16_workspace_bytes", (8 * J, 8 * Kd), lambda lib, N, J=8 * J, Kd=8 * Kd: lib.lipvq_wgrad_bf16_workspace_bytes(N, J, Kd),
            lambda N, J=8 * J, Kd=8 * Kd: _bf16_chunks(N, J, Kd) * (J * Kd + J) * 4)
    for K, D in ((2, 1), (16384, 512)):
        add("lipvq_scatter_add_sorted_workspace_bytes", (K, D), lambda lib, N, K=K, D=D: lib.lipvq_scatter_add_sorted_workspace_bytes(N, K, D),
            None, True)
    for E in (4, 1024):
        add("lipvq_gpt_layernorm_bwd_workspace_bytes", (E,), lambda lib, N, E=E: lib.lipvq_gpt_layernorm_bwd_workspace_bytes(N, E),
            lambda N, E=E: 2 * E * 4)                                                            # per-workgroup partial (gw, gb) rows: at least one
        for indexed in (0, 1):
            add("lipvq_embed_rows_bwd_det_workspace_bytes", (E, indexed),
                lambda lib, N, E=E, i=indexed: lib.lipvq_embed_rows_bwd_det_workspace_bytes(N, 10, E, 1024, i),
                (lambda N, E=E: N * E * 4) if indexed else (lambda N, E=E: 10 * 3 * E * 4))      # the rows' gradients, written once; dense: a
                                                                                                 # partial (g_pos, g_lnw, g_lnb) triple per time step
        add("lipvq_embed_rows_bwd_workspace_bytes", (E,), lambda lib, N, E=E: lib.lipvq_embed_rows_bwd_workspace_bytes(N, 10, E, 1024),
            lambda N, E=E: N * E * 4, True)
    for D in (1, 512):
        add("lipvq_tokenize_workspace_bytes", (D,), lambda lib, N, D=D: lib.lipvq_tokenize_workspace_bytes(N, D), lambda N, D=D: N * D * 4 + 72 * N)
    add("lipvq_nearest_workspace_bytes", (), lambda lib, N: lib.lipvq_nearest_workspace_bytes(N), None)
    for K in (1, 16384):
        add("lipvq_nearest_small_workspace_bytes", (K,), lambda lib, N, K=K: lib.lipvq_nearest_small_workspace_bytes(N, K), None)
        add("lipvq_kmeans_workspace_bytes", (K,), lambda lib, N, K=K: lib.lipvq_kmeans_workspace_bytes(N, K), None)
    # (the header says nothing about what the nearest, nearest_small and kmeans workspaces hold: monotonicity only)
    add("lipvq_gmm_workspace_bytes", (), lambda lib, N: lib.lipvq_gmm_workspace_bytes(N), lambda N: -(-N // 32) * 4)             # a partial sum per 32 rows
    add("lipvq_action_head_workspace_bytes", (), lambda lib, N: lib.lipvq_action_head_workspace_bytes(N), lambda N: -(-N // 32) * 12)   # three floats per 32 rows
    return rows
