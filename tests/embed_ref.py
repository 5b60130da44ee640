"""The embedding stage (csrc/lipvq_embed.hip: embed_rows and its backward) restated in plain torch, and the shapes its edge
tests run -- no GPU needed; tests/test_gpu_embed_edges.py runs the kernels on these, tests/test_embed_ref_host.py checks the
restatement, the yardstick's conditions and the oracle's LayerNorm themselves.

Inputs are the LayerNorm classes of tests/xf_edge_inputs.py (`layernorm_case`: a -> src, b -> pos with B = 1 and T = N, w and
bias -> ln_w and ln_b, gy -> the gradient of the output rows) and the results map back gs -> g_src (and g_pos: one row per time
step), gw -> g_lnw, gb -> g_lnb.  The yardstick is that file's: `embed_run` is evaluated in float64 and in float32 on the CPU,
dev = the fp32 run's deviation, a kernel tensor's bound is max(TOL, REF_FACTOR x dev).
"""
import functools

import torch
import torch.nn.functional as F

import xf_edge_inputs as X

# forward and backward NJ dispatch edges (64, 128, 256, 512 | 256, 512, 768 floats) and the two widths where fl(1/E) bites
EDGE_E = (4, 8, 128, 132, 252, 256, 260, 512, 516, 768, 772, 1020, 1024)
EDGE_N = (5, 2053)
EDGE_ROUTES = (("dense", True), ("dense", False), ("indexed", False))          # (route, with pos)
WS_EDGE_N, WS_EDGE_T, WS_EDGE_E = 32773, 7, (260, 772)                          # the dense workspace route, ragged (32773 = 7 * 4681 + 6)

# (N, T) of the forward kernel's row stepping: chunk = clamp(N / 32768, 1, 16) steps of 16 rows per work item, grid <= 2048
STEP_E, STEP_K = 8, 5
STEP_CASES = ((40000, 10),          # chunk 1, two grid-stride iterations
              (65536, 16),          # r16 = 0
              (65573, 10),          # chunk 2, ragged
              (98305, 3),           # chunk 3
              (262793, 17),         # chunk 8, T > 16
              (525061, 10),         # chunk 16, second grid-stride iteration, ragged
              (525061, 1),          # T = 1 with chunk 16
              (70001, 1000))        # large T

WIDE_BT = (3, 5)
WIDE_E = (512, 516, 768, 772, 1020, 1024)                                       # NJ = 2 | 3 | 3 | 4 | 4 | 4 of the backward kernels
WIDE_TOL = 2e-4                                                                 # tests/test_gpu_embed.py's large-batch bound, of the gradient's scale
WS_N = 32768 + 7
# (E, T, K, kind, indexed) on the workspace route at N = WS_N: NJ = 4 with its 48 KiB LDS reduction, one workgroup per time step
WS_CASES = ((772, 10, 300, "uniform", True), (772, 10, 300, "uniform", False), (1024, 10, 300, "uniform", True),
            (1024, 10, 300, "uniform", False), (64, 1000, 300, "uniform", True), (64, 1000, 300, "uniform", False),
            (64, 1024, 300, "uniform", True), (64, 1024, 300, "uniform", False), (772, 10, 300, "collapsed", True))

LINEAR_SMALL = (33, 40, (1, 63, 65, 127, 128, 129))                             # N, E, Kin: linear_kernel's 64-wide K chunk edges
LINEAR_BIG = ((66000, 36, 130), (131100, 8, 33), (65536, 100, 512))             # (N, Kin, E): 128 x 128, 256 x 64, 128 x 128 tiles


def embed_chunk(N):
    """The forward's steps per work item (embed_chunk in csrc/lipvq_embed.hip)."""
    return max(1, min(16, N // 32768))


def embed_run(src, idx, pos, T, w, bias, gout, dtype, eps=X.LN_EPS):
    """embed_rows and its gradients through (y * gout).sum(), for any (idx, pos, T): row n of y = LayerNorm(src[idx[n] | n] +
    pos[n % T]) * w + bias.  N = gout.shape[0] may be ragged (no multiple of T).  A row whose index is outside [0, src rows) is
    NaN in y / mean / rstd and contributes to no gradient.  Runs on the device of its arguments."""
    N, E = gout.shape
    R = src.shape[0]
    s_, w_, b_ = (t.to(dtype, copy=True).requires_grad_(True) for t in (src, w, bias))
    p_ = pos.to(dtype, copy=True).requires_grad_(True) if pos is not None else None
    k = torch.arange(N, device=gout.device) if idx is None else idx
    ok = (k >= 0) & (k < R)
    x = s_[k.clamp(0, R - 1)]
    if p_ is not None:
        x = x + p_[torch.arange(N, device=gout.device) % T]
    y = F.layer_norm(x, (E,), w_, b_, eps)
    (y * (gout.to(dtype) * ok[:, None])).sum().backward()
    with torch.no_grad():
        nan = torch.full((), float("nan"), dtype=dtype, device=gout.device)
        mean = torch.where(ok, x.mean(-1), nan)
        rstd = torch.where(ok, torch.rsqrt(x.var(-1, unbiased=False) + eps), nan)
        y = torch.where(ok[:, None], y.detach(), nan)
    return {"y": y, "mean": mean, "rstd": rstd, "g_src": s_.grad, "g_pos": None if p_ is None else p_.grad,
            "g_lnw": w_.grad, "g_lnb": b_.grad}


def edge_inputs(classes, N, E, with_b):
    """The inputs of X.layernorm_case(classes, N, E, with_b, False) -- same seed, same draws -- without its results."""
    g = X._gen("layernorm", classes, N, E, with_b, False)
    rows = X.layernorm_rows(classes, N)
    parts = [X._layernorm_class(c, rows[c].stop - rows[c].start, E, g, with_b) for c in classes]
    return {"a": torch.cat([p[0] for p in parts]), "b": torch.cat([p[1] for p in parts]) if with_b else None,
            "w": torch.randn(E, generator=g), "bias": torch.randn(E, generator=g), "gy": torch.randn(N, E, generator=g), "rows": rows}


def edge_index(N):
    """A fixed permutation of the N table rows in which every fourth entry repeats the one before it."""
    idx = torch.randperm(N, generator=X._gen("embed idx", N))
    idx[3::4] = idx[2::4][:idx[3::4].numel()]
    return idx


@functools.lru_cache(maxsize=2)
def edge_case(classes, N, E, route, with_pos, T=None):
    """One edge-value case as embed arguments: src [N, E], idx (route 'indexed': src is the table) or None, pos [T, E] or None
    (T = N, B = 1 unless given; pos only with T = N), the float64 and fp32 results and, per class, the output rows and the
    source rows that belong to it."""
    t = edge_inputs(classes, N, E, with_pos)
    T = N if T is None else T
    assert not (with_pos and (route == "indexed" or T != N))
    idx = edge_index(N) if route == "indexed" else None
    args = (t["a"], idx, t["b"], T, t["w"], t["bias"], t["gy"])
    src_cls = torch.empty(N, dtype=torch.int64)
    for i, c in enumerate(classes):
        src_cls[t["rows"][c]] = i
    out_cls = src_cls if idx is None else src_cls[idx]
    return {"src": t["a"], "idx": idx, "pos": t["b"], "T": T, "w": t["w"], "bias": t["bias"], "gout": t["gy"],
            "ref": embed_run(*args, torch.float64), "f32": embed_run(*args, torch.float32), "src_rows": t["rows"],
            "out_rows": {c: torch.nonzero(out_cls == i).flatten() for i, c in enumerate(classes)}}


ROW_OUT, ROW_SRC, COLUMNS = ("y", "rstd"), ("g_src", "g_pos"), ("g_lnw", "g_lnb")


def edge_rows(case, name, cls):
    """The rows of tensor `name` that belong to class `cls` (g_pos has one row per time step: with T = N, the source's rows)."""
    if name in COLUMNS:
        return slice(None)
    return case["out_rows"][cls] if name in ROW_OUT else case["src_rows"][cls]


def edge_dev(case, name, cls=None):
    sl = edge_rows(case, name, cls)
    return X.rel(case["f32"][name][sl], case["ref"][name][sl])


def edge_err(case, name, got, cls=None):
    sl = edge_rows(case, name, cls)
    return X.rel(got[sl], case["ref"][name][sl])
