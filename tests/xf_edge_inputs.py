"""Non-random inputs for the transformer kernels (csrc/lipvq_gpt.hip, csrc/lipvq_xf.hip) and the yardstick their errors are
held to -- plain seeded torch on the CPU, no GPU; tests/test_gpu_xf_edges.py runs the kernels on these inputs and
tests/test_xf_edge_inputs_host.py checks the generators and the yardstick themselves.

The yardstick.  An operation (forward, and backward through ``(out * gout).sum()``) is evaluated with the SAME torch ops in
float64 and in float32 on the CPU: ``gpt_ref.attention_ref`` (the unbatched sequence is a batch of one without a mask; the host
test ties that to ``test_gpu_default._attention_ref``) and ``F.layer_norm``.  ``dev`` of a tensor is the fp32 run's largest
deviation from the float64 run over the float64 result's largest magnitude.  A kernel tensor's bound is
``max(TOL, REF_FACTOR * dev)`` with tests/test_gpu_gpt.py's ``FWD_TOL`` / ``BWD_TOL`` / ``REF_FACTOR``: on inputs where fp32 itself
cannot reach 1e-5 (scores of several hundred, rows of 1000 + noise) the kernel may be as far from float64 as four times what
stock fp32 torch is, and no further.  ``dev`` never comes from the code under test, and DEV_CAP keeps the yardstick from
growing loose: a class whose 4 x dev exceeds it at a tested shape fails the host test.
"""
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import gpt_ref

FWD_TOL, BWD_TOL, REF_FACTOR = 1e-5, 1e-4, 4.0          # tests/test_gpu_gpt.py's
DEV_CAP = 2e-3                                          # REF_FACTOR x dev may not exceed this at any class and shape
CONTROL_DEV = 1e-6                                      # the plain-randn class: fp32 torch is this close to float64
LN_EPS = 1e-5
KEEP_PROB = 0.1                                         # the edge keep masks keep one probability in ten

# the shapes tests/test_gpu_xf_edges.py runs (the host test walks the same lists)
GPT_DH = (16, 32, 64)
GPT_L = (1, 31, 32, 33, 64, 65, 127, 128)               # the 32-query / 32-key tile edges and their neighbours
GPT_B, GPT_H = 3, 2
XF_S = (1, 15, 16, 17, 63, 64, 65, 130)                 # 16 queries per workgroup, 64-key LDS tiles
XF_DH_HEADS = ((64, 8), (24, 8), (208, 8), (128, 4))    # (D, H): head widths 8, 3 (padded to 8), 26 (padded to 32), 32
LN_E = (4, 8, 252, 256, 260, 1020, 1024)                # first and last float4 lane of each of the four per-lane slots
LN_N = (1, 5, 2053)                                     # 2053: 8 rows per block, a ragged last block, a last wave without rows
LN_VARIANTS = ((True, True, True), (False, False, False), (True, False, False), (False, True, True))   # (b, s_out, gres)

ATTENTION_CLASSES = ("control", "peaked4", "peaked16", "offset", "uniform", "dominant", "far_apart")
LAYERNORM_CLASSES = ("control", "plus100", "plus1000", "tiny", "underflow", "huge", "constant", "onehot", "halves", "cancel")
CONSTANT_VALUE, ONEHOT_VALUE, HALVES_VALUE = 3.0, 1e4, 1024.0


def rel(a, b):
    """max |a - b| / max |b|  (tests/test_gpu_gpt.py's _rel)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max())) if a.size else 0.0


def bound(tol, dev):
    return max(tol, REF_FACTOR * dev)


def report(what, err, dev, tol):
    """Print 'what: error, the fp32 reference's own, ratio, bound' and return (what, err, bound) for the assertion that follows."""
    b = bound(tol, dev)
    ratio = err / dev if dev > 0 else float("nan")
    print(f"{what}: error {err:.3e}, reference's own {dev:.3e}, ratio {ratio:.2f}, bound {b:.3e}")
    return what, err, b


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------

def dominant_pairs(B, L, H):
    """(b, h, i, j): query i of (b, h) gets key j as its one dominant key, j <= i.  Keys at the tile edges 31 | 32 and 63 | 64,
    the first and the last; one pair per (b, h), taken in turn."""
    js = sorted({j for j in (0, 31, 32, 63, 64, L - 1) if j < L}, reverse=True)
    cand = [(L - 1 - n, j) for n, j in enumerate(js) if j <= L - 1 - n]
    return [(b, h) + cand[(b * H + h) % len(cand)] for b in range(B) for h in range(H)]


def attention_inputs(cls, B, L, H, dh):
    """(qkv [B, L, 3 H dh], gout [B, L, H dh]) of one input class; the unbatched kernels take [0] of B = 1."""
    g = _gen("attention", cls, B, L, H, dh)
    t = torch.randn(B, L, 3, H, dh, generator=g)
    gout = torch.randn(B, L, H * dh, generator=g)
    q, k = t[:, :, 0], t[:, :, 1]                                   # views [B, L, H, dh]
    if cls == "peaked4":
        q *= 4.0
        k *= 4.0
    elif cls == "peaked16":
        q *= 16.0
        k *= 16.0
    elif cls == "offset":                                           # |u|^2 = dh: every score of a query moves by (8 q.u + 16 dh) / sqrt(dh)
        u = torch.randn(dh, generator=g)
        u *= math.sqrt(dh) / u.norm()
        k += 8.0 * u
        q += 2.0 * u
    elif cls == "uniform":
        q.zero_()
    elif cls == "dominant":                                         # |q_i|^2 = 4 dh and k_j = 6 q_i: score 24 sqrt(dh), the others ~ 2 N(0, 1)
        for b, h, i, j in dominant_pairs(B, L, H):
            q[b, i, h] *= 2.0 * math.sqrt(dh) / q[b, i, h].norm()
            k[b, j, h] = 6.0 * q[b, i, h]
    elif cls == "far_apart":                                        # every other key 100 x: its scores sit hundreds above or below the rest
        k[:, 1::2] *= 100.0
    elif cls != "control":
        raise ValueError(cls)
    return t.reshape(B, L, 3 * H * dh), gout


def dropped_rows(B, L, H):
    """Per (b, h): the query row that keeps no key and the key column nobody keeps."""
    return [(b, h, (7 * (b * H + h) + L // 2) % L, (5 * (b * H + h) + L // 3) % L) for b in range(B) for h in range(H)]


def keep_mask(B, L, H):
    """uint8 [B, H, L, L], one in ten kept, with dropped_rows() cleared."""
    keep = (torch.rand(B, H, L, L, generator=_gen("keep", B, L, H)) < KEEP_PROB).to(torch.uint8)
    for b, h, row, col in dropped_rows(B, L, H):
        keep[b, h, row, :] = 0
        keep[b, h, :, col] = 0
    return keep


def scores64(qkv, H, causal):
    """float64 scaled scores [B, H, L, L], closed positions at -inf."""
    B, L, E3 = qkv.shape
    E = E3 // 3
    dh = E // H
    qd = qkv.double()
    q, k = qd[..., :E].view(B, L, H, dh).transpose(1, 2), qd[..., E:2 * E].view(B, L, H, dh).transpose(1, 2)
    sc = (q @ k.transpose(-2, -1)) / math.sqrt(dh)
    if causal:
        sc = sc.masked_fill(gpt_ref.causal_mask(L) == 0, float("-inf"))
    return sc


def _attention_run(qkv, gout, H, causal, keep, dtype):
    x = qkv.to(dtype, copy=True).requires_grad_(True)
    out = gpt_ref.attention_ref(x, H, gpt_ref.causal_mask(qkv.shape[1]) if causal else None, keep, KEEP_PROB if keep is not None else 1.0)
    (out * gout.to(dtype)).sum().backward()
    out = out.detach()
    B, L, E = out.shape
    delta = (out * gout.to(dtype)).view(B, L, H, E // H).sum(-1).transpose(1, 2)          # [B, H, L], what the backward keeps
    return {"out": out, "gqkv": x.grad, "delta": delta}


@functools.lru_cache(maxsize=None)
def attention_case(cls, B, L, H, dh, causal, drop):
    """One case, computed once: inputs, the float64 results (out, gqkv, delta, lse, scores) and dev (out, gqkv, delta)."""
    qkv, gout = attention_inputs(cls, B, L, H, dh)
    keep = keep_mask(B, L, H) if drop else None
    ref = _attention_run(qkv, gout, H, causal, keep, torch.float64)
    f32 = _attention_run(qkv, gout, H, causal, keep, torch.float32)
    dev = {k: rel(f32[k], ref[k]) for k in ref}
    sc = scores64(qkv, H, causal)
    ref["scores"] = sc
    ref["lse"] = torch.logsumexp(sc, -1)
    ref["score_max"] = float(sc[sc > -1e300].abs().max())
    return {"qkv": qkv, "gout": gout, "keep": keep, "keep_prob": KEEP_PROB if drop else 1.0, "ref": ref, "dev": dev}


def lse_bound(case):
    return 1e-5 * max(1.0, case["ref"]["score_max"])                # tests/test_gpu_gpt.py's form


# ---------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------

def layernorm_groups(N):
    """The classes that share one [N, E] tensor: all ten where there are rows enough, else N at a time."""
    n = min(N, len(LAYERNORM_CLASSES))
    return [LAYERNORM_CLASSES[i:i + n] for i in range(0, len(LAYERNORM_CLASSES), n)]


def layernorm_rows(classes, N):
    """Row ranges {class: slice}: consecutive blocks of N // len(classes) rows, the last class takes the remainder."""
    per = N // len(classes)
    return {c: slice(i * per, N if i == len(classes) - 1 else (i + 1) * per) for i, c in enumerate(classes)}


def _layernorm_class(cls, n, E, g, with_b):
    """(a, b) rows [n, E] of one class; s = a + b is the class's row in fp32.  b is None without with_b."""
    z = torch.randn(n, E, generator=g)
    if cls == "control":
        return (z, torch.randn(n, E, generator=g)) if with_b else (z, None)
    if cls == "cancel":                                             # b = -a + 1e-3 randn: the sum cancels to the noise
        a = torch.randn(n, E, generator=g)
        b = -a + 1e-3 * z
        return (a, b) if with_b else (a + b, None)
    if cls == "plus100":
        x = 100.0 + z
    elif cls == "plus1000":                                         # (200 at E = 4, where a row of four can have a standard deviation of 0.02
        x = (1000.0 if E > 4 else 200.0) + z                        #  and fp32 torch itself is then 2e-3 off: DEV_CAP would not hold)
    elif cls == "tiny":                                             # variance 1e-6, below eps
        x = 1e-3 * z
    elif cls == "underflow":                                        # squares 1e-40: below the smallest normal fp32
        x = 1e-20 * z
    elif cls == "huge":                                             # squares 1e30, a row's sum of them < 1e35
        x = 1e15 * z
    elif cls == "constant":
        x = torch.full((n, E), CONSTANT_VALUE)
    elif cls == "onehot":                                           # the hot column walks over the lanes and slots
        x = torch.zeros(n, E)
        x[torch.arange(n), (torch.arange(n) * 61 + E - 1) % E] = ONEHOT_VALUE
    elif cls == "halves":                                           # mean exactly 0, variance c^2
        x = torch.full((n, E), HALVES_VALUE)
        x[:, E // 2:] = -HALVES_VALUE
    else:
        raise ValueError(cls)
    if not with_b:
        return x, None
    b = 0.25 * x                                                    # (exact; 3.0, 1e4 and 1024 split into exact parts)
    return x - b, b


def _layernorm_run(t, dtype):
    a, w, bias = (t[k].to(dtype, copy=True).requires_grad_(True) for k in ("a", "w", "bias"))
    E = a.shape[-1]
    s = a + t["b"].to(dtype) if t["b"] is not None else a * 1.0
    s.retain_grad()
    y = F.layer_norm(s, (E,), w, bias, LN_EPS)
    obj = (y * t["gy"].to(dtype)).sum()
    if t["gres"] is not None:
        obj = obj + (s * t["gres"].to(dtype)).sum()                 # s also feeds the residual stream: gres arrives there
    obj.backward()
    with torch.no_grad():
        xhat = F.layer_norm(s, (E,), None, None, LN_EPS)
        rstd = torch.rsqrt(s.var(-1, unbiased=False) + LN_EPS)
    return {"s": s.detach(), "y": y.detach(), "xhat": xhat, "rstd": rstd, "gs": s.grad, "gw": w.grad, "gb": bias.grad}


@functools.lru_cache(maxsize=None)
def layernorm_case(classes, N, E, with_b, with_gres):
    """One [N, E] tensor whose row blocks are `classes`: inputs, the float64 results, the fp32 torch results and the row ranges."""
    g = _gen("layernorm", classes, N, E, with_b, with_gres)
    rows = layernorm_rows(classes, N)
    parts = [_layernorm_class(c, rows[c].stop - rows[c].start, E, g, with_b) for c in classes]
    t = {"a": torch.cat([p[0] for p in parts]), "b": torch.cat([p[1] for p in parts]) if with_b else None,
         "w": torch.randn(E, generator=g), "bias": torch.randn(E, generator=g), "gy": torch.randn(N, E, generator=g),
         "gres": torch.randn(N, E, generator=g) if with_gres else None}
    t.update(rows=rows, ref=_layernorm_run(t, torch.float64), f32=_layernorm_run(t, torch.float32))
    return t


ROW_TENSORS, COLUMN_TENSORS = ("s", "y", "xhat", "rstd", "gs"), ("gw", "gb")


def layernorm_dev(case, name, cls=None):
    """dev of one tensor: over a class's rows against that class's own float64 maximum, or (gw, gb) over the whole tensor."""
    sl = case["rows"][cls] if cls is not None else slice(None)
    return rel(case["f32"][name][sl], case["ref"][name][sl])
