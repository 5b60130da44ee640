"""Tensor-level wrappers over the C ABI (include/lipvq.h): validation, output allocation and
stream plumbing only -- all arithmetic happens in the HIP library.

Every function takes CUDA(HIP) fp32 contiguous tensors on one device and enqueues work on
``torch.cuda.current_stream()``.  A CPU tensor is an error (there is no CPU path in the
product; the CPU restatement lives in oracle/ and is test infrastructure).
"""
from __future__ import annotations

import ctypes as _C

import torch

from . import _capi
from ._capi import (ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, DIST_NORM, DIST_SQSUM, check, get_option, lib, set_option)  # noqa: F401

__all__ = ["lipschitz_scale", "mlp3_pack", "mlp3", "nearest", "ste", "mse_pair", "ACT_NONE", "ACT_GELU",
           "ACT_SIGMOID", "ACT_RELU", "DIST_NORM", "DIST_SQSUM"]


def _chk(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the LipVQ tokenizer path runs on the GPU only (got a {t.device} tensor)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """Current HIP stream of the current device as an integer handle (the fast private accessor when torch has it)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


class _on:
    """`with _on(device):` -- torch.cuda.device(device), skipped when that device is already current (the usual case:
    one process per GPU), which saves a few microseconds on every small launch of a training step."""

    __slots__ = ("ctx",)

    def __init__(self, device):
        idx = device.index
        self.ctx = None if (idx is None or idx == torch.cuda.current_device()) else torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        return False


def lipschitz_scale(W: torch.Tensor, ci: torch.Tensor):
    """(scale[D], Wn[D,H]) of the reference's normalization() (backbone_lfqvae_v5.py:6-12)."""
    W, ci = _chk(W, "W"), _chk(ci, "ci")
    D, H = W.shape
    scale = torch.empty(D, device=W.device, dtype=torch.float32)
    Wn = torch.empty_like(W)
    with _on(W.device):
        check(lib.lipvq_lipschitz_scale_f32(_ptr(W), _ptr(ci), _ptr(scale), _ptr(Wn), D, H, _stream()),
              "lipvq_lipschitz_scale_f32")
    return scale, Wn


class PackedMlp3:
    """Weights of one three-layer stack in MFMA A-operand order (see csrc/lipvq_mlp.hip)."""

    __slots__ = ("buf", "K0", "J0", "J1", "J2")

    def __init__(self, buf, K0, J0, J1, J2):
        self.buf, self.K0, self.J0, self.J1, self.J2 = buf, K0, J0, J1, J2


def mlp3_pack(W0, b0, W1, b1, W2, b2) -> PackedMlp3:
    W0, b0, W1, b1, W2, b2 = (_chk(t, n) for t, n in
                              ((W0, "W0"), (b0, "b0"), (W1, "W1"), (b1, "b1"), (W2, "W2"), (b2, "b2")))
    J0, K0 = W0.shape
    J1, J2 = W1.shape[0], W2.shape[0]
    if W1.shape[1] != J0 or W2.shape[1] != J1 or b0.numel() != J0 or b1.numel() != J1 or b2.numel() != J2:
        raise ValueError("mlp3_pack: inconsistent layer shapes")
    n = lib.lipvq_mlp3_packed_floats(K0, J0, J1, J2)
    buf = torch.empty(n, device=W0.device, dtype=torch.float32)
    with _on(W0.device):
        check(lib.lipvq_mlp3_pack_f32(_ptr(W0), _ptr(b0), _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(buf),
                                      K0, J0, J1, J2, _stream()), "lipvq_mlp3_pack_f32")
    return PackedMlp3(buf, K0, J0, J1, J2)


def mlp3(x: torch.Tensor, packed: PackedMlp3, acts, gather_idx: torch.Tensor | None = None,
         N: int | None = None, save_pre: bool = False):
    """y[N,J2] (and the three pre-activation tensors when save_pre).  With gather_idx, row n of
    the input is x[gather_idx[n]] (x is then the table, e.g. the codebook)."""
    x = _chk(x, "x")
    if x.dim() != 2 or x.shape[1] != packed.K0:
        raise ValueError(f"mlp3: x must be [N,{packed.K0}], got {tuple(x.shape)}")
    if gather_idx is not None:
        gather_idx = _chk(gather_idx, "gather_idx", torch.int64)
        N = gather_idx.numel()
    else:
        N = x.shape[0]
    dev = x.device
    y = torch.empty((N, packed.J2), device=dev, dtype=torch.float32)
    pre = [torch.empty((N, J), device=dev, dtype=torch.float32) if save_pre else None
           for J in (packed.J0, packed.J1, packed.J2)]
    with _on(dev):
        check(lib.lipvq_mlp3_f32(_ptr(x), _ptr(gather_idx), _ptr(packed.buf), _ptr(y), _ptr(pre[0]),
                                 _ptr(pre[1]), _ptr(pre[2]), N, packed.K0, packed.J0, packed.J1, packed.J2,
                                 int(acts[0]), int(acts[1]), int(acts[2]), _stream()), "lipvq_mlp3_f32")
    return (y, pre) if save_pre else y


def mlp3_loss_supported(N, packed: PackedMlp3) -> bool:
    """Can lipvq_mlp3_loss_f32 (the forward stack with the two mean-squared errors folded in) take this batch and stack?"""
    return bool(lib.lipvq_mlp3_loss_supported(int(N), packed.K0, packed.J0, packed.J1, packed.J2))


def mlp3_loss(x, packed: PackedMlp3, acts, gather_idx, target, latent, w: float, form: int, save_pre: bool = False, ste: bool = False):
    """(y, pre or None, out3): mlp3() plus out3 = tensor([mean((y - target)^2), mean((input rows - latent)^2), loss]) as
    mse_pair_loss() forms it, summed by the stack's own launch (mlp3_loss_supported() must hold).  ste=True: the stack runs on
    latent + (input rows - latent), the plain VQVAE's straight-through value, which is returned as a fourth result."""
    x, target, latent = _chk(x, "x"), _chk(target, "target"), _chk(latent, "latent")
    if x.dim() != 2 or x.shape[1] != packed.K0:
        raise ValueError(f"mlp3_loss: x must be [N,{packed.K0}], got {tuple(x.shape)}")
    if gather_idx is not None:
        gather_idx = _chk(gather_idx, "gather_idx", torch.int64)
        N = gather_idx.numel()
    else:
        N = x.shape[0]
    if tuple(target.shape) != (N, packed.J2) or tuple(latent.shape) != (N, packed.K0):
        raise ValueError(f"mlp3_loss: target must be [{N},{packed.J2}] and latent [{N},{packed.K0}]")
    dev = x.device
    y = torch.empty((N, packed.J2), device=dev, dtype=torch.float32)
    pre = [torch.empty((N, J), device=dev, dtype=torch.float32) if save_pre else None
           for J in (packed.J0, packed.J1, packed.J2)]
    out = torch.empty(3, device=dev, dtype=torch.float32)
    zst = torch.empty((N, packed.K0), device=dev, dtype=torch.float32) if ste else None
    ws = torch.empty(lib.lipvq_mse_workspace_bytes(), device=dev, dtype=torch.uint8)
    with _on(dev):
        check(lib.lipvq_mlp3_loss_f32(_ptr(x), _ptr(gather_idx), _ptr(packed.buf), _ptr(y), _ptr(pre[0]), _ptr(pre[1]), _ptr(pre[2]),
                                      N, packed.K0, packed.J0, packed.J1, packed.J2, int(acts[0]), int(acts[1]), int(acts[2]),
                                      _ptr(target), _ptr(latent), _ptr(zst), _ptr(out), float(w), int(form), _ptr(ws), _stream()),
              "lipvq_mlp3_loss_f32")
    if ste:
        return y, (pre if save_pre else None), out, zst
    return y, (pre if save_pre else None), out


def nearest(z: torch.Tensor, codebook: torch.Tensor, dist: int = DIST_NORM, usage: torch.Tensor | None = None,
            want_zq: bool = True, want_best: bool = False):
    """(idx[N] int64, zq[N,D] or None, best[N] or None); usage[K] int64 is accumulated in place."""
    z, codebook = _chk(z, "z"), _chk(codebook, "codebook")
    N, D = z.shape
    K = codebook.shape[0]
    if codebook.shape[1] != D:
        raise ValueError(f"nearest: codebook must be [K,{D}], got {tuple(codebook.shape)}")
    if usage is not None:
        usage = _chk(usage, "usage", torch.int64)
        if usage.numel() != K:
            raise ValueError("nearest: usage must have K entries")
    idx = torch.empty(N, device=z.device, dtype=torch.int64)
    zq = torch.empty_like(z) if want_zq else None
    best = torch.empty(N, device=z.device, dtype=torch.float32) if want_best else None
    with _on(z.device):
        check(lib.lipvq_nearest_f32(_ptr(z), _ptr(codebook), _ptr(idx), _ptr(zq), _ptr(usage), _ptr(best),
                                    N, K, D, int(dist), _stream()), "lipvq_nearest_f32")
    return idx, zq, best


def ste(ze: torch.Tensor, zq: torch.Tensor) -> torch.Tensor:
    ze, zq = _chk(ze, "ze"), _chk(zq, "zq")
    out = torch.empty_like(ze)
    with _on(ze.device):
        check(lib.lipvq_ste_f32(_ptr(ze), _ptr(zq), _ptr(out), ze.numel(), _stream()), "lipvq_ste_f32")
    return out


def mse_pair(xr, x, zq, ze) -> torch.Tensor:
    """tensor([mean((xr-x)^2), mean((zq-ze)^2)]) on the device."""
    xr, x, zq, ze = _chk(xr, "xr"), _chk(x, "x"), _chk(zq, "zq"), _chk(ze, "ze")
    if x.numel() == 0 or ze.numel() == 0:        # F.mse_loss of an empty tensor is nan
        return torch.full((2,), float("nan"), device=x.device, dtype=torch.float32)
    out = torch.empty(2, device=x.device, dtype=torch.float32)
    ws = torch.empty(lib.lipvq_mse_workspace_bytes(), device=x.device, dtype=torch.uint8)
    with _on(x.device):
        check(lib.lipvq_mse_pair_f32(_ptr(xr), _ptr(x), x.numel(), _ptr(zq), _ptr(ze), ze.numel(), _ptr(out),
                                     _ptr(ws), _stream()), "lipvq_mse_pair_f32")
    return out


LOSS_LLFQ, LOSS_VQ = 0, 1


def mse_pair_loss(xr, x, zq, ze, w: float, form: int) -> torch.Tensor:
    """tensor([mean((xr-x)^2), mean((zq-ze)^2), loss]): the two means and the tokenizer's loss built from them on the device
    (LOSS_LLFQ: (m0 + w m1) + w m1;  LOSS_VQ: m0 + (m1 + w m1)) -- the reference's fp32 association, no torch arithmetic."""
    xr, x, zq, ze = _chk(xr, "xr"), _chk(x, "x"), _chk(zq, "zq"), _chk(ze, "ze")
    if x.numel() == 0 or ze.numel() == 0:        # F.mse_loss of an empty tensor is nan
        return torch.full((3,), float("nan"), device=x.device, dtype=torch.float32)
    out = torch.empty(3, device=x.device, dtype=torch.float32)
    ws = torch.empty(lib.lipvq_mse_workspace_bytes(), device=x.device, dtype=torch.uint8)
    with _on(x.device):
        check(lib.lipvq_mse_pair_loss_f32(_ptr(xr), _ptr(x), x.numel(), _ptr(zq), _ptr(ze), ze.numel(), _ptr(out), float(w), int(form),
                                          _ptr(ws), _stream()), "lipvq_mse_pair_loss_f32")
    return out


# ---- backward ---------------------------------------------------------------------------------

def mlp3_pack_bwd(W0, W1, W2) -> PackedMlp3:
    """Transposed weights of a stack for the backward-data chain (J2 -> J1 -> J0 -> K0)."""
    W0, W1, W2 = _chk(W0, "W0"), _chk(W1, "W1"), _chk(W2, "W2")
    J0, K0 = W0.shape
    J1, J2 = W1.shape[0], W2.shape[0]
    n = lib.lipvq_mlp3_packed_bwd_floats(K0, J0, J1, J2)
    buf = torch.empty(n, device=W0.device, dtype=torch.float32)
    with _on(W0.device):
        check(lib.lipvq_mlp3_pack_bwd_f32(_ptr(W0), _ptr(W1), _ptr(W2), _ptr(buf), K0, J0, J1, J2, _stream()),
              "lipvq_mlp3_pack_bwd_f32")
    return PackedMlp3(buf, K0, J0, J1, J2)


def mlp3_pack_bwd2(a, b):
    """mlp3_pack_bwd of two stacks, a = (W0, W1, W2) and b = (W0, W1, W2), in one launch -> (PackedMlp3, PackedMlp3)."""
    (aW0, aW1, aW2), (bW0, bW1, bW2) = ([_chk(t, "W") for t in a], [_chk(t, "W") for t in b])
    dims = []
    bufs = []
    for W0, W1, W2 in ((aW0, aW1, aW2), (bW0, bW1, bW2)):
        J0, K0 = W0.shape
        J1, J2 = W1.shape[0], W2.shape[0]
        dims.append((K0, J0, J1, J2))
        bufs.append(torch.empty(lib.lipvq_mlp3_packed_bwd_floats(K0, J0, J1, J2), device=W0.device, dtype=torch.float32))
    with _on(aW0.device):
        check(lib.lipvq_mlp3_pack_bwd2_f32(_ptr(aW0), _ptr(aW1), _ptr(aW2), _ptr(bufs[0]), *dims[0],
                                           _ptr(bW0), _ptr(bW1), _ptr(bW2), _ptr(bufs[1]), *dims[1], _stream()), "lipvq_mlp3_pack_bwd2_f32")
    return PackedMlp3(bufs[0], *dims[0]), PackedMlp3(bufs[1], *dims[1])


def mlp3_bwd_vq_supported(N, packed_bwd: PackedMlp3) -> bool:
    """Can lipvq_mlp3_bwd_vq_f32 (the chain with the VQ losses' gradient terms folded in) take this batch and stack?"""
    p = packed_bwd
    return bool(lib.lipvq_mlp3_bwd_vq_supported(int(N), p.K0, p.J0, p.J1, p.J2))


def _diff_term(term, N, width, name):
    """(a, a_idx, b, b_idx, alpha) -> checked tensors; an operand is [N, width] rows or (with its index vector) a table of such rows."""
    if term is None:
        return None, None, None, None, 0.0
    a, ia, b, ib, alpha = term
    a = _chk(a, name + ".a") if a is not None else None           # (in_term only: None = the forward's output, act2(pre2))
    b = _chk(b, name + ".b")
    ia = _chk(ia, name + ".a_idx", torch.int64) if ia is not None else None
    ib = _chk(ib, name + ".b_idx", torch.int64) if ib is not None else None
    for t, i, nm in ((a, ia, "a"), (b, ib, "b")):
        if t is None:
            continue
        if t.dim() != 2 or t.shape[1] != width or (i is None and t.shape[0] != N) or (i is not None and i.numel() != N):
            raise ValueError(f"{name}.{nm}: expected [{N}, {width}] rows or a table with an index vector of {N} entries")
    return a, ia, b, ib, float(alpha)


def mlp3_bwd(gy, pre, packed_bwd: PackedMlp3, acts, want_gx=True, in_term=None, out_term=None, gscale=None):
    """(g2, g1, g0, gx): dL/d(pre-activation) of the three layers and dL/d(input).
    in_term / out_term = (a, a_idx, b, b_idx, alpha): gy := alpha * gscale * (A - B) (gy may then be None; a = None stands for
    the forward's own output act2(pre2)) / gx += alpha * gscale * (A - B), folded into the launch; one term per launch,
    mlp3_bwd_vq_supported() must hold."""
    pre0, pre1 = _chk(pre[0], "pre0"), _chk(pre[1], "pre1")
    pre2 = _chk(pre[2], "pre2") if pre[2] is not None else None
    p = packed_bwd
    N = pre0.shape[0]
    dev = pre0.device
    ident = int(acts[2]) == ACT_NONE
    fused = in_term is not None or out_term is not None
    if gy is not None:
        gy = _chk(gy, "gy")
    elif in_term is None:
        raise ValueError("mlp3_bwd: gy is required without an in_term")
    if in_term is not None or not ident:
        g2 = torch.empty((N, p.J2), device=dev, dtype=torch.float32)
    else:
        g2 = gy
    g1 = torch.empty((N, p.J1), device=dev, dtype=torch.float32)
    g0 = torch.empty((N, p.J0), device=dev, dtype=torch.float32)
    gx = torch.empty((N, p.K0), device=dev, dtype=torch.float32) if want_gx else None
    with _on(dev):
        if fused:
            if out_term is not None and not want_gx:
                raise ValueError("mlp3_bwd: an out_term needs want_gx")
            ia_, iai, ib_, ibi, ial = _diff_term(in_term, N, p.J2, "in_term")
            if ia_ is not None or iai is not None:
                raise ValueError("mlp3_bwd: in_term's A is the forward's own output act2(pre2): pass a = a_idx = None")
            oa_, oai, ob_, obi, oal = _diff_term(out_term, N, p.K0, "out_term")
            gs = _chk(gscale, "gscale") if gscale is not None else None
            check(lib.lipvq_mlp3_bwd_vq_f32(_ptr(gy), _ptr(pre0), _ptr(pre1), _ptr(pre2), _ptr(p.buf),
                                            _ptr(g2) if g2 is not gy else None, _ptr(g1), _ptr(g0), _ptr(gx), N, p.K0, p.J0,
                                            p.J1, p.J2, int(acts[0]), int(acts[1]), int(acts[2]),
                                            _ptr(ib_), _ptr(ibi), ial,
                                            _ptr(oa_), _ptr(oai), _ptr(ob_), _ptr(obi), oal, _ptr(gs), _stream()),
                  "lipvq_mlp3_bwd_vq_f32")
        else:
            check(lib.lipvq_mlp3_bwd_f32(_ptr(gy), _ptr(pre0), _ptr(pre1), _ptr(pre2), _ptr(p.buf),
                                         None if ident else _ptr(g2), _ptr(g1), _ptr(g0), _ptr(gx), N, p.K0, p.J0,
                                         p.J1, p.J2, int(acts[0]), int(acts[1]), int(acts[2]), _stream()),
                  "lipvq_mlp3_bwd_f32")
    return g2, g1, g0, gx


def wgrad(G, H, h_act=ACT_NONE, hidx=None, want_bias=True):
    """(gW[J,Kd], gb[J]) of one Linear layer; H is the layer input (saved pre-activation + h_act,
    a raw tensor, or -- with hidx -- a table whose rows hidx select)."""
    G, H = _chk(G, "G"), _chk(H, "H")
    N, J = G.shape
    Kd = H.shape[1]
    if hidx is not None:
        hidx = _chk(hidx, "hidx", torch.int64)
    elif H.shape[0] != N:
        raise ValueError("wgrad: G and H must have the same number of rows")
    dev = G.device
    gW = torch.empty((J, Kd), device=dev, dtype=torch.float32)
    gb = torch.empty(J, device=dev, dtype=torch.float32) if want_bias else None
    ws = torch.empty(lib.lipvq_wgrad_workspace_bytes(N, J, Kd), device=dev, dtype=torch.uint8)
    with _on(dev):
        check(lib.lipvq_wgrad_f32(_ptr(G), _ptr(H), _ptr(hidx), int(h_act), _ptr(gW), _ptr(gb), _ptr(ws), N, J, Kd,
                                  _stream()), "lipvq_wgrad_f32")
    return gW, gb


def _scatter_route(N, K, D, deterministic=None):
    """THE rule of scatter_add / scatter_add_vq: "sequential_sorted" | "sequential_scan" where the sums must be in ascending row
    order (deterministic=None follows torch.are_deterministic_algorithms_enabled()), otherwise "sorted" -- the counting sort,
    for the shapes it takes from 65 536 rows on -- or "atomics"."""
    if deterministic is None:
        deterministic = torch.are_deterministic_algorithms_enabled()
    sortable = bool(lib.lipvq_scatter_add_sorted_supported(N, K, D))
    if deterministic:
        return "sequential_sorted" if sortable else "sequential_scan"
    return "sorted" if (sortable and N >= 65536) else "atomics"


def scatter_add(g, idx, K, deterministic=None, route=None):
    """gC[k] = sum of the rows of g whose idx is k (the gather's backward / index_add_).  deterministic=None follows
    torch.are_deterministic_algorithms_enabled(): strictly ascending row order per code, bit-identical to a sequential fp32
    index_add_.  Large batches go through a stable counting sort of the rows by code (csrc/lipvq_scatter.hip; no
    floating-point atomics): deterministic from 32 768 rows on (2.6 ms -> 0.1 ms at N = 524 288), otherwise from 65 536 rows
    on in 256-row segments (reproducible run to run; 70 vs 185 us) -- smaller batches: the scanning kernel / fp32 atomics.
    route = "atomics" | "sorted" | "sequential_sorted" | "sequential_scan" forces one (tests, measurements)."""
    g, idx = _chk(g, "g"), _chk(idx, "idx", torch.int64)
    N, D = g.shape
    if route is None:
        route = _scatter_route(N, K, D, deterministic)
    gC = torch.zeros((K, D), device=g.device, dtype=torch.float32)
    with _on(g.device):
        if route == "sequential_scan":
            check(lib.lipvq_scatter_add_det_f32(_ptr(g), _ptr(idx), _ptr(gC), N, K, D, _stream()), "lipvq_scatter_add_det_f32")
        elif route in ("sorted", "sequential_sorted"):
            ws = torch.empty(lib.lipvq_scatter_add_sorted_workspace_bytes(N, K, D), device=g.device, dtype=torch.uint8)
            check(lib.lipvq_scatter_add_sorted_f32(_ptr(g), _ptr(idx), _ptr(gC), _ptr(ws), N, K, D,
                                                   1 if route == "sequential_sorted" else 0, _stream()), "lipvq_scatter_add_sorted_f32")
        elif route == "atomics":
            check(lib.lipvq_scatter_add_f32(_ptr(g), _ptr(idx), _ptr(gC), N, K, D, _stream()), "lipvq_scatter_add_f32")
        else:
            raise ValueError(f"scatter_add: unknown route {route!r}")
    return gC


def scatter_add_vq(g, ze, table, idx, alpha, gscale=None, zq=None, deterministic=None):
    """gC[k] = sum over the rows n with idx[n] = k of  alpha * gscale * (table[k] - ze[n]) (+ g[n] when g is given):
    the codebook gradient of a training step -- the codebook-loss term formed per row plus what the decoder sent back --
    without the [N, D] intermediate.  Batches the counting-sort scatter takes (scatter_add's rule) form the rows inside its
    summing kernel (lipvq_scatter_add_sorted_vq_f32); smaller ones run scaled_diff + scatter_add: the same numbers either way."""
    ze, table, idx = _chk(ze, "ze"), _chk(table, "table"), _chk(idx, "idx", torch.int64)
    if g is not None:
        g = _chk(g, "g")
    N, D = ze.shape
    K = table.shape[0]
    if gscale is not None:
        gscale = _chk(gscale.reshape(1), "gscale")
    route = _scatter_route(N, K, D, deterministic)
    if route in ("sequential_scan", "atomics"):
        return scatter_add(scaled_diff(zq if zq is not None else table[idx], ze, alpha, gscale=gscale, c=g), idx, K, route=route)
    gC = torch.zeros((K, D), device=ze.device, dtype=torch.float32)
    ws = torch.empty(lib.lipvq_scatter_add_sorted_workspace_bytes(N, K, D), device=ze.device, dtype=torch.uint8)
    with _on(ze.device):
        check(lib.lipvq_scatter_add_sorted_vq_f32(_ptr(g), _ptr(ze), _ptr(table), float(alpha), _ptr(gscale), _ptr(idx), _ptr(gC),
                                                  _ptr(ws), N, K, D, 1 if route == "sequential_sorted" else 0, _stream()),
              "lipvq_scatter_add_sorted_vq_f32")
    return gC


def lipschitz_bwd(W, ci, gWn):
    W, ci, gWn = _chk(W, "W"), _chk(ci, "ci"), _chk(gWn, "gWn")
    gW, gci = torch.empty_like(W), torch.empty_like(ci)
    with _on(W.device):
        check(lib.lipvq_lipschitz_bwd_f32(_ptr(W), _ptr(ci), _ptr(gWn), _ptr(gW), _ptr(gci), W.shape[0], W.shape[1],
                                          _stream()), "lipvq_lipschitz_bwd_f32")
    return gW, gci


def scaled_diff(a, b, alpha, gscale=None, c=None):
    """alpha * gscale * (a - b) + c, gscale a 0-dim/1-element device tensor (the upstream dL/dloss)."""
    a, b = _chk(a, "a"), _chk(b, "b")
    if c is not None:
        c = _chk(c, "c")
    if gscale is not None:
        gscale = _chk(gscale.reshape(1), "gscale")
    out = torch.empty_like(a)
    with _on(a.device):
        check(lib.lipvq_scaled_diff_f32(_ptr(a), _ptr(b), _ptr(c), float(alpha), _ptr(gscale), _ptr(out), a.numel(),
                                        _stream()), "lipvq_scaled_diff_f32")
    return out


# ---- nearest code, screened fast path ------------------------------------------------------------

class PreparedCodebook:
    """Per-codebook data of the MFMA screen (lipvq_nearest_prepare_f32); rebuild when the codebook changes."""

    __slots__ = ("buf", "K", "D")

    def __init__(self, buf, K, D):
        self.buf, self.K, self.D = buf, K, D


def nearest_screen_supported(K: int, D: int) -> bool:
    return bool(lib.lipvq_nearest_screened_supported(int(K), int(D)))


def screen_is_coarse(K: int, D: int) -> bool:
    """True if the screened routes would run the one-product screen for this shape now (lipvq_screen_is_coarse)."""
    return bool(lib.lipvq_screen_is_coarse(int(K), int(D)))


def nearest_prepare(codebook: torch.Tensor) -> PreparedCodebook:
    codebook = _chk(codebook, "codebook")
    K, D = codebook.shape
    buf = torch.empty(lib.lipvq_nearest_prep_bytes(K, D), device=codebook.device, dtype=torch.uint8)
    with _on(codebook.device):
        check(lib.lipvq_nearest_prepare_f32(_ptr(codebook), _ptr(buf), K, D, _stream()), "lipvq_nearest_prepare_f32")
    return PreparedCodebook(buf, K, D)


_small_ws: dict = {}          # (device index, stream handle) -> zero-at-rest workspace of lipvq_nearest_small_f32


def _nearest_small_workspace(N, K, dev):
    """The chip-wide small-batch kernel meets a row's partial minima behind per-row-group counters that are zero between
    launches (the last workgroup resets them): one zero-filled buffer per (device, stream) serves every EAGER call -- no fill
    launch per call.  Under stream capture every call gets its own zeroed buffer (one memset node)."""
    need = lib.lipvq_nearest_small_workspace_bytes(N, K)
    if torch.cuda.is_current_stream_capturing():
        # Never shared across captures: a cached buffer's zero fill would be a node of the FIRST graph that used it only (a
        # second graph replayed first, or two graphs on two streams, would meet on uninitialised or shared counters).  A fresh
        # zeroed buffer per call puts the fill into this graph and the buffer into this graph's private pool.
        return torch.zeros(need, device=dev, dtype=torch.uint8)
    key = (dev.index, _stream())
    ws = _small_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _small_ws[key] = torch.zeros(max(need, 1 << 16), device=dev, dtype=torch.uint8)
    return ws


def nearest_rows(z, codebook, usage=None, want_zq=True, dist: int = DIST_NORM, route=None):
    """(idx, zq) exactly as nearest(z, codebook, dist), every row decided by an exact kernel (no prepared codebook): the
    route for small batches.  Up to 4 096 rows run lipvq_nearest_small_f32 (4 rows x 64 codes per workgroup, the whole chip
    busy at 80 rows), larger ones the row kernels (route = "small" | "rows" forces one: tests, measurements)."""
    z, codebook = _chk(z, "z"), _chk(codebook, "codebook")
    N, D = z.shape
    K = codebook.shape[0]
    if codebook.shape[1] != D:
        raise ValueError("nearest_rows: codebook width does not match")
    if usage is not None:
        usage = _chk(usage, "usage", torch.int64)
    if dist not in (DIST_NORM, DIST_SQSUM):
        raise ValueError(f"nearest_rows: unknown distance rule {dist}")
    idx = torch.empty(N, device=z.device, dtype=torch.int64)
    zq = torch.empty_like(z) if want_zq else None
    small = bool(lib.lipvq_nearest_small_supported(N, K, D)) if route is None else route == "small"
    if small and N > 0:
        with _on(z.device):
            ws = _nearest_small_workspace(N, K, z.device)
            check(lib.lipvq_nearest_small_f32(_ptr(z), _ptr(codebook), _ptr(idx), _ptr(zq), _ptr(usage), _ptr(ws), N, K, D, int(dist),
                                              _stream()), "lipvq_nearest_small_f32")
        return idx, zq
    fn, name = ((lib.lipvq_nearest_rows_f32, "lipvq_nearest_rows_f32") if dist == DIST_NORM else
                (lib.lipvq_vq_nearest_rows_f32, "lipvq_vq_nearest_rows_f32"))
    if dist not in (DIST_NORM, DIST_SQSUM):
        raise ValueError(f"nearest_rows: unknown distance rule {dist}")
    with _on(z.device):
        check(fn(_ptr(z), _ptr(codebook), _ptr(idx), _ptr(zq), _ptr(usage), N, K, D, _stream()), name)
    return idx, zq


def nearest_screened(z, codebook, prep: PreparedCodebook, usage=None, want_zq=True, return_workspace=False,
                     debug_gamma=None, dist: int = DIST_NORM):
    """Same results as nearest(z, codebook, dist), via MFMA screening + exact re-scoring of the
    rows the screen cannot certify.  With return_workspace the int32 workspace is returned too
    (element 0 = number of rows decided by the exact kernel).  debug_gamma: test hook, returns the
    approximate distance matrix as well."""
    z, codebook = _chk(z, "z"), _chk(codebook, "codebook")
    N, D = z.shape
    K = codebook.shape[0]
    if (prep.K, prep.D) != (K, D) or codebook.shape[1] != D:
        raise ValueError("nearest_screened: prepared codebook does not match")
    if usage is not None:
        usage = _chk(usage, "usage", torch.int64)
    dev = z.device
    idx = torch.empty(N, device=dev, dtype=torch.int64)
    zq = torch.empty_like(z) if want_zq else None
    ws = torch.empty(max(16, lib.lipvq_nearest_workspace_bytes(N) // 4), device=dev, dtype=torch.int32)
    dt = None
    if dist not in (DIST_NORM, DIST_SQSUM) or (dist != DIST_NORM and debug_gamma is not None):
        raise ValueError("nearest_screened: unknown distance rule (the debug hook runs the norm rule only)")
    with _on(dev):
        if debug_gamma is None and dist == DIST_SQSUM:        # the plain VQVAE's rule (vq:57-63)
            check(lib.lipvq_vq_nearest_screened_f32(_ptr(z), _ptr(codebook), _ptr(prep.buf), _ptr(idx), _ptr(zq),
                                                    _ptr(usage), _ptr(ws), N, K, D, _stream()),
                  "lipvq_vq_nearest_screened_f32")
        elif debug_gamma is None:
            check(lib.lipvq_nearest_screened_f32(_ptr(z), _ptr(codebook), _ptr(prep.buf), _ptr(idx), _ptr(zq),
                                                 _ptr(usage), _ptr(ws), N, K, D, _stream()),
                  "lipvq_nearest_screened_f32")
        else:
            kpad = (K + 31) // 32 * 32
            dt = torch.empty((N, kpad), device=dev, dtype=torch.float32)
            check(lib.lipvq_screen_debug_f32(_ptr(z), _ptr(codebook), _ptr(prep.buf), _ptr(idx), _ptr(zq),
                                             _ptr(usage), _ptr(ws), _ptr(dt), float(debug_gamma), N, K, D,
                                             _stream()), "lipvq_screen_debug_f32")
    out = (idx, zq)
    if return_workspace:
        out = out + (ws,)
    if debug_gamma is not None:
        out = out + (dt,)
    return out


# ---- fused encode + quantize ------------------------------------------------------------------------

def tokenize_supported(A, J0, J1, D, K) -> bool:
    return bool(lib.lipvq_tokenize_supported(int(A), int(J0), int(J1), int(D), int(K)))


def tokenize_fast_supported(A, J0, J1, D, K) -> bool:
    return bool(lib.lipvq_tokenize_fast_supported(int(A), int(J0), int(J1), int(D), int(K)))


def tokenize_workspace(N: int, D: int, device) -> torch.Tensor:
    """int32 workspace of lipvq_tokenize_f32 (row list + z_e scratch) with its header zeroed (lipvq_tokenize_workspace_init: the
    fused calls keep the header's counters at zero themselves); callers may keep and reuse it -- on one stream at a time."""
    ws = torch.empty(max(16, (lib.lipvq_tokenize_workspace_bytes(N, D) + 3) // 4), device=device, dtype=torch.int32)
    with _on(ws.device):
        check(lib.lipvq_tokenize_workspace_init(_ptr(ws), _stream()), "lipvq_tokenize_workspace_init")
    return ws


def mlp3_pack_f16(W0, W1, W2):
    """fp16 MFMA fragments of an encoder stack for the fast tokenize mode (uint8 buffer)."""
    W0, W1, W2 = _chk(W0, "W0"), _chk(W1, "W1"), _chk(W2, "W2")
    A, J0, J1, D = W0.shape[1], W0.shape[0], W1.shape[0], W2.shape[0]
    nbytes = lib.lipvq_mlp3_packed_f16_bytes(A, J0, J1, D)
    if not nbytes or W1.shape[1] != J0 or W2.shape[1] != J1:
        raise ValueError("mlp3_pack_f16: unsupported stack shape")
    buf = torch.empty(nbytes, device=W0.device, dtype=torch.uint8)
    with _on(W0.device):
        check(lib.lipvq_mlp3_pack_f16_f32(_ptr(W0), _ptr(W1), _ptr(W2), _ptr(buf), A, J0, J1, D, _stream()),
              "lipvq_mlp3_pack_f16_f32")
    return buf


def tokenize(x, packed: PackedMlp3, raw, codebook, prep: PreparedCodebook, usage=None, want_zq=True, want_ze=False,
             workspace=None, packed16=None, want_pre=False):
    """(idx, zq, ze, workspace) of the fused encode + quantize launch (lipvq_tokenize_f32).  raw = the encoder's six
    unpacked tensors (W0, b0, W1, b1, W2 normalised, b2): the exact kernel re-encodes uncertified rows with them.
    want_pre=True (training forward, lipvq_tokenize_train_f32): also returns the three pre-activations as a 5th element."""
    raw = tuple(_chk(t, f"raw[{i}]") for i, t in enumerate(raw))
    raw_arr = (_C.c_void_p * 6)(*[t.data_ptr() for t in raw])
    x, codebook = _chk(x, "x"), _chk(codebook, "codebook")
    N, A = x.shape
    K, D = codebook.shape
    if (packed.K0, packed.J2) != (A, D) or (prep.K, prep.D) != (K, D):
        raise ValueError("tokenize: packed encoder / prepared codebook do not match the inputs")
    if usage is not None:
        usage = _chk(usage, "usage", torch.int64)
    dev = x.device
    idx = torch.empty(N, device=dev, dtype=torch.int64)
    zq = torch.empty((N, D), device=dev, dtype=torch.float32) if want_zq else None
    ze = torch.empty((N, D), device=dev, dtype=torch.float32) if (want_ze or want_pre) else None
    ws = workspace if workspace is not None else tokenize_workspace(N, D, dev)
    if want_pre:
        if packed16 is not None:
            raise ValueError("tokenize: the fast mode has no training variant")
        pre = (torch.empty((N, packed.J0), device=dev, dtype=torch.float32), torch.empty((N, packed.J1), device=dev, dtype=torch.float32),
               torch.empty((N, D), device=dev, dtype=torch.float32))
        with _on(dev):
            check(lib.lipvq_tokenize_train_f32(_ptr(x), _ptr(packed.buf), raw_arr, _ptr(codebook), _ptr(prep.buf), _ptr(idx), _ptr(zq),
                                               _ptr(usage), _ptr(ze), _ptr(pre[0]), _ptr(pre[1]), _ptr(pre[2]), _ptr(ws), N, A,
                                               packed.J0, packed.J1, D, K, _stream()), "lipvq_tokenize_train_f32")
        return idx, zq, ze, ws, pre
    with _on(dev):
        if packed16 is not None:            # fast mode (fp16 encoder GEMMs): not bit-identical, see include/lipvq.h
            if want_ze:
                raise ValueError("tokenize: the fast mode does not return z_e")
            check(lib.lipvq_tokenize_fast_f32(_ptr(x), _ptr(packed.buf), _ptr(packed16), raw_arr, _ptr(codebook), _ptr(prep.buf),
                                              _ptr(idx), _ptr(zq), _ptr(usage), _ptr(ws), N, A, packed.J0, packed.J1, D, K,
                                              _stream()), "lipvq_tokenize_fast_f32")
        else:
            check(lib.lipvq_tokenize_f32(_ptr(x), _ptr(packed.buf), raw_arr, _ptr(codebook), _ptr(prep.buf), _ptr(idx), _ptr(zq),
                                         _ptr(usage), _ptr(ze), _ptr(ws), N, A, packed.J0, packed.J1, D, K, _stream()),
                  "lipvq_tokenize_f32")
    return idx, zq, ze, ws


def tokenize_tune(x, packed: PackedMlp3, raw, codebook, prep: PreparedCodebook, workspace=None, launches=150):
    """lipvq_tokenize_tune_f32: time the fused launch's four device-dependent schedule combinations (identical results) on this
    device, shape and data and keep the fastest for the process.  Synchronous.  Returns (choice, [ms per launch] * 4) with
    choice = defer_ze | nt_ze << 1."""
    raw = tuple(_chk(t, f"raw[{i}]") for i, t in enumerate(raw))
    raw_arr = (_C.c_void_p * 6)(*[t.data_ptr() for t in raw])
    x, codebook = _chk(x, "x"), _chk(codebook, "codebook")
    N, A = x.shape
    K, D = codebook.shape
    if (packed.K0, packed.J2) != (A, D) or (prep.K, prep.D) != (K, D):
        raise ValueError("tokenize_tune: packed encoder / prepared codebook do not match the inputs")
    dev = x.device
    idx = torch.empty(N, device=dev, dtype=torch.int64)
    zq = torch.empty((N, D), device=dev, dtype=torch.float32)
    usage = torch.zeros(K, device=dev, dtype=torch.int64)           # scratch: every timed launch accumulates into it
    ws = workspace if workspace is not None else tokenize_workspace(N, D, dev)
    choice = _C.c_int(-1)
    ms4 = (_C.c_float * 4)()
    with _on(dev):
        check(lib.lipvq_tokenize_tune_f32(_ptr(x), _ptr(packed.buf), raw_arr, _ptr(codebook), _ptr(prep.buf), _ptr(idx), _ptr(zq),
                                          _ptr(usage), None, _ptr(ws), N, A, packed.J0, packed.J1, D, K, _stream(), int(launches),
                                          _C.byref(choice), ms4), "lipvq_tokenize_tune_f32")
    return int(choice.value), [float(v) for v in ms4]


def vq_tokenize(x, packed: PackedMlp3, codebook, prep: PreparedCodebook, usage=None, workspace=None, want_pre=False):
    """(idx, zq, ze, workspace) of the plain VQVAE's fused encode + quantize launch (lipvq_vq_tokenize_f32: ReLU encoder,
    `pow(2).sum(-1)` argmin): the same results as mlp3(relu x 3) + nearest(DIST_SQSUM).  z_e is always returned (the
    straight-through value needs it).  want_pre: (idx, zq, ze, [pre0, pre1, pre2], workspace) -- the training forward,
    lipvq_vq_tokenize_train_f32."""
    x, codebook = _chk(x, "x"), _chk(codebook, "codebook")
    N, A = x.shape
    K, D = codebook.shape
    if (packed.K0, packed.J2) != (A, D) or (prep.K, prep.D) != (K, D):
        raise ValueError("vq_tokenize: packed encoder / prepared codebook do not match the inputs")
    if usage is not None:
        usage = _chk(usage, "usage", torch.int64)
    dev = x.device
    idx = torch.empty(N, device=dev, dtype=torch.int64)
    zq = torch.empty((N, D), device=dev, dtype=torch.float32)
    ze = torch.empty((N, D), device=dev, dtype=torch.float32)
    ws = workspace if workspace is not None else tokenize_workspace(N, D, dev)
    if want_pre:
        pre = [torch.empty((N, J), device=dev, dtype=torch.float32) for J in (packed.J0, packed.J1, D)]
        with _on(dev):
            check(lib.lipvq_vq_tokenize_train_f32(_ptr(x), _ptr(packed.buf), _ptr(codebook), _ptr(prep.buf), _ptr(idx), _ptr(zq),
                                                  _ptr(usage), _ptr(ze), _ptr(pre[0]), _ptr(pre[1]), _ptr(pre[2]), _ptr(ws), N, A,
                                                  packed.J0, packed.J1, D, K, _stream()), "lipvq_vq_tokenize_train_f32")
        return idx, zq, ze, pre, ws
    with _on(dev):
        check(lib.lipvq_vq_tokenize_f32(_ptr(x), _ptr(packed.buf), _ptr(codebook), _ptr(prep.buf), _ptr(idx), _ptr(zq), _ptr(usage),
                                        _ptr(ze), _ptr(ws), N, A, packed.J0, packed.J1, D, K, _stream()), "lipvq_vq_tokenize_f32")
    return idx, zq, ze, ws


# ---------------------------------------------------------------------------------------------------
# the in-kernel dropout source (csrc/lipvq_rng.h, csrc/lipvq_rng.hip; include/lipvq.h, "in-kernel dropout"): the wrappers below
# that take dropout=(snap, site, p) pick the library's _drop entry point of their kernel family
# ---------------------------------------------------------------------------------------------------

# the site words of the modules outside the backbone (include/lipvq.h): the backbone's are 4 layer + {0, 1, 2}
DROPOUT_SITE_EMBED = 0x40000000
DROPOUT_SITE_DEFAULT = 0x80000000


def dropout_begin(state):
    """snap, a fresh int64[2] device tensor = the (seed, step) of ``state`` (int64[2], device) as it was; ``state``'s step is
    advanced by one, on the device: one one-thread launch, no host synchronisation."""
    if not isinstance(state, torch.Tensor) or state.dtype != torch.int64 or state.shape != (2,) or not state.is_cuda or not state.is_contiguous():
        raise ValueError("dropout_begin: state must be a contiguous int64[2] device tensor (seed, step)")
    snap = torch.empty(2, device=state.device, dtype=torch.int64)
    with _on(state.device):
        check(lib.lipvq_dropout_begin(_ptr(state), _ptr(snap), _stream()), "lipvq_dropout_begin")
    return snap


def dropout_keep(snap, site: int, rows: int, cols: int, p: float):
    """The decisions of one site as a uint8 [rows, cols] device tensor (1 kept, 0 dropped), from a snap of dropout_begin."""
    if not isinstance(snap, torch.Tensor) or snap.dtype != torch.int64 or snap.numel() != 2 or not snap.is_cuda or not snap.is_contiguous():
        raise ValueError("dropout_keep: snap must be a contiguous int64[2] device tensor")
    ok = 0 <= int(rows) < 2 ** 32 and 0 <= int(cols) <= 2 ** 32            # (anything else the library refuses before it writes)
    out = torch.empty((int(rows), int(cols)) if ok else (0, 0), device=snap.device, dtype=torch.uint8)
    with _on(snap.device):
        check(lib.lipvq_dropout_keep_u8(_ptr(snap), int(site), int(rows), int(cols), float(p), _ptr(out), _stream()), "lipvq_dropout_keep_u8")
    return out


def dropout_keep_host(seed: int, step: int, site: int, rows: int, cols: int, p: float):
    """The same field as a uint8 [rows, cols] CPU tensor from (seed, step), computed on the host: no GPU call."""
    ok = 0 <= int(rows) < 2 ** 32 and 0 <= int(cols) <= 2 ** 32
    out = torch.empty((int(rows), int(cols)) if ok else (0, 0), dtype=torch.uint8)
    check(lib.lipvq_dropout_keep_host(int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), int(site), int(rows), int(cols), float(p),
                                      out.data_ptr()), "lipvq_dropout_keep_host")
    return out


def _dropout_args(what, dropout, dev, keep=None):
    """dropout = (snap, site, p) of the in-kernel source (include/lipvq.h, "in-kernel dropout") -> (snap, site, p) checked."""
    if keep is not None:
        raise ValueError(f"{what}: keep (mask bytes) and dropout (the in-kernel source) are mutually exclusive")
    snap, site, p = dropout
    if not isinstance(snap, torch.Tensor) or snap.dtype != torch.int64 or snap.numel() != 2 or not snap.is_contiguous() or snap.device != dev:
        raise ValueError(f"{what}: snap must be the contiguous int64[2] tensor of dropout_begin on the input's device")
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f"{what}: dropout p={p} (0 < p < 1; p == 0 is the plain form)")
    return snap, int(site), p


# ---------------------------------------------------------------------------------------------------
# the step after the tokenizer: input embedding + interleave (csrc/lipvq_embed.hip)
# ---------------------------------------------------------------------------------------------------

def linear(x, W, b=None, act=ACT_NONE, save_pre=False, *, dropout=None):
    """y = act(x . W^T + b) (nn.Linear), canonical fp32 (reference obs_nets.py:2536 `embed_encoder`; with act = GELU the
    second half of AdaptiveBinActionEmbedding.output_layer).  save_pre=True returns (y, pre-activation).
    dropout=(snap, site, p): the stored y is act(x . W^T + b) * m, m = 1 / (1 - p) where the in-kernel source keeps (row, col) of
    the [N, E] result and 0 where it drops it, decided inside the Linear's epilogue (no mask tensor); pre stays the plain one."""
    x, W = _chk(x, "x"), _chk(W, "W")
    if x.dim() != 2 or W.dim() != 2 or W.shape[1] != x.shape[1]:
        raise ValueError(f"linear: x {tuple(x.shape)} and W {tuple(W.shape)} do not match")
    if b is not None:
        b = _chk(b, "b")
        if b.shape != (W.shape[0],):
            raise ValueError("linear: bias shape")
    if dropout is not None:
        snap, site, p = _dropout_args("linear", dropout, x.device)
    N, Kin = x.shape
    E = W.shape[0]
    y = torch.empty((N, E), device=x.device, dtype=torch.float32)
    pre = torch.empty_like(y) if save_pre else None
    with _on(x.device):
        if dropout is not None:
            check(lib.lipvq_linear_act_drop_f32(_ptr(x), _ptr(W), _ptr(b), _ptr(y), _ptr(pre), _ptr(snap), site, p, N, Kin, E, int(act),
                                                _stream()), "lipvq_linear_act_drop_f32")
        else:
            check(lib.lipvq_linear_act_f32(_ptr(x), _ptr(W), _ptr(b), _ptr(y), _ptr(pre), N, Kin, E, int(act), _stream()),
                  "lipvq_linear_act_f32")
    return (y, pre) if save_pre else y


def _bf16_widths(what, Kin, E):
    if Kin % 8 or E % 8:
        raise ValueError(f"{what}: the bf16 mode needs both Linear widths to be multiples of 8 (got {Kin} -> {E})")


def _linear_pipe(name, entry, x, W, b, act, save_pre, dropout):
    if dropout is not None:
        raise ValueError(f"{name}: the in-kernel dropout source has fp32 entry points only (use linear)")
    x, W = _chk(x, "x"), _chk(W, "W")
    if x.dim() != 2 or W.dim() != 2 or W.shape[1] != x.shape[1]:
        raise ValueError(f"{name}: x {tuple(x.shape)} and W {tuple(W.shape)} do not match")
    if b is not None:
        b = _chk(b, "b")
        if b.shape != (W.shape[0],):
            raise ValueError(f"{name}: bias shape")
    N, Kin = x.shape
    E = W.shape[0]
    _bf16_widths(name, Kin, E)
    y = torch.empty((N, E), device=x.device, dtype=torch.float32)
    pre = torch.empty_like(y) if save_pre else None
    with _on(x.device):
        check(getattr(lib, entry)(_ptr(x), _ptr(W), _ptr(b), _ptr(y), _ptr(pre), N, Kin, E, int(act), _stream()), entry)
    return (y, pre) if save_pre else y


def _linear_nn_pipe(name, entry, g, W):
    g, W = _chk(g, "g"), _chk(W, "W")
    if g.dim() != 2 or W.dim() != 2 or W.shape[0] != g.shape[1]:
        raise ValueError(f"{name}: g {tuple(g.shape)} and W {tuple(W.shape)} do not match")
    N, J = g.shape
    K = W.shape[1]
    _bf16_widths(name, K, J)
    gx = torch.empty((N, K), device=g.device, dtype=torch.float32)
    with _on(g.device):
        check(getattr(lib, entry)(_ptr(g), _ptr(W), _ptr(gx), N, J, K, _stream()), entry)
    return gx


def _wgrad_pipe(name, entry, G, H, want_bias):
    G, H = _chk(G, "G"), _chk(H, "H")
    if G.dim() != 2 or H.dim() != 2 or H.shape[0] != G.shape[0]:
        raise ValueError(f"{name}: G and H must be 2-D with the same number of rows")
    N, J = G.shape
    K = H.shape[1]
    _bf16_widths(name, K, J)
    dev = G.device
    if N == 0:
        return torch.zeros((J, K), device=dev), (torch.zeros(J, device=dev) if want_bias else None)
    gW = torch.empty((J, K), device=dev, dtype=torch.float32)
    gb = torch.empty(J, device=dev, dtype=torch.float32) if want_bias else None
    ws = torch.empty(lib.lipvq_wgrad_bf16_workspace_bytes(N, J, K), device=dev, dtype=torch.uint8)
    with _on(dev):
        check(getattr(lib, entry)(_ptr(G), _ptr(H), _ptr(gW), _ptr(gb), _ptr(ws), N, J, K, _stream()), entry)
    return gW, gb


def linear_bf16(x, W, b=None, act=ACT_NONE, save_pre=False, *, dropout=None):
    """``linear`` in the bf16 matrix-pipe mode: x and W are rounded to bf16 (nearest even) as the kernel reads them, products
    are accumulated in fp32, bias and activation are the fp32 epilogue of ``linear``; every tensor stays fp32."""
    return _linear_pipe("linear_bf16", "lipvq_linear_act_bf16", x, W, b, act, save_pre, dropout)


def linear_nn_bf16(g, W):
    """gx = g . W in the bf16 mode (the input gradient of ``linear_bf16``): W [J, K] is read as stored, no transposed copy."""
    return _linear_nn_pipe("linear_nn_bf16", "lipvq_linear_nn_bf16", g, W)


def wgrad_bf16(G, H, want_bias=True):
    """(gW[J,K], gb[J]) of one Linear in the bf16 mode: gW = G^T . H on bf16-rounded operands with fp32 accumulation, gb = the
    fp32 column sums of the unrounded G.  Row chunks are added in a fixed order: repeated calls give the same bits."""
    return _wgrad_pipe("wgrad_bf16", "lipvq_wgrad_bf16", G, H, want_bias)


def linear_bf16x3(x, W, b=None, act=ACT_NONE, save_pre=False, *, dropout=None):
    """``linear`` in the bf16x3 mode: every element of x and W is split into hi = bf16(v) and lo = bf16(v - hi) as the kernel
    reads it, and a_lo b_hi + a_hi b_lo + a_hi b_hi is accumulated in fp32 on the bf16 matrix pipe (about 2^-16 relative per
    product instead of 2^-8; include/lipvq.h has the bound).  The epilogue and the tensors are those of ``linear_bf16``."""
    return _linear_pipe("linear_bf16x3", "lipvq_linear_act_bf16x3", x, W, b, act, save_pre, dropout)


def linear_nn_bf16x3(g, W):
    """gx = g . W in the bf16x3 mode (the input gradient of ``linear_bf16x3``): W [J, K] is read as stored."""
    return _linear_nn_pipe("linear_nn_bf16x3", "lipvq_linear_nn_bf16x3", g, W)


def wgrad_bf16x3(G, H, want_bias=True):
    """(gW[J,K], gb[J]) of one Linear in the bf16x3 mode: gW = G^T . H with both operands split into two bf16 numbers and
    three products per element pair, gb = the fp32 column sums of the unrounded G.  The chunks, their order and the
    workspace are those of ``wgrad_bf16``: repeated calls give the same bits."""
    return _wgrad_pipe("wgrad_bf16x3", "lipvq_wgrad_bf16x3", G, H, want_bias)


def _embed_args(src, idx, pos, N, T, E):
    if src.dim() != 2 or src.shape[1] != E:
        raise ValueError(f"embed_rows: src {tuple(src.shape)} is not [rows, {E}]")
    if idx is not None:
        idx = _chk(idx, "idx", torch.int64).reshape(-1)
        if idx.numel() != N:
            raise ValueError("embed_rows: idx must hold one index per row")
    if pos is not None:
        pos = _chk(pos, "pos")
        if pos.shape != (T, E):
            raise ValueError(f"embed_rows: pos {tuple(pos.shape)} is not [{T}, {E}]")
    return idx, pos


def embed_rows(src, idx, pos, ln_w, ln_b, eps, out, N, T, bstride, tstride, offset, want_stats=False, dropout=None):
    """out[slot(n)] = LayerNorm(src[idx[n] | n] + pos[n % T]) * ln_w + ln_b, slot(b*T+t) = b*bstride + t*tstride + offset
    floats into ``out`` (reference obs_nets.py:2537-2540 and the interleave of :2584-2596).  Returns stats [N,2] or None.
    dropout=(snap, site, p): the stored rows are multiplied by the in-kernel source's mask factor, decided at (output row
    slot // E, column e); stats stay the pre-dropout statistics."""
    src, ln_w, ln_b, out = _chk(src, "src"), _chk(ln_w, "ln_w"), _chk(ln_b, "ln_b"), _chk(out, "out")
    E = ln_w.numel()
    idx, pos = _embed_args(src, idx, pos, N, T, E)
    if N:
        B = (N + T - 1) // T
        last = (B - 1) * bstride + (min(T, N) - 1) * tstride + offset + E
        if last > out.numel():
            raise ValueError("embed_rows: the output slots do not fit in `out`")
    stats = torch.empty((N, 2), device=src.device, dtype=torch.float32) if want_stats else None
    with _on(src.device):
        if dropout is not None:
            snap, site, p = _dropout_args("embed_rows", dropout, src.device)
            check(lib.lipvq_embed_rows_drop_f32(_ptr(src), _ptr(idx), _ptr(pos), _ptr(ln_w), _ptr(ln_b), float(eps), _ptr(out),
                                                _ptr(stats), _ptr(snap), site, p, N, T, E, src.shape[0], bstride, tstride, offset,
                                                _stream()), "lipvq_embed_rows_drop_f32")
            return stats
        check(lib.lipvq_embed_rows_f32(_ptr(src), _ptr(idx), _ptr(pos), _ptr(ln_w), _ptr(ln_b), float(eps), _ptr(out),
                                       _ptr(stats), N, T, E, src.shape[0], bstride, tstride, offset, _stream()),
              "lipvq_embed_rows_f32")
    return stats


def embed_rows_bwd(gout, src, idx, pos, stats, ln_w, g_src, g_pos, g_lnw, g_lnb, N, T, bstride, tstride, offset, dropout=None):
    """Backward of embed_rows; accumulates into g_src / g_pos / g_lnw / g_lnb (each may be None), every sum in a fixed order
    (lipvq_embed_rows_bwd_det_f32).  dropout=(snap, site, p) of the forward: gout is read as gout * m, the decisions regenerated."""
    gout, src, stats, ln_w = _chk(gout, "gout"), _chk(src, "src"), _chk(stats, "stats"), _chk(ln_w, "ln_w")
    E = ln_w.numel()
    idx, pos = _embed_args(src, idx, pos, N, T, E)
    for name, t, shape in (("g_src", g_src, tuple(src.shape)), ("g_pos", g_pos, (T, E)), ("g_lnw", g_lnw, (E,)),
                           ("g_lnb", g_lnb, (E,))):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32):
            raise ValueError(f"embed_rows_bwd: {name} must be a contiguous fp32 tensor of shape {shape}")
    if dropout is None:
        snap, site, p = None, 0, 0.0
    else:
        snap, site, p = _dropout_args("embed_rows_bwd", dropout, src.device)
    with _on(src.device):
        if T <= 1024:
            # every sum in a fixed order (partial sums per workgroup and a second pass; the table through the counting-sort or the
            # row-order scatter): no float atomics, the gradients repeat bit for bit
            nbytes = lib.lipvq_embed_rows_bwd_det_workspace_bytes(N, T, E, src.shape[0], int(idx is not None))
            ws = torch.empty(max(16, nbytes), device=src.device, dtype=torch.uint8)
            check(lib.lipvq_embed_rows_bwd_det_f32(_ptr(gout), _ptr(src), _ptr(idx), _ptr(pos), _ptr(stats), _ptr(ln_w), _ptr(g_src),
                                                   _ptr(g_pos), _ptr(g_lnw), _ptr(g_lnb), _ptr(ws), _ptr(snap), site, p, N, T, E,
                                                   src.shape[0], bstride, tstride, offset, _stream()), "lipvq_embed_rows_bwd_det_f32")
            return
        # more than 1024 time steps: the atomic kernel
        drop, sfx = ((), "") if dropout is None else ((_ptr(snap), site, p), "drop_")
        entry = f"lipvq_embed_rows_bwd_{sfx}f32"
        check(getattr(lib, entry)(_ptr(gout), _ptr(src), _ptr(idx), _ptr(pos), _ptr(stats), _ptr(ln_w),
                                  _ptr(g_src), _ptr(g_pos), _ptr(g_lnw), _ptr(g_lnb), *drop, N, T, E, src.shape[0],
                                  bstride, tstride, offset, _stream()), entry)


# ---------------------------------------------------------------------------------------------------
# AdaptiveBinActionEmbedding (csrc/lipvq_bin.hip; reference robomimic/models/bin_action/backbone.py)
# ---------------------------------------------------------------------------------------------------

def bin_minmax(actions, running_min, running_max):
    """In-place running min/max update (backbone.py:37-40)."""
    actions = _chk(actions, "actions")
    for name, t in (("running_min", running_min), ("running_max", running_max)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (actions.shape[1],)):
            raise ValueError(f"bin_minmax: {name} must be a contiguous fp32 CUDA tensor of shape [{actions.shape[1]}]")
    N, A = actions.shape
    with _on(actions.device):
        check(lib.lipvq_bin_minmax_f32(_ptr(actions), _ptr(running_min), _ptr(running_max), N, A, _stream()),
              "lipvq_bin_minmax_f32")


def bin_discretize(actions, running_min, running_max, num_bins):
    """bins [A, N] int64 (backbone.py:42-66; the reference's [N, A] stack is bins.t())."""
    actions, running_min, running_max = _chk(actions, "actions"), _chk(running_min, "running_min"), _chk(running_max, "running_max")
    N, A = actions.shape
    bins = torch.empty((A, N), device=actions.device, dtype=torch.int64)
    with _on(actions.device):
        check(lib.lipvq_bin_discretize_f32(_ptr(actions), _ptr(running_min), _ptr(running_max), _ptr(bins), N, A,
                                           int(num_bins), _stream()), "lipvq_bin_discretize_f32")
    return bins


def bin_boundaries(running_min, running_max, num_bins):
    """[A, num_bins + 1] bin boundaries (backbone.py:42-53)."""
    running_min, running_max = _chk(running_min, "running_min"), _chk(running_max, "running_max")
    A = running_min.numel()
    out = torch.empty((A, num_bins + 1), device=running_min.device, dtype=torch.float32)
    with _on(out.device):
        check(lib.lipvq_bin_boundaries_f32(_ptr(running_min), _ptr(running_max), _ptr(out), A, int(num_bins), _stream()),
              "lipvq_bin_boundaries_f32")
    return out


def bin_hidden(bins, P, b1, save_pre=False):
    """h = gelu(b1 + sum_i P[i][bins[i]]) (backbone.py:77-86 up to the first GELU).  P [A, num_bins, H]."""
    bins, P, b1 = _chk(bins, "bins", torch.int64), _chk(P, "P"), _chk(b1, "b1")
    A, N = bins.shape
    if P.dim() != 3 or P.shape[0] != A or b1.shape != (P.shape[2],):
        raise ValueError("bin_hidden: P must be [A, num_bins, H] and b1 [H]")
    nb, H = P.shape[1], P.shape[2]
    h = torch.empty((N, H), device=P.device, dtype=torch.float32)
    pre = torch.empty_like(h) if save_pre else None
    with _on(P.device):
        check(lib.lipvq_bin_hidden_f32(_ptr(bins), _ptr(P), _ptr(b1), _ptr(h), _ptr(pre), N, A, nb, H, _stream()),
              "lipvq_bin_hidden_f32")
    return (h, pre) if save_pre else h


def act_bwd(g, pre, act, *, dropout=None):
    """g * act'(pre), elementwise.  dropout=(snap, site, p) of a ``linear(..., dropout=...)``: (g * m) * act'(pre) over the 2-D
    [rows, cols] gradient, m regenerated -- the first backward step of that Linear; pre may then be None for ACT_NONE (g * m)."""
    g = _chk(g, "g")
    if dropout is not None and pre is None:
        if act != ACT_NONE:
            raise ValueError("act_bwd: pre is required unless act is ACT_NONE")
    else:
        pre = _chk(pre, "pre")
        if g.shape != pre.shape:
            raise ValueError("act_bwd: shapes differ")
    out = torch.empty_like(g)
    if dropout is None:
        with _on(g.device):
            check(lib.lipvq_act_bwd_f32(_ptr(g), _ptr(pre), _ptr(out), g.numel(), int(act), _stream()), "lipvq_act_bwd_f32")
        return out
    if g.dim() != 2:
        raise ValueError("act_bwd: g must be 2-D [rows, cols] (the dropout field)")
    snap, site, p = _dropout_args("act_bwd", dropout, g.device)
    with _on(g.device):
        check(lib.lipvq_act_bwd_drop_f32(_ptr(g), _ptr(pre), _ptr(out), _ptr(snap), site, p, g.shape[0], g.shape[1], int(act), _stream()),
              "lipvq_act_bwd_drop_f32")
    return out


def ema_update(cluster_size, embed_sum, counts, dw, codebook, decay, eps):
    """In-place EMA codebook update (opt-in extension; include/lipvq.h lipvq_ema_update_f32)."""
    K, D = codebook.shape
    for name, t, shape, dt in (("cluster_size", cluster_size, (K,), torch.float32), ("embed_sum", embed_sum, (K, D), torch.float32),
                               ("counts", counts, (K,), torch.int64), ("dw", dw, (K, D), torch.float32),
                               ("codebook", codebook, (K, D), torch.float32)):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"ema_update: {name} must be a contiguous CUDA {dt} tensor of shape {shape}")
    ws = torch.empty(1, device=codebook.device, dtype=torch.float64)
    with _on(codebook.device):
        check(lib.lipvq_ema_update_f32(_ptr(cluster_size), _ptr(embed_sum), _ptr(counts), _ptr(dw), _ptr(codebook),
                                       float(decay), float(eps), K, D, _ptr(ws), _stream()), "lipvq_ema_update_f32")


# ---- opt-in extension: k-means++ seeding, dead-code revival, Lloyd means (include/lipvq.h lipvq_kmeans_*) ----------------------

def _chk_inplace(t, name, dtype=torch.float32):
    """An output written through its pointer: a contiguous copy would swallow the write."""
    t2 = _chk(t, name, dtype)
    if t2 is not t:
        raise ValueError(f"{name}: must be contiguous (it is written in place)")
    return t


def _kmeans_args(z, K, draws, dist, what):
    z = _chk(z, "z")
    if z.dim() != 2 or z.shape[0] < 1 or z.shape[1] < 1:
        raise ValueError(f"{what}: z must be [N >= 1, D >= 1], got {tuple(z.shape)}")
    if int(K) < 1:
        raise ValueError(f"{what}: K must be >= 1, got {K}")
    draws = _chk(draws, "draws", torch.float64)
    if draws.dim() != 1 or draws.numel() < K:
        raise ValueError(f"{what}: draws must hold at least K = {K} values, got {tuple(draws.shape)}")
    if dist not in (DIST_NORM, DIST_SQSUM):
        raise ValueError(f"{what}: unknown distance rule {dist}")
    if draws.device != z.device:
        raise ValueError(f"{what}: draws must be on {z.device}")
    return z, draws


def kmeans_seed(z, K: int, draws, dist: int = DIST_NORM, out=None):
    """k-means++ seeding (D^2 sampling, include/lipvq.h lipvq_kmeans_seed_f32) of K codes from the rows of z [N, D]: code 0 is
    row floor(draws[0] N), code k the row drawn with draws[k] (fp64 in [0, 1)).  out: the [K, D] codebook written in place
    (codes the draws cannot reach stay as they were); a new zero-filled one when None.  Returns (codebook, picks [K] int64:
    the row copied into each code or -1, written [1] int64), all on the device: nothing is synchronised."""
    K = int(K)
    z, draws = _kmeans_args(z, K, draws, dist, "kmeans_seed")
    N, D = z.shape
    if out is None:
        out = torch.zeros((K, D), device=z.device, dtype=torch.float32)
    out = _chk_inplace(out, "out")
    if tuple(out.shape) != (K, D) or out.device != z.device:
        raise ValueError(f"kmeans_seed: out must be [{K}, {D}] on {z.device}")
    picks = torch.empty(K, device=z.device, dtype=torch.int64)
    written = torch.empty(1, device=z.device, dtype=torch.int64)
    ws = torch.empty(lib.lipvq_kmeans_workspace_bytes(N, K), device=z.device, dtype=torch.uint8)
    with _on(z.device):
        check(lib.lipvq_kmeans_seed_f32(_ptr(z), _ptr(out), _ptr(draws), _ptr(picks), _ptr(written), _ptr(ws), N, K, D, int(dist),
                                        _stream()), "lipvq_kmeans_seed_f32")
    return out, picks, written


def kmeans_revive_(codebook, z, idx, counts, threshold: int, draws, dist: int = DIST_NORM, max_codes: int | None = None):
    """Dead-code revival in place (include/lipvq.h lipvq_kmeans_revive_f32): the codes with counts[k] < threshold are refilled
    in ascending code order by D^2 sampling over the rows of z, starting from each row's distance to its assigned code idx[n];
    code k uses draws[k].  max_codes bounds how many dead codes are served (default K; each costs two launches whether it
    exists or not).  Returns (picks [K] int64: the row copied into each code or -1, written [1] int64), on the device."""
    codebook = _chk_inplace(codebook, "codebook")
    if codebook.dim() != 2:
        raise ValueError("kmeans_revive_: codebook must be [K, D]")
    K, D = codebook.shape
    z, draws = _kmeans_args(z, K, draws, dist, "kmeans_revive_")
    N = z.shape[0]
    idx, counts = _chk(idx, "idx", torch.int64), _chk(counts, "counts", torch.int64)
    if z.shape[1] != D or idx.numel() != N or counts.numel() != K:
        raise ValueError("kmeans_revive_: shapes do not match (z [N, D], idx [N], counts [K], codebook [K, D])")
    if codebook.device != z.device or idx.device != z.device or counts.device != z.device:
        raise ValueError("kmeans_revive_: every tensor must be on one device")
    max_codes = K if max_codes is None else min(int(max_codes), K)
    if max_codes < 0:
        raise ValueError("kmeans_revive_: max_codes must be >= 0")
    picks = torch.empty(K, device=z.device, dtype=torch.int64)
    written = torch.empty(1, device=z.device, dtype=torch.int64)
    ws = torch.empty(lib.lipvq_kmeans_workspace_bytes(N, K), device=z.device, dtype=torch.uint8)
    with _on(z.device):
        check(lib.lipvq_kmeans_revive_f32(_ptr(z), _ptr(codebook), _ptr(idx), _ptr(counts), int(threshold), _ptr(draws), _ptr(picks),
                                          _ptr(written), _ptr(ws), N, K, D, int(dist), max_codes, _stream()), "lipvq_kmeans_revive_f32")
    return picks, written


def kmeans_means_(codebook, sums, counts):
    """The Lloyd update in place: codebook[k] = sums[k] / (float)counts[k] where counts[k] > 0 (lipvq_kmeans_means_f32)."""
    codebook = _chk_inplace(codebook, "codebook")
    sums, counts = _chk(sums, "sums"), _chk(counts, "counts", torch.int64)
    if codebook.dim() != 2 or tuple(sums.shape) != tuple(codebook.shape) or counts.numel() != codebook.shape[0]:
        raise ValueError("kmeans_means_: codebook and sums must be [K, D], counts [K]")
    if sums.device != codebook.device or counts.device != codebook.device:
        raise ValueError("kmeans_means_: every tensor must be on one device")
    K, D = codebook.shape
    with _on(codebook.device):
        check(lib.lipvq_kmeans_means_f32(_ptr(codebook), _ptr(sums), _ptr(counts), K, D, _stream()), "lipvq_kmeans_means_f32")


# ---------------------------------------------------------------------------------------------------
# the default action branch (obs_nets.py:1244-1260; csrc/lipvq_xf.hip)
# ---------------------------------------------------------------------------------------------------

def spectral_norm(W, u, v, do_power_iteration: bool, eps: float = 1e-12):
    """(W / sigma, sigma [1]) of torch.nn.utils.spectral_norm; with do_power_iteration u and v are UPDATED IN PLACE."""
    W, u, v = _chk(W, "W"), _chk(u, "u"), _chk(v, "v")
    if W.dim() != 2 or u.shape != (W.shape[0],) or v.shape != (W.shape[1],):
        raise ValueError(f"spectral_norm: W {tuple(W.shape)}, u {tuple(u.shape)}, v {tuple(v.shape)}")
    Wsn = torch.empty_like(W)
    sigma = torch.empty(1, device=W.device, dtype=torch.float32)
    with _on(W.device):
        check(lib.lipvq_spectral_norm_f32(_ptr(W), _ptr(u), _ptr(v), _ptr(Wsn), _ptr(sigma), W.shape[0], W.shape[1],
                                          int(bool(do_power_iteration)), float(eps), _stream()), "lipvq_spectral_norm_f32")
    return Wsn, sigma


def spectral_norm_bwd(gWsn, Wsn, u, v, sigma):
    gWsn, Wsn = _chk(gWsn, "gWsn"), _chk(Wsn, "Wsn")
    gW = torch.empty_like(Wsn)
    with _on(Wsn.device):
        check(lib.lipvq_spectral_norm_bwd_f32(_ptr(gWsn), _ptr(Wsn), _ptr(_chk(u, "u")), _ptr(_chk(v, "v")), _ptr(_chk(sigma, "sigma")),
                                              _ptr(gW), Wsn.shape[0], Wsn.shape[1], _stream()), "lipvq_spectral_norm_bwd_f32")
    return gW


def _chk_keep(keep, H, S, dev):
    if keep is None:
        return None
    if keep.dtype != torch.uint8 or keep.shape != (H, S, S) or not keep.is_contiguous() or keep.device != dev:
        raise ValueError("attention: keep must be a contiguous uint8 [H, S, S] tensor on the input's device")
    return keep


def attention(qkv, nhead: int, keep=None, keep_prob: float = 1.0, *, dropout=None):
    """(out [S, D], lse [H, S]) of multi-head self-attention over the unbatched sequence qkv [S, 3D] (q | k | v).
    Attention-probability dropout: keep [H, S, S] bytes with keep_prob, or dropout=(snap, site, p), drawn in the kernel at field
    row = h S + q, col = key -- the bits of keep = ``dropout_keep(snap, site, H S, S, p)`` reshaped [H, S, S], keep_prob = 1 - p."""
    qkv = _chk(qkv, "qkv")
    if qkv.dim() != 2 or qkv.shape[1] % 3 != 0:
        raise ValueError(f"attention: qkv {tuple(qkv.shape)}")
    S, D = qkv.shape[0], qkv.shape[1] // 3
    if dropout is not None:
        snap, site, p = _dropout_args("attention", dropout, qkv.device, keep)
    keep = _chk_keep(keep, nhead, S, qkv.device)
    out = torch.empty((S, D), device=qkv.device, dtype=torch.float32)
    lse = torch.empty((nhead, S), device=qkv.device, dtype=torch.float32)
    with _on(qkv.device):
        if dropout is not None:
            check(lib.lipvq_attention_drop_f32(_ptr(qkv), _ptr(out), _ptr(lse), _ptr(snap), site, p, S, D, int(nhead), _stream()),
                  "lipvq_attention_drop_f32")
        else:
            check(lib.lipvq_attention_f32(_ptr(qkv), _ptr(out), _ptr(lse), _ptr(keep), float(keep_prob), S, D, int(nhead), _stream()),
                  "lipvq_attention_f32")
    return out, lse


def attention_bwd(qkv, out, gout, lse, nhead: int, keep=None, keep_prob: float = 1.0, *, dropout=None):
    """gqkv of ``attention``; dropout=(snap, site, p) of the forward: the decisions are regenerated inside the two kernels."""
    qkv, out, gout, lse = _chk(qkv, "qkv"), _chk(out, "out"), _chk(gout, "gout"), _chk(lse, "lse")
    S, D = out.shape
    if qkv.shape != (S, 3 * D) or gout.shape != out.shape or lse.shape != (nhead, S):
        raise ValueError("attention_bwd: shapes do not match")
    if dropout is not None:
        snap, site, p = _dropout_args("attention_bwd", dropout, qkv.device, keep)
    keep = _chk_keep(keep, nhead, S, qkv.device)
    gqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    with _on(qkv.device):
        if dropout is not None:
            check(lib.lipvq_attention_bwd_drop_f32(_ptr(qkv), _ptr(out), _ptr(gout), _ptr(lse), _ptr(gqkv), _ptr(delta), _ptr(snap), site,
                                                   p, S, D, int(nhead), _stream()), "lipvq_attention_bwd_drop_f32")
        else:
            check(lib.lipvq_attention_bwd_f32(_ptr(qkv), _ptr(out), _ptr(gout), _ptr(lse), _ptr(gqkv), _ptr(delta), _ptr(keep),
                                              float(keep_prob), S, D, int(nhead), _stream()), "lipvq_attention_bwd_f32")
    return gqkv


# ---------------------------------------------------------------------------------------------------
# the transformer backbone (csrc/lipvq_gpt.hip; reference robomimic/models/transformers.py:80-439)
# ---------------------------------------------------------------------------------------------------

def _gpt_keep(keep, B, H, L, dev):
    if keep is None:
        return None
    if keep.dtype != torch.uint8 or keep.shape != (B, H, L, L) or not keep.is_contiguous() or keep.device != dev:
        raise ValueError("gpt_attention: keep must be a contiguous uint8 [B, H, L, L] tensor on the input's device")
    return keep


def gpt_attention(qkv, nhead: int, causal: bool = True, keep=None, keep_prob: float = 1.0, *, dropout=None):
    """(out [B, L, E], lse [B, H, L]) of batched multi-head self-attention over qkv [B, L, 3E] (q | k | v), causal or not.
    Attention-probability dropout: keep [B, H, L, L] bytes with keep_prob, or dropout=(snap, site, p), drawn in the kernel."""
    qkv = _chk(qkv, "qkv")
    if qkv.dim() != 3 or qkv.shape[2] % 3 != 0:
        raise ValueError(f"gpt_attention: qkv {tuple(qkv.shape)}")
    B, L, E = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    if dropout is not None:
        snap, site, p = _dropout_args("gpt_attention", dropout, qkv.device, keep)
    keep = _gpt_keep(keep, B, nhead, L, qkv.device)
    out = torch.empty((B, L, E), device=qkv.device, dtype=torch.float32)
    lse = torch.empty((B, nhead, L), device=qkv.device, dtype=torch.float32)
    with _on(qkv.device):
        if dropout is not None:
            check(lib.lipvq_gpt_attention_drop_f32(_ptr(qkv), _ptr(out), _ptr(lse), _ptr(snap), site, p, B, L, E, int(nhead),
                                                   int(bool(causal)), _stream()), "lipvq_gpt_attention_drop_f32")
        else:
            check(lib.lipvq_gpt_attention_f32(_ptr(qkv), _ptr(out), _ptr(lse), _ptr(keep), float(keep_prob), B, L, E, int(nhead),
                                              int(bool(causal)), _stream()), "lipvq_gpt_attention_f32")
    return out, lse


def gpt_attention_prefix(prefix_qkv, qkv, nhead: int):
    """out [B, Lq, E] of causal attention from the Lq new tokens of qkv [B, Lq, 3E] to the P cached keys and values of
    prefix_qkv [Bp, P, 3E] (a prefill's qkv tensor; Bp == B, or 1 for one prompt shared by every sequence) plus their own:
    the bits of gpt_attention(cat([prefix_qkv, qkv], 1), nhead, True)[0][:, P:].  Forward only."""
    prefix_qkv, qkv = _chk(prefix_qkv, "prefix_qkv"), _chk(qkv, "qkv")
    if qkv.dim() != 3 or qkv.shape[2] % 3 != 0 or prefix_qkv.dim() != 3 or prefix_qkv.shape[2] != qkv.shape[2]:
        raise ValueError(f"gpt_attention_prefix: prefix_qkv {tuple(prefix_qkv.shape)}, qkv {tuple(qkv.shape)}")
    if prefix_qkv.device != qkv.device:
        raise ValueError("gpt_attention_prefix: prefix_qkv and qkv are on different devices")
    B, Lq, E = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    out = torch.empty((B, Lq, E), device=qkv.device, dtype=torch.float32)
    with _on(qkv.device):
        check(lib.lipvq_gpt_attention_prefix_f32(_ptr(prefix_qkv), _ptr(qkv), _ptr(out), B, prefix_qkv.shape[0], prefix_qkv.shape[1],
                                                 Lq, E, int(nhead), _stream()), "lipvq_gpt_attention_prefix_f32")
    return out


def gpt_attention_bwd(qkv, out, gout, lse, nhead: int, causal: bool = True, keep=None, keep_prob: float = 1.0, *, dropout=None):
    qkv, out, gout, lse = _chk(qkv, "qkv"), _chk(out, "out"), _chk(gout, "gout"), _chk(lse, "lse")
    B, L, E = out.shape
    if qkv.shape != (B, L, 3 * E) or gout.shape != out.shape or lse.shape != (B, nhead, L):
        raise ValueError("gpt_attention_bwd: shapes do not match")
    if dropout is not None:
        snap, site, p = _dropout_args("gpt_attention_bwd", dropout, qkv.device, keep)
    keep = _gpt_keep(keep, B, nhead, L, qkv.device)
    gqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    with _on(qkv.device):
        if dropout is not None:
            check(lib.lipvq_gpt_attention_bwd_drop_f32(_ptr(qkv), _ptr(out), _ptr(gout), _ptr(lse), _ptr(gqkv), _ptr(delta), _ptr(snap),
                                                       site, p, B, L, E, int(nhead), int(bool(causal)), _stream()),
                  "lipvq_gpt_attention_bwd_drop_f32")
        else:
            check(lib.lipvq_gpt_attention_bwd_f32(_ptr(qkv), _ptr(out), _ptr(gout), _ptr(lse), _ptr(gqkv), _ptr(delta), _ptr(keep),
                                                  float(keep_prob), B, L, E, int(nhead), int(bool(causal)), _stream()),
                  "lipvq_gpt_attention_bwd_f32")
    return gqkv


def gpt_layernorm(a, b, w, bias, eps: float, want_s: bool = True, save: bool = False, *, dropout=None):
    """s = a + b (b may be None) and y = LayerNorm(s) * w + bias over the last dimension, one launch.
    Returns (s or None, y) and, with save=True, (s or None, y, xhat, rstd).
    dropout=(snap, site, p): the branch's dropout inside the launch, s = a + b * m, m = 1 / (1 - p) where the in-kernel source
    keeps (row, e) and 0 where it drops it; b is then required."""
    a = _chk(a, "a")
    if b is not None or dropout is not None:
        b = _chk(b, "b")
        if b.shape != a.shape:
            raise ValueError("gpt_layernorm: shapes differ")
    if dropout is not None:
        snap, site, p = _dropout_args("gpt_layernorm", dropout, a.device)
    E = a.shape[-1]
    N = a.numel() // E if E else 0
    s = torch.empty_like(a) if want_s else None
    y = torch.empty_like(a)
    xhat = torch.empty_like(a) if save else None
    rstd = torch.empty(N, device=a.device, dtype=torch.float32) if save else None
    with _on(a.device):
        if dropout is not None:
            check(lib.lipvq_gpt_layernorm_drop_f32(_ptr(a), _ptr(b), _ptr(_chk(w, "w")), _ptr(_chk(bias, "bias")), float(eps), _ptr(snap),
                                                   site, p, _ptr(s), _ptr(y), _ptr(xhat), _ptr(rstd), N, E, _stream()),
                  "lipvq_gpt_layernorm_drop_f32")
        else:
            check(lib.lipvq_gpt_layernorm_f32(_ptr(a), _ptr(b), _ptr(_chk(w, "w")), _ptr(_chk(bias, "bias")), float(eps), _ptr(s), _ptr(y),
                                              _ptr(xhat), _ptr(rstd), N, E, _stream()), "lipvq_gpt_layernorm_f32")
    return (s, y, xhat, rstd) if save else (s, y)


def gpt_layernorm_bwd(gy, xhat, rstd, w, gres=None, *, dropout=None):
    """(gs, gw, gb): gs = LayerNorm backward + gres (the residual stream's incoming gradient, may be None).
    dropout=(snap, site, p) of the forward: (gs, gbranch, gw, gb), gbranch = gs * m the gradient of the dropped branch b, from
    the decisions the source regenerates."""
    gy, xhat = _chk(gy, "gy"), _chk(xhat, "xhat")
    if gres is not None:
        gres = _chk(gres, "gres")
        if gres.shape != gy.shape:
            raise ValueError("gpt_layernorm_bwd: gres shape")
    if dropout is not None:
        snap, site, p = _dropout_args("gpt_layernorm_bwd", dropout, gy.device)
    E = gy.shape[-1]
    N = gy.numel() // E if E else 0
    gs = torch.empty_like(gy)
    gw = torch.empty(E, device=gy.device, dtype=torch.float32)
    gb = torch.empty(E, device=gy.device, dtype=torch.float32)
    ws = torch.empty(max(1, lib.lipvq_gpt_layernorm_bwd_workspace_bytes(N, E)), device=gy.device, dtype=torch.uint8)
    if dropout is not None:
        gbr = torch.empty_like(gy)
        with _on(gy.device):
            check(lib.lipvq_gpt_layernorm_bwd_drop_f32(_ptr(gy), _ptr(xhat), _ptr(_chk(rstd, "rstd")), _ptr(_chk(w, "w")), _ptr(gres),
                                                       _ptr(snap), site, p, _ptr(gs), _ptr(gbr), _ptr(gw), _ptr(gb), _ptr(ws), N, E,
                                                       _stream()), "lipvq_gpt_layernorm_bwd_drop_f32")
        return gs, gbr, gw, gb
    with _on(gy.device):
        check(lib.lipvq_gpt_layernorm_bwd_f32(_ptr(gy), _ptr(xhat), _ptr(_chk(rstd, "rstd")), _ptr(_chk(w, "w")), _ptr(gres), _ptr(gs),
                                              _ptr(gw), _ptr(gb), _ptr(ws), N, E, _stream()), "lipvq_gpt_layernorm_bwd_f32")
    return gs, gw, gb


# ---------------------------------------------------------------------------------------------------
# the policy's GMM output head (csrc/lipvq_gmm.hip)
# ---------------------------------------------------------------------------------------------------

GMM_SOFTPLUS, GMM_EXP, GMM_LOW_NOISE = 0, 1, 2


def _gmm_rows(feats, what="the GMM head"):
    """feats [B, T, E] (or [N, E]) -> (tensor, N, T, E, bstride): the tensor's own strides where the kernel can read them -- rows
    of E contiguous floats, T consecutive rows per batch entry, a batch stride that is a multiple of 4 floats, as for the view
    out[:, -T:] of a backbone output -- and a contiguous copy otherwise."""
    if not isinstance(feats, torch.Tensor):
        raise TypeError(f"feats: expected a tensor, got {type(feats).__name__}")
    if not feats.is_cuda:
        raise RuntimeError(f"feats: {what} runs on the HIP library only (got a {feats.device} tensor)")
    if feats.dtype != torch.float32:
        raise TypeError(f"feats: expected torch.float32, got {feats.dtype}")
    if feats.dim() == 2:
        feats = feats.unsqueeze(0)
    if feats.dim() != 3:
        raise ValueError(f"feats: expected [B, T, E], got {tuple(feats.shape)}")
    B, T, E = feats.shape
    if B * T == 0:
        return feats, 0, max(T, 1), E, 0
    ok = feats.stride(2) == 1 and (T == 1 or feats.stride(1) == E) and (B == 1 or feats.stride(0) % 4 == 0) and feats.data_ptr() % 16 == 0
    if not ok:
        feats = feats.contiguous()
    return feats, B * T, T, E, (feats.stride(0) if B > 1 else T * E)


MATMUL_PRECISIONS = {"fp32": 0, "bf16": 1, "bf16x3": 2}              # include/lipvq.h: LIPVQ_MATMUL_*


def _matmul_mode(what, precision, E=None):
    """The LIPVQ_MATMUL_* value of a precision name; ValueError for an unknown name, or a bf16 mode with E % 8 != 0."""
    if precision not in MATMUL_PRECISIONS:
        raise ValueError(f"{what}: matmul precision must be 'fp32', 'bf16' or 'bf16x3', got {precision!r}")
    if precision != "fp32" and E is not None and E % 8:
        raise ValueError(f"{what}: the {precision} mode needs the input width to be a multiple of 8 (got {E})")
    return MATMUL_PRECISIONS[precision]


def head_linear_grads(need_x, need_params, feats, gpre, weights, precision="fp32"):
    """The Linear gradients of an output head from gpre [N, P], the gradient of its pre-activations: (gx in feats' shape, gW [P, E],
    gb [P]) -- one Linear for gx = gpre . W over the stacked `weights` (a tuple of [P_i, E] matrices, P = sum P_i), one wgrad over
    all P columns; the caller cuts gW / gb by rows.  What is not needed is None.
    precision "bf16" / "bf16x3": the two products run on linear_nn_<mode> (the stacked weights as stored, no transposed copy)
    and wgrad_<mode>.  Those need widths that are multiples of 8: gpre's columns and the stacked weight's rows are extended with
    zeros to P8 = 8 ceil(P / 8) and the results cut -- zero lines add exact zeros.  Cost: one pad of gpre (skipped when P % 8 == 0;
    a fill and a copy of [N, P8]) and, for gx, one cat that writes the [P8, E] stack with its zero rows (it replaces the fp32
    path's cat + transposed copy)."""
    mode = _matmul_mode("head_linear_grads", precision, feats.shape[-1])
    gx = gW = gb = None
    if mode:
        P, E = gpre.shape[1], feats.shape[-1]
        P8 = (P + 7) // 8 * 8
        nn_fn, wg_fn = (linear_nn_bf16, wgrad_bf16) if precision == "bf16" else (linear_nn_bf16x3, wgrad_bf16x3)
        if not (need_x or need_params):
            return gx, gW, gb
        g8 = gpre if P8 == P else torch.nn.functional.pad(gpre, (0, P8 - P))
        if need_x:
            rows = tuple(weights) + ((torch.zeros((P8 - P, E), device=gpre.device, dtype=torch.float32),) if P8 != P else ())
            gx = nn_fn(g8, torch.cat(rows, 0) if len(rows) > 1 else rows[0]).view(feats.shape)
        if need_params:
            gW, gb = wg_fn(g8, feats.reshape(-1, E))
            gW, gb = gW[:P], gb[:P]
        return gx, gW, gb
    if need_x:
        Wt = torch.cat(tuple(weights), 0).t().contiguous()         # [E, P] -> gx = gpre . W
        gx = linear(gpre, Wt).view(feats.shape)
    if need_params:
        gW, gb = wgrad(gpre, feats.reshape(-1, feats.shape[-1]))
    return gx, gW, gb


def _gmm_params(params, M, A, E):
    Wm, bm, Ws, bs, Wl, bl = (_chk(p, "gmm parameter") for p in params)
    if Wm.shape != (M * A, E) or Ws.shape != (M * A, E) or Wl.shape != (M, E) or bm.shape != (M * A,) or bs.shape != (M * A,) or bl.shape != (M,):
        raise ValueError(f"gmm head: parameter shapes do not match M={M} A={A} E={E}")
    return Wm, bm, Ws, bs, Wl, bl


def gmm_head(feats, params, M: int, A: int, actions=None, scale_mode: int = GMM_SOFTPLUS, min_std: float = 0.01,
             want_pre: bool = False, want_params: bool = False, want_sum: bool = False, precision: str = "fp32"):
    """The GMM head in one launch (lipvq_gmm_head_f32; precision "bf16" / "bf16x3": lipvq_gmm_head_mp_f32, the product on the bf16
    matrix pipe with the bits of linear_bf16 / linear_bf16x3, the epilogue unchanged).  feats [B, T, E] (its strides are passed on, see _gmm_rows); params =
    (mean.weight, mean.bias, scale.weight, scale.bias, logits.weight, logits.bias); actions [B, T, A] or None.
    Returns a dict with the outputs asked for: log_prob [N] (with actions), pre [N, P] (want_pre), mean / scale [N, M, A] and
    logits [N, M] (want_params), sum [] (want_sum: the deterministic sum of log_prob)."""
    feats, N, T, E, bstride = _gmm_rows(feats)
    Wm, bm, Ws, bs, Wl, bl = _gmm_params(params, M, A, E)
    mode = _matmul_mode("gmm_head", precision, E)
    dev = feats.device
    P = M * (2 * A + 1)
    out = {}
    if actions is not None:
        actions = _chk(actions, "actions")
        if actions.numel() != N * A:
            raise ValueError(f"gmm_head: actions {tuple(actions.shape)} do not match {N} rows of {A}")
        out["log_prob"] = torch.empty(N, device=dev, dtype=torch.float32)
    elif want_sum:
        raise ValueError("gmm_head: the sum of log_prob needs actions")
    if want_pre:
        out["pre"] = torch.empty((N, P), device=dev, dtype=torch.float32)
    if want_params:
        out["mean"] = torch.empty((N, M, A), device=dev, dtype=torch.float32)
        out["scale"] = torch.empty((N, M, A), device=dev, dtype=torch.float32)
        out["logits"] = torch.empty((N, M), device=dev, dtype=torch.float32)
    ws = None
    if want_sum:
        out["sum"] = torch.empty((), device=dev, dtype=torch.float32)
        ws = torch.empty(max(1, lib.lipvq_gmm_workspace_bytes(N)), device=dev, dtype=torch.uint8)
    args = (_ptr(feats), bstride, _ptr(Wm), _ptr(bm), _ptr(Ws), _ptr(bs), _ptr(Wl), _ptr(bl), _ptr(actions), _ptr(out.get("log_prob")),
            _ptr(out.get("pre")), _ptr(out.get("mean")), _ptr(out.get("scale")), _ptr(out.get("logits")), _ptr(out.get("sum")), _ptr(ws),
            N, T, E, int(M), int(A), int(scale_mode), float(min_std))
    with _on(dev):
        if mode:
            check(lib.lipvq_gmm_head_mp_f32(*args, mode, _stream()), "lipvq_gmm_head_mp_f32")
        else:
            check(lib.lipvq_gmm_head_f32(*args, _stream()), "lipvq_gmm_head_f32")
    return out


def gmm_head_bwd(pre, actions, g, gsum, M: int, A: int, scale_mode: int = GMM_SOFTPLUS, min_std: float = 0.01):
    """gpre [N, P] (lipvq_gmm_head_bwd_f32): g [N] = gradient of log_prob, gsum [] = gradient of the sum; either may be None."""
    pre, actions = _chk(pre, "pre"), _chk(actions, "actions")
    N, P = pre.shape
    if P != M * (2 * A + 1) or actions.numel() != N * A:
        raise ValueError("gmm_head_bwd: shapes do not match")
    if g is None and gsum is None:
        raise ValueError("gmm_head_bwd: no upstream gradient")
    if g is not None:
        g = _chk(g, "g")
        if g.numel() != N:
            raise ValueError("gmm_head_bwd: g must have one entry per row")
    if gsum is not None:
        gsum = _chk(gsum, "gsum")
    gpre = torch.empty_like(pre)
    with _on(pre.device):
        check(lib.lipvq_gmm_head_bwd_f32(_ptr(pre), _ptr(actions), _ptr(g), _ptr(gsum), _ptr(gpre), N, int(M), int(A), int(scale_mode),
                                         float(min_std), _stream()), "lipvq_gmm_head_bwd_f32")
    return gpre


def gmm_params_bwd(pre, gmean, gscale, glogits, M: int, A: int, scale_mode: int = GMM_SOFTPLUS):
    """gpre [N, P] from the gradients of the head's mean / scale / logits outputs (lipvq_gmm_params_bwd_f32); None = zeros."""
    pre = _chk(pre, "pre")
    N, P = pre.shape
    if P != M * (2 * A + 1):
        raise ValueError("gmm_params_bwd: shapes do not match")
    gmean, gscale, glogits = (None if t is None else _chk(t, "gradient") for t in (gmean, gscale, glogits))
    for t, n in ((gmean, N * M * A), (gscale, N * M * A), (glogits, N * M)):
        if t is not None and t.numel() != n:
            raise ValueError("gmm_params_bwd: gradient shape")
    gpre = torch.empty_like(pre)
    with _on(pre.device):
        check(lib.lipvq_gmm_params_bwd_f32(_ptr(pre), _ptr(gmean), _ptr(gscale), _ptr(glogits), _ptr(gpre), N, int(M), int(A),
                                           int(scale_mode), _stream()), "lipvq_gmm_params_bwd_f32")
    return gpre


def gmm_sample(feats, params, M: int, A: int, u, eps, scale_mode: int = GMM_SOFTPLUS, min_std: float = 0.01, precision: str = "fp32"):
    """action [N, A] = mu_m + sigma_m eps with m drawn by inverse CDF from u (lipvq_gmm_sample_f32), one launch.  precision: as
    for gmm_head (lipvq_gmm_sample_mp_f32)."""
    feats, N, T, E, bstride = _gmm_rows(feats)
    Wm, bm, Ws, bs, Wl, bl = _gmm_params(params, M, A, E)
    mode = _matmul_mode("gmm_sample", precision, E)
    u, eps = _chk(u, "u"), _chk(eps, "eps")
    if u.numel() != N or eps.numel() != N * A:
        raise ValueError(f"gmm_sample: u {tuple(u.shape)} / eps {tuple(eps.shape)} do not match {N} rows of {A}")
    action = torch.empty((N, A), device=feats.device, dtype=torch.float32)
    args = (_ptr(feats), bstride, _ptr(Wm), _ptr(bm), _ptr(Ws), _ptr(bs), _ptr(Wl), _ptr(bl), _ptr(u), _ptr(eps), _ptr(action), N, T, E,
            int(M), int(A), int(scale_mode), float(min_std))
    with _on(feats.device):
        if mode:
            check(lib.lipvq_gmm_sample_mp_f32(*args, mode, _stream()), "lipvq_gmm_sample_mp_f32")
        else:
            check(lib.lipvq_gmm_sample_f32(*args, _stream()), "lipvq_gmm_sample_f32")
    return action


# the site word of the GMM head's in-kernel sampling noise (include/lipvq.h, "in-kernel sampling"): the uniform field; the normal
# field is SAMPLE_SITE_GMM + 1
SAMPLE_SITE_GMM = 0xC0000000


def _sample_snap(what, snap, dev=None):
    if not isinstance(snap, torch.Tensor) or snap.dtype != torch.int64 or snap.numel() != 2 or not snap.is_cuda or not snap.is_contiguous() \
            or (dev is not None and snap.device != dev):
        raise ValueError(f"{what}: snap must be the contiguous int64[2] tensor of dropout_begin on the input's device")
    return snap


def _sample_streams(what, streams, B, dev):
    """streams: None (stream b = batch position b) or one int64 id per batch entry, on `dev` (a torch.device, or None: the host)."""
    if streams is None:
        return None
    if not isinstance(streams, torch.Tensor) or streams.dtype != torch.int64 or tuple(streams.shape) != (B,):
        raise ValueError(f"{what}: streams must be an int64 [{B}] tensor (one stream id per batch entry)")
    if (streams.device != dev) if dev is not None else streams.is_cuda:
        raise ValueError(f"{what}: streams must be on " + ("the host" if dev is None else f"the device of the call ({dev})"))
    return streams.contiguous()


def gmm_sample_draw(feats, params, M: int, A: int, snap, streams=None, scale_mode: int = GMM_SOFTPLUS, min_std: float = 0.01,
                    precision: str = "fp32"):
    """gmm_sample whose u and eps are drawn inside the launch (lipvq_gmm_sample_draw_f32) from snap, the (seed, step) a
    dropout_begin on the sampling state wrote, and the rows' stream ids (streams int64 [B] on the device, None = batch position):
    the bits of gmm_sample(feats, ..., *gmm_noise(snap, B, T, A, streams)) at the same precision (lipvq_gmm_sample_draw_mp_f32).
    One launch, no noise tensor."""
    B = feats.shape[0] if isinstance(feats, torch.Tensor) and feats.dim() == 3 else 1
    feats, N, T, E, bstride = _gmm_rows(feats)
    Wm, bm, Ws, bs, Wl, bl = _gmm_params(params, M, A, E)
    mode = _matmul_mode("gmm_sample_draw", precision, E)
    snap = _sample_snap("gmm_sample_draw", snap, feats.device)
    streams = _sample_streams("gmm_sample_draw", streams, B, feats.device)
    action = torch.empty((N, A), device=feats.device, dtype=torch.float32)
    args = (_ptr(feats), bstride, _ptr(Wm), _ptr(bm), _ptr(Ws), _ptr(bs), _ptr(Wl), _ptr(bl), _ptr(snap), _ptr(streams), _ptr(action),
            N, T, E, int(M), int(A), int(scale_mode), float(min_std))
    with _on(feats.device):
        if mode:
            check(lib.lipvq_gmm_sample_draw_mp_f32(*args, mode, _stream()), "lipvq_gmm_sample_draw_mp_f32")
        else:
            check(lib.lipvq_gmm_sample_draw_f32(*args, _stream()), "lipvq_gmm_sample_draw_f32")
    return action


def gmm_noise(snap, B: int, T: int, A: int, streams=None):
    """(u [B, T], eps [B, T, A]) device tensors: the noise gmm_sample_draw forms from snap (and streams) for a [B, T] call."""
    snap = _sample_snap("gmm_noise", snap)
    B, T, A = int(B), int(T), int(A)
    if B < 0 or T <= 0:
        raise ValueError(f"gmm_noise: B={B} T={T}")
    streams = _sample_streams("gmm_noise", streams, B, snap.device)
    ok = 1 <= A <= 64                                                              # (anything else the library refuses before it writes)
    u = torch.empty((B, T) if ok else (0, T), device=snap.device, dtype=torch.float32)
    eps = torch.empty((B, T, A) if ok else (0, T, 0), device=snap.device, dtype=torch.float32)
    with _on(snap.device):
        check(lib.lipvq_gmm_noise_f32(_ptr(snap), _ptr(streams), _ptr(u), _ptr(eps), B, T, A, _stream()), "lipvq_gmm_noise_f32")
    return u, eps


def gmm_noise_host(seed: int, step: int, B: int, T: int, A: int, streams=None):
    """The same (u, eps) as CPU tensors from (seed, step), computed on the host (streams: a CPU int64 [B] tensor): no GPU call."""
    B, T, A = int(B), int(T), int(A)
    if B < 0 or T <= 0:
        raise ValueError(f"gmm_noise_host: B={B} T={T}")
    streams = _sample_streams("gmm_noise_host", streams, B, None)
    ok = 1 <= A <= 64
    u = torch.empty((B, T) if ok else (0, T), dtype=torch.float32)
    eps = torch.empty((B, T, A) if ok else (0, T, 0), dtype=torch.float32)
    check(lib.lipvq_gmm_noise_host(int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), None if streams is None else streams.data_ptr(),
                                   B, T, A, u.data_ptr(), eps.data_ptr()), "lipvq_gmm_noise_host")
    return u, eps


def normal_icdf_host(words):
    """eps [n] (CPU float32) for raw 32-bit draw words (a CPU tensor or array of integers below 2^32): v = (2 (w >> 9) + 1) 2^-24,
    then the library's inverse normal CDF, on the host."""
    import numpy as np
    w = np.ascontiguousarray(np.asarray(words).astype(np.uint32, copy=False).reshape(-1))
    out = torch.empty(w.size, dtype=torch.float32)
    check(lib.lipvq_normal_icdf_host(w.ctypes.data, out.data_ptr(), int(w.size)), "lipvq_normal_icdf_host")
    return out


# ---------------------------------------------------------------------------------------------------
# the deterministic policy's output head (csrc/lipvq_action_head.hip)
# ---------------------------------------------------------------------------------------------------

def action_head(feats, W, b, target=None, weights=(1.0, 0.0, 0.0), want_actions: bool = True, want_pre: bool = False,
                precision: str = "fp32"):
    """The Linear + tanh head and its losses (lipvq_action_head_f32; precision "bf16" / "bf16x3": lipvq_action_head_mp_f32, the
    product on the bf16 matrix pipe with the bits of linear_bf16 / linear_bf16x3, the epilogue unchanged).  feats [B, T, E] (its strides are passed on, see _gmm_rows);
    W [A, E], b [A]; target [B, T, A] or None; weights = (l2_weight, l1_weight, cos_weight).
    Returns a dict with the outputs asked for: actions [N, A] (want_actions), pre [N, A] (want_pre), losses [4] = (l2, l1, cos,
    action) (with a target: one more one-workgroup launch, a deterministic sum)."""
    feats, N, T, E, bstride = _gmm_rows(feats, "the action head")
    W, b = _chk(W, "W"), _chk(b, "b")
    if W.dim() != 2 or W.shape[1] != E or b.shape != (W.shape[0],):
        raise ValueError(f"action_head: W {tuple(W.shape)} / b {tuple(b.shape)} do not match E={E}")
    A = W.shape[0]
    mode = _matmul_mode("action_head", precision, E)
    dev = feats.device
    out = {}
    if want_actions:
        out["actions"] = torch.empty((N, A), device=dev, dtype=torch.float32)
    if want_pre:
        out["pre"] = torch.empty((N, A), device=dev, dtype=torch.float32)
    ws = None
    if target is not None:
        target = _chk(target, "target")
        if target.numel() != N * A:
            raise ValueError(f"action_head: target {tuple(target.shape)} does not match {N} rows of {A}")
        out["losses"] = torch.empty(4, device=dev, dtype=torch.float32)
        ws = torch.empty(max(1, lib.lipvq_action_head_workspace_bytes(N)), device=dev, dtype=torch.uint8)
    w2, w1, wc = (float(w) for w in weights)
    args = (_ptr(feats), bstride, _ptr(W), _ptr(b), _ptr(target), _ptr(out.get("actions")), _ptr(out.get("pre")), _ptr(out.get("losses")),
            _ptr(ws), N, T, E, int(A), w2, w1, wc)
    with _on(dev):
        if mode:
            check(lib.lipvq_action_head_mp_f32(*args, mode, _stream()), "lipvq_action_head_mp_f32")
        else:
            check(lib.lipvq_action_head_f32(*args, _stream()), "lipvq_action_head_f32")
    return out


def action_head_bwd(pre, target=None, g=None, gy=None, weights=(1.0, 0.0, 0.0)):
    """gpre [N, A] (lipvq_action_head_bwd_f32): g [4] = the gradient of (l2, l1, cos, action) -- a device tensor, with target
    [N, A] --, gy [N, A] = a gradient arriving at the actions output; either may be None."""
    pre = _chk(pre, "pre")
    N, A = pre.shape
    if g is None and gy is None:
        raise ValueError("action_head_bwd: no upstream gradient")
    if g is not None:
        g = _chk(g, "g")
        if g.numel() != 4:
            raise ValueError("action_head_bwd: g must have the four losses' gradients")
        if target is None:
            raise ValueError("action_head_bwd: the losses' gradient needs the target")
        target = _chk(target, "target")
        if target.numel() != N * A:
            raise ValueError("action_head_bwd: shapes do not match")
    else:
        target = None
    if gy is not None:
        gy = _chk(gy, "gy")
        if gy.numel() != N * A:
            raise ValueError("action_head_bwd: gy shape")
    gpre = torch.empty_like(pre)
    w2, w1, wc = (float(w) for w in weights)
    with _on(pre.device):
        check(lib.lipvq_action_head_bwd_f32(_ptr(pre), _ptr(target), _ptr(g), _ptr(gy), _ptr(gpre), N, int(A), w2, w1, wc, _stream()),
              "lipvq_action_head_bwd_f32")
    return gpre
