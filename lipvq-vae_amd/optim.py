"""The optimizers of the reference on the HIP library, and the step that closes the policy's training iteration.

``AdamW`` has the reference's constructor (``robomimic/algo/icl.py:885-889``:
``optim.AdamW(self.vq_vae_model.parameters(), lr=1e-3, weight_decay=1e-4)``); its ``step()`` is two HIP launches for the whole
parameter list (``lipvq_adamw_f32``) instead of torch's eight to ten foreach launches -- at the ICRT step shape the optimizer
was ~80 us of a 550 us step.  It subclasses ``torch.optim.AdamW`` and keeps torch's state layout (``step`` as a float32
device scalar per parameter -- the capturable layout --, ``exp_avg``, ``exp_avg_sq``), so ``state_dict()`` / ``load_state_dict()``
interchange with a stock ``AdamW(capturable=True)`` and the step can be captured in a HIP graph.  amsgrad / maximize are refused;
parameters that are not fp32 CUDA tensors fall back to nothing -- they raise.

``Adam`` is the policy's optimizer (``icl_config.py:27``, ``torch_utils.py:108-113``: ``optim.Adam`` with L2 regularisation, not
AdamW) in the same form (``lipvq_adam_f32``).  Both take

* ``lr`` as a float or as a 0-dim fp32 CUDA tensor.  A tensor is read by the kernel: a scheduler (``LambdaLR`` updates a tensor
  ``lr`` with ``fill_``, in place) keeps working when the step is replayed from a HIP graph; a float is frozen at capture.
* ``max_grad_norm`` (keyword only; also an attribute that may be changed between steps): ``step()`` then first runs the sum of
  squares over ALL groups' gradients, then the clip coefficient, then the Adam launches, which read each gradient as
  ``g * (float)clip_coef`` -- ``torch.nn.utils.clip_grad_norm_`` folded into the update, without a host synchronisation.
  ``p.grad`` itself keeps the unclipped gradient.  ``optimizer.grad_stats`` is the device record of the last such step:
  ``[total_norm, clip_coef, sumsq, sumsq_clipped]`` (float64).  ``math.inf`` only reports.

``clip_grad_norm_`` is the stand-alone in-place form for users who keep another optimizer, and ``backprop_for_loss`` the
reference's function (``robomimic/utils/torch_utils.py:196-234``) with one host synchronisation instead of one per parameter."""
from __future__ import annotations

import ctypes as C
import math

import torch

from ._capi import check, lib
from .derived import mark_written
from .ops import _on, _stream

_MAX = 32


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _numels(tensors):
    return (C.c_int64 * len(tensors))(*[t.numel() for t in tensors])


def _check_max_norm(max_norm):
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError(f"max_grad_norm must be >= 0 (math.inf reports the norm without clipping), got {max_norm}")
    return max_norm


class _GradNorm:
    """Workspace and ``stats`` record of the gradient-norm launches on one device; both are allocated once and keep their
    addresses (a captured graph refers to them)."""

    def __init__(self):
        self.device, self.ws, self.capacity, self.stats = None, None, 0, None

    def run(self, grads, max_norm):
        """stats = [total_norm, clip_coef, sumsq, sumsq_clipped] of the fp32 CUDA gradient list; nothing is scaled."""
        if not grads:
            raise RuntimeError("gradient norm: no parameter has a gradient")
        dev = grads[0].device
        for g in grads:
            if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.numel() > 0):
                raise RuntimeError("gradient norm: gradients must be non-empty contiguous fp32 CUDA tensors")
            if g.device != dev:
                raise RuntimeError("gradient norm: the gradients of one clipped step must live on one device")
        n = len(grads)
        if self.device != dev or self.capacity < n:
            self.ws = torch.empty(lib.lipvq_grad_sumsq_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
            self.capacity = n
            if self.device != dev:
                self.stats = torch.zeros(4, dtype=torch.float64, device=dev)
            self.device = dev
        with _on(dev):
            st = _stream()
            for s in range(0, n, _MAX):
                chunk = grads[s:s + _MAX]
                check(lib.lipvq_grad_sumsq_f32(_ptrs(chunk), _numels(chunk), len(chunk), s, self.capacity, self.ws.data_ptr(), st),
                      "lipvq_grad_sumsq_f32")
            check(lib.lipvq_clip_coef_f64(self.ws.data_ptr(), n, max_norm, self.stats.data_ptr(), st), "lipvq_clip_coef_f64")
        return self.stats


def clip_grad_norm_(parameters, max_norm):
    """``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` (2-norm, ``error_if_nonfinite=False``) in place on the HIP library:
    sum of squares in double, coefficient, ``g *= (float)clip_coef`` -- no host synchronisation.  Returns the float64 device
    record ``[total_norm, clip_coef, sumsq, sumsq_clipped]`` (a new tensor per call); parameters without a gradient are skipped."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    max_norm = _check_max_norm(max_norm)
    stats = _GradNorm().run(grads, max_norm)
    with _on(grads[0].device):
        for s in range(0, len(grads), _MAX):
            chunk = grads[s:s + _MAX]
            check(lib.lipvq_grad_scale_f32(_ptrs(chunk), _numels(chunk), len(chunk), stats.data_ptr(), _stream()),
                  "lipvq_grad_scale_f32")
    mark_written(grads)                  # lipvq_grad_scale_f32 scaled them through their raw pointers
    return stats


class _FusedStep:
    """step() of Adam and AdamW below; ``_decoupled`` tells them apart."""

    _decoupled = True

    def _init_fused(self, amsgrad, maximize, max_grad_norm):
        name = type(self).__name__
        if amsgrad or maximize:
            raise ValueError(f"lipvq_vae_amd.optim.{name} implements the plain {name} the reference uses (amsgrad=False, maximize=False)")
        self.max_grad_norm = None if max_grad_norm is None else _check_max_norm(max_grad_norm)
        self.grad_stats = None
        self._ws = {}
        self._norm = _GradNorm()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = type(self).__name__
        todo = []
        for group in self.param_groups:
            mine = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()
                        and p.grad.dtype == torch.float32):
                    raise RuntimeError(f"lipvq {name}: parameters and gradients must be contiguous fp32 CUDA tensors")
                st = self.state[p]
                if len(st) == 0:                               # torch's lazy state, capturable layout
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif not (torch.is_tensor(st["step"]) and st["step"].is_cuda):      # state loaded from an eager optimizer
                    st["step"] = torch.as_tensor(float(st["step"]), dtype=torch.float32, device=p.device)
                mine.append((p, p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"]))
            todo.append(mine)
        stats = None
        if self.max_grad_norm is not None and any(todo):
            # one norm over ALL groups' gradients, as clip_grad_norm_(net.parameters()) takes it
            stats = self.grad_stats = self._norm.run([t[1] for mine in todo for t in mine], _check_max_norm(self.max_grad_norm))
        for group, mine in zip(self.param_groups, todo):
            b1, b2 = group["betas"]
            lr = group["lr"]
            lr_dev = None
            if torch.is_tensor(lr):
                if not (lr.is_cuda and lr.dtype == torch.float32 and lr.numel() == 1):
                    raise RuntimeError(f"lipvq {name}: a tensor lr must be a 0-dim fp32 CUDA tensor")
                lr_dev = lr
            # AdamW called as before this module had Adam (float lr, no clipping) makes the library calls it always made
            legacy = self._decoupled and stats is None and lr_dev is None
            for s in range(0, len(mine), _MAX):
                chunk = mine[s:s + _MAX]
                dev = chunk[0][0].device
                if lr_dev is not None and lr_dev.device != dev:
                    raise RuntimeError(f"lipvq {name}: the lr tensor and the parameters must live on one device")
                ws = self._ws.get(dev)
                if ws is None:
                    ws = self._ws[dev] = torch.empty(lib.lipvq_adamw_workspace_bytes() // 4, dtype=torch.float32, device=dev)
                n = len(chunk)
                arr = lambda k: (C.c_void_p * n)(*[t[k].data_ptr() for t in chunk])
                numels = (C.c_int64 * n)(*[t[0].numel() for t in chunk])
                with _on(dev):
                    if legacy:
                        check(lib.lipvq_adamw_f32(arr(0), arr(1), arr(2), arr(3), arr(4), numels, n, float(lr), float(b1),
                                                  float(b2), float(group["eps"]), float(group["weight_decay"]), ws.data_ptr(),
                                                  _stream()), "lipvq_adamw_f32")
                    else:
                        check(lib.lipvq_adam_f32(arr(0), arr(1), arr(2), arr(3), arr(4), numels, n,
                                                 0.0 if lr_dev is not None else float(lr), float(b1), float(b2), float(group["eps"]),
                                                 float(group["weight_decay"]), int(self._decoupled),
                                                 None if lr_dev is None else lr_dev.data_ptr(),
                                                 None if stats is None else stats.data_ptr(), ws.data_ptr(), _stream()),
                              "lipvq_adam_f32")
                # the kernel wrote the parameters behind autograd's back: bump their version counters, as an in-place torch op
                # would (the tokenizer's packed-weight / prepared-codebook caches and autograd's saved-tensor checks key on them)
                mark_written(t[0] for t in chunk)
        return loss


class AdamW(_FusedStep, torch.optim.AdamW):
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 max_grad_norm=None):
        self._init_fused(amsgrad, maximize, max_grad_norm)
        torch.optim.AdamW.__init__(self, params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=True)


class Adam(_FusedStep, torch.optim.Adam):
    """``torch.optim.Adam`` (``weight_decay`` is L2 regularisation: ``g + weight_decay * p`` enters the moments)."""
    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 max_grad_norm=None):
        self._init_fused(amsgrad, maximize, max_grad_norm)
        torch.optim.Adam.__init__(self, params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=True)


def backprop_for_loss(net, optim, loss, max_grad_norm=None, retain_graph=False, sync=True):
    """``TorchUtils.backprop_for_loss`` (robomimic/utils/torch_utils.py:196-234): zero_grad, backward, clip, the sum of the
    clipped gradients' squared norms, ``optim.step()``.  With one of this module's optimizers the clip rides inside ``step()``
    (``p.grad`` keeps the unclipped gradient); with any other, ``clip_grad_norm_`` above scales the gradients in place first.
    Returns the reference's ``grad_norms`` = ``stats[3]``: as a float (ONE host synchronisation, where the reference makes one
    per parameter), or with ``sync=False`` as the float64 device scalar (none).  With ``max_grad_norm=None`` nothing is clipped
    and the norm is still reported, as in the reference."""
    optim.zero_grad()
    loss.backward(retain_graph=retain_graph)
    max_norm = math.inf if max_grad_norm is None else _check_max_norm(max_grad_norm)
    if isinstance(optim, _FusedStep):
        own = optim.max_grad_norm
        optim.max_grad_norm = max_norm
        try:
            optim.step()
        finally:
            optim.max_grad_norm = own
        stats = optim.grad_stats
    else:
        stats = clip_grad_norm_(net.parameters(), max_norm)
        optim.step()
    if stats is None:
        raise RuntimeError("backprop_for_loss: no parameter has a gradient")
    return stats[3].item() if sync else stats[3]
