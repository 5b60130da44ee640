"""What the transformer-style modules (embedding.py, default_branch.py, gpt.py) share: Linear and residual + LayerNorm as
``torch.autograd.Function``s over the library's kernels, and the eval-forward HIP-graph wrapper."""
from __future__ import annotations

import torch

from . import ops
from .capture import capture, copy_in, warm_up
from .ops import ACT_NONE

__all__ = ["LinearFn", "AddLayerNormFn", "GraphedEval"]


class LinearFn(torch.autograd.Function):
    """act(x W^T + b) over the last dimension, b optional; backward = act' (elementwise), one more Linear (gx), the wgrad kernel.
    precision="bf16": the three matrix products run on the bf16 matrix pipe (ops.linear_bf16 / linear_nn_bf16 / wgrad_bf16:
    operands rounded to bf16 as they are read, fp32 accumulation, fp32 tensors); precision="bf16x3": the same pipe with every
    operand split into two bf16 numbers and three products per product (ops.linear_bf16x3 / linear_nn_bf16x3 / wgrad_bf16x3);
    act' stays the fp32 kernel."""

    @staticmethod
    def forward(ctx, x, W, b, act, precision="fp32"):
        if precision not in ("fp32", "bf16", "bf16x3"):
            raise ValueError(f"LinearFn: precision must be 'fp32', 'bf16' or 'bf16x3', got {precision!r}")
        ctx.act, ctx.has_bias, ctx.shape, ctx.pipe = act, b is not None, x.shape, ("" if precision == "fp32" else "_" + precision)
        linear = getattr(ops, "linear" + ctx.pipe)
        x2 = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])      # (2-D callers: no view objects on their host-bound paths)
        if act != ACT_NONE:
            y, pre = linear(x2, W, b, act=act, save_pre=True)
            ctx.save_for_backward(x2, W, pre)
        else:
            y = linear(x2, W, b)
            ctx.save_for_backward(x2, W)
        return y if x.dim() == 2 else y.view(*x.shape[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, gy):
        gy = gy.reshape(-1, gy.shape[-1]).contiguous()
        if ctx.act != ACT_NONE:
            x2, W, pre = ctx.saved_tensors
            gy = ops.act_bwd(gy, pre, ctx.act)
        else:
            x2, W = ctx.saved_tensors
        gx = gW = gb = None
        if ctx.needs_input_grad[0]:
            gx = (getattr(ops, "linear_nn" + ctx.pipe)(gy, W) if ctx.pipe else ops.linear(gy, W.t().contiguous())).view(ctx.shape)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gW, gb = getattr(ops, "wgrad" + ctx.pipe)(gy, x2, want_bias=ctx.has_bias)
        return gx, gW, gb, None, None


class AddLayerNormFn(torch.autograd.Function):
    """(s, y) = (a + b, LayerNorm(a + b) w + bias), b optional; s is None unless want_s (a post-norm residual and the closing
    LayerNorm of a pre-norm stack discard it, and without b the caller keeps using a).  Backward: the gradient of a and of b is
    LayerNorm's plus the gradient that arrives for s (the residual stream), added inside the kernel."""

    @staticmethod
    def forward(ctx, a, b, w, bias, eps, want_s):
        ctx.set_materialize_grads(False)
        ctx.has_b = b is not None
        if not any(ctx.needs_input_grad):                      # eval / no_grad: nothing is kept for a backward
            return ops.gpt_layernorm(a, b, w, bias, eps, want_s=want_s)
        s, y, xhat, rstd = ops.gpt_layernorm(a, b, w, bias, eps, want_s=want_s, save=True)
        ctx.save_for_backward(xhat, rstd, w)
        return s, y

    @staticmethod
    def backward(ctx, gs, gy):
        if gy is None:
            return gs, (gs if ctx.has_b else None), None, None, None, None
        xhat, rstd, w = ctx.saved_tensors
        g, gw, gb = ops.gpt_layernorm_bwd(gy.contiguous(), xhat, rstd, w, None if gs is None else gs.contiguous())
        return g, (g if ctx.has_b else None), gw, gb, None, None


class GraphedEval:
    """Eval-mode forward of ``net`` captured in ONE HIP graph for the shape of ``example``.  Parameters are read at replay time
    through their storage, so in-place updates (optimizer steps, load_state_dict) are seen; re-capture after anything that
    REPLACES a parameter tensor (.to(), .cuda()).  The returned tensor is the graph's own output buffer: copy it before the next
    call if it must survive."""

    def __init__(self, net: torch.nn.Module, example: torch.Tensor, /):
        if net.training:
            raise RuntimeError(f"{type(self).__name__} captures the eval-mode forward: call net.eval() first")
        self.net = net
        self._x = example.detach().contiguous().float().clone()
        with torch.no_grad():
            warm_up(lambda: net(self._x), 3, self._x.device)      # first-use work (LDS reservations, lazy module state) stays out of the capture
            self._graph, self._y = capture(lambda: net(self._x))

    def __call__(self, inputs: torch.Tensor, /) -> torch.Tensor:
        copy_in(self._x, inputs, "captured")
        self._graph.replay()
        return self._y
