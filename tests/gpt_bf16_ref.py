"""The backbone's bf16 matrix-pipe mode restated in plain torch, on top of tests/gpt_ref.py (which is not edited): the same
op sequence with every Linear's two matrix operands rounded to bf16 (nearest even) in the forward, and -- because the mode
rounds the operands of the two backward products as well -- gx = round(g) round(W), gW = round(g)^T round(x), gb = sum(g)
in the backward.  Run on float64 tensors it is the emulation `emu` of tests/test_gpu_gemm_bf16.py: what the mode computes
with exact accumulation, so its distance from the float64 fixture is the mode's own rounding and nothing else."""
import torch
import torch.nn.functional as F

import gpt_ref


def bf16_round(t):
    """t with every element rounded to bf16 the way the kernels do it (from fp32, nearest even), in t's dtype."""
    return t.float().bfloat16().to(t.dtype)


class _RoundedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        ctx.has_bias = b is not None
        return F.linear(bf16_round(x), bf16_round(W), b)

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        gr = bf16_round(g)
        gx = gr @ bf16_round(W)
        gW = gr.reshape(-1, g.shape[-1]).t() @ bf16_round(x).reshape(-1, x.shape[-1])
        return gx, gW, (g.reshape(-1, g.shape[-1]).sum(0) if ctx.has_bias else None)


class _Functional:
    """torch.nn.functional with `linear` replaced; what gpt_ref's functions see as `F` inside `rounded_linears()`."""

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def linear(x, W, b=None):
        return _RoundedLinear.apply(x, W, b)


def gpt_forward_bf16(sd, inputs, num_layers, num_heads):
    """gpt_ref.gpt_forward with every F.linear of it replaced by the rounded Linear above."""
    saved = gpt_ref.F
    gpt_ref.F = _Functional()
    try:
        return gpt_ref.gpt_forward(sd, inputs, num_layers, num_heads)
    finally:
        gpt_ref.F = saved
