"""The DEFAULT action branch of the group encoder -- what ``ICLObservationGroupEncoder`` builds when none of
``fast_enabled / bin_enabled / vq_vae_enabled / ln_act_enabled`` is set (reference robomimic/models/obs_nets.py:1244-1260)
and calls as ``context_actions = self.action_network(prompt_actions)`` (obs_nets.py:1343-1344) -- on the HIP library.

``DefaultActionNetwork`` IS an ``nn.Sequential`` with the reference's children in the reference's order, so parameter names
(``0.weight_orig``, ``0.weight_u``, ``5.layers.2.self_attn.in_proj_weight``, ``6.bias`` ...), shapes, initial values and RNG
consumption are the reference's by construction and its checkpoints load unchanged.  The children are parameter CONTAINERS
only: ``forward`` never calls them.  The compute is
    3 x lipvq_spectral_norm_f32            (power iteration in training mode, writes weight_u / weight_v like torch's hook)
    lipvq_linear_act_f32 x 3               (spectral-norm MLP, GELU epilogues)
    4 x [in_proj Linear -> lipvq_attention_f32 -> out_proj Linear -> lipvq_gpt_layernorm_f32
         -> Linear+GELU -> Linear -> lipvq_gpt_layernorm_f32]                (post-norm encoder layers; the LayerNorm
                                                                              kernels are the backbone's, with s = NULL)
    lipvq_linear_act_f32                   (the closing Linear)
with backward kernels behind ``torch.autograd.Function``s.  The input is 2-D ``[B*T, A]``, which ``nn.TransformerEncoder``
treats as ONE unbatched sequence: every action of the batch attends to every other (S = B*T; the reference's behaviour,
kept).  Dropout (p = 0.1, four places per layer) follows torch's semantics with torch's own RNG -- elementwise ones through
``F.dropout``, the attention-probability one as a keep-mask handed to the kernel -- so training-mode outputs match the
reference in distribution, eval-mode outputs to 1e-5 (tests/test_gpu_default.py).

``set_dropout_source("kernel")`` (opt-in) decides the four dropouts of every encoder layer inside the kernels instead, at sites
``ops.DROPOUT_SITE_DEFAULT + 4 layer + k`` (include/lipvq.h): k = 0 the attention probabilities in lipvq_attention_drop_f32 /
_bwd_drop_f32, k = 1 dropout1 and k = 2 dropout2 in the residual launch that adds the branch (lipvq_gpt_layernorm_drop_f32 /
_bwd_drop_f32), k = 3 the FFN's inner dropout in linear1's epilogue (lipvq_linear_act_drop_f32 / lipvq_act_bwd_drop_f32).  One
``ops.dropout_begin`` launch per training forward; no ``rand``, no mask tensor, nothing of it saved, torch's generators untouched.
``forward`` is ONE encoder-layer loop for both sources: per site it hands the same Function either torch's mask / dropped tensor
or ``dropout=(snap, site, p)``; under the kernel source a site with p == 0 takes the plain entry point.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils import spectral_norm

from . import ops
from .nnfn import AddLayerNormFn, GraphedEval, KernelDropoutSource, KernelFunction, LinearFn, first_order_only, wants_backward
from .ops import ACT_GELU, ACT_NONE


class _SpectralFn(torch.autograd.Function):
    """weight_orig -> weight_orig / sigma (u, v: buffers, updated in place in training mode, constants for the gradient)."""

    @staticmethod
    def forward(ctx, W, u, v, training, eps):
        Wsn, sigma = ops.spectral_norm(W.detach(), u, v, training, eps)
        ctx.save_for_backward(Wsn, u.clone(), v.clone(), sigma)          # torch clones u, v after the iteration as well
        return Wsn

    @staticmethod
    @first_order_only
    def backward(ctx, gWsn):
        Wsn, u, v, sigma = ctx.saved_tensors
        return ops.spectral_norm_bwd(gWsn.contiguous(), Wsn, u, v, sigma), None, None, None, None


class _AttentionFn(KernelFunction):
    """Unbatched multi-head self-attention over qkv [S, 3D] (ops.attention) with the attention-probability dropout of either
    source: keep [H, S, S] bytes with keep_prob (torch's generator), or dropout=(snap, site, p) drawn inside the kernels -- then
    no mask is saved, the two backward launches regenerate the decisions."""

    @staticmethod
    def forward(ctx, qkv, nhead, keep=None, keep_prob=1.0, dropout=None):
        out, lse = ops.attention(qkv, nhead, keep, keep_prob, dropout=dropout)
        if wants_backward(ctx):
            ctx.nhead, ctx.keep, ctx.keep_prob, ctx.dropout = nhead, keep, keep_prob, dropout
            ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    @first_order_only
    def backward(ctx, gout):
        qkv, out, lse = ctx.saved_tensors
        return (ops.attention_bwd(qkv, out, gout.contiguous(), lse, ctx.nhead, ctx.keep, ctx.keep_prob, dropout=ctx.dropout),
                None, None, None, None)


class DefaultActionNetwork(KernelDropoutSource, nn.Sequential):
    """Drop-in for the reference's default ``action_network`` (obs_nets.py:1244-1260)."""

    NHEAD, FF = 8, 256
    DROPOUT_OWNER = "DefaultActionNetwork"

    def __init__(self, action_input_shape: int, action_output_shape: int, num_layers: int = 4):
        D = int(action_output_shape)
        if D % self.NHEAD != 0 or D // self.NHEAD > 32 or D > 256:
            raise ValueError(f"DefaultActionNetwork: action_output_shape={D} must be a multiple of {self.NHEAD} and <= 256")
        transformer_layer = nn.TransformerEncoderLayer(d_model=D, nhead=self.NHEAD, dim_feedforward=self.FF, activation="gelu")
        super().__init__(
            spectral_norm(nn.Linear(action_input_shape, 64)),
            nn.GELU(),
            spectral_norm(nn.Linear(64, 128)),
            nn.GELU(),
            spectral_norm(nn.Linear(128, D)),
            nn.TransformerEncoder(transformer_layer, num_layers=num_layers),
            nn.Linear(D, D),
        )
        self.latent_dim = D

    def _sn_weight(self, lin: nn.Linear) -> torch.Tensor:
        # torch's hook iterates only in training mode (spectral_norm.py: do_power_iteration=module.training)
        return _SpectralFn.apply(lin.weight_orig, lin.weight_u, lin.weight_v, self.training, 1e-12)

    def forward(self, prompt_actions: torch.Tensor) -> torch.Tensor:
        x = prompt_actions
        if x.dim() != 2:
            raise ValueError(f"DefaultActionNetwork expects the flattened [B*T, A] action tensor, got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("DefaultActionNetwork runs on the HIP library only (no CPU path)")
        x = x.contiguous().float()
        h = LinearFn.apply(x, self._sn_weight(self[0]), self[0].bias, ACT_GELU)
        h = LinearFn.apply(h, self._sn_weight(self[2]), self[2].bias, ACT_GELU)
        h = LinearFn.apply(h, self._sn_weight(self[4]), self[4].bias, ACT_NONE)
        S = h.shape[0]
        training, kernel = self.training, self._kernel_dropout()
        snap = self._dropout_begin(h.device) if kernel else None
        for i, layer in enumerate(self[5].layers):
            attn, site = layer.self_attn, ops.DROPOUT_SITE_DEFAULT + 4 * i
            keep, keep_prob = None, 1.0
            drops = (None, None, None, None)                   # site + k -> what its launch is handed under the kernel source
            if kernel:
                ps = (self._dropout_p(attn.dropout, "attention dropout"), self._dropout_p(layer.dropout1.p, "dropout1"),
                      self._dropout_p(layer.dropout2.p, "dropout2"), self._dropout_p(layer.dropout.p, "dropout"))
                drops = tuple((snap, site + k, p) if p > 0.0 else None for k, p in enumerate(ps))      # (p == 0: the plain form)
            elif training and float(attn.dropout) > 0.0:
                keep = (torch.rand((self.NHEAD, S, S), device=h.device) >= float(attn.dropout)).to(torch.uint8)
                keep_prob = 1.0 - float(attn.dropout)
            qkv = LinearFn.apply(h, attn.in_proj_weight, attn.in_proj_bias, ACT_NONE)
            a = _AttentionFn.apply(qkv, self.NHEAD, keep, keep_prob, drops[0])
            a = LinearFn.apply(a, attn.out_proj.weight, attn.out_proj.bias, ACT_NONE)
            if not kernel:
                a = F.dropout(a, layer.dropout1.p, training)
            h = AddLayerNormFn.apply(h, a, layer.norm1.weight, layer.norm1.bias, layer.norm1.eps, False, drops[1])[1]
            # the FFN's inner dropout: the kernel source decides it in linear1's epilogue, torch's on linear1's result
            f = LinearFn.apply(h, layer.linear1.weight, layer.linear1.bias, ACT_GELU, "fp32", drops[3])
            if not kernel:
                f = F.dropout(f, layer.dropout.p, training)
            f = LinearFn.apply(f, layer.linear2.weight, layer.linear2.bias, ACT_NONE)
            if not kernel:
                f = F.dropout(f, layer.dropout2.p, training)
            h = AddLayerNormFn.apply(h, f, layer.norm2.weight, layer.norm2.bias, layer.norm2.eps, False, drops[2])[1]
        return LinearFn.apply(h, self[6].weight, self[6].bias, ACT_NONE)


class GraphedDefaultBranch(GraphedEval):
    """Eval-mode forward of a DefaultActionNetwork captured in ONE HIP graph for a fixed [N, A] shape.

    The branch is ~40 small launches (at the ICRT step shape N = 80 every one of them is microseconds of GPU work), so an
    eager call is bound by Python + ctypes issue (~1.5 ms); a graph replay costs the GPU time alone.  Rollouts call the
    action branch once per environment step with the same prompt shape (obs_nets.py:1343-1344 under algo.py:736 set_eval()),
    which is what this serves.  Parameters are read at replay time through their storage, so in-place updates
    (optimizer steps, load_state_dict) are seen; re-capture after anything that REPLACES a parameter tensor (.to(), .cuda())."""
