"""The deterministic ICL transformer policy's output head -- what the reference's ``algo_factory`` (robomimic/algo/icl.py:41-75)
builds when ``algo.gmm.enabled`` is False (config/icl_config.py:63, the default): ``ICLTransformer``, whose network ends in the
``ObservationDecoder``'s one Linear ``action`` (robomimic/models/obs_nets.py:747-771 with ``output_shapes = OrderedDict(action=
(ac_dim,))``, policy_nets.py:1683-1690) and ``tanh`` (policy_nets.py:1728-1731), and whose losses are those of
``ICL._compute_losses`` (icl.py:174-202) with the weights of icl_config.py:43-45 (1.0 / 0.0 / 0.0):

    l2_weight MSELoss + l1_weight SmoothL1Loss + cos_weight cosine_loss(actions[..., :3], target[..., :3])

-- on the HIP library (csrc/lipvq_action_head.hip).

``ActionHead`` owns the decoder's module tree (``nets.action``: one ``nn.Linear`` with torch's default init), so ``state_dict()``
keys and the RNG consumption of a seeded construction are the reference's, and a checkpoint's ``policy.nets.decoder.*`` sub-dict
loads with ``strict=True``.  The child is a parameter CONTAINER only: no method calls it.  The compute is

    lipvq_action_head_f32       the Linear as one fp32-MFMA product (the GMM head's product stage), tanh, and -- with a target --
                                the three losses' deterministic sums (one more one-workgroup launch) and their weighted sum
    lipvq_action_head_bwd_f32   the gradient of the [rows, A] pre-activations, one elementwise launch; the upstream gradient of the
                                four losses is read on the device
    lipvq_wgrad_f32, lipvq_linear_act_f32      the two parameter gradients and the input gradient (ops.head_linear_grads)

``set_matmul_precision("bf16" | "bf16x3")`` moves the Linear onto the bf16 matrix pipe (lipvq_action_head_mp_f32; the gradients:
lipvq_linear_nn_<mode>, lipvq_wgrad_<mode>), as the backbone's setter does for its Linears; the default is fp32.

``feats`` may be the non-contiguous view ``out[:, -T:]`` or ``out[:, -1:]`` of a ``GPTBackbone`` output: its strides go to the
kernel and the forward makes no copy (the backward's wgrad reads a dense copy of those rows, and the input gradient comes back
dense, in the view's shape; autograd scatters it into the backbone output's gradient).  No kernel here uses float atomics and no
method reads a device value on the host: losses and gradients repeat bit for bit, and every method can be captured in a HIP graph.

Which rows are supervised is the caller's slice, as in the reference (icl.py:796-825):
``supervise_all_steps=True``  -> ``head.losses(out[:, -T:], actions)``;
``supervise_all_steps=False`` -> ``head.losses(out[:, -1:], actions[:, -1][:, None])`` (the last step alone).
``get_action`` (icl.py:845-851) picks one row of the forward: ``head(out[:, -T:])[:, -1]``, or ``[:, 0]`` with
``supervise_all_steps`` and ``pred_future_acs``.  ``use_tanh`` variants of the Gaussian policies are other heads, not built here.
"""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn as nn

from . import ops
from .nnfn import KernelFunction, first_order_only, wants_backward

__all__ = ["ActionHead"]

LOSS_KEYS = ("l2_loss", "l1_loss", "cos_loss", "action_loss")       # ICL._compute_losses' keys, in its order


class _ActionsFn(KernelFunction):
    """actions [B, T, A] over lipvq_action_head_f32 / lipvq_action_head_bwd_f32 (the gy mode)."""

    @staticmethod
    def forward(ctx, feats, W, b, precision="fp32"):
        keep = wants_backward(ctx)
        out = ops.action_head(feats, W, b, want_pre=keep, precision=precision)
        if keep:
            ctx.precision = precision
            ctx.save_for_backward(feats, out["pre"], W)
        return out["actions"].view(tuple(feats.shape[:-1]) + (W.shape[0],))

    @staticmethod
    @first_order_only
    def backward(ctx, gy):
        feats, pre, W = ctx.saved_tensors
        gpre = ops.action_head_bwd(pre, gy=gy.reshape(pre.shape))
        need = ctx.needs_input_grad
        g = ops.head_linear_grads(need[0], need[1] or need[2], feats, gpre, (W,), ctx.precision)
        return (g + (None,))[:len(need)]                            # (precision is optional: one gradient slot per argument given)


class _LossesFn(KernelFunction):
    """losses [4] = (l2, l1, cos, action) over lipvq_action_head_f32 / lipvq_action_head_bwd_f32; the backward's upstream
    gradient [4] stays on the device."""

    @staticmethod
    def forward(ctx, feats, target, W, b, weights, precision="fp32"):
        keep = wants_backward(ctx)
        out = ops.action_head(feats, W, b, target, weights, want_actions=False, want_pre=keep, precision=precision)
        if keep:
            ctx.weights, ctx.precision = weights, precision
            ctx.save_for_backward(feats, target, out["pre"], W)
        return out["losses"]

    @staticmethod
    @first_order_only
    def backward(ctx, g):
        feats, target, pre, W = ctx.saved_tensors
        gpre = ops.action_head_bwd(pre, target, g=g, weights=ctx.weights)
        need = ctx.needs_input_grad
        gx, gW, gb = ops.head_linear_grads(need[0], need[2] or need[3], feats, gpre, (W,), ctx.precision)
        return (gx, None, gW, gb, None, None)[:len(need)]         # (precision is optional: one gradient slot per argument given)


class ActionHead(nn.Module):
    """The head and losses of the reference's ``ICLTransformer`` (policy_nets.py:1683-1731, icl.py:174-202) on the HIP library.

    ``forward`` is the network's output (the actions), ``losses`` the training path's ``_compute_losses`` on them."""

    MAX_AC_DIM, MAX_EMBED = 64, 1024

    def __init__(self, embed_dim, ac_dim):
        super().__init__()
        if not 1 <= ac_dim <= self.MAX_AC_DIM:
            raise ValueError(f"ActionHead: 1 <= ac_dim <= {self.MAX_AC_DIM} (got {ac_dim})")
        if embed_dim <= 0 or embed_dim % 4 != 0 or embed_dim > self.MAX_EMBED:
            raise ValueError(f"ActionHead: embed_dim={embed_dim} must be a multiple of 4, <= {self.MAX_EMBED}")
        self.embed_dim = embed_dim
        self.ac_dim = ac_dim
        self.nets = nn.ModuleDict()                                 # ObservationDecoder._create_layers: one layer, `action`
        self.nets["action"] = nn.Linear(embed_dim, ac_dim)
        self._matmul_precision = "fp32"

    @property
    def matmul_precision(self) -> str:
        """"fp32" (default), "bf16" or "bf16x3": how the head's Linear multiplies (set_matmul_precision)."""
        return self._matmul_precision

    def set_matmul_precision(self, precision: str) -> "ActionHead":
        """"bf16" / "bf16x3": the head's Linear -- in ``forward`` and ``losses``, and its two gradients in their backward -- runs
        on the bf16 matrix pipe by ``GPTBackbone.set_matmul_precision``'s rules: operands rounded to bf16 (nearest even; "bf16x3":
        split into hi + lo, three products) as the kernel reads them, fp32 accumulation, every tensor fp32; the pre-activations
        have the bits of ``ops.linear_bf16`` / ``ops.linear_bf16x3``, and tanh, the losses and their backward are the fp32 code.
        "fp32" restores the default bit for bit.  The bf16 modes need embed_dim % 8 == 0.  Not part of state_dict(); a captured
        graph keeps the mode it was captured in; returns self."""
        ops._matmul_mode("ActionHead", precision, self.embed_dim)
        self._matmul_precision = precision
        return self

    def _check(self, feats, target=None):
        if not feats.is_cuda:
            raise RuntimeError("ActionHead runs on the HIP library only (no CPU path)")
        if feats.dim() != 3 or feats.shape[-1] != self.embed_dim:
            raise ValueError(f"ActionHead: feats must be [B, T, {self.embed_dim}], got {tuple(feats.shape)}")
        if target is not None and tuple(target.shape) != tuple(feats.shape[:2]) + (self.ac_dim,):
            raise ValueError(f"ActionHead: target must be {tuple(feats.shape[:2]) + (self.ac_dim,)}, got {tuple(target.shape)}")
        return feats if feats.dtype == torch.float32 else feats.float()

    def forward(self, feats):
        """actions [B, T, A] = tanh(feats W^T + b) (policy_nets.py:1728-1731), with autograd.  No host synchronisation: capturable
        by nnfn.GraphedEval, and the ``head`` of icl.PromptedPolicy."""
        feats = self._check(feats)
        return _ActionsFn.apply(feats, self.nets["action"].weight, self.nets["action"].bias, self._matmul_precision)

    def losses(self, feats, target, l2_weight=1.0, l1_weight=0.0, cos_weight=0.0):
        """ICL._compute_losses (icl.py:174-202) of the head's actions on feats [B, T, E] against target [B, T, A]: an OrderedDict
        with the reference's keys in its order -- l2_loss, l1_loss, cos_loss, action_loss (= the weighted sum) -- as 0-dim device
        tensors; a backward is possible through any of them.  No host read: capturable (icl.GraphedPolicyStep)."""
        feats = self._check(feats, target)
        out = _LossesFn.apply(feats, target.detach().float(), self.nets["action"].weight, self.nets["action"].bias,
                              (float(l2_weight), float(l1_weight), float(cos_weight)), self._matmul_precision)
        return OrderedDict((k, out[i]) for i, k in enumerate(LOSS_KEYS))
