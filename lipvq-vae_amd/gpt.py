"""The ICRT transformer backbone -- the reference's ``GPT_Backbone`` (robomimic/models/transformers.py:80-439), which
``ICLTransformer`` builds at obs_nets.py:2453-2463 (embed_dim 512, 8 heads, 6 layers, context 3 T = 30, icl_config.py:133-153)
and feeds with the ``[B, 3T, E]`` tensor that ``ICLInputEmbedding`` (embedding.py) writes -- on the HIP library.

``GPTBackbone`` has the reference's constructor signature and the reference's module tree (``nets.transformer.{i}.nets.
attention.nets.qkv`` ...), built in the reference's order, so ``state_dict()`` keys, shapes and order, the RNG consumption of a
seeded construction (default ``nn.Linear`` init, then ``normal_(0, 0.02)`` in ``apply`` order) and therefore the parameter
bytes are the reference's, and a checkpoint's ``policy.nets.transformer.*`` sub-dict loads with ``strict=True``.  The
children are parameter CONTAINERS only: ``forward`` never calls them.  Per block the compute is

    lipvq_gpt_layernorm_f32      s = x + previous sub-layer, y = ln1(s)              (one launch, both written)
    lipvq_linear_act_f32         qkv = y Wqkv^T                                      (no bias, transformers.py:136)
    lipvq_gpt_attention_f32      batched causal attention, all (b, h) in one launch
    lipvq_linear_act_f32         output projection
    lipvq_gpt_layernorm_f32      s = s + attention branch, y = ln2(s)
    lipvq_linear_act_f32 x 2     Linear(E, 4E) + GELU, Linear(4E, E)

and one more lipvq_gpt_layernorm_f32 closes the last residual and applies ``output_ln``: 6 launches per block, 37 for the ICRT
model.  Every op is a ``torch.autograd.Function`` over the backward kernels (lipvq_gpt_attention_bwd_f32,
lipvq_gpt_layernorm_bwd_f32 -- which folds the residual stream's incoming gradient in --, lipvq_act_bwd_f32, lipvq_wgrad_f32);
none of them uses float atomics, so gradients repeat bit for bit.  ``set_matmul_precision("bf16")`` moves the four Linears of
every block -- forward, input gradient, weight gradient -- to lipvq_linear_act_bf16 / lipvq_linear_nn_bf16 / lipvq_wgrad_bf16
(operands rounded to bf16 as they are read, fp32 accumulation, fp32 tensors, still no atomics), ``"bf16x3"`` to their
_bf16x3 siblings (every operand split into two bf16 numbers, three products per product: near fp32 accuracy on the same pipe);
the default is fp32.

Rollouts (``ICLTransformer.get_action``, icl.py:827-853) pass the same context for a whole evaluation, so the first 2T of the
3T positions (obs_nets.py:2584-2596) and, the backbone being causal and adding no positional term of its own, every block's
keys and values there are constants of it.  ``cache = prefill(prompt_embeddings)`` runs those rows once and keeps each block's
qkv tensor; ``forward_cached(embeddings, cache)`` runs the same 6 launches per block on the new rows alone, with
lipvq_gpt_attention_prefix_f32 in place of lipvq_gpt_attention_f32, and returns the bits ``forward`` gives for those rows
(DESIGN.md 4.6.2).  Eval mode and causal backbones only; ``PromptedGPTBackbone`` wraps a (backbone, cache) pair for GraphedEval.

Dropout (training mode, torch's RNG): the attention-probability mask is drawn here as ``keep`` bytes ``[B, H, L, L]`` and
applied inside the attention kernel; the two block-output dropouts (transformers.py:205, :289) are applied BY TORCH
(``F.dropout`` on the branch before the fused residual launch) -- they are elementwise over ``[B L, E]`` and vanish in eval.
Training-mode outputs match the reference in distribution, not in bits (torch draws the attention mask inside its own
dropout kernel).  ``activation="geglu"`` is not implemented (the ICRT configuration uses ``gelu``).

Dropout, the opt-in in-kernel source (``set_dropout_source("kernel")``): the same three sites are decided INSIDE the kernels
that touch those elements -- the attention probabilities in lipvq_gpt_attention_drop_f32 / _bwd_drop_f32, a branch in the
residual launch that adds it, lipvq_gpt_layernorm_drop_f32 / _bwd_drop_f32 (the attention-output branch on ln2, the MLP branch
on the next block's ln1 or the closing output_ln).  ``forward`` is ONE block loop for both sources: per site it hands the same
Function either the torch-drawn mask / dropped branch or ``dropout=(snap, site, p)``, and a site with p == 0 takes the plain form.  Every decision is a pure function of (seed, step, site = 4 layer + 0 / 1 / 2,
row, col) through Philox4x32-10 (csrc/lipvq_rng.h; the contract is in include/lipvq.h): no mask tensor exists, nothing of it is
saved, the backward regenerates it, and torch's generators are not touched.  One one-thread launch per training forward
(lipvq_dropout_begin) hands the call its (seed, step) and advances the step on the device, so a captured graph advances on every
replay.  The launch count of a training forward is the eval forward's plus that one.  Eval mode ignores the source.
"""
from __future__ import annotations

import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .derived import stamp
from .nnfn import AddLayerNormFn, GraphedEval, KernelDropoutSource, KernelFunction, LinearFn, first_order_only, wants_backward
from .ops import ACT_GELU, ACT_NONE

__all__ = ["GPTBackbone", "GraphedGPTBackbone", "PromptCache", "PromptedGPTBackbone", "StalePromptCache"]


class StalePromptCache(RuntimeError):
    """forward_cached: the cache no longer belongs to the backbone's parameters or matmul precision; prefill() again."""


class _AttentionFn(KernelFunction):
    """Batched attention over qkv [B, L, 3E] with the attention-probability dropout of either source: keep [B, H, L, L] bytes
    with keep_prob (torch's generator), or dropout=(snap, site, p) drawn inside the kernels -- then no mask is saved, the two
    backward launches regenerate the decisions from snap."""

    @staticmethod
    def forward(ctx, qkv, nhead, causal, keep=None, keep_prob=1.0, dropout=None):
        out, lse = ops.gpt_attention(qkv, nhead, causal, keep, keep_prob, dropout=dropout)
        if wants_backward(ctx):
            ctx.nhead, ctx.causal, ctx.keep, ctx.keep_prob, ctx.dropout = nhead, causal, keep, keep_prob, dropout
            ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    @first_order_only
    def backward(ctx, gout):
        qkv, out, lse = ctx.saved_tensors
        return (ops.gpt_attention_bwd(qkv, out, gout.contiguous(), lse, ctx.nhead, ctx.causal, ctx.keep, ctx.keep_prob,
                                      dropout=ctx.dropout), None, None, None, None, None)


class _SelfAttention(nn.Module):
    """Parameter container with the reference's names (transformers.py:133-151)."""

    def __init__(self, embed_dim, num_heads, context_length, causal, attn_dropout, output_dropout):
        super().__init__()
        self.nets = nn.ModuleDict()
        self.nets["qkv"] = nn.Linear(embed_dim, 3 * embed_dim, bias=False)
        self.nets["attn_dropout"] = nn.Dropout(attn_dropout)
        self.nets["output_dropout"] = nn.Dropout(output_dropout)
        self.nets["output"] = nn.Linear(embed_dim, embed_dim)
        mask = torch.ones(context_length, context_length)
        if causal:
            mask = torch.tril(mask)
        self.register_buffer("mask", mask.view(1, 1, context_length, context_length))


class _SelfAttentionBlock(nn.Module):
    """Parameter container with the reference's names (transformers.py:267-294)."""

    def __init__(self, embed_dim, num_heads, context_length, causal, attn_dropout, output_dropout):
        super().__init__()
        self.nets = nn.ModuleDict()
        self.nets["attention"] = _SelfAttention(embed_dim, num_heads, context_length, causal, attn_dropout, output_dropout)
        self.nets["mlp"] = nn.Sequential(nn.Linear(embed_dim, 4 * embed_dim), nn.GELU(), nn.Linear(4 * embed_dim, embed_dim),
                                         nn.Dropout(output_dropout))
        self.nets["ln1"] = nn.LayerNorm(embed_dim)
        self.nets["ln2"] = nn.LayerNorm(embed_dim)


class GPTBackbone(KernelDropoutSource, nn.Module):
    """Drop-in for the reference's ``GPT_Backbone`` (transformers.py:321-440) on the HIP library."""

    MAX_CONTEXT, MAX_EMBED, HEAD_WIDTHS = 128, 1024, (16, 32, 64)
    DROPOUT_OWNER = "GPTBackbone"

    def __init__(self, embed_dim, context_length, causal=True, attn_dropout=0.1, block_output_dropout=0.1, num_layers=6,
                 num_heads=8, activation="gelu"):
        super().__init__()
        if activation == "geglu":
            raise NotImplementedError("GPTBackbone: activation='geglu' is not implemented on the HIP path (the ICRT configuration "
                                      "uses 'gelu'); keep the reference's GPT_Backbone for GEGLU models")
        if activation != "gelu":
            raise ValueError(f"GPTBackbone: unknown activation {activation!r}")
        if embed_dim % num_heads != 0 or embed_dim // num_heads not in self.HEAD_WIDTHS:
            raise ValueError(f"GPTBackbone: embed_dim={embed_dim} / num_heads={num_heads} must give a head width in {self.HEAD_WIDTHS}")
        if embed_dim > self.MAX_EMBED or not 1 <= context_length <= self.MAX_CONTEXT:
            raise ValueError(f"GPTBackbone: embed_dim <= {self.MAX_EMBED} and 1 <= context_length <= {self.MAX_CONTEXT} "
                             f"(got {embed_dim}, {context_length})")
        self.embed_dim = embed_dim
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.context_length = context_length
        self.causal = causal
        self.attn_dropout = attn_dropout
        self.block_output_dropout = block_output_dropout
        self.nets = nn.ModuleDict()
        self.nets["transformer"] = nn.Sequential(*[
            _SelfAttentionBlock(embed_dim, num_heads, context_length, causal, attn_dropout, block_output_dropout)
            for _ in range(num_layers)])
        self.nets["output_ln"] = nn.LayerNorm(embed_dim)
        self.apply(self._init_weights)
        self._matmul_precision = "fp32"
        self._dropout_source = "torch"            # (set_dropout_source, reseed_dropout, dropout_state: nnfn.KernelDropoutSource)

    @property
    def matmul_precision(self) -> str:
        """"fp32" (default), "bf16" or "bf16x3": how the four Linears of every block multiply (set_matmul_precision)."""
        return self._matmul_precision

    def set_matmul_precision(self, precision: str) -> "GPTBackbone":
        """"bf16": the four Linears of every block -- forward, input gradient and weight gradient -- run on the bf16 matrix
        pipe: both operands of each product are rounded to bf16 (nearest even) as the kernel reads them, products are
        accumulated in fp32, and every tensor (activations, saved tensors, gradients, parameters) stays fp32.  Attention,
        LayerNorm, GELU and its derivative stay fp32.  "fp32" restores the default bit for bit.  Needs embed_dim % 8 == 0
        (every supported head width gives that).  Not part of state_dict(); returns self.

        "bf16x3" (torch's "bfloat16_3x"): the same Linears on the same pipe, with every fp32 operand element split into
        hi = bf16(v) and lo = bf16(v - hi) and a_lo b_hi + a_hi b_lo + a_hi b_hi accumulated in fp32: about 2^-16 relative
        per product instead of 2^-8, for three times the matrix-pipe work (include/lipvq.h states the bound and its limits)."""
        if precision not in ("fp32", "bf16", "bf16x3"):
            raise ValueError(f"GPTBackbone: matmul precision must be 'fp32', 'bf16' or 'bf16x3', got {precision!r}")
        self._matmul_precision = precision
        return self

    @staticmethod
    def _init_weights(module):
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(mean=0.0, std=0.02)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)

    def output_shape(self, input_shape=None):
        return list(input_shape)

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        """One block loop for eval and for training under either dropout source.  Torch source: the attention mask is drawn here
        as keep bytes and a branch is dropped by F.dropout before the residual launch.  Kernel source: one dropout_begin launch,
        then the same launches per block as eval, each site with p > 0 handed dropout=(snap, site, p); a branch's dropout rides
        on the residual launch that adds the branch: the attention-output branch's on ln2, the MLP branch's on the NEXT block's
        ln1 (the closing output_ln for the last)."""
        assert inputs.shape[1:] == (self.context_length, self.embed_dim), inputs.shape
        if not inputs.is_cuda:
            raise RuntimeError("GPTBackbone runs on the HIP library only (no CPU path)")
        x = inputs.contiguous().float()
        B, L, H = x.shape[0], self.context_length, self.num_heads
        prec, causal = self._matmul_precision, bool(self.causal)
        training, kernel = self.training, self._kernel_dropout()
        snap = self._dropout_begin(x.device) if kernel else None

        def drop(t, site, p):
            """a branch of site `site` with p > 0 -> (the tensor to add, the dropout the adding launch applies or None)"""
            return (t, (snap, site, p)) if kernel else (F.dropout(t, p, True), None)

        a, b, b_drop = x, None, None
        p_att = p_out = p_mlp = 0.0                            # eval: every site takes the plain form
        for i, blk in enumerate(self.nets["transformer"]):
            att, mlp, ln1, ln2 = blk.nets["attention"], blk.nets["mlp"], blk.nets["ln1"], blk.nets["ln2"]
            if kernel:
                p_att, p_out, p_mlp = (self._dropout_p(att.nets["attn_dropout"].p, "attn_dropout"),
                                       self._dropout_p(att.nets["output_dropout"].p, "output_dropout"),
                                       self._dropout_p(mlp[3].p, "mlp dropout"))
            elif training:
                p_att, p_out, p_mlp = float(att.nets["attn_dropout"].p), float(att.nets["output_dropout"].p), float(mlp[3].p)
            keep, keep_prob, att_drop = None, 1.0, None
            if p_att > 0.0:
                if kernel:
                    att_drop = (snap, 4 * i, p_att)
                else:
                    keep = (torch.rand((B, H, L, L), device=x.device) >= p_att).to(torch.uint8)
                    keep_prob = 1.0 - p_att
            if b is None:                                      # first block: the stream is the input itself, nothing to add or copy
                s, y = a, AddLayerNormFn.apply(a, None, ln1.weight, ln1.bias, ln1.eps, False)[1]
            else:
                s, y = AddLayerNormFn.apply(a, b, ln1.weight, ln1.bias, ln1.eps, True, b_drop)
            qkv = LinearFn.apply(y, att.nets["qkv"].weight, None, ACT_NONE, prec)
            o = _AttentionFn.apply(qkv, H, causal, keep, keep_prob, att_drop)
            o = LinearFn.apply(o, att.nets["output"].weight, att.nets["output"].bias, ACT_NONE, prec)
            o_drop = None
            if p_out > 0.0:
                o, o_drop = drop(o, 4 * i + 1, p_out)
            s, y = AddLayerNormFn.apply(s, o, ln2.weight, ln2.bias, ln2.eps, True, o_drop)
            f = LinearFn.apply(y, mlp[0].weight, mlp[0].bias, ACT_GELU, prec)
            f = LinearFn.apply(f, mlp[2].weight, mlp[2].bias, ACT_NONE, prec)
            a, b, b_drop = s, f, None
            if p_mlp > 0.0:
                b, b_drop = drop(f, 4 * i + 2, p_mlp)
        ln = self.nets["output_ln"]
        return AddLayerNormFn.apply(a, b, ln.weight, ln.bias, ln.eps, False, b_drop)[1]

    # -- the prompt cache: a rollout's constant prefix is run once, every step runs its new tokens alone ---------------------
    def _cacheable(self, what):
        if self.training:
            raise RuntimeError(f"GPTBackbone.{what} is an eval-mode path (no dropout, no backward): call eval() first")
        if not self.causal:
            raise ValueError(f"GPTBackbone.{what}: a non-causal prefix sees the tokens after it, so no cache of it is valid")

    def _param_versions(self):
        """``derived.stamp`` of every parameter: an in-place write moves the version, ``p.data = new`` / ``.to()`` the address."""
        return stamp(self.parameters())

    def _blocks_eval(self, x, prefix, record):
        """The eval forward on the rows of x.  record (a list): plain causal attention, every block's qkv is appended and the
        last block stops there (prefill).  Otherwise the attention of block i also sees the cached keys and values prefix[i]."""
        H, prec = self.num_heads, self._matmul_precision
        blocks = self.nets["transformer"]
        a, b = x, None
        for i, blk in enumerate(blocks):
            att, mlp, ln1, ln2 = blk.nets["attention"], blk.nets["mlp"], blk.nets["ln1"], blk.nets["ln2"]
            if b is None:
                s, y = a, AddLayerNormFn.apply(a, None, ln1.weight, ln1.bias, ln1.eps, False)[1]
            else:
                s, y = AddLayerNormFn.apply(a, b, ln1.weight, ln1.bias, ln1.eps, True)
            qkv = LinearFn.apply(y, att.nets["qkv"].weight, None, ACT_NONE, prec)
            if record is not None:
                record.append(qkv)
                if i == len(blocks) - 1:                        # the prefix's own output is not needed
                    return None
                o = ops.gpt_attention(qkv, H, True)[0]
            else:
                o = ops.gpt_attention_prefix(prefix[i], qkv, H)
            o = LinearFn.apply(o, att.nets["output"].weight, att.nets["output"].bias, ACT_NONE, prec)
            s, y = AddLayerNormFn.apply(s, o, ln2.weight, ln2.bias, ln2.eps, True)
            f = LinearFn.apply(y, mlp[0].weight, mlp[0].bias, ACT_GELU, prec)
            f = LinearFn.apply(f, mlp[2].weight, mlp[2].bias, ACT_NONE, prec)
            a, b = s, f
        ln = self.nets["output_ln"]
        return AddLayerNormFn.apply(a, b, ln.weight, ln.bias, ln.eps, False)[1]

    @torch.no_grad()
    def prefill(self, prompt_embeddings: torch.Tensor) -> "PromptCache":
        """Run the constant prefix [Bp, P, E] of a rollout once and keep every block's qkv rows (``PromptCache``:
        layers x Bp x P x 3E floats).  Blocks 0 .. n-2 run in full on the P rows, the last one up to its qkv Linear.  Eval mode,
        causal backbones only.  The cache belongs to the parameters and the matmul precision it was made under."""
        self._cacheable("prefill")
        if prompt_embeddings.dim() != 3 or prompt_embeddings.shape[2] != self.embed_dim:
            raise ValueError(f"GPTBackbone.prefill: prompt embeddings must be [Bp, P, {self.embed_dim}], got {tuple(prompt_embeddings.shape)}")
        Bp, P, E = prompt_embeddings.shape
        if P > self.context_length:
            raise ValueError(f"GPTBackbone.prefill: P={P} exceeds context_length={self.context_length}")
        if not prompt_embeddings.is_cuda:
            raise RuntimeError("GPTBackbone runs on the HIP library only (no CPU path)")
        x = prompt_embeddings.contiguous().float()
        qkv = []
        if Bp == 0 or P == 0:                                       # no rows: nothing to launch
            qkv = [x.new_empty((Bp, P, 3 * E)) for _ in self.nets["transformer"]]
        else:
            self._blocks_eval(x, None, qkv)
        return PromptCache(tuple(qkv), Bp, P, self._matmul_precision, self._param_versions(), weakref.ref(self))

    @torch.no_grad()
    def forward_cached(self, embeddings: torch.Tensor, cache: "PromptCache") -> torch.Tensor:
        """[B, Lq, E] -> [B, Lq, E]: ``self(cat([prompt, embeddings], 1))[:, P:]`` from the Lq new rows and ``cache =
        prefill(prompt)`` alone -- the same 6 launches per block and the closing LayerNorm, on Lq rows, with
        lipvq_gpt_attention_prefix_f32 reading the cached keys and values.  P + Lq <= context_length; Bp == B or 1."""
        self._cacheable("forward_cached")
        if embeddings.dim() != 3 or embeddings.shape[2] != self.embed_dim:
            raise ValueError(f"GPTBackbone.forward_cached: embeddings must be [B, Lq, {self.embed_dim}], got {tuple(embeddings.shape)}")
        if not embeddings.is_cuda:
            raise RuntimeError("GPTBackbone runs on the HIP library only (no CPU path)")
        B, Lq = embeddings.shape[:2]
        if cache.P + Lq > self.context_length:
            raise ValueError(f"GPTBackbone.forward_cached: P + Lq = {cache.P} + {Lq} exceeds context_length={self.context_length}")
        if cache.Bp not in (1, B):
            raise ValueError(f"GPTBackbone.forward_cached: the cache holds {cache.Bp} prompts, the input {B} sequences (B, or 1 shared by all)")
        if len(cache.qkv) != len(self.nets["transformer"]) or any(t.shape[2] != 3 * self.embed_dim or t.device != embeddings.device
                                                                  for t in cache.qkv):
            raise ValueError("GPTBackbone.forward_cached: the cache was made by another backbone or on another device")
        if cache.owner is not None and cache.owner() is not self:      # (same shapes and versions do not make it this one's)
            raise ValueError("GPTBackbone.forward_cached: the cache was made by another backbone (or a copy of this one): call "
                             "prefill() on this backbone")
        if cache.precision != self._matmul_precision:
            raise StalePromptCache(f"GPTBackbone.forward_cached: the cache was made under matmul precision {cache.precision!r}, "
                                   f"the backbone is now {self._matmul_precision!r}: call prefill() again")
        if cache.versions != self._param_versions():
            raise StalePromptCache("GPTBackbone.forward_cached: a parameter changed or was replaced after the cache was made (an "
                                   "optimizer step, load_state_dict, p.data = ..., .to()): the cached keys and values are stale, "
                                   "call prefill() again")
        x = embeddings.contiguous().float()
        if B == 0 or Lq == 0:
            return torch.empty_like(x)
        return self._blocks_eval(x, cache.qkv, None)


class PromptCache:
    """What ``GPTBackbone.prefill`` keeps of a prompt: ``qkv``, one [Bp, P, 3E] tensor per block exactly as the qkv Linear wrote it
    (the attention kernel reads K and V in place), with ``Bp``, ``P``, the matmul ``precision``, the ``(data_ptr, _version)`` of
    every parameter at that moment and a weak reference to the backbone that made it, all of which ``forward_cached`` compares
    with its own.  A write that moves neither a version nor an address (``p.data.add_()``) is invisible: prefill again."""

    __slots__ = ("qkv", "Bp", "P", "precision", "versions", "owner")

    def __init__(self, qkv, Bp, P, precision, versions, owner=None):
        self.qkv, self.Bp, self.P, self.precision, self.versions = qkv, int(Bp), int(P), precision, versions
        self.owner = owner

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.qkv)


class PromptedGPTBackbone(nn.Module):
    """``forward(embeddings) = backbone.forward_cached(embeddings, cache)``: a rollout step as a module, so that
    ``nnfn.GraphedEval(PromptedGPTBackbone(net.eval(), cache), example)`` replays it as one HIP graph (a single chain of
    launches on one stream).  The graph reads the cache by address and checks nothing at replay: after a parameter update or
    set_matmul_precision(), prefill again and capture again."""

    def __init__(self, backbone: GPTBackbone, cache: PromptCache):
        super().__init__()
        self.backbone = backbone
        self.cache = cache
        self.train(backbone.training)

    def forward(self, embeddings: torch.Tensor) -> torch.Tensor:
        return self.backbone.forward_cached(embeddings, self.cache)


class GraphedGPTBackbone(GraphedEval):
    """Eval-mode forward of a GPTBackbone captured in ONE HIP graph for a fixed [B, L, E] shape.

    The backbone is 6 small launches per block; at the ICRT step shape (B = 8, 240 rows) each is microseconds of GPU work, so
    an eager call is bound by Python + ctypes issue and a graph replay costs the GPU time alone.  Rollouts call the policy
    once per environment step with the same shape, which is what this serves.  Parameters are read at replay time through
    their storage, so in-place updates (optimizer steps, load_state_dict) are seen; re-capture after anything that REPLACES a
    parameter tensor (.to(), .cuda()).  The graph holds the kernels of the matmul precision that was set when it was captured:
    re-capture after set_matmul_precision().  The returned tensor is the graph's own output buffer: copy it before the next call
    if it must survive."""
