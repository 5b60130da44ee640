"""torch.autograd.Function wrapper: the reference's forward()/backward() contract on the HIP path.

Forward value flow (LLFQVAE_V4, reference backbone_lfqvae_v5.py:70-84):
    x --mlp3(gelu,gelu,sigmoid; W2 = Lipschitz-normalised)--> z_e --nearest--> (idx, z_q)
    z_q --mlp3(gelu,gelu,none; input gathered from the codebook)--> x_recon
    loss = mse(x_recon,x) + 0.25*mse(z_q.detach(),z_e) + 0.25*mse(z_q,z_e.detach())
Gradient routing (no straight-through estimator in this variant):
    recon     -> to_output, decoder, codebook (through the gather)
    codebook  -> codebook
    commit    -> to_latent.{W,b,ci}, encoder
The two latent mse terms have the same VALUE; the library computes it once.

The plain VQVAE (reference backbone.py:38-76) runs the same function: ReLU stacks, the decoder on the straight-through value
z_st = z_e + (z_q - z_e), loss = m0 + (m1 + commitment_cost m1).  What differs is class data of the two modules (tokenizer.py).
"""
from __future__ import annotations

import torch

from . import ops
from .derived import stamp
from .nnfn import first_order_only
from .tokenizer import LLFQVAE_V4, VQVAE

# (the triples are defined on the tokenizer classes; these names are kept for tests and measurement scripts)
_ENC_ACTS, _DEC_ACTS, _RELU3 = LLFQVAE_V4._ENC_ACTS, LLFQVAE_V4._DEC_ACTS, VQVAE._ENC_ACTS


def _check_versions(ctx, params):
    """The backward kernels read the module's LIVE weights; refuse to run if one was modified in place or replaced since (``stamp``)."""
    saved = getattr(ctx, "param_versions", None) or ()       # (None: the forward kept nothing for a backward)
    for i, (p, was, now) in enumerate(zip(params, saved, stamp(params))):
        if now != was:
            raise RuntimeError(f"lipvq: parameter #{i} (shape {tuple(p.shape)}) was modified in place or replaced between forward "
                               f"and backward (version {was[1]} -> {now[1]}); the gradient would be computed with the new weights")


class _TokenizerFn(torch.autograd.Function):
    """(z_latent, loss) = f(x, the module's parameters in module._params() order).  z_latent is non-differentiable (v5:74).
    x gets NO gradient: backward returns None for it even where x.requires_grad (the reference's autograd would return one, the
    loss depends on x through the encoder and the reconstruction error; no caller here differentiates the tokenizer's input).
    The parameter gradients are all formed together, whichever subset of the parameters requires one; need_grad -- any parameter
    does -- picks the plan and what is saved.  First order only (nnfn.first_order_only)."""

    @staticmethod
    def forward(ctx, module, x, *params):
        # (the engine would otherwise hand backward() a materialised [N, D] zero tensor for the non-differentiable z_latent: a 134 MB
        # fill per step at the metric's batch)
        ctx.set_materialize_grads(False)
        m = module
        enc = m._packed_encoder()                        # LLFQVAE_V4: (packed, scale, W_norm) -- its backward reads the last two
        enc_packed, lipschitz = (enc[0], enc[1:]) if isinstance(enc, tuple) else (enc, ())
        dec_packed = m._packed_decoder()
        codebook = m._codebook().detach()
        need_grad = any(ctx.needs_input_grad[2:])
        # ask the plan (one routing decision per call) and run its route: large batches encoder + quantizer + everything the
        # backward needs in ONE launch (lipvq_tokenize_train_f32; without autograd lipvq_tokenize_f32, z_e written for the loss),
        # otherwise mlp3 (saved pre-activations) + one of the three quantizer routes
        plan = m._plan(x.shape[0], "forward", need_grad, decoder=dec_packed)
        idx, z_q, z_e, pre_e = m._encode_quantize(x, m.code_usage, plan, enc_packed)
        w = m._loss_weight
        if plan.fold_loss:
            # large batches: the decoder launch sums both squared errors itself (its input rows ARE z_q, its output x_rec); with
            # ste it forms z_st = z_e + (z_q - z_e) (vq:74) from codebook[idx] and z_e itself, runs on it and stores it -- no
            # separate straight-through and mse passes over the [N, D] operands
            out = ops.mlp3_loss(codebook, dec_packed, m._DEC_ACTS, idx, x, z_e, w, m._LOSS, save_pre=need_grad, ste=m._STE)
            x_rec, pre_d, l3 = out[:3]
            z_st = out[3] if m._STE else None
        else:
            z_st = ops.ste(z_e, z_q) if m._STE else None                                   # vq:74
            src, gather = (codebook, idx) if z_st is None else (z_st, None)
            if need_grad:
                x_rec, pre_d = ops.mlp3(src, dec_packed, m._DEC_ACTS, gather_idx=gather, save_pre=True)
            else:
                x_rec, pre_d = ops.mlp3(src, dec_packed, m._DEC_ACTS, gather_idx=gather), None
            l3 = ops.mse_pair_loss(x_rec, x, z_q, z_e, w, m._LOSS)
        latent = z_q if z_st is None else z_st
        m.last_indices = idx
        ctx.module = m
        if need_grad:
            ctx.save_for_backward(x, z_e, z_q, idx, x_rec, *lipschitz, *(() if z_st is None else (z_st,)), *pre_e, *pre_d)
            # backward() re-reads the module's live weights (decoder, codebook, encoder, to_latent): remember their versions, so
            # that a parameter update between forward and backward raises, as torch's saved-tensor check would
            ctx.param_versions = stamp(params)
        ctx.mark_non_differentiable(latent)
        return latent, l3[2]

    @staticmethod
    @first_order_only
    def backward(ctx, _g_latent, g_loss):
        m = ctx.module
        _check_versions(ctx, m._params())
        if g_loss is None:                               # the loss took no part in what is being differentiated
            return (None,) * len(ctx.needs_input_grad)
        return (None, None) + tuple(m._backward(ctx.saved_tensors, g_loss))


class _Ctx:
    """Stand-in for the autograd context where the engine is not used: the no-grad path (rollouts, tokenisation; nothing is
    saved) and forward_backward() (need_grad: the saved tensors are kept for the backward launches)."""

    def __init__(self, n_params, need_grad):
        self.needs_input_grad = (False, False) + (need_grad,) * n_params
        self.saved_tensors = ()
        self.module = None
        self.param_versions = None

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *a):
        pass

    def set_materialize_grads(self, flag):
        pass


def tokenizer_forward(module, x):
    """(z_latent, loss) of module(x).  Autograd is involved only where grad mode is on AND a parameter requires a gradient;
    otherwise the no-autograd path runs (nothing saved).  x.requires_grad plays no part: with every parameter frozen the returned
    loss does not require a gradient even if x does, and with a trainable parameter x still gets none (_TokenizerFn).  The three
    paths and forward_backward return the same z_latent and loss bits."""
    params = module._params()
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return _TokenizerFn.apply(module, x, *params)
    with torch.no_grad():
        return _TokenizerFn.forward(_Ctx(len(params), False), module, x, *params)


llfq_forward = vq_forward = tokenizer_forward


def forward_backward(module, x):
    """(z_latent, loss, params, grads) with grads = dloss/dparams computed by the library's backward kernels,
    without touching torch.autograd.  params are in the order of the returned gradients.  Engine-free: used under HIP-graph
    capture, where the autograd engine's per-parameter AccumulateGrad nodes -- bound to whatever stream first produced a
    gradient -- must stay out of the way."""
    with torch.no_grad():
        params = module._params()
        ctx = _Ctx(len(params), True)
        z, loss = _TokenizerFn.forward(ctx, module, x, *params)
        grads = module._backward(ctx.saved_tensors, torch.ones((), device=x.device, dtype=x.dtype))
    return z, loss, params, grads
