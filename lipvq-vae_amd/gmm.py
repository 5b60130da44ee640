"""The ICRT policy's GMM output head -- what the reference runs on the backbone output's last T positions (robomimic/models/
obs_nets.py:2602-2605): the ``ObservationDecoder``'s three Linears ``mean`` / ``scale`` / ``logits`` (obs_nets.py:747-771 with
the shapes of policy_nets.py:2507-2516), ``tanh``, ``softplus + min_std``, the ``Normal`` / ``Independent`` / ``Categorical`` /
``MixtureSameFamily`` objects and their ``log_prob`` (policy_nets.py:2545-2575, algo/icl.py:947), the NLL (icl.py:966) and
``.sample()`` (policy_nets.py:2599) -- on the HIP library (csrc/lipvq_gmm.hip).

``GMMActionHead`` owns the decoder's module tree (``nets.mean``, ``nets.scale``, ``nets.logits``: three ``nn.Linear`` created in
that order with torch's default init), so ``state_dict()`` keys, shapes and order and the RNG consumption of a seeded construction
are the reference's, and a checkpoint's ``policy.nets.decoder.*`` sub-dict loads with ``strict=True``.  The children are
parameter CONTAINERS only: no method calls them.  The compute is

    lipvq_gmm_head_f32        the three Linears as one fp32-MFMA product, then tanh / softplus / the mixture's log_prob (and the
                              NLL's deterministic sum: one more one-workgroup launch), or mean / scale / logits for a distribution
    lipvq_gmm_head_bwd_f32    the gradient of the [rows, P] pre-activations from the responsibilities, one launch
    lipvq_wgrad_f32, lipvq_linear_act_f32      the six parameter gradients and the input gradient
    lipvq_gmm_sample_f32      inverse-CDF mode choice + mu + sigma eps, one launch
    lipvq_gmm_sample_draw_f32 the same launch drawing u and eps itself (``set_sample_source("kernel")``), after one
                              lipvq_dropout_begin launch on the module's (seed, step) state

``set_matmul_precision("bf16" | "bf16x3")`` moves the three Linears onto the bf16 matrix pipe (the lipvq_gmm_*_mp_f32 entry points;
the gradients: lipvq_linear_nn_<mode>, lipvq_wgrad_<mode>), as the backbone's setter does for its Linears; the default is fp32.

``feats`` may be the non-contiguous view ``out[:, -T:]`` of a ``GPTBackbone`` output: its strides go to the kernel and the
forward makes no copy (the backward's wgrad reads a dense copy of those rows, and the input gradient comes back dense, in the
view's shape; autograd scatters it into the backbone output's gradient).  No kernel here uses float atomics: losses and gradients
repeat bit for bit.

Sampling: ``forward`` draws ``u`` / ``eps`` with ``torch.rand`` / ``torch.randn`` and picks the mode by inverse CDF, where the
reference's ``MixtureSameFamily.sample()`` draws a ``Categorical`` and a ``Normal`` sample for every mode and gathers: the actions
agree with the reference in distribution, not in bits.  Opt-in, ``set_sample_source("kernel")`` moves both draws into the sampling
launch (Philox4x32-10 and an fp32 inverse normal CDF; include/lipvq.h, "in-kernel sampling"), addressed by a per-environment
stream id instead of the batch position: no noise tensors, torch's generators untouched.  ``use_tanh=True`` (the TanhWrappedDistribution variant) is not implemented
(the ICRT configuration does not use it).
"""
from __future__ import annotations

import torch
import torch.distributions as D
import torch.nn as nn

from . import ops
from .nnfn import KernelFunction, KernelSampleSource, first_order_only, wants_backward
from .ops import GMM_EXP, GMM_LOW_NOISE, GMM_SOFTPLUS

__all__ = ["GMMActionHead"]


def _linear_grads(need_x, need_params, feats, gpre, Wm, Ws, Wl, MA, precision):
    """(gx in feats' shape, gWm, gbm, gWs, gbs, gWl, gbl) from gpre [N, P]: ops.head_linear_grads' results cut by rows."""
    gx, gW, gb = ops.head_linear_grads(need_x, need_params, feats, gpre, (Wm, Ws, Wl), precision)
    if gW is None:
        return (gx,) + (None,) * 6
    return gx, gW[:MA], gb[:MA], gW[MA:2 * MA], gb[MA:2 * MA], gW[2 * MA:], gb[2 * MA:]


class _LogProbFn(KernelFunction):
    """(log_prob [B, T], sum of log_prob or None) over lipvq_gmm_head_f32 / lipvq_gmm_head_bwd_f32."""

    @staticmethod
    def forward(ctx, feats, actions, Wm, bm, Ws, bs, Wl, bl, M, A, mode, min_std, want_sum, precision="fp32"):
        ctx.set_materialize_grads(False)
        keep = wants_backward(ctx)
        out = ops.gmm_head(feats, (Wm, bm, Ws, bs, Wl, bl), M, A, actions, mode, min_std, want_pre=keep, want_sum=want_sum,
                           precision=precision)
        if keep:
            ctx.cfg = (M, A, mode, min_std, precision)
            ctx.save_for_backward(feats, actions, out["pre"], Wm, Ws, Wl)
        lp = out["log_prob"].view(feats.shape[:-1])
        return lp, out.get("sum")

    @staticmethod
    @first_order_only
    def backward(ctx, glp, gsum):
        feats, actions, pre, Wm, Ws, Wl = ctx.saved_tensors
        M, A, mode, min_std, precision = ctx.cfg
        need = ctx.needs_input_grad                                 # (precision is optional: one gradient slot per argument given)
        if glp is None and gsum is None:
            return (None,) * len(need)
        gpre = ops.gmm_head_bwd(pre, actions, None if glp is None else glp.reshape(-1), gsum, M, A, mode, min_std)
        g = _linear_grads(need[0], any(need[2:8]), feats, gpre, Wm, Ws, Wl, M * A, precision)
        return ((g[0], None) + g[1:] + (None,) * 6)[:len(need)]


class _ParamsFn(KernelFunction):
    """(mean [B, T, M, A], scale [B, T, M, A], logits [B, T, M]) over lipvq_gmm_head_f32 / lipvq_gmm_params_bwd_f32."""

    @staticmethod
    def forward(ctx, feats, Wm, bm, Ws, bs, Wl, bl, M, A, mode, min_std, precision="fp32"):
        ctx.set_materialize_grads(False)
        keep = wants_backward(ctx)
        out = ops.gmm_head(feats, (Wm, bm, Ws, bs, Wl, bl), M, A, None, mode, min_std, want_pre=keep, want_params=True,
                           precision=precision)
        if keep:
            ctx.cfg = (M, A, mode, precision)
            ctx.save_for_backward(feats, out["pre"], Wm, Ws, Wl)
        lead = tuple(feats.shape[:-1])
        return out["mean"].view(lead + (M, A)), out["scale"].view(lead + (M, A)), out["logits"].view(lead + (M,))

    @staticmethod
    @first_order_only
    def backward(ctx, gmean, gscale, glogits):
        feats, pre, Wm, Ws, Wl = ctx.saved_tensors
        M, A, mode, precision = ctx.cfg
        need = ctx.needs_input_grad                                 # (precision is optional: one gradient slot per argument given)
        if gmean is None and gscale is None and glogits is None:
            return (None,) * len(need)
        gpre = ops.gmm_params_bwd(pre, gmean, gscale, glogits, M, A, mode)
        g = _linear_grads(need[0], any(need[1:7]), feats, gpre, Wm, Ws, Wl, M * A, precision)
        return ((g[0],) + g[1:] + (None,) * 5)[:len(need)]


class GMMActionHead(KernelSampleSource, nn.Module):
    """The GMM head of the reference's ``ICL_MIMO_Transformer_GMM`` (policy_nets.py:2507-2599) on the HIP library.

    ``log_prob`` / ``nll`` are the training path (icl.py:916-966: ``forward_train(..., low_noise_eval=False).log_prob``, then
    ``-log_probs.mean()``), ``forward_train`` returns the reference's distribution object built from kernel-produced tensors, and
    ``forward`` samples actions.  ``set_sample_source("kernel")`` (nnfn.KernelSampleSource) makes the sampling launch draw its
    own noise, addressed by per-environment stream ids (``forward``'s ``streams``)."""

    MAX_MODES, MAX_AC_DIM, MAX_COLUMNS, MAX_EMBED = 16, 64, 512, 1024
    _MODES = {"softplus": GMM_SOFTPLUS, "exp": GMM_EXP}

    def __init__(self, embed_dim, ac_dim, num_modes=5, min_std=0.01, std_activation="softplus", low_noise_eval=True, use_tanh=False):
        super().__init__()
        if use_tanh:
            raise NotImplementedError("GMMActionHead: use_tanh=True (TanhWrappedDistribution) is not implemented on the HIP path "
                                      "(the ICRT configuration does not use it)")
        if std_activation not in self._MODES:
            raise ValueError(f"GMMActionHead: unknown std_activation {std_activation!r} (softplus or exp)")
        if not 1 <= num_modes <= self.MAX_MODES or not 1 <= ac_dim <= self.MAX_AC_DIM:
            raise ValueError(f"GMMActionHead: 1 <= num_modes <= {self.MAX_MODES} and 1 <= ac_dim <= {self.MAX_AC_DIM} "
                             f"(got {num_modes}, {ac_dim})")
        if num_modes * (2 * ac_dim + 1) > self.MAX_COLUMNS:
            raise ValueError(f"GMMActionHead: num_modes (2 ac_dim + 1) = {num_modes * (2 * ac_dim + 1)} output columns exceed {self.MAX_COLUMNS}")
        if embed_dim <= 0 or embed_dim % 4 != 0 or embed_dim > self.MAX_EMBED:
            raise ValueError(f"GMMActionHead: embed_dim={embed_dim} must be a multiple of 4, <= {self.MAX_EMBED}")
        self.embed_dim = embed_dim
        self.ac_dim = ac_dim
        self.num_modes = num_modes
        self.min_std = min_std
        self.std_activation = std_activation
        self.low_noise_eval = low_noise_eval
        self.use_tanh = use_tanh
        self.nets = nn.ModuleDict()                                 # ObservationDecoder._create_layers: mean, scale, logits in this order
        self.nets["mean"] = nn.Linear(embed_dim, num_modes * ac_dim)
        self.nets["scale"] = nn.Linear(embed_dim, num_modes * ac_dim)
        self.nets["logits"] = nn.Linear(embed_dim, num_modes)
        self._matmul_precision = "fp32"

    @property
    def matmul_precision(self) -> str:
        """"fp32" (default), "bf16" or "bf16x3": how the head's three Linears multiply (set_matmul_precision)."""
        return self._matmul_precision

    def set_matmul_precision(self, precision: str) -> "GMMActionHead":
        """"bf16" / "bf16x3": the head's three Linears -- in ``forward`` (both noise sources), ``log_prob``, ``nll`` and
        ``forward_train``, and their gradients in the backward -- run on the bf16 matrix pipe by ``GPTBackbone.
        set_matmul_precision``'s rules: operands rounded to bf16 (nearest even; "bf16x3": split into hi + lo, three products) as the
        kernel reads them, fp32 accumulation, every tensor fp32; the pre-activations have the bits of ``ops.linear_bf16`` /
        ``ops.linear_bf16x3``, and everything after them is the fp32 code.  "fp32" restores the default bit for bit.  The bf16
        modes need embed_dim % 8 == 0.  Not part of state_dict(); a captured graph keeps the mode it was captured in; returns self."""
        ops._matmul_mode("GMMActionHead", precision, self.embed_dim)
        self._matmul_precision = precision
        return self

    def _params(self):
        n = self.nets
        return (n["mean"].weight, n["mean"].bias, n["scale"].weight, n["scale"].bias, n["logits"].weight, n["logits"].bias)

    def _mode(self, low_noise_eval):
        """policy_nets.py:2553-2560: low noise only when the flag is set AND the module is in eval mode."""
        if low_noise_eval is None:
            low_noise_eval = self.low_noise_eval
        return GMM_LOW_NOISE if (low_noise_eval and not self.training) else self._MODES[self.std_activation]

    def _check(self, feats, actions=None):
        if not feats.is_cuda:
            raise RuntimeError("GMMActionHead runs on the HIP library only (no CPU path)")
        if feats.dim() != 3 or feats.shape[-1] != self.embed_dim:
            raise ValueError(f"GMMActionHead: feats must be [B, T, {self.embed_dim}], got {tuple(feats.shape)}")
        if actions is not None and tuple(actions.shape) != tuple(feats.shape[:2]) + (self.ac_dim,):
            raise ValueError(f"GMMActionHead: actions must be {tuple(feats.shape[:2]) + (self.ac_dim,)}, got {tuple(actions.shape)}")
        return feats if feats.dtype == torch.float32 else feats.float()

    def _log_prob(self, feats, actions, low_noise_eval, want_sum):
        feats = self._check(feats, actions)
        return _LogProbFn.apply(feats, actions.detach().float(), *self._params(), self.num_modes, self.ac_dim,
                                self._mode(low_noise_eval), float(self.min_std), want_sum, self._matmul_precision)

    def log_prob(self, feats, actions, low_noise_eval=False):
        """log-likelihood [B, T] of actions [B, T, A] under the mixture (icl.py:916-947; the training path passes low_noise_eval=False)."""
        return self._log_prob(feats, actions, low_noise_eval, False)[0]

    def nll(self, feats, actions, low_noise_eval=False):
        """-log_prob.mean() (icl.py:966) from the kernel's deterministic sum: the same bits on every run."""
        feats = self._check(feats, actions)
        rows = feats.shape[0] * feats.shape[1]
        return -self._log_prob(feats, actions, low_noise_eval, True)[1] / rows

    def forward_train(self, feats, low_noise_eval=None):
        """The reference's distribution object (policy_nets.py:2545-2575) over kernel-produced mean / scale / logits, with
        autograd through them; batch_shape [B, T], event_shape [A]."""
        feats = self._check(feats)
        mean, scale, logits = _ParamsFn.apply(feats, *self._params(), self.num_modes, self.ac_dim, self._mode(low_noise_eval),
                                              float(self.min_std), self._matmul_precision)
        component = D.Independent(D.Normal(loc=mean, scale=scale), 1)
        return D.MixtureSameFamily(mixture_distribution=D.Categorical(logits=logits), component_distribution=component)

    def forward(self, feats, u=None, eps=None, streams=None):
        """Sampled actions [B, T, A] (policy_nets.py:2593-2599).  u [B, T] uniform in [0, 1) picks each row's mode by inverse CDF
        over softmax(logits), eps [B, T, A] standard normal is the component's noise; both are drawn on feats' device when not
        given.  In eval mode with low_noise_eval the scale is 1e-4.  The actions agree with the reference's ``.sample()`` in
        distribution, not in bits (see the module docstring).  No host synchronisation: capturable by nnfn.GraphedEval.

        Under ``set_sample_source("kernel")`` (eval and train mode alike) a call without u and eps makes one ``dropout_begin``
        launch on ``sample_state`` and one sampling launch that draws the noise itself (include/lipvq.h, "in-kernel sampling"):
        batch entry b draws from stream ``streams[b]`` (int64 [B] on feats' device; None: b itself), so an environment's noise
        follows its id through any re-packing of the batch.  With u AND eps given they are used as they are, row by position, and
        the state is not advanced; exactly one of them is a ValueError.  The "torch" source only validates streams' shape."""
        feats = self._check(feats)
        B, T = feats.shape[:2]
        if streams is not None and (not isinstance(streams, torch.Tensor) or streams.dtype != torch.int64 or tuple(streams.shape) != (B,)):
            raise ValueError(f"GMMActionHead: streams must be an int64 [{B}] tensor (one stream id per batch entry)")
        if self.sample_source == "kernel" and (u is None or eps is None):
            if u is not None or eps is not None:
                raise ValueError("GMMActionHead: under the kernel sample source give both u and eps (explicit noise) or neither "
                                 "(the launch draws both)")
            with torch.no_grad():
                act = ops.gmm_sample_draw(feats.detach(), tuple(p.detach() for p in self._params()), self.num_modes, self.ac_dim,
                                          self._sample_begin(feats.device), streams, self._mode(None), float(self.min_std),
                                          self._matmul_precision)
            return act.view(B, T, self.ac_dim)
        if u is None:
            u = torch.rand((B, T), device=feats.device, dtype=torch.float32)
        if eps is None:
            eps = torch.randn((B, T, self.ac_dim), device=feats.device, dtype=torch.float32)
        with torch.no_grad():
            act = ops.gmm_sample(feats.detach(), tuple(p.detach() for p in self._params()), self.num_modes, self.ac_dim, u, eps,
                                 self._mode(None), float(self.min_std), self._matmul_precision)
        return act.view(B, T, self.ac_dim)
