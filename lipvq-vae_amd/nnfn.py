"""What the transformer-style modules (embedding.py, default_branch.py, gpt.py) share: Linear and residual + LayerNorm as
``torch.autograd.Function``s over the library's kernels, and the eval-forward HIP-graph wrapper."""
from __future__ import annotations

import functools
import threading

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .capture import capture, copy_in, warm_up
from .ops import ACT_NONE

__all__ = ["LinearFn", "AddLayerNormFn", "GraphedEval", "KernelDropoutSource", "KernelSampleSource", "KernelFunction",
           "first_order_only", "wants_backward"]

_applying = threading.local()


class KernelFunction(torch.autograd.Function):
    """Base of the library's Functions.  ``forward`` always runs with grad mode off and ``ctx.needs_input_grad`` repeats the inputs'
    ``requires_grad`` whatever the caller's grad mode was, so a forward cannot tell a ``torch.no_grad()`` call of a trainable
    module from a training call: ``apply`` notes the caller's grad mode for ``wants_backward``."""

    @classmethod
    def apply(cls, *args):
        prev = getattr(_applying, "grad_mode", True)
        _applying.grad_mode = torch.is_grad_enabled()
        try:
            return super().apply(*args)
        finally:
            _applying.grad_mode = prev


def wants_backward(ctx) -> bool:
    """In ``forward``: will a backward of this call ever run?  No under ``torch.no_grad()`` and no when no input requires a
    gradient: then nothing is written or kept for it (no pre-activations, LayerNorm statistics, saved tensors)."""
    return getattr(_applying, "grad_mode", True) and any(ctx.needs_input_grad)


def first_order_only(backward):
    """The decorator of every ``backward`` of the library: ``torch.autograd.function.once_differentiable``, closed where that one
    is open.  The backward kernels return tensors without a graph, so a gradient of a gradient does not exist.  torch's decorator
    makes a second differentiation raise only when an upstream gradient itself requires a gradient; under ``create_graph=True``
    with a constant upstream gradient (``out.sum()``, any scalar loss) it hands the graph-less tensors on, and a loss that adds a
    function of such a gradient to an ordinary term would train on the ordinary term alone, silently.  Here every gradient that
    leaves a backward run under ``create_graph=True`` hangs on an error node: differentiating through it raises ``RuntimeError``.
    A first-order backward (grad mode off inside the engine) returns what the wrapped function returned, untouched."""
    inner = once_differentiable(backward)

    @functools.wraps(backward)
    def wrapper(ctx, *grads):
        outputs = inner(ctx, *grads)
        if not torch.is_grad_enabled():
            return outputs
        outs = outputs if isinstance(outputs, tuple) else (outputs,)
        tensors = [o for o in outs if isinstance(o, torch.Tensor)]
        if not tensors or any(o.requires_grad for o in tensors):      # nothing to guard, or once_differentiable's error node is there already
            return outputs
        err = torch._C._functions.DelayedError(
            b"lipvq: this function's backward runs graph-less HIP kernels and is differentiable once only "
            b"(first_order_only): a gradient computed under create_graph=True cannot be differentiated again", len(outs))
        guarded = err(*[None if o is None else o.detach().requires_grad_(True) for o in outs])
        return guarded if isinstance(outputs, tuple) else guarded[0]

    wrapper.first_order_only = True
    return wrapper


class LinearFn(KernelFunction):
    """act(x W^T + b) over the last dimension, b optional; backward = act' (elementwise), one more Linear (gx), the wgrad kernel.
    precision="bf16": the three matrix products run on the bf16 matrix pipe (ops.linear_bf16 / linear_nn_bf16 / wgrad_bf16:
    operands rounded to bf16 as they are read, fp32 accumulation, fp32 tensors); precision="bf16x3": the same pipe with every
    operand split into two bf16 numbers and three products per product (ops.linear_bf16x3 / linear_nn_bf16x3 / wgrad_bf16x3);
    act' stays the fp32 kernel.
    dropout=(snap, site, p) of the in-kernel source (fp32 only): the result is act(x W^T + b) * m, decided in the Linear's epilogue
    over the rows and columns of the 2-D result.  No mask is saved: the backward's first launch forms act'(pre) (gy m) from the
    regenerated decisions (ops.act_bwd with dropout), whatever act is."""

    @staticmethod
    def forward(ctx, x, W, b, act, precision="fp32", dropout=None):
        if precision not in ("fp32", "bf16", "bf16x3"):
            raise ValueError(f"LinearFn: precision must be 'fp32', 'bf16' or 'bf16x3', got {precision!r}")
        if dropout is not None and precision != "fp32":
            raise ValueError(f"LinearFn: dropout (the in-kernel source) has fp32 kernels only, got precision {precision!r}")
        ctx.act, ctx.has_bias, ctx.shape, ctx.pipe = act, b is not None, x.shape, ("" if precision == "fp32" else "_" + precision)
        ctx.dropout = dropout
        linear = getattr(ops, "linear" + ctx.pipe)
        x2 = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])      # (2-D callers: no view objects on their host-bound paths)
        if not wants_backward(ctx):                            # eval / no_grad: no pre-activation is written, nothing is kept
            y = linear(x2, W, b, act=act, dropout=dropout)
        elif act != ACT_NONE:
            y, pre = linear(x2, W, b, act=act, save_pre=True, dropout=dropout)
            ctx.save_for_backward(x2, W, pre)
        else:
            y = linear(x2, W, b, dropout=dropout)
            ctx.save_for_backward(x2, W)
        return y if x.dim() == 2 else y.view(*x.shape[:-1], W.shape[0])

    @staticmethod
    @first_order_only
    def backward(ctx, gy):
        gy = gy.reshape(-1, gy.shape[-1]).contiguous()
        if ctx.act != ACT_NONE:
            x2, W, pre = ctx.saved_tensors
        else:
            (x2, W), pre = ctx.saved_tensors, None
        if pre is not None or ctx.dropout is not None:
            gy = ops.act_bwd(gy, pre, ctx.act, dropout=ctx.dropout)
        gx = gW = gb = None
        if ctx.needs_input_grad[0]:
            gx = (getattr(ops, "linear_nn" + ctx.pipe)(gy, W) if ctx.pipe else ops.linear(gy, W.t().contiguous())).view(ctx.shape)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gW, gb = getattr(ops, "wgrad" + ctx.pipe)(gy, x2, want_bias=ctx.has_bias)
        return gx, gW, gb, None, None, None


class AddLayerNormFn(KernelFunction):
    """(s, y) = (a + b, LayerNorm(a + b) w + bias), b optional; s is None unless want_s (a post-norm residual and the closing
    LayerNorm of a pre-norm stack discard it, and without b the caller keeps using a).  Backward: the gradient of a and of b is
    LayerNorm's plus the gradient that arrives for s (the residual stream), added inside the kernel.
    dropout=(snap, site, p) of the in-kernel source: (s, y) = (a + drop(b), LayerNorm(a + drop(b)) w + bias), the branch's dropout
    decided inside the launch.  No mask is saved: the backward launch regenerates the decisions from snap and writes the gradient
    of a (LayerNorm's plus the stream's) and that of b (the same times the mask factor) itself."""

    @staticmethod
    def forward(ctx, a, b, w, bias, eps, want_s, dropout=None):
        ctx.set_materialize_grads(False)
        ctx.has_b, ctx.dropout = b is not None, dropout
        if not wants_backward(ctx):                            # eval / no_grad: nothing is kept for a backward
            return ops.gpt_layernorm(a, b, w, bias, eps, want_s=want_s, dropout=dropout)
        s, y, xhat, rstd = ops.gpt_layernorm(a, b, w, bias, eps, want_s=want_s, save=True, dropout=dropout)
        ctx.save_for_backward(xhat, rstd, w)
        return s, y

    @staticmethod
    @first_order_only
    def backward(ctx, gs, gy):
        if ctx.dropout is None:                                # a and b share one gradient tensor
            if gy is None:
                return gs, (gs if ctx.has_b else None), None, None, None, None, None
            xhat, rstd, w = ctx.saved_tensors
            g, gw, gb = ops.gpt_layernorm_bwd(gy.contiguous(), xhat, rstd, w, None if gs is None else gs.contiguous())
            return g, (g if ctx.has_b else None), gw, gb, None, None, None
        xhat, rstd, w = ctx.saved_tensors
        if gy is None and gs is None:
            return (None,) * 7
        if gy is None:                                         # only s was used: LayerNorm's part is that of a zero gradient
            gy = torch.zeros_like(xhat)
        g, gbr, gw, gb = ops.gpt_layernorm_bwd(gy.contiguous(), xhat, rstd, w, None if gs is None else gs.contiguous(),
                                               dropout=ctx.dropout)
        need = ctx.needs_input_grad
        return (g if need[0] else None, gbr if need[1] else None, gw if need[2] else None, gb if need[3] else None,
                None, None, None)


class _SourceState:
    """The (seed, step) state of an in-kernel random source, kept on the host module as the non-persistent buffer
    ``_{word}_state`` beside the attribute ``_{word}_source``: what KernelDropoutSource (word "dropout") and KernelSampleSource
    (word "sample") share.  ``reseed`` names the module's reseeding method, ``noun`` the state in the device message, and
    ``owner(module)`` gives the class name the messages carry."""

    def __init__(self, word, reseed, noun, owner):
        self.word, self.reseed, self.noun, self.owner = word, reseed, noun, owner
        self.state_attr, self.source_attr = f"_{word}_state", f"_{word}_source"

    def set_source(self, mod, source, seed):
        """Create-on-first-"kernel": nothing exists before it, a later call with a seed reseeds (step 0), one without leaves it."""
        if source not in ("torch", "kernel"):
            raise ValueError(f"{self.owner(mod)}: {self.word} source must be 'torch' or 'kernel', got {source!r}")
        if source == "kernel":
            if getattr(mod, self.state_attr, None) is None:
                dev = next(mod.parameters()).device
                mod.register_buffer(self.state_attr, torch.zeros(2, dtype=torch.int64, device=dev), persistent=False)
                getattr(mod, self.reseed)(torch.initial_seed() if seed is None else seed)
            elif seed is not None:
                getattr(mod, self.reseed)(seed)
        setattr(mod, self.source_attr, source)
        return mod

    def reseed_state(self, mod, seed, step):
        state = getattr(mod, self.state_attr, None)
        if state is None:
            raise RuntimeError(f"{self.owner(mod)}.{self.reseed}: call set_{self.word}_source('kernel') first (it creates the state)")
        words = [int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)]
        words = [v - 2 ** 64 if v >= 2 ** 63 else v for v in words]          # (the bit pattern, as int64)
        state.copy_(torch.tensor(words, dtype=torch.int64))
        return mod

    def begin(self, mod, device):
        """The snap of one call: one dropout_begin launch on the module's own state."""
        state = getattr(mod, self.state_attr)
        if state.device != device:
            raise RuntimeError(f"{self.owner(mod)}: the {self.noun} state is not on the input's device (move the module with .to())")
        return ops.dropout_begin(state)


_DROPOUT_STATE = _SourceState("dropout", "reseed_dropout", "dropout", lambda mod: mod._dropout_owner())
_SAMPLE_STATE = _SourceState("sample", "reseed_sampling", "sampling", lambda mod: type(mod).__name__)


class KernelDropoutSource:
    """Mixin of the modules with training-mode dropout (GPTBackbone, ICLInputEmbedding, DefaultActionNetwork): where the decisions
    come from, and the state of the in-kernel source.  The host class is an ``nn.Module``; nothing is created at construction
    (the attributes are looked up with defaults), so a seeded construction consumes torch's RNG exactly as without the mixin."""

    DROPOUT_OWNER = None        # the class name the messages carry; a subclass keeps its base's texts unless it sets its own

    def _dropout_owner(self) -> str:
        return self.DROPOUT_OWNER or type(self).__name__

    @property
    def dropout_source(self) -> str:
        """"torch" (default) or "kernel": where training-mode dropout decisions come from (set_dropout_source)."""
        return getattr(self, "_dropout_source", "torch")

    def set_dropout_source(self, source: str, seed: int | None = None):
        """"kernel": every training-mode dropout of the module is decided inside the HIP kernels that touch those elements, each
        decision a pure function of (seed, step, site, row, col) (include/lipvq.h, "in-kernel dropout"; the module's docstring
        lists its sites).  No mask tensor is drawn, stored or saved for the backward, and torch's generators are not touched.  A
        training-mode forward makes one ``ops.dropout_begin`` launch, which hands the call its (seed, step) and advances the step
        on the device -- also under ``torch.no_grad()`` and inside a captured graph, where every replay advances it.  "torch"
        restores the default (masks from torch's generator) bit for bit.  Eval mode ignores the source.

        The state, ``dropout_state`` -- a device int64[2] tensor (seed, step) --, is created by the first call with "kernel" (never
        at construction: a seeded construction consumes torch's RNG exactly as before), seeded with ``seed`` or, for None,
        ``torch.initial_seed()``; a later call with a seed reseeds it (step 0), one without leaves it.  It is a non-persistent
        buffer: ``.to()`` moves it, ``state_dict()`` does not hold it.  Each module owns its state; the sites of different
        modules differ, so equal (seed, step) pairs still give unrelated fields.  Returns self."""
        return _DROPOUT_STATE.set_source(self, source, seed)

    @property
    def dropout_state(self):
        """The device int64[2] tensor (seed, step) of the in-kernel source, None before the first set_dropout_source("kernel").
        Pass it to ``icl.GraphedPolicyStep(..., extra_state=[net.dropout_state])`` so that the warm-up steps do not advance it."""
        return getattr(self, "_dropout_state", None)

    def reseed_dropout(self, seed: int, step: int = 0):
        """Set the in-kernel source's (seed, step) in place: seed any integer (taken modulo 2^64), step the next forward's."""
        return _DROPOUT_STATE.reseed_state(self, seed, step)

    def _kernel_dropout(self) -> bool:
        """Is this call's dropout the in-kernel source's?  (Training mode only: eval ignores the source.)"""
        return self.training and getattr(self, "_dropout_source", "torch") == "kernel"

    def _dropout_begin(self, device):
        """The snap of one training forward: one dropout_begin launch on the module's own state."""
        return _DROPOUT_STATE.begin(self, device)

    def _dropout_p(self, p, what) -> float:
        p = float(p)
        if p >= 1.0:
            raise ValueError(f"{self._dropout_owner()}: {what} p={p} under the kernel dropout source (0 <= p < 1)")
        return p


class KernelSampleSource:
    """Mixin of the modules that SAMPLE (GMMActionHead): where the sampling noise comes from, and the state of the in-kernel
    source.  The state holder, its rules and its error types are KernelDropoutSource's (_SourceState); unlike dropout, sampling is
    not a training-only act, so the source applies in eval and in train mode.  Nothing is created at construction."""

    @property
    def sample_source(self) -> str:
        """"torch" (default) or "kernel": where the sampling noise comes from (set_sample_source)."""
        return getattr(self, "_sample_source", "torch")

    def set_sample_source(self, source: str, seed: int | None = None):
        """"kernel": the sampling launch draws its own uniform and normals, each a pure function of (seed, step, site, stream id,
        t, component) (include/lipvq.h, "in-kernel sampling").  No noise tensor is drawn or stored and torch's generators are not
        touched.  A sampling call makes one ``ops.dropout_begin`` launch, which hands the call its (seed, step) and advances the
        step on the device -- also under ``torch.no_grad()`` and inside a captured graph, where every replay advances it.
        "torch" restores the default (``torch.rand`` / ``torch.randn``) bit for bit.

        The state, ``sample_state`` -- a device int64[2] tensor (seed, step) --, is created by the first call with "kernel" (never
        at construction), seeded with ``seed`` or, for None, ``torch.initial_seed()``; a later call with a seed reseeds it
        (step 0), one without leaves it.  It is a non-persistent buffer: ``.to()`` moves it, ``state_dict()`` does not hold it.
        Returns self."""
        return _SAMPLE_STATE.set_source(self, source, seed)

    @property
    def sample_state(self):
        """The device int64[2] tensor (seed, step) of the in-kernel source, None before the first set_sample_source("kernel")."""
        return getattr(self, "_sample_state", None)

    def reseed_sampling(self, seed: int, step: int = 0):
        """Set the in-kernel source's (seed, step) in place: seed any integer (taken modulo 2^64), step the next sampling call's."""
        return _SAMPLE_STATE.reseed_state(self, seed, step)

    def _sample_begin(self, device):
        """The snap of one sampling call: one dropout_begin launch on the module's own state."""
        return _SAMPLE_STATE.begin(self, device)


def _sample_states(net):
    """The in-kernel sampling states of net and its sub-modules (KernelSampleSource), those that exist."""
    states = [getattr(m, "sample_state", None) for m in net.modules()]
    return [s for s in states if isinstance(s, torch.Tensor)]


class GraphedEval:
    """Eval-mode forward of ``net`` captured in ONE HIP graph for the shape of ``example``.  Parameters are read at replay time
    through their storage, so in-place updates (optimizer steps, load_state_dict) are seen; re-capture after anything that
    REPLACES a parameter tensor (.to(), .cuda()).  The returned tensor is the graph's own output buffer: copy it before the next
    call if it must survive.  A net that samples from the in-kernel source (KernelSampleSource) keeps its ``sample_state``: the
    warm-up and the capture do not advance it, and every replay does, so replay k draws what eager call k would."""

    def __init__(self, net: torch.nn.Module, example: torch.Tensor, /):
        if net.training:
            raise RuntimeError(f"{type(self).__name__} captures the eval-mode forward: call net.eval() first")
        self.net = net
        self._x = example.detach().contiguous().float().clone()
        states = _sample_states(net)
        kept = [s.clone() for s in states]
        with torch.no_grad():
            warm_up(lambda: net(self._x), 3, self._x.device)      # first-use work (LDS reservations, lazy module state) stays out of the capture
            self._graph, self._y = capture(lambda: net(self._x))
            for s, k in zip(states, kept):
                s.copy_(k)

    def __call__(self, inputs: torch.Tensor, /) -> torch.Tensor:
        copy_in(self._x, inputs, "captured")
        self._graph.replay()
        return self._y
