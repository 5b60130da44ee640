"""Drop-in replacements for the reference's action tokenizers, running on the HIP library.

``LLFQVAE_V4``  mirrors robomimic/models/vq_vae/backbone_lfqvae_v5.py:51-84 (the paper's
                LipVQ-VAE): same constructor signature and defaults, same 14 ``state_dict``
                keys/shapes/dtypes, same RNG consumption at construction (so the same
                ``torch.manual_seed`` gives the same initial weights), and
                ``forward(x[N,A]) -> (z_latent[N,D] without grad, loss 0-dim with grad_fn)``.
``VQVAE``       mirrors robomimic/models/vq_vae/backbone.py:6-76 (ReLU stacks, squared-L2
                argmin, commitment 0.25, straight-through estimator).

The ``nn.Linear`` / container sub-modules exist only to own the parameters under the
reference's names; they are never called.  All arithmetic is issued through
``lipvq_vae_amd.ops`` (C ABI -> hand-written gfx950 kernels).  Gradients are produced by the
library's backward kernels through one ``torch.autograd.Function`` for both variants, so
``loss.backward(); AdamW.step()`` in the ICRT loop (robomimic/algo/icl.py:885-889,968-970)
works unchanged.

Extras that the reference does not have (allowed by SURVEY.md section 8b): ``last_indices``,
``code_usage`` (int64 [K], accumulated over forwards), ``tokenize()`` (encode + quantize
only: the BASELINE metric's path) and ``perplexity()``; opt-in, never called by ``forward()``: ``init_codebook_()`` and
``revive_dead_codes_()`` (kmeans.py).
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn as nn

from . import ops
from .backward import llfq_backward, vq_backward
from .derived import _PackCache, mark_written  # noqa: F401  (_PackCache: embedding.py, binning.py and tests import it from here)
from .ops import ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, DIST_NORM, DIST_SQSUM

__all__ = ["LLFQVAE_V4", "VQVAE", "LipschitzMLP", "LFQQuantizer"]


class LipschitzMLP(nn.Module):
    """Parameter holder of the Lipschitz latent layer (reference v5:15-24): W ~ N(0,1), b = 0, ci = 1."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.W = nn.Parameter(torch.randn(out_dim, in_dim))
        self.b = nn.Parameter(torch.zeros(out_dim))
        self.ci = nn.Parameter(torch.ones(out_dim))

    def normalized_weight(self):
        """(scale[D], W_norm[D,H]) = normalization(W, ci) of v5:6-12, computed on the GPU."""
        return ops.lipschitz_scale(self.W.detach(), self.ci.detach())


class LFQQuantizer(nn.Module):
    """Parameter holder of the codebook (reference v5:27-35): randn then kaiming_uniform_."""

    def __init__(self, num_codes, code_dim):
        super().__init__()
        self.num_codes = num_codes
        self.code_dim = code_dim
        self.codebook = nn.Parameter(torch.randn(num_codes, code_dim))
        nn.init.kaiming_uniform_(self.codebook)

    def forward(self, z_e):
        """(z_q, indices) of v5:37-48 for callers that use the quantizer on its own (no grad)."""
        idx, zq, _ = ops.nearest(z_e.detach(), self.codebook.detach(), DIST_NORM)
        return zq, idx


class _ScreenMonitor:
    """Keeps the certified screen from being used where it does not pay, without ever synchronising.

    The screen hands the rows it cannot certify to the exact kernel.  With trained parameters that is a fraction of a percent;
    with a DEGENERATE codebook -- the reference's own default initialisation maps every row to one code, a
    collapsed training run does the same -- it is (almost) every row, and the exact kernel, built for a few thousand rows with
    short candidate lists, would scan the whole codebook for each of them: orders of magnitude slower than the all-pairs exact
    kernel (results are the same on every route).  So after each screened call the uncertified-row count (workspace[0]) is
    copied to pinned host memory asynchronously; the NEXT call looks at it only if the copy's event has already completed
    (``event.query()``: never a wait).  A fraction above ``THRESHOLD`` routes the following ``PROBE_EVERY`` large-batch calls
    through the all-pairs kernel, then the screen is tried again."""

    THRESHOLD = 1.0 / 16.0        # three-product screen: a fraction of a percent is normal
    THRESHOLD_COARSE = 0.6        # one-product screen: 10-40 % of the rows go to the exact stage BY DESIGN (lipvq_screen_is_coarse)
    PROBE_EVERY = 16

    def __init__(self):
        self.reset()

    def reset(self):
        """Forget every reading (a new codebook; a graph capture that must not inherit its warm-up steps' readings)."""
        self._pending = None
        self.bypass_calls = 0
        self.last_fraction = None

    def __deepcopy__(self, memo):
        return type(self)()          # (a pending reading holds an event, which cannot be copied, and is the original's anyway)

    ENABLED = True                # tests / measurements: False = always the screen (class attribute; no environment variable)

    def use_screen(self) -> bool:
        if not _ScreenMonitor.ENABLED:
            return True
        if torch.cuda.is_current_stream_capturing():
            # a graph capture records ONE route and no host decision can run at replay: take the route the last eager reading
            # chose (a codebook that was sending every row to the exact stage keeps the all-pairs kernel in the graph too)
            return self.bypass_calls <= 0
        if self._pending is not None:
            ev, host, n, coarse = self._pending
            if ev.query():
                self.last_fraction = float(host[0]) / max(1, n)
                self._pending = None
                if self.last_fraction > (self.THRESHOLD_COARSE if coarse else self.THRESHOLD):
                    self.bypass_calls = self.PROBE_EVERY
        if self.bypass_calls > 0:
            self.bypass_calls -= 1
            return False
        return True

    def record(self, ws: torch.Tensor, n: int, coarse: bool = False) -> None:
        if torch.cuda.is_current_stream_capturing() or self._pending is not None:
            return
        host = torch.empty(1, dtype=torch.int32, pin_memory=True)
        host.copy_(ws[:1], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending = (ev, host, int(n), bool(coarse))


# The encoder + quantizer routes of a call (identical results on every one):
FUSED = "fused"            # encoder + screen in ONE persistent launch (csrc/lipvq_fused.hip), z_e never re-read
ROWS = "rows"              # mlp3, then the exact kernel on every row (no prepared codebook)
SCREENED = "screened"      # mlp3, then the stand-alone MFMA screen + exact re-scoring of the rows it cannot certify
ALL_PAIRS = "all_pairs"    # mlp3, then the all-pairs exact kernel


class _Plan(NamedTuple):
    """What _TokenizerBase._plan decided for one call."""
    route: str             # FUSED | ROWS | SCREENED | ALL_PAIRS
    keep: str | None       # what the encoder stage hands back besides (idx, z_q): "pre" (z_e + the three pre-activations a
    #                        training step saves), "ze" (z_e, for the loss) or None
    fast: bool             # the fused launch runs the encoder's GEMMs on fp16 MFMAs (tokenize(mode="fast"))
    fold_loss: bool        # the decoder launch sums both squared errors itself (mlp3_loss) instead of mlp3 + mse_pair_loss


class _TokenizerBase(nn.Module):
    """What the two tokenizers share: derived buffers, codebook maintenance and the ROUTING POLICY (_plan), with everything that
    differs between them as class data: _DIST, the activation triples, the loss form, the thresholds below."""

    # rows up to which every row is decided by the exact kernel, without a prepared codebook or a screen launch: measured
    # (scripts/measure_quantize_small.py, K = 1024) exact rows vs screen [+ codebook preparation]: D = 208: 36 vs 75 [+69] us at
    # N = 80, 74 vs 122 [+69] at 2048, 143 vs 89 [+69] at 4096
    EXACT_ROWS_MAX = 2048
    SCREEN_MIN_CODES = 0          # codebook size from which the stand-alone screen is a route at all
    FUSED_MIN_CODES = 0           # ... and the fused launch
    FUSED_SMALL_TOKENIZE = False  # tokenize() takes the fused launch up to EXACT_ROWS_MAX rows too (forward() never does)

    def _init_extras(self, K):
        self._screen_monitor = _ScreenMonitor()
        self.register_buffer("code_usage", torch.zeros(K, dtype=torch.int64), persistent=False)
        self.last_indices = None
        self._enc_cache = _PackCache()
        self._dec_cache = _PackCache()
        self._cb_cache = _PackCache()
        self._enc16_cache = _PackCache()
        self._tok_ws, self._tok_ws_key = None, None
        self.last_exact_rows = None      # int32 device tensor: element 0 = rows the screen could not certify

    def reset_usage(self):
        self.code_usage.zero_()

    # -- derived buffers (packed weights, prepared codebook, fused-launch workspace) -------------------
    def invalidate_caches(self):
        """Drop everything derived from the parameters; the next call rebuilds it.  Needed after a write the version
        counter does not see (see derived.stamp); cheap (a few small launches on the next forward)."""
        for c in (self._enc_cache, self._dec_cache, self._cb_cache, self._enc16_cache):
            c.invalidate()
        self._tok_ws, self._tok_ws_key = None, None

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_caches()
        return out

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        if hasattr(self, "_enc_cache"):
            self.invalidate_caches()
        return out

    def train(self, mode: bool = True):
        out = super().train(mode)
        if hasattr(self, "_enc_cache"):
            self.invalidate_caches()
        return out

    def _packed_decoder(self):
        return self._dec_cache.get(self._dec_params(), lambda: ops.mlp3_pack(*(t.detach() for t in self._dec_params())))

    def _enc_packed(self):
        """The packed encoder stack alone (LLFQVAE_V4._packed_encoder returns the Lipschitz scale and W_norm with it)."""
        p = self._packed_encoder()
        return p[0] if isinstance(p, tuple) else p

    # -- opt-in codebook maintenance (extensions, not reference behaviour: kmeans.py) -------------------
    def _codebook_written(self):
        """After an in-place write through a raw pointer: bump the version (autograd's saved-tensor checks), drop the prepared
        codebook and the fused workspace, and forget what the screen monitor learnt about the OLD codebook (a collapsed one sets
        its all-pairs bypass)."""
        mark_written((self._codebook(),))
        self.invalidate_caches()
        self._screen_monitor.reset()

    @torch.no_grad()
    def init_codebook_(self, x, iters: int = 10, generator=None, seed_rows=None):
        """Data-dependent codebook initialisation: k-means++ seeding on the encoder outputs of x, then ``iters`` Lloyd steps
        (kmeans.kmeans, with this tokenizer's distance rule).  Writes the codebook in place; returns self."""
        from .kmeans import kmeans
        z = self.encode(x)
        kmeans(z, self._codebook().detach(), iters=iters, generator=generator, dist=self._DIST, seed_rows=seed_rows)
        self._codebook_written()
        return self

    @torch.no_grad()
    def revive_dead_codes_(self, x, threshold: int = 1, generator=None, ema=None):
        """Refill the codes used fewer than ``threshold`` times since reset_usage() (``code_usage``) by D^2 sampling over the
        encoder outputs of x, starting from each row's distance to its assigned code.  Resets ``code_usage``; with an
        ``ema.EMACodebook`` of this codebook, restarts the revived codes' statistics.  Returns the revived code ids (int64).
        Not inside a captured graph replay (icl.GraphedTokenizerStep): call it between replays."""
        from .kmeans import assign, draws
        cb = self._codebook().detach()
        K = cb.shape[0]
        z = self.encode(x)
        idx = assign(z, cb, self._DIST)
        u = draws(K, generator, z.device)
        n_dead = int((self.code_usage < threshold).sum())
        revived = torch.zeros(0, device=cb.device, dtype=torch.int64)
        if n_dead and z.shape[0] > 0:
            picks, _ = ops.kmeans_revive_(cb, z, idx, self.code_usage, threshold, u, self._DIST, max_codes=n_dead)
            revived = torch.nonzero(picks >= 0).reshape(-1)
            if ema is not None:
                ema.reset_codes_(revived)
            self._codebook_written()
        self.reset_usage()
        return revived

    def perplexity(self):
        """exp(entropy) of the accumulated code-usage histogram."""
        c = self.code_usage.to(torch.float64)
        p = c / c.sum().clamp_min(1)
        nz = p > 0
        return float(torch.exp(-(p[nz] * p[nz].log()).sum()))

    @staticmethod
    def _as_rows(x):
        if x.dim() != 2:
            raise ValueError(f"expected [N, feature_dim] (the reference flattens [B,T,A] to [B*T,A] "
                             f"before the tokenizer, tensor_utils.py:1066-1067); got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise TypeError(f"expected float32 actions, got {x.dtype}")
        return x.contiguous()

    # -- which launches a call runs -------------------------------------------------
    def fused_shape(self) -> bool:
        K, D = self._codebook().shape
        return ops.tokenize_supported(self.feature_dim, 64, self.hidden_dim, D, K)

    def _plan(self, n, entry, need_grad=False, mode="parity", screen=None, decoder=None) -> _Plan:
        """THE routing policy: which encoder + quantizer route a call of n rows runs, and whether its decoder folds the loss.
        entry = "tokenize" | "forward" | "quantize" (_quantize called on its own: z_e exists, no fused launch); decoder = the
        packed decoder stack of a forward.  The screen monitor is consulted at most ONCE, only for a batch above EXACT_ROWS_MAX
        (the exact kernel copes with all the rows of a smaller one) and only where a screened route exists; screen = an answer
        the caller already has.  The one difference between the entry points: tokenize() takes the fused launch at small batches as
        well where FUSED_SMALL_TOKENIZE says so (the metric's path; its small launch has its own workgroup shape), a small forward()
        keeps mlp3 + exact rows, which hands it the pre-activations or z_e it saves."""
        K, D = self._codebook().shape
        if mode != "parity":
            if mode != "fast":
                raise ValueError(f"unknown tokenize mode {mode!r}")
            if not ops.tokenize_fast_supported(self.feature_dim, 64, self.hidden_dim, D, K):
                raise RuntimeError("tokenize(mode='fast') needs the fast kernel's shapes (hidden 64/128, D in {32, 64, 128})")
        keep = "pre" if need_grad else ("ze" if entry == "forward" else None)
        fold = decoder is not None and ops.mlp3_loss_supported(n, decoder)
        fusable = entry != "quantize" and K >= self.FUSED_MIN_CODES            # (... and fused_shape(), asked where it matters)
        if n == 0:
            route = ALL_PAIRS
        elif self._small(n):
            # training-step batches: the exact kernel on every row beats preparing the codebook + one screen launch
            if fusable and entry == "tokenize" and self.FUSED_SMALL_TOKENIZE and self.fused_shape():
                route = FUSED
            else:
                route = ROWS if self._screenable(K, D) else ALL_PAIRS
        else:
            fusable = fusable and self.fused_shape()
            if (fusable or self._screenable(K, D)) and (self.screen_pays(n) if screen is None else screen):
                route = FUSED if fusable else SCREENED
            else:
                route = ALL_PAIRS
        return _Plan(route, keep, mode == "fast", fold)

    def _screenable(self, K, D):
        return K >= self.SCREEN_MIN_CODES and ops.nearest_screen_supported(K, D)

    def _small(self, n_rows):
        return n_rows <= self.EXACT_ROWS_MAX

    def screen_pays(self, n_rows: int) -> bool:
        """Small batches never consult the monitor (the exact kernel copes with all of their rows); large ones ask it whether the
        screen has been certifying its rows (see _ScreenMonitor)."""
        return self._small(n_rows) or self._screen_monitor.use_screen()

    def _quantize(self, z_e, usage, screen=None, route=None):
        """(idx, z_q) of v5:37-48 / vq:57-66 (``self._DIST``; first minimum) on one of the three unfused routes: exact rows, MFMA
        screen + exact re-scoring where the latent width has a screening instance and the codebook is large enough to pay for
        it, the all-pairs exact kernel otherwise.  Identical results on every route."""
        cb = self._codebook().detach()
        if route is None:
            route = self._plan(z_e.shape[0], "quantize", screen=screen).route
        if route == SCREENED:
            idx, zq, ws = ops.nearest_screened(z_e, cb, self._prepared(cb), usage=usage, return_workspace=True, dist=self._DIST)
            self._screened(ws, z_e.shape[0], ops.screen_is_coarse(*cb.shape))
            return idx, zq
        self.last_exact_rows = None
        if route == ROWS:
            return ops.nearest_rows(z_e, cb, usage=usage, dist=self._DIST)
        idx, zq, _ = ops.nearest(z_e, cb, self._DIST, usage=usage)
        return idx, zq

    def _encode_quantize(self, x, usage, plan, packed=None):
        """(idx, z_q, z_e, pre) on the plan's route; z_e / pre are None where the plan does not keep them (fused launch)."""
        if plan.route == FUSED:
            out = self._tokenize_fused(x, usage, want_ze=plan.keep == "ze", fast=plan.fast, want_pre=plan.keep == "pre")
            return out if plan.keep == "pre" else (*out, None)
        if packed is None:
            packed = self._enc_packed()
        if plan.keep == "pre":
            z_e, pre = ops.mlp3(x, packed, self._ENC_ACTS, save_pre=True)
        else:
            z_e, pre = ops.mlp3(x, packed, self._ENC_ACTS), None
        idx, zq = self._quantize(z_e, usage, route=plan.route)
        return idx, zq, z_e, pre

    # prologue and epilogue of a screened launch (fused or stand-alone)
    def _prepared(self, cb):
        return self._cb_cache.get((self._codebook(),), lambda: ops.nearest_prepare(cb))

    def _fused_operands(self, x):
        """(codebook, prepared codebook, workspace) of a fused launch; the workspace (row list) is reused across calls."""
        cb = self._codebook().detach()
        prep = self._prepared(cb)
        key = (x.shape[0], x.device)
        if self._tok_ws_key != key:
            self._tok_ws, self._tok_ws_key = ops.tokenize_workspace(x.shape[0], cb.shape[1], x.device), key
        return cb, prep, self._tok_ws

    def _screened(self, ws, n, coarse):
        self.last_exact_rows = ws
        self._screen_monitor.record(ws, n, coarse)

    # -- the metric's path ------------------------------------------------------------------
    @torch.no_grad()
    def encode(self, x):
        """z_e = to_latent(encoder(x))   (v5:71-72; vq:38-43)."""
        return ops.mlp3(self._as_rows(x), self._enc_packed(), self._ENC_ACTS)

    def _tokenize(self, x, count_usage, mode="parity"):
        x = self._as_rows(x)
        plan = self._plan(x.shape[0], "tokenize", mode=mode)
        idx, zq, z_e, _ = self._encode_quantize(x, self.code_usage if count_usage else None, plan)
        self.last_indices = idx
        return idx, zq, z_e

    # -- reference forward ------------------------------------------------------------------
    def forward(self, x):
        from .autograd import tokenizer_forward
        return tokenizer_forward(self, self._as_rows(x))


class LLFQVAE_V4(_TokenizerBase):
    def __init__(self, feature_dim, latent_dim, num_codes=1024, hidden_dim=128):
        super().__init__()
        if hidden_dim % 32 or not (32 <= hidden_dim <= 256):
            raise ValueError("hidden_dim must be a multiple of 32 in [32, 256] on the MI355X path (MFMA tiles of 32)")
        # construction order = the reference's (v5:54-68), so RNG draws line up
        self.encoder = nn.Sequential(nn.Linear(feature_dim, 64), nn.GELU(), nn.Linear(64, hidden_dim), nn.GELU())
        self.to_latent = LipschitzMLP(hidden_dim, latent_dim)
        self.quantizer = LFQQuantizer(num_codes, latent_dim)
        self.decoder = nn.Sequential(nn.Linear(latent_dim, 64), nn.GELU(), nn.Linear(64, hidden_dim), nn.GELU())
        self.to_output = nn.Linear(hidden_dim, feature_dim)
        self.feature_dim, self.latent_dim, self.num_codes, self.hidden_dim = feature_dim, latent_dim, num_codes, hidden_dim
        self._init_extras(num_codes)

    _DIST = DIST_NORM
    _ENC_ACTS = (ACT_GELU, ACT_GELU, ACT_SIGMOID)
    _DEC_ACTS = (ACT_GELU, ACT_GELU, ACT_NONE)
    # recon + 0.25*commit + 0.25*codebook, left to right (v5:83): (m0 + q) + q with q = 0.25 m1, evaluated on the device
    _LOSS = ops.LOSS_LLFQ
    _loss_weight = 0.25
    _STE = False                  # the decoder runs on codebook[idx] (no straight-through estimator, v5:74-81); z_latent = z_q
    _backward = llfq_backward
    FUSED_SMALL_TOKENIZE = True

    def _codebook(self):
        return self.quantizer.codebook

    # -- packed weights ---------------------------------------------------------------------
    def _enc_params(self):
        return (self.encoder[0].weight, self.encoder[0].bias, self.encoder[2].weight, self.encoder[2].bias,
                self.to_latent.W, self.to_latent.b, self.to_latent.ci)

    def _dec_params(self):
        return (self.decoder[0].weight, self.decoder[0].bias, self.decoder[2].weight, self.decoder[2].bias,
                self.to_output.weight, self.to_output.bias)

    def _params(self):
        return (*self._enc_params(), self.quantizer.codebook, *self._dec_params())

    def _packed_encoder(self):
        def build():
            w0, b0, w1, b1, W, b, ci = (t.detach() for t in self._enc_params())
            scale, Wn = ops.lipschitz_scale(W, ci)
            return ops.mlp3_pack(w0, b0, w1, b1, Wn, b), scale, Wn
        return self._enc_cache.get(self._enc_params(), build)

    def _fused_inputs(self, x):
        """(packed encoder, its six raw tensors -- the exact stage re-encodes uncertified rows with them --, codebook, prepared
        codebook, workspace) of the fused launch and of its tuner."""
        packed, _, Wn = self._packed_encoder()
        w0, b0, w1, b1, _, b2, _ = (t.detach() for t in self._enc_params())
        return (packed, (w0, b0, w1, b1, Wn, b2), *self._fused_operands(x))

    def _tokenize_fused(self, x, usage, want_ze=False, fast=False, want_pre=False):
        """(idx, z_q, z_e | None) from ONE persistent launch: z_e never leaves registers unless asked for
        (csrc/lipvq_fused.hip).  want_pre (training forward): (idx, z_q, z_e, pre) with the three pre-activations as well.
        Caller checks fused_shape()."""
        packed, raw, cb, prep, ws = self._fused_inputs(x)
        packed16 = None
        if fast:
            packed16 = self._enc16_cache.get((raw[0], raw[2], self.to_latent.W, self.to_latent.ci),
                                             lambda: ops.mlp3_pack_f16(raw[0], raw[2], raw[4]))
        out = ops.tokenize(x, packed, raw, cb, prep, usage=usage, want_ze=want_ze, workspace=ws, packed16=packed16,
                           want_pre=want_pre)
        self._screened(out[3], x.shape[0], (not fast) and ops.screen_is_coarse(*cb.shape))
        return (*out[:3], out[4]) if want_pre else out[:3]

    @torch.no_grad()
    def tune(self, x, launches=150):
        """Measure the fused launch's device-dependent schedule choices on THIS device with this batch and keep the fastest for the
        process (lipvq_tokenize_tune_f32; MI355X devices hold different clocks under the same kernel, and what wins on one loses on
        another: profiles/r04_i_clock_ab.txt).  Results are identical under every choice.  Synchronous: call it once, outside any
        timed or captured region.  Returns {"choice": {"defer_ze", "nt_ze"}, "ms_per_launch": {...}} or None (no fused launch here)."""
        x = self._as_rows(x)
        if x.shape[0] == 0 or not self.fused_shape():
            return None
        packed, raw, cb, prep, ws = self._fused_inputs(x)
        choice, ms = ops.tokenize_tune(x, packed, raw, cb, prep, workspace=ws, launches=launches)
        if choice < 0:                                       # latent widths above 64: nothing device-dependent to choose
            return None
        return {"choice": {"defer_ze": choice & 1, "nt_ze": (choice >> 1) & 1},
                "ms_per_launch": {f"defer_ze={c & 1},nt_ze={(c >> 1) & 1}": ms[c] for c in range(4)}}

    @torch.no_grad()
    def tokenize(self, x, count_usage=True, mode="parity"):
        """encode + quantize: (indices[N] int64, z_latent[N,D])   (v5:71-74).

        mode="parity" (default): fp32 everywhere, indices bit-identical to the CPU oracle / the reference.
        mode="fast": the encoder's GEMMs on fp16 MFMAs (fp32 accumulation) -- SURVEY section 7's throughput mode; a
        fraction of a percent of the indices differ from parity mode, always between near-equidistant codes."""
        return self._tokenize(x, count_usage, mode)[:2]

    @torch.no_grad()
    def decode(self, indices):
        """x_recon = to_output(decoder(codebook[indices]))   (v5:75-76)."""
        return ops.mlp3(self.quantizer.codebook.detach(), self._packed_decoder(), self._DEC_ACTS, gather_idx=indices)


class VQVAE(_TokenizerBase):
    def __init__(self, feature_dim, latent_dim, num_embeddings=128, commitment_cost=0.25):
        super().__init__()
        self.feature_dim = feature_dim
        self.latent_dim = latent_dim
        self.num_embeddings = num_embeddings
        self.commitment_cost = commitment_cost
        self.encoder = nn.Sequential(nn.Linear(feature_dim, 64), nn.ReLU(), nn.Linear(64, 128), nn.ReLU(),
                                     nn.Linear(128, latent_dim), nn.ReLU())
        self.decoder = nn.Sequential(nn.Linear(latent_dim, 128), nn.ReLU(), nn.Linear(128, 64), nn.ReLU(),
                                     nn.Linear(64, feature_dim), nn.ReLU())
        self.embedding = nn.Embedding(num_embeddings, latent_dim)
        self.embedding.weight.data.uniform_(-1 / num_embeddings, 1 / num_embeddings)
        self._init_extras(num_embeddings)

    _DIST = DIST_SQSUM
    _ENC_ACTS = _DEC_ACTS = (ACT_RELU, ACT_RELU, ACT_RELU)
    # q_loss = m1 + commitment_cost m1 (vq:69-71); loss = m0 + q_loss (vq:50-51): evaluated on the device
    _LOSS = ops.LOSS_VQ
    _loss_weight = property(lambda self: float(self.commitment_cost))
    _STE = True                   # the decoder runs on z_st = z_e + (z_q - z_e) (vq:74), which is also the returned latent
    _backward = vq_backward
    hidden_dim = 128              # (the encoder's second width, fixed in the reference: vq:20)
    # the all-pairs kernel stays the route for small codebooks: at K = 128 (the reference's default, vq:7) it runs at its VALU
    # bound in 0.4 ms per 524 288 rows, where a screen launch + its uncertified rows would gain nothing
    SCREEN_MIN_CODES = 256
    # ... but the FUSED launch (encoder + screen in one kernel, z_e never re-read) beats encoder + all-pairs from far fewer codes on
    FUSED_MIN_CODES = 64

    def _codebook(self):
        return self.embedding.weight

    def _enc_params(self):
        e = self.encoder
        return (e[0].weight, e[0].bias, e[2].weight, e[2].bias, e[4].weight, e[4].bias)

    def _dec_params(self):
        d = self.decoder
        return (d[0].weight, d[0].bias, d[2].weight, d[2].bias, d[4].weight, d[4].bias)

    def _params(self):
        return (*self._enc_params(), *self._dec_params(), self.embedding.weight)

    def _packed_encoder(self):
        return self._enc_cache.get(self._enc_params(),
                                   lambda: ops.mlp3_pack(*(t.detach() for t in self._enc_params())))

    def _tokenize_fused(self, x, usage, want_ze=True, fast=False, want_pre=False):
        """(idx, z_q, z_e) from ONE persistent launch (lipvq_vq_tokenize_f32: the fused kernel's ReLU instance, per-row fp16
        scales): encoder + screen, then the exact stage for the rows the screen leaves.  z_e is always returned (the
        straight-through value needs it).  want_pre: (idx, z_q, z_e, pre) with the three pre-activations a training step saves
        (lipvq_vq_tokenize_train_f32)."""
        if fast:
            raise ValueError("the plain VQVAE has no fast mode")
        cb, prep, ws = self._fused_operands(x)
        out = ops.vq_tokenize(x, self._packed_encoder(), cb, prep, usage=usage, workspace=ws, want_pre=want_pre)
        self._screened(out[-1], x.shape[0], ops.screen_is_coarse(*cb.shape))
        return out[:-1]

    @torch.no_grad()
    def tokenize(self, x, count_usage=True):
        idx, zq, z_e = self._tokenize(x, count_usage)
        return idx, ops.ste(z_e, zq)
