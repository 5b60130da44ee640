"""Data-dependent codebook initialisation and dead-code revival -- an EXTENSION, not reference behaviour.

The reference initialises its codebooks without looking at data (backbone_lfqvae_v5.py:32-35: kaiming_uniform_; backbone.py:36:
U(-1/K, 1/K)), and at that initialisation every encoder output maps to one code.  The standard VQ remedies
are built here, off by default and never called by ``forward()``:

* ``kmeans(z, codebook, ...)``: k-means++ seeding (Arthur & Vassilvitskii 2007; D^2 sampling, include/lipvq.h
  lipvq_kmeans_seed_f32) on at most ``seed_rows`` rows, then ``iters`` Lloyd steps on all rows.  A Lloyd step assigns every row
  with the exact nearest-code kernels, sums the rows per code in ascending row order (``ops.scatter_add(deterministic=True)``),
  divides (lipvq_kmeans_means_f32) and refills the codes left empty by D^2 sampling (lipvq_kmeans_revive_f32).
* ``lloyd_step`` and ``assign`` for callers that drive the loop themselves; the tokenizers' ``init_codebook_`` and
  ``revive_dead_codes_`` (tokenizer.py) use them.

Every random number is a ``torch.rand(..., dtype=torch.float64, generator=generator)`` draw (the seed subset: ``torch.randperm``
with the same generator), so one generator state gives one codebook.  Single rank: the statistics are not all-reduced.
"""
from __future__ import annotations

import torch

from . import ops
from .ops import DIST_NORM
from .tokenizer import _TokenizerBase

__all__ = ["kmeans", "lloyd_step", "assign", "draws"]


def draws(n: int, generator=None, device=None) -> torch.Tensor:
    """n fp64 draws in [0, 1) from ``generator`` (on the generator's device, then moved to ``device``)."""
    gdev = generator.device if generator is not None else torch.device("cpu")
    u = torch.rand(int(n), dtype=torch.float64, generator=generator, device=gdev)
    return u if device is None else u.to(device)


def assign(z, codebook, dist: int = DIST_NORM, usage=None):
    """Exact nearest-code indices of the rows of z (the tokenizers' decision, first minimum); usage [K] int64 is accumulated."""
    if z.shape[0] <= _TokenizerBase.EXACT_ROWS_MAX:     # the small-batch exact kernel up to the tokenizers' own threshold
        return ops.nearest_rows(z, codebook, usage=usage, want_zq=False, dist=dist)[0]
    return ops.nearest(z, codebook, dist, usage=usage, want_zq=False)[0]


@torch.no_grad()
def lloyd_step(z, codebook, dist: int = DIST_NORM, generator=None):
    """One Lloyd iteration on codebook [K, D] in place: assignment, per-code means of the rows, D^2 refill of the codes that
    received no row (each from its own draw; the refill starts from every row's distance to its UPDATED code).  Returns
    (idx [N], counts [K]) of the assignment.  Reads one host scalar (how many codes are empty) to size the refill."""
    K = codebook.shape[0]
    counts = torch.zeros(K, device=z.device, dtype=torch.int64)
    idx = assign(z, codebook, dist, usage=counts)
    sums = ops.scatter_add(z, idx, K, deterministic=True)
    ops.kmeans_means_(codebook, sums, counts)
    u = draws(K, generator, z.device)                 # drawn every step: the generator advances the same way whatever is empty
    n_empty = int((counts == 0).sum())
    if n_empty:
        ops.kmeans_revive_(codebook, z, idx, counts, 1, u, dist, max_codes=n_empty)
    return idx, counts


@torch.no_grad()
def kmeans(z, codebook, iters: int = 10, generator=None, dist: int = DIST_NORM, seed_rows: int | None = None):
    """k-means++ seeding then ``iters`` Lloyd steps; writes codebook [K, D] (contiguous fp32 on z's device) in place and returns
    it.  Seeding runs on at most ``seed_rows`` rows (default 256 K; a subset drawn with ``generator`` when z has more)."""
    z = z.detach()
    if z.dim() != 2 or codebook.dim() != 2 or codebook.shape[1] != z.shape[1]:
        raise ValueError(f"kmeans: z must be [N, D] and codebook [K, D], got {tuple(z.shape)} and {tuple(codebook.shape)}")
    if int(iters) < 0:
        raise ValueError("kmeans: iters must be >= 0")
    K = codebook.shape[0]
    seed_rows = 256 * K if seed_rows is None else int(seed_rows)
    if seed_rows < 1:
        raise ValueError("kmeans: seed_rows must be >= 1")
    zs = z
    if z.shape[0] > seed_rows:
        gdev = generator.device if generator is not None else torch.device("cpu")
        sub = torch.randperm(z.shape[0], generator=generator, device=gdev)[:seed_rows].to(z.device)
        zs = z.index_select(0, sub)
    ops.kmeans_seed(zs, K, draws(K, generator, z.device), dist, out=codebook)
    for _ in range(int(iters)):
        lloyd_step(z, codebook, dist, generator)
    return codebook
