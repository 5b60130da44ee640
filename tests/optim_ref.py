"""Yardsticks for the policy update (tests/test_gpu_policy_update.py; their own conditions: tests/test_optim_ref_host.py).

The yardstick is torch itself on float64 CPU copies fed the same fp32 gradients: ``torch.nn.utils.clip_grad_norm_`` followed by
``torch.optim.Adam`` / ``AdamW``.  The same sequence on fp32 CPU copies is "stock fp32 torch": its error against the yardstick is
what fp32 arithmetic costs, and where the project's bound is exceeded the bound becomes 4 x that error (the rule LABNOTES already
uses for gradients)."""
import functools

import numpy as np
import torch

import bin_ref as B

CLIP_REGIMES = ("randn_decades", "spike", "huge", "tiny", "alternating", "zero")
MAX_NORMS = (1.0, 100.0)
LIST_LENGTHS = (1, 32, 33, 65)
EPS52 = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _grad(regime, n, step, index):
    g = B.adamw_grad(regime, n, step, index)
    if g is not None:
        g.setflags(write=False)
    return g


def grads_at(regime, sizes, step):
    """The fp32 gradients (read-only arrays, or None) of a parameter list at one step."""
    return [_grad(regime, int(n), step, i) for i, n in enumerate(sizes)]


def sumsq_f64(grads):
    """(sum of squares in float64, number of elements) over the gradients that are not None."""
    present = [g for g in grads if g is not None]
    return float(sum(np.sum(np.square(g.astype(np.float64)), dtype=np.float64) for g in present)), sum(g.size for g in present)


def clip_yardstick(grads, max_norm, dtype=torch.float64):
    """torch.nn.utils.clip_grad_norm_ on CPU copies of `dtype`: (stats [total_norm, clip_coef, sumsq, sumsq_clipped] as floats,
    the clipped gradients as tensors, None kept)."""
    ps = []
    for g in grads:
        p = torch.zeros(1 if g is None else g.size, dtype=dtype, requires_grad=True)
        p.grad = None if g is None else torch.from_numpy(np.array(g)).to(dtype)
        ps.append(p)
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    clipped = [p.grad for p in ps]
    after = sum(float(c.norm(2).pow(2)) for c in clipped if c is not None)           # the reference's grad_norms loop
    return (float(norm), float(coef), float(norm) ** 2, after), clipped


@functools.lru_cache(maxsize=None)
def _sumsq_at(regime, sizes, step):
    return sumsq_f64(grads_at(regime, sizes, step))[0]


def clip_ratio(regime, sizes, step, max_norm):
    """max_norm / (total_norm + 1e-6) of the float64 yardstick: the clamp's corner is at 1."""
    return max_norm / (np.sqrt(_sumsq_at(regime, tuple(sizes), step)) + 1e-6)


def stats_at(regime, sizes, step, max_norm):
    """torch's rule written out on the float64 sum of squares: [total_norm, clip_coef, sumsq, sumsq_clipped]
    (tests/test_optim_ref_host.py holds it against clip_yardstick)."""
    s = _sumsq_at(regime, tuple(sizes), step)
    coef = min(1.0, clip_ratio(regime, sizes, step, max_norm))
    return float(np.sqrt(s)), coef, s, coef * coef * s


class Trajectory:
    """`cls` (torch.optim.Adam or AdamW) with clip_grad_norm_(max_norm) in front of every step, on CPU copies of `dtype`.
    groups: list of (initial fp32 arrays, optimizer kwargs)."""

    def __init__(self, cls, groups, dtype, max_norm, **defaults):
        self.max_norm = max_norm
        spec = [dict(params=[torch.from_numpy(np.array(p)).to(dtype).requires_grad_(True) for p in init], **kw) for init, kw in groups]
        self.flat = [p for g in spec for p in g["params"]]
        self.opt = cls(spec, **defaults)

    def step(self, grads):
        for p, g in zip(self.flat, grads):
            p.grad = None if g is None else torch.from_numpy(np.array(g)).to(p.dtype)
        if self.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.flat, self.max_norm)
        self.opt.step()


def ulp32(x):
    """Spacing of fp32 at |x| (float64 array in, float64 out); the smallest normal's spacing below it."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), np.finfo(np.float32).tiny).astype(np.float32)
    return np.spacing(a).astype(np.float64)
