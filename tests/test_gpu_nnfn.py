"""GPU: lipvq_vae_amd.nnfn.LinearFn on its own -- the one Linear autograd function of embedding.py, default_branch.py and
gpt.py -- against float64 F.linear + autograd at the smallest shapes that take each of its branches (2-D / N-D input, with /
without bias, with / without an activation, a gradient only for the weight).  Tolerances as in the module tests: 1e-5 of the
forward's scale, 1e-4 of a gradient's."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


@pytest.fixture
def calls(monkeypatch):
    """What LinearFn asked of ops.linear / ops.wgrad: the number of Linear launches and the (gW, gb) pairs that came back."""
    from lipvq_vae_amd import ops
    seen = {"linear": 0, "wgrad": []}
    linear, wgrad = ops.linear, ops.wgrad

    def linear_(*a, **k):
        seen["linear"] += 1
        return linear(*a, **k)

    def wgrad_(*a, **k):
        seen["wgrad"].append(wgrad(*a, **k))
        return seen["wgrad"][-1]

    monkeypatch.setattr(ops, "linear", linear_)
    monkeypatch.setattr(ops, "wgrad", wgrad_)
    return seen


@pytest.mark.parametrize("shape,E,with_b,gelu,only_w", [((5, 12), 64, True, False, False), ((2, 3, 8), 24, False, False, False),
                                                        ((7, 64), 128, True, True, False), ((5, 12), 64, True, False, True)])
def test_linear_fn_against_float64_autograd(calls, shape, E, with_b, gelu, only_w):
    from lipvq_vae_amd.nnfn import LinearFn
    from lipvq_vae_amd.ops import ACT_GELU, ACT_NONE
    g = torch.Generator().manual_seed(sum(shape) + E)
    x, W = torch.randn(*shape, generator=g), torch.randn(E, shape[-1], generator=g) / shape[-1] ** 0.5
    b = torch.randn(E, generator=g) if with_b else None
    gy = torch.randn(*shape[:-1], E, generator=g)
    xd, Wd = x.double().requires_grad_(not only_w), W.double().requires_grad_(True)
    bd = b.double().requires_grad_(not only_w) if with_b else None
    ref = F.linear(xd, Wd, bd)
    if gelu:
        ref = F.gelu(ref)
    (ref * gy.double()).sum().backward()

    xc, Wc = x.cuda().requires_grad_(not only_w), W.cuda().requires_grad_(True)
    bc = b.cuda().requires_grad_(not only_w) if with_b else None
    y = LinearFn.apply(xc, Wc, bc, ACT_GELU if gelu else ACT_NONE)
    assert y.shape == ref.shape and _rel(y.detach().cpu(), ref.detach()) <= 1e-5
    y.backward(gy.cuda())
    assert _rel(Wc.grad.cpu(), Wd.grad) <= 1e-4
    (gW, gb), = calls["wgrad"]
    if only_w:
        assert calls["linear"] == 1                                                  # gx is None: no second Linear was launched
    else:
        assert calls["linear"] == 2 and xc.grad.shape == x.shape and _rel(xc.grad.cpu(), xd.grad) <= 1e-4
    if with_b:
        assert only_w or _rel(bc.grad.cpu(), bd.grad) <= 1e-4
    else:
        assert gb is None                                                            # no bias: the wgrad kernel forms none
