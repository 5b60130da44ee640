"""No GPU: the references of tests/autograd_cases.py are what they claim -- freezing a leaf changes no other leaf's float64
gradient, an unused output drops exactly its own term -- and each property of tests/test_gpu_autograd_contract.py can be SEEN at
the case's shape: a deliberately wrong evaluation (the residual stream's gradient dropped, the sum's gradient dropped, a frozen
leaf's gradient routed to its neighbour, the second call's spectral state in the backward of the first) leaves the bound by
``MARGIN``.  A case at which it does not could not notice the bug and has to change."""
import pytest
import torch

import autograd_cases as C
import xf_edge_inputs as X

ALL = C.NAMES + C.register_fused()
EXACT = 1e-12                     # float64 runs of the same ops on the same numbers: equal up to the order autograd sums in


def _bound(case, leaf, trainable=None, coeff=None):
    return X.bound(X.BWD_TOL, C.dev(case, trainable, coeff)[1][leaf])


@pytest.mark.parametrize("name", ALL)
def test_every_leaf_has_a_gradient_and_the_yardstick_stays_tight(name):
    case = C.get(name)
    outs, grads = C.evaluate(case)
    dev_o, dev_g = C.dev(case)
    for k, g in grads.items():
        assert g is not None and g.shape == case.leaves[k].shape and float(g.abs().max()) > 0, (name, k)
        print(f"{name} {k}: dev {dev_g[k]:.3e}")
        assert X.REF_FACTOR * dev_g[k] <= X.DEV_CAP, (name, k, dev_g[k])
    for k in outs:
        assert X.REF_FACTOR * dev_o[k] <= X.DEV_CAP, (name, k, dev_o[k])
    labels = [label for label, _ in case.patterns()]
    assert len(set(labels)) == len(labels) and all(tr <= set(case.leaves) for _, tr in case.patterns())


@pytest.mark.parametrize("name", C.FREEZE_NAMES + C.register_fused())
def test_freezing_leaves_changes_no_kept_gradient(name):
    case = C.get(name)
    _, full = C.evaluate(case)
    for label, trainable in case.patterns():
        _, part = C.evaluate(case, trainable=trainable)
        for k in case.leaves:
            if k in trainable:
                err = X.rel(part[k], full[k])
                assert err <= EXACT, (name, label, k, err)
            else:
                assert part[k] is None, (name, label, k)
        # the fp32 run of the frozen pattern is the yardstick's other half: it exists and stays tight
        assert all(X.REF_FACTOR * d <= X.DEV_CAP for d in C.dev(case, trainable)[1].values())


USES = ([("addln_ab", u) for u in ({"y": 1.0}, {"s": 1.0}, {"s": 1.0, "y": 1.0})] + [("addln_a", {"y": 1.0}), ("addln_a", {"s": 1.0})]
        + [(f"gmm_{a}_{lay}", u) for a in ("softplus", "exp") for lay in ("dense", "view")
           for u in list(C.GMM_LOGPROB_USES.values()) + list(C.GMM_PARAM_USES.values())]
        + [(f"head_{lay}", u) for lay in ("dense", "view") for u in C.HEAD_USES.values()])


@pytest.mark.parametrize("name,use", USES, ids=[f"{n}-{'+'.join(u)}" for n, u in USES])
def test_an_unused_output_drops_its_own_term_and_nothing_else(name, use):
    """grad(sum_k c_k L_k) = sum_k c_k grad(L_k) over the outputs that remain."""
    case = C.get(name)
    _, got = C.evaluate(case, coeff=use)
    singles = {k: C.evaluate(case, coeff={k: 1.0})[1] for k in use}
    for leaf in case.leaves:
        want = sum(c * singles[k][leaf] for k, c in use.items() if singles[k][leaf] is not None)
        if not torch.is_tensor(want):
            assert got[leaf] is None, (name, leaf)                 # (no remaining output depends on this leaf)
            continue
        assert X.rel(got[leaf], want) <= EXACT, (name, use, leaf)


def _misses(case, leaf, wrong, coeff=None, trainable=None):
    """The wrong value's distance from the reference over the bound: must be >= MARGIN."""
    want = C.evaluate(case, coeff=coeff, trainable=trainable)[1][leaf]
    err, b = X.rel(wrong, want), _bound(case, leaf, trainable, coeff)
    print(f"{case.name} {leaf}: wrong evaluation off by {err:.3e}, bound {b:.3e}, ratio {err / b:.1f}")
    return err / b


def test_wrong_dropping_the_residual_gradient_is_seen():
    """AddLayerNormFn.backward without gs, and with None for b."""
    case = C.get("addln_ab")
    both = {"s": 0.8, "y": 1.0}
    y_only = C.evaluate(case, coeff={"y": 1.0})[1]
    for leaf in ("in.a", "in.b"):
        assert _misses(case, leaf, y_only[leaf], coeff=both) >= C.MARGIN
        assert _misses(case, leaf, torch.zeros_like(y_only[leaf]), coeff=both) >= C.MARGIN
        assert _misses(case, leaf, torch.zeros_like(y_only[leaf]), coeff={"s": 1.0}) >= C.MARGIN
    # a + a: twice the one-sided gradient, not once
    assert _misses(case, "in.a", 0.5 * C.evaluate(case, coeff=both)[1]["in.a"], coeff=both) >= C.MARGIN


@pytest.mark.parametrize("name", [n for n in C.NAMES if n.startswith("gmm_")])
def test_wrong_dropping_one_gmm_upstream_gradient_is_seen(name):
    """_LogProbFn.backward without gsum (or without glp); _ParamsFn.backward without one of the gradients it was given."""
    case = C.get(name)
    both = C.GMM_LOGPROB_USES["both"]
    for dropped in both:
        wrong = C.evaluate(case, coeff={k: c for k, c in both.items() if k != dropped})[1]
        assert max(_misses(case, leaf, wrong[leaf], coeff=both) for leaf in case.leaves) >= C.MARGIN
        for leaf in case.leaves:
            assert _misses(case, leaf, wrong[leaf], coeff=both) >= C.MARGIN, (name, dropped, leaf)
    for use in C.GMM_PARAM_USES.values():
        for dropped in use:
            rest = {k: c for k, c in use.items() if k != dropped}
            wrong = C.evaluate(case, coeff=rest)[1] if rest else {leaf: None for leaf in case.leaves}
            hit = f"nets.{dropped}.weight"                             # the dropped output's own Linear must notice
            assert _misses(case, hit, torch.zeros_like(case.leaves[hit]) if wrong[hit] is None else wrong[hit], coeff=use) >= C.MARGIN
            feats = case.inputs[0]
            assert _misses(case, feats, torch.zeros_like(case.leaves[feats]) if wrong[feats] is None else wrong[feats], coeff=use) >= C.MARGIN


@pytest.mark.parametrize("name", [n for n in C.NAMES if n.startswith("head_")])
def test_wrong_dropping_one_loss_gradient_is_seen(name):
    case = C.get(name)
    use = C.HEAD_USES["each_loss"]
    for dropped in use:
        wrong = C.evaluate(case, coeff={k: c for k, c in use.items() if k != dropped})[1]
        for leaf in case.leaves:
            assert _misses(case, leaf, wrong[leaf], coeff=use) >= C.MARGIN, (name, dropped, leaf)


@pytest.mark.parametrize("name", ALL)
def test_wrong_routing_a_gradient_to_a_neighbour_is_seen(name):
    """Any two leaves of one shape (the three dense streams of the embedding, the Linears of one width, a and b of the LayerNorm
    with the affine terms trained) have gradients further apart than MARGIN bounds -- except a and b of a + b, whose gradients ARE
    equal -- and every gradient is that far from zero and from its own double."""
    case = C.get(name)
    _, grads = C.evaluate(case)
    leaves = list(case.leaves)
    for i, a in enumerate(leaves):
        assert _misses(case, a, torch.zeros_like(grads[a])) >= C.MARGIN
        assert _misses(case, a, 2.0 * grads[a]) >= C.MARGIN
        for b in leaves[i + 1:]:
            if grads[a].shape == grads[b].shape and {a, b} != {"in.a", "in.b"}:
                assert _misses(case, a, grads[b]) >= C.MARGIN, (name, a, b)
    if case.kind == "addln" and "in.b" in case.leaves:
        assert torch.equal(grads["in.a"], grads["in.b"])


def test_wrong_spectral_state_of_the_second_call_is_seen():
    """Two training forwards, backward of the first: the reference is the single call's (the stock hook clones u and v); with the
    second call's state the spectral layers' gradients leave the bound."""
    first, single, second = (C.get(n) for n in ("default_L1_first_of_two", "default_L1", "default_L1_second_of_two"))
    g_first, g_single, g_second = (C.evaluate(c)[1] for c in (first, single, second))
    for k in first.leaves:
        assert X.rel(g_first[k], g_single[k]) <= EXACT, k
    for k in first.groups["spectral"]:
        if k.endswith("weight_orig"):
            assert _misses(first, k, g_second[k]) >= C.MARGIN, k


def test_fused_rows_is_the_plans_threshold():
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.tokenizer import FUSED, ROWS, LLFQVAE_V4, VQVAE, _TokenizerBase
    n = C.fused_train_rows()
    assert n == _TokenizerBase.EXACT_ROWS_MAX + 1
    for cls, args in ((LLFQVAE_V4, dict(num_codes=C.TOK["K"])), (VQVAE, dict(num_embeddings=C.TOK["K"]))):
        m = cls(C.TOK["A"], C.TOK["D"], **args)
        assert m._plan(n, "forward", True, screen=True).route == FUSED and m._plan(n - 1, "forward", True).route != FUSED
        assert m._plan(C.TOK["N"], "forward", True).route in (ROWS, "all_pairs")


# ---------------------------------------------------------------------------------------------------
# nnfn.first_order_only, on a CPU function
# ---------------------------------------------------------------------------------------------------

def _square_fn(decorator):
    class Square(torch.autograd.Function):
        """(x^2, None) with a graph-less backward, as the library's kernels give."""

        @staticmethod
        def forward(ctx, x, flag):
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(x)
            return x * x, None

        @staticmethod
        @decorator
        def backward(ctx, g, _g2):
            x, = ctx.saved_tensors
            return torch.from_numpy((2.0 * x * g).detach().numpy().copy()), None

    return Square


def test_first_order_only_refuses_the_second_differentiation_that_once_differentiable_lets_through():
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.nnfn import first_order_only
    x0 = torch.tensor([0.5, -1.5, 2.0])

    def mixed_loss(decorator):
        x = x0.clone().requires_grad_(True)
        out = _square_fn(decorator).apply(x, 3)[0]
        gx, = torch.autograd.grad(out.sum(), x, create_graph=True)
        assert torch.equal(gx.detach(), 2.0 * x0)
        (out.sum() + gx.square().sum()).backward()
        return x.grad

    # torch's decorator alone: the upstream gradient of out.sum() requires none, so the graph-less gx goes through and the second
    # term is silently ignored (the gradient of sum x^2 + sum 4 x^2 is 10 x, this is 2 x)
    assert torch.equal(mixed_loss(torch.autograd.function.once_differentiable), 2.0 * x0)
    with pytest.raises(RuntimeError, match="differentiable once only"):
        mixed_loss(first_order_only)
    # an upstream gradient that requires one: torch's own error node, kept
    x = x0.clone().requires_grad_(True)
    w = torch.ones(3, requires_grad=True)
    gx, = torch.autograd.grad((_square_fn(first_order_only).apply(x, 3)[0] * w).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()
    # first order: same bits, plain tensors, retain_graph and accumulation as before
    x = x0.clone().requires_grad_(True)
    out = _square_fn(first_order_only).apply(x, 3)[0]
    out.sum().backward(retain_graph=True)
    assert torch.equal(x.grad, 2.0 * x0) and x.grad.grad_fn is None and not x.grad.requires_grad
    out.sum().backward()
    assert torch.equal(x.grad, 4.0 * x0)
    g, = torch.autograd.grad(_square_fn(first_order_only).apply(x, 3)[0].sum(), x, create_graph=True)
    assert torch.equal(g.detach(), 2.0 * x0)                        # create_graph alone still gives the first-order numbers


def test_wants_backward_sees_the_callers_grad_mode():
    """Inside forward, grad mode is always off and needs_input_grad repeats requires_grad: only KernelFunction.apply knows that
    the caller stood under torch.no_grad()."""
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.nnfn import KernelFunction, wants_backward
    seen = []

    class Probe(KernelFunction):
        @staticmethod
        def forward(ctx, x, flag):
            seen.append((torch.is_grad_enabled(), any(ctx.needs_input_grad), wants_backward(ctx)))
            return x * 2.0

        @staticmethod
        def backward(ctx, g):
            return 2.0 * g, None

    x = torch.ones(3, requires_grad=True)
    y = Probe.apply(x, 1)
    with torch.no_grad():
        y_ng = Probe.apply(x, 1)
        with torch.enable_grad():
            y_in = Probe.apply(x, 1)
    y_frozen = Probe.apply(x.detach(), 1)
    y_after = Probe.apply(x, 1)                          # the note is restored after a no_grad call
    assert seen == [(False, True, True), (False, True, False), (False, True, True), (False, False, False), (False, True, True)]
    assert y.requires_grad and not y_ng.requires_grad and y_in.requires_grad and not y_frozen.requires_grad and y_after.requires_grad
    y.sum().backward()
    assert torch.equal(x.grad, torch.full((3,), 2.0))
