"""GPU: ICLInputEmbedding and DefaultActionNetwork under set_dropout_source("kernel") (include/lipvq.h, "in-kernel dropout for the
embedding stage and the default action branch").

Every claim is an equality of bits.  A training forward under the kernel source must give what a test-local restatement of the
module's forward gives over the EXISTING Functions -- keep bytes into the attention Function, torch multiplies by the mask
factor elsewhere --, the masks materialised by ops.dropout_keep at the documented sites of the snap the forward used; the step,
reseeding, eval mode, the way back to the torch source and a graphed training step follow."""
import copy
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 2 ** 63 + 4242


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _snap(seed, step=0):
    words = [v - 2 ** 64 if v >= 2 ** 63 else v for v in (seed & (2 ** 64 - 1), step & (2 ** 64 - 1))]
    return torch.tensor(words, dtype=torch.int64).cuda()


def _state_snap(net):
    """the (seed, step) a forward is about to use, as a snap of its own"""
    return net.dropout_state.detach().clone()


def _scale(ops, snap, site, rows, cols, p):
    inv_keep = float(np.float32(1.0) / np.float32(1.0 - p))
    return ops.dropout_keep(snap, site, rows, cols, p).float() * inv_keep


def _randn(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _default(D, layers=2, A=12, seed=3):
    from lipvq_vae_amd.default_branch import DefaultActionNetwork
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DefaultActionNetwork(A, D, num_layers=layers).cuda()


def _embedding(E=64, T=4, Din=64, p=0.1, seed=5):
    from lipvq_vae_amd.embedding import ICLInputEmbedding
    torch.manual_seed(seed)
    net = ICLInputEmbedding(Din, embed_dim=E, context_length=T, emb_dropout=p).cuda()
    with torch.no_grad():
        net.params["embed_timestep"].normal_(0.0, 0.5)
    return net


def _set_ps(net, p_att, p1, p2, p_ff):
    for layer in net[5].layers:
        layer.self_attn.dropout, layer.dropout1.p, layer.dropout2.p, layer.dropout.p = p_att, p1, p2, p_ff


def _default_restated(net, x, snap):
    """DefaultActionNetwork.forward in training mode over the existing Functions, the four masks of every layer explicit."""
    from lipvq_vae_amd import ops
    from lipvq_vae_amd.default_branch import _AttentionFn
    from lipvq_vae_amd.nnfn import AddLayerNormFn, LinearFn
    from lipvq_vae_amd.ops import ACT_GELU, ACT_NONE
    H, FF = net.NHEAD, net.FF
    h = LinearFn.apply(x, net._sn_weight(net[0]), net[0].bias, ACT_GELU)
    h = LinearFn.apply(h, net._sn_weight(net[2]), net[2].bias, ACT_GELU)
    h = LinearFn.apply(h, net._sn_weight(net[4]), net[4].bias, ACT_NONE)
    S, D = h.shape

    def mul(t, site, p):
        return t * _scale(ops, snap, site, t.shape[0], t.shape[1], p) if p > 0.0 else t

    for i, layer in enumerate(net[5].layers):
        attn, site = layer.self_attn, ops.DROPOUT_SITE_DEFAULT + 4 * i
        p_att = float(attn.dropout)
        keep, keep_prob = None, 1.0
        if p_att > 0.0:
            keep, keep_prob = ops.dropout_keep(snap, site, H * S, S, p_att).view(H, S, S), 1.0 - p_att
        qkv = LinearFn.apply(h, attn.in_proj_weight, attn.in_proj_bias, ACT_NONE)
        a = _AttentionFn.apply(qkv, H, keep, keep_prob)
        a = LinearFn.apply(a, attn.out_proj.weight, attn.out_proj.bias, ACT_NONE)
        a = mul(a, site + 1, float(layer.dropout1.p))
        h = AddLayerNormFn.apply(h, a, layer.norm1.weight, layer.norm1.bias, layer.norm1.eps, False)[1]
        f = LinearFn.apply(h, layer.linear1.weight, layer.linear1.bias, ACT_GELU)
        assert f.shape == (S, FF)
        f = mul(f, site + 3, float(layer.dropout.p))
        f = LinearFn.apply(f, layer.linear2.weight, layer.linear2.bias, ACT_NONE)
        f = mul(f, site + 2, float(layer.dropout2.p))
        h = AddLayerNormFn.apply(h, f, layer.norm2.weight, layer.norm2.bias, layer.norm2.eps, False)[1]
    return LinearFn.apply(h, net[6].weight, net[6].bias, ACT_NONE)


def _run(net, forward, x0, R):
    for q in net.parameters():
        q.grad = None
    x = x0.clone().requires_grad_(True)
    out = forward(x)
    (out * R).sum().backward()
    return out.detach(), x.grad, {k: q.grad.clone() for k, q in net.named_parameters()}


# ---------------------------------------------------------------------------------------------------
# 1. the modules against their restatements
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ps", [(0.1, 0.1, 0.1, 0.1), (0.0, 0.1, 0.1, 0.1), (0.1, 0.0, 0.1, 0.1), (0.1, 0.1, 0.0, 0.1), (0.1, 0.1, 0.1, 0.0)],
                         ids=["all", "att0", "drop1_0", "drop2_0", "ff0"])
@pytest.mark.parametrize("D", [64, 208])
def test_default_branch_equals_the_restated_forward(ops, D, ps):
    A, S = 12, 37
    base = _default(D, 2, A).train().set_dropout_source("kernel", seed=SEED)
    base.reseed_dropout(SEED, step=3)
    _set_ps(base, *ps)
    x0, R = _randn(1, S, A), _randn(2, S, D)
    # (a training forward runs the spectral norm's power iteration in place: each run starts from its own copy of the module)
    net, ref = copy.deepcopy(base), copy.deepcopy(base)
    snap = _state_snap(net)
    got = _run(net, net, x0, R)
    assert net.dropout_state.tolist() == [SEED - 2 ** 64, 4], "one dropout_begin per forward"
    want = _run(ref, lambda x: _default_restated(ref, x, snap), x0, R)
    assert torch.equal(got[0], want[0]), (D, ps, "output")
    assert torch.equal(got[1], want[1]), (D, ps, "input gradient")
    assert sorted(got[2]) == sorted(want[2]) and len(got[2]) > 20
    for k in want[2]:
        assert torch.equal(got[2][k], want[2][k]), (D, ps, k)
    for k in ("weight_u", "weight_v"):
        assert torch.equal(getattr(net[0], k), getattr(ref[0], k))
    plain = copy.deepcopy(base).eval()
    assert not torch.equal(got[0], plain(x0)), "no dropout happened"


def _embedding_against_restated(ops, kind):
    """the module under the kernel source against its plain path and ONE multiply; asserts the output and the input gradient,
    returns the parameter gradients of both"""
    B, T, E, Din, p = 2, 4, 64, 10, 0.1
    net = _embedding(E, T, Din, p).train().set_dropout_source("kernel", seed=SEED)
    net.reseed_dropout(SEED, step=9)
    obs, cobs, cact = (_randn(10 + k, B, T, Din) for k in range(3))
    S = {"forward": 3 * T, "prompt": 2 * T, "input": T}[kind]
    R = _randn(3, B, S, E)

    def call(x):
        if kind == "forward":
            return net(x, cobs, cact)
        return net.prompt_embedding(x, cact) if kind == "prompt" else net.input_embedding(x)

    snap = _state_snap(net)
    got = _run(net, call, obs, R)
    assert net.dropout_state.tolist() == [SEED - 2 ** 64, 10]
    m = _scale(ops, snap, ops.DROPOUT_SITE_EMBED, B * S, E, p).view(B, S, E)
    net.eval()                                                       # the module's plain path, then ONE multiply
    want = _run(net, lambda x: call(x) * m, obs, R)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), kind
    for k in want[2]:
        print(f"embedding {kind} {k}: |kernel - restated| max {float((got[2][k] - want[2][k]).abs().max()):.3e}")
    return got[2], want[2]


# the gradients that the atomic embed_rows backward entry points add with fp32 atomics; the module's backward
# (lipvq_embed_rows_bwd_det_f32) sums them in a fixed order, so they are held to torch.equal like the rest
ATOMIC = ("nets.embed_ln.weight", "nets.embed_ln.bias", "params.embed_timestep")


@pytest.mark.parametrize("kind", ["forward", "prompt", "input"])
def test_embedding_equals_the_restated_forward(ops, kind):
    """Output, input gradient and the embed_encoder's gradients: every sum with a fixed order."""
    got, want = _embedding_against_restated(ops, kind)
    for k in want:
        if k not in ATOMIC:
            assert torch.equal(got[k], want[k]), (kind, k)


@pytest.mark.parametrize("kind", ["forward", "prompt", "input"])
def test_embedding_atomically_summed_gradients_equal_the_restated_forward(ops, kind):
    """The LayerNorm weight and bias and the time embedding, torch.equal like the rest (sums in workgroup order, no atomics)."""
    got, want = _embedding_against_restated(ops, kind)
    for k in ATOMIC:
        assert torch.equal(got[k], want[k]), (kind, k)


# ---------------------------------------------------------------------------------------------------
# 2. the step: two forwards differ, reseeding reproduces, a backward uses its own forward's snap, torch's generators stay
# ---------------------------------------------------------------------------------------------------

def _both():
    emb = _embedding(64, 4, 10).train().set_dropout_source("kernel", seed=11)
    dflt = _default(64, 1).train().set_dropout_source("kernel", seed=11)
    obs = _randn(20, 2, 4, 10)
    acts = _randn(21, 9, 12)
    return (emb, lambda net, x: net.input_embedding(x), obs), (dflt, lambda net, x: net(x), acts)


def test_step_behaviour(ops):
    for base, call, x0 in _both():
        name = type(base).__name__
        net = copy.deepcopy(base)
        y1 = call(net, x0)
        assert net.dropout_state.tolist() == [11, 1], name
        y2 = call(net, x0)
        assert net.dropout_state.tolist() == [11, 2] and not torch.equal(y1, y2), name
        net = copy.deepcopy(base).reseed_dropout(11, 0)              # (a fresh copy: the spectral norm's u, v of the first forward)
        assert torch.equal(call(net, x0), y1), name
        # a backward that runs after a second forward still uses its own forward's snap
        net, ref = copy.deepcopy(base), copy.deepcopy(base)
        xa = x0.clone().requires_grad_(True)
        ya = call(net, xa)
        call(net, x0)                                                # the state moves on before the backward
        ya.square().sum().backward()
        xb = x0.clone().requires_grad_(True)
        call(ref, xb).square().sum().backward()
        assert torch.equal(xa.grad, xb.grad), name
        # equal (seed, step) in the two modules: unrelated fields, because the sites differ
    snap = _snap(11, 0)
    assert not torch.equal(ops.dropout_keep(snap, ops.DROPOUT_SITE_EMBED, 9, 64, 0.1), ops.dropout_keep(snap, ops.DROPOUT_SITE_DEFAULT + 1, 9, 64, 0.1))


def test_torch_rng_is_not_used(monkeypatch):
    pairs = _both()
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("the kernel dropout source called torch's RNG")
    monkeypatch.setattr(torch, "rand", refuse)
    monkeypatch.setattr(torch.nn.functional, "dropout", refuse)
    cpu_state, cuda_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    for net, call, x0 in pairs:
        x = x0.clone().requires_grad_(True)
        call(net, x).square().sum().backward()
        assert x.grad is not None and all(q.grad is not None for q in net.parameters()), type(net).__name__
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), cuda_state)
    monkeypatch.undo()
    for net, call, x0 in pairs:
        before = torch.cuda.get_rng_state()
        call(net.set_dropout_source("torch"), x0)
        assert not torch.equal(torch.cuda.get_rng_state(), before), "the torch source does draw from the CUDA generator"


def test_eval_mode_ignores_the_source(ops, monkeypatch):
    begins = []
    begin = ops.dropout_begin
    monkeypatch.setattr(ops, "dropout_begin", lambda st: begins.append(1) or begin(st))
    for net, call, x0 in _both():
        net.eval()
        before = net.dropout_state.tolist()
        with torch.no_grad():
            y_kernel = call(net, x0)
        assert not begins and net.dropout_state.tolist() == before
        with torch.no_grad():
            assert torch.equal(call(net.set_dropout_source("torch"), x0), y_kernel), type(net).__name__
        assert "_dropout_state" not in net.state_dict()


def test_back_to_the_torch_source_gives_the_never_switched_bits():
    for base, call, x0 in _both():
        never = copy.deepcopy(base).set_dropout_source("torch")
        never._buffers.pop("_dropout_state")                        # (as constructed: no state at all)
        back = copy.deepcopy(base)
        stepped = call(back, x0)                                     # a kernel-source step, then back to "torch" on the SAME module
        assert back.dropout_state.tolist()[1] == 1
        back.set_dropout_source("torch")
        if any(k.endswith("weight_u") for k, _ in back.named_buffers()):
            # the default branch's training forward also moved the spectral norm's u, v: the never-switched module takes the
            # same plain step first (under "torch" p = 0 would change nothing else; here the buffers are simply copied over)
            theirs = dict(never.named_buffers())
            for k, buf in back.named_buffers():
                if k.endswith(("weight_u", "weight_v")):
                    theirs[k].copy_(buf)
        outs = []
        for net in (never, back):
            torch.manual_seed(99)
            outs.append(call(net, x0))
        assert torch.equal(outs[0], outs[1]), type(base).__name__
        assert not torch.equal(outs[1], stepped)
        assert back.dropout_state.tolist()[1] == 1, "a torch-source forward moved the kernel source's state"
        torch.manual_seed(100)
        assert not torch.equal(call(copy.deepcopy(base).set_dropout_source("torch"), x0), outs[0])


# ---------------------------------------------------------------------------------------------------
# 3. the graphed training step: replay k = eager step k for every module
# ---------------------------------------------------------------------------------------------------

def _compare_graphed(make, batch, steps=(1, 2, 3)):
    """make() -> (loss_fn, params, extra_state tensors, states to watch); eager steps against replays from equal starts"""
    from lipvq_vae_amd import optim
    from lipvq_vae_amd.icl import GraphedPolicyStep
    runs = []
    for graphed in (False, True):
        loss_fn, params, extra, states = make()
        opt = optim.Adam(params, lr=torch.tensor(1e-3, device="cuda"), max_grad_norm=1.0)
        if graphed:
            start = [q.detach().clone() for q in params]
            step = GraphedPolicyStep(loss_fn, params, opt, batch(0), warmup=3, extra_state=extra)
            assert all(torch.equal(q.detach(), s) for q, s in zip(params, start))
            assert all(st.tolist()[1] == 0 for st in states), "construction advanced a dropout state"
        record = []
        for k in steps:
            inputs = batch(k)
            if graphed:
                loss, _ = step.step(*inputs)
            else:
                opt.zero_grad(set_to_none=True)
                loss = loss_fn(*inputs)
                loss.backward()
                opt.step()
            record.append([loss.detach().clone()] + [q.detach().clone() for q in params])
            assert all(st.tolist()[1] == k for st in states), (graphed, k, [st.tolist() for st in states])
        runs.append(record)
    for k, (eager, replay) in zip(steps, zip(*runs)):
        assert all(torch.equal(a, b) for a, b in zip(eager, replay)), f"replay {k} differs from eager step {k}"
    assert not torch.equal(runs[0][0][0], runs[0][1][0])


@pytest.mark.parametrize("train_atomic", [False, True], ids=["fixed_order_sums", "every_parameter"])
def test_graphed_policy_step_with_every_module_under_the_kernel_source(train_atomic):
    """embedding -> GPTBackbone -> ActionHead, all three under the kernel source, their states in extra_state: the loss and every
    parameter after replays 1 .. 3 equal eager steps 1 .. 3.

    [every_parameter] is the whole policy; [fixed_order_sums] leaves the embedding's LayerNorm and time embedding out of the
    optimizer (the three gradients the atomic backward entry points would not repeat)."""
    from lipvq_vae_amd.action_head import ActionHead
    from lipvq_vae_amd.gpt import GPTBackbone
    B, T, Din, A = 2, 4, 10, 7

    def make():
        emb = _embedding(64, T, Din, 0.1, seed=31).train().set_dropout_source("kernel", seed=71)
        if not train_atomic:
            for k, q in emb.named_parameters():
                q.requires_grad_(k not in ATOMIC)
        torch.manual_seed(32)
        net = GPTBackbone(64, 12, num_layers=1, num_heads=4).cuda().train().set_dropout_source("kernel", seed=72)
        torch.manual_seed(33)
        head = ActionHead(64, A).cuda().train()
        params = [q for q in (*emb.parameters(), *net.parameters(), *head.parameters()) if q.requires_grad]
        states = [emb.dropout_state, net.dropout_state]
        loss_fn = lambda obs, cobs, cact, a: head.losses(net(emb(obs, cobs, cact))[:, -T:], a)["action_loss"]      # noqa: E731
        return loss_fn, params, states, states

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        return tuple(torch.randn(B, T, Din, generator=g).cuda() for _ in range(3)) + ((torch.rand(B, T, A, generator=g) * 3.0 - 1.5).cuda(),)

    _compare_graphed(make, batch)


def test_graphed_step_of_the_default_branch_alone():
    S, A, D = 9, 12, 64

    def make():
        net = _default(D, 2, A, seed=41).train().set_dropout_source("kernel", seed=73)
        # what a training step writes besides the parameters: the dropout state and the spectral norm's u, v
        extra = [net.dropout_state] + [b for k, b in net.named_buffers() if k.endswith(("weight_u", "weight_v"))]
        assert len(extra) == 7
        loss_fn = lambda x, y: (net(x) - y).square().mean()          # noqa: E731
        return loss_fn, list(net.parameters()), extra, [net.dropout_state]

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(S, A, generator=g).cuda(), torch.randn(S, D, generator=g).cuda()

    _compare_graphed(make, batch)


def test_new_functions_are_marked_first_order_only():
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd import default_branch, embedding, nnfn
    for f in (nnfn.LinearFn, default_branch._AttentionFn, embedding._EmbedStreamsFn):
        assert issubclass(f, nnfn.KernelFunction)
        assert getattr(f.backward, "first_order_only", False) and callable(getattr(f.backward, "__wrapped__", None)), f
