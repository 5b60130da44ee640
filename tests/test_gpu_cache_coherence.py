"""GPU: every cache of derived state against every writer of the parameters under it (tests/cache_coherence_cases.py).

For each tested (writer, consumer) pair: run the consumer (every cache is now warm with pre-write state), apply the writer, run
the consumer again and compare it, with ``torch.equal``, with a fresh twin loaded from the written module's state_dict().  A stale
copy gives well-formed but wrong tokens or features, so two conditions are asserted BEFORE the module's post-write output is
looked at: the consumer takes the route that reads the cache (``_plan`` / ``fused_shape``), and the twin's post-write output
differs from the module's own pre-write output in at least 5 % of the rows (indices) or elements (floats) -- otherwise a stale
cache would pass.  Consumers that must REFUSE after a write (PromptCache, PromptedPolicy, the tokenizer's backward) and captured
graphs that must SEE an in-place write have their own tests below; the three defects found by reading the code have named ones.
"""
import numpy as np
import pytest
import torch

import cache_coherence_cases as C

pytestmark = pytest.mark.gpu

POWER = 0.05


def _run(cname, rig, data):
    return tuple(t.detach().clone() for t in C.CONSUMERS[cname].fn(rig, data))


def _differs(a, b):
    """Fraction of the rows (integer outputs) or elements (float outputs) in which two outputs differ."""
    if a.dim() == 0:
        return float(not torch.equal(a, b))
    ne = a != b
    if not a.is_floating_point() and ne.dim() > 1:
        ne = ne.reshape(ne.shape[0], -1).any(1)
    return float(ne.float().mean())


def _assert_power(tag, ref, pre):
    for i, (r, p) in enumerate(zip(ref, pre)):
        f = _differs(r, p)
        print(f"{tag}[{i}]: the twin differs from the pre-write output in {100 * f:.1f} % (needs {100 * POWER:.0f} %)")
        assert f >= POWER, f"{tag}[{i}]: the write is too small to tell a stale cache ({f:.3f})"


def _assert_equal(tag, got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), f"{tag}[{i}]: differs from the twin in {100 * _differs(g, w):.1f} %"


def _check_route(rig, data, cname):
    """The consumer takes the cached route it is in the table for (tests/test_tokenizer_routes_host.py reads the same plan)."""
    c = C.CONSUMERS[cname]
    if c.route is None:
        return
    from lipvq_vae_amd.tokenizer import FUSED
    entry, key, mode, want = c.route
    tok, n = rig.tok, data[key].shape[0]
    assert tok.fused_shape()
    plan = tok._plan(n, entry, mode=mode)
    assert plan.route == want[type(tok).__name__], (cname, plan)
    assert plan.fast == (mode == "fast")
    if key == "x_big":                      # the smallest batch whose forward is the fused launch
        assert tok._plan(n - 1, "forward").route != FUSED and tok._plan(n, "forward").route == FUSED


def _group(subject, wname, oracle, consumers=None, target=None):
    """Warm, write, compare for every value consumer paired with the writer on the subject.  Returns what a caller may go on with."""
    w = C.WRITERS[wname]
    rig, data = C.build(subject, oracle)
    consumers = C.value_consumers(wname, subject) if consumers is None else consumers
    assert consumers
    state = w.prepare(rig, data) if w.prepare else None
    for cn in consumers:
        _check_route(rig, data, cn)
    pre = {cn: _run(cn, rig, data) for cn in consumers}
    for cn in consumers:                                             # a second call reads the warm caches: same bits
        _assert_equal(f"{wname}/{cn} warm", _run(cn, rig, data), pre[cn])
    ret = w.fn(rig if target is None else getattr(rig, target), data, state)
    written = rig
    if w.kind == "copy":
        for cn in consumers:
            _assert_equal(f"{wname}/{cn}: the original moved", _run(cn, rig, data), pre[cn])
        written = ret
    twin = C.twin_of(subject, written)
    ref = {cn: _run(cn, twin, data) for cn in consumers}
    for cn in consumers:
        if w.kind == "none":
            _assert_equal(f"{wname}/{cn}: a toggle changed the twin", ref[cn], pre[cn])
        else:
            _assert_power(f"{subject}/{wname}/{cn}", ref[cn], pre[cn])
    post = {cn: _run(cn, written, data) for cn in consumers}
    for cn in consumers:
        _check_route(written, data, cn)
        _assert_equal(f"{subject}/{wname}/{cn}", post[cn], ref[cn])
    return dict(rig=written, data=data, state=state, pre=pre, post=post, twin=twin)


def _close(got, ref, tol=1e-5):
    """tests/test_gpu_embed.py's tolerance for ops.linear."""
    return np.all(np.abs(got.astype(np.float64) - ref) <= tol * (1.0 + np.abs(ref)))


def _anchor(ns, oracle):
    """The absolute references, once: parity tokenize against the oracle (as tests/test_gpu_random_shapes.py compares it), the
    code table against float64 -- a common error of module and twin cannot hide behind their equality."""
    rig, data, post = ns["rig"], ns["data"], ns["post"]
    p = {k: v.detach().cpu().numpy() for k, v in rig.tok.state_dict().items()}
    cb = rig.tok._codebook().detach().cpu().numpy()
    if type(rig.tok).__name__ == "LLFQVAE_V4":
        for key in [k for k in ("big", "small") if "tokenize_" + k in post]:
            ze = oracle.llfq_encode(p, data["x_" + key].cpu().numpy())
            idx_ref, zq_ref, _ = oracle.nearest(ze, cb)
            idx, zq = post["tokenize_" + key]
            assert np.array_equal(idx.cpu().numpy(), idx_ref) and np.array_equal(zq.cpu().numpy(), zq_ref), key
    lin = rig.emb.nets["embed_encoder"]
    W, b = lin.weight.detach().cpu().numpy().astype(np.float64), lin.bias.detach().cpu().numpy().astype(np.float64)
    assert _close(post["code_table"][0].cpu().numpy(), cb.astype(np.float64) @ W.T + b)


def _matrix():
    return [(s, wn) for s in ("llfq", "vq", "bin") for wn, w in C.WRITERS.items()
            if w.scope in ("params", "codebook") and C.value_consumers(wn, s)]


@pytest.mark.parametrize("subject,wname", _matrix())
def test_consumer_after_writer_equals_a_fresh_twin(oracle, no_screen_monitor, subject, wname):
    ns = _group(subject, wname, oracle)
    if wname == "load_state_dict" and subject != "bin":
        _anchor(ns, oracle)


# ---------------------------------------------------------------------------------------------------------------------------
# the two graphed steps (one capture per test)
# ---------------------------------------------------------------------------------------------------------------------------

def test_validation_between_graphed_tokenizer_steps(oracle, no_screen_monitor):
    """Defect 1: a replayed AdamW step bumps no version; GraphedTokenizerStep.step invalidated the MODEL's caches alone, so the
    embedding's code table (keyed on the codebook's data_ptr / version) and the backward's version check missed the write."""
    import lipvq_vae_amd
    ns = _group("icrt", "graphed_tokenizer_step", oracle)
    rig = ns["rig"]
    lin = rig.emb.nets["embed_encoder"]
    first, table = ns["pre"]["code_table"][0], ns["post"]["code_table"][0]
    want = lipvq_vae_amd.ops.linear(rig.tok._codebook().detach(), lin.weight.detach(), lin.bias.detach())
    assert torch.equal(table, want), "code_table after three graphed steps is not the table of the current codebook"
    assert not torch.equal(table, first)
    _anchor(ns, oracle)


def test_backward_after_a_graphed_replay_refuses(oracle, no_screen_monitor):
    """Defect 1, second half: eager forward, one replay, backward -- the backward kernels would read the replay's weights."""
    rig, data = C.build("icrt", oracle)
    graphed = C.WRITERS["graphed_tokenizer_step"].prepare(rig, data)
    _, loss = rig.tok(data["x_small"])
    graphed.step(data["x_small"])
    with pytest.raises(RuntimeError, match="modified in place"):
        loss.backward()


def test_graphed_policy_step(oracle, no_screen_monitor):
    """GraphedPolicyStep bumps every version itself: the embedding's table, the prompt cache and the prompted policy see it."""
    from lipvq_vae_amd.icl import PromptedPolicy
    w = C.WRITERS["graphed_policy_step"]
    consumers = C.value_consumers("graphed_policy_step", "policy")
    assert set(consumers) == {"code_table", "embedding_forward", "prompt_embedding"}
    rig, data = C.build("policy", oracle)
    graphed = w.prepare(rig, data)
    policy = PromptedPolicy(rig.emb, rig.net, lambda f: f)
    kw = dict(action_indices=data["aidx"], codebook=rig.tok._codebook())
    cache = policy.set_prompt(data["ctx_obs"], **kw)
    pre = {cn: _run(cn, rig, data) for cn in consumers}
    pre_feats = policy.features(data["obs"]).clone()
    w.fn(rig, data, graphed)
    twin = C.twin_of("policy", rig)
    for cn in consumers:
        ref = _run(cn, twin, data)
        _assert_power(f"policy/graphed_policy_step/{cn}", ref, pre[cn])
        _assert_equal(f"policy/graphed_policy_step/{cn}", _run(cn, rig, data), ref)
    with torch.no_grad():
        want = twin.net(twin.emb(data["obs"], data["ctx_obs"], action_indices=data["aidx"], codebook=twin.tok._codebook()))[:, 2 * C.T_CTX:]
    _assert_power("policy/graphed_policy_step/policy_features", (want,), (pre_feats,))
    with pytest.raises(RuntimeError, match="prefill"):
        rig.net.forward_cached(rig.emb.input_embedding(data["obs"]).detach(), cache)
    with pytest.raises(RuntimeError, match="set_prompt"):
        policy.features(data["obs"])
    policy.set_prompt(data["ctx_obs"], **kw)
    assert torch.equal(policy.features(data["obs"]), want)


# ---------------------------------------------------------------------------------------------------------------------------
# consumers that must refuse
# ---------------------------------------------------------------------------------------------------------------------------

def _refusing(cname, subject="policy"):
    return [wn for wn, cn, subjects in C.tested("raise") if cn == cname and subject in subjects
            and C.WRITERS[wn].scope in ("params", "codebook")]


def _apply(wname, rig, data, target):
    """The writer on one part of the rig (codebook maintenance: on the rig, it writes the tokenizer's codebook)."""
    w = C.WRITERS[wname]
    if w.scope == "codebook":
        return w.fn(rig, data, w.prepare(rig, data) if w.prepare else None)
    return w.fn(getattr(rig, target), data, None)


@pytest.mark.parametrize("wname", [wn for wn in _refusing("forward_cached") if C.WRITERS[wn].scope == "params"])
def test_prompt_cache_after_a_write_to_the_backbone(oracle, wname):
    """Defect 3, the ``.data`` case among them: ``p.data = new`` keeps every version, so a cache keyed on versions alone stayed
    "valid"; a deep copy carries the original's versions, so it accepted the original's cache."""
    w = C.WRITERS[wname]
    rig, data = C.build("policy", oracle)
    net, P = rig.net, 2 * C.T_CTX
    x = torch.randn(3, 3 * C.T_CTX, C.E_POL, generator=torch.Generator().manual_seed(5)).cuda()
    cache = net.prefill(x[:, :P])
    pre = net.forward_cached(x[:, P:], cache).clone()
    ret = _apply(wname, rig, data, "net")
    if w.kind in ("none", "copy"):
        assert torch.equal(net.forward_cached(x[:, P:], cache), pre)          # nothing moved: the cache still serves
        if w.kind == "copy":
            with pytest.raises((RuntimeError, ValueError), match="prefill|another backbone"):
                ret.forward_cached(x[:, P:], cache)
        return
    net = rig.net
    twin = C.twin_of("policy", rig)
    with torch.no_grad():
        want = twin.net(x)[:, P:]
    _assert_power(f"policy/{wname}/forward_cached", (want,), (pre,))
    with pytest.raises(RuntimeError, match="prefill"):
        net.forward_cached(x[:, P:], cache)
    assert torch.equal(net.forward_cached(x[:, P:], net.prefill(x[:, :P])), want)


def test_prompt_cache_of_another_backbone_is_refused(oracle):
    """Defect 3, the foreign-cache case: two backbones of one shape, each loaded once, carry identical version tuples."""
    a, _ = C.build("policy", oracle, seed=1)
    b, _ = C.build("policy", oracle, seed=2)
    for rig in (a, b):
        rig.net.load_state_dict({k: v.clone() for k, v in rig.net.state_dict().items()})
    assert [p._version for p in a.net.parameters()] == [p._version for p in b.net.parameters()]
    assert not torch.equal(a.net.nets["transformer"][0].nets["mlp"][0].weight, b.net.nets["transformer"][0].nets["mlp"][0].weight)
    x = torch.randn(3, 3 * C.T_CTX, C.E_POL, generator=torch.Generator().manual_seed(6)).cuda()
    P = 2 * C.T_CTX
    cache = a.net.prefill(x[:, :P])
    with pytest.raises((RuntimeError, ValueError), match="another backbone"):
        b.net.forward_cached(x[:, P:], cache)
    with torch.no_grad():
        assert torch.equal(a.net.forward_cached(x[:, P:], cache), a.net(x)[:, P:])


def _policy_cases():
    """(writer, written part): codebook maintenance writes the tokenizer alone."""
    return [(wn, t) for wn in _refusing("policy_features") for t in ("emb", "tok", "net")
            if (C.WRITERS[wn].scope == "params" or t == "tok") and (wn, "policy_features", t) not in C.PART_NOT_PAIRED]


@pytest.mark.parametrize("wname,target", _policy_cases())
def test_prompted_policy_after_a_write(oracle, wname, target):
    """Defect 2: PromptCache.versions covers the backbone alone; a write to the embedding (Linear, LayerNorm, time table) or to
    the codebook that set_prompt embedded went unnoticed and the stale prompt keys and values were served.  ``fused_adamw`` on
    ``emb`` and on ``tok`` are the two named cases."""
    from lipvq_vae_amd.icl import PromptedPolicy
    w = C.WRITERS[wname]
    rig, data = C.build("policy", oracle)
    policy = PromptedPolicy(rig.emb, rig.net, lambda f: f)
    kw = lambda r: dict(action_indices=data["aidx"], codebook=r.tok._codebook())      # noqa: E731
    policy.set_prompt(data["ctx_obs"], **kw(rig))
    pre = policy.features(data["obs"]).clone()
    _apply(wname, rig, data, target)
    if w.kind in ("none", "copy"):
        assert torch.equal(policy.features(data["obs"]), pre)
        return
    twin = C.twin_of("policy", rig)
    with torch.no_grad():
        want = twin.net(twin.emb(data["obs"], data["ctx_obs"], **kw(twin)))[:, 2 * C.T_CTX:]
    _assert_power(f"policy/{wname}@{target}/policy_features", (want,), (pre,))
    with pytest.raises(RuntimeError, match="set_prompt"):
        policy.features(data["obs"])
    policy.set_prompt(data["ctx_obs"], **kw(rig))
    assert torch.equal(policy.features(data["obs"]), want)


@pytest.mark.parametrize("subject", ["llfq", "vq"])
@pytest.mark.parametrize("wname", _refusing("tokenizer_backward", "llfq"))
def test_backward_refuses_after_a_write(oracle, no_screen_monitor, subject, wname):
    """The backward kernels read the module's LIVE weights: any write between forward and backward must raise."""
    rig, data = C.build(subject, oracle)
    w = C.WRITERS[wname]
    state = w.prepare(rig, data) if w.prepare else None
    _, loss = rig.tok(data["x_small"])
    assert loss.requires_grad
    w.fn(rig if w.scope == "codebook" else rig.tok, data, state)
    with pytest.raises(RuntimeError, match="modified in place"):
        loss.backward()


# ---------------------------------------------------------------------------------------------------------------------------
# captured graphs that must see an in-place write
# ---------------------------------------------------------------------------------------------------------------------------

def _replayed(cname):
    return [wn for wn, cn, _ in C.tested("replay") if cn == cname]


@pytest.mark.parametrize("cname", ["graphed_gpt_replay", "graphed_eval_replay"])
def test_graph_replay_sees_in_place_writes(oracle, cname):
    from lipvq_vae_amd.gpt import GraphedGPTBackbone
    from lipvq_vae_amd.nnfn import GraphedEval
    rig, data = C.build("policy", oracle)
    g = torch.Generator().manual_seed(8)
    if cname == "graphed_gpt_replay":
        x = torch.randn(3, 3 * C.T_CTX, C.E_POL, generator=g).cuda()
        graphed, eager, part = GraphedGPTBackbone(rig.net, x), (lambda r: r.net(x)), "net"
    else:
        x = data["obs"]
        ctx_act = torch.randn(x.shape, generator=g).cuda()
        graphed = GraphedEval(C.DensePolicy(rig, data["ctx_obs"], ctx_act), x)
        eager, part = (lambda r: C.DensePolicy(r, data["ctx_obs"], ctx_act)(x)), None
    writers = _replayed(cname)
    assert len(writers) >= 6 and all(C.WRITERS[wn].kind == "inplace" for wn in writers)
    last = graphed(x).clone()
    for wn in writers:
        C.WRITERS[wn].fn(rig if part is None else getattr(rig, part), data, None)
        twin = C.twin_of("policy", rig)
        with torch.no_grad():
            want = eager(twin)
        _assert_power(f"policy/{wn}/{cname}", (want,), (last,))
        last = graphed(x).clone()
        assert torch.equal(last, want), wn
