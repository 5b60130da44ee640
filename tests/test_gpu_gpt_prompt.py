"""GPU: the prompt key/value cache of the transformer backbone -- lipvq_gpt_attention_prefix_f32 (csrc/lipvq_gpt.hip),
GPTBackbone.prefill / forward_cached / PromptedGPTBackbone (gpt.py), ICLInputEmbedding.prompt_embedding (embedding.py) and
icl.PromptedPolicy.

What is pinned is BIT equality with the uncached path: the attention of Lq new tokens over P cached keys plus their own must
give the bits lipvq_gpt_attention_f32 gives for rows P.. of the concatenated tensor (the same tiles of the
concatenated key index, the same chains; a trailing masked tile adds exp(-inf) = 0 and 0 * v), and the cached module the bits
of the full forward's last Lq rows (Linear and LayerNorm rows do not depend on their position).  Beside that every result is
held to the float64 bounds of tests/test_gpu_gpt.py: a forward tensor within 1e-5 of the reference's maximum magnitude, the
module within max(1e-5, 4 x the fixture's own fp32-vs-float64 deviation).  Every figure is printed before it is asserted.
"""
import numpy as np
import pytest
import torch

import gpt_bf16_ref
import gpt_ref
from fenced import _Fenced

pytestmark = pytest.mark.gpu

FWD_TOL, REF_FACTOR = 1e-5, 4.0
H = 2
# (P, Lq): no prefix; one key each; the ICRT step; a prefix ending one short of, on and one past a key-tile edge (the last with
# new tokens up to the next edge); two query tiles; a full context in two halves; the last query tile alone; one token at the limit
PLQ = [(0, 5), (1, 1), (20, 10), (31, 1), (32, 1), (33, 31), (2, 33), (64, 64), (96, 32), (127, 1)]


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def _ref64(qkv, P):
    """Rows P.. of the float64 causal attention over the whole of qkv."""
    return gpt_ref.attention_ref(qkv.double(), H, gpt_ref.causal_mask(qkv.shape[1]))[:, P:]


def _check(ops, tag, qkv, P, bp1=False):
    """The two conditions of every kernel case: the bits of the full kernel's rows P.., and the float64 bound.  Returns out."""
    qc = qkv.cuda()
    prefix, new = qc[:(1 if bp1 else None), :P].contiguous(), qc[:, P:].contiguous()
    out = ops.gpt_attention_prefix(prefix, new, H)
    assert out.shape == (qkv.shape[0], qkv.shape[1] - P, qkv.shape[2] // 3)
    full = ops.gpt_attention(qc, H, True)[0]
    e = _rel(out.cpu(), _ref64(qkv, P))
    same = torch.equal(out, full[:, P:])
    print(f"{tag}: error {e:.3e} (bound {FWD_TOL:.0e}), bits of the full kernel's rows: {same}")
    assert same, tag
    assert e <= FWD_TOL, (tag, e)
    return out


# ---------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,Lq", PLQ)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dh", [16, 32, 64])
def test_prefix_attention_has_the_full_kernels_bits(ops, dh, B, P, Lq):
    g = torch.Generator().manual_seed(100000 * dh + 1000 * P + 10 * Lq + B)
    qkv = torch.randn(B, P + Lq, 3 * H * dh, generator=g)
    _check(ops, f"prefix attention dh={dh} B={B} P={P} Lq={Lq}", qkv, P)


@pytest.mark.parametrize("P,Lq", [(1, 1), (20, 10), (33, 31), (2, 33), (96, 32)])
@pytest.mark.parametrize("dh", [16, 32, 64])
def test_one_shared_prompt_equals_its_expansion(ops, dh, P, Lq):
    B = 3
    g = torch.Generator().manual_seed(7 * dh + 1000 * P + Lq)
    qkv = torch.randn(B, P + Lq, 3 * H * dh, generator=g)
    qkv[:, :P] = qkv[:1, :P]                                          # one prompt, B different suffixes
    shared = _check(ops, f"shared prompt dh={dh} P={P} Lq={Lq}", qkv, P, bp1=True)
    qc = qkv.cuda()
    expanded = ops.gpt_attention_prefix(qc[:1, :P].expand(B, P, qkv.shape[2]), qc[:, P:], H)
    assert torch.equal(shared, expanded)
    other = qkv.clone()
    other[1:, :P] = torch.randn(B - 1, P, qkv.shape[2], generator=g)  # ... which the other sequences really read
    oc = other.cuda()
    assert not torch.equal(ops.gpt_attention_prefix(oc[:, :P].contiguous(), oc[:, P:].contiguous(), H)[1:], shared[1:])


@pytest.mark.parametrize("P,Lq", [(20, 10), (2, 33), (33, 31), (96, 32), (127, 1), (0, 5)])
@pytest.mark.parametrize("dh", [16, 32, 64])
def test_kernel_writes_its_output_and_nothing_else(ops, dh, P, Lq):
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    B, E = 3, H * dh
    g = torch.Generator().manual_seed(31 * dh + 1000 * P + Lq)
    qc = torch.randn(B, P + Lq, 3 * E, generator=g).cuda()
    prefix, new = qc[:, :P].contiguous(), qc[:, P:].contiguous()
    out = _Fenced(f"out dh={dh} P={P} Lq={Lq}", B, Lq, E)
    _capi.check(_capi.lib.lipvq_gpt_attention_prefix_f32(prefix.data_ptr() if P else None, new.data_ptr(), out.ptr(), B, B, P, Lq, E, H,
                                                         lipvq_vae_amd.ops._stream()), "lipvq_gpt_attention_prefix_f32")
    torch.cuda.synchronize()
    assert torch.equal(out.check(), ops.gpt_attention(qc, H, True)[0][:, P:])


def _peaked(dh, B, P, Lq, key, g):
    """Every query is 1 + 0.25 N(0, 1) in every coordinate and key `key` is 4 in every coordinate: its scaled score is
    4 sqrt(dh) + N(0, 1) >= 16 - 5 while the other keys' are N(0, ~1): it takes nearly the whole softmax of every query open to it."""
    E = H * dh
    qkv = torch.randn(B, P + Lq, 3 * E, generator=g)
    qkv[..., :E] = 0.25 * qkv[..., :E] + 1.0
    qkv[:, key, E:2 * E] = 4.0
    return qkv


def _weight_of(qkv, dh, key):
    """The float64 softmax weight of key `key` in every (b, h, row >= key): the premise of the peaked cases."""
    B, L, E = qkv.shape[0], qkv.shape[1], H * dh
    q, k = (qkv[..., i * E:(i + 1) * E].double().view(B, L, H, dh).transpose(1, 2) for i in (0, 1))
    sc = (q @ k.transpose(-2, -1) / dh ** 0.5).masked_fill(gpt_ref.causal_mask(L) == 0, float("-inf"))
    return torch.softmax(sc, -1)[:, :, key:, key]


@pytest.mark.parametrize("P,Lq", [(20, 10), (33, 31), (64, 64)])
@pytest.mark.parametrize("dh", [16, 32, 64])
def test_peaked_and_uniform_rows(ops, dh, P, Lq):
    B, E = 2, H * dh
    g = torch.Generator().manual_seed(13 * dh + 1000 * P + Lq)
    for what, key in (("a prefix key", P // 2), ("a new key", P + Lq // 2)):
        qkv = _peaked(dh, B, P, Lq, key, g)
        w = float(_weight_of(qkv, dh, key).min())
        print(f"peaked on {what} dh={dh} P={P} Lq={Lq}: the key's smallest softmax weight {w:.6f}")
        assert w >= 0.99, "the case is not peaked"
        _check(ops, f"peaked on {what} dh={dh} P={P} Lq={Lq}", qkv, P)
    qkv = torch.randn(B, P + Lq, 3 * E, generator=g)
    qkv[..., :E] = 0.0                                                # all scores equal: row P + iq is the mean of values 0 .. P + iq
    out = _check(ops, f"uniform dh={dh} P={P} Lq={Lq}", qkv, P)
    n = torch.arange(1, P + Lq + 1, dtype=torch.float64).view(1, -1, 1)
    assert _rel(out.cpu(), (qkv[..., 2 * E:].double().cumsum(1) / n)[:, P:]) <= FWD_TOL


def test_degenerate_calls_and_refusals(ops):
    from lipvq_vae_amd._capi import LipvqLibraryError
    E = 2 * 16
    z = lambda *s: torch.zeros(*s, device="cuda")                     # noqa: E731
    assert ops.gpt_attention_prefix(z(3, 20, 3 * E), z(3, 0, 3 * E), 2).shape == (3, 0, E)         # Lq = 0
    assert ops.gpt_attention_prefix(z(0, 20, 3 * E), z(0, 10, 3 * E), 2).shape == (0, 10, E)       # B = 0
    assert ops.gpt_attention_prefix(z(1, 20, 3 * E), z(0, 10, 3 * E), 2).shape == (0, 10, E)
    with pytest.raises(LipvqLibraryError, match="128"):
        ops.gpt_attention_prefix(z(1, 100, 3 * E), z(1, 29, 3 * E), 2)                             # P + Lq = 129
    with pytest.raises(LipvqLibraryError, match="head width"):
        ops.gpt_attention_prefix(z(1, 20, 3 * 16), z(1, 10, 3 * 16), 2)                            # head width 8
    with pytest.raises(LipvqLibraryError, match="Bp"):
        ops.gpt_attention_prefix(z(2, 20, 3 * E), z(3, 10, 3 * E), 2)                              # Bp = 2 with B = 3
    with pytest.raises(ValueError):
        ops.gpt_attention_prefix(z(3, 20, 3 * E), z(3, 10, 3 * 2 * E), 2)                          # widths differ
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------

MODULE_CASES = [("gpt_icrt", 20), ("gpt_small", 8), ("gpt_small", 11), ("gpt_small", 0), ("gpt_len3", 2)]
_full = {}


def _module(golden_dir, name):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gpt import GPTBackbone
    g = np.load(golden_dir / f"{name}.npz", allow_pickle=False)
    cfg = {k: int(g[k]) for k in ("seed", "B", "L", "E", "H", "layers", "causal")}
    torch.manual_seed(cfg["seed"])
    net = GPTBackbone(embed_dim=cfg["E"], context_length=cfg["L"], causal=bool(cfg["causal"]), num_layers=cfg["layers"],
                      num_heads=cfg["H"], attn_dropout=0.0, block_output_dropout=0.0)
    assert gpt_ref.state_hash(net.state_dict()) == str(g["params_sha256"]), "seeded parameters differ from the fixture's"
    return net.cuda().eval(), g, cfg


def _shared(golden_dir, name):
    """(net, fixture, x, the full fp32 forward of x): built once per fixture and left unchanged (tests that touch parameters or
    the precision build their own)."""
    if name not in _full:
        net, g, cfg = _module(golden_dir, name)
        x = torch.from_numpy(g["x"]).cuda()
        with torch.no_grad():
            _full[name] = (net, g, x, net(x))
    return _full[name]


@pytest.mark.parametrize("name,P", MODULE_CASES)
def test_cached_forward_against_the_float64_fixture(golden_dir, name, P):
    net, g, x, _ = _shared(golden_dir, name)
    cache = net.prefill(x[:, :P])
    assert cache.P == P and cache.Bp == x.shape[0] and cache.precision == "fp32" and len(cache.qkv) == net.num_layers
    assert all(t.shape == (x.shape[0], P, 3 * net.embed_dim) for t in cache.qkv)
    assert cache.nbytes == net.num_layers * x.shape[0] * P * 3 * net.embed_dim * 4
    out = net.forward_cached(x[:, P:], cache)
    assert out.shape == x[:, P:].shape and not out.requires_grad
    e = _rel(out.cpu(), g["out64"][:, P:])
    bound = max(FWD_TOL, REF_FACTOR * float(g["dev/out"]))
    print(f"{name} P={P}: cached out error {e:.3e}, reference's own {float(g['dev/out']):.3e}, bound {bound:.3e}")
    assert e <= bound


@pytest.mark.parametrize("name,P", MODULE_CASES)
def test_cached_forward_has_the_full_forwards_bits(golden_dir, name, P):
    net, g, x, full = _shared(golden_dir, name)
    out = net.forward_cached(x[:, P:], net.prefill(x[:, :P]))
    d = float((out - full[:, P:]).abs().max())
    print(f"{name} P={P}: largest |cached - full| = {d:.3e}")
    assert torch.equal(out, full[:, P:])


@pytest.mark.parametrize("name,P", [("gpt_icrt", 20), ("gpt_small", 8)])
def test_one_cache_serves_many_suffixes_and_many_sequences(golden_dir, name, P):
    net, g, x, full = _shared(golden_dir, name)
    B = x.shape[0]
    cache = net.prefill(x[:, :P])
    x2 = torch.cat([x[:, :P], torch.randn(x[:, P:].shape, generator=torch.Generator().manual_seed(P)).cuda()], 1)
    with torch.no_grad():
        full2 = net(x2)
    assert torch.equal(net.forward_cached(x2[:, P:], cache), full2[:, P:])
    assert torch.equal(net.forward_cached(x[:, P:], cache), full[:, P:])          # ... and the cache is left as it was
    # one prompt for every sequence: a Bp = 1 cache against the same prompt expanded to B
    xs = torch.cat([x[:1, :P].expand(B, P, x.shape[2]), x[:, P:]], 1).contiguous()
    one = net.prefill(xs[:1, :P])
    assert one.Bp == 1 and one.nbytes * B == cache.nbytes
    with torch.no_grad():
        assert torch.equal(net.forward_cached(xs[:, P:], one), net(xs)[:, P:])
    assert torch.equal(net.forward_cached(xs[:, P:], one), net.forward_cached(xs[:, P:], net.prefill(xs[:, :P])))
    # fewer new tokens than the context has room for
    short = net.forward_cached(x[:, P:P + 1], cache)
    assert torch.equal(short, full[:, P:P + 1])                                    # (causal: row P does not see the rows after it)


def test_cached_forward_in_bf16_mode(golden_dir):
    """The bound of tests/test_gpu_gemm_bf16.py for the module's output: 2 e0, e0 = the distance of the float64 emulation of the
    mode from the float64 fixture -- here for the distance of the cached bf16 rows from the full bf16 forward's, and from the
    fixture's.  The cached rows also have the full forward's BITS; every Linear of this fixture runs the 32 tile
    on both sides -- tests/test_gpu_gemm_bf16_tiles.py repeats the comparison where the two sides use different tiles."""
    net, g, cfg = _module(golden_dir, "gpt_small")
    P = 8
    out64 = torch.from_numpy(g["out64"])
    sd64 = {k: v.double().cpu() for k, v in net.state_dict().items()}
    emu = gpt_bf16_ref.gpt_forward_bf16(sd64, torch.from_numpy(g["x"]).double(), cfg["layers"], cfg["H"])
    e0 = float((emu - out64).abs().max() / out64.abs().max())
    x = torch.from_numpy(g["x"]).cuda()
    with torch.no_grad():
        fp32 = net.forward_cached(x[:, P:], net.prefill(x[:, :P]))
        net.set_matmul_precision("bf16")
        full = net(x)
    cache = net.prefill(x[:, :P])
    assert cache.precision == "bf16"
    out = net.forward_cached(x[:, P:], cache)
    d = float((out - full[:, P:]).abs().max() / full.abs().max())
    e = float((out.cpu().double() - out64[:, P:]).abs().max() / out64.abs().max())
    print(f"gpt_small bf16 P={P}: |cached - full bf16| = {d:.3e}, cached error to float64 {e:.3e}, e0 = {e0:.3e} (bound 2 e0); "
          f"cached == full bf16 in bits: {torch.equal(out, full[:, P:])}")
    assert not torch.equal(out, fp32), "the cached path ignored the matmul precision"
    assert torch.equal(out, full[:, P:])        # a bf16 Linear row does not depend on the rows around it
    assert d <= 2 * e0
    assert e <= 2 * e0


def test_refusals(golden_dir):
    net, g, cfg = _module(golden_dir, "gpt_small")                    # B = 3, context 12
    x = torch.from_numpy(g["x"]).cuda()
    cache = net.prefill(x[:, :8])
    with pytest.raises(ValueError, match="context_length"):
        net.forward_cached(torch.cat([x[:, 8:], x[:, :1]], 1), cache)                 # 8 + 5 > 12
    with pytest.raises(ValueError, match="context_length"):
        net.prefill(torch.cat([x, x[:, :1]], 1))
    with pytest.raises(ValueError, match="prompts"):
        net.forward_cached(x[:, 8:], net.prefill(x[:2, :8]))                          # Bp = 2 with B = 3
    net.train()
    with pytest.raises(RuntimeError, match="eval"):
        net.prefill(x[:, :8])
    with pytest.raises(RuntimeError, match="eval"):
        net.forward_cached(x[:, 8:], cache)
    net.eval()
    net.set_matmul_precision("bf16")
    with pytest.raises(RuntimeError, match="precision"):
        net.forward_cached(x[:, 8:], cache)
    net.set_matmul_precision("fp32")
    good = net.forward_cached(x[:, 8:], cache)
    with torch.no_grad():
        net.nets["output_ln"].bias.add_(1.0)                          # what an optimizer step does: in place, the version moves
    with pytest.raises(RuntimeError, match="prefill"):
        net.forward_cached(x[:, 8:], cache)
    cache = net.prefill(x[:, :8])                                     # a new prefill serves the new parameters
    with torch.no_grad():
        assert torch.equal(net.forward_cached(x[:, 8:], cache), net(x)[:, 8:])
    assert not torch.equal(net.forward_cached(x[:, 8:], cache), good)
    net.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    with pytest.raises(RuntimeError, match="prefill"):
        net.forward_cached(x[:, 8:], cache)
    loose, g2, _ = _module(golden_dir, "gpt_noncausal")
    x2 = torch.from_numpy(g2["x"]).cuda()
    with pytest.raises(ValueError, match="non-causal"):
        loose.prefill(x2[:, :8])
    with pytest.raises(ValueError, match="non-causal"):
        loose.forward_cached(x2[:, 8:], cache)


@pytest.mark.parametrize("name,P", [("gpt_icrt", 20), ("gpt_small", 8)])
def test_graph_replay_of_a_cached_step_equals_eager(golden_dir, name, P):
    from lipvq_vae_amd.gpt import PromptedGPTBackbone
    from lipvq_vae_amd.nnfn import GraphedEval
    net, g, x, full = _shared(golden_dir, name)
    cache = net.prefill(x[:, :P])
    step = PromptedGPTBackbone(net, cache)
    assert not step.training
    graphed = GraphedEval(step, torch.zeros_like(x[:, P:]))
    new = x[:, P:].contiguous()
    for xin in (new, new.flip(0) * 0.5, new):
        assert torch.equal(graphed(xin), net.forward_cached(xin, cache))
    assert torch.equal(graphed(new), full[:, P:])
    with pytest.raises(ValueError):
        graphed(new[:, :1])


# ---------------------------------------------------------------------------------------------------
# embedding and policy glue
# ---------------------------------------------------------------------------------------------------

T, E_POL, DIN, K = 3, 64, 16, 32


def _policy_parts(seed):
    from lipvq_vae_amd.embedding import ICLInputEmbedding
    from lipvq_vae_amd.gmm import GMMActionHead
    from lipvq_vae_amd.gpt import GPTBackbone
    torch.manual_seed(seed)
    emb = ICLInputEmbedding(DIN, E_POL, T, emb_dropout=0.1)
    with torch.no_grad():
        emb.params["embed_timestep"].normal_()
    net = GPTBackbone(E_POL, 3 * T, num_layers=2, num_heads=4)
    head = GMMActionHead(E_POL, 7)
    return emb.cuda().eval(), net.cuda().eval(), head.cuda().eval()


def _policy_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    obs, ctx_obs, ctx_act = (torch.randn(B, T, DIN, generator=g).cuda() for _ in range(3))
    idx = torch.randint(0, K, (B, T), generator=g).cuda()
    return obs, ctx_obs, ctx_act, idx, torch.randn(K, DIN, generator=g).cuda()


def test_prompt_embedding_is_the_first_2t_positions():
    emb, _, _ = _policy_parts(11)
    obs, ctx_obs, ctx_act, idx, book = _policy_inputs(4, 12)
    with torch.no_grad():
        for kw in (dict(context_actions=ctx_act), dict(action_indices=idx, codebook=book)):
            prompt = emb.prompt_embedding(ctx_obs, **kw)
            assert prompt.shape == (4, 2 * T, E_POL)
            assert torch.equal(torch.cat([prompt, emb.input_embedding(obs)], 1), emb(obs, ctx_obs, **kw))


def test_prompted_policy_equals_the_uncached_chain():
    from lipvq_vae_amd.icl import PromptedPolicy
    emb, net, head = _policy_parts(21)
    B = 5
    obs, ctx_obs, ctx_act, idx, book = _policy_inputs(B, 22)
    actions = torch.randn(B, T, 7, generator=torch.Generator().manual_seed(23)).cuda()
    policy = PromptedPolicy(emb, net, head)
    with pytest.raises(RuntimeError, match="set_prompt"):
        policy.features(obs)
    for kw in (dict(context_actions=ctx_act), dict(action_indices=idx, codebook=book)):
        with torch.no_grad():
            want = net(emb(obs, ctx_obs, **kw))[:, 2 * T:]
            want_lp = head.log_prob(want, actions)
        cache = policy.set_prompt(ctx_obs, **kw)
        assert cache.P == 2 * T and cache.Bp == B
        feats = policy.features(obs)
        assert feats.shape == (B, T, E_POL) and torch.equal(feats, want)
        with torch.no_grad():
            assert torch.equal(head.log_prob(feats, actions), want_lp)
        obs2 = obs.flip(0) * 0.5                                      # the next step: new frames, the same prompt
        with torch.no_grad():
            assert torch.equal(policy.features(obs2), net(emb(obs2, ctx_obs, **kw))[:, 2 * T:])
    act = policy(obs)
    assert act.shape == (B, T, 7) and torch.isfinite(act).all()
    # one context for all environments
    policy.set_prompt(ctx_obs[:1], ctx_act[:1])
    with torch.no_grad():
        want = net(emb(obs, ctx_obs[:1].expand(B, T, DIN), ctx_act[:1].expand(B, T, DIN)))[:, 2 * T:]
    assert policy.cache.Bp == 1 and torch.equal(policy.features(obs), want)
    emb.train()
    with pytest.raises(RuntimeError, match="eval"):
        policy.set_prompt(ctx_obs, ctx_act)
    with pytest.raises(RuntimeError, match="eval"):
        policy.features(obs)
