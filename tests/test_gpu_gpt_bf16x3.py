"""GPU: GPTBackbone.set_matmul_precision("bf16x3") on small backbones -- the gpt_small fixture (E = 64, 4 heads, 2 layers,
context 12, B = 3) and a freshly seeded backbone of the same shape with wider weights.

Accuracy is measured against float64 torch on the CPU (tests/gpt_ref.py with float64 parameters, autograd for the gradients)
for three sides of the same module -- the fp32 path, "bf16", "bf16x3" -- as max |difference| / max |reference| per tensor,
printed before anything is asserted.  Condition: err(bf16x3) <= err(bf16) / 16 for the output, the input gradient and every
parameter gradient that a Linear enters (all but the closing LayerNorm's bias: UNTOUCHED below).  Derivation: per product the two modes lose 2^-8 and 3 2^-16, a ratio of about 85; the fp32 parts the
modes share (attention, LayerNorm, GELU, the accumulations) leave a margin of about 5.  Measured on an MI355X: DESIGN.md
section 4.6.1.

Then what the switch promises: the mode is really taken and leaves nothing behind, gradients repeat bit for bit, the prompt
cache gives the full forward's bits (also where prompt rows and step rows run different tile instances) and refuses a cache of
another precision, and graph replays equal the eager calls.
"""
import numpy as np
import pytest
import torch

import gpt_ref

pytestmark = pytest.mark.gpu

MODES = ("fp32", "bf16", "bf16x3")
# With the objective sum(out * r) the gradient of the closing LayerNorm's bias is the sum of r over the rows: no Linear, and so no
# matmul precision, enters it.  Its error is the same number on all three sides (asserted); "16 times smaller" cannot apply.
UNTOUCHED = "nets.output_ln.bias"


def _fixture_net(golden_dir, name="gpt_small"):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gpt import GPTBackbone
    g = np.load(golden_dir / f"{name}.npz", allow_pickle=False)
    cfg = {k: int(g[k]) for k in ("seed", "B", "L", "E", "H", "layers", "causal")}
    torch.manual_seed(cfg["seed"])
    net = GPTBackbone(embed_dim=cfg["E"], context_length=cfg["L"], causal=bool(cfg["causal"]), num_layers=cfg["layers"],
                      num_heads=cfg["H"], attn_dropout=0.0, block_output_dropout=0.0)
    assert gpt_ref.state_hash(net.state_dict()) == str(g["params_sha256"]), "seeded parameters differ from the fixture's"
    return net, torch.from_numpy(g["x"]), cfg


def _seeded_net():
    """E = 64, 4 heads, 2 layers, context 12, B = 3; weights of std 1 / sqrt(fan_in) and non-zero biases, so that every
    Linear's product is of order one and the rounding of its operands is what the output sees."""
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gpt import GPTBackbone
    cfg = dict(seed=5, B=3, L=12, E=64, H=4, layers=2, causal=1)
    torch.manual_seed(cfg["seed"])
    net = GPTBackbone(embed_dim=64, context_length=12, causal=True, num_layers=2, num_heads=4, attn_dropout=0.0,
                      block_output_dropout=0.0)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.normal_(0.0, m.in_features ** -0.5)
                if m.bias is not None:
                    m.bias.normal_(0.0, 0.1)
            elif isinstance(m, torch.nn.LayerNorm):
                m.weight.normal_(1.0, 0.1)
                m.bias.normal_(0.0, 0.1)
    return net, torch.randn(3, 12, 64), cfg


def _net(golden_dir, which):
    return _fixture_net(golden_dir) if which == "gpt_small" else _seeded_net()


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("which", ["gpt_small", "seeded"])
def test_accuracy_against_float64_on_three_sides(golden_dir, which):
    net, x, cfg = _net(golden_dir, which)
    r = gpt_ref.objective_weights(cfg["seed"], x.shape)
    sd64 = {k: v.detach().double().requires_grad_(True) for k, v in net.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    out64 = gpt_ref.gpt_forward(sd64, x64, cfg["layers"], cfg["H"])
    (out64 * r.double()).sum().backward()
    names = [k for k, _ in net.named_parameters()]
    assert set(names) <= set(sd64) and all(sd64[k].grad is not None for k in names)
    net = net.cuda().train()                                                   # all dropout p = 0: the eval function, with autograd
    err = {}
    for mode in MODES:
        net.set_matmul_precision(mode)
        net.zero_grad(set_to_none=True)
        xg = x.cuda().requires_grad_(True)
        out = net(xg)
        (out * r.cuda()).sum().backward()
        e = {"out": _rel(out.detach().cpu(), out64.detach()), "gx": _rel(xg.grad.cpu(), x64.grad)}
        for k, p in net.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (mode, k)
            e[k] = _rel(p.grad.cpu(), sd64[k].grad)
        err[mode] = e
    worst = {m: max(v for k, v in err[m].items() if k not in ("out", "gx")) for m in MODES}
    for m in MODES:
        print(f"{which} {m:7s}: out {err[m]['out']:.3e}  gx {err[m]['gx']:.3e}  worst parameter gradient {worst[m]:.3e}")
    for k in err["bf16"]:
        print(f"{which} {k}: fp32 {err['fp32'][k]:.3e}  bf16 {err['bf16'][k]:.3e}  bf16x3 {err['bf16x3'][k]:.3e}  "
              f"bf16 / bf16x3 = {err['bf16'][k] / max(err['bf16x3'][k], 1e-300):.1f}")
    for k in err["bf16"]:
        if k == UNTOUCHED:
            assert err["fp32"][k] == err["bf16"][k] == err["bf16x3"][k], k       # the same sum on all three sides
            continue
        assert err["bf16x3"][k] <= err["bf16"][k] / 16, (k, err["bf16x3"][k], err["bf16"][k])


def test_mode_is_taken_and_leaves_nothing_behind(golden_dir):
    net, x, cfg = _fixture_net(golden_dir)
    net, x = net.cuda().eval(), x.cuda()
    with torch.no_grad():
        fp32 = net(x)
        bf16 = net.set_matmul_precision("bf16")(x)
        assert net.set_matmul_precision("bf16x3") is net and net.matmul_precision == "bf16x3"
        x3 = net(x)
        assert not torch.equal(x3, fp32) and not torch.equal(x3, bf16)
        assert torch.equal(net(x), x3)
        assert torch.equal(net.set_matmul_precision("fp32")(x), fp32), "the bf16x3 mode left something behind"
        assert torch.equal(net.set_matmul_precision("bf16")(x), bf16)


def test_gradients_repeat_bit_for_bit(golden_dir):
    net, x, cfg = _seeded_net()
    net = net.cuda().train().set_matmul_precision("bf16x3")
    r = gpt_ref.objective_weights(cfg["seed"], x.shape).cuda()
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        xg = x.cuda().requires_grad_(True)
        out = net(xg)
        (out * r).sum().backward()
        runs.append([out.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in net.parameters()])
    assert len(runs[0]) == 2 + len(list(net.parameters()))
    for i, (p, q) in enumerate(zip(*runs)):
        assert torch.equal(p, q), i


@pytest.mark.parametrize("P", [8, 11, 0])
def test_cached_forward_has_the_full_forwards_bits(golden_dir, P):
    net, x, cfg = _fixture_net(golden_dir)
    net, x = net.cuda().eval().set_matmul_precision("bf16x3"), x.cuda()
    with torch.no_grad():
        full = net(x)
    cache = net.prefill(x[:, :P])
    assert cache.precision == "bf16x3"
    out = net.forward_cached(x[:, P:], cache)
    print(f"gpt_small bf16x3 P={P}: largest |cached - full| = {float((out - full[:, P:]).abs().max()):.3e}")
    assert torch.equal(out, full[:, P:])


def test_cached_backbone_equals_full_across_tiles():
    """B = 128 sequences of 64 tokens, E = 128: the full call's 8192 rows run the four Linears at tiles 64 / 64 / 128 / 64, the
    cached call's 1024 rows at 32 everywhere (asked of the entry point), and forward_cached == net(x)[:, P:] in bits."""
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd import _capi
    from lipvq_vae_amd.gpt import GPTBackbone
    tile = _capi.lib.lipvq_gemm_bf16_tile
    E, L, B, P = 128, 64, 128, 56
    torch.manual_seed(7)
    net = GPTBackbone(embed_dim=E, context_length=L, causal=True, num_layers=1, num_heads=4, attn_dropout=0.0,
                      block_output_dropout=0.0).cuda().eval().set_matmul_precision("bf16x3")
    widths = [m.out_features for m in net.modules() if isinstance(m, torch.nn.Linear)]
    assert widths == [3 * E, E, 4 * E, E]
    assert [tile(B * L, w, 1) for w in widths] == [64, 64, 128, 64]
    assert [tile(B * (L - P), w, 1) for w in widths] == [32, 32, 32, 32]
    x = torch.randn(B, L, E).cuda()
    with torch.no_grad():
        full = net(x)
        out = net.forward_cached(x[:, P:], net.prefill(x[:, :P]))
    assert out.shape == (B, L - P, E) and bool(torch.isfinite(full).all())
    print(f"cached vs full bf16x3, 8192 / 1024 rows: max |difference| = {float((out - full[:, P:]).abs().max()):.3e}")
    assert torch.equal(out, full[:, P:])


def test_a_cache_of_another_precision_is_refused(golden_dir):
    from lipvq_vae_amd.gpt import StalePromptCache
    net, x, cfg = _fixture_net(golden_dir)
    net, x = net.cuda().eval(), x.cuda()
    caches = {}
    for mode in MODES:
        caches[mode] = net.set_matmul_precision(mode).prefill(x[:, :8])
        assert caches[mode].precision == mode
    for mode in MODES:
        net.set_matmul_precision(mode)
        for made, cache in caches.items():
            if made == mode:
                with torch.no_grad():
                    assert torch.equal(net.forward_cached(x[:, 8:], cache), net(x)[:, 8:])
            elif "bf16x3" in (made, mode):
                with pytest.raises(StalePromptCache, match="precision"):
                    net.forward_cached(x[:, 8:], cache)


def test_graph_replays_equal_the_eager_calls(golden_dir):
    from lipvq_vae_amd.gpt import GraphedGPTBackbone, PromptedGPTBackbone
    from lipvq_vae_amd.nnfn import GraphedEval
    net, x, cfg = _fixture_net(golden_dir)
    net, x = net.cuda().eval().set_matmul_precision("bf16x3"), x.cuda()
    graphed = GraphedGPTBackbone(net, torch.zeros_like(x))
    P = 8
    cache = net.prefill(x[:, :P])
    step = GraphedEval(PromptedGPTBackbone(net, cache), torch.zeros_like(x[:, P:]))
    new = x[:, P:].contiguous()
    with torch.no_grad():
        for xin in (x, x.flip(0) * 0.5, x):
            assert torch.equal(graphed(xin), net(xin))
        for xin in (new, new.flip(0) * 0.5, new):
            assert torch.equal(step(xin), net.forward_cached(xin, cache))
        assert torch.equal(step(new), net(x)[:, P:])
        fp32 = net.set_matmul_precision("fp32")(x)
        assert not torch.equal(fp32, graphed(x))                                # the graph keeps the mode it was captured in
