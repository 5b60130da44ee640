"""GPU: the transformer backbone (reference robomimic/models/transformers.py:80-439) on the HIP library.

Per kernel: lipvq_gpt_attention_f32 / _bwd_f32 and lipvq_gpt_layernorm_f32 / _bwd_f32 against a float64 torch evaluation of the
same op (tests/gpt_ref.py on .double() tensors), with the bounds tests/test_gpu_default.py established: a forward tensor within
1e-5 of the reference's maximum magnitude, a gradient within 1e-4.

Whole module: GPTBackbone against the float64 columns of tests/golden/gpt_*.npz.  The bound is the larger of the per-kernel
tolerance and 4 x the fp32 reference's own deviation from float64 stored in that fixture (a different but equally accurate
summation order and erf over 6 x 4 GEMMs); every figure is printed before it is asserted.  This file reads tests/golden only.
Every kernel input here is torch.randn; the non-random inputs, tile edges and fenced outputs are tests/test_gpu_xf_edges.py.
"""
import numpy as np
import pytest
import torch

import gpt_ref

pytestmark = pytest.mark.gpu

CASES = ("gpt_icrt", "gpt_small", "gpt_noncausal", "gpt_len3")
FWD_TOL, BWD_TOL, REF_FACTOR = 1e-5, 1e-4, 4.0


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


# ---------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B", [1, 8, 257])
@pytest.mark.parametrize("L", [1, 3, 30, 33, 96, 128])
@pytest.mark.parametrize("dh", [16, 32, 64])
def test_attention_forward_backward(ops, dh, L, B, causal, drop):
    H = 8 if B == 8 else 2                       # (8 heads at the step batch; 2 keep the float64 evaluation of B = 257 small)
    E = H * dh
    g = torch.Generator().manual_seed(1000 * dh + 10 * L + B + 2 * causal + drop)
    qkv = torch.randn(B, L, 3 * E, generator=g)
    gout = torch.randn(B, L, E, generator=g)
    keep = (torch.rand(B, H, L, L, generator=g) >= 0.1).to(torch.uint8) if drop else None
    kp = 0.9 if drop else 1.0
    qd = qkv.double().requires_grad_(True)
    ref = gpt_ref.attention_ref(qd, H, gpt_ref.causal_mask(L, causal), keep, kp)
    (ref * gout.double()).sum().backward()
    kc = keep.cuda() if drop else None
    qc = qkv.cuda()
    out, lse = ops.gpt_attention(qc, H, causal, kc, kp)
    e_out = _rel(out.cpu(), ref.detach())
    gq = ops.gpt_attention_bwd(qc, out, gout.cuda(), lse, H, causal, kc, kp)
    e_gq = _rel(gq.cpu(), qd.grad)
    print(f"attention dh={dh} L={L} B={B} causal={causal} drop={drop}: out {e_out:.3e} gqkv {e_gq:.3e}")
    assert e_out <= FWD_TOL
    assert e_gq <= BWD_TOL
    # lse is the log-sum-exp of the masked scaled scores
    q, k = qd.detach()[..., :E].view(B, L, H, dh).transpose(1, 2), qd.detach()[..., E:2 * E].view(B, L, H, dh).transpose(1, 2)
    sc = (q @ k.transpose(-2, -1)) / np.sqrt(dh)
    if causal:
        sc = sc.masked_fill(gpt_ref.causal_mask(L) == 0, float("-inf"))
    assert np.abs(lse.cpu().double().numpy() - torch.logsumexp(sc, -1).numpy()).max() <= 1e-5 * max(1.0, float(sc[sc > -1e30].abs().max()))
    # no atomics: a second backward gives the same bits
    assert torch.equal(gq, ops.gpt_attention_bwd(qc, out, gout.cuda(), lse, H, causal, kc, kp))


def test_attention_degenerate_and_unsupported(ops):
    from lipvq_vae_amd._capi import LipvqLibraryError
    for B, L in ((0, 30), (4, 0)):
        qkv = torch.zeros(B, L, 3 * 128, device="cuda")
        out, lse = ops.gpt_attention(qkv, 8, True)
        assert out.shape == (B, L, 128) and lse.shape == (B, 8, L)
        assert ops.gpt_attention_bwd(qkv, out, torch.zeros_like(out), lse, 8, True).shape == qkv.shape
    with pytest.raises(LipvqLibraryError, match="128"):
        ops.gpt_attention(torch.zeros(1, 129, 3 * 128, device="cuda"), 8, True)
    with pytest.raises(LipvqLibraryError, match="head width"):
        ops.gpt_attention(torch.zeros(1, 16, 3 * 64, device="cuda"), 8, True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("N,E", [(1, 8), (37, 8), (70000, 8), (3, 64), (240, 64), (70000, 64), (1, 512), (240, 512), (20000, 512),
                                 (5, 1024), (240, 1024), (20000, 1024), (7, 260)])
def test_layernorm_forward_backward(ops, N, E, with_b):
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(N + E)
    a, b = torch.randn(N, E, generator=g), torch.randn(N, E, generator=g)
    w, bias = torch.randn(E, generator=g), torch.randn(E, generator=g)
    gy, gres = torch.randn(N, E, generator=g), torch.randn(N, E, generator=g)
    ad, wd, biasd = (t.double().requires_grad_(True) for t in (a, w, bias))
    sd = ad + b.double() if with_b else ad * 1.0
    sd.retain_grad()
    ref = F.layer_norm(sd, (E,), wd, biasd, 1e-5)
    ((ref * gy.double()).sum() + (sd * gres.double()).sum()).backward()           # s also feeds the residual stream: gres arrives there
    ac, wc = a.cuda(), w.cuda()
    s, y, xhat, rstd = ops.gpt_layernorm(ac, b.cuda() if with_b else None, wc, bias.cuda(), 1e-5, want_s=True, save=True)
    e_s, e_y = _rel(s.cpu(), sd.detach()), _rel(y.cpu(), ref.detach())
    gs, gw, gb = ops.gpt_layernorm_bwd(gy.cuda(), xhat, rstd, wc, gres.cuda())
    e_gs, e_gw, e_gb = _rel(gs.cpu(), sd.grad), _rel(gw.cpu(), wd.grad), _rel(gb.cpu(), biasd.grad)
    print(f"layernorm N={N} E={E} b={with_b}: s {e_s:.3e} y {e_y:.3e} gs {e_gs:.3e} gw {e_gw:.3e} gb {e_gb:.3e}")
    assert e_s == 0.0 or (with_b and e_s <= 1e-7)
    assert e_y <= FWD_TOL
    assert e_gs <= BWD_TOL and e_gw <= BWD_TOL and e_gb <= BWD_TOL
    # without gres the kernel returns LayerNorm's own gradient; s may be left out; the bits repeat
    gs0, gw0, gb0 = ops.gpt_layernorm_bwd(gy.cuda(), xhat, rstd, wc, None)
    assert _rel((gs0 + gres.cuda()).cpu(), sd.grad) <= BWD_TOL and torch.equal(gw0, gw) and torch.equal(gb0, gb)
    s_none, y2 = ops.gpt_layernorm(ac, b.cuda() if with_b else None, wc, bias.cuda(), 1e-5, want_s=False)
    assert s_none is None and torch.equal(y2, y)


def test_layernorm_limits(ops):
    from lipvq_vae_amd._capi import LipvqLibraryError
    for E in (1028, 6):
        with pytest.raises(LipvqLibraryError, match="multiple of 4"):
            ops.gpt_layernorm(torch.zeros(4, E, device="cuda"), None, torch.ones(E, device="cuda"), torch.zeros(E, device="cuda"), 1e-5)
    s, y = ops.gpt_layernorm(torch.zeros(0, 512, device="cuda"), None, torch.ones(512, device="cuda"), torch.zeros(512, device="cuda"), 1e-5)
    assert y.shape == (0, 512)


# ---------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------

def _module(golden_dir, name, **kw):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gpt import GPTBackbone
    g = np.load(golden_dir / f"{name}.npz", allow_pickle=False)
    cfg = {k: int(g[k]) for k in ("seed", "B", "L", "E", "H", "layers", "causal")}
    torch.manual_seed(cfg["seed"])
    args = dict(attn_dropout=0.0, block_output_dropout=0.0)
    args.update(kw)
    net = GPTBackbone(embed_dim=cfg["E"], context_length=cfg["L"], causal=bool(cfg["causal"]), num_layers=cfg["layers"],
                      num_heads=cfg["H"], **args)
    assert gpt_ref.state_hash(net.state_dict()) == str(g["params_sha256"]), "seeded parameters differ from the fixture's"
    return net.cuda(), g, cfg


@pytest.mark.parametrize("name", CASES)
def test_module_against_the_float64_fixture(golden_dir, name):
    """Output, input gradient and every stored parameter gradient: error <= max(tolerance, 4 x the fp32 reference's own deviation)."""
    net, g, cfg = _module(golden_dir, name)
    x = torch.from_numpy(g["x"]).cuda()
    net.eval()
    with torch.no_grad():
        out_eval = net(x)
    e = _rel(out_eval.cpu(), g["out64"])
    bound = max(FWD_TOL, REF_FACTOR * float(g["dev/out"]))
    print(f"{name}: out error {e:.3e}, reference's own {float(g['dev/out']):.3e}, ratio {e / float(g['dev/out']):.2f}, bound {bound:.3e}")
    results = [("out", e, bound)]
    net.train()                                                     # all dropout p = 0: the same function, with the autograd graph
    xg = x.clone().requires_grad_(True)
    out = net(xg)
    assert torch.equal(out.detach(), out_eval), "training-mode forward with p = 0 differs from the eval forward"
    (out * gpt_ref.objective_weights(cfg["seed"], out.shape).cuda()).sum().backward()
    e = _rel(xg.grad.cpu(), g["gx64"])
    bound = max(BWD_TOL, REF_FACTOR * float(g["dev/gx"]))
    print(f"{name}: gx error {e:.3e}, reference's own {float(g['dev/gx']):.3e}, ratio {e / float(g['dev/gx']):.2f}, bound {bound:.3e}")
    results.append(("gx", e, bound))
    params = dict(net.named_parameters())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params.values()), "a parameter got no gradient"
    stored = [(n.format(last=cfg["layers"] - 1), None) for n in gpt_ref.STORED_PARAM_GRADS] + list(gpt_ref.STORED_WEIGHT_ROWS)
    for n, rows in stored:
        key = n if rows is None else f"{n}[:{rows}]"
        got = params[n].grad if rows is None else params[n].grad[:rows]
        e, dev = _rel(got.cpu(), g["gp64/" + key]), float(g["dev/gp/" + key])
        bound = max(BWD_TOL, REF_FACTOR * dev)
        print(f"{name}: grad {key} error {e:.3e}, reference's own {dev:.3e}, ratio {e / dev:.2f}, bound {bound:.3e}")
        results.append((key, e, bound))
    for what, e, bound in results:
        assert e <= bound, (what, e, bound)


@pytest.mark.parametrize("name", ["gpt_icrt", "gpt_small"])
def test_causal_outputs_ignore_later_inputs(golden_dir, name):
    net, g, cfg = _module(golden_dir, name)
    net.eval()
    x = torch.from_numpy(g["x"]).cuda()
    with torch.no_grad():
        base = net(x)
        for j in (1, cfg["L"] // 2, cfg["L"] - 1):
            x2 = x.clone()
            x2[:, j:] += torch.randn_like(x2[:, j:])
            out = net(x2)
            assert torch.equal(out[:, :j], base[:, :j]), j
            assert not torch.equal(out[:, j:], base[:, j:])


def test_noncausal_outputs_see_later_inputs(golden_dir):
    net, g, cfg = _module(golden_dir, "gpt_noncausal")
    net.eval()
    x = torch.from_numpy(g["x"]).cuda()
    with torch.no_grad():
        x2 = x.clone()
        x2[:, -1] += 1.0
        assert not torch.equal(net(x2)[:, 0], net(x)[:, 0])


@pytest.mark.parametrize("name", ["gpt_icrt", "gpt_small"])
def test_training_backward_repeats_bit_for_bit(golden_dir, name):
    net, g, cfg = _module(golden_dir, name, attn_dropout=0.1, block_output_dropout=0.1)
    net.train()
    x = torch.from_numpy(g["x"]).cuda()
    r = gpt_ref.objective_weights(cfg["seed"], x.shape).cuda()
    grads = []
    for _ in range(2):
        torch.manual_seed(7)                                        # the same three kinds of dropout mask in both passes
        net.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        (net(xg) * r).sum().backward()
        grads.append([xg.grad.clone()] + [p.grad.clone() for p in net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    net.eval()
    with torch.no_grad():
        assert not torch.equal(net(x), net.train()(x))              # dropout is live in training mode


@pytest.mark.parametrize("name", ["gpt_icrt", "gpt_small"])
def test_graph_replay_equals_eager(golden_dir, name):
    from lipvq_vae_amd.gpt import GraphedGPTBackbone
    net, g, cfg = _module(golden_dir, name)
    net.eval()
    x = torch.from_numpy(g["x"]).cuda()
    graphed = GraphedGPTBackbone(net, torch.zeros_like(x))
    with torch.no_grad():
        for xin in (x, x.flip(0) * 0.5, x):
            assert torch.equal(graphed(xin), net(xin))
    with pytest.raises(ValueError):
        graphed(x[:1])
    with pytest.raises(RuntimeError):
        GraphedGPTBackbone(net.train(), x)
