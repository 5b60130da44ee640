"""GPU: the backbone's in-kernel dropout (GPTBackbone.set_dropout_source("kernel"); include/lipvq.h, "in-kernel dropout").

Every claim is an equality of bits.  The yardstick is the keep-byte path the library already has: a kernel that draws its
decisions itself must give what the existing kernel gives when it is handed the same decisions as mask bytes (materialised by
ops.dropout_keep, which tests/test_dropout_host.py's numpy restatement holds through ops.dropout_keep_host), and a module
forward under the kernel source must give what the existing Functions give with those masks applied explicitly."""
import numpy as np
import pytest
import torch

from fenced import _Fenced

pytestmark = pytest.mark.gpu

SEED = 2 ** 63 + 20240607          # (above 2^63: the state holds it as a bit pattern)
ATT_SHAPES = [(2, 33, 2, 16), (1, 128, 1, 64), (3, 30, 8, 64), (2, 1, 2, 32)]          # (B, L, H, head width)
ATT_PS = (0.1, 0.5, 0.999)
LN_N, LN_E = (1, 5, 130), (4, 36, 512, 1024)
LN_PS = (0.1, 0.5)
EPS = 1e-5


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _snap(seed, step=0):
    words = [v - 2 ** 64 if v >= 2 ** 63 else v for v in (seed & (2 ** 64 - 1), step & (2 ** 64 - 1))]
    return torch.tensor(words, dtype=torch.int64).cuda()


def _inv_keep(p):
    return float(np.float32(1.0) / np.float32(1.0 - p))


def _scale(ops, snap, site, rows, cols, p):
    """mask_f * inv_keep as an fp32 [rows, cols] tensor: inv_keep where kept, 0 where dropped."""
    return ops.dropout_keep(snap, site, rows, cols, p).float() * _inv_keep(p)


def _randn(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


# ---------------------------------------------------------------------------------------------------
# 1. the materialised mask
# ---------------------------------------------------------------------------------------------------

def test_device_mask_equals_host_mask(ops):
    fields = [(B * H * L, L) for B, L, H, _ in ATT_SHAPES] + [(N, E) for N in LN_N for E in LN_E] + [(7, 33), (3, 5)]
    for k, (rows, cols) in enumerate(fields):
        for p in ATT_PS:
            for seed, step, site in ((SEED, 0, k), (12345, 2 ** 32 + 7, 4 * k + 2)):
                dev = ops.dropout_keep(_snap(seed, step), site, rows, cols, p)
                host = ops.dropout_keep_host(seed, step, site, rows, cols, p)
                assert dev.shape == (rows, cols) and torch.equal(dev.cpu(), host), (rows, cols, p, seed, step, site)


def test_begin_snapshots_and_advances(ops):
    state = _snap(SEED, 41)
    snap = ops.dropout_begin(state)
    assert snap.data_ptr() != state.data_ptr()
    assert snap.tolist() == [SEED - 2 ** 64, 41] and state.tolist() == [SEED - 2 ** 64, 42]
    assert ops.dropout_begin(state).tolist() == [SEED - 2 ** 64, 42] and snap.tolist() == [SEED - 2 ** 64, 41]
    wrap = _snap(3, 2 ** 63 - 1)                                     # (the step is a 64-bit counter; its low 32 bits are what is used)
    ops.dropout_begin(wrap)
    assert wrap.tolist() == [3, -2 ** 63]


# ---------------------------------------------------------------------------------------------------
# 2. attention forward and backward
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,L,H,dh", ATT_SHAPES)
def test_attention_equals_the_keep_byte_form(ops, B, L, H, dh, causal):
    E = H * dh
    qkv, gout = _randn(1, B, L, 3 * E), _randn(2, B, L, E)
    plain_out, plain_lse = ops.gpt_attention(qkv, H, causal)
    for p in ATT_PS:
        site = 4
        snap = _snap(SEED, 3)
        keep = ops.dropout_keep(snap, site, B * H * L, L, p).view(B, H, L, L)
        want_out, want_lse = ops.gpt_attention(qkv, H, causal, keep, 1.0 - p)
        want_g = ops.gpt_attention_bwd(qkv, want_out, gout, want_lse, H, causal, keep, 1.0 - p)
        out, lse = ops.gpt_attention(qkv, H, causal, dropout=(snap, site, p))
        g = ops.gpt_attention_bwd(qkv, out, gout, lse, H, causal, dropout=(snap, site, p))
        tag = (B, L, H, dh, causal, p)
        assert torch.equal(out, want_out), tag
        assert torch.equal(lse, want_lse) and torch.equal(lse, plain_lse), tag          # (dropout acts after the softmax)
        assert torch.equal(g, want_g), tag
        assert torch.isfinite(g).all() and not torch.equal(out, plain_out)
        if p == 0.999:                                              # a query row with every open key dropped: a zero output row
            open_ = torch.ones(L, L, dtype=torch.bool, device="cuda").tril() if causal else torch.ones(L, L, dtype=torch.bool, device="cuda")
            dead = ((keep.bool() & open_).sum(-1) == 0)              # [B, H, L]
            assert bool(dead.any()), (tag, "the fixture has no query row with every key dropped")
            rows = out.view(B, L, H, dh).permute(0, 2, 1, 3)[dead]
            assert rows.numel() > 0 and not bool(rows.any()), tag
            assert torch.equal(lse[dead], plain_lse[dead])
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.gpt_attention(qkv, H, causal, keep, 0.5, dropout=(snap, 0, 0.5))
    with pytest.raises(ValueError):
        ops.gpt_attention(qkv, H, causal, dropout=(snap, 0, 1.0))


# ---------------------------------------------------------------------------------------------------
# 3. add + dropout + LayerNorm, outputs fenced
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", LN_E)
@pytest.mark.parametrize("N", LN_N)
def test_add_dropout_layernorm_equals_the_explicit_mask(ops, N, E):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd._capi import check, lib
    stream = lambda: torch.cuda.current_stream().cuda_stream          # noqa: E731
    a, b, gy, gres = (_randn(10 + k, N, E, scale=s) for k, s in enumerate((1.0, 0.7, 1.0, 0.5)))
    w, bias = 1.0 + _randn(20, E, scale=0.1), _randn(21, E, scale=0.1)
    for p in LN_PS:
        for want_s in (True, False):
            site, snap = 6, _snap(SEED, 9)
            m = _scale(ops, snap, site, N, E, p)
            s0, y0, xhat0, rstd0 = ops.gpt_layernorm(a, b * m, w, bias, EPS, want_s=want_s, save=True)
            gs0, gw0, gb0 = ops.gpt_layernorm_bwd(gy, xhat0, rstd0, w, gres if want_s else None)
            f = {k: _Fenced(k, N, E) for k in ("y", "xhat", "gs", "gbranch")}
            f.update(rstd=_Fenced("rstd", N), gw=_Fenced("gw", E), gb=_Fenced("gb", E))
            if want_s:
                f["s"] = _Fenced("s", N, E)
            nbytes = lib.lipvq_gpt_layernorm_bwd_workspace_bytes(N, E)
            ws = _Fenced("workspace", nbytes // 4)
            check(lib.lipvq_gpt_layernorm_drop_f32(a.data_ptr(), b.data_ptr(), w.data_ptr(), bias.data_ptr(), EPS, snap.data_ptr(), site, p,
                                                   f["s"].ptr() if want_s else None, f["y"].ptr(), f["xhat"].ptr(), f["rstd"].ptr(), N, E,
                                                   stream()), "lipvq_gpt_layernorm_drop_f32")
            check(lib.lipvq_gpt_layernorm_bwd_drop_f32(gy.data_ptr(), f["xhat"].ptr(), f["rstd"].ptr(), w.data_ptr(),
                                                       gres.data_ptr() if want_s else None, snap.data_ptr(), site, p, f["gs"].ptr(),
                                                       f["gbranch"].ptr(), f["gw"].ptr(), f["gb"].ptr(), ws.ptr(), N, E, stream()),
                  "lipvq_gpt_layernorm_bwd_drop_f32")
            torch.cuda.synchronize()
            ws.check()
            got = {k: v.check() for k, v in f.items()}
            tag = (N, E, p, want_s)
            want = dict(y=y0, xhat=xhat0, rstd=rstd0, gs=gs0, gw=gw0, gb=gb0, gbranch=gs0 * m)
            if want_s:
                want["s"] = s0
            for k, v in want.items():
                assert torch.equal(got[k], v), (tag, k)
            # and through ops
            s1, y1, xhat1, rstd1 = ops.gpt_layernorm(a, b, w, bias, EPS, want_s=want_s, save=True, dropout=(snap, site, p))
            assert (s1 is None) == (not want_s) and torch.equal(y1, y0) and torch.equal(xhat1, xhat0) and torch.equal(rstd1, rstd0)
            gs1, gbr1, gw1, gb1 = ops.gpt_layernorm_bwd(gy, xhat1, rstd1, w, gres if want_s else None, dropout=(snap, site, p))
            assert torch.equal(gs1, gs0) and torch.equal(gbr1, gs0 * m) and torch.equal(gw1, gw0) and torch.equal(gb1, gb0)


# ---------------------------------------------------------------------------------------------------
# 4. the module against a reference forward over the existing Functions
# ---------------------------------------------------------------------------------------------------

def _small_net(seed=7, attn=0.1, out=0.1):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gpt import GPTBackbone
    torch.manual_seed(seed)
    return GPTBackbone(64, 12, num_layers=2, num_heads=4, attn_dropout=attn, block_output_dropout=out).cuda()


def _golden_net(golden_dir):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gpt import GPTBackbone
    g = np.load(golden_dir / "gpt_small.npz", allow_pickle=False)
    cfg = {k: int(g[k]) for k in ("seed", "B", "L", "E", "H", "layers", "causal")}
    torch.manual_seed(cfg["seed"])
    net = GPTBackbone(embed_dim=cfg["E"], context_length=cfg["L"], causal=bool(cfg["causal"]), num_layers=cfg["layers"],
                      num_heads=cfg["H"], attn_dropout=0.1, block_output_dropout=0.1).cuda()
    return net, cfg["B"]


def _reference_forward(net, x, seed, step):
    """GPTBackbone's training forward over the EXISTING Functions: keep bytes into _AttentionFn, b * (mask_f * inv_keep) branches
    through torch, every mask materialised from (seed, step, site = 4 layer + 0 / 1 / 2)."""
    from lipvq_vae_amd import ops
    from lipvq_vae_amd.gpt import _AttentionFn
    from lipvq_vae_amd.nnfn import AddLayerNormFn, LinearFn
    from lipvq_vae_amd.ops import ACT_GELU, ACT_NONE
    B, L, E, H, prec = x.shape[0], net.context_length, net.embed_dim, net.num_heads, net.matmul_precision
    snap = _snap(seed, step)
    a, b = x, None
    for i, blk in enumerate(net.nets["transformer"]):
        att, mlp, ln1, ln2 = blk.nets["attention"], blk.nets["mlp"], blk.nets["ln1"], blk.nets["ln2"]
        p_att, p_out, p_mlp = float(att.nets["attn_dropout"].p), float(att.nets["output_dropout"].p), float(mlp[3].p)
        if b is None:
            s, y = a, AddLayerNormFn.apply(a, None, ln1.weight, ln1.bias, ln1.eps, False)[1]
        else:
            s, y = AddLayerNormFn.apply(a, b, ln1.weight, ln1.bias, ln1.eps, True)
        qkv = LinearFn.apply(y, att.nets["qkv"].weight, None, ACT_NONE, prec)
        keep = ops.dropout_keep(snap, 4 * i, B * H * L, L, p_att).view(B, H, L, L)
        o = _AttentionFn.apply(qkv, H, bool(net.causal), keep, 1.0 - p_att)
        o = LinearFn.apply(o, att.nets["output"].weight, att.nets["output"].bias, ACT_NONE, prec)
        o = o * _scale(ops, snap, 4 * i + 1, B * L, E, p_out).view(B, L, E)
        s, y = AddLayerNormFn.apply(s, o, ln2.weight, ln2.bias, ln2.eps, True)
        f = LinearFn.apply(y, mlp[0].weight, mlp[0].bias, ACT_GELU, prec)
        f = LinearFn.apply(f, mlp[2].weight, mlp[2].bias, ACT_NONE, prec)
        f = f * _scale(ops, snap, 4 * i + 2, B * L, E, p_mlp).view(B, L, E)
        a, b = s, f
    ln = net.nets["output_ln"]
    return AddLayerNormFn.apply(a, b, ln.weight, ln.bias, ln.eps, False)[1]


def _run(net, forward, x0, R):
    for p in net.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    out = forward(x)
    (out * R).sum().backward()
    return out.detach(), x.grad, {k: p.grad.clone() for k, p in net.named_parameters()}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("which", ["two_layer", "gpt_small"])
def test_module_equals_the_reference_forward(golden_dir, which, precision):
    net, B = (_small_net(), 3) if which == "two_layer" else _golden_net(golden_dir)
    net.set_matmul_precision(precision).set_dropout_source("kernel").train()
    x0, R = _randn(31, B, net.context_length, net.embed_dim), _randn(32, B, net.context_length, net.embed_dim)
    s = 987654321
    net.reseed_dropout(s)
    out, gx, grads = _run(net, net, x0, R)
    assert net.dropout_state.tolist() == [s, 1]
    ref_out, ref_gx, ref_grads = _run(net, lambda x: _reference_forward(net, x, s, 0), x0, R)
    assert torch.equal(out, ref_out) and torch.equal(gx, ref_gx)
    assert set(grads) == set(ref_grads)
    for k in grads:
        assert torch.equal(grads[k], ref_grads[k]), k
    net.eval()
    with torch.no_grad():
        assert not torch.equal(net(x0), out), "dropout changed nothing: the reference comparison would be empty"


# ---------------------------------------------------------------------------------------------------
# 5. state
# ---------------------------------------------------------------------------------------------------

def test_state_advances_reseeds_and_stays_out_of_eval(ops, monkeypatch):
    net = _small_net().set_dropout_source("kernel", seed=5).train()
    x = _randn(41, 3, 12, 64)
    state = net.dropout_state
    assert state.is_cuda and state.tolist() == [5, 0]
    y1 = net(x)
    assert state.tolist() == [5, 1]
    y2 = net(x)
    assert state.tolist() == [5, 2] and not torch.equal(y1, y2)
    net.reseed_dropout(5)
    assert net.dropout_state is state and state.tolist() == [5, 0]
    assert torch.equal(net(x), y1) and torch.equal(net(x), y2)
    net.reseed_dropout(5, step=1)
    assert torch.equal(net(x), y2)
    net.reseed_dropout(6)
    assert not torch.equal(net(x), y1)
    with torch.no_grad():                                            # a forward without a graph advances the step too, same bits
        net.reseed_dropout(5)
        assert torch.equal(net(x), y1.detach()) and state.tolist() == [5, 1]
    # the masks of layer 0 and layer 1 differ (the site enters the counter)
    snap = _snap(5, 0)
    for k in range(3):
        assert not torch.equal(ops.dropout_keep(snap, k, 36, 64, 0.1), ops.dropout_keep(snap, 4 + k, 36, 64, 0.1))
    # eval: no begin launch, the state stays, and the bits are those of the "torch"-source eval forward
    begins = []
    begin = ops.dropout_begin
    monkeypatch.setattr(ops, "dropout_begin", lambda st: begins.append(1) or begin(st))
    net.eval()
    before = state.tolist()
    with torch.no_grad():
        y_eval = net(x)
    assert not begins and state.tolist() == before
    net.set_dropout_source("torch")
    with torch.no_grad():
        assert torch.equal(net(x), y_eval)
    net.set_dropout_source("kernel").train()
    net(x)
    assert len(begins) == 1 and state.tolist() == [before[0], before[1] + 1]
    # .to() moves the state with the module; state_dict() does not hold it
    assert "_dropout_state" not in net.state_dict() and net.cpu().dropout_state.device.type == "cpu"


def test_p_of_one_is_refused_under_the_kernel_source():
    net = _small_net().set_dropout_source("kernel").train()
    net.nets["transformer"][0].nets["attention"].nets["attn_dropout"].p = 1.0
    with pytest.raises(ValueError, match="0 <= p < 1"):
        net(_randn(43, 2, 12, 64))


def test_p_of_zero_means_no_dropout():
    net = _small_net(attn=0.0, out=0.0).set_dropout_source("kernel").train()
    x = _randn(44, 2, 12, 64)
    y = net(x)
    net.set_dropout_source("torch")
    assert torch.equal(net(x), y)


# ---------------------------------------------------------------------------------------------------
# 6. torch's generators are not used
# ---------------------------------------------------------------------------------------------------

def test_torch_rng_is_not_used(monkeypatch):
    net = _small_net().set_dropout_source("kernel", seed=3).train()
    x = _randn(51, 3, 12, 64).requires_grad_(True)
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("the kernel dropout source called torch's RNG")
    monkeypatch.setattr(torch, "rand", refuse)
    monkeypatch.setattr(torch.nn.functional, "dropout", refuse)
    cpu_state, cuda_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    net(x).square().sum().backward()
    torch.cuda.synchronize()
    assert x.grad is not None and all(p.grad is not None for p in net.parameters())
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), cuda_state)
    monkeypatch.undo()
    net.set_dropout_source("torch")
    net(x)
    assert not torch.equal(torch.cuda.get_rng_state(), cuda_state), "the torch source does draw from the CUDA generator"


# ---------------------------------------------------------------------------------------------------
# 7. the graphed training step
# ---------------------------------------------------------------------------------------------------

def _policy(seed, source, p):
    from lipvq_vae_amd.action_head import ActionHead
    net = _small_net(seed, attn=p, out=p)
    torch.manual_seed(seed + 1)
    head = ActionHead(64, 7).cuda()
    return net.set_dropout_source(source, seed=77 if source == "kernel" else None).train(), head.train()


@pytest.mark.parametrize("source,p", [("kernel", 0.1), ("torch", 0.0)])
def test_graphed_policy_step_replays_the_eager_steps(source, p):
    """Replay k = eager step k, losses and parameters, bit for bit: under the kernel source with the dropout state in extra_state
    (the warm-up steps advance it; the snapshot puts it back), and as before without extra_state on a torch-source backbone."""
    from lipvq_vae_amd import optim
    from lipvq_vae_amd.icl import GraphedPolicyStep
    B, L, T, A = 3, 12, 4, 7

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(B, L, 64, generator=g).cuda(), (torch.rand(B, T, A, generator=g) * 3.0 - 1.5).cuda()

    runs = []
    for graphed in (False, True):
        net, head = _policy(61, source, p)
        params = list(net.parameters()) + list(head.parameters())
        opt = optim.Adam(params, lr=torch.tensor(1e-3, device="cuda"), max_grad_norm=1.0)
        loss_fn = lambda x, a: head.losses(net(x)[:, -T:], a)["action_loss"]      # noqa: E731
        if graphed:
            start = [q.detach().clone() for q in params]
            extra = dict(extra_state=[net.dropout_state]) if source == "kernel" else {}
            step = GraphedPolicyStep(loss_fn, params, opt, batch(0), warmup=3, **extra)
            assert all(torch.equal(q.detach(), s) for q, s in zip(params, start))
            if source == "kernel":                                   # (the capture records its begin launch, it does not run it)
                assert net.dropout_state.tolist() == [77, 0], "construction advanced the dropout state"
        record = []
        for k in (1, 2, 3):
            x, a = batch(k)
            if graphed:
                loss, _ = step.step(x, a)
            else:
                opt.zero_grad(set_to_none=True)
                loss = loss_fn(x, a)
                loss.backward()
                opt.step()
            record.append([loss.detach().clone()] + [q.detach().clone() for q in params])
            if source == "kernel":
                assert net.dropout_state.tolist() == [77, k]
        runs.append(record)
    for k, (eager, replay) in enumerate(zip(*runs), 1):
        assert all(torch.equal(a, b) for a, b in zip(eager, replay)), f"replay {k} differs from eager step {k}"
    assert not torch.equal(runs[0][0][0], runs[0][1][0])


# ---------------------------------------------------------------------------------------------------
# 8. the autograd contract of the two new Functions
# ---------------------------------------------------------------------------------------------------

def test_new_functions_are_marked_first_order_only():
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd import gpt, nnfn
    for f in (nnfn.AddLayerNormFn, gpt._AttentionFn):
        assert issubclass(f, nnfn.KernelFunction)
        assert getattr(f.backward, "first_order_only", False) and callable(getattr(f.backward, "__wrapped__", None)), f


def _leaf(t, need):
    return t.detach().clone().requires_grad_(need)


def test_add_drop_layernorm_fn_contract(ops):
    from lipvq_vae_amd.nnfn import AddLayerNormFn
    N, E, p, site = 5, 36, 0.5, 2
    a0, b0, Rs, Ry = (_randn(70 + k, N, E) for k in range(4))
    w0, bias0 = 1.0 + _randn(75, E, scale=0.1), _randn(76, E, scale=0.1)
    snap = _snap(SEED, 2)
    m = _scale(ops, snap, site, N, E, p)

    def run(needs, use_s=True, use_y=True, twice=False):
        lv = [_leaf(t, n) for t, n in zip((a0, b0, w0, bias0), needs)]
        s, y = AddLayerNormFn.apply(*lv, EPS, True, (snap, site, p))
        obj = sum(t for t, u in (((s * Rs).sum(), use_s), ((y * Ry).sum(), use_y)) if u)
        obj.backward(retain_graph=twice)
        if twice:
            obj.backward()
        return s.detach(), y.detach(), [t.grad for t in lv]

    s, y, full = run((True,) * 4)
    s_again, _, again = run((True,) * 4)
    assert torch.equal(s, s_again) and all(torch.equal(g, h) for g, h in zip(full, again)), "two identical runs differ"
    s0, y0, xhat, rstd = ops.gpt_layernorm(a0, b0 * m, w0, bias0, EPS, want_s=True, save=True)
    gs, gw, gb = ops.gpt_layernorm_bwd(Ry, xhat, rstd, w0, Rs)
    assert torch.equal(s, s0) and torch.equal(y, y0)
    for got, want in zip(full, (gs, gs * m, gw, gb)):
        assert torch.equal(got, want)
    for needs in ((True, False, False, False), (False, True, True, False), (False, False, False, True)):
        _, _, part = run(needs)
        for g, f, n in zip(part, full, needs):
            assert (g is None) == (not n) and (g is None or torch.equal(g, f)), needs
    _, _, twice = run((True,) * 4, twice=True)                       # the mask is regenerated from snap: the same bits again
    assert all(torch.equal(t, 2.0 * f) for t, f in zip(twice, full))
    _, _, only_s = run((True,) * 4, use_y=False)                     # y unused: a None upstream gradient
    assert torch.equal(only_s[0], Rs) and torch.equal(only_s[1], Rs * m)
    _, _, only_y = run((True,) * 4, use_s=False)
    gs_y = ops.gpt_layernorm_bwd(Ry, xhat, rstd, w0, None)[0]
    assert torch.equal(only_y[0], gs_y) and torch.equal(only_y[1], gs_y * m)
    with torch.no_grad():
        s_ng, y_ng = AddLayerNormFn.apply(_leaf(a0, True), b0, w0, bias0, EPS, True, (snap, site, p))
    assert torch.equal(s_ng, s) and torch.equal(y_ng, y) and not y_ng.requires_grad
    lv = [_leaf(t, True) for t in (a0, b0, w0, bias0)]
    y2 = AddLayerNormFn.apply(*lv, EPS, True, (snap, site, p))[1]
    ga, = torch.autograd.grad(y2.sum(), lv[0], create_graph=True)
    assert ga.requires_grad
    with pytest.raises(RuntimeError, match="differentiable once only|once_differentiable"):
        (y2.sum() + ga.square().sum()).backward()


def test_attention_drop_fn_contract(ops):
    from lipvq_vae_amd.gpt import _AttentionFn
    B, L, H, dh, p, site = 2, 33, 2, 16, 0.5, 8
    qkv0, R = _randn(80, B, L, 3 * H * dh), _randn(81, B, L, H * dh)
    snap = _snap(SEED, 4)
    keep = ops.dropout_keep(snap, site, B * H * L, L, p).view(B, H, L, L)

    def run(twice=False):
        q = _leaf(qkv0, True)
        out = _AttentionFn.apply(q, H, True, None, 1.0, (snap, site, p))
        obj = (out * R).sum()
        obj.backward(retain_graph=twice)
        if twice:
            obj.backward()
        return out.detach(), q.grad

    out, g = run()
    out_again, g_again = run()
    assert torch.equal(out, out_again) and torch.equal(g, g_again), "two identical runs differ"
    q = _leaf(qkv0, True)
    want = _AttentionFn.apply(q, H, True, keep, 1.0 - p)
    (want * R).sum().backward()
    assert torch.equal(out, want.detach()) and torch.equal(g, q.grad)
    assert torch.equal(run(twice=True)[1], 2.0 * g)
    frozen = _AttentionFn.apply(qkv0, H, True, None, 1.0, (snap, site, p))
    with torch.no_grad():
        no_grad = _AttentionFn.apply(_leaf(qkv0, True), H, True, None, 1.0, (snap, site, p))
    assert not frozen.requires_grad and torch.equal(frozen, out) and torch.equal(no_grad, out)
    q = _leaf(qkv0, True)
    o2 = _AttentionFn.apply(q, H, True, None, 1.0, (snap, site, p))
    gq, = torch.autograd.grad(o2.sum(), q, create_graph=True)
    assert gq.requires_grad
    with pytest.raises(RuntimeError, match="differentiable once only|once_differentiable"):
        (o2.sum() + gq.square().sum()).backward()
