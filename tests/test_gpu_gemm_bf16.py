"""GPU: the bf16 matrix-pipe mode of the transformer's Linears (csrc/lipvq_gemm_bf16.hip; ops.linear_bf16 / linear_nn_bf16 /
wgrad_bf16; nnfn.LinearFn(..., "bf16"); GPTBackbone.set_matmul_precision).

Per kernel the reference is torch float64 on the operands ROUNDED to bf16 (`t.bfloat16().double()`); inputs are randn, so
more than 90 % of their elements change under that rounding (asserted) and neither a truncating convert nor an fp32
fall-through can pass.  With R = sum_k |x^ w^| per output, any-order round-to-nearest fp32 accumulation of the (exact) bf16
products over a reduction of length K stays within (K + 1) 2^-24 R of the float64 value; how the matrix pipe rounds inside a
k-step is not documented, so the tests allow TWICE that.  Every case prints its largest error / RN-bound ratio before it
asserts.  The distance to the product of the UNROUNDED operands is bounded too: each factor moves by at most 2^-9 relative,
a product by 2^-8 (1 + 2^-9).  gb is compared with the float64 column sums of the unrounded g within N 2^-24 sum |g|.

Measured on an MI355X (largest error / RN bound over all cases): see DESIGN.md section 4.6.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gpt_bf16_ref
import gpt_ref
from gemm_bf16_cases import EPS, case as _case, ratio as _ratio, rb as _rb   # shared with test_gpu_gemm_bf16_tiles.py

pytestmark = pytest.mark.gpu

NS = (1, 33, 130, 240)
KJ = ((16, 8), (72, 24), (512, 136), (2048, 512))


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


@pytest.mark.parametrize("K,J", KJ)
@pytest.mark.parametrize("N", NS)
def test_forward_against_float64_on_rounded_operands(ops, N, K, J):
    c = _case(N, K, J)
    xc, Wc, bc = c["x"].cuda(), c["W"].cuda(), c["b"].cuda()
    worst = 0.0
    for with_b in (False, True):
        want = c["y"] + (c["b"].double() if with_b else 0.0)
        for gelu in (False, True):
            tag = f"linear_bf16 N={N} K={K} J={J} bias={with_b} gelu={gelu}"
            if gelu:
                y, pre = ops.linear_bf16(xc, Wc, bc if with_b else None, act=ops.ACT_GELU, save_pre=True)
                ref = F.gelu(pre.cpu().double())
                assert float((y.cpu().double() - ref).abs().max()) <= 1e-5 * max(1e-30, float(ref.abs().max())), tag
            else:
                pre = ops.linear_bf16(xc, Wc, bc if with_b else None)
            assert pre.shape == (N, J)
            worst = max(worst, _ratio(tag, pre, want, c["Ry"], K))
            # ... and the distance to the product of the unrounded operands
            exact = c["y_exact"] + (c["b"].double() if with_b else 0.0)
            slack = 2.0 ** -8 * (1 + 2.0 ** -9) * c["Ry_exact"] + 2 * (K + 1) * EPS * c["Ry"]
            assert bool(((pre.cpu().double() - exact).abs() <= slack).all()), tag
            if K >= 72:                                                         # ... which the rounding really moved
                assert float((pre.cpu().double() - exact).abs().max()) > 64 * EPS * float(exact.abs().max()), tag
    assert worst <= 2.0, worst


@pytest.mark.parametrize("K,J", KJ)
@pytest.mark.parametrize("N", NS)
def test_input_gradient_against_float64_on_rounded_operands(ops, N, K, J):
    c = _case(N, K, J)
    gx = ops.linear_nn_bf16(c["g"].cuda(), c["W"].cuda())
    assert gx.shape == (N, K)
    assert _ratio(f"linear_nn_bf16 N={N} K={K} J={J}", gx, c["gx"], c["Rgx"], J) <= 2.0


@pytest.mark.parametrize("K,J", KJ)
@pytest.mark.parametrize("N", NS)
def test_weight_gradient_against_float64_on_rounded_operands(ops, N, K, J):
    c = _case(N, K, J)
    gW, gb = ops.wgrad_bf16(c["g"].cuda(), c["x"].cuda())
    assert gW.shape == (J, K) and gb.shape == (J,)
    assert _ratio(f"wgrad_bf16 gW N={N} K={K} J={J}", gW, c["gW"], c["RgW"], N) <= 2.0
    e = (gb.cpu().double() - c["gb"]).abs()
    print(f"wgrad_bf16 gb N={N} J={J}: error / (N 2^-24 sum|g|) = {float((e / (N * EPS * c['Rgb'])).max()):.3f}")
    assert bool((e <= N * EPS * c["Rgb"]).all())
    gW2, none = ops.wgrad_bf16(c["g"].cuda(), c["x"].cuda(), want_bias=False)
    assert none is None and torch.equal(gW2, gW)


# ---------------------------------------------------------------------------------------------------
# guard bands and full coverage of the outputs, through the C ABI (the pattern of tests/test_gpu_xf_edges.py)
# ---------------------------------------------------------------------------------------------------

SENTINEL = 0x7FC0DEAD                   # a NaN with a payload: no arithmetic on finite inputs stores this word
PAD = 1024                              # words (4 KiB) of sentinel before and after every output


class _Fenced:
    """An fp32 output of `shape` in the middle of a sentinel-filled int32 buffer."""

    def __init__(self, what, *shape, offset_words=0):
        self.what, self.n = what, int(np.prod(shape))
        self.buf = torch.full((PAD + offset_words + self.n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.words = self.buf[PAD + offset_words:PAD + offset_words + self.n]
        self.t = self.words.view(torch.float32).view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        lo, hi = self.buf[:self.words.storage_offset()], self.buf[self.words.storage_offset() + self.n:]
        assert lo.numel() >= PAD and hi.numel() >= PAD
        assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), f"{self.what}: a word outside the output was written"
        assert not bool((self.words == SENTINEL).any()), f"{self.what}: an output word was never written"
        return self.t


@pytest.mark.parametrize("K,J", [(72, 24), (512, 136)])
@pytest.mark.parametrize("N", [33, 130])
def test_kernels_write_their_outputs_and_nothing_else(ops, N, K, J):
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    lib, check, stream = _capi.lib, _capi.check, lipvq_vae_amd.ops._stream
    c = _case(N, K, J)
    xc, Wc, bc, gc = c["x"].cuda(), c["W"].cuda(), c["b"].cuda(), c["g"].cuda()
    y, pre = _Fenced("y", N, J, offset_words=1), _Fenced("pre", N, J, offset_words=3)      # outputs need no alignment
    gx, gW, gb = _Fenced("gx", N, K, offset_words=2), _Fenced("gW", J, K, offset_words=1), _Fenced("gb", J, offset_words=3)
    ws = torch.empty(lib.lipvq_wgrad_bf16_workspace_bytes(N, J, K), dtype=torch.uint8, device="cuda")
    check(lib.lipvq_linear_act_bf16(xc.data_ptr(), Wc.data_ptr(), bc.data_ptr(), y.ptr(), pre.ptr(), N, K, J, ops.ACT_GELU, stream()),
          "lipvq_linear_act_bf16")
    check(lib.lipvq_linear_nn_bf16(gc.data_ptr(), Wc.data_ptr(), gx.ptr(), N, J, K, stream()), "lipvq_linear_nn_bf16")
    check(lib.lipvq_wgrad_bf16(gc.data_ptr(), xc.data_ptr(), gW.ptr(), gb.ptr(), ws.data_ptr(), N, J, K, stream()), "lipvq_wgrad_bf16")
    torch.cuda.synchronize()
    want_pre = c["y"] + c["b"].double()
    assert _ratio(f"fenced pre N={N} K={K} J={J}", pre.check(), want_pre, c["Ry"], K) <= 2.0
    assert float((y.check().cpu().double() - F.gelu(pre.t.cpu().double())).abs().max()) <= 1e-5 * float(want_pre.abs().max())
    assert _ratio(f"fenced gx N={N} K={K} J={J}", gx.check(), c["gx"], c["Rgx"], J) <= 2.0
    assert _ratio(f"fenced gW N={N} K={K} J={J}", gW.check(), c["gW"], c["RgW"], N) <= 2.0
    assert bool(((gb.check().cpu().double() - c["gb"]).abs() <= N * EPS * c["Rgb"]).all())


@pytest.mark.parametrize("N,K,J", [(240, 512, 1536), (4100, 64, 64)])
def test_results_repeat_bit_for_bit(ops, N, K, J):
    """(4100, 64, 64): 65 row chunks in the weight gradient, the last one of 4 rows."""
    torch.manual_seed(N + K + J)
    x, W, b, g = (torch.randn(N, K).cuda(), (torch.randn(J, K) / K ** 0.5).cuda(), torch.randn(J).cuda(), torch.randn(N, J).cuda())
    first = (ops.linear_bf16(x, W, b), ops.linear_nn_bf16(g, W), *ops.wgrad_bf16(g, x))
    again = (ops.linear_bf16(x, W, b), ops.linear_nn_bf16(g, W), *ops.wgrad_bf16(g, x))
    for what, p, q in zip(("y", "gx", "gW", "gb"), first, again):
        assert torch.equal(p, q), what
    gW, gb = first[2].cpu().double(), first[3].cpu().double()                    # and the chunks add up to the right thing
    gr, xr = _rb(g.cpu()), _rb(x.cpu())
    assert bool(((gW - gr.t() @ xr).abs() <= 2 * (N + 1) * EPS * (gr.abs().t() @ xr.abs())).all())
    assert bool(((gb - g.cpu().double().sum(0)).abs() <= N * EPS * g.cpu().double().abs().sum(0)).all())


# ---------------------------------------------------------------------------------------------------
# LinearFn(..., "bf16"): the branches of tests/test_gpu_nnfn.py
# ---------------------------------------------------------------------------------------------------

@pytest.fixture
def calls(monkeypatch):
    """What LinearFn asked of the ops: calls per entry point, fp32 and bf16."""
    from lipvq_vae_amd import ops
    seen = {}
    for name in ("linear", "wgrad", "linear_bf16", "linear_nn_bf16", "wgrad_bf16", "act_bwd"):
        def counted(*a, _fn=getattr(ops, name), _name=name, **k):
            seen[_name] = seen.get(_name, 0) + 1
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    return seen


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


@pytest.mark.parametrize("shape,E,with_b,gelu,only_w", [((5, 16), 64, True, False, False), ((2, 3, 8), 24, False, False, False),
                                                        ((7, 64), 128, True, True, False), ((5, 16), 64, True, False, True)])
def test_linear_fn_bf16_against_float64_autograd_on_rounded_operands(calls, shape, E, with_b, gelu, only_w):
    """The float64 reference rounds the operands of all three products (gpt_bf16_ref._RoundedLinear); what is left is fp32
    accumulation over at most 128 terms and the fp32 GELU / GELU' (1e-5 / 1e-4 of the scale, as in test_gpu_nnfn.py)."""
    from lipvq_vae_amd.nnfn import LinearFn
    from lipvq_vae_amd.ops import ACT_GELU, ACT_NONE
    g = torch.Generator().manual_seed(sum(shape) + E)
    x, W = torch.randn(*shape, generator=g), torch.randn(E, shape[-1], generator=g) / shape[-1] ** 0.5
    b = torch.randn(E, generator=g) if with_b else None
    gy = torch.randn(*shape[:-1], E, generator=g)
    xd, Wd = x.double().requires_grad_(not only_w), W.double().requires_grad_(True)
    bd = b.double().requires_grad_(not only_w) if with_b else None
    ref = gpt_bf16_ref._RoundedLinear.apply(xd, Wd, bd)
    if gelu:
        ref = F.gelu(ref)
    (ref * gy.double()).sum().backward()

    xc, Wc = x.cuda().requires_grad_(not only_w), W.cuda().requires_grad_(True)
    bc = b.cuda().requires_grad_(not only_w) if with_b else None
    y = LinearFn.apply(xc, Wc, bc, ACT_GELU if gelu else ACT_NONE, "bf16")
    assert y.shape == ref.shape and _rel(y.detach().cpu(), ref.detach()) <= 1e-5
    exact = F.linear(x.double(), W.double(), None if b is None else b.double())
    assert _rel(y.detach().cpu(), F.gelu(exact) if gelu else exact) > 1e-4, "the operands were not rounded"
    y.backward(gy.cuda())
    assert _rel(Wc.grad.cpu(), Wd.grad) <= 1e-4
    assert "linear" not in calls and "wgrad" not in calls and calls["linear_bf16"] == 1 and calls["wgrad_bf16"] == 1
    assert calls.get("act_bwd", 0) == (1 if gelu else 0)
    if only_w:
        assert "linear_nn_bf16" not in calls                                     # gx is None: no second product was launched
    else:
        assert calls["linear_nn_bf16"] == 1 and xc.grad.shape == x.shape and _rel(xc.grad.cpu(), xd.grad) <= 1e-4
    if with_b:
        assert only_w or _rel(bc.grad.cpu(), bd.grad) <= 1e-4
    with pytest.raises(ValueError):
        LinearFn.apply(xc, Wc, bc, ACT_NONE, "fp16")


# ---------------------------------------------------------------------------------------------------
# the whole backbone on the gpt_small fixture
# ---------------------------------------------------------------------------------------------------

def _module(golden_dir, name="gpt_small"):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gpt import GPTBackbone
    g = np.load(golden_dir / f"{name}.npz", allow_pickle=False)
    cfg = {k: int(g[k]) for k in ("seed", "B", "L", "E", "H", "layers", "causal")}
    torch.manual_seed(cfg["seed"])
    net = GPTBackbone(embed_dim=cfg["E"], context_length=cfg["L"], causal=bool(cfg["causal"]), num_layers=cfg["layers"],
                      num_heads=cfg["H"], attn_dropout=0.0, block_output_dropout=0.0)
    assert gpt_ref.state_hash(net.state_dict()) == str(g["params_sha256"]), "seeded parameters differ from the fixture's"
    return net, g, cfg


def _rel_t(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def test_backbone_error_is_the_modes_own_rounding(golden_dir):
    """e0 = the distance of the float64 emulation of the mode (every Linear's operands rounded, exact accumulation) from the
    float64 fixture, computed here on the CPU.  The GPU's bf16 output must lie within [0.25 e0, 2 e0] of the fixture: no
    more than the mode's rounding (the kernels add nothing), no less (bf16 really ran); the input gradient likewise."""
    net, g, cfg = _module(golden_dir)
    out64, gx64 = torch.from_numpy(g["out64"]), torch.from_numpy(g["gx64"])
    sd64 = {k: v.double() for k, v in net.state_dict().items()}
    r = gpt_ref.objective_weights(cfg["seed"], out64.shape)
    x64 = torch.from_numpy(g["x"]).double().requires_grad_(True)
    emu = gpt_bf16_ref.gpt_forward_bf16(sd64, x64, cfg["layers"], cfg["H"])
    (emu * r.double()).sum().backward()
    e0_out, e0_gx = _rel_t(emu.detach(), out64), _rel_t(x64.grad, gx64)
    print(f"gpt_small: e0(out) = {e0_out:.3e}, e0(gx) = {e0_gx:.3e}; the fp32 reference's own {float(g['dev/out']):.3e}, {float(g['dev/gx']):.3e}")
    assert e0_out > 100 * float(g["dev/out"])                                 # the emulation itself rounds

    net = net.cuda()
    x = torch.from_numpy(g["x"]).cuda()
    net.eval()
    with torch.no_grad():
        before = net(x)
        assert net.set_matmul_precision("bf16") is net
        out_eval = net(x)
    net.train()                                                               # all dropout p = 0: the same function, with the autograd graph
    xg = x.clone().requires_grad_(True)
    out = net(xg)
    assert torch.equal(out.detach(), out_eval)
    (out * r.cuda()).sum().backward()
    e_out, e_gx = _rel_t(out_eval.cpu(), out64), _rel_t(xg.grad.cpu(), gx64)
    print(f"gpt_small bf16: out error {e_out:.3e} = {e_out / e0_out:.2f} e0, gx error {e_gx:.3e} = {e_gx / e0_gx:.2f} e0")
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters()), "a parameter got no gradient"
    net.eval()
    with torch.no_grad():
        assert torch.equal(net.set_matmul_precision("fp32")(x), before), "the bf16 mode left something behind"
    assert 0.25 * e0_out <= e_out <= 2 * e0_out, (e_out, e0_out)
    assert 0.25 * e0_gx <= e_gx <= 2 * e0_gx, (e_gx, e0_gx)


def test_graph_replay_equals_eager_in_bf16_mode(golden_dir):
    from lipvq_vae_amd.gpt import GraphedGPTBackbone
    net, g, cfg = _module(golden_dir)
    net = net.cuda().eval().set_matmul_precision("bf16")
    x = torch.from_numpy(g["x"]).cuda()
    graphed = GraphedGPTBackbone(net, torch.zeros_like(x))
    with torch.no_grad():
        for xin in (x, x.flip(0) * 0.5, x):
            assert torch.equal(graphed(xin), net(xin))
        fp32 = net.set_matmul_precision("fp32")(x)
        assert not torch.equal(fp32, graphed(x))                                # the graph keeps the mode it was captured in
