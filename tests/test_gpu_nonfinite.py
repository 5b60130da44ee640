"""GPU: NaN and +-inf traced through the kernels that feed the policy (cases, restatements and rule: tests/nonfinite_cases.py).

Every case is two calls through ``lipvq_vae_amd.ops`` (or a module) -- the clean input and the input with ONE element set to
NaN, +inf or -inf -- and ``judge``: inside the strict cone the result is non-finite wherever the float64 reference is (a swallowed
NaN fails) and finite and within the operation's tolerance elsewhere; outside the loose cone it equals the clean call bit for bit
(a neighbour's row read through tile padding, a clamped index, a reused LDS slot or a wrong shuffle partner and multiplied by 0
fails: 0 * NaN = NaN).  Cone sizes are printed before the assertion.

No address or loop bound of the kernels run here comes from a float value -- read in the sources before the first run:
  linear_kernel / linear_big_kernel (lipvq_embed.hip), mlp3_kernel / mlp3_wg_kernel / mlp3_lds_kernel (lipvq_mlp.hip),
  act_bwd_kernel (lipvq_bin.hip), the wgrad kernels (lipvq_bwd.hip): indices from N, the widths and the tile position alone; rows
      past N are clamped to N - 1 on loads and skipped on stores.
  gpt_layernorm(_bwd)_kernel, gpt_attention(_prefix / _bwd_q / _bwd_kv)_kernel (lipvq_gpt.hip), attention(_bwd_q / _bwd_kv)_kernel
      (lipvq_xf.hip): row, key and head indices from B, L, H, P and the tile position; keys past L are clamped to L - 1 and masked by
      a select; the keep mask is an integer input read at a shape-only index.
  embed_rows(_bwd) (lipvq_embed.hip): table rows are addressed by the INTEGER input idx (checked against the table size, no float).
  gmm_head_kernel (lipvq_gmm.hip): the sampler's `pick` is the one data-dependent index; it starts at M - 1 and is only ever
      assigned a loop counter m < M, so a NaN CDF (every comparison false) leaves M - 1.  gmm_head_bwd / gmm_params_bwd /
      action_head(_bwd) (lipvq_action_head.hip): shape-only.
  The fused VQ tokenize instance (lipvq_fused.hip) books codes from comparisons (k1 starts at 0 and takes loop indices < K); a NaN
      distance never wins, so the index stays in range (DESIGN 4.1 "Rows that are not finite").

What the tests found, and which test fails when a fix is reverted, is in LABNOTES.md ("Non-finite values in the policy stack").
"""
import numpy as np
import pytest
import torch

import nonfinite_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _dev(t):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in t.items()}


def _run_linear(ops, t, act):
    return {"y": ops.linear(t["x"], t["W"], t["b"], act)}


def _run_mlp3(ops, t, acts):
    pk = ops.mlp3_pack(*(t[k] for k in ("W0", "b0", "W1", "b1", "W2", "b2")))
    y, pre = ops.mlp3(t["x"], pk, acts, save_pre=True)
    return {"y": y, "pre0": pre[0], "pre1": pre[1], "pre2": pre[2]}


def _run_act_bwd(ops, t, act):
    return {"out": ops.act_bwd(t["g"], t["pre"], act)}


def _run_wgrad(ops, t, h_act):
    gW, gb = ops.wgrad(t["G"], t["H"], h_act)
    return {"gW": gW, "gb": gb}


def _run_layernorm(ops, t):
    s, y, xhat, rstd = ops.gpt_layernorm(t["a"], t["b"], t["w"], t["bias"], C.X.LN_EPS, save=True)
    gs, gw, gb = ops.gpt_layernorm_bwd(t["gy"], xhat, rstd, t["w"], t["gres"])
    return {"s": s, "y": y, "xhat": xhat, "rstd": rstd, "gs": gs, "gw": gw, "gb": gb}


def _run_gpt_attention(ops, t, H, causal, keep_prob):
    keep = t.get("keep")
    out, lse = ops.gpt_attention(t["qkv"], H, causal, keep, keep_prob)
    return {"out": out, "lse": lse, "gqkv": ops.gpt_attention_bwd(t["qkv"], out, t["gout"], lse, H, causal, keep, keep_prob)}


def _run_prefix(ops, t, H):
    return {"out": ops.gpt_attention_prefix(t["prefix"], t["qkv"], H)}


def _run_attention(ops, t, H):
    out, lse = ops.attention(t["qkv"], H)
    return {"out": out, "lse": lse, "gqkv": ops.attention_bwd(t["qkv"], out, t["gout"], lse, H)}


def _run_embed(ops, t, T):
    N, E = t["gout"].shape
    B = -(-N // T)
    out = torch.zeros(B * T, E, device="cuda")
    stats = ops.embed_rows(t["src"], t["idx"], t["pos"], t["w"], t["bias"], C.X.LN_EPS, out, N, T, T * E, E, 0, want_stats=True)
    gout = torch.zeros(B * T, E, device="cuda")
    gout[:N] = t["gout"]
    g = {"g_src": torch.zeros_like(t["src"]), "g_pos": torch.zeros_like(t["pos"]), "g_lnw": torch.zeros(E, device="cuda"),
         "g_lnb": torch.zeros(E, device="cuda")}
    ops.embed_rows_bwd(gout, t["src"], t["idx"], t["pos"], stats, t["w"], g["g_src"], g["g_pos"], g["g_lnw"], g["g_lnb"], N, T, T * E, E, 0)
    return {"y": out[:N], "rstd": stats[:, 1], **g}


def _run_gmm(ops, t, M, A, std):
    mode = {"softplus": ops.GMM_SOFTPLUS, "exp": ops.GMM_EXP}[std]
    params = tuple(t[k] for k in ("mean.weight", "mean.bias", "scale.weight", "scale.bias", "logits.weight", "logits.bias"))
    o = ops.gmm_head(t["feats"], params, M, A, actions=t["actions"], scale_mode=mode, min_std=C.GMM_MIN_STD, want_pre=True,
                     want_params=True, want_sum=True)
    o["gpre"] = ops.gmm_head_bwd(o["pre"], t["actions"], t["g"], t["gsum"], M, A, mode, C.GMM_MIN_STD)
    o["gpre_params"] = ops.gmm_params_bwd(o["pre"], t["gmean"], t["gscale"], t["glogits"], M, A, mode)
    o["sample"] = ops.gmm_sample(t["feats"], params, M, A, t["u"], t["eps"], mode, C.GMM_MIN_STD)
    return o


def _run_action_head(ops, t):
    o = ops.action_head(t["feats"], t["W"], t["b"], t["target"], C.ACTION_HEAD_WEIGHTS, want_actions=True, want_pre=True)
    o["gpre"] = ops.action_head_bwd(o["pre"], t["target"], t["g"], t["gy"], C.ACTION_HEAD_WEIGHTS)
    return o


_nets = {}


def _run_gpt_module(ops, t, sd):
    if "gpt" not in _nets:
        from lipvq_vae_amd.gpt import GPTBackbone
        m = C.GPT_MODULE
        net = GPTBackbone(embed_dim=m["E"], context_length=m["L"], causal=True, attn_dropout=0.0, block_output_dropout=0.0,
                          num_layers=m["num_layers"], num_heads=m["num_heads"])
        own = net.state_dict()
        assert {k for k, _ in net.named_parameters()} <= set(sd), "a parameter of the module has no seeded value"
        net.load_state_dict({k: (sd[k] if k in sd else v) for k, v in own.items()})
        _nets["gpt"] = net.cuda().eval()
    with torch.no_grad():
        return {"y": _nets["gpt"](t["x"])}


RUN = {"linear": _run_linear, "mlp3": _run_mlp3, "act_bwd": _run_act_bwd, "wgrad": _run_wgrad, "layernorm": _run_layernorm,
       "gpt_attention": _run_gpt_attention, "gpt_attention_prefix": _run_prefix, "attention": _run_attention, "embed_rows": _run_embed,
       "gmm": _run_gmm, "action_head": _run_action_head, "gpt_module": _run_gpt_module}


def _call(ops, group, inputs):
    out = RUN[group.op](ops, _dev(inputs), **group.params)
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}


def _trace(ops, group):
    """the clean call once, then every case of the group: sizes printed, every failing case collected, one assertion at the end"""
    clean = _call(ops, group, group.inputs)
    for k, v in clean.items():
        assert bool(v.isfinite().all()), f"{group.name}: the clean call's {k} is not finite"
    failures = []
    for case in group.cases():
        got = _call(ops, group, case.planted())
        sizes = case.cone_sizes()
        print(f"{case.name}: " + ", ".join(f"{k} {s}/{l}/{n}" for k, (s, l, n) in sizes.items()) + "  (strict / loose / all)")
        try:
            C.judge(got, clean, case)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, f"{len(failures)} of {len(group.cases())} cases:\n" + "\n".join(failures)
    return clean


def _param(op):
    gs = C.groups(op)
    return pytest.mark.parametrize("group", gs, ids=[g.name for g in gs])


@_param("linear")
def test_linear(ops, group):
    _trace(ops, group)


@_param("mlp3")
def test_mlp3(ops, group):
    _trace(ops, group)


@_param("act_bwd")
def test_act_bwd(ops, group):
    _trace(ops, group)


@_param("wgrad")
def test_wgrad(ops, group):
    _trace(ops, group)


@_param("layernorm")
def test_layernorm(ops, group):
    _trace(ops, group)


@_param("gpt_attention")
def test_gpt_attention(ops, group):
    _trace(ops, group)


@_param("gpt_attention_prefix")
def test_gpt_attention_prefix(ops, group):
    _trace(ops, group)


@_param("attention")
def test_attention_unbatched(ops, group):
    _trace(ops, group)


@_param("embed_rows")
def test_embed_rows(ops, group):
    _trace(ops, group)


@_param("gmm")
def test_gmm_head(ops, group):
    _trace(ops, group)


@_param("action_head")
def test_action_head(ops, group):
    _trace(ops, group)


@_param("gpt_module")
def test_gpt_backbone_eval(ops, group):
    """x[1, 7, 3] planted: sequences 0 and 2 equal the clean run bit for bit (and judge's rule for sequence 1)."""
    clean = _trace(ops, group)
    for case in group.cases():
        got = _call(ops, group, case.planted())
        for b in (0, 2):
            assert torch.equal(got["y"][b].view(torch.int32), clean["y"][b].view(torch.int32)), (case.name, b)
        assert not bool(got["y"][1, 7:].isfinite().all()), case.name


def test_vqvae_nan_weight_reaches_the_loss_and_its_gradient():
    """encoder.0.weight[3, 2] = NaN in the plain VQVAE: the loss and that weight's gradient are NaN, as in the torch restatement
    (before the ReLU fix the unit went silently dead: a finite loss).  The clean module's loss is finite."""
    from lipvq_vae_amd.tokenizer import VQVAE
    m = C.VQ_MODULE
    p, planted, x = C.vq_module_case()
    ref_loss, ref_grads = C.vq_module_ref(planted, x)
    assert bool(ref_loss.isnan()) and bool(ref_grads["encoder.0.weight"][3, 2].isnan())
    xt = torch.from_numpy(x).cuda()
    results = {}
    for name, params in (("clean", p), ("planted", planted)):
        model = VQVAE(m["A"], m["D"], num_embeddings=m["K"]).cuda()
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
        _, loss = model(xt)
        loss.backward()
        torch.cuda.synchronize()
        results[name] = (loss.detach().cpu(), {k: v.grad.detach().cpu() for k, v in model.named_parameters() if v.grad is not None})
        print(f"{name}: loss {float(loss.detach()):.6g}, non-finite gradient elements "
              + ", ".join(f"{k} {int((~g.isfinite()).sum())}/{g.numel()}" for k, g in results[name][1].items()))
    loss, grads = results["clean"]
    assert bool(loss.isfinite()) and all(bool(g.isfinite().all()) for g in grads.values())
    loss, grads = results["planted"]
    assert bool(loss.isnan()), loss
    assert bool(grads["encoder.0.weight"][3, 2].isnan())
    # every gradient the restatement shows as non-finite is non-finite here
    for k, g in grads.items():
        want = ~ref_grads[k].isfinite()
        assert bool((~g.isfinite())[want].all()), (k, int(want.sum()), int(((~g.isfinite()) & want).sum()))
