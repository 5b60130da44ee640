"""GPU: the layer between the kernels and ``loss.backward()`` -- the twelve ``torch.autograd.Function`` classes of the library -- under
what training code does besides "every leaf trains, one backward, every output used, a dense upstream gradient": frozen subsets
of the leaves, unused outputs (a ``None`` upstream gradient), scaled / expanded / non-contiguous upstream gradients, a retained
graph differentiated twice, micro-batches accumulated into ``.grad``, two forwards before one backward, and a second
differentiation, which is refused.

The cases, their float64 references and the yardstick are tests/autograd_cases.py's (a gradient's bound is
``X.bound(BWD_TOL, dev)``, an output's ``X.bound(FWD_TOL, dev)``, dev = the fp32 restatement against the float64 one);
tests/test_autograd_cases_host.py shows that each bug this file guards against leaves that bound at these shapes.  Every
figure is printed before it is asserted.  A bit-equality claim about gradients is made only after two identical all-trainable
runs of the same case gave equal bits in the same test; the kinds whose backward adds with float atomics (the embedding's
row sums, the tokenizers' and the binning module's scatter at these row counts) are held to the bound alone.
"""
import warnings

import pytest
import torch

import autograd_cases as C
import xf_edge_inputs as X

pytestmark = pytest.mark.gpu

FUSED_NAMES = C.register_fused()
ATOMIC_KINDS = ("embed", "tokenizer", "bin")          # unordered float sums in the backward: no bit-equality between two runs


def _cuda_leaf(t):
    return t.detach().clone().cuda().requires_grad_(True)


# ---------------------------------------------------------------------------------------------------
# one builder per kind: ({leaf name: CUDA leaf tensor}, forward() -> {output name: tensor})
# ---------------------------------------------------------------------------------------------------

def _build_addln(case, precision):
    from lipvq_vae_amd.nnfn import AddLayerNormFn
    lv = {k: _cuda_leaf(v) for k, v in case.leaves.items()}

    def fwd():
        s, y = AddLayerNormFn.apply(lv["in.a"], lv.get("in.b"), lv["w"], lv["bias"], case.info["eps"], True)
        return {"s": s, "y": y}
    return lv, fwd


def _gpt_module(precision):
    from lipvq_vae_amd.gpt import GPTBackbone
    g = C.GPT
    m = GPTBackbone(g["embed_dim"], g["context_length"], attn_dropout=0.0, block_output_dropout=0.0, num_layers=g["num_layers"],
                    num_heads=g["num_heads"]).cuda().train()
    m.load_state_dict(C.gpt_state(), strict=True)
    return m.set_matmul_precision(precision or "fp32")


def _build_gpt(case, precision):
    m = _gpt_module(precision)
    lv = dict(m.named_parameters())
    lv["in.x"] = _cuda_leaf(case.leaves["in.x"])
    return lv, lambda: {"out": m(lv["in.x"])}


def _build_gpt_dropout(case, precision):
    """GPTBackbone.forward's one block, with the three keep masks GIVEN: the Functions directly (the module draws its own)."""
    from lipvq_vae_amd.gpt import _AttentionFn
    from lipvq_vae_amd.nnfn import AddLayerNormFn, LinearFn
    from lipvq_vae_amd.ops import ACT_GELU, ACT_NONE
    lv = {k: _cuda_leaf(v) for k, v in case.leaves.items()}
    ka, ko, km = (k.cuda() for k in case.info["keeps"])
    kp, H, prec = case.info["keep_prob"], C.GPT["num_heads"], precision or "fp32"

    def fwd():
        x = lv["in.x"]
        y = AddLayerNormFn.apply(x, None, lv["ln1.weight"], lv["ln1.bias"], X.LN_EPS, False)[1]
        qkv = LinearFn.apply(y, lv["attention.nets.qkv.weight"], None, ACT_NONE, prec)
        o = _AttentionFn.apply(qkv, H, True, ka, kp)
        o = LinearFn.apply(o, lv["attention.nets.output.weight"], lv["attention.nets.output.bias"], ACT_NONE, prec)
        o = o * ko.float() / kp
        s, y = AddLayerNormFn.apply(x, o, lv["ln2.weight"], lv["ln2.bias"], X.LN_EPS, True)
        f = LinearFn.apply(y, lv["mlp.0.weight"], lv["mlp.0.bias"], ACT_GELU, prec)
        f = LinearFn.apply(f, lv["mlp.2.weight"], lv["mlp.2.bias"], ACT_NONE, prec)
        return {"out": s + f * km.float() / kp}
    return lv, fwd


def _feats(case, lv):
    return lv["in.feats"] if case.info["layout"] == "dense" else lv["in.base"][:, -C.HEAD["T"]:]


def _build_gmm(case, precision):
    from lipvq_vae_amd.gmm import GMMActionHead, _ParamsFn
    h = C.HEAD
    head = GMMActionHead(h["E"], h["A"], num_modes=h["M"], min_std=case.info["min_std"], std_activation=case.info["act"]).cuda().train()
    head.load_state_dict({k: v for k, v in case.leaves.items() if not k.startswith("in.")}, strict=True)
    lv = dict(head.named_parameters())
    lv.update({k: _cuda_leaf(case.leaves[k]) for k in case.inputs})
    actions = case.info["actions"].cuda()

    def fwd():
        feats = _feats(case, lv)
        assert case.info["layout"] == "dense" or not feats.is_contiguous()
        lp, total = head._log_prob(feats, actions, False, True)
        mean, scale, logits = _ParamsFn.apply(feats, *head._params(), h["M"], h["A"], head._mode(None), float(head.min_std))
        return {"log_prob": lp, "sum": total, "mean": mean, "scale": scale, "logits": logits}
    return lv, fwd


def _build_head(case, precision):
    from lipvq_vae_amd.action_head import ActionHead
    h = C.HEAD
    head = ActionHead(h["E"], h["A"]).cuda().train()
    head.load_state_dict({k: v for k, v in case.leaves.items() if not k.startswith("in.")}, strict=True)
    lv = dict(head.named_parameters())
    lv.update({k: _cuda_leaf(case.leaves[k]) for k in case.inputs})
    target = case.info["target"].cuda()

    def fwd():
        feats = _feats(case, lv)
        return dict({"actions": head(feats)}, **head.losses(feats, target, *case.info["weights"]))
    return lv, fwd


def _embed_key(k):
    return ("params." if k == "embed_timestep" else "nets.") + k


def _build_embed(case, precision):
    from lipvq_vae_amd.embedding import ICLInputEmbedding
    e, mode = C.EMBED, case.info["mode"]
    m = ICLInputEmbedding(e["Din"], e["E"], e["T"], emb_dropout=0.0, sinusoidal_embedding=mode == "sinusoidal",
                          nn_parameter_for_timesteps=mode == "parameter").cuda().train()
    m.load_state_dict({_embed_key(k): v for k, v in case.leaves.items() if not k.startswith("in.")}, strict=True)
    named = dict(m.named_parameters())
    lv = {k: named[_embed_key(k)] for k in case.params}
    lv.update({k: _cuda_leaf(case.leaves[k]) for k in case.inputs})
    idx, cb = case.info["idx"].cuda(), case.info["codebook"].cuda()

    def fwd():
        if case.info["route"] == "dense":
            return {"out": m(lv["in.obs"], lv["in.context_obs"], lv["in.context_actions"])}
        return {"out": m(lv["in.obs"], lv["in.context_obs"], action_indices=idx, codebook=cb)}
    fwd.module, fwd.codebook = m, cb
    return lv, fwd


def _build_bin(case, precision):
    from lipvq_vae_amd.binning import AdaptiveBinActionEmbedding
    i = case.info
    m = AdaptiveBinActionEmbedding(i["A"], i["D"], num_bins=i["nb"]).cuda().train()
    sd = dict(case.leaves)
    sd["running_min"], sd["running_max"] = m.running_min.cpu(), m.running_max.cpu()
    m.load_state_dict(sd, strict=True)
    actions = i["actions"].cuda()
    return dict(m.named_parameters()), lambda: {"out": m(actions)}


def _default_module(case):
    from lipvq_vae_amd.default_branch import DefaultActionNetwork
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = DefaultActionNetwork(C.DEFAULT["A"], C.DEFAULT["D"], num_layers=case.info["num_layers"])
    m.load_state_dict(case.info["state"], strict=True)
    m = m.cuda().train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    return m


def _build_default(case, precision):
    m = _default_module(case)                           # (a fresh module per run: a training forward moves weight_u / weight_v)
    lv = dict(m.named_parameters())
    lv["in.x"] = _cuda_leaf(case.leaves["in.x"])

    def fwd():
        outs = [m(lv["in.x"]) for _ in range(case.info["calls"])]
        return {"out": outs[0]}
    return lv, fwd


def _tokenizer_module(case):
    from lipvq_vae_amd.tokenizer import LLFQVAE_V4, VQVAE
    t = C.TOK
    m = (LLFQVAE_V4(t["A"], t["D"], num_codes=t["K"]) if case.info["variant"] == "llfq" else VQVAE(t["A"], t["D"], num_embeddings=t["K"])).cuda()
    m.load_state_dict(case.leaves, strict=True)
    return m.train()


def _build_tokenizer(case, precision):
    m = _tokenizer_module(case)
    x = case.info["x"].cuda()
    fwd = lambda: {"loss": m(x)[1]}                     # noqa: E731
    fwd.module, fwd.x = m, x
    return dict(m.named_parameters()), fwd


_BUILD = {"addln": _build_addln, "gpt": _build_gpt, "gpt_dropout": _build_gpt_dropout, "gmm": _build_gmm, "head": _build_head,
          "embed": _build_embed, "bin": _build_bin, "default": _build_default, "tokenizer": _build_tokenizer}


def build(case, precision=None):
    import lipvq_vae_amd  # noqa: F401
    lv, fwd = _BUILD[case.kind](case, precision)
    assert set(lv) == set(case.leaves), (case.name, set(lv) ^ set(case.leaves))
    return lv, fwd


def objective(case, outs, coeff=None):
    coeff = {k: 1.0 for k in case.outputs} if coeff is None else coeff
    return sum(c * (outs[k] * case.R[k].cuda()).sum() for k, c in coeff.items())


def run(case, trainable=None, coeff=None, precision=None):
    """One fresh module, one forward, one backward of the case's objective: (outputs, {leaf: .grad or None})."""
    lv, fwd = build(case, precision)
    for k, t in lv.items():
        t.requires_grad_(trainable is None or k in trainable)
    outs = fwd()
    objective(case, outs, coeff).backward()
    return {k: v.detach() for k, v in outs.items()}, {k: t.grad for k, t in lv.items()}


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and torch.equal(a[k], b[k])) for k in a)


def against_reference(case, outs, grads, trainable=None, coeff=None, tag=""):
    """Every output and every gradient against the float64 reference of the same trainable set and coefficients; frozen leaves None."""
    ref_o, ref_g = C.evaluate(case, torch.float64, trainable, coeff)
    dev_o, dev_g = C.dev(case, trainable, coeff)
    bad = []
    for k, v in (outs or {}).items():
        bad.append(C.check(f"{case.name}{tag} {k}", v.cpu(), ref_o[k], dev_o[k], X.FWD_TOL))
    for k, g in grads.items():
        if ref_g[k] is None:                            # frozen, or reached by no used output: None, or (a trainable leaf whose columns
            if g is not None and (trainable is not None and k not in trainable or bool(g.count_nonzero())):     # saw a zero gradient) zeros
                bad.append((f"{case.name}{tag} {k}", "has a gradient, the reference has none"))
            continue
        if g is None:
            bad.append((f"{case.name}{tag} {k}", "no gradient"))
            continue
        bad.append(C.check(f"{case.name}{tag} grad {k}", g.cpu(), ref_g[k], dev_g[k], X.BWD_TOL))
    bad = [b for b in bad if b]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------
# frozen subsets
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.FREEZE_NAMES + FUSED_NAMES)
def test_frozen_subsets(name):
    """All-trainable against float64; then every freeze pattern: kept leaves meet the bound and -- where two all-trainable runs
    agree in bits -- carry the all-trainable run's bits, frozen leaves end with .grad None."""
    case = C.get(name)
    outs, full = run(case)
    _, again = run(case)
    repeatable = same_bits(full, again)
    print(f"{name}: two all-trainable runs agree in bits: {repeatable}")
    assert repeatable or case.kind in ATOMIC_KINDS, f"{name}: no float atomics in this backward, yet two runs differ"
    against_reference(case, outs, full)
    for label, trainable in case.patterns():
        outs_p, part = run(case, trainable=trainable)
        assert all(torch.equal(outs_p[k], outs[k]) for k in outs), (name, label, "freezing a leaf changed the forward")
        against_reference(case, None, part, trainable=trainable, tag=f" [{label}]")
        if repeatable and case.kind not in ATOMIC_KINDS:
            for k in trainable:
                assert torch.equal(part[k], full[k]), (name, label, k, "kept leaf differs in bits from the all-trainable run")


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_frozen_subsets_on_the_bf16_pipes(precision):
    """LinearFn takes other ops in the two bf16 modes (linear_nn_*, wgrad_*): every freeze pattern of the backbone once in each.
    The numbers of these modes are held by the bf16 tests; here a kept leaf must carry the all-trainable run's bits (checked to
    repeat first) and a frozen one none.  bf16x3, whose products are within 2^-16, meets the float64 bound as well."""
    case = C.get("gpt")
    outs, full = run(case, precision=precision)
    _, again = run(case, precision=precision)
    assert same_bits(full, again), "no atomics in the backbone's backward, yet two runs differ"
    if precision == "bf16x3":
        against_reference(case, outs, full, tag=" bf16x3")
    for label, trainable in case.patterns():
        outs_p, part = run(case, trainable=trainable, precision=precision)
        assert torch.equal(outs_p["out"], outs["out"])
        for k in case.leaves:
            if k in trainable:
                assert part[k] is not None and torch.equal(part[k], full[k]), (precision, label, k)
            else:
                assert part[k] is None, (precision, label, k)


@pytest.fixture
def calls(monkeypatch):
    """What the Functions asked of ops: launches of the gx Linears and of the wgrad family, and the keep flags of the forwards."""
    from lipvq_vae_amd import ops
    seen = {"linear": 0, "linear_nn": 0, "wgrad": 0, "save_pre": 0, "want_pre": 0, "want_stats": 0, "ln_save": 0, "head_grads": []}

    def count(name, key, flag=None):
        fn = getattr(ops, name)

        def wrapped(*a, **k):
            if flag is None:
                seen[key] += 1
            elif k.get(flag):
                seen[key] += 1
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)

    for n in ("linear", "linear_bf16", "linear_bf16x3"):
        count(n, "save_pre", "save_pre")
    for n in ("linear", "linear_bf16", "linear_bf16x3"):
        count(n, "linear")
    for n in ("linear_nn_bf16", "linear_nn_bf16x3"):
        count(n, "linear_nn")
    for n in ("wgrad", "wgrad_bf16", "wgrad_bf16x3"):
        count(n, "wgrad")
    count("bin_hidden", "save_pre", "save_pre")
    count("gmm_head", "want_pre", "want_pre")
    count("action_head", "want_pre", "want_pre")
    count("embed_rows", "want_stats", "want_stats")
    count("gpt_layernorm", "ln_save", "save")
    grads = ops.head_linear_grads

    def head_grads(need_x, need_params, *a, **k):
        seen["head_grads"].append((bool(need_x), bool(need_params)))
        return grads(need_x, need_params, *a, **k)
    monkeypatch.setattr(ops, "head_linear_grads", head_grads)
    return seen


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("act", ["none", "gelu"])
def test_linear_fn_launches_only_what_is_needed(calls, precision, act):
    from lipvq_vae_amd.nnfn import LinearFn
    from lipvq_vae_amd.ops import ACT_GELU, ACT_NONE
    a = ACT_GELU if act == "gelu" else ACT_NONE
    x0, W0, b0 = (C._randn(("linear_fn", k), *s) for k, s in (("x", (5, 16)), ("W", (24, 16)), ("b", (24,))))
    gy = C._randn(("linear_fn", "gy"), 5, 24).cuda()
    want = {}
    for need_x, need_w, need_b in ((True, True, True), (True, True, True), (False, True, True), (True, False, False), (False, False, True), (True, True, False)):
        x, W, b = (t.cuda().requires_grad_(n) for t, n in ((x0, need_x), (W0, need_w), (b0, need_b)))
        before = dict(calls)
        y = LinearFn.apply(x, W, b, a, precision)
        y.backward(gy)
        gx_launches = (calls["linear"] - before["linear"] - 1) + (calls["linear_nn"] - before["linear_nn"])
        assert gx_launches == int(need_x), (need_x, need_w, need_b, gx_launches)
        assert calls["wgrad"] - before["wgrad"] == int(need_w or need_b)
        for t, n, k in ((x, need_x, "x"), (W, need_w, "W"), (b, need_b, "b")):
            assert (t.grad is not None) == n, k
            if n:
                # (the first two rounds are two identical all-trainable runs: they must agree before any pattern is compared)
                assert torch.equal(t.grad, want.setdefault(k, t.grad)), (k, "differs in bits from the all-trainable run")
    before = dict(calls)
    with torch.no_grad():
        y_ng = LinearFn.apply(x0.cuda().requires_grad_(True), W0.cuda(), b0.cuda(), a, precision)
    y_frozen = LinearFn.apply(x0.cuda(), W0.cuda(), b0.cuda(), a, precision)
    assert calls["save_pre"] == before["save_pre"], "a forward that keeps nothing for a backward asked for the pre-activation"
    assert torch.equal(y_ng, y.detach()) and torch.equal(y_frozen, y.detach()) and not y_frozen.requires_grad


def test_frozen_module_launches_no_wgrad_and_no_gx(calls):
    """input_only: no wgrad-family launch in the backbone, the heads' head_linear_grads asked for gx alone; parameters only: the
    heads ask for no gx Linear."""
    case = C.get("gpt")
    before = calls["wgrad"]
    run(case, trainable=case.inputs)
    assert calls["wgrad"] == before
    for name in ("gmm_softplus_view", "head_view"):
        case = C.get(name)
        calls["head_grads"].clear()
        before = dict(calls)
        _, g = run(case, trainable=case.inputs)
        assert calls["head_grads"] and all(h == (True, False) for h in calls["head_grads"]), calls["head_grads"]
        assert calls["wgrad"] == before["wgrad"] and g[case.inputs[0]] is not None
        calls["head_grads"].clear()
        before = dict(calls)
        run(case, trainable=case.params)
        assert calls["head_grads"] and all(h == (False, True) for h in calls["head_grads"]), calls["head_grads"]
        assert calls["linear"] == before["linear"]                          # (the heads' forward is its own kernel: no Linear at all)


@pytest.mark.parametrize("name", ["gpt", "gmm_softplus_dense", "head_dense", "embed_parameter_dense", "embed_parameter_index", "bin_a7",
                                  "default_L1"])
def test_a_forward_that_needs_no_backward_keeps_nothing(calls, name):
    """Under torch.no_grad(), and in grad mode with nothing requiring a gradient, no forward asks for pre / stats / save -- and
    both return the bits of the training forward."""
    case = C.get(name)
    lv, fwd = build(case)
    ref = {k: v.detach() for k, v in fwd().items()}
    again = build(case)[1]()
    assert all(torch.equal(again[k], ref[k]) for k in ref), "two identical training forwards differ: no bit claim can be made"
    asked = ("save_pre", "want_pre", "want_stats", "ln_save")
    assert sum(calls[k] for k in asked) > 0, "the training forward keeps something: the counters see it"
    for mode in ("no_grad", "frozen"):
        lv, fwd = build(case)
        before = {k: calls[k] for k in asked}
        if mode == "no_grad":
            with torch.no_grad():
                outs = fwd()
        else:
            for t in lv.values():
                t.requires_grad_(False)
            outs = fwd()
        assert {k: calls[k] for k in asked} == before, (name, mode, before, {k: calls[k] for k in asked})
        for k, v in outs.items():
            assert not v.requires_grad and torch.equal(v, ref[k]), (name, mode, k)


@pytest.mark.parametrize("mode", C.O.EMBED_MODES)
def test_code_table_follows_the_encoders_requires_grad(mode):
    """ICLInputEmbedding.code_table: LinearFn while the embed_encoder trains, the cached detached table once both its tensors
    are frozen -- the same bits, gradients for what still trains, and the cache sees a later un-freezing."""
    case = C.get(f"embed_{mode}_index")
    lv, fwd = build(case)
    m = fwd.module
    out_train = fwd()["out"]
    assert torch.equal(fwd()["out"], out_train), "two identical forwards differ: no bit claim can be made"
    for k in case.groups["encoder"]:
        lv[k].requires_grad_(False)
    table = m.code_table(fwd.codebook)
    assert not table.requires_grad and table is m.code_table(fwd.codebook)                          # the cached tensor
    outs = fwd()
    assert torch.equal(outs["out"], out_train.detach())
    objective(case, outs).backward()
    trainable = set(case.leaves) - set(case.groups["encoder"])
    against_reference(case, None, {k: t.grad for k, t in lv.items()}, trainable=trainable, tag=" [encoder frozen]")
    lv["embed_encoder.bias"].requires_grad_(True)                           # bias-only tuning: back on LinearFn
    assert m.code_table(fwd.codebook).requires_grad


# ---------------------------------------------------------------------------------------------------
# unused outputs
# ---------------------------------------------------------------------------------------------------

def _uses():
    out = [("addln_ab", "y", {"y": 1.0}), ("addln_ab", "s", {"s": 1.0}), ("addln_ab", "both", {"s": 0.8, "y": 1.0}),
           ("addln_a", "y", {"y": 1.0}), ("addln_a", "s", {"s": 1.0}), ("addln_a", "both", {"s": 0.8, "y": 1.0})]
    for act, lay in (("softplus", "dense"), ("exp", "view")):
        out += [(f"gmm_{act}_{lay}", k, u) for k, u in list(C.GMM_LOGPROB_USES.items()) + list(C.GMM_PARAM_USES.items())]
    out += [(f"head_{lay}", k, u) for lay in ("dense", "view") for k, u in C.HEAD_USES.items()]
    return out


@pytest.mark.parametrize("name,label,use", _uses(), ids=[f"{n}-{k}" for n, k, _ in _uses()])
def test_unused_outputs(name, label, use):
    """Only some outputs take part in the loss: the others' upstream gradient is None (AddLayerNormFn, _LogProbFn, _ParamsFn:
    set_materialize_grads(False)) or zeros (the losses vector).  The gradients are the reference's for the outputs that remain."""
    case = C.get(name)
    outs, grads = run(case, coeff=use)
    against_reference(case, outs, grads, coeff=use, tag=f" [{label}]")


@pytest.mark.parametrize("name", ["llfq_n64", "vq_n64"])
def test_tokenizer_loss_unused(name):
    """z_latent alone feeds what follows (it is non-differentiable) and the loss is dropped: nothing to differentiate, every .grad
    stays None and no error; with the loss in a sum whose other term is differentiated alone, g_loss is None in backward."""
    case = C.get(name)
    lv, fwd = build(case)
    z, loss = fwd.module(fwd.x)
    assert not z.requires_grad and loss.requires_grad
    w = torch.ones((), device="cuda", requires_grad=True)
    (z.sum() * w).backward()
    assert all(t.grad is None for t in lv.values()) and w.grad is not None
    other = (z.sum() * w)
    grads = torch.autograd.grad(other, [w] + list(lv.values()), allow_unused=True)
    assert grads[0] is not None and all(g is None for g in grads[1:])


# ---------------------------------------------------------------------------------------------------
# upstream forms
# ---------------------------------------------------------------------------------------------------

UPSTREAM = {"addln_ab": "y", "gpt": "out", "gmm_softplus_view": "log_prob", "gmm_exp_dense": "scale", "head_view": "actions",
            "embed_parameter_dense": "out", "bin_a7": "out", "default_L1": "out"}          # case: the output the gradient arrives at


@pytest.mark.parametrize("name", list(UPSTREAM))
def test_upstream_gradient_forms(name):
    """out.backward(g) with g contiguous is the yardstick (held to float64 elsewhere); the same values as 3.5 x a scalar loss, as
    the expanded zero-stride tensor that .sum() hands down, as a transposed-back and as a sliced non-contiguous tensor must give
    its bits (bound only where the backward adds with atomics)."""
    case = C.get(name)
    key = UPSTREAM[name]
    exact = case.kind not in ATOMIC_KINDS

    def grads_of(make_loss=None, upstream=None):
        lv, fwd = build(case)
        out = fwd()[key]
        if make_loss is not None:
            make_loss(out).backward()
        else:
            g = upstream(out)
            assert g.shape == out.shape
            out.backward(g)
        return out.detach(), {k: t.grad for k, t in lv.items()}

    def same(got, want, what):
        for k in want:
            if want[k] is None or got[k] is None:       # (a leaf this output does not depend on)
                assert want[k] is None and got[k] is None, (name, what, k)
            elif exact:
                assert torch.equal(got[k], want[k]), (name, what, k)
            else:
                b = X.bound(X.BWD_TOL, C.dev(case)[1][k])
                err = X.rel(got[k].cpu(), want[k].cpu())
                print(f"{name} {what} {k}: {err:.3e} from the contiguous run, bound {b:.3e}")
                assert err <= b, (name, what, k, err)

    R = case.R[key].cuda()
    out, base = grads_of(upstream=lambda o: R.clone())
    if exact:
        _, again = grads_of(upstream=lambda o: R.clone())
        assert same_bits(base, again), "two identical runs differ: no bit claim can be made"
    # a scalar loss times 3.5: the gradient 3.5 R arrives through autograd's own mul / sum nodes
    _, scaled = grads_of(make_loss=lambda o: 3.5 * (o * R).sum())
    _, scaled_dense = grads_of(upstream=lambda o: (3.5 * R).contiguous())
    same(scaled, scaled_dense, "3.5 x scalar loss")
    # .sum(): an expanded zero-stride gradient
    _, expanded = grads_of(make_loss=lambda o: o.sum())
    _, ones = grads_of(upstream=lambda o: torch.ones_like(o))
    probe = torch.ones((), device="cuda").expand(out.shape)
    assert all(s == 0 for s in probe.stride())
    _, expanded2 = grads_of(upstream=lambda o: probe)
    same(expanded, ones, "expanded (.sum())")
    same(expanded2, ones, "expanded (zero strides)")
    # transposed-back and sliced: the values of R, other strides
    t_back = R.transpose(-1, -2).contiguous().transpose(-1, -2)
    wide = torch.zeros(R.shape[:-1] + (2 * R.shape[-1],), device="cuda")
    wide[..., ::2] = R
    sliced = wide[..., ::2]
    assert not t_back.is_contiguous() and not sliced.is_contiguous() and torch.equal(t_back, R) and torch.equal(sliced, R)
    same(grads_of(upstream=lambda o: t_back)[1], base, "transposed-back")
    same(grads_of(upstream=lambda o: sliced)[1], base, "sliced")


@pytest.mark.parametrize("name", ["llfq_n64", "vq_n64"])
def test_tokenizer_scaled_loss(name):
    case = C.get(name)
    _, grads = run(case, coeff={"loss": 3.5 / float(case.R["loss"])})
    ref = C.evaluate(case)[1]
    dev_g = C.dev(case)[1]
    bad = [C.check(f"{name} 3.5 x loss {k}", g.cpu() / 3.5 * float(case.R["loss"]), ref[k], dev_g[k], X.BWD_TOL) for k, g in grads.items()]
    assert not [b for b in bad if b], bad


# ---------------------------------------------------------------------------------------------------
# repeats
# ---------------------------------------------------------------------------------------------------

REPEAT_NAMES = ("addln_ab", "gpt", "gpt_dropout", "gmm_softplus_view", "gmm_exp_dense", "head_view", "embed_parameter_dense",
                "embed_embedding_index", "bin_a7", "default_L1", "llfq_n64", "vq_n64") + FUSED_NAMES


@pytest.mark.parametrize("name", REPEAT_NAMES)
def test_retained_graph_backward_twice_doubles_the_gradient(name):
    """backward(retain_graph=True) twice: .grad = g + g, exactly 2 g where a run repeats in bits (checked first); the saved
    tensors survive the first backward unchanged either way (the bound, for the atomic kinds)."""
    case = C.get(name)
    _, single = run(case)
    _, again = run(case)
    repeatable = same_bits(single, again) and case.kind not in ATOMIC_KINDS
    print(f"{name}: two runs agree in bits: {same_bits(single, again)}")
    lv, fwd = build(case)
    obj = objective(case, fwd())
    obj.backward(retain_graph=True)
    obj.backward()
    ref, dev_g = C.evaluate(case)[1], C.dev(case)[1]
    bad = []
    for k, t in lv.items():
        if repeatable:
            assert torch.equal(t.grad, 2.0 * single[k]), (name, k, "twice the backward is not twice the gradient")
        bad.append(C.check(f"{name} retained, twice: grad {k} / 2", t.grad.cpu() / 2.0, ref[k], dev_g[k], X.BWD_TOL))
    assert not [b for b in bad if b], bad
    with pytest.raises(RuntimeError):                   # and without retain_graph the second backward is torch's usual error
        lv, fwd = build(case)
        obj = objective(case, fwd())
        obj.backward()
        obj.backward()


@pytest.mark.parametrize("name", ["gpt", "gmm_softplus_view", "head_dense", "embed_parameter_index", "default_L1", "llfq_n64"])
def test_two_micro_batches_accumulate(name):
    """Two forward / backward passes into the same .grad (the second with another upstream weighting, standing for another
    micro-batch) equal g1 + g2 formed from two separate runs: in bits where a run repeats in bits; where the backward adds with
    atomics, against the float64 gradient of the summed objective (1 + 0.5 times the case's: both passes err in the same
    direction of scale, so the usual bound holds for the sum)."""
    case = C.get(name)
    second = {k: 0.5 for k in case.outputs}
    _, g1 = run(case)
    _, g2 = run(case, coeff=second)
    _, g1_again = run(case)
    exact = same_bits(g1, g1_again) and case.kind not in ATOMIC_KINDS
    lv, fwd = build(case)
    objective(case, fwd()).backward()
    if case.kind == "default":                          # (a fresh module's first forward, with the accumulated .grad carried over)
        lv2, fwd2 = build(case)
        for k in lv:
            lv2[k].grad = lv[k].grad
        lv, fwd = lv2, fwd2
    objective(case, fwd(), second).backward()
    ref, dev_g = C.evaluate(case)[1], C.dev(case)[1]
    bad = []
    for k, t in lv.items():
        if exact:
            assert torch.equal(t.grad, g1[k] + g2[k]), (name, k)
        bad.append(C.check(f"{name} accumulated grad {k}", t.grad.cpu(), 1.5 * ref[k], dev_g[k], X.BWD_TOL))
    assert not [b for b in bad if b], bad


def test_backprop_for_loss_with_a_retained_graph():
    """optim.backprop_for_loss(..., retain_graph=True) on one head's loss, then the backward of a second head's loss through the
    shared backbone graph: the backbone's .grad is g(loss 1) + g(loss 2) of two separate runs (torch's own optimizer steps the
    first head only, so no saved tensor of the shared part moves)."""
    from lipvq_vae_amd import optim
    gpt, gmm, det = C.get("gpt"), C.get("gmm_softplus_view"), C.get("head_view")
    T, E = C.HEAD["T"], C.HEAD["E"]

    def graph():
        lv, fwd = build(gpt)
        lv_g, _ = build(gmm)
        lv_d, _ = build(det)
        from lipvq_vae_amd.nnfn import LinearFn
        from lipvq_vae_amd.ops import ACT_NONE
        proj = C._randn(("retain", "proj"), E, C.GPT["embed_dim"], scale=0.2).cuda()
        feats = LinearFn.apply(fwd()["out"], proj, None, ACT_NONE)[:, -T:]            # [B, T, E], a non-contiguous view
        from lipvq_vae_amd.action_head import _LossesFn
        from lipvq_vae_amd.gmm import _LogProbFn
        h = C.HEAD
        loss1 = _LossesFn.apply(feats, det.info["target"].cuda(), lv_d["nets.action.weight"], lv_d["nets.action.bias"], det.info["weights"])[3]
        loss2 = -_LogProbFn.apply(feats, gmm.info["actions"].cuda(), *(lv_g[k] for k in C.gmm_ref.KEYS), h["M"], h["A"], 0, 0.01, True)[1]
        return lv, lv_d, lv_g, loss1, loss2

    lv, lv_d, lv_g, loss1, loss2 = graph()
    loss1.backward()
    g1 = {k: t.grad.clone() for k, t in lv.items()}
    lv, lv_d, lv_g, loss1, loss2 = graph()
    loss2.backward()
    g2 = {k: t.grad.clone() for k, t in lv.items()}
    lv, lv_d, lv_g, loss1, loss2 = graph()
    loss1.backward()
    assert all(torch.equal(lv[k].grad, g1[k]) for k in lv), "two identical runs differ: no bit claim can be made"

    lv, lv_d, lv_g, loss1, loss2 = graph()
    w_before = lv_d["nets.action.weight"].detach().clone()
    head_params = [lv_d[k] for k in det.params]
    sgd = torch.optim.SGD(head_params, lr=0.1)
    norm = optim.backprop_for_loss(torch.nn.ParameterList(head_params), sgd, loss1, retain_graph=True)
    assert norm > 0 and not torch.equal(lv_d["nets.action.weight"].detach(), w_before)
    loss2.backward()
    for k, t in lv.items():
        assert torch.equal(t.grad, g1[k] + g2[k]), k
    assert all(lv_g[k].grad is not None for k in gmm.params)


def test_default_branch_two_training_forwards_then_the_backward_of_the_first():
    """Each training forward runs one power iteration in place on weight_u / weight_v; the backward of the FIRST call must use the
    first call's u, v and sigma (the clones _SpectralFn saves), as the stock hook's does."""
    case = C.get("default_L1_first_of_two")
    outs, grads = run(case)
    against_reference(case, outs, grads, tag=" [first of two forwards]")
    single = run(C.get("default_L1"))[1]
    assert same_bits(single, run(C.get("default_L1"))[1]), "two identical runs differ: no bit claim can be made"
    assert same_bits(grads, single), "the second forward changed the first one's backward"


def test_add_layernorm_of_a_tensor_with_itself():
    """AddLayerNormFn.apply(a, a, ...): backward returns the same tensor for both inputs; a.grad must be twice the one-sided
    gradient of the same forward values."""
    from lipvq_vae_amd.nnfn import AddLayerNormFn
    case = C.get("addln_ab")
    a0, w, bias = case.leaves["in.a"], case.leaves["w"].cuda(), case.leaves["bias"].cuda()
    Rs, Ry = case.R["s"].cuda(), case.R["y"].cuda()
    a = _cuda_leaf(a0)
    s, y = AddLayerNormFn.apply(a, a, w, bias, X.LN_EPS, True)
    ((s * Rs).sum() + (y * Ry).sum()).backward()
    a1, b1 = _cuda_leaf(a0), a0.clone().cuda()
    s1, y1 = AddLayerNormFn.apply(a1, b1, w, bias, X.LN_EPS, True)
    ((s1 * Rs).sum() + (y1 * Ry).sum()).backward()
    a2 = _cuda_leaf(a0)
    s2, y2 = AddLayerNormFn.apply(a2, b1, w, bias, X.LN_EPS, True)
    ((s2 * Rs).sum() + (y2 * Ry).sum()).backward()
    assert torch.equal(a2.grad, a1.grad) and torch.equal(s2, s1), "two identical runs differ: no bit claim can be made"
    assert torch.equal(s1, s) and torch.equal(y1, y)
    assert torch.equal(a.grad, a1.grad + a1.grad)
    # and two leaves a, b end with equal values in separate tensors: writing one leaves the other
    lv, fwd = build(case)
    objective(case, fwd()).backward()
    keep = lv["in.b"].grad.clone()
    assert torch.equal(lv["in.a"].grad, keep) and lv["in.a"].grad.data_ptr() != lv["in.b"].grad.data_ptr()
    lv["in.a"].grad.mul_(2.0)
    assert torch.equal(lv["in.b"].grad, keep)


def test_gmm_weight_gradients_share_a_buffer_and_stay_apart():
    """The three weight gradients (and the three bias gradients) come back as row slices of one buffer: an in-place mul_ on one
    .grad leaves the other two unchanged."""
    case = C.get("gmm_softplus_dense")
    lv, fwd = build(case)
    objective(case, fwd()).backward()
    for kind in ("weight", "bias"):
        names = [f"nets.{g}.{kind}" for g in ("mean", "scale", "logits")]
        before = {k: lv[k].grad.clone() for k in names}
        lv[names[1]].grad.mul_(3.0)
        assert torch.equal(lv[names[1]].grad, 3.0 * before[names[1]])
        assert torch.equal(lv[names[0]].grad, before[names[0]]) and torch.equal(lv[names[2]].grad, before[names[2]])
        lv[names[0]].grad.zero_()
        assert torch.equal(lv[names[2]].grad, before[names[2]]) and torch.equal(lv[names[1]].grad, 3.0 * before[names[1]])


# ---------------------------------------------------------------------------------------------------
# forward identity; tokenizer inputs
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["llfq_n64", "vq_n64"] + list(FUSED_NAMES))
def test_tokenizer_forwards_return_the_same_bits(name):
    """The grad-mode forward, the no_grad forward, the all-frozen forward and forward_backward: one z_latent, one loss; and
    forward_backward's gradients are loss.backward()'s (bits where two backward runs agree, the bound otherwise)."""
    from lipvq_vae_amd.autograd import forward_backward
    case = C.get(name)
    lv, fwd = build(case)
    m, x = fwd.module, fwd.x
    z, loss = m(x)
    z_again, loss_again = m(x)
    assert torch.equal(z_again, z) and torch.equal(loss_again, loss), "two identical forwards differ: no bit claim can be made"
    loss.backward()
    with torch.no_grad():
        z_ng, loss_ng = m(x)
    z_fb, loss_fb, params, grads = forward_backward(m, x)
    for t in lv.values():
        t.requires_grad_(False)
    z_fr, loss_fr = m(x)
    for what, (zz, ll) in {"no_grad": (z_ng, loss_ng), "forward_backward": (z_fb, loss_fb), "frozen": (z_fr, loss_fr)}.items():
        assert torch.equal(zz, z) and torch.equal(ll, loss.detach()) and not zz.requires_grad and not ll.requires_grad, (name, what)
    dev_g = C.dev(case)[1]
    by_id = {id(p): k for k, p in lv.items()}
    for p, g in zip(params, grads):
        k = by_id[id(p)]
        b = X.bound(X.BWD_TOL, dev_g[k])
        err = X.rel(g.cpu(), p.grad.cpu())
        print(f"{name} forward_backward {k}: {err:.3e} from loss.backward(), bound {b:.3e}")
        assert err <= b, (name, k, err)


@pytest.mark.parametrize("name", ["llfq_n64", "vq_n64"])
def test_tokenizer_inputs_get_no_gradient(name):
    """Pinned, not endorsed: the reference returns a gradient for the actions (the loss depends on x through the encoder and the
    reconstruction error); this library returns none.  With a trainable parameter, x.grad stays None after loss.backward(); with
    every parameter frozen, tokenizer_forward takes the no-autograd path and the loss does not require a gradient although x
    does."""
    case = C.get(name)
    lv, fwd = build(case)
    m = fwd.module
    x = fwd.x.clone().requires_grad_(True)
    z, loss = m(x)
    assert loss.requires_grad and not z.requires_grad
    assert torch.equal(m(x)[1], loss), "two identical forwards differ: no bit claim can be made"
    loss.backward()
    assert x.grad is None and all(t.grad is not None for t in lv.values())
    gx, = torch.autograd.grad(m(x)[1], [x], allow_unused=True)
    assert gx is None
    ref_x = case.info["x"].double().requires_grad_(True)          # the reference does have one
    restatement = C.O.torch_llfq_forward if case.info["variant"] == "llfq" else C.O.torch_vq_forward
    restatement({k: v.double() for k, v in case.leaves.items()}, ref_x)[1].backward()
    assert float(ref_x.grad.abs().max()) > 0
    for t in lv.values():
        t.requires_grad_(False)
    z, loss_frozen = m(x)
    assert not loss_frozen.requires_grad and torch.equal(loss_frozen, loss.detach())


# ---------------------------------------------------------------------------------------------------
# second order is refused
# ---------------------------------------------------------------------------------------------------

def _second_order_targets():
    """(the Functions whose backward the first differentiation runs, case name, output, leaf to differentiate)."""
    return [("LinearFn+AddLayerNormFn+gpt._AttentionFn", "gpt", "out", "in.x"),
            ("AddLayerNormFn", "addln_ab", "y", "in.a"),
            ("default_branch._SpectralFn+_AttentionFn", "default_L1", "out", "in.x"),
            ("default_branch._SpectralFn (weight_orig)", "default_L1", "out", "0.weight_orig"),
            ("embedding._EmbedStreamsFn", "embed_parameter_dense", "out", "in.obs"),
            ("gmm._LogProbFn", "gmm_softplus_dense", "log_prob", "in.feats"),
            ("gmm._ParamsFn", "gmm_softplus_dense", "mean", "in.feats"),
            ("action_head._ActionsFn", "head_dense", "actions", "in.feats"),
            ("action_head._LossesFn", "head_dense", "action_loss", "in.feats"),
            ("binning._BinFn", "bin_a7", "out", "output_layer.2.weight"),
            ("autograd._TokenizerFn llfq", "llfq_n64", "loss", "to_output.weight"),
            ("autograd._TokenizerFn vq", "vq_n64", "loss", "decoder.4.weight")]


@pytest.mark.parametrize("what,name,key,leaf", _second_order_targets(), ids=[t[0] for t in _second_order_targets()])
def test_second_order_is_refused(what, name, key, leaf):
    """The backward kernels return graph-less tensors.  gx = grad(out.sum(), x, create_graph=True) still gives the first-order
    numbers, but a loss that adds a function of gx to an ordinary term must raise instead of training on the ordinary term alone."""
    case = C.get(name)
    lv, fwd = build(case)
    out = fwd()[key]
    gx, = torch.autograd.grad(out.sum(), lv[leaf], create_graph=True)
    assert gx.requires_grad, f"{what}: the gradient left create_graph=True without an error node behind it"
    with pytest.raises(RuntimeError, match="differentiable once only|once_differentiable"):
        (out.sum() + gx.square().sum()).backward()


def test_every_function_is_marked_first_order_only():
    """Every torch.autograd.Function of the package (twelve classes): backward is wrapped by nnfn.first_order_only, itself over
    once_differentiable."""
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd import action_head, autograd, binning, default_branch, embedding, gmm, gpt, nnfn
    fns = [nnfn.LinearFn, nnfn.AddLayerNormFn, gpt._AttentionFn, default_branch._SpectralFn, default_branch._AttentionFn,
           embedding._EmbedStreamsFn, gmm._LogProbFn, gmm._ParamsFn, action_head._ActionsFn, action_head._LossesFn, binning._BinFn,
           autograd._TokenizerFn]
    assert len(fns) == 12 and len({f.__qualname__ + f.__module__ for f in fns}) == 12
    for f in fns:
        assert getattr(f.backward, "first_order_only", False) and callable(getattr(f.backward, "__wrapped__", None)), f
