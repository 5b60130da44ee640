"""The cases of the autograd contract (tests/test_gpu_autograd_contract.py) and their float64 references -- plain seeded torch on
the CPU, no GPU; tests/test_autograd_cases_host.py checks that the references are what they claim and that a wrong gradient of
the kind each property guards against leaves the bound.

A case is one module (or one Function) at its smallest useful shape: its differentiable LEAVES (parameters by their
``state_dict`` key, inputs as ``in.<name>``), the parameter GROUPS that freeze together, and ``fwd``: the existing restatement of
the operation (gpt_ref, gmm_ref, action_head_ref, the oracle's torch_* functions, stock torch modules for the default branch) as
a function of the leaves in any float dtype.  No operation is restated here.  ``evaluate`` runs it through stock autograd with a
chosen subset of the leaves trainable and a chosen use of the outputs:

    objective = sum over outputs k of coeff[k] * (out_k * R_k).sum()          (R_k: fixed seeded tensors; coeff 0 = output unused)

The yardstick is the suite's own (xf_edge_inputs): a gradient's bound is ``X.bound(BWD_TOL, dev)``, an output's
``X.bound(FWD_TOL, dev)``, with ``dev`` the fp32 run of the same restatement against its float64 run on the same inputs, the
same trainable set and the same coefficients.  ``dev`` never comes from the code under test.
"""
import functools
import warnings
import zlib
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

import action_head_ref
import gmm_ref
import gpt_ref
import xf_edge_inputs as X
from oracle import lipvq_oracle as O

GOLDEN = Path(__file__).resolve().parent / "golden"
MARGIN = 10.0                     # a wrong evaluation must miss the bound by this factor, or the case cannot notice the bug


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randn(key, *shape, scale=1.0):
    return torch.randn(*shape, generator=_gen(*key)) * scale


class Case:
    """name; leaves {name: fp32 CPU tensor}; groups {group: (parameter leaf names)}; inputs (leaf names); biases (leaf names);
    fwd(t, dtype) -> {output name: tensor}; R {output name: fp32 tensor of the output's shape}; info: what the GPU side needs to
    build the module (shapes, non-differentiable inputs)."""

    def __init__(self, name, kind, leaves, groups, inputs, biases, fwd, info=None, r_key=None):
        self.name, self.kind, self.leaves, self.groups, self.inputs, self.biases = name, kind, leaves, groups, tuple(inputs), tuple(biases)
        self.fwd, self.info = fwd, info or {}
        self.params = tuple(k for k in leaves if k not in self.inputs)
        assert sorted(sum((list(v) for v in groups.values()), [])) == sorted(self.params), name
        with torch.no_grad():
            outs = fwd({k: v.double() for k, v in leaves.items()}, torch.float64)
        self.outputs = tuple(outs)
        self.R = {k: _randn(("R", r_key or name, k), *v.shape) if v.dim() else torch.ones(()) * (1.0 + 0.25 * i)
                  for i, (k, v) in enumerate(outs.items())}

    def patterns(self):
        """[(label, frozenset of trainable leaves)]: each group alone trainable, each group alone frozen, biases only, input only,
        parameters only.  Patterns that coincide (a case with one group, no input, no bias) are listed once."""
        every = frozenset(self.leaves)
        out = [(f"only_{g}", frozenset(v)) for g, v in self.groups.items()]
        out += [(f"frozen_{g}", every - frozenset(v)) for g, v in self.groups.items()]
        out += [("biases_only", frozenset(self.biases)), ("input_only", frozenset(self.inputs)), ("params_only", frozenset(self.params))]
        seen, uniq = {every}, []
        for label, tr in out:
            if tr and tr not in seen:
                seen.add(tr)
                uniq.append((label, tr))
        return uniq


def _coeff_key(case, coeff):
    coeff = {k: 1.0 for k in case.outputs} if coeff is None else coeff
    assert set(coeff) <= set(case.outputs), (case.name, coeff)
    return tuple((k, float(coeff.get(k, 0.0))) for k in case.outputs)


@functools.lru_cache(maxsize=None)
def _evaluate(name, dtype, trainable, coeff):
    case = get(name)
    t = {k: v.to(dtype).clone().requires_grad_(trainable is None or k in trainable) for k, v in case.leaves.items()}
    outs = case.fwd(t, dtype)
    obj = sum(c * (outs[k] * case.R[k].to(dtype)).sum() for k, c in coeff if c != 0.0)
    if any(v.requires_grad for v in t.values()) and torch.is_tensor(obj) and obj.requires_grad:
        obj.backward()
    return {k: v.detach() for k, v in outs.items()}, {k: v.grad for k, v in t.items()}


def evaluate(case, dtype=torch.float64, trainable=None, coeff=None):
    """(outputs, gradients) of the restatement in `dtype` through stock autograd: leaves outside `trainable` (None = all) do not
    require a gradient and get None; coeff {output: factor} (None = every output with factor 1).  Computed once per argument set;
    the tensors are shared: do not write to them."""
    return _evaluate(case.name, dtype, None if trainable is None else frozenset(trainable), _coeff_key(case, coeff))


def dev(case, trainable=None, coeff=None):
    """({output: dev}, {leaf: dev}) of the fp32 restatement against the float64 one: the yardstick of X.bound."""
    o64, g64 = evaluate(case, torch.float64, trainable, coeff)
    o32, g32 = evaluate(case, torch.float32, trainable, coeff)
    return ({k: X.rel(o32[k], o64[k]) for k in o64}, {k: X.rel(g32[k], g64[k]) for k in g64 if g64[k] is not None})


def check(what, got, want, dev_, tol):
    """Print the figure (X.report) and return the failure or None."""
    what, err, b = X.report(what, X.rel(got, want), dev_, tol)
    return None if err <= b else (what, err, b)


# ---------------------------------------------------------------------------------------------------
# nnfn.AddLayerNormFn on its own
# ---------------------------------------------------------------------------------------------------

ADDLN_N, ADDLN_E = 5, 8


def _addln(with_b):
    name = "addln_ab" if with_b else "addln_a"
    leaves = {"in.a": _randn((name, "a"), ADDLN_N, ADDLN_E)}
    if with_b:
        leaves["in.b"] = _randn((name, "b"), ADDLN_N, ADDLN_E)
    leaves["w"] = 1.0 + 0.3 * _randn((name, "w"), ADDLN_E)
    leaves["bias"] = 0.3 * _randn((name, "bias"), ADDLN_E)

    def fwd(t, dtype):
        s = t["in.a"] + t["in.b"] if with_b else t["in.a"] * 1.0
        return {"s": s, "y": F.layer_norm(s, (ADDLN_E,), t["w"], t["bias"], X.LN_EPS)}

    return Case(name, "addln", leaves, {"affine": ("w", "bias")}, [k for k in leaves if k.startswith("in.")], ("bias",), fwd,
                {"with_b": with_b, "eps": X.LN_EPS})


# ---------------------------------------------------------------------------------------------------
# GPTBackbone: embed_dim 32, 2 heads (head width 16), context 33 (two key tiles), 2 layers, B = 2
# ---------------------------------------------------------------------------------------------------

GPT = dict(embed_dim=32, num_heads=2, context_length=33, num_layers=2, B=2)
GPT_DROP_KEEP = 0.75


def gpt_state(key="gpt"):
    """A GPTBackbone state_dict by its keys (the reference's initial LayerNorms are 1 / 0 and its biases 0: a trained-like draw
    instead, so that every term carries a gradient)."""
    E, L, n = GPT["embed_dim"], GPT["context_length"], GPT["num_layers"]
    sd = {}
    for i in range(n):
        p = f"nets.transformer.{i}.nets."
        sd[p + "attention.nets.qkv.weight"] = _randn((key, i, "qkv"), 3 * E, E, scale=E ** -0.5)
        sd[p + "attention.nets.output.weight"] = _randn((key, i, "ow"), E, E, scale=E ** -0.5)
        sd[p + "attention.nets.output.bias"] = _randn((key, i, "ob"), E, scale=0.1)
        sd[p + "attention.mask"] = gpt_ref.causal_mask(L)
        sd[p + "mlp.0.weight"] = _randn((key, i, "m0w"), 4 * E, E, scale=E ** -0.5)
        sd[p + "mlp.0.bias"] = _randn((key, i, "m0b"), 4 * E, scale=0.1)
        sd[p + "mlp.2.weight"] = _randn((key, i, "m2w"), E, 4 * E, scale=(4 * E) ** -0.5)
        sd[p + "mlp.2.bias"] = _randn((key, i, "m2b"), E, scale=0.1)
        for ln in ("ln1", "ln2"):
            sd[p + ln + ".weight"] = 1.0 + 0.2 * _randn((key, i, ln, "w"), E)
            sd[p + ln + ".bias"] = 0.2 * _randn((key, i, ln, "b"), E)
    sd["nets.output_ln.weight"] = 1.0 + 0.2 * _randn((key, "oln", "w"), E)
    sd["nets.output_ln.bias"] = 0.2 * _randn((key, "oln", "b"), E)
    return sd


def _gpt():
    sd = gpt_state()
    masks = {k: v for k, v in sd.items() if k.endswith(".mask")}
    leaves = {k: v for k, v in sd.items() if k not in masks}
    leaves["in.x"] = _randn(("gpt", "x"), GPT["B"], GPT["context_length"], GPT["embed_dim"])
    groups = {"ln": tuple(k for k in leaves if ".ln1." in k or ".ln2." in k), "qkv": tuple(k for k in leaves if ".qkv." in k),
              "attn_out": tuple(k for k in leaves if ".output." in k), "mlp": tuple(k for k in leaves if ".mlp." in k),
              "output_ln": tuple(k for k in leaves if "output_ln" in k)}

    def fwd(t, dtype):
        full = dict(t, **{k: v.to(dtype) for k, v in masks.items()})
        return {"out": gpt_ref.gpt_forward(full, t["in.x"], GPT["num_layers"], GPT["num_heads"])}

    return Case("gpt", "gpt", leaves, groups, ("in.x",), tuple(k for k in leaves if k.endswith(".bias")), fwd, {"masks": masks})


def _gpt_dropout():
    """One block with FIXED keep masks (attention probabilities, attention output, mlp output), through gpt_ref.block_forward:
    what the GPU side reaches through the Functions directly (the module draws its own masks)."""
    E, L, H, B = GPT["embed_dim"], GPT["context_length"], GPT["num_heads"], GPT["B"]
    sd = {k[len("nets.transformer.0.nets."):]: v for k, v in gpt_state("gpt_dropout").items() if k.startswith("nets.transformer.0.")}
    mask = sd.pop("attention.mask")
    leaves = dict(sd)
    leaves["in.x"] = _randn(("gpt_dropout", "x"), B, L, E)
    keeps = tuple((torch.rand(*shape, generator=_gen("gpt_dropout", "keep", i)) < GPT_DROP_KEEP).to(torch.uint8)
                  for i, shape in enumerate(((B, H, L, L), (B, L, E), (B, L, E))))
    groups = {"ln": tuple(k for k in leaves if k.startswith("ln")), "qkv": ("attention.nets.qkv.weight",),
              "attn_out": tuple(k for k in leaves if ".output." in k), "mlp": tuple(k for k in leaves if k.startswith("mlp."))}

    def fwd(t, dtype):
        full = dict(t, **{"attention.mask": mask.to(dtype)})
        return {"out": gpt_ref.block_forward(full, "", t["in.x"], H, keeps, (GPT_DROP_KEEP,) * 3)}

    return Case("gpt_dropout", "gpt_dropout", leaves, groups, ("in.x",), tuple(k for k in leaves if k.endswith(".bias")), fwd,
                {"keeps": keeps, "keep_prob": GPT_DROP_KEEP})


# ---------------------------------------------------------------------------------------------------
# the two output heads: E = 8, A = 3, B = 2, T = 3; feats contiguous or the [:, -T:] view of a [B, 3T, E] leaf
# ---------------------------------------------------------------------------------------------------

HEAD = dict(E=8, A=3, B=2, T=3, M=2)
HEAD_WEIGHTS = (1.0, 0.5, 0.25)                     # l2, l1, cos: all three non-zero


def _feats(name, layout):
    B, T, E = HEAD["B"], HEAD["T"], HEAD["E"]
    if layout == "dense":
        return "in.feats", _randn((name, "feats"), B, T, E), (lambda t: t["in.feats"])
    return "in.base", _randn((name, "base"), B, 3 * T, E), (lambda t: t["in.base"][:, -T:])


def _gmm(act, layout):
    name = f"gmm_{act}_{layout}"
    E, A, M, B, T = (HEAD[k] for k in ("E", "A", "M", "B", "T"))
    shapes = {"mean": M * A, "scale": M * A, "logits": M}
    leaves = {}
    for g, rows in shapes.items():
        leaves[f"nets.{g}.weight"] = _randn((name, g, "w"), rows, E, scale=E ** -0.5)
        leaves[f"nets.{g}.bias"] = _randn((name, g, "b"), rows, scale=0.3)
    in_name, in_val, view = _feats(name, layout)
    leaves[in_name] = in_val
    actions = torch.tanh(_randn((name, "actions"), B, T, A))

    def fwd(t, dtype):
        feats = view(t)
        pm, ps, lg = gmm_ref.decoder(t, feats, M, A)
        mu, sg = gmm_ref.activate(pm, ps, 0.01, act)
        lp = gmm_ref.mixture(mu, sg, lg).log_prob(actions.to(dtype))
        return {"log_prob": lp, "sum": lp.sum(), "mean": mu, "scale": sg, "logits": lg}

    return Case(name, "gmm", leaves, {g: (f"nets.{g}.weight", f"nets.{g}.bias") for g in shapes}, (in_name,),
                tuple(k for k in leaves if k.endswith(".bias")), fwd, {"act": act, "layout": layout, "actions": actions, "min_std": 0.01})


GMM_LOGPROB_USES = {"log_prob": {"log_prob": 1.0}, "sum": {"sum": 1.0}, "both": {"log_prob": 0.7, "sum": -1.3}}
GMM_PARAM_USES = {"+".join(s): {k: 1.0 for k in s} for s in (("mean",), ("scale",), ("logits",), ("mean", "scale"), ("mean", "logits"),
                                                               ("scale", "logits"), ("mean", "scale", "logits"))}


def _head(layout):
    name = f"head_{layout}"
    E, A, B, T = (HEAD[k] for k in ("E", "A", "B", "T"))
    leaves = {"nets.action.weight": _randn((name, "w"), A, E, scale=E ** -0.5), "nets.action.bias": _randn((name, "b"), A, scale=0.3)}
    in_name, in_val, view = _feats(name, layout)
    leaves[in_name] = in_val
    target = torch.tanh(_randn((name, "target"), B, T, A))

    def fwd(t, dtype):
        acts = action_head_ref.actions(t, view(t))
        return dict({"actions": acts}, **action_head_ref.compute_losses(acts, target.to(dtype), HEAD_WEIGHTS))

    return Case(name, "head", leaves, {"weight": ("nets.action.weight",), "bias": ("nets.action.bias",)}, (in_name,),
                ("nets.action.bias",), fwd, {"layout": layout, "target": target, "weights": HEAD_WEIGHTS})


HEAD_USES = {"actions": {"actions": 1.0}, "action_loss": {"action_loss": 1.0},
             "each_loss": {"l2_loss": 0.7, "l1_loss": -1.3, "cos_loss": 0.9, "action_loss": 1.1}}


# ---------------------------------------------------------------------------------------------------
# ICLInputEmbedding: input_dim 8, E = 8, T = 3, B = 2, K = 16; three time-embedding modes; dense and index + codebook routes
# ---------------------------------------------------------------------------------------------------

EMBED = dict(Din=8, E=8, T=3, B=2, K=16)


def _embed(mode, route):
    name = f"embed_{mode}_{route}"
    Din, E, T, B, K = (EMBED[k] for k in ("Din", "E", "T", "B", "K"))
    ep = O.to_torch(O.make_embed_params(17, Din, E, T, mode))
    leaves = dict(ep)
    leaves["in.obs"] = _randn((name, "obs"), B, T, Din)
    leaves["in.context_obs"] = _randn((name, "cobs"), B, T, Din)
    codebook = torch.rand(K, Din, generator=_gen(name, "codebook"))
    idx = torch.randint(0, K, (B, T), generator=_gen(name, "idx"))
    if route == "dense":
        leaves["in.context_actions"] = codebook[idx].clone()
    groups = {"encoder": ("embed_encoder.weight", "embed_encoder.bias"), "ln": ("embed_ln.weight", "embed_ln.bias")}
    time_key = {"parameter": "embed_timestep", "embedding": "embed_timestep.weight"}.get(mode)
    if time_key:
        groups["time"] = (time_key,)

    def fwd(t, dtype):
        ca = t["in.context_actions"] if route == "dense" else codebook[idx].to(dtype)       # z_latent is detached in the reference
        return {"out": O.torch_transformer_embeddings(t, t["in.obs"], t["in.context_obs"], ca)}

    return Case(name, "embed", leaves, groups, tuple(k for k in leaves if k.startswith("in.")), ("embed_encoder.bias", "embed_ln.bias"),
                fwd, {"mode": mode, "route": route, "codebook": codebook, "idx": idx})


# ---------------------------------------------------------------------------------------------------
# AdaptiveBinActionEmbedding at the bin_a7 fixture's widths, N = 17
# ---------------------------------------------------------------------------------------------------

BIN_N = 17


def _bin():
    g = np.load(GOLDEN / "bin_a7.npz")
    meta = dict(eval(str(g["meta"])))
    A, D, nb = meta["A"], meta["D"], meta["nb"]
    leaves = O.to_torch(O.make_bin_params(meta["seed"], A, D, nb))
    actions = torch.from_numpy(np.ascontiguousarray(g["x0"][:BIN_N]))
    groups = {"embeddings": tuple(k for k in leaves if k.startswith("embedding_layers.")),
              "l1": ("output_layer.0.weight", "output_layer.0.bias"), "l2": ("output_layer.2.weight", "output_layer.2.bias")}
    inf = torch.full((A,), float("inf"))

    def fwd(t, dtype):
        return {"out": O.torch_bin_forward(t, actions, inf, -inf, update=True)[0]}      # (actions and boundaries stay fp32: bins only)

    return Case("bin_a7", "bin", leaves, groups, (), ("output_layer.0.bias", "output_layer.2.bias"), fwd,
                {"A": A, "D": D, "nb": nb, "actions": actions})


# ---------------------------------------------------------------------------------------------------
# DefaultActionNetwork: A = 7, D = 64, N = 17, 1 and 2 layers, dropout 0 -- the stock modules, in training mode
# ---------------------------------------------------------------------------------------------------

DEFAULT = dict(A=7, D=64, N=17, seed=5)
DEFAULT_GROUPS = {"spectral": ("0.", "2.", "4."), "attention": (".self_attn.",), "feedforward": (".linear1.", ".linear2."),
                  "norms": (".norm1.", ".norm2."), "closing": ("6.",)}


def default_state(num_layers):
    """make_default_branch_params' state (4 layers) cut to its first num_layers layers."""
    p = O.make_default_branch_params(DEFAULT["seed"], DEFAULT["A"], DEFAULT["D"])
    keep = lambda k: not k.startswith("5.layers.") or int(k.split(".")[2]) < num_layers            # noqa: E731
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items() if keep(k)}


def stock_default_branch(state, num_layers, dtype):
    """The reference's constructor text with stock torch modules (O.build_default_branch_modules with num_layers layers), loaded
    with `state`, in training mode with every dropout probability at 0."""
    import torch.nn as nn
    from torch.nn.utils import spectral_norm
    A, D = DEFAULT["A"], DEFAULT["D"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        layer = nn.TransformerEncoderLayer(d_model=D, nhead=O.DEFAULT_NHEAD, dim_feedforward=O.DEFAULT_FF, activation="gelu")
        net = nn.Sequential(spectral_norm(nn.Linear(A, 64)), nn.GELU(), spectral_norm(nn.Linear(64, 128)), nn.GELU(),
                            spectral_norm(nn.Linear(128, D)), nn.TransformerEncoder(layer, num_layers=num_layers), nn.Linear(D, D))
    net = net.to(dtype).train()
    net.load_state_dict(state, strict=False)                  # (strict=False: `weight` of the hooked Linears is derived state)
    for m in net.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
        if isinstance(m, nn.MultiheadAttention):
            m.dropout = 0.0
    return net


def _default(num_layers, calls=1, use=0):
    """calls = 2: TWO training forwards (two power iterations); use = 0: the objective on the FIRST call's output, whose backward
    must use the first call's u, v, sigma (the stock hook clones them for this); use = 1: on the second call's -- the host test's
    stand-in for a backward that read the second call's state."""
    name = f"default_L{num_layers}" + ("" if calls == 1 else "_first_of_two" if use == 0 else "_second_of_two")
    state = default_state(num_layers)
    uv = {k: v for k, v in state.items() if k.endswith("_u") or k.endswith("_v")}
    leaves = {k: v for k, v in state.items() if k not in uv}
    leaves["in.x"] = _randn((f"default_L{num_layers}", "x"), DEFAULT["N"], DEFAULT["A"])     # (the _of_two variants share x and R)
    groups = {g: tuple(k for k in leaves if k != "in.x" and any((k.startswith(p) if p[0] != "." else p in k) for p in pats))
              for g, pats in DEFAULT_GROUPS.items()}

    def fwd(t, dtype):
        net = stock_default_branch(dict(uv, **{k: v.detach() for k, v in t.items() if k != "in.x"}), num_layers, dtype)
        named = dict(net.named_parameters())
        for k, v in t.items():                                   # the leaves ARE the module's parameters
            if k != "in.x":
                mod, _, attr = k.rpartition(".")
                del net.get_submodule(mod)._parameters[attr]
                setattr(net.get_submodule(mod), attr, v)
                assert k in named
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            outs = [net(t["in.x"]) for _ in range(calls)]
        return {"out": outs[use]}

    return Case(name, "default", leaves, groups, ("in.x",), tuple(k for k in leaves if k.endswith("bias")), fwd,
                {"num_layers": num_layers, "calls": calls, "state": state}, r_key=f"default_L{num_layers}")


# ---------------------------------------------------------------------------------------------------
# the tokenizers: A = 7, D = 32, K = 128, N = 64 (the small routes) and the smallest N of the fused training launch
# ---------------------------------------------------------------------------------------------------

TOK = dict(A=7, D=32, K=128, N=64, seed=5)
TOK_GROUPS = {"llfq": {"encoder": ("encoder.",), "to_latent": ("to_latent.",), "codebook": ("quantizer.",), "decoder": ("decoder.", "to_output.")},
              "vq": {"encoder": ("encoder.",), "codebook": ("embedding.",), "decoder": ("decoder.",)}}


def _tokenizer(variant, N):
    name = f"{variant}_n{N}"
    A, D, K = TOK["A"], TOK["D"], TOK["K"]
    leaves = O.to_torch(O.make_params(TOK["seed"], A, D, K, variant=variant))
    x = torch.from_numpy(O.make_inputs(TOK["seed"], N, A))
    groups = {g: tuple(k for k in leaves if k.startswith(pats)) for g, pats in TOK_GROUPS[variant].items()}
    restatement = O.torch_llfq_forward if variant == "llfq" else O.torch_vq_forward

    def fwd(t, dtype):
        return {"loss": restatement(t, x.to(dtype))[1]}

    return Case(name, "tokenizer", leaves, groups, (), tuple(k for k in leaves if k.endswith(".bias") or k.endswith(".b")), fwd,
                {"variant": variant, "x": x, "N": N})


_BUILDERS = {
    "addln_ab": lambda: _addln(True), "addln_a": lambda: _addln(False),
    "gpt": _gpt, "gpt_dropout": _gpt_dropout,
    "bin_a7": _bin,
    "default_L1": lambda: _default(1), "default_L2": lambda: _default(2), "default_L1_first_of_two": lambda: _default(1, calls=2),
    "default_L1_second_of_two": lambda: _default(1, calls=2, use=1),
    "llfq_n64": lambda: _tokenizer("llfq", TOK["N"]), "vq_n64": lambda: _tokenizer("vq", TOK["N"]),
}
_BUILDERS.update({f"gmm_{a}_{lay}": functools.partial(_gmm, a, lay) for a in ("softplus", "exp") for lay in ("dense", "view")})
_BUILDERS.update({f"head_{lay}": functools.partial(_head, lay) for lay in ("dense", "view")})
_BUILDERS.update({f"embed_{m}_{r}": functools.partial(_embed, m, r) for m in O.EMBED_MODES for r in ("dense", "index")})

NAMES = tuple(_BUILDERS)
FREEZE_NAMES = tuple(n for n in NAMES if not n.endswith("_of_two"))


def fused_train_rows():
    """The smallest N at which the tokenizers' _plan leaves the small routes for the fused training launch: one row more than
    _TokenizerBase.EXACT_ROWS_MAX, read from lipvq-vae_amd/tokenizer.py's text (no import of the package here)."""
    import re
    text = (Path(__file__).resolve().parent.parent / "lipvq-vae_amd" / "tokenizer.py").read_text()
    return int(re.search(r"^\s+EXACT_ROWS_MAX = (\d+)\s*$", text, re.M).group(1)) + 1


def register_fused():
    """The two cases at fused_train_rows() rows; their names."""
    n = fused_train_rows()
    for v in ("llfq", "vq"):
        _BUILDERS.setdefault(f"{v}_n{n}", functools.partial(_tokenizer, v, n))
    return tuple(f"{v}_n{n}" for v in ("llfq", "vq"))


@functools.lru_cache(maxsize=None)
def get(name):
    return _BUILDERS[name]()
