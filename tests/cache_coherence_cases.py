"""The two tables behind tests/test_gpu_cache_coherence.py and tests/test_cache_coherence_host.py, and the twin builder.

The Python layer keeps copies derived from parameters (packed weights, the prepared codebook, the [K, E] code table, the bin
table, prompt keys and values, the parameter versions a backward checks).  WRITERS lists everything that moves parameters under
those copies, CONSUMERS everything that reads through one.  A test warms a consumer, applies a writer, runs the consumer again
and compares it with a fresh TWIN: a new module of the same constructor arguments, loaded from the written module's
``state_dict()``, that has never run -- nothing cached, the same kernels, so every comparison is ``torch.equal``.

``pairing(writer, consumer)`` says for EVERY pair whether it is tested or why not (a key of NOT_PAIRED): nothing is skipped
silently.  A helper module, not a conftest: it imports torch alone; the package is imported inside the functions.
"""
from __future__ import annotations

import copy
import importlib
from typing import Callable, NamedTuple

import torch
import torch.nn as nn

# ---------------------------------------------------------------------------------------------------------------------------
# subjects: what is built, written and read
# ---------------------------------------------------------------------------------------------------------------------------

T_CTX, E_POL = 4, 64                      # ICLInputEmbedding(input_dim, embed_dim=64, context_length=4); P = 2 T = 8, Lq = T = 4
N_SMALL = 80                              # the ICRT step's batch: the small-batch routes


class Rig(nn.Module):
    """The parts of one subject under one roof: ``tok`` (a tokenizer), ``emb`` (ICLInputEmbedding), ``net`` (GPTBackbone),
    ``bin`` (the bin tokenizer) -- whichever the subject has.  Writers write all of it or one part; consumers read parts."""

    def __init__(self, **parts):
        super().__init__()
        for k, v in parts.items():
            setattr(self, k, v)


# part name -> (module path, class, args, kwargs) per subject; built in this order
_LLFQ = ("tokenizer", "LLFQVAE_V4", (7, 64), {"num_codes": 256})
_VQ = ("tokenizer", "VQVAE", (7, 64), {"num_embeddings": 128})
_ICRT = ("tokenizer", "LLFQVAE_V4", (12, 208), {"num_codes": 1024})       # the shape tests/test_gpu_icl.py captures
_EMB64 = ("embedding", "ICLInputEmbedding", (64,), {"embed_dim": E_POL, "context_length": T_CTX, "emb_dropout": 0.1})
_EMB208 = ("embedding", "ICLInputEmbedding", (208,), {"embed_dim": E_POL, "context_length": T_CTX, "emb_dropout": 0.1})
_NET = ("gpt", "GPTBackbone", (E_POL, 3 * T_CTX), {"num_layers": 2, "num_heads": 4})
_BIN = ("binning", "AdaptiveBinActionEmbedding", (7, 64), {"num_bins": 20})

SUBJECTS = {
    "llfq": {"tok": _LLFQ, "emb": _EMB64},
    "vq": {"tok": _VQ, "emb": _EMB64},
    "icrt": {"tok": _ICRT, "emb": _EMB208},
    "bin": {"bin": _BIN},
    "policy": {"tok": _LLFQ, "emb": _EMB64, "net": _NET},
}


def _construct(subject):
    import lipvq_vae_amd  # noqa: F401
    parts = {}
    for name, (mod, cls, args, kwargs) in SUBJECTS[subject].items():
        parts[name] = getattr(importlib.import_module("lipvq_vae_amd." + mod), cls)(*args, **kwargs)
    return Rig(**parts)


def _oracle_params(rig, seed, oracle):
    """Trained-regime parameters of the rig's tokenizer from the oracle's generator (the default initialisation maps every row
    to one code: no index could ever differ), as a CPU state dict."""
    from oracle import lipvq_oracle as O
    tok = rig.tok
    K, D = tok._codebook().shape
    variant = "llfq" if type(tok).__name__ == "LLFQVAE_V4" else "vq"
    p = O.make_params(seed, tok.feature_dim, D, K, variant=variant, oracle=oracle)
    return {k: torch.from_numpy(v.copy()) for k, v in p.items()}


def build(subject, oracle, seed=0):
    """(rig on the GPU in eval mode, data): seeded parameters, every input a consumer or a writer needs."""
    from oracle import lipvq_oracle as O
    torch.manual_seed(1000 + seed)
    rig = _construct(subject)
    g = torch.Generator().manual_seed(2000 + seed)
    data = {}
    if hasattr(rig, "tok"):
        rig.tok.load_state_dict(_oracle_params(rig, 50 + seed, oracle))
        A, (K, D) = rig.tok.feature_dim, rig.tok._codebook().shape
        n_big = rig.tok.EXACT_ROWS_MAX + 1                     # asserted to be the smallest fused N by the route check
        data["x_big"] = torch.from_numpy(O.make_inputs(60 + seed, n_big, A)).cuda()
        data["x_small"] = torch.from_numpy(O.make_inputs(61 + seed, N_SMALL, A)).cuda()
        data["codes"] = torch.randint(0, K, (300,), generator=g).cuda()
        data["aidx"] = torch.randint(0, K, (3, T_CTX), generator=g).cuda()
    if hasattr(rig, "emb"):
        with torch.no_grad():
            rig.emb.params["embed_timestep"].normal_(generator=g)
        Din = rig.emb.input_dim
        data["obs"], data["ctx_obs"] = (torch.randn(3, T_CTX, Din, generator=g).cuda() for _ in range(2))
    if hasattr(rig, "bin"):
        data["actions"] = torch.randn(64, 7, generator=g).cuda()
    return rig.cuda().eval(), data


def twin_of(subject, written):
    """A fresh rig of the same constructor arguments, each part loaded from the written part's state_dict(); what the state dict
    omits is copied by hand: non-persistent buffers (code_usage), the mode, the bin tokenizer's step bookkeeping and the
    backbone's matmul precision.  It has never run."""
    twin = _construct(subject).cuda()
    for name, part in written.named_children():
        tp = getattr(twin, name)
        tp.load_state_dict(part.state_dict())
        for (_, m), (_, tm) in zip(part.named_modules(), tp.named_modules()):
            for b in m._non_persistent_buffers_set:
                getattr(tm, b).copy_(getattr(m, b))
        for attr in ("_num_step", "_update_enabled", "_matmul_precision"):
            if hasattr(part, attr):
                setattr(tp, attr, getattr(part, attr))
        tp.train(part.training)
    return twin


# ---------------------------------------------------------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------------------------------------------------------

class Writer(NamedTuple):
    fn: Callable              # (module, data, state) -> None, or the written copy (kind "copy")
    kind: str                 # "inplace": same storage, new values | "replace": a tensor object or its storage is replaced |
    #                           "none": no write at all | "copy": a deep copy is written, the original must not move
    scope: str                # "params": any module's parameters | "codebook": a tokenizer's codebook maintenance |
    #                           "tok_step" / "policy_step": the two graphed steps
    api: tuple                # dotted names of what the writer exercises (the host test resolves each)
    prepare: Callable | None = None     # (module, data) -> state, run BEFORE the consumer warms the caches (a graph capture
    #                                     restores parameters in place and invalidates: it would mask a stale cache)


LR, STEPS = 2e-2, 3           # three Adam-family steps of lr 2e-2: every element moves by ~6e-2


def _units(module):
    """The modules whose own load_state_dict / invalidate_caches a writer calls: a rig's parts, or the module itself."""
    return list(module.children()) if isinstance(module, Rig) else [module]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _set_grads(params, seed):
    g = _gen(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(p.device)


def _optimizer_steps(make):
    def fn(module, data, state):
        params = list(module.parameters())
        opt = make(params)
        for s in range(STEPS):
            _set_grads(params, 7 + s)
            opt.step()
        for p in params:
            p.grad = None
    return fn


def _torch_adamw(params):
    return torch.optim.AdamW(params, lr=LR, weight_decay=1e-4)


def _fused(name):
    def make(params):
        from lipvq_vae_amd import optim
        return getattr(optim, name)(params, lr=LR, weight_decay=1e-4)
    return make


def _other_state(unit, seed):
    """A state dict of other values for one module: every parameter scaled and shifted by seeded noise, buffers as they are."""
    g = _gen(seed)
    names = {k for k, _ in unit.named_parameters()}
    return {k: (v.detach().cpu() * 1.25 + 0.1 * torch.randn(v.shape, generator=g)).to(v.device) if k in names
            else v.detach().clone() for k, v in unit.state_dict().items()}


def _load(assign):
    def fn(module, data, state):
        for i, u in enumerate(_units(module)):
            u.load_state_dict(_other_state(u, 11 + i), assign=assign)
    return fn


def _cpu_write_cuda(module, data, state):
    module.cpu()
    with torch.no_grad():
        for p in module.parameters():
            p.mul_(1.5)
    module.cuda()


def _deepcopy_write(module, data, state):
    other = copy.deepcopy(module)
    with torch.no_grad():
        for p in other.parameters():
            p.mul_(1.5)
    return other


def _mul(module, data, state):
    with torch.no_grad():
        for p in module.parameters():
            p.mul_(1.5)


def _copy(module, data, state):
    g = _gen(13)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_((p.cpu() * 0.75 + 0.1 * torch.randn(p.shape, generator=g)).to(p.device))


def _data_assign(module, data, state):
    g = _gen(17)
    for p in module.parameters():
        p.data = (p.detach().cpu() * 1.25 + 0.1 * torch.randn(p.shape, generator=g)).to(p.device)


def _toggle(module, data, state):
    module.train()              # (the rigs are built in eval mode and end in it)
    module.eval()


def _blind_then_invalidate(module, data, state):
    g = _gen(19)
    for p in module.parameters():
        p.data.add_((0.1 * torch.randn(p.shape, generator=g)).to(p.device))      # the version counter does not move
    for u in _units(module):
        if hasattr(u, "invalidate_caches"):
            u.invalidate_caches()


# -- codebook maintenance (module = a rig with a tokenizer; all on the big batch) --
def _ema_prepare(rig, data):
    from lipvq_vae_amd.ema import EMACodebook
    cb = rig.tok._codebook()
    ema = EMACodebook(cb, decay=0.5)
    ema.reset_codes_(torch.arange(cb.shape[0]))              # cluster sizes of 1: an unused code keeps its row
    return ema


def _ema_update(rig, data, ema):
    from lipvq_vae_amd.kmeans import assign
    for _ in range(STEPS):
        z = rig.tok.encode(data["x_big"])
        ema.update(z, assign(z, rig.tok._codebook().detach(), rig.tok._DIST))


def _init_codebook(rig, data, state):
    rig.tok.init_codebook_(data["x_big"], iters=2, generator=_gen(23))


def _revive(with_ema):
    def fn(rig, data, ema):
        # every code counts as dead: all K rows are redrawn from the encoder outputs
        got = rig.tok.revive_dead_codes_(data["x_big"], threshold=1_000_000, generator=_gen(29), ema=ema if with_ema else None)
        assert got.numel() > 0
    return fn


# -- the two graphed steps --
def _tok_step_prepare(rig, data):
    from lipvq_vae_amd.icl import GraphedTokenizerStep
    return GraphedTokenizerStep(rig.tok, data["x_small"], lr=LR)


def _tok_step(rig, data, graphed):
    for _ in range(STEPS):
        graphed.step(data["x_small"])


def policy_loss(rig, data):
    def loss_fn(obs):
        return rig.net(rig.emb(obs, data["ctx_obs"], action_indices=data["aidx"], codebook=rig.tok._codebook())).square().mean()
    return loss_fn


def _policy_step_prepare(rig, data):
    from lipvq_vae_amd import optim
    from lipvq_vae_amd.icl import GraphedPolicyStep
    params = [*rig.emb.parameters(), *rig.net.parameters()]
    return GraphedPolicyStep(policy_loss(rig, data), params, optim.Adam(params, lr=LR), data["obs"])


def _policy_step(rig, data, graphed):
    for _ in range(STEPS):
        graphed.step(data["obs"])


WRITERS = {
    "torch_adamw": Writer(_optimizer_steps(_torch_adamw), "inplace", "params", ("torch.optim.AdamW.step",)),
    "fused_adamw": Writer(_optimizer_steps(_fused("AdamW")), "inplace", "params", ("lipvq_vae_amd.optim.AdamW.step",)),
    "fused_adam": Writer(_optimizer_steps(_fused("Adam")), "inplace", "params", ("lipvq_vae_amd.optim.Adam.step",)),
    "graphed_tokenizer_step": Writer(_tok_step, "inplace", "tok_step", ("lipvq_vae_amd.icl.GraphedTokenizerStep.step",),
                                     _tok_step_prepare),
    "graphed_policy_step": Writer(_policy_step, "inplace", "policy_step", ("lipvq_vae_amd.icl.GraphedPolicyStep.step",),
                                  _policy_step_prepare),
    "load_state_dict": Writer(_load(False), "inplace", "params", ("torch.nn.Module.load_state_dict",)),
    "load_state_dict_assign": Writer(_load(True), "replace", "params", ("torch.nn.Module.load_state_dict",)),
    "cpu_write_cuda": Writer(_cpu_write_cuda, "replace", "params", ("torch.nn.Module.cpu", "torch.nn.Module.cuda")),
    "deepcopy_write": Writer(_deepcopy_write, "copy", "params", ("copy.deepcopy",)),
    "no_grad_mul_": Writer(_mul, "inplace", "params", ("torch.Tensor.mul_",)),
    "no_grad_copy_": Writer(_copy, "inplace", "params", ("torch.Tensor.copy_",)),
    "data_assign": Writer(_data_assign, "replace", "params", ("torch.Tensor.data",)),
    "ema_update": Writer(_ema_update, "inplace", "codebook", ("lipvq_vae_amd.ema.EMACodebook.update",), _ema_prepare),
    "init_codebook_": Writer(_init_codebook, "inplace", "codebook", ("lipvq_vae_amd.tokenizer.LLFQVAE_V4.init_codebook_",)),
    "revive_dead_codes_": Writer(_revive(False), "inplace", "codebook",
                                 ("lipvq_vae_amd.tokenizer.LLFQVAE_V4.revive_dead_codes_",)),
    "revive_dead_codes_ema": Writer(_revive(True), "inplace", "codebook",
                                    ("lipvq_vae_amd.tokenizer.LLFQVAE_V4.revive_dead_codes_",
                                     "lipvq_vae_amd.ema.EMACodebook.reset_codes_"), _ema_prepare),
    "train_eval_toggle": Writer(_toggle, "none", "params", ("torch.nn.Module.train", "torch.nn.Module.eval")),
    "blind_add_then_invalidate": Writer(_blind_then_invalidate, "inplace", "params",
                                        ("lipvq_vae_amd.tokenizer.LLFQVAE_V4.invalidate_caches",
                                         "lipvq_vae_amd.embedding.ICLInputEmbedding.invalidate_caches",
                                         "lipvq_vae_amd.binning.AdaptiveBinActionEmbedding.invalidate_caches")),
}


# ---------------------------------------------------------------------------------------------------------------------------
# consumers
# ---------------------------------------------------------------------------------------------------------------------------

class Consumer(NamedTuple):
    fn: Callable | None       # (rig, data) -> tuple of tensors; None: the consumer has a test of its own (expect != "value")
    part: str                 # the part that owns the cache: "tok" | "emb" | "bin" | "net" | "policy" (emb + net + codebook)
    expect: str               # "value": equals the twin | "raise": RuntimeError after a write | "replay": a captured graph
    subjects: tuple           # the subjects it runs on
    route: tuple | None = None           # (entry, batch key, mode, {tokenizer class: route}): asserted through _plan
    cache: str = ""           # the derived state it reads through (for INTEGRATION.md's table and the reader)


def _tokenize(key, mode=None):
    def fn(rig, data):
        kw = {} if mode is None else {"mode": mode}
        return rig.tok.tokenize(data[key], count_usage=False, **kw)
    return fn


def _forward(key):
    def fn(rig, data):
        with torch.no_grad():
            return rig.tok(data[key])
    return fn


def _unfused(key):
    def fn(rig, data):
        return rig.tok._quantize(rig.tok.encode(data[key]), None)
    return fn


def _decode(rig, data):
    tok = rig.tok
    if hasattr(tok, "decode"):
        return (tok.decode(data["codes"]),)
    # the plain VQVAE has no decode(): the same launch on its packed decoder, which is the cache this consumer is about
    from lipvq_vae_amd import ops
    return (ops.mlp3(tok._codebook().detach(), tok._packed_decoder(), tok._DEC_ACTS, gather_idx=data["codes"]),)


def _code_table(rig, data):
    with torch.no_grad():
        return (rig.emb.code_table(rig.tok._codebook()),)


def _emb_forward(rig, data):
    with torch.no_grad():
        return (rig.emb(data["obs"], data["ctx_obs"], action_indices=data["aidx"], codebook=rig.tok._codebook()),)


def _prompt_embedding(rig, data):
    with torch.no_grad():
        return (rig.emb.prompt_embedding(data["ctx_obs"], action_indices=data["aidx"], codebook=rig.tok._codebook()),)


def _bin_forward(rig, data):
    with torch.no_grad():
        return (rig.bin(data["actions"]),)


_TOKS, _ALL_TOKS = ("llfq", "vq"), ("llfq", "vq", "icrt")
_F, _R, _S, _AP = "fused", "rows", "screened", "all_pairs"

CONSUMERS = {
    "tokenize_big": Consumer(_tokenize("x_big"), "tok", "value", _TOKS, ("tokenize", "x_big", "parity", {"LLFQVAE_V4": _F, "VQVAE": _F}),
                             "packed encoder, prepared codebook, _tok_ws"),
    "tokenize_small": Consumer(_tokenize("x_small"), "tok", "value", _ALL_TOKS,
                               ("tokenize", "x_small", "parity", {"LLFQVAE_V4": _F, "VQVAE": _AP}), "packed encoder, prepared codebook"),
    "tokenize_fast_big": Consumer(_tokenize("x_big", "fast"), "tok", "value", ("llfq",),
                                  ("tokenize", "x_big", "fast", {"LLFQVAE_V4": _F}), "fp16 pack of the fast mode"),
    "tokenize_fast_small": Consumer(_tokenize("x_small", "fast"), "tok", "value", ("llfq",),
                                    ("tokenize", "x_small", "fast", {"LLFQVAE_V4": _F}), "fp16 pack of the fast mode"),
    "decode": Consumer(_decode, "tok", "value", _ALL_TOKS, None, "packed decoder"),
    "forward_big": Consumer(_forward("x_big"), "tok", "value", _TOKS, ("forward", "x_big", "parity", {"LLFQVAE_V4": _F, "VQVAE": _F}),
                            "packed encoder and decoder, prepared codebook"),
    "forward_small": Consumer(_forward("x_small"), "tok", "value", _ALL_TOKS,
                              ("forward", "x_small", "parity", {"LLFQVAE_V4": _R, "VQVAE": _AP}), "packed encoder and decoder"),
    "unfused_big": Consumer(_unfused("x_big"), "tok", "value", _TOKS, ("quantize", "x_big", "parity", {"LLFQVAE_V4": _S, "VQVAE": _AP}),
                            "packed encoder, prepared codebook (stand-alone screen)"),
    "unfused_small": Consumer(_unfused("x_small"), "tok", "value", _ALL_TOKS,
                              ("quantize", "x_small", "parity", {"LLFQVAE_V4": _R, "VQVAE": _AP}), "packed encoder"),
    "code_table": Consumer(_code_table, "emb", "value", _ALL_TOKS, None, "ICLInputEmbedding._table_cache"),
    "embedding_forward": Consumer(_emb_forward, "emb", "value", _ALL_TOKS, None, "ICLInputEmbedding._table_cache"),
    "prompt_embedding": Consumer(_prompt_embedding, "emb", "value", _ALL_TOKS, None, "ICLInputEmbedding._table_cache"),
    "bin_forward": Consumer(_bin_forward, "bin", "value", ("bin",), None, "AdaptiveBinActionEmbedding._table_cache"),
    "forward_cached": Consumer(None, "net", "raise", ("policy",), None, "gpt.PromptCache"),
    "policy_features": Consumer(None, "policy", "raise", ("policy",), None, "the prompt icl.PromptedPolicy keeps"),
    "tokenizer_backward": Consumer(None, "tok", "raise", ("llfq", "vq", "icrt"), None, "autograd._TokenizerFn's saved parameter versions"),
    "graphed_gpt_replay": Consumer(None, "net", "replay", ("policy",), None, "GraphedGPTBackbone's captured graph"),
    "graphed_eval_replay": Consumer(None, "policy", "replay", ("policy",), None, "GraphedEval's captured graph"),
}


class DensePolicy(nn.Module):
    """forward(obs) = net(emb(obs, ctx_obs, ctx_act)) on dense context actions: a module with no derived caches, which is what
    GraphedEval's contract covers."""

    def __init__(self, rig, ctx_obs, ctx_act):
        super().__init__()
        self.rig, self.ctx_obs, self.ctx_act = rig, ctx_obs, ctx_act
        self.train(False)

    def forward(self, obs):
        return self.rig.net(self.rig.emb(obs, self.ctx_obs, self.ctx_act))


# ---------------------------------------------------------------------------------------------------------------------------
# which pairs are tested
# ---------------------------------------------------------------------------------------------------------------------------

NOT_PAIRED = {
    "no codebook": "codebook maintenance writes a tokenizer's codebook: the bin tokenizer and the backbone have none",
    "backbone not written": "codebook maintenance and the tokenizer's graphed step write no backbone or embedding parameter, and "
                            "GraphedGPTBackbone / GraphedEval(DensePolicy) read no codebook",
    "policy step writes no tokenizer": "GraphedPolicyStep here owns the embedding's and the backbone's parameters: the tokenizer's "
                                       "packs, the bin table and the tokenizer's backward see no write",
    "captured shape": "GraphedTokenizerStep is captured at the ICRT shape (N = 80, D = 208): no big batch, no fast mode, no bin "
                      "tokenizer, no backbone (PromptedPolicy sees a codebook write through the optimizers on the tokenizer)",
    "one capture per test": "GraphedPolicyStep's writes are optim.Adam's in-place writes, which fused_adam pairs with both replays; "
                            "a second capture beside the step's own is what keeps a test at a few seconds",
    "replaces the tensor": "a captured graph reads parameters by address: writers that replace a tensor (or write a copy) are "
                           "outside the contract of GraphedEval / GraphedGPTBackbone, which asks for a new capture",
    "nothing to refuse": "no parameter of the original moved (train()/eval() toggles, a written deep copy), so its backward has "
                         "nothing to refuse and reads the weights its forward read: what every training test already runs",
    "replaced codebook object": "load_state_dict(assign=True) on the TOKENIZER puts a new Parameter in the module; the policy "
                                "holds the tensor set_prompt was given, which did not move (on the embedding and the backbone, "
                                "whose modules the policy holds, the pair is tested): documented in INTEGRATION.md",
    "blind by design": "p.data.add_() moves no version counter and no address: PromptCache, PromptedPolicy, the backward check "
                       "and they alone cannot be told by invalidate_caches(); documented in INTEGRATION.md (prefill / "
                       "set_prompt / forward again)",
}


# One pair is tested on two of its three written parts only: (writer, consumer, part) -> key of NOT_PAIRED
PART_NOT_PAIRED = {("load_state_dict_assign", "policy_features", "tok"): "replaced codebook object"}


def pairing(wname, cname):
    """("tested", subjects) or ("not_paired", key of NOT_PAIRED) for one (writer, consumer) pair."""
    w, c = WRITERS[wname], CONSUMERS[cname]
    if w.scope == "codebook":
        if c.part == "bin":
            return "not_paired", "no codebook"
        if c.part == "net" or c.expect == "replay":
            return "not_paired", "backbone not written"
    elif w.scope == "tok_step":
        if c.part == "net" or c.expect == "replay":
            return "not_paired", "backbone not written"
        if "icrt" not in c.subjects:
            return "not_paired", "captured shape"
        return "tested", ("icrt",)
    elif w.scope == "policy_step":
        if c.part in ("tok", "bin"):
            return "not_paired", "policy step writes no tokenizer"
        if c.expect == "replay":
            return "not_paired", "one capture per test"
        return "tested", ("policy",)
    else:
        if c.expect == "replay" and w.kind != "inplace":
            return "not_paired", "replaces the tensor"
        if cname == "tokenizer_backward" and w.kind in ("none", "copy"):
            return "not_paired", "nothing to refuse"
        if wname == "blind_add_then_invalidate" and c.expect == "raise":
            return "not_paired", "blind by design"
    return "tested", tuple(s for s in c.subjects if s != "icrt")      # (icrt is the captured shape's subject alone)


def tested(expect=None, scope=None):
    """[(writer, consumer, subjects)] of every tested pair, optionally of one consumer kind / writer scope."""
    out = []
    for wn, w in WRITERS.items():
        for cn, c in CONSUMERS.items():
            what, arg = pairing(wn, cn)
            if what == "tested" and (expect is None or c.expect == expect) and (scope is None or w.scope == scope):
                out.append((wn, cn, arg))
    return out


def value_consumers(wname, subject):
    return [cn for wn, cn, subjects in tested("value") if wn == wname and subject in subjects]


def resolve(dotted):
    """The object a dotted name of Writer.api stands for."""
    parts = dotted.split(".")
    for i in range(len(parts), 0, -1):
        try:
            obj = importlib.import_module(".".join(parts[:i]))
        except ImportError:
            continue
        for p in parts[i:]:
            obj = getattr(obj, p)
        return obj
    raise ImportError(dotted)
