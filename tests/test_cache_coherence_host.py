"""CPU: the contract of the version-keyed caches, and the tables of tests/cache_coherence_cases.py.

``_PackCache`` (tokenizer.py; reused by ICLInputEmbedding._table_cache and the bin tokenizer's) rebuilds exactly after the writes
it can see -- listed in REBUILDS -- never without a write, and not after ``p.data.add_()``, the documented blind spot that
``invalidate_caches()`` exists for.  The keys of ``gpt.PromptCache``, ``icl.PromptedPolicy`` and the tokenizer's backward check are
pure host code and are held to the same list.  The package is imported as tests/test_tokenizer_routes_host.py imports it; the one
launcher a consumer here would call (``ops.linear``) is replaced with a counting CPU stand-in.
"""
import copy

import pytest
import torch
import torch.nn as nn

import cache_coherence_cases as C


def _package():
    import lipvq_vae_amd
    import lipvq_vae_amd.tokenizer  # noqa: F401
    return lipvq_vae_amd


class _Holder(nn.Module):
    """One Linear and a table derived from its weight through a _PackCache with a counting build."""

    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(4, 3)
        self.cache = _package().tokenizer._PackCache()
        self.builds = 0

    def table(self):
        def build():
            self.builds += 1
            return self.lin.weight.detach() * 2.0
        return self.cache.get((self.lin.weight,), build)


def _other(m):
    return {k: v.detach() * 1.5 + 1.0 for k, v in m.state_dict().items()}


def _in_place(m):
    with torch.no_grad():
        m.lin.weight.mul_(1.5)
        return m


def _copy_(m):
    with torch.no_grad():
        m.lin.weight.copy_(m.lin.weight * 0.5 + 1.0)
    return m


def _load(m):
    m.load_state_dict(_other(m))
    return m


def _assign(m):
    m.load_state_dict(_other(m), assign=True)
    return m


def _data(m):
    m.lin.weight.data = m.lin.weight.detach() * 1.5 + 1.0
    return m


def _increment(m):
    m.lin.weight.data.add_(1.0)                                       # a raw-pointer writer ...
    torch.autograd.graph.increment_version(m.lin.weight)              # ... that tells torch, as optim.py and ema.py do
    return m


def _optimizer(m):
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    return m


def _deepcopy(m):
    other = copy.deepcopy(m)
    other.builds = 0
    with torch.no_grad():
        other.lin.weight.mul_(1.5)
    return other


# every visible writer of the table that can run on the CPU: the set that must rebuild is exactly this
REBUILDS = {"in-place op under no_grad": _in_place, "copy_ under no_grad": _copy_, "load_state_dict": _load,
            "load_state_dict(assign=True)": _assign, ".data = new": _data, "increment_version": _increment,
            "optimizer step": _optimizer, "deepcopy": _deepcopy}


@pytest.mark.parametrize("name", sorted(REBUILDS))
def test_pack_cache_rebuilds_after_a_visible_write(name):
    m = _Holder()
    first = m.table().clone()
    assert m.builds == 1
    assert m.table() is m.table() and m.builds == 1                   # no rebuild without a write
    written = REBUILDS[name](m)
    got = written.table()
    assert written.builds == 1 + (written is m), name
    assert torch.equal(got, written.lin.weight.detach() * 2.0) and not torch.equal(got, first)
    written.table()
    assert written.builds == 1 + (written is m)
    if written is not m:                                              # the original did not move and kept its pack
        assert torch.equal(m.table(), first) and m.builds == 1


def test_pack_cache_without_a_write_and_after_a_blind_one():
    m = _Holder()
    first = m.table()
    m.train()
    m.eval()
    m.lin.weight.requires_grad_(False).requires_grad_(True)
    m.lin.weight.grad = torch.ones_like(m.lin.weight)
    assert m.table() is first and m.builds == 1
    m.lin.weight.data.add_(1.0)                                       # the documented blind spot: no version, no address moves
    assert m.table() is first and m.builds == 1
    m.cache.invalidate()                                              # ... which is what invalidate_caches() is for
    assert torch.equal(m.table(), m.lin.weight.detach() * 2.0) and m.builds == 2


@pytest.fixture
def counted_linear():
    """ops.linear as a CPU stand-in that counts its calls (the real one launches a kernel)."""
    ops = _package().ops
    real, calls = ops.linear, []

    def linear(x, W, b=None, act=0, save_pre=False):
        calls.append(tuple(x.shape))
        y = x @ W.t()
        return y if b is None else y + b

    ops.linear = linear
    yield calls
    ops.linear = real


@pytest.mark.parametrize("name,target", [(n, t) for n in sorted(REBUILDS) for t in ("codebook", "embedding")
                                         if (n, t) != ("deepcopy", "embedding")])      # (a copied embedding: the test below)
def test_code_table_follows_the_writers(counted_linear, name, target):
    """ICLInputEmbedding.code_table under no_grad: the [K, E] table follows a visible write to the codebook OR to the Linear."""
    from lipvq_vae_amd.embedding import ICLInputEmbedding
    emb = ICLInputEmbedding(4, embed_dim=8, context_length=2).eval()
    book, mine = _Holder(), _Holder()                                 # book.lin.weight [3, 4] plays the codebook
    mine.lin = emb.nets["embed_encoder"]                              # ... and the writers reach the embedding's Linear through `mine`
    with torch.no_grad():
        first = emb.code_table(book.lin.weight).clone()
        assert emb.code_table(book.lin.weight) is emb.code_table(book.lin.weight) and len(counted_linear) == 1
        if target == "codebook":
            book = REBUILDS[name](book)
        else:
            REBUILDS[name](mine)
        lin = emb.nets["embed_encoder"]
        table = emb.code_table(book.lin.weight)
        assert torch.equal(table, book.lin.weight.detach() @ lin.weight.t() + lin.bias) and not torch.equal(table, first)
        assert len(counted_linear) == 2
        assert emb.code_table(book.lin.weight) is table and len(counted_linear) == 2
        book.lin.weight.data.add_(1.0)                                # blind: the stale table is served until invalidate_caches()
        assert emb.code_table(book.lin.weight) is table
        emb.invalidate_caches()
        assert torch.equal(emb.code_table(book.lin.weight), book.lin.weight.detach() @ lin.weight.t() + lin.bias)
        assert len(counted_linear) == 3


def test_a_copied_embedding_builds_its_own_table(counted_linear):
    from lipvq_vae_amd.embedding import ICLInputEmbedding
    emb = ICLInputEmbedding(4, embed_dim=8, context_length=2).eval()
    book = torch.randn(3, 4)
    with torch.no_grad():
        first = emb.code_table(book)
        other = copy.deepcopy(emb)
        other.nets["embed_encoder"].weight.mul_(1.5)
        lin = other.nets["embed_encoder"]
        assert torch.equal(other.code_table(book), book @ lin.weight.t() + lin.bias) and len(counted_linear) == 2
        assert emb.code_table(book) is first and len(counted_linear) == 2


def _backbone():
    from lipvq_vae_amd.gpt import GPTBackbone
    return GPTBackbone(32, 6, num_layers=1, num_heads=2)


def test_prompt_cache_key_sees_what_versions_alone_do_not():
    a, b = _backbone(), _backbone()
    for net in (a, b):
        net.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    assert [p._version for p in a.parameters()] == [p._version for p in b.parameters()]
    assert a._param_versions() != b._param_versions()                 # two backbones loaded once each
    key, versions = a._param_versions(), [p._version for p in a.parameters()]
    w = a.nets["output_ln"].weight
    w.data = w.detach() * 2.0                                         # keeps _version
    assert [p._version for p in a.parameters()] == versions and a._param_versions() != key
    key = a._param_versions()
    a.train()
    a.eval()
    assert a._param_versions() == key
    with torch.no_grad():
        w.mul_(2.0)
    assert a._param_versions() != key


def test_prompted_policy_key_covers_the_embedding_and_the_codebook():
    from lipvq_vae_amd.embedding import ICLInputEmbedding
    from lipvq_vae_amd.icl import PromptedPolicy
    emb = ICLInputEmbedding(4, embed_dim=32, context_length=2).eval()
    book = nn.Parameter(torch.randn(5, 4))
    policy = PromptedPolicy(emb, _backbone().eval(), lambda f: f)
    policy._codebook = book
    key = policy._embedded_key()
    assert len(key) == len(list(emb.parameters())) + 1 and policy._embedded_key() == key
    for t in (*emb.parameters(), book):
        with torch.no_grad():
            t.mul_(1.5)
        assert policy._embedded_key() != key
        key = policy._embedded_key()
        t.data = t.detach().clone()
        assert policy._embedded_key() != key
        key = policy._embedded_key()
    policy._codebook = None
    assert len(policy._embedded_key()) == len(key) - 1


def test_backward_check_sees_a_replaced_parameter():
    from lipvq_vae_amd.autograd import _check_versions

    class Ctx:
        pass
    p = nn.Parameter(torch.randn(3))
    ctx = Ctx()
    ctx.param_versions = ((p.data_ptr(), p._version),)
    _check_versions(ctx, (p,))
    p.data = p.detach().clone()                                       # keeps _version
    with pytest.raises(RuntimeError, match="modified in place"):
        _check_versions(ctx, (p,))
    ctx.param_versions = ((p.data_ptr(), p._version),)
    with torch.no_grad():
        p.add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        _check_versions(ctx, (p,))


def test_a_warm_tokenizer_deep_copies_without_the_originals_caches():
    """The screen monitor's pending reading holds an event (not copyable) and the packs are keyed on the original's addresses."""
    tok = _package().tokenizer
    m = tok.LLFQVAE_V4(7, 64, num_codes=256)
    m._enc_cache.get(m._enc_params(), lambda: "pack of the original")
    m._screen_monitor._pending = (object(), None, 1, False)
    m._screen_monitor.bypass_calls = 3
    other = copy.deepcopy(m)
    assert other._enc_cache._key is None and other._enc_cache._val is None
    assert other._screen_monitor._pending is None and other._screen_monitor.bypass_calls == 0
    assert m._enc_cache._val == "pack of the original" and m._screen_monitor.bypass_calls == 3


# ---------------------------------------------------------------------------------------------------------------------------
# the helper tables
# ---------------------------------------------------------------------------------------------------------------------------

# the writers and consumers the tables must name
WRITER_NAMES = {"torch_adamw", "fused_adamw", "fused_adam", "graphed_tokenizer_step", "graphed_policy_step", "load_state_dict",
                "load_state_dict_assign", "cpu_write_cuda", "deepcopy_write", "no_grad_mul_", "no_grad_copy_", "data_assign",
                "ema_update", "init_codebook_", "revive_dead_codes_", "revive_dead_codes_ema", "train_eval_toggle",
                "blind_add_then_invalidate"}
CONSUMER_NAMES = {"tokenize_big", "tokenize_small", "tokenize_fast_big", "tokenize_fast_small", "decode", "forward_big",
                  "forward_small", "unfused_big", "unfused_small", "code_table", "embedding_forward", "prompt_embedding",
                  "bin_forward", "forward_cached", "policy_features", "tokenizer_backward", "graphed_gpt_replay",
                  "graphed_eval_replay"}


def test_every_named_writer_and_consumer_exists():
    _package()
    assert set(C.WRITERS) == WRITER_NAMES and set(C.CONSUMERS) == CONSUMER_NAMES
    for name, w in C.WRITERS.items():
        assert w.kind in ("inplace", "replace", "none", "copy") and w.scope in ("params", "codebook", "tok_step", "policy_step")
        assert w.api, name
        for dotted in w.api:
            assert C.resolve(dotted) is not None, (name, dotted)
        assert callable(w.fn) and (w.prepare is None or callable(w.prepare))
    for name, c in C.CONSUMERS.items():
        assert (c.fn is not None) == (c.expect == "value"), name
        assert c.expect in ("value", "raise", "replay") and c.cache and set(c.subjects) <= set(C.SUBJECTS)
        assert all(c.part in C.SUBJECTS[s] or c.part == "policy" for s in c.subjects), name


def test_every_pair_is_tested_or_listed_with_a_reason():
    used = set()
    for wn in C.WRITERS:
        for cn in C.CONSUMERS:
            what, arg = C.pairing(wn, cn)
            assert what in ("tested", "not_paired"), (wn, cn)
            if what == "tested":
                assert arg and set(arg) <= set(C.CONSUMERS[cn].subjects) | {"policy"}, (wn, cn)
            else:
                assert arg in C.NOT_PAIRED, (wn, cn, arg)
                used.add(arg)
    for (wn, cn, part), reason in C.PART_NOT_PAIRED.items():
        assert C.pairing(wn, cn)[0] == "tested" and part in C.SUBJECTS["policy"] and reason in C.NOT_PAIRED
        used.add(reason)
    assert used == set(C.NOT_PAIRED), "a reason nobody gives"
    assert len(C.NOT_PAIRED) <= 10 and all(r and "\n" not in r for r in C.NOT_PAIRED.values())
    pairs = {(wn, cn) for wn, cn, _ in C.tested()}
    assert {wn for wn, _ in pairs} == set(C.WRITERS) and {cn for _, cn in pairs} == set(C.CONSUMERS)
    # what the three defects found by reading need
    for pair in (("graphed_tokenizer_step", "code_table"), ("graphed_tokenizer_step", "tokenizer_backward"),
                 ("fused_adamw", "policy_features"), ("data_assign", "forward_cached"), ("deepcopy_write", "forward_cached")):
        assert pair in pairs, pair


def test_the_gpu_file_runs_every_tested_pair():
    import test_gpu_cache_coherence as G
    ran = set()
    for subject, wn in G._matrix():
        ran |= {(wn, cn, subject) for cn in C.value_consumers(wn, subject)}
    ran |= {("graphed_tokenizer_step", cn, "icrt") for cn in C.value_consumers("graphed_tokenizer_step", "icrt")}
    ran.add(("graphed_tokenizer_step", "tokenizer_backward", "icrt"))
    ran |= {("graphed_policy_step", cn, "policy") for cn in C.value_consumers("graphed_policy_step", "policy")}
    ran |= {("graphed_policy_step", cn, "policy") for cn in ("forward_cached", "policy_features")}
    ran |= {(wn, "forward_cached", "policy") for wn in G._refusing("forward_cached")}
    ran |= {(wn, "policy_features", "policy") for wn, _ in G._policy_cases()}
    ran |= {(wn, "tokenizer_backward", s) for wn in G._refusing("tokenizer_backward", "llfq") for s in ("llfq", "vq")}
    ran |= {(wn, cn, "policy") for cn in ("graphed_gpt_replay", "graphed_eval_replay") for wn in G._replayed(cn)}
    want = {(wn, cn, s) for wn, cn, subjects in C.tested() for s in subjects}
    assert ran == want, (sorted(want - ran), sorted(ran - want))
