"""CPU: the in-kernel dropout source outside the backbone (include/lipvq.h, "in-kernel dropout for the embedding stage and the
default action branch") without a GPU: the site constants, that a site of its own gives a field of its own, what
set_dropout_source must leave alone in ICLInputEmbedding and DefaultActionNetwork, and that the new entry points refuse a bad p
or row count before they touch a pointer."""
import copy
import math
import warnings

import pytest
import torch


def _ops():
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd import ops
    return ops


def _embedding():
    from lipvq_vae_amd.embedding import ICLInputEmbedding
    torch.manual_seed(4321)
    return ICLInputEmbedding(9, embed_dim=64, context_length=5, emb_dropout=0.1)


def _default():
    from lipvq_vae_amd.default_branch import DefaultActionNetwork
    torch.manual_seed(4321)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DefaultActionNetwork(7, 64, num_layers=2)


MODULES = {"embedding": _embedding, "default": _default}


def test_site_constants_are_exported():
    ops = _ops()
    assert ops.DROPOUT_SITE_EMBED == 0x40000000 and ops.DROPOUT_SITE_DEFAULT == 0x80000000
    # the backbone's sites are 4 layer + {0, 1, 2}: no depth reaches the embedding's word, and the default branch's four per
    # layer start above it
    assert 4 * 10 ** 6 + 2 < ops.DROPOUT_SITE_EMBED < ops.DROPOUT_SITE_DEFAULT
    assert ops.DROPOUT_SITE_DEFAULT + 4 * 10 ** 6 + 3 < 2 ** 32


def test_the_embed_site_draws_a_field_of_its_own():
    """Same (seed, step), the embedding's site against the backbone's 4 * 0 + 1 on a [30, 512] field: the fields differ like
    independent ones, and the kept fraction stays within test_dropout_host.py::test_kept_fraction's binomial bound."""
    ops = _ops()
    seed, step, p, rows, cols = 20240607, 3, 0.1, 30, 512
    emb = ops.dropout_keep_host(seed, step, ops.DROPOUT_SITE_EMBED, rows, cols, p)
    gpt = ops.dropout_keep_host(seed, step, 4 * 0 + 1, rows, cols, p)
    n = rows * cols
    differ = float((emb != gpt).float().mean())
    # two independent fields of keep probability 0.9 differ at 2 * 0.9 * 0.1 = 0.18 of the positions: +- 5 sigma
    sigma = math.sqrt(0.18 * 0.82 / n)
    print(f"embed vs backbone site: {differ:.4f} of {n} decisions differ (0.18 +- {5 * sigma:.4f})")
    assert not torch.equal(emb, gpt) and abs(differ - 0.18) <= 5 * sigma
    bound = 5.0 * math.sqrt(p * (1.0 - p) / n)
    for name, f in (("embed", emb), ("backbone", gpt)):
        kept = float(f.sum()) / n
        print(f"{name}: kept {kept:.6f}, expected {1 - p:.6f}, bound {bound:.2e}")
        assert abs(kept - (1.0 - p)) <= bound, name
    # and the default branch's four sites of a layer are four fields
    fields = [ops.dropout_keep_host(seed, step, ops.DROPOUT_SITE_DEFAULT + k, rows, cols, p) for k in range(4)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert not torch.equal(fields[i], fields[j]), (i, j)


@pytest.mark.parametrize("which", sorted(MODULES))
def test_set_dropout_source_leaves_construction_and_state_dict_alone(which):
    make = MODULES[which]
    plain = make()
    after_plain = torch.rand(4)
    net = make()
    assert net.dropout_source == "torch" and net.dropout_state is None
    assert "_dropout_state" not in dict(net.named_buffers()), "the state must not exist before the first 'kernel' call"
    keys = list(net.state_dict().keys())
    with pytest.raises(ValueError, match=type(net).__name__):
        net.set_dropout_source("philox")
    assert net.dropout_state is None
    assert net.set_dropout_source("torch") is net and net.dropout_state is None          # "torch" creates nothing either
    assert net.set_dropout_source("kernel") is net and net.dropout_source == "kernel"
    after_kernel = torch.rand(4)
    assert torch.equal(after_plain, after_kernel), "set_dropout_source consumed torch's RNG"
    assert list(net.state_dict().keys()) == keys and keys == list(plain.state_dict().keys())
    for (k, a), (_, b) in zip(plain.state_dict().items(), net.state_dict().items()):
        assert torch.equal(a, b), k
    plain.load_state_dict(net.state_dict(), strict=True)
    state = net.dropout_state
    assert state.dtype == torch.int64 and state.shape == (2,) and state.tolist() == [torch.initial_seed(), 0]
    assert "_dropout_state" in dict(net.named_buffers())
    net.reseed_dropout(2 ** 63 + 5, step=9)
    assert net.dropout_state is state and state.tolist() == [2 ** 63 + 5 - 2 ** 64, 9]
    assert net.set_dropout_source("torch").dropout_source == "torch" and net.dropout_state is state
    net.set_dropout_source("kernel", seed=77)
    assert state.tolist() == [77, 0]
    net.set_dropout_source("kernel")                                                       # no seed: the state is left alone
    assert state.tolist() == [77, 0]


@pytest.mark.parametrize("which", sorted(MODULES))
def test_reseed_before_the_kernel_source_raises(which):
    net = MODULES[which]()
    with pytest.raises(RuntimeError, match=f"{type(net).__name__}.reseed_dropout"):
        net.reseed_dropout(1)


@pytest.mark.parametrize("which", sorted(MODULES))
def test_deepcopy_has_its_own_state(which):
    net = MODULES[which]().set_dropout_source("kernel", seed=31)
    net.reseed_dropout(31, step=4)
    twin = copy.deepcopy(net)
    assert twin.dropout_source == "kernel"
    assert twin.dropout_state is not net.dropout_state and twin.dropout_state.data_ptr() != net.dropout_state.data_ptr()
    assert torch.equal(twin.dropout_state, net.dropout_state)
    twin.reseed_dropout(32)
    assert net.dropout_state.tolist() == [31, 4] and twin.dropout_state.tolist() == [32, 0]


def test_the_backbone_keeps_its_messages():
    """GPTBackbone now takes the holder from the shared mixin: same types, same texts."""
    from lipvq_vae_amd.gpt import GPTBackbone
    torch.manual_seed(1)
    net = GPTBackbone(64, 12, num_layers=1, num_heads=4)
    with pytest.raises(ValueError, match=r"^GPTBackbone: dropout source must be 'torch' or 'kernel', got 'philox'$"):
        net.set_dropout_source("philox")
    with pytest.raises(RuntimeError, match=r"^GPTBackbone\.reseed_dropout: call set_dropout_source\('kernel'\) first \(it creates the state\)$"):
        net.reseed_dropout(1)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_linear_fn_refuses_dropout_on_the_bf16_pipes(precision):
    """The in-kernel dropout source has fp32 Linear kernels only: LinearFn says so before it touches a tensor (CPU tensors here,
    which every kernel wrapper would refuse with another error type)."""
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.nnfn import LinearFn
    from lipvq_vae_amd.ops import ACT_NONE
    x, W, snap = torch.zeros(3, 8), torch.zeros(16, 8, requires_grad=True), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="LinearFn: dropout"):
        LinearFn.apply(x, W, None, ACT_NONE, precision, (snap, 0x80000003, 0.1))


def test_new_entry_points_refuse_before_they_touch_anything():
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd import _capi
    lib, EINVAL, EUNSUPPORTED = _capi.lib, -1, -2
    site = 0x80000000
    for p in (0.0, 1.0):
        assert lib.lipvq_attention_drop_f32(None, None, None, None, site, p, 17, 64, 8, None) == EINVAL
        assert lib.lipvq_attention_bwd_drop_f32(None, None, None, None, None, None, None, site, p, 17, 64, 8, None) == EINVAL
        assert lib.lipvq_linear_act_drop_f32(None, None, None, None, None, None, site, p, 33, 12, 100, 0, None) == EINVAL
        assert lib.lipvq_act_bwd_drop_f32(None, None, None, None, site, p, 33, 100, 0, None) == EINVAL
        assert lib.lipvq_embed_rows_drop_f32(None, None, None, None, None, 1e-5, None, None, None, site, p, 15, 5, 64, 15, 320, 64, 0,
                                             None) == EINVAL
        assert lib.lipvq_embed_rows_bwd_drop_f32(None, None, None, None, None, None, None, None, None, None, None, site, p, 15, 5, 64,
                                                 15, 320, 64, 0, None) == EINVAL
        assert lib.lipvq_embed_rows_bwd_ws_drop_f32(None, None, None, None, None, None, None, None, None, None, None, None, site, p,
                                                    15, 5, 64, 15, 320, 64, 0, None) == EINVAL
    # rows >= 2^32
    assert lib.lipvq_linear_act_drop_f32(None, None, None, None, None, None, site, 0.5, 2 ** 32, 12, 100, 0, None) == EUNSUPPORTED
    assert lib.lipvq_act_bwd_drop_f32(None, None, None, None, site, 0.5, 2 ** 32, 100, 0, None) == EUNSUPPORTED
    # H S = 4097 * 1 048 560 rows of attention decisions
    assert lib.lipvq_attention_drop_f32(None, None, None, None, site, 0.5, 1048560, 4097, 4097, None) == EUNSUPPORTED
    assert lib.lipvq_attention_bwd_drop_f32(None, None, None, None, None, None, None, site, 0.5, 1048560, 4097, 4097, None) == EUNSUPPORTED
    # the last output row of an embed_rows call: batch 2^27 of [32][E] blocks ends at row 2^32 - 32 + 4 (fits), 2^27 + 1 does not
    E, T, S = 64, 5, 32
    for B, want in ((2 ** 27, EINVAL), (2 ** 27 + 1, EUNSUPPORTED)):          # (a row count that fits goes on to the null-pointer check)
        got = lib.lipvq_embed_rows_drop_f32(None, None, None, None, None, 1e-5, None, None, None, site, 0.5, B * T, T, E, B * T, S * E,
                                            E, 0, None)
        assert got == want, (B, got)
    # the field row is the output slot's: slots that are not whole rows of E floats are refused
    assert lib.lipvq_embed_rows_drop_f32(None, None, None, None, None, 1e-5, None, None, None, site, 0.5, 15, 5, 64, 15, 320, 64, 4,
                                         None) == EINVAL
