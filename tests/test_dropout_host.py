"""CPU: the in-kernel dropout contract (include/lipvq.h, "in-kernel dropout") without a GPU.  The generator against the Random123
known answers, the library's host function (the very header the kernels compile) against the numpy restatement in
tests/dropout_ref.py byte for byte, the refusals, and what set_dropout_source must leave alone in GPTBackbone."""
import math

import numpy as np
import pytest
import torch

import dropout_ref as R

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

SEEDS = (20240607, 2 ** 63 + 12345)
STEPS = (0, 2 ** 32 - 1)
SITES = (0, 9)
FIELDS = ((1, 1), (3, 5), (7, 33), (2, 1024))
PS = (1e-9, 0.1, 0.5, 0.999)


def _ops():
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd import ops
    return ops


def test_known_answers():
    for counter, key, want in KNOWN:
        got = R.philox4x32_10(counter, key)
        assert tuple(int(w) for w in got) == want, (counter, key, [hex(int(w)) for w in got])


@pytest.mark.parametrize("rows,cols", FIELDS)
def test_host_function_against_numpy(rows, cols):
    ops = _ops()
    for p in PS:
        for seed in SEEDS:
            for step in STEPS:
                for site in SITES:
                    got = ops.dropout_keep_host(seed, step, site, rows, cols, p).numpy()
                    want = R.keep_field(seed, step, site, rows, cols, p)
                    assert got.shape == (rows, cols) and got.dtype == np.uint8
                    assert np.array_equal(got, want), (rows, cols, p, seed, step, site)


def test_the_known_answers_reach_the_host_function():
    """The host function's words ARE the generator's: with thr = floor(p 2^32) just below / just above a known output word, the
    decision of that column flips.  counter (col >> 2, row, site, step) = 0, key = seed = 0: the first known answer."""
    ops = _ops()
    words = KNOWN[0][2]
    for col, w in enumerate(words):
        below, above = w / 4294967296.0, (w + 1) / 4294967296.0          # thr = w: kept (word >= thr); thr = w + 1: dropped
        assert math.floor(below * 4294967296.0) == w and math.floor(above * 4294967296.0) == w + 1
        assert int(ops.dropout_keep_host(0, 0, 0, 1, 4, below)[0, col]) == 1
        assert int(ops.dropout_keep_host(0, 0, 0, 1, 4, above)[0, col]) == 0


def test_step_enters_with_its_low_32_bits():
    ops = _ops()
    a = ops.dropout_keep_host(5, 7, 2, 16, 64, 0.5)
    assert torch.equal(a, ops.dropout_keep_host(5, 7 + 2 ** 32, 2, 16, 64, 0.5))
    assert not torch.equal(a, ops.dropout_keep_host(5, 8, 2, 16, 64, 0.5))


def test_fields_differ_when_one_input_differs():
    ops = _ops()
    base = dict(seed=11, step=3, site=4)
    f0 = ops.dropout_keep_host(base["seed"], base["step"], base["site"], 16, 64, 0.5)
    for key, other in (("seed", 12), ("seed", 11 + 2 ** 32), ("step", 4), ("site", 5)):
        args = dict(base, **{key: other})
        f1 = ops.dropout_keep_host(args["seed"], args["step"], args["site"], 16, 64, 0.5)
        differ = float((f0 != f1).float().mean())
        print(f"{key} {base[key]} -> {other}: {differ:.3f} of the decisions differ")
        assert 0.4 < differ < 0.6, (key, differ)          # independent fair bits: 1024 decisions, 0.5 +- 5 sigma = 0.42 .. 0.58


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_fraction(p):
    """2^20 decisions of one field: |kept / n - (1 - p)| <= 5 sqrt(p (1 - p) / n), the binomial bound.  Deterministic: one seed."""
    ops = _ops()
    n = 1 << 20
    kept = float(ops.dropout_keep_host(20240607, 0, 1, 1024, 1024, p).sum()) / n
    bound = 5.0 * math.sqrt(p * (1.0 - p) / n)
    print(f"p={p}: kept {kept:.6f}, expected {1 - p:.6f}, |diff| {abs(kept - (1 - p)):.2e}, bound {bound:.2e}")
    assert abs(kept - (1.0 - p)) <= bound


def test_refusals_make_no_gpu_call():
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd import _capi
    ops = _ops()
    EINVAL, EUNSUPPORTED = -1, -2
    host = _capi.lib.lipvq_dropout_keep_host
    for p in (0.0, -0.1, 1.0, 1.5, float("nan")):
        assert host(1, 0, 0, 4, 4, p, None) == EINVAL, p
        with pytest.raises(_capi.LipvqLibraryError, match="status -1"):
            ops.dropout_keep_host(1, 0, 0, 4, 4, p)
    assert host(1, 0, 0, 2 ** 32, 4, 0.5, None) == EUNSUPPORTED
    assert host(1, 0, 0, 2 ** 32 - 1, 0, 0.5, None) == 0                   # (an empty field of the largest row count: nothing to write)
    with pytest.raises(_capi.LipvqLibraryError, match="status -2"):
        ops.dropout_keep_host(1, 0, 0, 2 ** 32, 4, 0.5)
    # the device entry points check p and the row count before they touch a pointer or launch anything
    lib = _capi.lib
    assert lib.lipvq_dropout_keep_u8(None, 0, 4, 4, 1.0, None, None) == EINVAL
    assert lib.lipvq_dropout_keep_u8(None, 0, 2 ** 32, 4, 0.5, None, None) == EUNSUPPORTED
    assert lib.lipvq_gpt_attention_drop_f32(None, None, None, None, 0, 0.0, 2, 30, 64, 4, 1, None) == EINVAL
    assert lib.lipvq_gpt_attention_drop_f32(None, None, None, None, 0, 0.5, 2 ** 25, 128, 64, 1, 1, None) == EUNSUPPORTED      # B H L = 2^32
    assert lib.lipvq_gpt_attention_bwd_drop_f32(None, None, None, None, None, None, None, 0, 1.0, 2, 30, 64, 4, 1, None) == EINVAL
    assert lib.lipvq_gpt_layernorm_drop_f32(None, None, None, None, 1e-5, None, 0, 1.0, None, None, None, None, 4, 64, None) == EINVAL
    assert lib.lipvq_gpt_layernorm_drop_f32(None, None, None, None, 1e-5, None, 0, 0.5, None, None, None, None, 2 ** 32, 64, None) == EUNSUPPORTED
    assert lib.lipvq_gpt_layernorm_bwd_drop_f32(None, None, None, None, None, None, 0, 0.0, None, None, None, None, None, 4, 64, None) == EINVAL


def _backbone():
    from lipvq_vae_amd.gpt import GPTBackbone
    torch.manual_seed(1234)
    return GPTBackbone(64, 12, num_layers=2, num_heads=4, attn_dropout=0.1, block_output_dropout=0.1)


def test_seeded_construction_and_state_dict_are_unchanged():
    import lipvq_vae_amd  # noqa: F401
    plain = _backbone()
    after_plain = torch.rand(4)
    net = _backbone()
    assert net.dropout_source == "torch" and net.dropout_state is None
    keys = list(net.state_dict().keys())
    assert net.set_dropout_source("kernel") is net and net.dropout_source == "kernel"
    after_kernel = torch.rand(4)
    assert torch.equal(after_plain, after_kernel), "set_dropout_source consumed torch's RNG"
    assert list(net.state_dict().keys()) == keys and keys == list(plain.state_dict().keys())
    for (k, a), (_, b) in zip(plain.state_dict().items(), net.state_dict().items()):
        assert torch.equal(a, b), k
    plain.load_state_dict(net.state_dict(), strict=True)
    state = net.dropout_state
    assert state.dtype == torch.int64 and state.shape == (2,) and state.tolist() == [torch.initial_seed(), 0]
    assert "_dropout_state" in dict(net.named_buffers())                  # a buffer (so .to() moves it), a non-persistent one
    # a seed above 2^63 is kept as its bit pattern; reseeding writes in place; "torch" keeps the state for a later return
    net.reseed_dropout(2 ** 63 + 5, step=9)
    assert net.dropout_state is state and state.tolist() == [2 ** 63 + 5 - 2 ** 64, 9]
    assert net.set_dropout_source("torch").dropout_source == "torch" and net.dropout_state is state
    net.set_dropout_source("kernel", seed=77)
    assert state.tolist() == [77, 0]
    with pytest.raises(ValueError):
        net.set_dropout_source("philox")
    with pytest.raises(RuntimeError):
        _backbone().reseed_dropout(1)
