"""CPU: the host side of the output heads' matmul precision (ActionHead / GMMActionHead.set_matmul_precision, icl.PromptedPolicy.
set_matmul_precision): the setters' default, validation and absence from state_dict(), the new symbols in include/lipvq.h, the
library and _capi, the ops wrappers' keyword, and the library's argument checks, which come before any launch and so run with
null pointers on a host without a GPU.  The kernels are covered in tests/test_gpu_head_precision.py."""
import inspect
import re
from pathlib import Path

import pytest
import torch

import lipvq_vae_amd
from lipvq_vae_amd import _capi, ops
from lipvq_vae_amd.action_head import ActionHead
from lipvq_vae_amd.gmm import GMMActionHead

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("lipvq_action_head_mp_f32", "lipvq_gmm_head_mp_f32", "lipvq_gmm_sample_mp_f32", "lipvq_gmm_sample_draw_mp_f32")
EINVAL, EUNSUPPORTED = -1, -2


def _heads(E=64):
    return ActionHead(E, 7), GMMActionHead(E, 7, num_modes=3)


def test_default_is_fp32_and_the_setter_returns_the_module():
    for head in _heads():
        assert head.matmul_precision == "fp32"
        for p in ("bf16", "bf16x3", "fp32"):
            assert head.set_matmul_precision(p) is head and head.matmul_precision == p


def test_unknown_names_are_refused_and_change_nothing():
    for head in _heads():
        head.set_matmul_precision("bf16")
        for bad in ("fp16", "BF16", "", None, 1):
            with pytest.raises(ValueError, match="matmul precision"):
                head.set_matmul_precision(bad)
        assert head.matmul_precision == "bf16"


def test_bf16_modes_need_an_embed_dim_that_is_a_multiple_of_8():
    for head in _heads(E=36):
        for p in ("bf16", "bf16x3"):
            with pytest.raises(ValueError, match="multiple of 8"):
                head.set_matmul_precision(p)
        assert head.matmul_precision == "fp32"
        head.set_matmul_precision("fp32")
    for head in _heads(E=8):
        head.set_matmul_precision("bf16x3")


def test_not_part_of_state_dict():
    for head in _heads():
        keys = tuple(head.state_dict())
        head.set_matmul_precision("bf16")
        assert tuple(head.state_dict()) == keys and not any("precision" in k for k in keys)
        assert not any("precision" in n for n, _ in head.named_buffers())
        fresh = type(head)(64, 7) if isinstance(head, ActionHead) else GMMActionHead(64, 7, num_modes=3)
        fresh.load_state_dict(head.state_dict(), strict=True)
        assert fresh.matmul_precision == "fp32"                                     # loading a checkpoint sets no mode


def test_symbols_in_header_library_and_capi():
    header = (ROOT / "include" / "lipvq.h").read_text()
    assert re.search(r"enum\s*\{\s*LIPVQ_MATMUL_FP32\s*=\s*0\s*,\s*LIPVQ_MATMUL_BF16\s*=\s*1\s*,\s*LIPVQ_MATMUL_BF16X3\s*=\s*2\s*\}", header)
    assert "#define LIPVQ_ABI_VERSION 1" in header                                  # an additive change
    for name in ENTRY_POINTS:
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, name
        assert re.search(r"int matmul,\s*void\* stream$", decl.group(1)), name      # the trailing argument before the stream
        base = re.search(r"\bint " + name.replace("_mp_f32", "_f32") + r"\(([^;]*)\);", header).group(1)
        squeeze = lambda s: " ".join(s.split())                                      # noqa: E731
        assert squeeze(decl.group(1)) == squeeze(base).replace("void* stream", "int matmul, void* stream"), name
        assert name in _capi.SIGNATURES
        fn = getattr(_capi.lib, name)                                               # AttributeError: not in the .so
        assert fn.argtypes is not None and len(fn.argtypes) == len(getattr(_capi.lib, name.replace("_mp_f32", "_f32")).argtypes) + 1
    assert ops.MATMUL_PRECISIONS == {"fp32": 0, "bf16": 1, "bf16x3": 2}


def test_ops_wrappers_take_the_keyword():
    for fn in (ops.action_head, ops.gmm_head, ops.gmm_sample, ops.gmm_sample_draw, ops.head_linear_grads):
        assert inspect.signature(fn).parameters["precision"].default == "fp32", fn.__name__
    feats = torch.zeros(2, 3, 64)
    head = ActionHead(64, 7)
    with pytest.raises(RuntimeError, match="HIP library only"):                     # the CPU refusal is still the first one
        ops.action_head(feats, head.nets["action"].weight, head.nets["action"].bias, precision="bf16")


def test_library_checks_the_mode_before_any_pointer():
    lib = _capi.lib

    def ah(E, matmul, N=80):
        return lib.lipvq_action_head_mp_f32(None, 0, *([None] * 7), N, 10, E, 12, 1.0, 0.0, 0.0, matmul, None)

    def gh(E, matmul, N=80):
        return lib.lipvq_gmm_head_mp_f32(None, 0, *([None] * 14), N, 10, E, 5, 12, 0, 0.01, matmul, None)

    def gs(E, matmul, N=80):
        return lib.lipvq_gmm_sample_mp_f32(None, 0, *([None] * 9), N, 10, E, 5, 12, 0, 0.01, matmul, None)

    def gd(E, matmul, N=80):
        return lib.lipvq_gmm_sample_draw_mp_f32(None, 0, *([None] * 9), N, 10, E, 5, 12, 0, 0.01, matmul, None)

    for call in (ah, gh, gs, gd):
        for m in (0, 1, 2):
            assert call(512, m) == EINVAL and b"null" in lib.lipvq_last_error()     # sizes and mode pass, then the pointers
            assert call(512, m, N=0) == 0                                           # zero rows: no-op
        assert call(516, 0) == EINVAL and b"null" in lib.lipvq_last_error()         # fp32 keeps its E % 4 rule
        for m in (1, 2):
            assert call(516, m) == EUNSUPPORTED and b"multiple of 8" in lib.lipvq_last_error()
            assert call(516, m, N=0) == EUNSUPPORTED                                # ... also before the no-op
        for m in (-1, 3, 99):
            assert call(512, m) == EINVAL and b"matmul" in lib.lipvq_last_error()
        assert call(1028, 1) == EUNSUPPORTED and b"1024" in lib.lipvq_last_error()  # the head's own limits come first


def test_prompted_policy_sets_both_and_drops_the_prompt():
    from lipvq_vae_amd.gpt import GPTBackbone
    from lipvq_vae_amd.icl import PromptedPolicy
    net, head = GPTBackbone(64, 12, num_layers=1, num_heads=4), ActionHead(64, 7)
    policy = PromptedPolicy(object(), net, head)
    policy.cache = "a prompt"
    assert policy.set_matmul_precision("bf16") is policy
    assert net.matmul_precision == "bf16" and head.matmul_precision == "bf16" and policy.cache is None
    with pytest.raises(RuntimeError, match=r"call set_prompt\(\) first"):           # the error a missing prompt gives
        policy.features(torch.zeros(1, 4, 8))
    policy.cache = "a prompt"
    with pytest.raises(ValueError, match="matmul precision"):
        policy.set_matmul_precision("fp8")
    assert net.matmul_precision == "bf16" and head.matmul_precision == "bf16" and policy.cache == "a prompt"
    with pytest.raises(TypeError, match="no matmul precision"):
        PromptedPolicy(object(), net, lambda f: f).set_matmul_precision("bf16")
    assert lipvq_vae_amd.ActionHead is ActionHead
