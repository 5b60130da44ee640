"""CPU: the host side of the prompt cache (GPTBackbone.prefill / forward_cached, lipvq_gpt_attention_prefix_f32) -- the argument
checks that come before any launch, with null pointers and CPU tensors.  The kernel and the modules run in
tests/test_gpu_gpt_prompt.py."""
import pytest
import torch

import lipvq_vae_amd  # noqa: F401
from lipvq_vae_amd import _capi
from lipvq_vae_amd.gpt import GPTBackbone, PromptCache, PromptedGPTBackbone

EINVAL, EUNSUPPORTED = -1, -2


def _call(B, Bp, P, Lq, E, H):
    return _capi.lib.lipvq_gpt_attention_prefix_f32(None, None, None, B, Bp, P, Lq, E, H, None)


def test_library_limits_are_reported_without_a_gpu():
    assert _capi.lib.lipvq_gpt_attention_f32(None, None, None, None, 1.0, 2, 30, 64, 8, 1, None) == EUNSUPPORTED    # (the codes)
    assert _capi.lib.lipvq_gpt_attention_f32(None, None, None, None, 1.0, -1, 30, 512, 8, 1, None) == EINVAL
    assert _call(2, 2, 100, 29, 512, 8) == EUNSUPPORTED and b"128" in _capi.lib.lipvq_last_error()            # P + Lq = 129
    assert _call(2, 2, 129, 0, 512, 8) == EUNSUPPORTED
    assert _call(2, 2, 2**31 - 1, 2**31 - 1, 512, 8) == EUNSUPPORTED                                         # no overflow in P + Lq
    assert _call(2, 2, 20, 10, 64, 8) == EUNSUPPORTED and b"head width" in _capi.lib.lipvq_last_error()       # head width 8
    assert _call(3, 2, 20, 10, 512, 8) == EINVAL and b"Bp" in _capi.lib.lipvq_last_error()                    # Bp is neither B nor 1
    assert _call(2, 2, -1, 10, 512, 8) == EINVAL and _call(2, 2, 20, -1, 512, 8) == EINVAL
    assert _call(2, 2, 20, 10, 510, 8) == EINVAL                                                              # E % H != 0
    assert _call(0, 0, 20, 10, 512, 8) == 0 and _call(0, 1, 20, 10, 512, 8) == 0                             # B = 0: no-op
    assert _call(4, 4, 20, 0, 512, 8) == 0 and _call(4, 1, 128, 0, 512, 8) == 0                              # Lq = 0: no-op
    assert _call(4, 4, 20, 10, 512, 8) == EINVAL and b"null" in _capi.lib.lipvq_last_error()                  # past the checks


def test_cache_paths_refuse_training_mode_and_noncausal_backbones():
    net = GPTBackbone(64, 12, num_layers=2, num_heads=4)
    cache = PromptCache((), 1, 4, "fp32", ())
    with pytest.raises(RuntimeError, match="eval"):
        net.prefill(torch.zeros(1, 4, 64))
    with pytest.raises(RuntimeError, match="eval"):
        net.forward_cached(torch.zeros(1, 4, 64), cache)
    assert PromptedGPTBackbone(net, cache).training and not PromptedGPTBackbone(net.eval(), cache).training
    with pytest.raises(RuntimeError, match="HIP library only"):
        net.prefill(torch.zeros(1, 4, 64))
    with pytest.raises(ValueError, match="context_length"):
        net.prefill(torch.zeros(1, 13, 64))
    with pytest.raises(ValueError):
        net.prefill(torch.zeros(1, 4, 32))
    loose = GPTBackbone(64, 12, causal=False, num_layers=2, num_heads=4).eval()
    with pytest.raises(ValueError, match="non-causal"):
        loose.prefill(torch.zeros(1, 4, 64))
    with pytest.raises(ValueError, match="non-causal"):
        loose.forward_cached(torch.zeros(1, 4, 64), cache)


def test_prompt_embedding_validates_like_forward():
    from lipvq_vae_amd.embedding import ICLInputEmbedding
    emb = ICLInputEmbedding(8, 64, 3)
    ctx = torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match="exactly one"):
        emb.prompt_embedding(ctx)
    with pytest.raises(ValueError, match="exactly one"):
        emb.prompt_embedding(ctx, ctx, action_indices=torch.zeros(2, 3, dtype=torch.int64), codebook=torch.zeros(4, 8))
    with pytest.raises(ValueError, match="codebook"):
        emb.prompt_embedding(ctx, action_indices=torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="same shape"):
        emb.prompt_embedding(ctx, torch.zeros(2, 2, 8))
