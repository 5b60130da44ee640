"""CPU: the host side of the transformer backbone (lipvq-vae_amd/gpt.py) against the fixtures the reference's GPT_Backbone
produced (tests/golden/gpt_*.npz, scripts/gen_golden_gpt.py) -- no kernel runs here; the kernels and the whole module are
covered on the GPU in tests/test_gpu_gpt.py.

The restatement tests/gpt_ref.py issues the reference's own torch ops in the reference's order, so its fp32 output and input
gradient are compared with ``torch.equal``.  That holds on one thread (the fixtures were written on one thread; a threaded
fp32 GEMM may split its sums differently), so these tests pin torch to one thread while they run.  Given one thread,
``torch.equal`` is used for every stored fp32 array -- output, input gradient and parameter gradients; there is no fp32 array
it cannot be used for.  Only the float64 column is compared with a tolerance (1e-12)."""
import numpy as np
import pytest
import torch

import gpt_ref
import lipvq_vae_amd  # noqa: F401
from lipvq_vae_amd.gpt import GPTBackbone, GraphedGPTBackbone  # noqa: F401

CASES = ("gpt_icrt", "gpt_small", "gpt_noncausal", "gpt_len3")


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _load(golden_dir, name):
    g = np.load(golden_dir / f"{name}.npz", allow_pickle=False)
    cfg = {k: int(g[k]) for k in ("seed", "B", "L", "E", "H", "layers", "causal")}
    return g, cfg


def _build(cfg, **kw):
    torch.manual_seed(cfg["seed"])
    return GPTBackbone(embed_dim=cfg["E"], context_length=cfg["L"], causal=bool(cfg["causal"]), attn_dropout=0.0,
                       block_output_dropout=0.0, num_layers=cfg["layers"], num_heads=cfg["H"], **kw)


@pytest.mark.parametrize("name", CASES)
def test_state_dict_matches_the_reference(golden_dir, name):
    g, cfg = _load(golden_dir, name)
    sd = _build(cfg).state_dict()
    assert list(sd) == [str(k) for k in g["keys"]]                                   # keys AND order
    for k, shp in zip(sd, g["shapes"]):
        assert tuple(sd[k].shape) == tuple(int(s) for s in shp if s >= 0), k
    assert all(v.dtype == torch.float32 for v in sd.values())


@pytest.mark.parametrize("name", CASES)
def test_seeded_parameters_are_the_reference_bytes(golden_dir, name):
    g, cfg = _load(golden_dir, name)
    assert gpt_ref.state_hash(_build(cfg).state_dict()) == str(g["params_sha256"])


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_fixture(golden_dir, name):
    g, cfg = _load(golden_dir, name)
    net = _build(cfg)
    params = dict(net.named_parameters())
    sd = {k: params.get(k, v) for k, v in net.state_dict().items()}                  # parameters as leaves, buffers as they are
    x = torch.from_numpy(g["x"]).requires_grad_(True)
    out = gpt_ref.gpt_forward(sd, x, cfg["layers"], cfg["H"])
    (out * gpt_ref.objective_weights(cfg["seed"], out.shape)).sum().backward()
    assert torch.equal(out.detach(), torch.from_numpy(g["out32"]))
    assert torch.equal(x.grad, torch.from_numpy(g["gx32"]))
    for n in gpt_ref.STORED_PARAM_GRADS:
        n = n.format(last=cfg["layers"] - 1)
        assert torch.equal(params[n].grad, torch.from_numpy(g["gp32/" + n])), n
    for n, rows in gpt_ref.STORED_WEIGHT_ROWS:
        assert torch.equal(params[n].grad[:rows], torch.from_numpy(g[f"gp32/{n}[:{rows}]"])), n
    # and the fixture's own float64 columns are this restatement in float64 (what test_gpu_gpt.py measures against)
    sd64 = {k: v.detach().double() for k, v in sd.items()}
    out64 = gpt_ref.gpt_forward(sd64, torch.from_numpy(g["x"]).double(), cfg["layers"], cfg["H"])
    assert float((out64 - torch.from_numpy(g["out64"])).abs().max()) <= 1e-12 * float(np.abs(g["out64"]).max())
    assert 0.0 < float(g["dev/out"]) < 1e-5 and 0.0 < float(g["dev/gx"]) < 1e-5


def test_constructor_defaults_are_the_reference_signature():
    import inspect
    sig = inspect.signature(GPTBackbone.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("embed_dim", inspect.Parameter.empty), ("context_length", inspect.Parameter.empty), ("causal", True),
        ("attn_dropout", 0.1), ("block_output_dropout", 0.1), ("num_layers", 6), ("num_heads", 8), ("activation", "gelu")]


def test_checkpoint_subdict_loads_strict(golden_dir):
    g, cfg = _load(golden_dir, "gpt_small")
    src = _build(cfg)
    ckpt = {"policy.nets.transformer." + k: v.clone() + 1.0 for k, v in src.state_dict().items()}      # as algo.serialize() names them
    sub = {k[len("policy.nets.transformer."):]: v for k, v in ckpt.items()}
    dst = GPTBackbone(cfg["E"], cfg["L"], num_layers=cfg["layers"], num_heads=cfg["H"])
    res = dst.load_state_dict(sub, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(dst.nets["output_ln"].weight, src.nets["output_ln"].weight + 1.0)


def test_geglu_raises():
    with pytest.raises(NotImplementedError, match="geglu"):
        GPTBackbone(64, 12, num_layers=1, num_heads=4, activation="geglu")


def test_unsupported_shapes_raise_at_construction():
    with pytest.raises(ValueError):
        GPTBackbone(64, 12, num_layers=1, num_heads=8)            # head width 8
    with pytest.raises(ValueError):
        GPTBackbone(64, 129, num_layers=1, num_heads=4)           # context beyond the attention kernel's 128


def test_cpu_input_raises():
    net = GPTBackbone(64, 12, num_layers=1, num_heads=4)
    with pytest.raises(RuntimeError, match="HIP library only"):
        net(torch.zeros(2, 12, 64))
    with pytest.raises(AssertionError):
        net(torch.zeros(2, 11, 64))                               # transformers.py:437


def test_library_limits_are_reported_without_a_gpu():
    """Argument checks come before any launch, so they can be exercised with null pointers on a host without a GPU."""
    from lipvq_vae_amd import _capi
    lib = _capi.lib
    assert lib.lipvq_gpt_attention_f32(None, None, None, None, 1.0, 2, 129, 512, 8, 1, None) == -2          # L > 128
    assert b"128" in lib.lipvq_last_error()
    assert lib.lipvq_gpt_attention_f32(None, None, None, None, 1.0, 2, 30, 64, 8, 1, None) == -2            # head width 8
    assert lib.lipvq_gpt_attention_f32(None, None, None, None, 1.0, 0, 30, 512, 8, 1, None) == 0            # B = 0: no-op
    assert lib.lipvq_gpt_attention_bwd_f32(None, None, None, None, None, None, None, 1.0, 4, 0, 512, 8, 1, None) == 0
    assert lib.lipvq_gpt_layernorm_f32(None, None, None, None, 1e-5, None, None, None, None, 4, 1028, None) == -2
    assert lib.lipvq_gpt_layernorm_f32(None, None, None, None, 1e-5, None, None, None, None, 4, 6, None) == -2
    assert lib.lipvq_gpt_layernorm_f32(None, None, None, None, 1e-5, None, None, None, None, 0, 512, None) == 0
    assert lib.lipvq_gpt_layernorm_bwd_workspace_bytes(240, 512) == 60 * 2 * 512 * 4                         # 4 rows per workgroup
    assert lib.lipvq_gpt_layernorm_bwd_workspace_bytes(70000, 1024) == 500 * 2 * 1024 * 4                    # 140 rows per workgroup
