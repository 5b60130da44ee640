"""CPU: the host side of the deterministic policy's output head (lipvq-vae_amd/action_head.py) -- module tree, seeded bytes,
checkpoint loading, the constructor's and the library's limits -- and the restatement tests/action_head_ref.py: its cosine term
against formulas written out by hand and, where the reference tree is present, against the reference's own ``cosine_loss``.
No kernel runs here; the kernels and the whole module are covered on the GPU in tests/test_gpu_action_head.py."""
import importlib.util
import inspect
import os
from pathlib import Path

import pytest
import torch
import torch.nn as nn

import action_head_ref
import lipvq_vae_amd  # noqa: F401
from lipvq_vae_amd.action_head import LOSS_KEYS, ActionHead

# the reference tree, where oracle/gen_golden.py looks for it (--ref); absent on most hosts
REFERENCE = Path(os.environ.get("LIPVQ_REFERENCE", "/root/reference"))
LOSS_UTILS = REFERENCE / "robomimic" / "utils" / "loss_utils.py"


def test_exported_from_the_package():
    assert lipvq_vae_amd.ActionHead is ActionHead and "ActionHead" in lipvq_vae_amd.__all__
    assert LOSS_KEYS == action_head_ref.LOSS_KEYS


def test_state_dict_keys_order_and_shapes():
    E, A = 64, 7
    sd = ActionHead(E, A).state_dict()
    assert tuple(sd) == action_head_ref.KEYS                                        # keys AND order
    assert [tuple(v.shape) for v in sd.values()] == [(A, E), (A,)]
    assert all(v.dtype == torch.float32 for v in sd.values())


def test_seeded_parameters_are_one_linear():
    E, A = 32, 12
    torch.manual_seed(3)
    head = ActionHead(E, A)
    after_head = torch.rand(1)
    torch.manual_seed(3)
    lin = nn.Linear(E, A)
    after_lin = torch.rand(1)
    assert torch.equal(head.nets["action"].weight, lin.weight) and torch.equal(head.nets["action"].bias, lin.bias)
    assert torch.equal(after_head, after_lin)                                       # the same RNG consumption


def test_checkpoint_subdict_loads_strict():
    src = ActionHead(64, 7)
    ckpt = {"policy.nets.decoder." + k: v.clone() + 1.0 for k, v in src.state_dict().items()}      # as algo.serialize() names them
    sub = {k[len("policy.nets.decoder."):]: v for k, v in ckpt.items()}
    dst = ActionHead(64, 7)
    res = dst.load_state_dict(sub, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(dst.nets["action"].bias, src.nets["action"].bias + 1.0)


def test_signatures():
    sig = inspect.signature(ActionHead.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("embed_dim", inspect.Parameter.empty), ("ac_dim", inspect.Parameter.empty)]
    sig = inspect.signature(ActionHead.losses)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[3:]] == [
        ("l2_weight", 1.0), ("l1_weight", 0.0), ("cos_weight", 0.0)]               # icl_config.py:43-45
    assert (1.0, 0.0, 0.0) == action_head_ref.DEFAULT_WEIGHTS


def test_unsupported_configurations_raise():
    with pytest.raises(ValueError, match="ac_dim"):
        ActionHead(64, 0)
    with pytest.raises(ValueError, match="ac_dim"):
        ActionHead(64, 65)
    with pytest.raises(ValueError, match="embed_dim"):
        ActionHead(1028, 7)
    with pytest.raises(ValueError, match="embed_dim"):
        ActionHead(510, 7)
    ActionHead(1024, 64)                                                            # the largest tested shape is legal
    ActionHead(4, 1)


def test_cpu_input_raises():
    head = ActionHead(64, 7)
    feats, target = torch.zeros(2, 3, 64), torch.zeros(2, 3, 7)
    for call in (lambda: head(feats), lambda: head.losses(feats, target)):
        with pytest.raises(RuntimeError, match="HIP library only"):
            call()
    from lipvq_vae_amd import ops
    with pytest.raises(RuntimeError, match="HIP library only"):
        ops.action_head(feats, head.nets["action"].weight, head.nets["action"].bias)


def test_library_limits_are_reported_without_a_gpu():
    """Argument checks come before any launch, so they can be exercised with null pointers on a host without a GPU."""
    from lipvq_vae_amd import _capi
    lib = _capi.lib

    def head(N, T, E, A, bstride=0):
        return lib.lipvq_action_head_f32(None, bstride, *([None] * 7), N, T, E, A, 1.0, 0.0, 0.0, None)

    def bwd(N, A):
        return lib.lipvq_action_head_bwd_f32(None, None, None, None, None, N, A, 1.0, 0.0, 0.0, None)

    assert head(80, 10, 512, 0) == -2 and b"64" in lib.lipvq_last_error()                            # ac_dim
    assert head(80, 10, 512, 65) == -2 and b"64" in lib.lipvq_last_error()
    assert head(80, 10, 1028, 12) == -2 and b"1024" in lib.lipvq_last_error()                        # E
    assert head(80, 10, 510, 12) == -2 and b"multiple of 4" in lib.lipvq_last_error()
    assert head(80, 10, 512, 12, bstride=15362) == -1 and b"stride" in lib.lipvq_last_error()        # unaligned batch stride
    assert head(-1, 10, 512, 12) == -1 and head(80, 0, 512, 12) == -1                                # not sizes
    assert head(80, 10, 512, 12) == -1 and b"null" in lib.lipvq_last_error()                         # limits pass, then the pointers
    assert head(80, 10, 512, 64) == -1 and b"null" in lib.lipvq_last_error()
    assert head(0, 10, 512, 12) == 0                                                                 # zero rows: no-op
    assert head(0, 10, 512, 65) == -2                                                                # ... after the limits
    assert bwd(80, 0) == -2 and bwd(80, 65) == -2
    assert bwd(80, 12) == -1 and b"null" in lib.lipvq_last_error()
    assert bwd(0, 12) == 0
    assert lib.lipvq_action_head_workspace_bytes(80) == 3 * 12 and lib.lipvq_action_head_workspace_bytes(4097) == 129 * 12
    assert lib.lipvq_action_head_workspace_bytes(0) == 0                                             # three floats per 32 rows


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------

def _cos_rows():
    """[rows, 3] predictions and labels: random rows, a zero label, a zero prediction, and p = t = (1e-5, 0, 0)."""
    g = torch.Generator().manual_seed(4)
    p, t = torch.randn(16, 3, generator=g).double(), torch.randn(16, 3, generator=g).double()
    t[3] = 0.0
    p[5] = 0.0
    p[7] = t[7] = torch.tensor([1e-5, 0.0, 0.0], dtype=torch.float64)
    return p, t


def test_cosine_term_clamps_each_norm_on_its_own():
    """The installed torch's nn.CosineSimilarity: sim = sum (p / max(|p|, 1e-8)) (t / max(|t|, 1e-8)).  p = t = (1e-5, 0, 0) gives
    1.0; clamping the PRODUCT of the norms at 1e-8 would give 1e-10 / 1e-8 = 0.01."""
    p, t = _cos_rows()
    for dtype in (torch.float64, torch.float32):
        pd, td = p.to(dtype), t.to(dtype)
        sim = nn.CosineSimilarity(dim=1)(pd, td)
        want = ((pd / pd.norm(dim=1, keepdim=True).clamp_min(1e-8)) * (td / td.norm(dim=1, keepdim=True).clamp_min(1e-8))).sum(1)
        assert float((sim - want).abs().max()) <= (1e-12 if dtype == torch.float64 else 1e-6)
        assert float(sim[7]) == 1.0 and float(sim[3]) == 0.0 and float(sim[5]) == 0.0
        got = action_head_ref.cosine_loss(pd, td)
        assert abs(float(got) - float((1.0 - want).mean())) <= (1e-12 if dtype == torch.float64 else 1e-6)


def test_losses_are_the_written_out_formulas():
    g = torch.Generator().manual_seed(6)
    torch.manual_seed(6)
    sd = {k: v.double() for k, v in ActionHead(64, 7).state_dict().items()}
    feats = torch.randn(5, 9, 64, generator=g).double() * 2.0
    target = torch.rand(5, 9, 7, generator=g).double() * 6.0 - 3.0                 # both SmoothL1 branches
    w = (0.5, 2.0, 0.25)
    out = action_head_ref.head_losses(sd, feats, target, w)
    assert tuple(out) == action_head_ref.LOSS_KEYS
    y = torch.tanh(feats @ sd["nets.action.weight"].t() + sd["nets.action.bias"])
    d = y - target
    assert float((d.abs() > 1).double().mean()) > 0.1 and float((d.abs() < 1).double().mean()) > 0.1
    l2 = (d ** 2).mean()
    l1 = torch.where(d.abs() < 1, 0.5 * d ** 2, d.abs() - 0.5).mean()
    p3, t3 = y[..., :3], target[..., :3]
    sim = ((p3 / p3.norm(dim=-1, keepdim=True).clamp_min(1e-8)) * (t3 / t3.norm(dim=-1, keepdim=True).clamp_min(1e-8))).sum(-1)
    cos = 1.0 - sim.mean()
    for k, want in zip(action_head_ref.LOSS_KEYS, (l2, l1, cos, w[0] * l2 + w[1] * l1 + w[2] * cos)):
        assert abs(float(out[k]) - float(want)) <= 1e-12 * max(1.0, abs(float(want))), k
    # the last-step form: supervise_all_steps = False is the caller's slice
    last = action_head_ref.head_losses(sd, feats[:, -1:], target[:, -1][:, None], w)
    assert abs(float(last["l2_loss"]) - float((d[:, -1] ** 2).mean())) <= 1e-12


@pytest.mark.skipif(not LOSS_UTILS.exists(), reason="the reference tree is not on this host")
def test_cosine_term_is_the_reference_cosine_loss():
    """robomimic/utils/loss_utils.py needs torch and numpy only: imported by file path, nothing of it is copied."""
    spec = importlib.util.spec_from_file_location("reference_loss_utils", LOSS_UTILS)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p, t = _cos_rows()
    for dtype in (torch.float64, torch.float32):
        for rows in (slice(None), slice(3, 4), slice(7, 8)):                        # all rows; the zero label; (1e-5, 0, 0)
            pd, td = p[rows].to(dtype), t[rows].to(dtype)
            assert torch.equal(action_head_ref.cosine_loss(pd, td), mod.cosine_loss(pd, td))
            pb, tb = pd.view(1, -1, 3), td.view(1, -1, 3)                           # the [B, T, 3] form of icl.py:193
            assert torch.equal(action_head_ref.cosine_loss(pb, tb), mod.cosine_loss(pb, tb))
    assert float(mod.cosine_loss(p[7:8], t[7:8])) == 0.0 and float(mod.cosine_loss(p[3:4], t[3:4])) == 1.0
