"""CPU: the host side of the GMM output head (lipvq-vae_amd/gmm.py) -- module tree, seeded bytes, checkpoint loading, the
constructor's and the library's limits -- and the float64 restatement tests/gmm_ref.py against formulas written out by hand.
No kernel runs here; the kernels and the whole module are covered on the GPU in tests/test_gpu_gmm.py."""
import inspect
import math

import pytest
import torch
import torch.nn as nn

import gmm_ref
import lipvq_vae_amd  # noqa: F401
from lipvq_vae_amd.gmm import GMMActionHead


def test_state_dict_keys_order_and_shapes():
    E, A, M = 64, 7, 5
    sd = GMMActionHead(E, A, num_modes=M).state_dict()
    assert tuple(sd) == gmm_ref.KEYS                                               # keys AND order
    assert [tuple(v.shape) for v in sd.values()] == [(M * A, E), (M * A,), (M * A, E), (M * A,), (M, E), (M,)]
    assert all(v.dtype == torch.float32 for v in sd.values())


def test_seeded_parameters_are_three_linears_in_order():
    E, A, M = 32, 12, 5
    torch.manual_seed(3)
    head = GMMActionHead(E, A, num_modes=M)
    after_head = torch.rand(1)
    torch.manual_seed(3)
    lins = [nn.Linear(E, M * A), nn.Linear(E, M * A), nn.Linear(E, M)]             # ObservationDecoder._create_layers' order
    after_lins = torch.rand(1)
    for name, lin in zip(("mean", "scale", "logits"), lins):
        assert torch.equal(head.nets[name].weight, lin.weight) and torch.equal(head.nets[name].bias, lin.bias), name
    assert torch.equal(after_head, after_lins)                                     # the same RNG consumption


def test_checkpoint_subdict_loads_strict():
    src = GMMActionHead(64, 7)
    ckpt = {"policy.nets.decoder." + k: v.clone() + 1.0 for k, v in src.state_dict().items()}      # as algo.serialize() names them
    sub = {k[len("policy.nets.decoder."):]: v for k, v in ckpt.items()}
    dst = GMMActionHead(64, 7)
    res = dst.load_state_dict(sub, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(dst.nets["logits"].bias, src.nets["logits"].bias + 1.0)


def test_constructor_defaults():
    sig = inspect.signature(GMMActionHead.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("embed_dim", inspect.Parameter.empty), ("ac_dim", inspect.Parameter.empty), ("num_modes", 5), ("min_std", 0.01),
        ("std_activation", "softplus"), ("low_noise_eval", True), ("use_tanh", False)]


def test_unsupported_configurations_raise():
    with pytest.raises(NotImplementedError, match="use_tanh"):
        GMMActionHead(64, 7, use_tanh=True)
    with pytest.raises(ValueError, match="std_activation"):
        GMMActionHead(64, 7, std_activation="relu")
    with pytest.raises(ValueError):
        GMMActionHead(64, 7, num_modes=17)
    with pytest.raises(ValueError):
        GMMActionHead(64, 65, num_modes=1)
    with pytest.raises(ValueError, match="columns"):
        GMMActionHead(64, 20, num_modes=13)                                        # P = 13 * 41 = 533 > 512
    with pytest.raises(ValueError, match="embed_dim"):
        GMMActionHead(1028, 7)
    GMMActionHead(1024, 15, num_modes=16)                                          # P = 496: the largest tested shape is legal


def test_cpu_input_raises():
    head = GMMActionHead(64, 7)
    feats, actions = torch.zeros(2, 3, 64), torch.zeros(2, 3, 7)
    for call in (lambda: head(feats), lambda: head.log_prob(feats, actions), lambda: head.nll(feats, actions),
                 lambda: head.forward_train(feats)):
        with pytest.raises(RuntimeError, match="HIP library only"):
            call()


def test_library_limits_are_reported_without_a_gpu():
    """Argument checks come before any launch, so they can be exercised with null pointers on a host without a GPU."""
    from lipvq_vae_amd import _capi
    lib = _capi.lib

    def head(N, T, E, M, A, mode=0, bstride=0):
        return lib.lipvq_gmm_head_f32(None, bstride, *([None] * 14), N, T, E, M, A, mode, 0.01, None)

    def sample(N, T, E, M, A):
        return lib.lipvq_gmm_sample_f32(None, 0, *([None] * 9), N, T, E, M, A, 0, 0.01, None)

    assert head(80, 10, 512, 17, 12) == -2 and b"16" in lib.lipvq_last_error()                       # num_modes
    assert head(80, 10, 512, 0, 12) == -2
    assert head(80, 10, 512, 5, 65) == -2 and b"64" in lib.lipvq_last_error()                        # ac_dim
    assert head(80, 10, 512, 13, 20) == -2 and b"512" in lib.lipvq_last_error()                      # P = 533
    assert head(80, 10, 1028, 5, 12) == -2 and b"1024" in lib.lipvq_last_error()                     # E
    assert head(80, 10, 510, 5, 12) == -2 and b"multiple of 4" in lib.lipvq_last_error()
    assert head(80, 10, 512, 5, 12, mode=3) == -1                                                    # not a scale mode
    assert head(80, 10, 512, 5, 12, bstride=15362) == -1                                             # unaligned batch stride
    assert head(80, 10, 512, 5, 12) == -1 and b"null" in lib.lipvq_last_error()                      # limits pass, then the pointers
    assert head(0, 10, 512, 5, 12) == 0                                                              # zero rows: no-op
    assert sample(80, 10, 512, 17, 12) == -2 and sample(80, 10, 1028, 5, 12) == -2 and sample(0, 10, 512, 5, 12) == 0
    assert lib.lipvq_gmm_head_bwd_f32(None, None, None, None, None, 80, 17, 12, 0, 0.01, None) == -2
    assert lib.lipvq_gmm_head_bwd_f32(None, None, None, None, None, 80, 5, 65, 0, 0.01, None) == -2
    assert lib.lipvq_gmm_head_bwd_f32(None, None, None, None, None, 0, 5, 12, 0, 0.01, None) == 0
    assert lib.lipvq_gmm_params_bwd_f32(None, None, None, None, None, 80, 13, 20, 0, None) == -2
    assert lib.lipvq_gmm_params_bwd_f32(None, None, None, None, None, 0, 5, 12, 0, None) == 0
    assert lib.lipvq_gmm_workspace_bytes(80) == 3 * 4 and lib.lipvq_gmm_workspace_bytes(4097) == 129 * 4   # one float per 32 rows
    assert lib.lipvq_gmm_workspace_bytes(0) == 0


# ---------------------------------------------------------------------------------------------------
# the float64 restatement against formulas written out by hand
# ---------------------------------------------------------------------------------------------------

def _inputs(seed, N, E, M, A):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    sd = {k: v.double() for k, v in GMMActionHead(E, A, num_modes=M).state_dict().items()}
    feats = torch.randn(N, E, generator=g).double() * 2.0
    actions = (torch.rand(N, A, generator=g).double() * 3.0 - 1.5)
    gl = torch.randn(N, generator=g).double()
    return sd, feats, actions, gl


@pytest.mark.parametrize("std_activation", ["softplus", "exp"])
@pytest.mark.parametrize("M,A", [(1, 1), (5, 12), (16, 15)])
def test_restatement_log_prob_is_the_logsumexp_formula(M, A, std_activation):
    sd, feats, actions, _ = _inputs(11 + M, 37, 64, M, A)
    lp = gmm_ref.gmm_log_prob(sd, feats, actions, M, A, 0.01, std_activation)
    pm, ps, lg = gmm_ref.decoder(sd, feats, M, A)
    mu = torch.tanh(pm)
    sg = (torch.log1p(torch.exp(ps)) if std_activation == "softplus" else torch.exp(ps)) + 0.01
    want = torch.empty(37, dtype=torch.float64)
    for n in range(37):                                                            # scalar arithmetic, mode by mode
        logz = math.log(sum(math.exp(float(v)) for v in lg[n]))
        terms = []
        for m in range(M):
            ell = sum(-(float(actions[n, a]) - float(mu[n, m, a])) ** 2 / (2.0 * float(sg[n, m, a]) ** 2) - math.log(float(sg[n, m, a]))
                      - 0.5 * math.log(2.0 * math.pi) for a in range(A))
            terms.append(float(lg[n, m]) - logz + ell)
        top = max(terms)
        want[n] = top + math.log(sum(math.exp(t - top) for t in terms))
    err = float((lp - want).abs().max()) / float(want.abs().max())
    print(f"M={M} A={A} {std_activation}: restatement vs hand formula {err:.3e}")
    assert err <= 1e-12
    by_hand = gmm_ref.log_prob_by_hand(mu, sg, lg, actions)[0]
    assert float((by_hand - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("std_activation", ["softplus", "exp"])
@pytest.mark.parametrize("M,A", [(1, 1), (5, 12), (16, 15)])
def test_restatement_gradients_are_the_closed_forms(M, A, std_activation):
    sd, feats, actions, gl = _inputs(23 + M, 37, 64, M, A)
    pm, ps, lg = (t.detach().requires_grad_(True) for t in gmm_ref.decoder(sd, feats, M, A))
    if std_activation == "softplus":                                               # both sides of F.softplus's threshold
        with torch.no_grad():
            ps[0, 0, 0], ps[1, 0, 0], ps[2, 0, 0] = 19.5, 20.5, -30.0
    mu, sg = gmm_ref.activate(pm, ps, 0.01, std_activation)
    (gmm_ref.mixture(mu, sg, lg).log_prob(actions) * gl).sum().backward()
    want = gmm_ref.closed_form_grads(pm.detach(), ps.detach(), lg.detach(), actions, gl, 0.01, std_activation)
    for name, got, ref in zip(("mean", "scale", "logits"), (pm.grad, ps.grad, lg.grad), want):
        err = float((got - ref).abs().max()) / max(1e-300, float(ref.abs().max()))
        print(f"M={M} A={A} {std_activation}: d/d{name} autograd vs closed form {err:.3e}")
        assert err <= 1e-10, name


def test_restatement_sampler_picks_by_inverse_cdf():
    sd, feats, _, _ = _inputs(5, 64, 32, 5, 7)
    g = torch.Generator().manual_seed(9)
    u, eps = torch.rand(64, generator=g).double(), torch.randn(64, 7, generator=g).double()
    act, modes, margin = gmm_ref.sample_by_inverse_cdf(sd, feats, u, eps, 5, 7)
    pm, ps, lg = gmm_ref.decoder(sd, feats, 5, 7)
    pi = torch.softmax(lg, -1)
    for n in range(64):
        c, pick = 0.0, 4
        for m in range(5):
            c += float(pi[n, m])
            if float(u[n]) < c:
                pick = m
                break
        assert int(modes[n]) == pick
        want = torch.tanh(pm[n, pick]) + (torch.nn.functional.softplus(ps[n, pick]) + 0.01) * eps[n]
        assert float((act[n] - want).abs().max()) <= 1e-12
    assert float(margin.min()) > 0.0
    first = gmm_ref.sample_by_inverse_cdf(sd, feats, torch.zeros(64).double(), eps, 5, 7)[1]
    last = gmm_ref.sample_by_inverse_cdf(sd, feats, torch.full((64,), 1.0 - 2.0 ** -24).double(), eps, 5, 7)[1]
    assert int(first.max()) == 0 and int(last.min()) == 4
