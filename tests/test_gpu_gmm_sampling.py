"""GPU: GMMActionHead under the in-kernel sample source (include/lipvq.h, "in-kernel sampling").  The drawing instances of
gmm_head_kernel are held to the instances that read u / eps: the noise the launch draws is written out by ops.gmm_noise, held to
the host mirror bit for bit, and fed back through the explicit-noise path, which must return the same bits.  Then the state
(steps, reseeding, graphs, the prompted policy), torch's generator left alone, the stream addressing, non-finite rows and the
sampled distribution.  Shapes are the smallest at which a tile edge, a draw group of four or a stride can go wrong."""
import numpy as np
import pytest
import torch

import gmm_ref
import gmm_sampling_ref as R
from fenced import _Fenced

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
MODES = {"softplus": 0, "exp": 1, "low_noise": 2}


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _head(E, A, M, act="softplus", seed=0):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gmm import GMMActionHead
    torch.manual_seed(seed)
    head = GMMActionHead(E, A, num_modes=M, std_activation="exp" if act == "exp" else "softplus", low_noise_eval=(act == "low_noise"))
    return head.cuda().eval()


def _feats(B, T, E, layout, seed=1):
    g = torch.Generator().manual_seed(seed)
    if layout == "view":
        return (torch.randn(B, 3 * T, E, generator=g) * 2.0).cuda()[:, -T:]
    return (torch.randn(B, T, E, generator=g) * 2.0).cuda()


def _snap(seed, step):
    words = [v - 2 ** 64 if v >= 2 ** 63 else v for v in (seed & (2 ** 64 - 1), step)]
    return torch.tensor(words, dtype=torch.int64, device="cuda")


def _nt(M, A):
    nt = ((M * (2 * A + 1) + 31) // 32 + 3) // 4
    return 1 if nt <= 1 else (2 if nt <= 2 else 4)


# (B, T, A, M, E, layout, act, explicit streams): rows 1 / 31 / 32 / 33 / 65 / 80; A 1, 3, 4, 5, 12, 64 and the widths that put
# P = M (2 A + 1) at 127, 129 (either side of one column tile per wave), 255 and 258 (of two); E 4, 36, 512
CASES = [
    (1, 1, 1, 1, 4, "dense", "softplus", False),            # P = 3
    (31, 1, 3, 5, 36, "dense", "exp", True),                # P = 35
    (4, 8, 4, 5, 512, "view", "softplus", True),            # 32 rows: one full tile
    (3, 11, 5, 16, 36, "view", "low_noise", False),         # 33 rows, P = 176: NT = 2
    (13, 5, 12, 5, 512, "view", "softplus", True),          # 65 rows, P = 125
    (8, 10, 12, 5, 512, "view", "low_noise", False),        # the rollout shape
    (8, 10, 64, 3, 36, "dense", "exp", True),               # P = 387: NT = 4, two draw groups per item
    (13, 5, 63, 1, 36, "view", "softplus", False),          # P = 127
    (3, 11, 21, 3, 4, "dense", "softplus", True),           # P = 129: NT = 2
    (4, 8, 8, 15, 36, "view", "exp", False),                # P = 255
    (31, 1, 21, 6, 512, "dense", "softplus", False),        # P = 258: NT = 4
    (13, 5, 64, 1, 36, "dense", "low_noise", True),         # A = 64 alone: P = 129
    (3, 11, 15, 16, 36, "view", "softplus", False),         # P = 496: the tile is past 64 KiB of LDS, reserved per instance
]


def test_the_cases_reach_every_instance(ops):
    assert ops.SAMPLE_SITE_GMM == R.SITE_U
    assert {_nt(c[3], c[2]) for c in CASES} == {1, 2, 4}
    assert {c[3] * (2 * c[2] + 1) for c in CASES} >= {127, 129, 255, 258}
    assert {c[0] * c[1] for c in CASES} == {1, 31, 32, 33, 65, 80} and {c[2] for c in CASES} >= {1, 3, 4, 5, 12, 64}
    assert {c[4] for c in CASES} == {4, 36, 512} and {c[5] for c in CASES} == {"dense", "view"} and {c[6] for c in CASES} == set(MODES)


@pytest.mark.parametrize("B,T,A,M,E,layout,act,with_ids", CASES)
def test_drawn_samples_are_the_explicit_noise_samples(ops, B, T, A, M, E, layout, act, with_ids):
    from lipvq_vae_amd import _capi
    head = _head(E, A, M, act, seed=B + A).set_sample_source("kernel", seed=SEED)
    feats = _feats(B, T, E, layout, seed=M)
    ids = torch.tensor([3 * (B - 1 - b) + 2 for b in range(B)], dtype=torch.int64) if with_ids else None
    dev_ids = None if ids is None else ids.cuda()
    step = 3
    head.reseed_sampling(SEED, step)
    got = head(feats, streams=dev_ids)
    assert got.shape == (B, T, A)
    u, eps = ops.gmm_noise(_snap(SEED, step), B, T, A, dev_ids)
    hu, heps = ops.gmm_noise_host(SEED, step, B, T, A, ids)
    assert torch.equal(u.cpu(), hu) and torch.equal(eps.cpu(), heps)                    # the device's noise is the host mirror's
    want = head(feats, u=u, eps=eps, streams=dev_ids)                                   # the instances that read u / eps
    assert torch.equal(got, want)
    assert head.sample_state.tolist() == [SEED - 2 ** 64, step + 1]                     # one draw call, the explicit call moved nothing
    if act != "low_noise":
        assert float((got - head(feats, u=u, eps=torch.zeros_like(eps))).abs().max()) > 0.0     # the noise is in the samples

    # the C entry point on a fenced output: the same bits, and not a word outside
    action = _Fenced("action", B * T, A, offset_words=1)
    pp = [p.detach().data_ptr() for p in head._params()]
    bstride = feats.stride(0) if B > 1 else T * E
    mode, snap = MODES[act], _snap(SEED, step)
    _capi.check(_capi.lib.lipvq_gmm_sample_draw_f32(feats.data_ptr(), bstride, *pp, snap.data_ptr(),
                                                    None if dev_ids is None else dev_ids.data_ptr(), action.ptr(), B * T, T, E, M, A, mode,
                                                    float(head.min_std), ops._stream()), "lipvq_gmm_sample_draw_f32")
    torch.cuda.synchronize()
    assert torch.equal(action.check().view(B, T, A), got)
    nu, neps = _Fenced("u", B * T, offset_words=1), _Fenced("eps", B * T, A, offset_words=1)
    _capi.check(_capi.lib.lipvq_gmm_noise_f32(snap.data_ptr(), None if dev_ids is None else dev_ids.data_ptr(), nu.ptr(), neps.ptr(),
                                              B, T, A, ops._stream()), "lipvq_gmm_noise_f32")
    torch.cuda.synchronize()
    assert torch.equal(nu.check().view(B, T), u) and torch.equal(neps.check().view(B, T, A), eps)


# ---------------------------------------------------------------------------------------------------
# state
# ---------------------------------------------------------------------------------------------------

def test_steps_reseeding_and_explicit_noise(ops):
    B, T, A, M, E = 3, 11, 5, 4, 36
    head = _head(E, A, M, seed=2)
    assert head.sample_state is None
    head.set_sample_source("kernel", seed=77)
    assert head.sample_state.is_cuda and head.sample_state.tolist() == [77, 0]
    feats = _feats(B, T, E, "view")
    s0 = 5
    head.reseed_sampling(77, s0)
    first = []
    for k in range(4):
        if k % 2:
            with torch.no_grad():
                first.append(head(feats).clone())
        else:
            first.append(head(feats).clone())
        assert head.sample_state.tolist() == [77, s0 + k + 1]
        u, eps = ops.gmm_noise(_snap(77, s0 + k), B, T, A)
        assert torch.equal(first[k], head(feats, u=u, eps=eps))                        # call k drew step s0 + k
        assert head.sample_state.tolist() == [77, s0 + k + 1]                          # both given: the state stays
    assert not torch.equal(first[0], first[1])
    head.reseed_sampling(77, 0)
    for k in range(3):
        head(feats)
    assert head.sample_state[1].item() == 3                                            # the number of calls
    head.reseed_sampling(77, s0)
    again = [head(feats).clone() for _ in range(4)]
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    u, eps = ops.gmm_noise(_snap(77, 0), B, T, A)
    before = head.sample_state.tolist()
    for kw in (dict(u=u), dict(eps=eps)):
        with pytest.raises(ValueError, match="both u and eps"):
            head(feats, **kw)
    with pytest.raises(ValueError, match="streams"):
        head(feats, streams=torch.arange(B + 1, device="cuda"))
    assert head.sample_state.tolist() == before
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gmm import GMMActionHead
    moved = GMMActionHead(E, A, num_modes=M).set_sample_source("kernel", seed=3)       # created on the host ...
    assert not moved.sample_state.is_cuda
    moved.cuda()                                                                       # ... .to() moves it with the parameters
    assert moved.sample_state.is_cuda and moved.sample_state.tolist() == [3, 0] and "_sample_state" not in moved.state_dict()
    head.train()                                                                       # sampling is not a training-only act
    head.reseed_sampling(77, s0)
    u, eps = ops.gmm_noise(_snap(77, s0), B, T, A)
    assert torch.equal(head(feats), head(feats, u=u, eps=eps)) and head.sample_state.tolist() == [77, s0 + 1]


def test_torch_generator_is_left_alone_and_the_default_source_keeps_its_bits():
    B, T, A, M, E = 4, 8, 12, 5, 36
    head = _head(E, A, M, seed=4)
    feats = _feats(B, T, E, "dense")
    torch.manual_seed(9)
    before = [head(feats).clone(), head(feats).clone()]                                # before the source was ever set
    head.set_sample_source("kernel", seed=1)
    state = torch.cuda.get_rng_state()
    cpu_state = torch.get_rng_state()
    outs = [head(feats).clone() for _ in range(3)]
    assert torch.equal(torch.cuda.get_rng_state(), state) and torch.equal(torch.get_rng_state(), cpu_state)
    assert not torch.equal(outs[0], outs[1])
    head.set_sample_source("torch")
    torch.manual_seed(9)
    after = [head(feats, streams=torch.arange(B, device="cuda")).clone(), head(feats).clone()]     # streams: validated, ignored
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert head.sample_state.tolist() == [1, 3]                                        # the torch source does not touch the state
    with pytest.raises(ValueError, match="streams"):
        head(feats, streams=torch.arange(B + 1, device="cuda"))


# ---------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,layout", [(1, "dense"), (4, "view")])
def test_an_environment_keeps_its_noise_wherever_it_sits(T, layout):
    A, M, E = 5, 3, 36
    ids = [7, 3, 0, 9, 2]
    head = _head(E, A, M, seed=6).set_sample_source("kernel", seed=SEED)
    feats = _feats(5, T, E, layout)
    dev_ids = torch.tensor(ids, device="cuda")
    head.reseed_sampling(SEED, 2)
    batch = head(feats, streams=dev_ids).clone()
    for pos, i in enumerate(ids):                                                      # the five B = 1 calls at the same step
        head.reseed_sampling(SEED, 2)
        assert torch.equal(head(feats[pos:pos + 1], streams=torch.tensor([i], device="cuda")), batch[pos:pos + 1]), i
    perm = torch.tensor([3, 0, 4, 1, 2], device="cuda")
    head.reseed_sampling(SEED, 2)
    assert torch.equal(head(feats[perm], streams=dev_ids[perm]), batch[perm])          # environments, features and ids together
    head.reseed_sampling(SEED, 2)
    moved = head(feats[perm], streams=dev_ids)                                         # ids left behind: other noise for these features
    assert not torch.equal(moved, batch[perm])
    head.reseed_sampling(SEED, 2)
    default = head(feats).clone()
    head.reseed_sampling(SEED, 2)
    assert torch.equal(head(feats, streams=torch.arange(5, device="cuda")), default)   # None = arange(B)
    big = torch.tensor([2 ** 32 + 7, 3, 2 ** 40, 9, 2], device="cuda")                 # T = 1: 2^32 + 7 wraps onto 7, 2^40 onto 0
    if T == 1:
        head.reseed_sampling(SEED, 2)
        assert torch.equal(head(feats, streams=big), batch)


# ---------------------------------------------------------------------------------------------------
# graph and policy
# ---------------------------------------------------------------------------------------------------

def test_graphed_eval_replays_the_eager_sequence():
    from lipvq_vae_amd.nnfn import GraphedEval
    B, T, A, M, E = 8, 10, 12, 5, 64
    head = _head(E, A, M, "low_noise", seed=8).set_sample_source("kernel", seed=5)
    feats = _feats(B, T, E, "dense")
    head.reseed_sampling(5, 11)
    eager = [head(feats).clone() for _ in range(4)]
    head.reseed_sampling(5, 11)
    graphed = GraphedEval(head, feats)
    assert head.sample_state.tolist() == [5, 11]                                       # construction gives the state back
    for k in range(4):
        assert torch.equal(graphed(feats), eager[k]), k
        assert head.sample_state.tolist() == [5, 12 + k]
    plain = _head(E, A, M, "low_noise", seed=8)                                        # a net without a state: nothing changes
    u, eps = torch.rand(B, T).cuda(), torch.randn(B, T, A).cuda()
    assert plain.sample_state is None
    GraphedEval(plain, feats)
    assert plain.sample_state is None and torch.equal(plain(feats, u=u, eps=eps), head(feats, u=u, eps=eps))


def test_prompted_policy_passes_streams_to_the_head():
    from lipvq_vae_amd.embedding import ICLInputEmbedding
    from lipvq_vae_amd.gpt import GPTBackbone
    from lipvq_vae_amd.icl import PromptedPolicy
    T, E, DIN, A, B = 4, 64, 16, 7, 5
    torch.manual_seed(21)
    emb = ICLInputEmbedding(DIN, E, T, emb_dropout=0.1).cuda().eval()
    net = GPTBackbone(E, 3 * T, num_layers=2, num_heads=4).cuda().eval()
    head = _head(E, A, 5, seed=22).set_sample_source("kernel", seed=SEED)
    g = torch.Generator().manual_seed(23)
    obs, ctx_obs, ctx_act = (torch.randn(B, T, DIN, generator=g).cuda() for _ in range(3))
    ids = torch.tensor([7, 3, 0, 9, 2], device="cuda")
    policy = PromptedPolicy(emb, net, head)
    policy.set_prompt(ctx_obs, ctx_act)
    head.reseed_sampling(SEED, 4)
    got = policy(obs, streams=ids).clone()
    assert head.sample_state.tolist() == [SEED - 2 ** 64, 5]                           # a policy step advances the state
    head.reseed_sampling(SEED, 4)
    assert got.shape == (B, T, A) and torch.equal(got, head(policy.features(obs), streams=ids))
    head.reseed_sampling(SEED, 4)
    assert not torch.equal(policy(obs), got)                                           # without ids: the batch positions' noise


# ---------------------------------------------------------------------------------------------------
# non-finite rows
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("A,M", [(5, 4), (64, 3)])
def test_a_nan_row_samples_nan_and_its_neighbours_do_not_notice(A, M):
    B, T, E = 13, 5, 36
    head = _head(E, A, M, seed=3).set_sample_source("kernel", seed=SEED)
    feats = _feats(B, T, E, "dense")
    head.reseed_sampling(SEED, 1)
    clean = head(feats).clone()
    bad = feats.clone()
    bad.view(-1, E)[[0, 17, 33, 64]] = float("nan")                                    # first row, mid tile, second row of tile 2, last row
    head.reseed_sampling(SEED, 1)
    got = head(bad).view(-1, A)
    rows = torch.zeros(B * T, dtype=torch.bool, device="cuda")
    rows[[0, 17, 33, 64]] = True
    assert bool(torch.isnan(got[rows]).all())
    assert torch.equal(got[~rows], clean.view(-1, A)[~rows]) and bool(torch.isfinite(got[~rows]).all())


# ---------------------------------------------------------------------------------------------------
# the distribution, through the kernel
# ---------------------------------------------------------------------------------------------------

DIST = dict(n=1 << 15, E=36, M=3, A=4, seed=12345, step=0, head_seed=31, feat_seed=32)


def dist_inputs():
    """(head on the CPU, the one feature row [E]) of the distribution test: seeded on the host, so that the seed can be checked
    against the host mirror before it is committed."""
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gmm import GMMActionHead
    torch.manual_seed(DIST["head_seed"])
    head = GMMActionHead(DIST["E"], DIST["A"], num_modes=DIST["M"], low_noise_eval=False)
    row = torch.randn(DIST["E"], generator=torch.Generator().manual_seed(DIST["feat_seed"])) * 2.0
    return head, row


def dist_caps():
    return 5.0, R.chi2_quantile(DIST["M"] - 1)


def test_sampled_moments_and_mode_frequencies(ops):
    n, M, A = DIST["n"], DIST["M"], DIST["A"]
    head, row = dist_inputs()
    sd = {k: v.double() for k, v in head.state_dict().items()}
    moments = R.mixture_moments(sd, row, M, A, head.min_std)
    head = head.cuda().eval().set_sample_source("kernel", seed=DIST["seed"])
    head.reseed_sampling(DIST["seed"], DIST["step"])
    feats = row.cuda().view(1, 1, -1).repeat(n, 1, 1)
    act = head(feats).view(n, A).cpu().double().numpy()
    assert np.isfinite(act).all()
    eps = ops.gmm_noise_host(DIST["seed"], DIST["step"], n, 1, A)[1].view(n, A).double().numpy()
    modes, residual = R.modes_of(act, moments[1], moments[2], eps)
    assert float(residual.max()) <= 1e-5                                               # every row is one mode's mu + sigma eps
    z_mean, z_var, chi2 = R.distribution_figures(act, modes, moments)
    cap, chi2_cap = dist_caps()
    print(f"pi {moments[0]}; z(mean) {z_mean}; z(var) {z_var}; chi-squared of the mode counts {chi2:.2f} (cap {chi2_cap:.2f})")
    assert float(np.abs(z_mean).max()) <= cap and float(np.abs(z_var).max()) <= cap
    assert chi2 < chi2_cap
    assert float(moments[0].min()) * n >= 100.0                                        # every mode is expected often enough for the test
