"""GPU: the policy's GMM output head (reference robomimic/models/policy_nets.py:2545-2599, obs_nets.py:747-771) on the HIP library.

The yardstick is the plain-torch restatement tests/gmm_ref.py on ``.double()`` tensors (CPU).  Bounds (tests/test_gpu_gpt.py's):
a forward tensor within 1e-5 of the yardstick's maximum magnitude, a gradient within 1e-4 -- or 4 x the deviation of the SAME
restatement in fp32 (CPU) from float64 on the same inputs if that is larger.  Every figure is printed before it is asserted.
Inputs are drawn from seeds; nothing is read from tests/golden.
"""
import numpy as np
import pytest
import torch

import gmm_ref
import gpt_ref

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL, REF_FACTOR = 1e-5, 1e-4, 4.0
MODES = {"softplus": 0, "exp": 1}


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _head(E, A, M, seed=0, **kw):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gmm import GMMActionHead
    torch.manual_seed(seed)
    return GMMActionHead(E, A, num_modes=M, **kw)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def _t(x):
    return x.detach().cpu().double().numpy()


def _reference(sd, feats, actions, g, M, A, min_std, act, dtype):
    """The restatement in `dtype` on the CPU: log_prob, activated mean / scale, raw logits, and the gradients of sum(g log_prob)
    with respect to the pre-activations [N, P], the input and the six parameters."""
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    x = feats.detach().to(dtype).requires_grad_(True)
    pm, ps, lg = gmm_ref.decoder(sd, x, M, A)
    for t in (pm, ps, lg):
        t.retain_grad()
    mu, sg = gmm_ref.activate(pm, ps, min_std, act)
    lp = gmm_ref.mixture(mu, sg, lg).log_prob(actions.to(dtype))
    (lp * g.to(dtype)).sum().backward()
    N = x.shape[0]
    out = {"log_prob": lp, "mean": mu, "scale": sg, "logits": lg, "gx": x.grad,
           "gpre": torch.cat((pm.grad.reshape(N, -1), ps.grad.reshape(N, -1), lg.grad.reshape(N, -1)), 1)}
    out.update({"g:" + k: v.grad for k, v in sd.items()})
    return {k: _t(v) for k, v in out.items()}


def _compare(tag, got, ref64, ref32):
    """Print every figure, then assert all of them."""
    bad = []
    for k, v in got.items():
        tol = FWD_TOL if k in ("log_prob", "mean", "scale", "logits", "sample", "nll") else BWD_TOL
        e, dev = _rel(v, ref64[k]), _rel(ref32[k], ref64[k])
        bound = max(tol, REF_FACTOR * dev)
        print(f"{tag}: {k} error {e:.3e}, fp32 restatement's own {dev:.3e}, bound {bound:.3e}")
        if not e <= bound:
            bad.append((k, e, bound))
    assert not bad, bad


def _layout(feats2, layout, T):
    """feats [B, T, E] on the GPU holding the rows of feats2 [N, E]: dense, or the view [:, -T:] of a [B, 3T, E] tensor."""
    N, E = feats2.shape
    B = N // T
    if layout == "dense":
        return feats2.view(B, T, E).cuda()
    full = torch.randn(B, 3 * T, E, generator=torch.Generator().manual_seed(1))
    full[:, -T:] = feats2.view(B, T, E)
    view = full.cuda()[:, -T:]
    assert not view.is_contiguous() or B == 1
    return view


# rows, E, (M, A), std_activation, layout, T: every listed size, both activations, both layouts, T = 1 and 10, P = 3 .. 496
CASES = [
    (1, 4, 1, 1, "softplus", "dense", 1),
    (31, 64, 5, 12, "softplus", "dense", 31),
    (33, 260, 5, 7, "exp", "dense", 1),
    (80, 512, 5, 12, "softplus", "view", 10),
    (80, 512, 5, 12, "exp", "view", 10),
    (31, 512, 3, 10, "exp", "view", 1),
    (33, 1024, 16, 15, "softplus", "dense", 33),
    (80, 1024, 16, 15, "exp", "view", 10),
    (4097, 64, 5, 12, "softplus", "dense", 1),
    (4097, 260, 3, 10, "exp", "view", 1),
    (4097, 4, 1, 1, "exp", "dense", 4097),
]


@pytest.mark.parametrize("N,E,M,A,act,layout,T", CASES)
def test_kernels_against_the_float64_restatement(ops, N, E, M, A, act, layout, T):
    from lipvq_vae_amd.gmm import _LogProbFn
    head = _head(E, A, M, seed=N + E + M)
    gen = torch.Generator().manual_seed(7 * N + E + A)
    feats2 = torch.randn(N, E, generator=gen)
    actions = torch.rand(N, A, generator=gen) * 3.0 - 1.5                          # partly outside tanh's range
    g = torch.randn(N, generator=gen)
    sd = head.state_dict()
    ref64 = _reference(sd, feats2, actions, g, M, A, 0.01, act, torch.float64)
    ref32 = _reference(sd, feats2, actions, g, M, A, 0.01, act, torch.float32)
    head = head.cuda()
    params = head._params()
    feats = _layout(feats2, layout, T).requires_grad_(True)
    ac = actions.cuda()
    out = ops.gmm_head(feats.detach(), params, M, A, ac, MODES[act], 0.01, want_pre=True, want_params=True, want_sum=True)
    got = {k: _t(out[k]) for k in ("log_prob", "mean", "scale", "logits")}
    got["log_prob"] = got["log_prob"].reshape(ref64["log_prob"].shape)
    for k in ("mean", "scale", "logits"):
        got[k] = got[k].reshape(ref64[k].shape)
    # the product is lipvq_linear_act_f32's chain on the stacked parameters: the same bits
    stacked = ops.linear(feats.detach().reshape(N, E), torch.cat(params[0::2], 0), torch.cat(params[1::2], 0))
    assert torch.equal(out["pre"], stacked)
    got["gpre"] = _t(ops.gmm_head_bwd(out["pre"], ac, g.cuda(), None, M, A, MODES[act], 0.01))
    lp = _LogProbFn.apply(feats, ac.view(feats.shape[0], feats.shape[1], A), *params, M, A, MODES[act], 0.01, False)[0]
    assert torch.equal(lp.reshape(-1), out["log_prob"])
    (lp.reshape(-1) * g.cuda()).sum().backward()
    assert feats.grad.shape == feats.shape
    got["gx"] = _t(feats.grad).reshape(N, E)
    for k, p in zip(gmm_ref.KEYS, params):
        got["g:" + k] = _t(p.grad)
    # the sum output: the rows' log_prob added up (float64 accumulation of the fp32 values)
    s = float(out["sum"])
    print(f"sum {s!r} vs {float(got['log_prob'].sum())!r}")
    assert abs(s - got["log_prob"].sum()) <= FWD_TOL * np.abs(got["log_prob"]).max() * N
    _compare(f"N={N} E={E} M={M} A={A} {act} {layout} T={T}", got, ref64, ref32)


def _edge(ops, pm, ps, lg, actions, act="softplus", min_std=0.01):
    """Kernels and restatement on GIVEN pre-activations pm, ps [N, M, A], lg [N, M] (log_prob and, with g = 1, gpre).  Rows are
    independent, so row n runs as its own call with E = 4, zero weights and bias = that row's pre-activations: exact."""
    N, M, A = pm.shape
    rows = {"log_prob": [], "gpre": []}
    for n in range(N):
        bias = (pm[n].reshape(-1), ps[n].reshape(-1), lg[n].reshape(-1))
        params = []
        for b in bias:
            params += [torch.zeros(b.numel(), 4, device="cuda"), b.float().cuda()]
        out = ops.gmm_head(torch.ones(1, 1, 4, device="cuda"), tuple(params), M, A, actions[n:n + 1].float().cuda(), MODES[act], min_std,
                           want_pre=True)
        assert torch.equal(out["pre"].cpu().reshape(-1), torch.cat(bias).float())
        rows["log_prob"].append(out["log_prob"])
        rows["gpre"].append(ops.gmm_head_bwd(out["pre"], actions[n:n + 1].float().cuda(), torch.ones(1, device="cuda"), None, M, A,
                                             MODES[act], min_std))
    got = {k: _t(torch.cat(v, 0)) for k, v in rows.items()}
    refs = []
    for dtype in (torch.float64, torch.float32):
        p = [t.detach().clone().to(dtype).requires_grad_(True) for t in (pm, ps, lg)]
        mu, sg = gmm_ref.activate(p[0], p[1], min_std, act)
        lp = gmm_ref.mixture(mu, sg, p[2]).log_prob(actions.float().to(dtype))
        lp.sum().backward()
        refs.append({"log_prob": _t(lp), "gpre": _t(torch.cat([t.grad.reshape(N, -1) for t in p], 1))})
    return got, refs[0], refs[1]


def _edge_inputs(seed, N=6, M=5, A=12):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, M, A, generator=g), torch.randn(N, M, A, generator=g), torch.randn(N, M, generator=g),
            torch.rand(N, A, generator=g) * 3.0 - 1.5)


def test_edge_softplus_threshold(ops):
    pm, ps, lg, x = _edge_inputs(1)
    for n, v in enumerate((19.5, 20.0, 20.5, -30.0)):
        ps[n, :, ::2] = v
    ps[4, 0], ps[4, 1], ps[4, 2], ps[4, 3] = 19.5, 20.0, 20.5, -30.0
    got, r64, r32 = _edge(ops, pm, ps, lg, x)
    assert np.isfinite(got["log_prob"]).all() and np.isfinite(got["gpre"]).all()
    _compare("softplus threshold", got, r64, r32)


def test_edge_all_modes_far_away(ops):
    """Every mode's l is about -1e6: the max-subtracted logsumexp stays finite."""
    pm, ps, lg, x = _edge_inputs(2)
    ps[:] = -6.0 + 0.1 * ps                                                        # sigma ~ 0.0075 (min_std 0.005) ...
    ps[:3] = -9.0                                                                  # ... and 0.0051
    pm[:] = -3.0 + 0.1 * pm                                                        # mu ~ -0.995, actions +1.5: (d / sigma)^2 / 2 ~ 5e4 .. 1.2e5
    x[:] = 1.5                                                                     # per component, 12 components
    got, r64, r32 = _edge(ops, pm, ps, lg, x, min_std=0.005)
    print("log_prob", got["log_prob"])
    assert (r64["log_prob"] < -5e5).all() and r64["log_prob"].min() < -1e6
    assert np.isfinite(got["log_prob"]).all() and np.isfinite(got["gpre"]).all()
    _compare("all modes far", got, r64, r32)


def test_edge_one_mode_dominant(ops):
    pm, ps, lg, x = _edge_inputs(3)
    lg[:, 2] += 50.0                                                               # by 50 nats
    got, r64, r32 = _edge(ops, pm, ps, lg, x)
    _compare("dominant mode", got, r64, r32)


def test_edge_logits_spread(ops):
    pm, ps, lg, x = _edge_inputs(4)
    lg[:] = torch.linspace(-40.0, 40.0, 5).repeat(6, 1)
    lg[1] = lg[1].flip(0)
    lg[2] = torch.tensor([40.0, -40.0, 40.0, -40.0, 0.0])
    got, r64, r32 = _edge(ops, pm, ps, lg, x)
    _compare("logits +-40", got, r64, r32)


def test_edge_min_std_zero(ops):
    pm, ps, lg, x = _edge_inputs(5)
    ps[:] = ps.clamp(min=-10.0)
    ps[0] = -10.0                                                                  # sigma = softplus(-10) = 4.5e-5, a normal fp32 number
    ps[1, :, 0] = -10.0
    for act in ("softplus", "exp"):
        got, r64, r32 = _edge(ops, pm, ps, lg, x, act=act, min_std=0.0)
        assert np.isfinite(got["log_prob"]).all() and np.isfinite(got["gpre"]).all()
        _compare(f"min_std 0 {act}", got, r64, r32)


# ---------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def step():
    """The ICRT step shape: head, a [B, 3T, E] backbone-like output, actions, and the float64 / fp32 restatement's log_prob."""
    B, T, E, M, A = 8, 10, 512, 5, 12
    head = _head(E, A, M, seed=5)
    gen = torch.Generator().manual_seed(6)
    full = torch.randn(B, 3 * T, E, generator=gen)
    actions = torch.rand(B, T, A, generator=gen) * 3.0 - 1.5
    sd = head.state_dict()
    lp = {}
    for dtype in (torch.float64, torch.float32):
        sdd = {k: v.to(dtype) for k, v in sd.items()}
        lp[dtype] = _t(gmm_ref.gmm_log_prob(sdd, full[:, -T:].to(dtype), actions.to(dtype), M, A))
    return head.cuda(), full.cuda(), actions.cuda(), lp, (B, T, E, M, A)


def test_nll_is_minus_mean_log_prob_and_repeats_bit_for_bit(step):
    head, full, actions, lp, (B, T, E, M, A) = step
    head.train()
    feats = full[:, -T:]
    want = -lp[torch.float64].mean()
    dev = abs(-lp[torch.float32].mean() - want) / np.abs(lp[torch.float64]).max()
    runs = []
    for _ in range(2):
        head.zero_grad(set_to_none=True)
        fg = full.clone().requires_grad_(True)
        loss = head.nll(fg[:, -T:], actions)
        loss.backward()
        runs.append([loss.detach().clone(), fg.grad.clone()] + [p.grad.clone() for p in head.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "a second pass gave other bits"
    assert runs[0][1].shape == full.shape and float(runs[0][1][:, :-T].abs().max()) == 0.0
    with torch.no_grad():
        e = abs(float(runs[0][0]) - want) / np.abs(lp[torch.float64]).max()
        e2 = abs(float(runs[0][0]) + float(head.log_prob(feats, actions).double().mean())) / np.abs(lp[torch.float64]).max()
    bound = max(FWD_TOL, REF_FACTOR * dev)
    print(f"nll {float(runs[0][0])!r} vs float64 {want!r}: error {e:.3e} (vs own log_prob mean {e2:.3e}), bound {bound:.3e}")
    assert e <= bound and e2 <= bound
    # nll's gradients are log_prob's with g = -1 / rows
    head.zero_grad(set_to_none=True)
    (-head.log_prob(feats, actions).sum() / (B * T)).backward()
    for p, ref in zip(head.parameters(), runs[0][2:]):
        assert _rel(_t(p.grad), _t(ref)) <= 1e-6


def test_forward_train_distribution(step):
    head, full, actions, lp, (B, T, E, M, A) = step
    feats = full[:, -T:]
    head.train()
    dist = head.forward_train(feats)
    assert tuple(dist.batch_shape) == (B, T) and tuple(dist.event_shape) == (A,)
    ours = head.log_prob(feats, actions)
    bound = max(FWD_TOL, REF_FACTOR * _rel(lp[torch.float32], lp[torch.float64]))
    e1, e2 = _rel(_t(dist.log_prob(actions)), lp[torch.float64]), _rel(_t(dist.log_prob(actions)), _t(ours))
    print(f"forward_train().log_prob vs float64 {e1:.3e}, vs log_prob() {e2:.3e}, bound {bound:.3e}")
    assert e1 <= bound and e2 <= bound
    soft = dist.component_distribution.base_dist.scale.detach()
    assert float(soft.min()) > 0.01 and float(soft.max()) > 0.1                     # softplus + min_std
    # the low-noise rule (policy_nets.py:2553-2560): the flag AND eval mode
    assert torch.equal(head.forward_train(feats, low_noise_eval=True).component_distribution.base_dist.scale, soft)    # training mode
    head.eval()
    low = head.forward_train(feats).component_distribution.base_dist.scale
    assert torch.equal(low, torch.full_like(low, 1e-4))
    assert torch.equal(head.forward_train(feats, low_noise_eval=False).component_distribution.base_dist.scale, soft)
    head.train()
    # icl.py:931-945: the last-timestep-only rebuild works on the returned object, with autograd through it
    import torch.distributions as D
    head.zero_grad(set_to_none=True)
    dist = head.forward_train(feats, low_noise_eval=False)
    comp = D.Independent(D.Normal(loc=dist.component_distribution.base_dist.loc[:, -1],
                                  scale=dist.component_distribution.base_dist.scale[:, -1]), 1)
    last = D.MixtureSameFamily(mixture_distribution=D.Categorical(logits=dist.mixture_distribution.logits[:, -1]),
                               component_distribution=comp)
    lp_last = last.log_prob(actions[:, -1])
    e = _rel(_t(lp_last), lp[torch.float64][:, -1])
    print(f"last-timestep rebuild {e:.3e}, bound {bound:.3e}")
    assert tuple(lp_last.shape) == (B,) and e <= bound
    (-lp_last.mean()).backward()
    grads_dist = [p.grad.clone() for p in head.parameters()]
    head.zero_grad(set_to_none=True)
    (-head.log_prob(feats, actions)[:, -1].mean()).backward()
    for a, b in zip(grads_dist, head.parameters()):
        e = _rel(_t(a), _t(b.grad))
        print(f"gradient through the distribution object vs log_prob(): {e:.3e}")
        assert e <= BWD_TOL


def _sampling_inputs():
    """Seeds checked on the CPU: in float64 no row's u is within 1e-5 of a CDF boundary."""
    B, T, E, M, A = 8, 10, 512, 5, 12
    head = _head(E, A, M, seed=5)
    gen = torch.Generator().manual_seed(21)
    feats = torch.randn(B, T, E, generator=gen)
    u = torch.rand(B, T, generator=gen)
    eps = torch.randn(B, T, A, generator=gen)
    return head, feats, u, eps, (B, T, E, M, A)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_sampling_matches_the_float64_sampler(mode):
    head, feats, u, eps, (B, T, E, M, A) = _sampling_inputs()
    sd64 = {k: v.double() for k, v in head.state_dict().items()}
    low = mode == "eval"
    want, modes, margin = gmm_ref.sample_by_inverse_cdf(sd64, feats.double(), u.double(), eps.double(), M, A, low_noise=low)
    sd32 = dict(head.state_dict())
    want32 = gmm_ref.sample_by_inverse_cdf(sd32, feats, u, eps, M, A, low_noise=low)[0]
    keep = margin >= 1e-5
    assert bool(keep.all()), "the seeds must leave every row away from the CDF boundaries"
    assert len(set(modes.reshape(-1).tolist())) >= 3                                # several modes are actually drawn
    head = head.cuda().train(not low)
    got = head(feats.cuda(), u.cuda(), eps.cuda())
    assert got.shape == (B, T, A)
    e, dev = _rel(_t(got)[keep.numpy()], _t(want)[keep.numpy()]), _rel(_t(want32), _t(want))
    bound = max(FWD_TOL, REF_FACTOR * dev)
    print(f"sampling ({mode}): error {e:.3e}, fp32 restatement's own {dev:.3e}, bound {bound:.3e}, rows excluded {int((~keep).sum())}")
    assert e <= bound
    # u = 0 picks the first mode, u just below 1 the last
    z = torch.zeros_like(eps).cuda()
    mu = torch.tanh(gmm_ref.decoder(sd64, feats.double(), M, A)[0])
    first, last = head(feats.cuda(), torch.zeros(B, T).cuda(), z), head(feats.cuda(), torch.full((B, T), 1.0 - 2.0 ** -24).cuda(), z)
    assert _rel(_t(first), _t(mu[:, :, 0])) <= FWD_TOL and _rel(_t(last), _t(mu[:, :, M - 1])) <= FWD_TOL
    # drawn inside: the right shape, finite, and different from call to call
    a1, a2 = head(feats.cuda()), head(feats.cuda())
    assert a1.shape == (B, T, A) and bool(torch.isfinite(a1).all()) and not torch.equal(a1, a2)


def test_graph_replay_samples_around_a_mode(step):
    """sigma = 1e-4 in eval mode, and |eps| > 6 has probability 2e-9 per draw: every row is within 6e-4 of one mode's tanh(mean)."""
    from lipvq_vae_amd.nnfn import GraphedEval
    head, full, actions, lp, (B, T, E, M, A) = step
    head.eval()
    feats = full[:, -T:].contiguous()
    graphed = GraphedEval(head, torch.zeros_like(feats))
    gen = torch.Generator().manual_seed(3)
    seen = []
    for i in range(3):
        x = (feats if i == 0 else torch.randn(B, T, E, generator=gen).cuda())
        out = graphed(x).clone()
        with torch.no_grad():
            means = head.forward_train(x).component_distribution.base_dist.loc          # [B, T, M, A], tanh applied
        d = (out.unsqueeze(2) - means).abs().amax(-1).amin(-1)                          # distance to the nearest mode, per row
        print(f"replay {i}: largest distance to the nearest mode {float(d.max()):.3e}")
        assert out.shape == (B, T, A) and float(d.max()) <= 6e-4
        seen.append(out)
    assert not torch.equal(seen[0], seen[1])
    with pytest.raises(ValueError):
        graphed(feats[:1])
    with pytest.raises(RuntimeError):
        GraphedEval(head.train(), feats)


def test_backbone_feeds_the_head():
    """tokenizer -> embedding -> backbone -> head: the NLL's gradient reaches the backbone's first block."""
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gpt import GPTBackbone
    B, L, E, H, layers, T, M, A = 3, 12, 64, 4, 2, 4, 5, 7
    torch.manual_seed(31)
    net = GPTBackbone(E, L, attn_dropout=0.0, block_output_dropout=0.0, num_layers=layers, num_heads=H)
    head = _head(E, A, M, seed=32)
    gen = torch.Generator().manual_seed(33)
    x = torch.randn(B, L, E, generator=gen)
    actions = torch.rand(B, T, A, generator=gen) * 3.0 - 1.5
    ref = {}
    for dtype in (torch.float64, torch.float32):
        params = dict(net.named_parameters())
        sd = {k: params[k].detach().to(dtype).requires_grad_(True) if k in params else v for k, v in net.state_dict().items()}
        hsd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in head.state_dict().items()}
        out = gpt_ref.gpt_forward(sd, x.to(dtype), layers, H)
        loss = -gmm_ref.gmm_log_prob(hsd, out[:, -T:], actions.to(dtype), M, A).mean()
        loss.backward()
        ref[dtype] = {"nll": _t(loss), "qkv": _t(sd["nets.transformer.0.nets.attention.nets.qkv.weight"].grad),
                      "head.mean": _t(hsd["nets.mean.weight"].grad)}
    net, head = net.cuda().train(), head.cuda().train()
    out = net(x.cuda())
    loss = head.nll(out[:, -T:], actions.cuda())
    loss.backward()
    got = {"nll": _t(loss), "qkv": _t(net.nets["transformer"][0].nets["attention"].nets["qkv"].weight.grad),
           "head.mean": _t(head.nets["mean"].weight.grad)}
    bad = []
    for k in got:
        tol = FWD_TOL if k == "nll" else BWD_TOL
        e, dev = _rel(got[k], ref[torch.float64][k]), _rel(ref[torch.float32][k], ref[torch.float64][k])
        bound = max(tol, REF_FACTOR * dev)
        print(f"chain: {k} error {e:.3e}, fp32 restatement's own {dev:.3e}, bound {bound:.3e}")
        if not e <= bound:
            bad.append((k, e, bound))
    assert not bad, bad
