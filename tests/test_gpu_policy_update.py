"""GPU: the policy's update on the HIP library (csrc/lipvq_optim.hip through lipvq_vae_amd.optim and icl.GraphedPolicyStep): the
multi-tensor sum of squares, the clip coefficient, the in-place scale, Adam / AdamW with the clip and a device learning rate
folded in, ``backprop_for_loss`` and the graphed training step.

Yardsticks (tests/optim_ref.py; conditions in tests/test_optim_ref_host.py): torch's clip_grad_norm_ followed by torch.optim.Adam /
AdamW on float64 CPU copies fed the same fp32 gradients.  Bounds: the sum of squares total_numel 2^-52 relative against float64
numpy (the squares are exact in double, at most total_numel double additions follow); stats 1e-12 relative; clipped gradients
2 ulp of fp32; trajectories the project's existing AdamW bound, 2e-6 max(1, max|p|) on parameters and rtol 1e-5 on exp_avg_sq, or
where stock fp32 torch on the CPU itself exceeds it, 4 x stock fp32 torch's own error against the same yardstick.

Worst figures, MI355X (also LABNOTES "Policy update"): the sum of squares uses 0.0031 of its bound; total_norm and clip_coef
4.2e-13 from torch's float64 values, sumsq 3.9e-16 from numpy's; clipped gradients 1.09 ulp; parameters 0.28 of the existing
bound (AdamW, huge, scale 1e4) and exp_avg_sq 0.19; one comparison (Adam, two groups, randn_decades, max_grad_norm 1.0) is over
the existing bound and at 0.18 of 4 x stock fp32's error."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import bin_ref as B
import optim_ref as R
from fenced import _Fenced

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()                  # a copy: the yardstick's arrays are read-only


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _off_boundary(t):
    """The same values as a view one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    v = buf[1:]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _params_with_grads(grads, shifted=False):
    ps = []
    for g in grads:
        p = torch.zeros(1 if g is None else g.size, device="cuda", requires_grad=True)
        if g is not None:
            p.grad = _off_boundary(cuda(g)) if shifted else cuda(g)
        ps.append(p)
    return ps


def _lists(count):
    """Parameter-size lists of one length: every size of ADAMW_SIZES alone for length 1."""
    return [[n] for n in B.ADAMW_SIZES] if count == 1 else [B.adamw_sizes(count)]


# ---- sum of squares ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", R.LIST_LENGTHS)
@pytest.mark.parametrize("regime", R.CLIP_REGIMES)
def test_sum_of_squares(regime, count):
    from lipvq_vae_amd.optim import clip_grad_norm_
    for sizes in _lists(count):
        for step, shifted in ((0, False), (1, True)):                   # step 1: parameters 3, 14, ... have no gradient
            grads = R.grads_at(regime, sizes, step)
            if count > 3:
                assert (step == 1) == any(g is None for g in grads)
            if all(g is None for g in grads):
                continue
            want, numel = R.sumsq_f64(grads)
            ps = _params_with_grads(grads, shifted)
            before = [None if p.grad is None else p.grad.clone() for p in ps]
            s1 = clip_grad_norm_(ps, math.inf).clone()                   # max_norm = +inf: report only
            s2 = clip_grad_norm_(ps, math.inf)
            assert s1.dtype == torch.float64 and s1.shape == (4,)
            assert torch.equal(s1.view(torch.int64), s2.view(torch.int64))                  # two runs: the same bits
            for p, b in zip(ps, before):                                                    # scaled by 1.0f: exact
                assert (p.grad is None) == (b is None) and (b is None or same_bits(p.grad, b))
            norm, coef, sumsq, clipped = (float(v) for v in s1)
            rel = abs(sumsq - want) / want if want else abs(sumsq)
            print(f"{regime} {count} tensors step {step} shifted {shifted}: sumsq uses {rel / (numel * R.EPS52):.3g} of numel 2^-52")
            assert rel <= numel * R.EPS52, (sumsq, want)
            assert abs(norm - math.sqrt(want)) <= (numel + 1) * R.EPS52 * math.sqrt(want)
            assert coef == 1.0 and clipped == sumsq
            if regime in ("huge", "tiny"):
                assert math.isfinite(norm) and norm > 0.0
            if regime == "zero":
                assert norm == 0.0


# ---- clip --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", R.MAX_NORMS)
@pytest.mark.parametrize("regime", R.CLIP_REGIMES)
def test_clip_grad_norm_in_place(regime, max_norm):
    from lipvq_vae_amd.optim import clip_grad_norm_
    sizes = B.adamw_sizes(33)
    for step in (0, 3, 4):
        grads = R.grads_at(regime, sizes, step)
        want, clipped = R.clip_yardstick(grads, max_norm)
        ps = _params_with_grads(grads, shifted=(step == 3))
        versions = [None if p.grad is None else p.grad._version for p in ps]
        stats = host(clip_grad_norm_(ps, max_norm))
        # total_norm and clip_coef against torch's own; the two sums of squares against the float64 numpy sum (torch's float64
        # norm is itself up to 4.2e-13 from the exact value on `huge`; squaring it, or summing its per-tensor norms as the
        # reference's loop does, reaches 1.1e-12)
        sumsq, _ = R.sumsq_f64(grads)
        coef = min(1.0, max_norm / (math.sqrt(sumsq) + 1e-6))
        want = (want[0], want[1], sumsq, coef * coef * sumsq)
        for name, g, w in zip(("total_norm", "clip_coef", "sumsq", "sumsq_clipped"), stats, want):
            print(f"{regime} max_norm {max_norm} step {step}: {name} {abs(g - w) / abs(w) if w else abs(g):.2e} relative")
            assert abs(g - w) <= 1e-12 * abs(w), (regime, step, name, g, w)
        worst = 0.0
        for p, c, v in zip(ps, clipped, versions):
            assert (p.grad is None) == (c is None)
            if c is None:
                continue
            assert p.grad._version > v
            got, ref = host(p.grad).astype(np.float64), c.numpy()
            worst = max(worst, float((np.abs(got - ref) / R.ulp32(ref)).max()))
        print(f"{regime} max_norm {max_norm} step {step}: coef {want[1]:.3g}, clipped gradients within {worst:.3f} ulp")
        assert worst <= 2.0


@pytest.mark.parametrize("offset", (0, 1, 2, 3))
def test_scale_writes_inside_its_tensors_only(offset):
    from lipvq_vae_amd.optim import clip_grad_norm_
    sizes = (1, 2, 3, 4, 5, 7, 8, 9, 255, 1030, 4099)
    rng = B.rng_of(offset, 41)
    fences = [_Fenced(f"grad[{n}]", n, offset_words=offset) for n in sizes]
    vals = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    ps = []
    for f, v in zip(fences, vals):
        f.t.copy_(cuda(v))
        p = torch.zeros(v.size, device="cuda", requires_grad=True)
        p.grad = f.t
        ps.append(p)
    stats = host(clip_grad_norm_(ps, 0.5))
    want, clipped = R.clip_yardstick(vals, 0.5)
    assert want[1] < 1.0 and abs(stats[1] - want[1]) <= 1e-12 * want[1]
    for f, c in zip(fences, clipped):
        got = host(f.check()).astype(np.float64)
        assert (np.abs(got - c.numpy()) <= 2.0 * R.ulp32(c.numpy())).all()


@pytest.mark.parametrize("bad", (float("nan"), float("inf")))
def test_clip_non_finite_as_stock_torch(bad):
    from lipvq_vae_amd.optim import clip_grad_norm_
    sizes = B.adamw_sizes(33)
    grads = [np.array(g) for g in R.grads_at("randn_decades", sizes, 2)]
    at = sizes.index(65537)
    grads[at][grads[at].size // 2] = bad
    _, want = R.clip_yardstick(grads, 1.0, dtype=torch.float32)                             # stock fp32 torch on the CPU
    ps = _params_with_grads(grads)
    stats = host(clip_grad_norm_(ps, 1.0))
    if math.isnan(bad):
        assert np.isnan(stats).all()
    else:
        assert stats[0] == math.inf and stats[1] == 0.0 and stats[2] == math.inf and math.isnan(stats[3])
    kinds = set()
    for p, w in zip(ps, want):
        got, w = host(p.grad), w.numpy()
        assert np.array_equal(np.isnan(got), np.isnan(w))
        assert np.array_equal(got[~np.isnan(got)], w[~np.isnan(w)])                         # zeros where torch has zeros
        kinds.add((bool(np.isnan(got).all()), bool(np.isnan(got).any())))
    assert kinds == ({(True, True)} if math.isnan(bad) else {(False, False), (False, True)})


# ---- Adam and AdamW with clipping ----------------------------------------------------------------------------------------------

def _classes(decoupled):
    from lipvq_vae_amd import optim
    return (optim.AdamW, torch.optim.AdamW) if decoupled else (optim.Adam, torch.optim.Adam)


def _adam_run(groups, regime, scale, decoupled, max_grad_norm, lr=1e-3, schedule=None):
    """groups: list of (sizes, kwargs).  ADAMW_STEPS steps of the fused optimizer on the GPU and of the float64 yardstick on the CPU
    with the same fp32 gradients; asserts after every step.  Stock fp32 torch on the CPU is run (up to the step in question) only
    where the project's bound is exceeded.  schedule: a LambdaLR multiplier; ours then runs with a device-tensor lr."""
    ours_cls, torch_cls = _classes(decoupled)
    inits = [(B.adamw_params(sizes, scale, seed=len(sizes)), kw) for sizes, kw in groups]
    sizes = [n for s, _ in groups for n in s]
    gp = [dict(params=[cuda(p).requires_grad_(True) for p in init], **kw) for init, kw in inits]
    flat_g = [p for g in gp for p in g["params"]]
    lr_ours = torch.tensor(lr, dtype=torch.float32, device="cuda") if schedule else lr
    ours = ours_cls(gp, lr=lr_ours, weight_decay=1e-4, max_grad_norm=max_grad_norm)
    ref = R.Trajectory(torch_cls, inits, torch.float64, max_grad_norm, lr=lr, weight_decay=1e-4)
    scheds = []
    if schedule:
        scheds = [torch.optim.lr_scheduler.LambdaLR(o, schedule) for o in (ours, ref.opt)]
        lr_ptr = lr_ours.data_ptr()
    stock = {}

    def stock_at(step):
        """Stock fp32 torch after `step` + 1 steps."""
        if not stock:
            stock["t"], stock["done"] = R.Trajectory(torch_cls, inits, torch.float32, max_grad_norm, lr=lr, weight_decay=1e-4), 0
            stock["sched"] = torch.optim.lr_scheduler.LambdaLR(stock["t"].opt, schedule) if schedule else None
        while stock["done"] <= step:
            stock["t"].step(R.grads_at(regime, sizes, stock["done"]))
            if schedule:
                stock["sched"].step()
            stock["done"] += 1
        return stock["t"]
    worst_p, worst_v, widened = 0.0, 0.0, 0
    for step in range(B.ADAMW_STEPS):
        grads = R.grads_at(regime, sizes, step)
        for a, g in zip(flat_g, grads):
            a.grad = None if g is None else cuda(g)
        before = [a._version for a in flat_g]
        ours.step()
        ref.step(grads)
        for s in scheds:
            s.step()
        if schedule:
            assert ours.param_groups[0]["lr"] is lr_ours and lr_ours.data_ptr() == lr_ptr
            assert abs(float(lr_ours) - ref.opt.param_groups[0]["lr"]) <= 1e-7 * lr
        if max_grad_norm is not None:
            want = R.stats_at(regime, sizes, step, max_grad_norm)
            got = host(ours.grad_stats)
            assert all(abs(g - w) <= 1e-12 * abs(w) for g, w in zip(got, want)), (regime, step, got, want)
        else:
            assert ours.grad_stats is None
        for index, (a, b, g) in enumerate(zip(flat_g, ref.flat, grads)):
            assert (a._version > before[index]) == (g is not None), (step, index)
            if g is not None:
                assert same_bits(a.grad, cuda(g))                                            # p.grad keeps the unclipped gradient
            err = float((a.detach().cpu().double() - b.detach()).abs().max())
            bound = existing = 2e-6 * max(1.0, float(b.detach().abs().max()))
            if err > existing:
                c = stock_at(step).flat[index]
                bound = max(existing, 4.0 * float((c.detach().double() - b.detach()).abs().max()))
                widened += 1
            worst_p = max(worst_p, err / bound)
            assert err <= bound, (regime, scale, step, index, a.numel(), err, existing, bound)
    for index, (a, b) in enumerate(zip(flat_g, ref.flat)):
        sa, sb = ours.state[a], ref.opt.state[b]
        assert (len(sa) == 0) == (len(sb) == 0)
        assert float(sa["step"]) == float(sb["step"]), index
        va, vb = sa["exp_avg_sq"].cpu().double(), sb["exp_avg_sq"]
        tol = 1e-12 + 1e-5 * vb.abs()
        if not bool(((va - vb).abs() <= tol).all()):
            c = stock_at(B.ADAMW_STEPS - 1).flat[index]
            tol = torch.maximum(tol, 4.0 * (stock["t"].opt.state[c]["exp_avg_sq"].double() - vb).abs())
            widened += 1
        assert bool(((va - vb).abs() <= tol).all()), (regime, scale, index)
        worst_v = max(worst_v, float(((va - vb).abs() / tol).max()))
    steps = {float(ours.state[a]["step"]) for a in flat_g}
    assert steps == {float(B.ADAMW_STEPS), float(B.ADAMW_STEPS - 2)}                        # some parameters skipped two steps
    print(f"{ours_cls.__name__} {regime} scale {scale:g} max_grad_norm {max_grad_norm} {[len(s) for s, _ in groups]} tensors: "
          f"parameters use {worst_p:.3f} of the bound ({widened} comparisons needed 4 x stock fp32's error), exp_avg_sq {worst_v:.3f}")


@pytest.mark.parametrize("decoupled", (False, True))
@pytest.mark.parametrize("count", (33, 65))
@pytest.mark.parametrize("regime", R.CLIP_REGIMES)
def test_adam_with_clipping(regime, count, decoupled):
    for max_grad_norm in R.MAX_NORMS + (None,):
        _adam_run([(B.adamw_sizes(count), {})], regime, 1.0, decoupled, max_grad_norm)
    if count == 33:
        _adam_run([(B.adamw_sizes(count), {})], regime, 1e4, decoupled, 1.0)


@pytest.mark.parametrize("decoupled", (False, True))
@pytest.mark.parametrize("regime", ("randn_decades", "spike"))
def test_adam_two_groups_one_norm(regime, decoupled):
    sizes = B.adamw_sizes(33)
    for max_grad_norm in R.MAX_NORMS + (None,):
        _adam_run([(sizes[:20], dict(lr=3e-3, betas=(0.8, 0.99), weight_decay=0.1)),
                   (sizes[20:], dict(lr=1e-4, betas=(0.95, 0.9999), weight_decay=0.0))], regime, 1.0, decoupled, max_grad_norm)


@pytest.mark.parametrize("decoupled", (False, True))
def test_scheduler_drives_a_device_lr(decoupled):
    _adam_run([(B.adamw_sizes(33), {})], "randn_decades", 1.0, decoupled, 1.0, schedule=lambda i: min(1.0, (i + 1) / 4))


# ---- equalities, bit for bit ---------------------------------------------------------------------------------------------------

def _trajectory_bits(make, regime="randn_decades", count=33, scale=1.0):
    """Six steps of make(params) on fresh copies of the same start; the final parameters and moments."""
    sizes = B.adamw_sizes(count)
    ps = [cuda(p).requires_grad_(True) for p in B.adamw_params(sizes, scale, seed=count)]
    step_fn = make(ps)
    for step in range(B.ADAMW_STEPS):
        for p, g in zip(ps, R.grads_at(regime, sizes, step)):
            p.grad = None if g is None else cuda(g)
        step_fn()
    return ps


def _assert_same_run(opt_a, ps_a, opt_b, ps_b):
    for a, b in zip(ps_a, ps_b):
        assert same_bits(a, b)
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert same_bits(opt_a.state[a][k], opt_b.state[b][k]), k


def _run_opt(cls, regime="randn_decades", **kw):
    box = {}

    def make(ps):
        box["opt"] = cls(ps, **kw)
        return box["opt"].step
    ps = _trajectory_bits(make, regime)
    return box["opt"], ps


LR32 = float(np.float32(1e-3))


@pytest.mark.parametrize("max_grad_norm", (None, 1.0))
def test_adam_and_adamw_without_decay_are_the_same(max_grad_norm):
    from lipvq_vae_amd import optim
    a = _run_opt(optim.Adam, lr=1e-3, weight_decay=0.0, max_grad_norm=max_grad_norm)
    b = _run_opt(optim.AdamW, lr=1e-3, weight_decay=0.0, max_grad_norm=max_grad_norm)
    _assert_same_run(*a, *b)


@pytest.mark.parametrize("cls", ("Adam", "AdamW"))
@pytest.mark.parametrize("regime", ("randn_decades", "huge"))
def test_no_clipping_and_a_clip_that_never_binds_are_the_same(cls, regime):
    from lipvq_vae_amd import optim
    a = _run_opt(getattr(optim, cls), regime, lr=1e-3, weight_decay=1e-4)
    b = _run_opt(getattr(optim, cls), regime, lr=1e-3, weight_decay=1e-4, max_grad_norm=1e30)
    _assert_same_run(*a, *b)
    assert a[0].grad_stats is None and float(b[0].grad_stats[1]) == 1.0


@pytest.mark.parametrize("max_grad_norm", (None, 1.0))
@pytest.mark.parametrize("cls", ("Adam", "AdamW"))
def test_float_lr_and_device_lr_are_the_same(cls, max_grad_norm):
    from lipvq_vae_amd import optim
    a = _run_opt(getattr(optim, cls), lr=LR32, weight_decay=1e-2, max_grad_norm=max_grad_norm)
    b = _run_opt(getattr(optim, cls), lr=torch.tensor(LR32, dtype=torch.float32, device="cuda"), weight_decay=1e-2,
                 max_grad_norm=max_grad_norm)
    _assert_same_run(*a, *b)


def test_adamw_defaults_are_the_direct_library_call():
    from lipvq_vae_amd import _capi, ops, optim
    opt, ps = _run_opt(optim.AdamW, lr=1e-3, weight_decay=1e-4)
    sizes = B.adamw_sizes(33)
    qs = [cuda(p) for p in B.adamw_params(sizes, 1.0, seed=33)]
    m, v = [torch.zeros_like(q) for q in qs], [torch.zeros_like(q) for q in qs]
    steps = [torch.zeros((), device="cuda") for _ in qs]
    ws = torch.empty(_capi.lib.lipvq_adamw_workspace_bytes() // 4, device="cuda")
    for step in range(B.ADAMW_STEPS):
        grads = R.grads_at("randn_decades", sizes, step)
        live = [i for i, g in enumerate(grads) if g is not None]
        dev = {i: cuda(grads[i]) for i in live}
        for s in range(0, len(live), 32):
            idx = live[s:s + 32]
            arr = lambda ts: (C.c_void_p * len(idx))(*[t.data_ptr() for t in ts])
            rc = _capi.lib.lipvq_adamw_f32(arr([qs[i] for i in idx]), arr([dev[i] for i in idx]), arr([m[i] for i in idx]),
                                           arr([v[i] for i in idx]), arr([steps[i] for i in idx]),
                                           (C.c_int64 * len(idx))(*[sizes[i] for i in idx]), len(idx), 1e-3, 0.9, 0.999, 1e-8, 1e-4,
                                           ws.data_ptr(), ops._stream())
            assert rc == 0
    torch.cuda.synchronize()
    for i, p in enumerate(ps):
        assert same_bits(p, qs[i]) and same_bits(opt.state[p]["exp_avg"], m[i]) and same_bits(opt.state[p]["exp_avg_sq"], v[i])
        assert float(opt.state[p]["step"]) == float(steps[i])


# ---- the reference's function and the graphed step -------------------------------------------------------------------------------

class _Policy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from lipvq_vae_amd.gmm import GMMActionHead
        from lipvq_vae_amd.gpt import GPTBackbone
        self.backbone = GPTBackbone(64, 12, num_layers=1, num_heads=4, attn_dropout=0.0, block_output_dropout=0.0)
        self.head = GMMActionHead(64, 7, num_modes=3)

    def forward(self, x, actions):
        return self.head.nll(self.backbone(x), actions)


def _policy(seed=0):
    torch.manual_seed(seed)
    return _Policy().cuda()


def _batch(seed, B_=4):
    rng = B.rng_of(seed, 51)
    return cuda(rng.standard_normal((B_, 12, 64)).astype(np.float32)), cuda(rng.uniform(-1, 1, (B_, 12, 7)).astype(np.float32))


@pytest.mark.parametrize("ours", (True, False))
@pytest.mark.parametrize("max_grad_norm", (None, 0.01))
def test_backprop_for_loss_reports_the_reference_grad_norms(max_grad_norm, ours):
    from lipvq_vae_amd import optim
    net = _policy()
    x, act = _batch(1)
    opt = (optim.Adam if ours else torch.optim.Adam)(net.parameters(), lr=1e-3, weight_decay=1e-4)
    net(x, act).backward()
    raw = [p.grad.detach().clone() for p in net.parameters()]
    cpu = [torch.nn.Parameter(torch.zeros(g.shape)) for g in raw]                           # the reference's lines on the same gradients
    for c, g in zip(cpu, raw):
        c.grad = g.cpu()
    if max_grad_norm is not None:
        assert float(torch.nn.utils.clip_grad_norm_(cpu, max_grad_norm)) > 2 * max_grad_norm   # it clips
    want = 0.0
    for c in cpu:
        want += c.grad.data.norm(2).pow(2).item()
    start = [p.detach().clone() for p in net.parameters()]
    got = optim.backprop_for_loss(net, opt, net(x, act), max_grad_norm=max_grad_norm)
    assert isinstance(got, float) and abs(got - want) <= 1e-5 * want, (got, want)
    assert all(not torch.equal(p.detach(), s) for p, s in zip(net.parameters(), start))     # it stepped
    for p, g, c in zip(net.parameters(), raw, cpu):
        if ours:
            assert torch.allclose(p.grad, g, rtol=1e-4, atol=1e-7)                          # unclipped gradient kept
        else:
            assert torch.allclose(p.grad.cpu(), c.grad, rtol=1e-5, atol=1e-12)              # clipped in place
    if ours:
        assert opt.max_grad_norm is None
        dev = optim.backprop_for_loss(net, opt, net(x, act), max_grad_norm=max_grad_norm, sync=False)
        assert torch.is_tensor(dev) and dev.is_cuda and dev.dtype == torch.float64 and dev.dim() == 0


def test_graphed_policy_step_equals_eager_steps():
    from lipvq_vae_amd import optim
    from lipvq_vae_amd.icl import GraphedPolicyStep
    schedule = lambda i: min(1.0, (i + 1) / 4)
    runs = []
    for graphed in (False, True):
        net = _policy(3)
        params = list(net.parameters())
        opt = optim.Adam(params, lr=torch.tensor(1e-3, device="cuda"), weight_decay=1e-4, max_grad_norm=1.0)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, schedule)
        if graphed:
            start = [p.detach().clone() for p in params]
            lr0 = opt.param_groups[0]["lr"].clone()
            g = GraphedPolicyStep(net, params, opt, _batch(0), warmup=3)
            for p, s in zip(params, start):                                                 # construction trained nothing
                assert torch.equal(p.detach(), s)
                st = opt.state[p]
                assert float(st["step"]) == 0.0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
            assert torch.equal(opt.param_groups[0]["lr"], lr0)
            with pytest.raises(ValueError):
                g.step(_batch(1, B_=5)[0], _batch(1)[1])
        record = []
        for k in (1, 2, 3):
            x, act = _batch(k)
            if graphed:
                versions = [p._version for p in params]
                loss, stats = g.step(x, act)
                assert all(p._version > v for p, v in zip(params, versions))
            else:
                opt.zero_grad(set_to_none=True)
                loss = net(x, act)
                loss.backward()
                opt.step()
                stats = opt.grad_stats
            sched.step()
            record.append((loss.detach().clone(), stats.clone(), opt.param_groups[0]["lr"].clone()))
        runs.append((params, opt, record))
    (pa, oa, ra), (pb, ob, rb) = runs
    for (la, sa, lra), (lb, sb, lrb) in zip(ra, rb):
        assert torch.equal(la, lb) and torch.equal(sa, sb) and torch.equal(lra, lrb)
    assert not torch.equal(rb[0][1], rb[1][1])                                              # grad_stats is a live record
    assert not torch.equal(ra[0][2], ra[2][2])                                              # the schedule moved the lr
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(oa.state[a][k], ob.state[b][k]), k
        assert float(oa.state[a]["step"]) == 3.0


def test_graphed_policy_step_refusals():
    from lipvq_vae_amd import optim
    from lipvq_vae_amd.icl import GraphedPolicyStep
    net = _policy(4)
    with pytest.raises(TypeError):
        GraphedPolicyStep(net, net.parameters(), torch.optim.Adam(net.parameters(), capturable=True), _batch(0))
    opt = optim.Adam(net.parameters(), lr=1e-3)
    torch.optim.lr_scheduler.LambdaLR(opt, lambda i: 1.0)
    with pytest.raises(ValueError, match="float"):
        GraphedPolicyStep(net, net.parameters(), opt, _batch(0))
