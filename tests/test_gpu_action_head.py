"""GPU: the deterministic policy's output head (reference robomimic/models/policy_nets.py:1683-1731, obs_nets.py:747-771,
algo/icl.py:174-202) on the HIP library: csrc/lipvq_action_head.hip through ops.action_head / ops.action_head_bwd and
lipvq_vae_amd.action_head.ActionHead.

The yardstick is the plain-torch restatement tests/action_head_ref.py on ``.double()`` tensors (CPU).  Bounds (tests/test_gpu_gmm.py's):
a forward tensor or a loss within 1e-5 of the yardstick's maximum magnitude, a gradient within 1e-4 -- or 4 x the deviation of the
SAME restatement in fp32 (CPU) from float64 on the same inputs if that is larger.  Every figure is printed before it is asserted.
Nothing is compared with the code under test except where bit-equality between two runs of it is the property (repeatability, row
permutation, the fenced C ABI call against the ops wrapper, graph replay against eager, the product against ops.linear).
Inputs are drawn from seeds; nothing is read from tests/golden.

Shapes: rows 1 / 31 / 33 / 65 / 4097 (one live row, a ragged tile, one row in the second and third workgroup, 129 partial sums);
E = 4 / 64 / 260 / 512 / 1024 (one ragged K chunk, whole chunks, 8 chunks + 4, the limit); A = 1, 2, 3, 4 (the cosine term's
C = min(3, A) edges), 32, 33 (the second column tile: one full tile, one live column in wave 1's), 64 (the limit); dense rows and
the strided views [:, -T:] and [:, -1:] of a longer sequence.
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import action_head_ref as ref
import gpt_ref
from fenced import _Fenced

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL, REF_FACTOR = 1e-5, 1e-4, 4.0
FORWARD_KEYS = ("actions",) + ref.LOSS_KEYS
MIXED = (0.5, 2.0, 0.25)


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _head(E, A, seed=0):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.action_head import ActionHead
    torch.manual_seed(seed)
    return ActionHead(E, A)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def _t(x):
    return x.detach().cpu().double().numpy()


def _reference(sd, feats2, target, gl, weights, dtype):
    """The restatement in `dtype` on the CPU: actions, the four losses, and the gradients of sum_i gl[i] loss_i with respect to
    the pre-activations [N, A], the input and the two parameters."""
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    x = feats2.detach().to(dtype).requires_grad_(True)
    pre = ref.decoder(sd, x)
    pre.retain_grad()
    y = torch.tanh(pre)
    losses = ref.compute_losses(y, target.to(dtype), weights)
    sum(float(g) * losses[k] for g, k in zip(gl, ref.LOSS_KEYS)).backward()
    out = {"actions": y, "gpre": pre.grad, "gx": x.grad, "gW": sd[ref.KEYS[0]].grad, "gb": sd[ref.KEYS[1]].grad}
    out.update(losses)
    return {k: _t(v) for k, v in out.items()}


def _compare(tag, got, ref64, ref32):
    """Print every figure, then assert all of them."""
    bad = []
    for k, v in got.items():
        tol = FWD_TOL if k in FORWARD_KEYS else BWD_TOL
        e, dev = _rel(v, ref64[k]), _rel(ref32[k], ref64[k])
        bound = max(tol, REF_FACTOR * dev)
        print(f"{tag}: {k} error {e:.3e}, fp32 restatement's own {dev:.3e}, bound {bound:.3e}")
        if not e <= bound:
            bad.append((k, e, bound))
    assert not bad, bad


def _layout(feats2, layout, T):
    """feats [B, T, E] on the GPU holding the rows of feats2 [N, E]: dense, or the view [:, -T:] of a longer [B, L, E] tensor
    (L = 3 T, or 30 for the last-step view T = 1)."""
    N, E = feats2.shape
    B = N // T
    assert B * T == N
    if layout == "dense":
        return feats2.view(B, T, E).cuda()
    assert B > 1
    L = 3 * T if T > 1 else 30
    full = torch.randn(B, L, E, generator=torch.Generator().manual_seed(1))
    full[:, -T:] = feats2.view(B, T, E)
    view = full.cuda()[:, -T:]
    assert not view.is_contiguous()
    return view


def _inputs(N, E, A):
    gen = torch.Generator().manual_seed(7 * N + E + A)
    feats2 = torch.randn(N, E, generator=gen)
    target = torch.rand(N, A, generator=gen) * 6.0 - 3.0                           # +-3: both SmoothL1 branches
    gl = torch.randn(4, generator=gen)
    return feats2, target, gl


# rows, E, A, layout, T
CASES = [
    (1, 4, 1, "dense", 1),
    (31, 64, 12, "dense", 31),
    (33, 260, 7, "dense", 1),
    (80, 512, 12, "view", 10),
    (8, 512, 12, "view", 1),               # the last-step form out[:, -1:]
    (33, 1024, 64, "dense", 33),
    (4097, 64, 12, "dense", 1),
    (4097, 4, 2, "view", 1),               # C = 2
    (65, 64, 1, "dense", 65),
    (65, 64, 2, "dense", 1),
    (65, 64, 3, "view", 5),
    (65, 64, 4, "dense", 65),
    (65, 64, 32, "view", 5),
    (65, 64, 33, "dense", 1),
]


@pytest.mark.parametrize("N,E,A,layout,T", CASES)
def test_kernels_against_the_float64_restatement(ops, N, E, A, layout, T):
    from lipvq_vae_amd.action_head import _LossesFn
    head = _head(E, A, seed=N + E + A)
    feats2, target, gl = _inputs(N, E, A)
    sd = head.state_dict()
    head = head.cuda()
    W, b = head.nets["action"].weight, head.nets["action"].bias
    feats = _layout(feats2, layout, T).requires_grad_(True)
    B = N // T
    tg = target.cuda()
    one = torch.tensor([0.0, 0.0, 0.0, 1.0])
    # upstream gradients on all four losses at once; on action_loss alone with the default and with mixed weights
    for name, weights, g in (("all four", MIXED, gl), ("action_loss", ref.DEFAULT_WEIGHTS, one), ("action_loss", MIXED, one)):
        ref64 = _reference(sd, feats2, target, g, weights, torch.float64)
        ref32 = _reference(sd, feats2, target, g, weights, torch.float32)
        out = ops.action_head(feats.detach(), W, b, tg, weights, want_pre=True)
        # the product is lipvq_linear_act_f32's chain: the same bits
        assert torch.equal(out["pre"], ops.linear(feats.detach().reshape(N, E), W.detach(), b.detach()))
        got = {"actions": _t(out["actions"])}
        got.update({k: _t(out["losses"][i]) for i, k in enumerate(ref.LOSS_KEYS)})
        got["gpre"] = _t(ops.action_head_bwd(out["pre"], tg, g=g.cuda(), weights=weights))
        runs = []
        for _ in range(2):
            head.zero_grad(set_to_none=True)
            feats.grad = None
            if name == "all four":
                losses = _LossesFn.apply(feats, tg.view(B, T, A), W, b, weights)
                (losses * g.cuda()).sum().backward()
            else:
                named = head.losses(feats, tg.view(B, T, A), *weights)
                losses = torch.stack(list(named.values()))
                named["action_loss"].backward()
            runs.append([losses.detach().clone(), feats.grad.clone(), W.grad.clone(), b.grad.clone()])
        assert all(torch.equal(x, y) for x, y in zip(*runs)), "a second forward and backward gave other bits"
        assert torch.equal(runs[0][0], out["losses"])
        assert feats.grad.shape == feats.shape
        got["gx"], got["gW"], got["gb"] = _t(feats.grad).reshape(N, E), _t(W.grad), _t(b.grad)
        _compare(f"N={N} E={E} A={A} {layout} T={T} weights={weights} upstream={name}", got, ref64, ref32)


# ---------------------------------------------------------------------------------------------------
# edge values
# ---------------------------------------------------------------------------------------------------

def _edge(ops, pre, target, weights=MIXED, gl=(0.7, -1.3, 0.9, 1.1)):
    """Kernels and restatement on GIVEN pre-activations pre [N, A] (fp32) against target [N, A].  Rows are independent, so row n
    runs as its own call with E = 4, zero weights and bias = that row's pre-activations (exact), N = 1 in every mean: a huge value
    in one row cannot set the scale of another row's call.  Returns (got, ref64, ref32) with the rows stacked."""
    N, A = pre.shape
    g = torch.tensor(gl)
    rows = {k: [] for k in ("actions", "gpre") + ref.LOSS_KEYS}
    for n in range(N):
        bias = pre[n].float().cuda()
        out = ops.action_head(torch.ones(1, 1, 4, device="cuda"), torch.zeros(A, 4, device="cuda"), bias, target[n:n + 1].float().cuda(),
                              weights, want_pre=True)
        assert torch.equal(out["pre"].reshape(-1), bias)
        rows["actions"].append(out["actions"])
        rows["gpre"].append(ops.action_head_bwd(out["pre"], target[n:n + 1].float().cuda(), g=g.cuda(), weights=weights))
        for i, k in enumerate(ref.LOSS_KEYS):
            rows[k].append(out["losses"][i:i + 1])
    got = {k: _t(torch.cat(v, 0)) for k, v in rows.items()}
    refs = []
    for dtype in (torch.float64, torch.float32):
        r = {k: [] for k in rows}
        for n in range(N):
            p = pre[n:n + 1].float().to(dtype).requires_grad_(True)
            y = torch.tanh(p)
            losses = ref.compute_losses(y, target[n:n + 1].float().to(dtype), weights)
            sum(float(c) * losses[k] for c, k in zip(g, ref.LOSS_KEYS)).backward()
            r["actions"].append(y)
            r["gpre"].append(p.grad)
            for k in ref.LOSS_KEYS:
                r[k].append(losses[k].reshape(1))
        refs.append({k: _t(torch.cat(v, 0)) for k, v in r.items()})
    return got, refs[0], refs[1]


def _edge_inputs(seed, N=6, A=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, A, generator=g), torch.rand(N, A, generator=g) * 2.0 - 1.0


def test_edge_targets_outside_tanhs_range(ops):
    """Targets in +-3: |d| < 1 and |d| >= 1 both occur, in every row."""
    pre, target = _edge_inputs(1)
    target = target * 3.0
    got, r64, r32 = _edge(ops, pre, target)
    d = np.abs(r64["actions"] - target.double().numpy())
    assert ((d < 1).any(1) & (d > 1).any(1)).all()
    _compare("targets in +-3", got, r64, r32)


def test_edge_d_is_plus_or_minus_one(ops):
    """y = tanh(0) = 0 and target = -+1 in columns 3..: d = +-1 exactly, the point where SmoothL1's branches meet."""
    pre, target = _edge_inputs(2)
    pre[:, 3:] = 0.0
    target[:, 3:] = torch.tensor([1.0, -1.0, 1.0, -1.0])
    target[1::2, 3:] *= -1.0
    got, r64, r32 = _edge(ops, pre, target)
    assert (np.abs(r64["actions"][:, 3:] - target.double().numpy()[:, 3:]) == 1.0).all()
    assert (np.abs(got["actions"][:, 3:] - target.double().numpy()[:, 3:]) == 1.0).all()
    _compare("d = +-1", got, r64, r32)


def test_edge_saturated(ops):
    """pre = +-20: tanh is 1 in fp32 and the gradient through it is exactly zero (float64: 1 - tanh^2 = 1.7e-17)."""
    pre, target = _edge_inputs(3)
    pre[0], pre[1] = 20.0, -20.0
    pre[2, ::2], pre[3, 1::2] = 20.0, -20.0
    pre[4, :3], pre[5, 3:] = -20.0, 20.0
    got, r64, r32 = _edge(ops, pre, target)
    sat = (pre.abs() == 20.0).numpy()
    assert (np.abs(got["actions"][sat]) == 1.0).all() and (got["gpre"][sat] == 0.0).all()
    assert np.isfinite(got["gpre"]).all()
    _compare("pre = +-20", got, r64, r32)


def test_edge_zero_prediction_triple(ops):
    """pre = 0 on the first three columns: |y[:3]| = 0 <= 1e-8, the clamped-norm branch: d sim / d y_c = t_c / (1e-8 |t|), so the
    cosine term's gradient is of order 1e7 .. 1e8 (it sets this call's scale: the other columns are the other groups' business)."""
    pre, target = _edge_inputs(4)
    pre[:, :3] = 0.0
    got, r64, r32 = _edge(ops, pre, target)
    print("largest |gpre| per row", np.abs(r64["gpre"]).max(1))
    assert (np.abs(r64["gpre"][:, :3]).max(1) > 1e6).all() and np.isfinite(got["gpre"]).all()
    assert (r64["cos_loss"] == 1.0).all()
    _compare("pre = 0 on the first three columns", got, r64, r32)


def test_edge_zero_target_triple(ops):
    """target[:3] = 0: sim = 0 and the cosine term has no gradient."""
    pre, target = _edge_inputs(5)
    target[:, :3] = 0.0
    got, r64, r32 = _edge(ops, pre, target, weights=(0.0, 0.0, 1.0), gl=(0.0, 0.0, 1.0, 1.0))
    assert (r64["cos_loss"] == 1.0).all() and (got["cos_loss"] == 1.0).all()
    assert (r64["gpre"] == 0.0).all() and (got["gpre"] == 0.0).all()
    got, r64, r32 = _edge(ops, pre, target)
    _compare("zero target triple", got, r64, r32)


def test_edge_tiny_vectors_clamp_each_norm_on_its_own(ops):
    """p = t = (1e-5, 0, 0): each norm is 1e-5 > 1e-8, sim = 1 and cos_loss = 0 (clamping the product of the norms at 1e-8 would
    give sim = 0.01, cos_loss = 0.99).  Beside it: t = (0, 1e-5, 0) (sim 0) and p = -t (sim -1)."""
    A = 5
    pre, target = _edge_inputs(6, N=3, A=A)
    pre[:, :3] = torch.tensor([1e-5, 0.0, 0.0])
    target[:, :3] = torch.tensor([1e-5, 0.0, 0.0])
    target[1, :3] = torch.tensor([0.0, 1e-5, 0.0])
    pre[2, 0] = -1e-5
    got, r64, r32 = _edge(ops, pre, target)
    print("cos_loss", got["cos_loss"], "float64", r64["cos_loss"])
    assert r64["cos_loss"][0] == 0.0 and got["cos_loss"][0] == 0.0
    _compare("p = t = (1e-5, 0, 0)", got, r64, r32)


# ---------------------------------------------------------------------------------------------------
# rows do not see each other
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E,A", [(36, 3), (64, 12), (20, 33)])
def test_permuting_rows_permutes_the_outputs(ops, E, A):
    """A row's bits do not depend on its workgroup or on its slot in the 32-row tile (N stays the same: the means' 1 / N does)."""
    N = 65
    head = _head(E, A, seed=E + A).cuda()
    W, b = head.nets["action"].weight.detach(), head.nets["action"].bias.detach()
    feats2, target, gl = _inputs(N, E, A)
    feats2, target, gl = feats2.cuda(), target.cuda(), gl.cuda()
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).cuda()
    assert not torch.equal(perm, torch.arange(N).cuda())

    def run(x, t):
        out = ops.action_head(x, W, b, t, MIXED, want_pre=True)
        return out["actions"], out["pre"], ops.action_head_bwd(out["pre"], t, g=gl, weights=MIXED)

    whole, moved = run(feats2, target), run(feats2[perm].contiguous(), target[perm].contiguous())
    for k, a, m in zip(("actions", "pre", "gpre"), whole, moved):
        rows = (a[perm] != m).any(1).nonzero().flatten().tolist()
        assert not rows, f"{k}: rows {rows} of the permuted call differ"


# ---------------------------------------------------------------------------------------------------
# guard bands, through the C ABI
# ---------------------------------------------------------------------------------------------------

HEAD_ORDER = ("actions", "pre", "losses", "workspace")


@pytest.mark.parametrize("N", [1, 33, 65])
@pytest.mark.parametrize("E,A", [(4, 1), (36, 12), (64, 33)])
def test_the_head_writes_its_outputs_and_nothing_else(ops, E, A, N):
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    lib, check, stream = _capi.lib, _capi.check, lipvq_vae_amd.ops._stream
    head = _head(E, A, seed=N + A).cuda()
    W, b = head.nets["action"].weight.detach(), head.nets["action"].bias.detach()
    feats2, target, gl = _inputs(N, E, A)
    x, target, gl = feats2.cuda(), target.cuda(), gl.cuda()
    gy = torch.randn(N, A, generator=torch.Generator().manual_seed(3)).cuda()
    want = ops.action_head(x, W, b, target, MIXED, want_pre=True)
    nbytes = lib.lipvq_action_head_workspace_bytes(N)
    assert nbytes == 12 * ((N + 31) // 32)

    def outputs():
        return {"actions": _Fenced("actions", N, A, offset_words=1), "pre": _Fenced("pre", N, A, offset_words=1),
                "losses": _Fenced("losses", 4, offset_words=1),
                "workspace": _Fenced("workspace", nbytes // 4, offset_words=1)}     # exactly the bytes the library asks for

    def head_call(asked, with_target=True):
        f = outputs()
        ptrs = [f[k].ptr() if k in asked else None for k in HEAD_ORDER]
        check(lib.lipvq_action_head_f32(x.data_ptr(), N * E, W.data_ptr(), b.data_ptr(), target.data_ptr() if with_target else None, *ptrs,
                                        N, N, E, A, *MIXED, stream()), "lipvq_action_head_f32")
        torch.cuda.synchronize()
        for k in HEAD_ORDER:
            if k not in asked:
                assert f[k].untouched(), f"{k} was not asked for"
            elif k == "workspace":
                f[k].check()
            else:
                assert torch.equal(f[k].check().reshape(want[k].shape), want[k]), f"{k}: other bits than the ops wrapper's"

    head_call(HEAD_ORDER)                                                           # everything
    head_call(("actions",), with_target=False)                                     # the eval forward
    head_call(("losses", "workspace"))                                             # the losses alone
    head_call(("pre",))                                                            # a target without losses asked for: no sums

    for g, y in ((gl, None), (None, gy), (gl, gy)):
        gpre = _Fenced("gpre", N, A, offset_words=1)
        check(lib.lipvq_action_head_bwd_f32(want["pre"].data_ptr(), target.data_ptr(), None if g is None else g.data_ptr(),
                                            None if y is None else y.data_ptr(), gpre.ptr(), N, A, *MIXED, stream()), "lipvq_action_head_bwd_f32")
        torch.cuda.synchronize()
        assert torch.equal(gpre.check(), ops.action_head_bwd(want["pre"], target, g=g, gy=y, weights=MIXED))


def test_the_actions_gradient_mode(ops):
    """gpre = gy (1 - y^2), alone and added to the losses' gradient."""
    N, A = 33, 12
    gen = torch.Generator().manual_seed(8)
    pre, gy, target, gl = torch.randn(N, A, generator=gen), torch.randn(N, A, generator=gen), torch.rand(N, A, generator=gen), torch.randn(4, generator=gen)
    res = {}
    for dtype in (torch.float64, torch.float32):
        p = pre.to(dtype).requires_grad_(True)
        y = torch.tanh(p)
        (y * gy.to(dtype)).sum().backward()
        alone = p.grad.clone()
        p.grad = None
        y = torch.tanh(p)
        losses = ref.compute_losses(y, target.to(dtype), MIXED)
        ((y * gy.to(dtype)).sum() + sum(float(c) * losses[k] for c, k in zip(gl, ref.LOSS_KEYS))).backward()
        res[dtype] = {"gpre.gy": _t(alone), "gpre.both": _t(p.grad)}
    got = {"gpre.gy": _t(ops.action_head_bwd(pre.cuda(), gy=gy.cuda())),
           "gpre.both": _t(ops.action_head_bwd(pre.cuda(), target.cuda(), g=gl.cuda(), gy=gy.cuda(), weights=MIXED))}
    _compare("actions gradient", got, res[torch.float64], res[torch.float32])


# ---------------------------------------------------------------------------------------------------
# the sum
# ---------------------------------------------------------------------------------------------------

def test_the_sums_are_every_element_added_once(ops):
    """N = 4097: 129 partial sums per loss.  l2_loss / l1_loss against the float64 sum of the kernel's OWN fp32 per-element terms
    (from the returned actions: fp32 d = y - target, d^2 and smoothl1(d) as the kernel forms them), within 1e-5 relative.  One
    missing 32-row tile moves a sum by ~1/129 of it, the last tile's single row by ~1/4097."""
    N, E, A = 4097, 64, 12
    head = _head(E, A, seed=1).cuda()
    W, b = head.nets["action"].weight.detach(), head.nets["action"].bias.detach()
    feats2, target, _ = _inputs(N, E, A)
    out = ops.action_head(feats2.cuda().view(1, N, E), W, b, target.cuda(), MIXED)
    d = out["actions"] - target.cuda()                                              # fp32, the kernel's own subtraction
    sq = d * d
    sl = torch.where(d.abs() < 1.0, (0.5 * d) * d, d.abs() - 0.5)
    for i, (k, terms) in enumerate((("l2_loss", sq), ("l1_loss", sl))):
        want = float(terms.double().sum()) / (N * A)
        e = abs(float(out["losses"][i]) - want) / want
        print(f"{k}: kernel {float(out['losses'][i])!r} vs float64 sum of its own terms {want!r}: relative {e:.3e}")
        assert e <= 1e-5
    again = ops.action_head(feats2.cuda().view(1, N, E), W, b, target.cuda(), MIXED)
    assert torch.equal(out["losses"], again["losses"])


# ---------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def step():
    """The ICRT step shape: head, a [B, 3T, E] backbone-like output and targets."""
    B, T, E, A = 8, 10, 512, 12
    head = _head(E, A, seed=5)
    gen = torch.Generator().manual_seed(6)
    full = torch.randn(B, 3 * T, E, generator=gen)
    target = torch.rand(B, T, A, generator=gen) * 3.0 - 1.5
    return head, full, target, (B, T, E, A)


def test_losses_keys_order_and_the_last_step_form(step):
    head, full, target, (B, T, E, A) = step
    sd = head.state_dict()
    hc = _head(E, A, seed=5).cuda()
    out = hc.losses(full.cuda()[:, -T:], target.cuda())
    assert isinstance(out, OrderedDict) and tuple(out) == ("l2_loss", "l1_loss", "cos_loss", "action_loss")
    assert all(v.dim() == 0 and v.is_cuda and v.dtype == torch.float32 for v in out.values())
    assert torch.equal(out["action_loss"], out["l2_loss"])                          # the default weights 1 / 0 / 0
    # supervise_all_steps = False: the caller passes out[:, -1:] and target[:, None]
    last_target = target[:, -1]                                                     # [B, A]
    got = hc.losses(full.cuda()[:, -1:], last_target.cuda()[:, None], *MIXED)
    r = {}
    for dtype in (torch.float64, torch.float32):
        sdd = {k: v.to(dtype) for k, v in sd.items()}
        r[dtype] = {k: _t(v) for k, v in ref.head_losses(sdd, full[:, -1].to(dtype), last_target.to(dtype), MIXED).items()}
    _compare("last step", {k: _t(v) for k, v in got.items()}, r[torch.float64], r[torch.float32])
    with pytest.raises(ValueError, match="target"):
        hc.losses(full.cuda()[:, -1:], last_target.cuda())
    with pytest.raises(ValueError, match="feats"):
        hc(full.cuda()[:, :, :64])


def test_forward_has_autograd_and_replays_equal_eager(step):
    from lipvq_vae_amd.nnfn import GraphedEval
    head, full, target, (B, T, E, A) = step
    sd = head.state_dict()
    hc = _head(E, A, seed=5).cuda()
    gy = torch.randn(B, T, A, generator=torch.Generator().manual_seed(2))
    r = {}
    for dtype in (torch.float64, torch.float32):
        sdd = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
        x = full.detach().to(dtype).requires_grad_(True)           # (.detach(): for fp32 .to() returns the fixture's own tensor)
        y = ref.actions(sdd, x[:, -T:])
        (y * gy.to(dtype)).sum().backward()
        r[dtype] = {"actions": _t(y), "gx": _t(x.grad), "gW": _t(sdd[ref.KEYS[0]].grad), "gb": _t(sdd[ref.KEYS[1]].grad)}
    fg = full.cuda().requires_grad_(True)
    y = hc(fg[:, -T:])
    assert y.shape == (B, T, A)
    (y * gy.cuda()).sum().backward()
    assert float(fg.grad[:, :-T].abs().max()) == 0.0
    got = {"actions": _t(y), "gx": _t(fg.grad), "gW": _t(hc.nets["action"].weight.grad), "gb": _t(hc.nets["action"].bias.grad)}
    _compare("forward", got, r[torch.float64], r[torch.float32])
    hc.eval()
    feats = full.cuda()[:, -T:].contiguous()
    graphed = GraphedEval(hc, torch.zeros_like(feats))
    gen = torch.Generator().manual_seed(3)
    for i in range(3):
        x = feats if i == 0 else torch.randn(B, T, E, generator=gen).cuda()
        with torch.no_grad():
            assert torch.equal(graphed(x), hc(x)), f"replay {i}"
    with pytest.raises(ValueError):
        graphed(feats[:1])


def _chain(seed):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gpt import GPTBackbone
    torch.manual_seed(seed)
    net = GPTBackbone(64, 12, attn_dropout=0.0, block_output_dropout=0.0, num_layers=1, num_heads=4)
    return net, _head(64, 7, seed=seed + 1)


def test_backbone_feeds_the_head():
    """backbone -> head: action_loss's gradient reaches the backbone's first block."""
    B, L, H, T, A = 3, 12, 4, 4, 7
    net, head = _chain(31)
    gen = torch.Generator().manual_seed(33)
    x = torch.randn(B, L, 64, generator=gen)
    target = torch.rand(B, T, A, generator=gen) * 3.0 - 1.5
    r = {}
    for dtype in (torch.float64, torch.float32):
        params = dict(net.named_parameters())
        sd = {k: params[k].detach().to(dtype).requires_grad_(True) if k in params else v for k, v in net.state_dict().items()}
        hsd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in head.state_dict().items()}
        out = gpt_ref.gpt_forward(sd, x.to(dtype), 1, H)
        loss = ref.head_losses(hsd, out[:, -T:], target.to(dtype), MIXED)["action_loss"]
        loss.backward()
        r[dtype] = {"action_loss": _t(loss), "qkv": _t(sd["nets.transformer.0.nets.attention.nets.qkv.weight"].grad),
                    "head.weight": _t(hsd[ref.KEYS[0]].grad)}
    net, head = net.cuda().train(), head.cuda().train()
    loss = head.losses(net(x.cuda())[:, -T:], target.cuda(), *MIXED)["action_loss"]
    loss.backward()
    got = {"action_loss": _t(loss), "qkv": _t(net.nets["transformer"][0].nets["attention"].nets["qkv"].weight.grad),
           "head.weight": _t(head.nets["action"].weight.grad)}
    _compare("chain", got, r[torch.float64], r[torch.float32])


def test_prompted_policy_equals_the_uncached_chain():
    from lipvq_vae_amd.embedding import ICLInputEmbedding
    from lipvq_vae_amd.gpt import GPTBackbone
    from lipvq_vae_amd.icl import PromptedPolicy
    T, E, DIN, A, B = 3, 64, 16, 7, 5
    torch.manual_seed(21)
    emb = ICLInputEmbedding(DIN, E, T, emb_dropout=0.1).cuda().eval()
    net = GPTBackbone(E, 3 * T, num_layers=2, num_heads=4).cuda().eval()
    head = _head(E, A, seed=22).cuda().eval()
    g = torch.Generator().manual_seed(23)
    obs, ctx_obs, ctx_act = (torch.randn(B, T, DIN, generator=g).cuda() for _ in range(3))
    policy = PromptedPolicy(emb, net, head)
    policy.set_prompt(ctx_obs, ctx_act)
    with torch.no_grad():
        want = head(net(emb(obs, ctx_obs, context_actions=ctx_act))[:, 2 * T:])
    got = policy(obs)
    assert got.shape == (B, T, A) and torch.equal(got, want)
    assert 0.0 < float(got.detach().abs().max()) <= 1.0


def test_graphed_policy_step_equals_eager_steps():
    """zero_grad -> backbone -> head.losses()["action_loss"] -> backward -> Adam with clipping and a device lr, captured: replay k
    equals eager step k bit for bit, in parameters and loss."""
    from lipvq_vae_amd import optim
    from lipvq_vae_amd.icl import GraphedPolicyStep
    B, L, T, A = 4, 12, 4, 7

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(B, L, 64, generator=g).cuda(), (torch.rand(B, T, A, generator=g) * 3.0 - 1.5).cuda()

    runs = []
    for graphed in (False, True):
        net, head = _chain(41)
        net, head = net.cuda().train(), head.cuda().train()
        params = list(net.parameters()) + list(head.parameters())
        opt = optim.Adam(params, lr=torch.tensor(1e-3, device="cuda"), max_grad_norm=1.0)
        loss_fn = lambda x, a: head.losses(net(x)[:, -T:], a, *MIXED)["action_loss"]      # noqa: E731
        if graphed:
            start = [p.detach().clone() for p in params]
            step = GraphedPolicyStep(loss_fn, params, opt, batch(0), warmup=3)
            assert all(torch.equal(p.detach(), s) for p, s in zip(params, start))           # construction trained nothing
        record = []
        for k in (1, 2, 3):
            x, a = batch(k)
            if graphed:
                loss, _ = step.step(x, a)
            else:
                opt.zero_grad(set_to_none=True)
                loss = loss_fn(x, a)
                loss.backward()
                opt.step()
            record.append([loss.detach().clone()] + [p.detach().clone() for p in params])
        runs.append(record)
    for k, (eager, replay) in enumerate(zip(*runs), 1):
        assert all(torch.equal(a, b) for a, b in zip(eager, replay)), f"replay {k} differs from eager step {k}"
    assert not torch.equal(runs[0][0][-1], runs[0][2][-1])                                  # the head's bias moved
