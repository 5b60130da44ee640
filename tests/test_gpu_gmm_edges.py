"""GPU: the GMM head's kernels (csrc/lipvq_gmm.hip) at the shapes and on the code paths tests/test_gpu_gmm.py does not reach: every
forward variant at its tile edges, row independence, guard bands around every output, the sum's own rounding bound, the backward
paths that never ran, and the sampler epilogue beyond one shape.

The yardstick is tests/test_gpu_gmm.py's: tests/gmm_ref.py on ``.double()`` CPU tensors built from the same fp32 inputs.  A forward
tensor is held to max(1e-5, 4 x dev) of the yardstick's largest magnitude, a gradient to max(1e-4, 4 x dev), dev = the deviation
of the same restatement in fp32 on the CPU.  Every figure is printed, then all are asserted.  Nothing is compared with the code
under test except where bit-equality between two runs of it is the property (row independence, repeatability, the fenced C ABI
call against the ops wrapper, the product against ops.linear on the stacked parameters).

Which kernel a case reaches, from gmm_launch's rule (P = M (2 A + 1), tiles = ceil(P / 32), nt = ceil(tiles / 4); NT = 1 | 2 | 4 for
nt = 1 | 2 | 3..4; KC = 32 for NT <= 2, 16 for NT = 4; staging = (32 + 128 NT)(KC + 1) floats, tile = 32 (P | 1) floats):

  (M, A)   P    kernel   what the shape reaches
  (16, 1)   48  <1, 32>  M at its limit, A = 1: two tiles, waves 2 and 3 idle, seven of the sampler's eight parts idle
  (1, 63)  127  <1, 32>  the last tile one column short of full; M = 1: no CDF boundary, one-term logsumexp
  (3, 21)  129  <2, 32>  the fifth tile (wave 0, j = 1) has ONE live column; tile_ok false for j = 1 on waves 1..3
  (5, 16)  165  <2, 32>  interior of NT = 2 (six tiles); the strided [:, -T:] view with T = 5
  (5, 25)  255  <2, 32>  eight full tiles but for one column: every (wave, j) is live
  (7, 18)  259  <4, 16>  nine tiles, tile_ok false for j >= 1 on waves 1..3 and j >= 3 on wave 0; staging 9248 > tile 8288 floats,
                         so the side arrays sit at side_off = staging (P = 257 .. 290)
  (3, 64)  387  <4, 16>  A at its limit: 64-trip mode loops, the sampler's eight trips
  (7, 36)  511  <4, 16>  the largest P: the last column of tile 15, LDS 69 888 bytes (forward) / 69 760 (backward) > 64 KiB: reserved
  E: 4, 36, 60 = ragged last chunk of KC = 32 (kend = 2, 2, 14); 12, 20, 260 = ragged last chunk of KC = 16 (kend = 6, 2, 2);
     8, 16, 32, 64, 1024 = whole chunks; 260 with KC = 32 = eight whole chunks and kend = 2.
  N: 1 (one live row), 31, 32, 33 (one row in the second workgroup), 65 (one row in the third); 8225 = 258 partial sums (the sum
     kernel's second trip); 2200 x 496 elements = more than 4096 x 256 (gmm_params_bwd_kernel's second grid-stride trip).

What these tests found when they were written: no miss.  Largest error / bound on an MI355X: forward tensors 0.16 (logits, NT = 2),
gradients 0.08, the sum against its derived rounding bound 0.061, the near-mode low-noise class 0.30 (its figures are in
test_low_noise_near_a_mode's docstring).  Seven wrong-value variants of the kernels (the sum kernel and gmm_params_bwd_kernel
without their second trip, the ragged K chunk one step short, gsum ignored when g is given, NT = 2's partial tile skipped, the
sampler's loop cut to one trip, one wrong operand in column 510 of P = 511) each failed between 1 and 34 of these tests;
tests/test_gpu_gmm.py noticed two of the seven.
"""
import numpy as np
import pytest
import torch

import gmm_ref
from fenced import PAD, SENTINEL, _Fenced  # noqa: F401

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL, REF_FACTOR = 1e-5, 1e-4, 4.0
MODES = {"softplus": 0, "exp": 1, "low_noise": 2}
FORWARD_KEYS = ("log_prob", "mean", "scale", "logits", "sample", "sum")
MIN_STD = 0.01


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _nt(M, A):
    """gmm_launch's rule: column tiles per wave."""
    nt = ((M * (2 * A + 1) + 31) // 32 + 3) // 4
    return 1 if nt <= 1 else (2 if nt <= 2 else 4)


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


def _grad(t):
    return torch.zeros_like(t) if t.grad is None else t.grad


def _reference(sd, feats, actions, g, c, M, A, act, dtype):
    """The restatement in `dtype` on the CPU: log_prob, activated mean / scale, raw logits, and the gradients of
    sum(g log_prob) + c sum(log_prob) with respect to the pre-activations [N, P], the input and the six parameters."""
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    x = feats.detach().to(dtype).requires_grad_(True)
    pm, ps, lg = gmm_ref.decoder(sd, x, M, A)
    for t in (pm, ps, lg):
        t.retain_grad()
    low = act == "low_noise"
    mu, sg = gmm_ref.activate(pm, ps, MIN_STD, "softplus" if low else act, low_noise=low)
    lp = gmm_ref.mixture(mu, sg, lg).log_prob(actions.to(dtype))
    ((lp * g.to(dtype)).sum() + c * lp.sum()).backward()
    N = x.shape[0]
    out = {"log_prob": lp, "mean": mu, "scale": sg, "logits": lg, "gx": x.grad, "sum": lp.sum(),
           "gpre": torch.cat((_grad(pm).reshape(N, -1), _grad(ps).reshape(N, -1), _grad(lg).reshape(N, -1)), 1)}
    out.update({"g:" + k: _grad(v) for k, v in sd.items()})
    return {k: _t(v) for k, v in out.items()}


def _compare(tag, got, ref64, ref32):
    """Print every figure, then assert all of them."""
    bad = []
    for k, v in got.items():
        tol = FWD_TOL if k.split(".")[0] in FORWARD_KEYS else BWD_TOL
        e, dev = _rel(v, ref64[k]), _rel(ref32[k], ref64[k])
        bound = max(tol, REF_FACTOR * dev)
        print(f"{tag}: {k} error {e:.3e}, fp32 restatement's own {dev:.3e}, bound {bound:.3e}")
        if not e <= bound:
            bad.append((k, e, bound))
    assert not bad, bad


def _sum_rounding(tag, s, log_prob):
    """The kernel's own worst case: a partial is a sequential fp32 sum of at most 32 terms, the partials are added in float64
    and rounded once: |sum - sum_n lp[n]| <= 32 2^-24 sum_n |lp[n]|, both sides in float64 from the kernel's fp32 log_prob."""
    lp = log_prob.detach().cpu().double()
    err, bound = abs(float(s) - float(lp.sum())), 32.0 * 2.0 ** -24 * float(lp.abs().sum())
    print(f"{tag}: sum {float(s)!r} vs its rows' {float(lp.sum())!r}: off by {err:.3e}, rounding bound {bound:.3e}, ratio {err / bound:.3e}")
    return err, bound


def _layout(feats2, layout, T):
    """feats [B, T, E] on the GPU holding the rows of feats2 [N, E]: dense, or the view [:, -T:] of a [B, 3T, E] tensor."""
    N, E = feats2.shape
    B = N // T
    assert B * T == N
    if layout == "dense":
        return feats2.view(B, T, E).cuda()
    assert B > 1 and T > 1                                                          # so that n / T matters
    full = torch.randn(B, 3 * T, E, generator=torch.Generator().manual_seed(1))
    full[:, -T:] = feats2.view(B, T, E)
    view = full.cuda()[:, -T:]
    assert not view.is_contiguous()
    return view


def _stacked(ops, feats, params, N, E):
    """lipvq_linear_act_f32 on the concatenated parameters: the documented bit-identity of the head's product."""
    return ops.linear(feats.detach().reshape(N, E), torch.cat(params[0::2], 0), torch.cat(params[1::2], 0))


# ---------------------------------------------------------------------------------------------------
# 1. every variant, at its edges
# ---------------------------------------------------------------------------------------------------

# rows, E, (M, A), std_activation, layout, T
CASES = [
    (33, 36, 1, 63, "softplus", "dense", 1),          # <1, 32> P = 127
    (33, 64, 1, 63, "exp", "dense", 33),
    (65, 8, 16, 1, "exp", "dense", 65),               # <1, 32> P = 48
    (1, 4, 3, 21, "softplus", "dense", 1),            # <2, 32> P = 129
    (31, 36, 3, 21, "exp", "dense", 31),
    (32, 60, 3, 21, "softplus", "dense", 1),
    (33, 64, 3, 21, "exp", "dense", 33),
    (65, 36, 3, 21, "softplus", "dense", 1),
    (65, 260, 5, 16, "exp", "view", 5),               # <2, 32> P = 165
    (33, 32, 5, 25, "softplus", "dense", 1),          # <2, 32> P = 255
    (33, 1024, 5, 25, "exp", "dense", 33),
    (1, 12, 7, 18, "softplus", "dense", 1),           # <4, 16> P = 259
    (33, 16, 7, 18, "exp", "dense", 33),
    (65, 20, 7, 18, "softplus", "dense", 1),
    (33, 260, 7, 18, "exp", "dense", 1),
    (33, 20, 3, 64, "softplus", "view", 3),           # <4, 16> P = 387
    (31, 20, 7, 36, "exp", "dense", 31),              # <4, 16> P = 511
    (65, 1024, 7, 36, "softplus", "dense", 1),
]


@pytest.mark.parametrize("N,E,M,A,act,layout,T", CASES)
def test_every_variant_against_the_float64_restatement(ops, N, E, M, A, act, layout, T):
    from lipvq_vae_amd.gmm import _LogProbFn
    head = _head(E, A, M, seed=N + E + M)
    gen = torch.Generator().manual_seed(7 * N + E + A)
    feats2 = torch.randn(N, E, generator=gen)
    actions = torch.rand(N, A, generator=gen) * 3.0 - 1.5                          # partly outside tanh's range
    g = torch.randn(N, generator=gen)
    sd = head.state_dict()
    ref64 = _reference(sd, feats2, actions, g, 0.0, M, A, act, torch.float64)
    ref32 = _reference(sd, feats2, actions, g, 0.0, M, A, act, torch.float32)
    head = head.cuda()
    params = head._params()
    feats = _layout(feats2, layout, T).requires_grad_(True)
    ac = actions.cuda()
    out = ops.gmm_head(feats.detach(), params, M, A, ac, MODES[act], MIN_STD, want_pre=True, want_params=True, want_sum=True)
    got = {k: _t(out[k]).reshape(ref64[k].shape) for k in ("log_prob", "mean", "scale", "logits", "sum")}
    assert torch.equal(out["pre"], _stacked(ops, feats, params, N, E))             # the same bits as the Linear on the stacked parameters
    got["gpre"] = _t(ops.gmm_head_bwd(out["pre"], ac, g.cuda(), None, M, A, MODES[act], MIN_STD))
    lp = _LogProbFn.apply(feats, ac.view(feats.shape[0], feats.shape[1], A), *params, M, A, MODES[act], MIN_STD, False)[0]
    assert torch.equal(lp.reshape(-1), out["log_prob"])
    (lp.reshape(-1) * g.cuda()).sum().backward()
    assert feats.grad.shape == feats.shape
    got["gx"] = _t(feats.grad).reshape(N, E)
    for k, p in zip(gmm_ref.KEYS, params):
        got["g:" + k] = _t(p.grad)
    tag = f"NT={_nt(M, A)} N={N} E={E} M={M} A={A} {act} {layout} T={T}"
    err, bound = _sum_rounding(tag, out["sum"], out["log_prob"])
    _compare(tag, got, ref64, ref32)
    assert err <= bound


# ---------------------------------------------------------------------------------------------------
# 2. rows do not see each other
# ---------------------------------------------------------------------------------------------------

def _all_outputs(ops, feats2, params, actions, g, M, A, mode):
    out = ops.gmm_head(feats2, params, M, A, actions, mode, MIN_STD, want_pre=True, want_params=True, want_sum=True)
    out["gpre"] = ops.gmm_head_bwd(out["pre"], actions, g, None, M, A, mode, MIN_STD)
    return out


ROW_KEYS = ("log_prob", "pre", "mean", "scale", "logits", "gpre")


@pytest.mark.parametrize("E,M,A,act", [(36, 1, 63, "exp"), (36, 3, 21, "softplus"), (20, 7, 18, "exp"), (20, 7, 36, "softplus")])
def test_rows_do_not_see_each_other(ops, E, M, A, act):
    """A row's bits do not depend on the other rows of its call, on its workgroup or on its slot in the 32-row tile."""
    N = 65
    head = _head(E, A, M, seed=E + M).cuda()
    params = head._params()
    gen = torch.Generator().manual_seed(100 + E + A)
    feats2 = torch.randn(N, E, generator=gen).cuda()
    actions = (torch.rand(N, A, generator=gen) * 3.0 - 1.5).cuda()
    g = torch.randn(N, generator=gen).cuda()
    whole = _all_outputs(ops, feats2, params, actions, g, M, A, MODES[act])
    again = _all_outputs(ops, feats2, params, actions, g, M, A, MODES[act])
    for k in ROW_KEYS + ("sum",):
        assert torch.equal(whole[k], again[k]), f"{k}: a second call gave other bits"
    # rows 32..64 alone; rows 0..32 (one row in the second workgroup); rows 1..64 (every row one slot earlier)
    for lo, hi in ((32, 65), (0, 33), (1, 65)):
        part = _all_outputs(ops, feats2[lo:hi], params, actions[lo:hi], g[lo:hi], M, A, MODES[act])
        for k in ROW_KEYS:
            assert part[k].shape[0] == hi - lo
            rows = (part[k] != whole[k][lo:hi]).reshape(hi - lo, -1).any(1).nonzero().flatten().tolist()
            assert not rows, f"NT={_nt(M, A)} {k}: rows {[lo + r for r in rows]} of the {N}-row call differ from the call on rows {lo}..{hi - 1}"


# ---------------------------------------------------------------------------------------------------
# 3. guard bands, through the C ABI
# ---------------------------------------------------------------------------------------------------

def _capi():
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    return _capi.lib, _capi.check, lipvq_vae_amd.ops._stream


def _head_outputs(N, M, A, lib):
    P = M * (2 * A + 1)
    nbytes = lib.lipvq_gmm_workspace_bytes(N)
    assert nbytes == 4 * ((N + 31) // 32)
    return {"log_prob": _Fenced("log_prob", N, offset_words=1), "pre": _Fenced("pre", N, P, offset_words=1),
            "mean": _Fenced("mean", N, M, A, offset_words=1), "scale": _Fenced("scale", N, M, A, offset_words=1),
            "logits": _Fenced("logits", N, M, offset_words=1), "sum": _Fenced("lp_sum", 1, offset_words=1),
            "workspace": _Fenced("workspace", nbytes // 4, offset_words=1)}         # exactly the bytes the library asks for


HEAD_ORDER = ("log_prob", "pre", "mean", "scale", "logits", "sum", "workspace")


@pytest.mark.parametrize("N", [1, 33, 65])
@pytest.mark.parametrize("E,M,A,act", [(8, 16, 1, "softplus"), (4, 3, 21, "exp"), (12, 7, 18, "softplus"), (20, 7, 36, "exp")])
def test_the_head_writes_its_outputs_and_nothing_else(ops, E, M, A, act, N):
    lib, check, stream = _capi()
    mode, P = MODES[act], M * (2 * A + 1)
    head = _head(E, A, M, seed=N + M).cuda()
    params = head._params()
    gen = torch.Generator().manual_seed(200 + N + A)
    x = torch.randn(N, E, generator=gen).cuda()
    actions = (torch.rand(N, A, generator=gen) * 3.0 - 1.5).cuda()
    u, eps = torch.rand(N, generator=gen).cuda(), torch.randn(N, A, generator=gen).cuda()
    g, gsum = torch.randn(N, generator=gen).cuda(), torch.full((), -1.0 / N).cuda()
    gmean, gscale, glogits = (torch.randn(N, n, generator=gen).cuda() for n in (M * A, M * A, M))
    pp = [p.data_ptr() for p in params]
    want = ops.gmm_head(x, params, M, A, actions, mode, MIN_STD, want_pre=True, want_params=True, want_sum=True)

    def head_call(f, asked, with_actions=True):
        ptrs = [f[k].ptr() if k in asked else None for k in HEAD_ORDER]
        check(lib.lipvq_gmm_head_f32(x.data_ptr(), N * E, *pp, actions.data_ptr() if with_actions else None, *ptrs, N, N, E, M, A, mode,
                                     MIN_STD, stream()), "lipvq_gmm_head_f32")
        torch.cuda.synchronize()
        for k in HEAD_ORDER:
            if k not in asked:
                assert f[k].untouched(), f"{k} was not asked for"
            elif k == "workspace":
                f[k].check()
            else:
                assert torch.equal(f[k].check().reshape(want[k].shape), want[k]), f"{k}: other bits than the ops wrapper's"

    head_call(_head_outputs(N, M, A, lib), HEAD_ORDER)                             # everything
    head_call(_head_outputs(N, M, A, lib), ("log_prob",))                          # log_prob alone: no partial sums either
    head_call(_head_outputs(N, M, A, lib), ("sum", "workspace"))                   # the sum alone
    head_call(_head_outputs(N, M, A, lib), ("pre", "mean", "scale", "logits"), with_actions=False)

    action = _Fenced("action", N, A, offset_words=1)
    check(lib.lipvq_gmm_sample_f32(x.data_ptr(), N * E, *pp, u.data_ptr(), eps.data_ptr(), action.ptr(), N, N, E, M, A, mode, MIN_STD, stream()),
          "lipvq_gmm_sample_f32")
    torch.cuda.synchronize()
    assert torch.equal(action.check(), ops.gmm_sample(x, params, M, A, u, eps, mode, MIN_STD))

    for gg, gs in ((g, None), (None, gsum), (g, gsum)):
        gpre = _Fenced("gpre", N, P, offset_words=1)
        check(lib.lipvq_gmm_head_bwd_f32(want["pre"].data_ptr(), actions.data_ptr(), None if gg is None else gg.data_ptr(),
                                         None if gs is None else gs.data_ptr(), gpre.ptr(), N, M, A, mode, MIN_STD, stream()), "lipvq_gmm_head_bwd_f32")
        torch.cuda.synchronize()
        assert torch.equal(gpre.check(), ops.gmm_head_bwd(want["pre"], actions, gg, gs, M, A, mode, MIN_STD))

    gpre = _Fenced("gpre", N, P, offset_words=1)
    check(lib.lipvq_gmm_params_bwd_f32(want["pre"].data_ptr(), gmean.data_ptr(), gscale.data_ptr(), glogits.data_ptr(), gpre.ptr(), N, M, A, mode,
                                       stream()), "lipvq_gmm_params_bwd_f32")
    torch.cuda.synchronize()
    assert torch.equal(gpre.check(), ops.gmm_params_bwd(want["pre"], gmean, gscale, glogits, M, A, mode))


# ---------------------------------------------------------------------------------------------------
# 4. the sum
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,E,M,A", [(8225, 4, 1, 1), (8225, 4, 3, 21), (65, 20, 7, 36)])
def test_the_sum_is_every_tile_added_once(ops, N, E, M, A):
    """8225 = 32 x 257 + 1 rows are 258 partial sums: thread 0 and 1 of gmm_sum_kernel take a second trip.  One missing tile
    moves the sum by ~1/258 of it, 2000 x the rounding bound; the last tile's single row by ~1/8225, 60 x the bound."""
    head = _head(E, A, M, seed=N + A)
    gen = torch.Generator().manual_seed(300 + N + A)
    feats2 = torch.randn(N, E, generator=gen)
    actions = torch.rand(N, A, generator=gen) * 3.0 - 1.5
    sd = head.state_dict()
    lp = {}
    for dtype in (torch.float64, torch.float32):
        sdd = {k: v.to(dtype) for k, v in sd.items()}
        lp[dtype] = _t(gmm_ref.gmm_log_prob(sdd, feats2.to(dtype), actions.to(dtype), M, A, MIN_STD))
    # the input condition: every tile carries a share of the same order (mean |lp| per live row, so the ragged tile counts)
    tiles = [np.abs(lp[torch.float64][i:i + 32]).mean() for i in range(0, N, 32)]
    print(f"N={N} M={M} A={A}: {len(tiles)} tiles, mean |log_prob| per row between {min(tiles):.3e} and {max(tiles):.3e}")
    assert max(tiles) <= 10.0 * min(tiles)
    head = head.cuda()
    out = ops.gmm_head(feats2.cuda().view(1, N, E), head._params(), M, A, actions.cuda(), 0, MIN_STD, want_sum=True)
    tag = f"NT={_nt(M, A)} N={N} E={E} M={M} A={A} sum"
    err, bound = _sum_rounding(tag, out["sum"], out["log_prob"])
    got = {"log_prob": _t(out["log_prob"]), "sum": _t(out["sum"])}
    ref64, ref32 = ({"log_prob": lp[d], "sum": lp[d].sum()} for d in (torch.float64, torch.float32))
    _compare(tag, got, ref64, ref32)
    assert err <= bound
    assert torch.equal(out["sum"], ops.gmm_head(feats2.cuda().view(1, N, E), head._params(), M, A, actions.cuda(), 0, MIN_STD, want_sum=True)["sum"])


# ---------------------------------------------------------------------------------------------------
# 5. backward paths that never ran
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E,M,A,act", [(36, 1, 63, "softplus"), (36, 3, 21, "exp"), (20, 7, 18, "softplus"), (20, 7, 36, "exp")])
def test_backward_with_the_rows_and_the_sums_gradient_together(ops, E, M, A, act):
    """gpre of sum(g log_prob) + c sum(log_prob), g = randn, c = -1 / N: gmm_head_bwd_kernel adds gsum[0] to every row's g."""
    N = 33
    head = _head(E, A, M, seed=E + A)
    gen = torch.Generator().manual_seed(400 + E + A)
    feats2 = torch.randn(N, E, generator=gen)
    actions = torch.rand(N, A, generator=gen) * 3.0 - 1.5
    g, c = torch.randn(N, generator=gen), -1.0 / N
    sd = head.state_dict()
    ref64 = _reference(sd, feats2, actions, g, c, M, A, act, torch.float64)
    ref32 = _reference(sd, feats2, actions, g, c, M, A, act, torch.float32)
    head = head.cuda()
    out = ops.gmm_head(feats2.cuda(), head._params(), M, A, actions.cuda(), MODES[act], MIN_STD, want_pre=True)
    gsum = torch.full((), c, dtype=torch.float32).cuda()
    got = {"gpre": _t(ops.gmm_head_bwd(out["pre"], actions.cuda(), g.cuda(), gsum, M, A, MODES[act], MIN_STD))}
    _compare(f"NT={_nt(M, A)} N={N} E={E} M={M} A={A} {act} g+gsum", got, ref64, ref32)


def _params_bwd_case(N, M, A, seed):
    gen = torch.Generator().manual_seed(seed)
    MA = M * A
    pre = torch.randn(N, 2 * MA + M, generator=gen)
    pre[:, MA:2 * MA] = torch.rand(N, MA, generator=gen) * 37.0 - 12.0               # [-12, 25]: both sides of softplus's 20
    grads = {"mean": torch.randn(N, MA, generator=gen), "scale": torch.randn(N, MA, generator=gen), "logits": torch.randn(N, M, generator=gen)}
    return pre, grads


def _params_bwd_reference(pre, grads, subset, M, A, act, dtype):
    """Autograd through gmm_ref.activate: the gradient of sum(gmean mu) + sum(gscale sigma) + sum(glogits logits) over `subset`."""
    N, MA = pre.shape[0], M * A
    p = pre.to(dtype).requires_grad_(True)
    low = act == "low_noise"
    mu, sg = gmm_ref.activate(p[:, :MA], p[:, MA:2 * MA], MIN_STD, "softplus" if low else act, low_noise=low)
    outs = {"mean": mu, "scale": sg, "logits": p[:, 2 * MA:]}
    (sum((outs[k] * grads[k].to(dtype)).sum() for k in subset) + 0.0 * p.sum()).backward()      # (low noise: sigma is a constant)
    gp = _t(p.grad)
    return {"gpre.mean": gp[:, :MA], "gpre.scale": gp[:, MA:2 * MA], "gpre.logits": gp[:, 2 * MA:]}


def _params_bwd_check(ops, tag, pre, grads, subset, M, A, act):
    MA = M * A
    ref64 = _params_bwd_reference(pre, grads, subset, M, A, act, torch.float64)
    ref32 = _params_bwd_reference(pre, grads, subset, M, A, act, torch.float32)
    given = [grads[k].cuda() if k in subset else None for k in ("mean", "scale", "logits")]
    gp = ops.gmm_params_bwd(pre.cuda(), *given, M, A, MODES[act])
    assert torch.equal(gp, ops.gmm_params_bwd(pre.cuda(), *given, M, A, MODES[act]))
    gp = _t(gp)
    got = {"gpre.mean": gp[:, :MA], "gpre.scale": gp[:, MA:2 * MA], "gpre.logits": gp[:, 2 * MA:]}
    for k in ("mean", "scale", "logits"):
        if k not in subset or (k == "scale" and act == "low_noise"):
            assert (got["gpre." + k] == 0).all(), f"{tag}: the {k} columns have no gradient and must be exactly 0"
            assert (ref64["gpre." + k] == 0).all()
    _compare(tag, got, ref64, ref32)


SUBSETS = [("mean",), ("scale",), ("logits",), ("mean", "scale"), ("mean", "logits"), ("scale", "logits"), ("mean", "scale", "logits")]


@pytest.mark.parametrize("act", ["softplus", "exp"])
@pytest.mark.parametrize("subset", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_params_backward_subsets(ops, subset, act):
    N, M, A = 33, 5, 12
    pre, grads = _params_bwd_case(N, M, A, 500)
    assert float(pre[:, M * A:2 * M * A].max()) > 20.0 > 0.0 > float(pre[:, M * A:2 * M * A].min())
    _params_bwd_check(ops, f"params_bwd N={N} M={M} A={A} {act} {'+'.join(subset)}", pre, grads, subset, M, A, act)


def test_params_backward_low_noise(ops):
    N, M, A = 33, 5, 12
    pre, grads = _params_bwd_case(N, M, A, 501)
    _params_bwd_check(ops, f"params_bwd N={N} M={M} A={A} low_noise", pre, grads, SUBSETS[-1], M, A, "low_noise")


def test_params_backward_grid_stride_second_trip(ops):
    """2200 x 496 = 1 091 200 elements > 4096 x 256: the elements past 1 048 576 are the grid-stride loop's second trip."""
    N, M, A = 2200, 16, 15
    assert N * M * (2 * A + 1) > 4096 * 256
    pre, grads = _params_bwd_case(N, M, A, 502)
    _params_bwd_check(ops, f"params_bwd N={N} M={M} A={A} softplus", pre, grads, SUBSETS[-1], M, A, "softplus")


@pytest.mark.parametrize("E,M,A", [(36, 1, 63), (36, 3, 21), (20, 7, 18)])
def test_low_noise_log_prob_and_its_backward(ops, E, M, A):
    """sigma = 1e-4: l ~ -1e8 A, well conditioned in relative terms for actions that are not within a few sigma of a mode."""
    N, T = 33, 3
    head = _head(E, A, M, seed=E + M + A)
    gen = torch.Generator().manual_seed(600 + E + A)
    feats2 = torch.randn(N, E, generator=gen)
    actions = torch.rand(N, A, generator=gen) * 3.0 - 1.5
    g = torch.randn(N, generator=gen)
    sd = head.state_dict()
    ref64 = _reference(sd, feats2, actions, g, 0.0, M, A, "low_noise", torch.float64)
    ref32 = _reference(sd, feats2, actions, g, 0.0, M, A, "low_noise", torch.float32)
    assert ref64["log_prob"].max() < -1e6
    head = head.cuda().eval()
    feats = _layout(feats2, "view", T)
    ac = actions.cuda()
    out = ops.gmm_head(feats, head._params(), M, A, ac, MODES["low_noise"], MIN_STD, want_pre=True, want_params=True)
    assert torch.equal(out["scale"], torch.full_like(out["scale"], 1e-4))
    with torch.no_grad():                                                          # the module's path: the flag AND eval mode
        assert torch.equal(head.log_prob(feats, ac.view(N // T, T, A), low_noise_eval=True).reshape(-1), out["log_prob"])
    gpre = ops.gmm_head_bwd(out["pre"], ac, g.cuda(), None, M, A, MODES["low_noise"], MIN_STD)
    assert bool(torch.isfinite(out["log_prob"]).all()) and bool(torch.isfinite(gpre).all())
    assert bool((gpre[:, M * A:2 * M * A] == 0).all()), "sigma is a constant: its pre-activations have no gradient"
    got = {"log_prob": _t(out["log_prob"]), "mean": _t(out["mean"]), "gpre": _t(gpre)}
    _compare(f"NT={_nt(M, A)} N={N} E={E} M={M} A={A} low_noise", got, ref64, ref32)


def _near_mode_reference(sd, feats, actions, g, M, A, dtype, shift=None):
    """log_prob and gpre of the low-noise restatement; `shift` [N, M, A] is added to every tanh output (the envelope's probe)."""
    sd = {k: v.detach().to(dtype) for k, v in sd.items()}
    pm, ps, lg = (t.detach().requires_grad_(True) for t in gmm_ref.decoder(sd, feats.to(dtype), M, A))
    mu, sg = gmm_ref.activate(pm, ps, MIN_STD, low_noise=True)
    if shift is not None:
        mu = mu + shift.to(dtype)
    lp = gmm_ref.mixture(mu, sg, lg).log_prob(actions.to(dtype))
    ((lp * g.to(dtype)).sum() + 0.0 * ps.sum()).backward()
    N = feats.shape[0]
    return {"log_prob": _t(lp), "gpre": _t(torch.cat((pm.grad.reshape(N, -1), ps.grad.reshape(N, -1), lg.grad.reshape(N, -1)), 1))}


@pytest.mark.parametrize("E,M,A", [(36, 3, 21), (20, 7, 18)])
def test_low_noise_near_a_mode(ops, E, M, A):
    """Actions within 3 sigma of one mode's mean at sigma = 1e-4: ill-conditioned by construction, d log_prob / d mu = z / sigma
    ~ 1e4 and d gpre / d mu = (1 - mu^2) / sigma^2 ~ 1e8, so one fp32 ulp of a tanh output (6e-8 at |mu| ~ 0.5) is 6e-4 sigma.
    Held to the usual bound, which the fp32 restatement's own deviation decides here.  Measured on an MI355X, as fractions of the
    float64 maximum (|log_prob| ~ 150, |gpre| ~ 7e4): log_prob 3.58e-5 against 2.28e-4 at (M, A) = (3, 21) and 4.19e-5 against
    1.41e-4 at (7, 18); gpre 5.29e-4 against 2.12e-3 and 2.96e-4 against 1.24e-3.  The envelope printed next to them -- the float64
    yardstick with every tanh output moved by one fp32 ulp -- is 5.5e-5 / 6.7e-5 for log_prob and 1.5e-4 for gpre: the
    pre-activations' own fp32 rounding weighs as much as tanh's, so the envelope is recorded, not used as the bound."""
    N = 33
    head = _head(E, A, M, seed=E + M + A + 1)
    gen = torch.Generator().manual_seed(700 + E + A)
    feats2 = torch.randn(N, E, generator=gen)
    z = torch.rand(N, A, generator=gen).double() * 6.0 - 3.0
    g = torch.randn(N, generator=gen)
    sd = head.state_dict()
    sd64 = {k: v.double() for k, v in sd.items()}
    mu64 = torch.tanh(gmm_ref.decoder(sd64, feats2.double(), M, A)[0])              # [N, M, A]
    near = mu64[torch.arange(N), torch.arange(N) % M]                               # row n sits on mode n % M
    actions = (near + gmm_ref.LOW_NOISE_STD * z).float()
    ref64 = _near_mode_reference(sd, feats2, actions, g, M, A, torch.float64)
    ref32 = _near_mode_reference(sd, feats2, actions, g, M, A, torch.float32)
    # the envelope: the float64 yardstick with every tanh output moved by one fp32 ulp, all up, all down, all towards the
    # action and all away from it (the two patterns that move every term of l_m the same way); element-wise largest change
    ulp = torch.from_numpy(np.spacing(mu64.float().numpy()).astype(np.float64))
    away = torch.sign(mu64 - actions.double().unsqueeze(1))
    envelope = {k: np.zeros_like(v) for k, v in ref64.items()}
    for pattern in (ulp, -ulp, ulp * away, -ulp * away):
        moved = _near_mode_reference(sd, feats2, actions, g, M, A, torch.float64, shift=pattern)
        for k in envelope:
            envelope[k] = np.maximum(envelope[k], np.abs(moved[k] - ref64[k]))
    head = head.cuda()
    out = ops.gmm_head(feats2.cuda(), head._params(), M, A, actions.cuda(), MODES["low_noise"], MIN_STD, want_pre=True)
    gpre = ops.gmm_head_bwd(out["pre"], actions.cuda(), g.cuda(), None, M, A, MODES["low_noise"], MIN_STD)
    assert bool(torch.isfinite(out["log_prob"]).all()) and bool(torch.isfinite(gpre).all())
    assert bool((gpre[:, M * A:2 * M * A] == 0).all())
    got = {"log_prob": _t(out["log_prob"]), "gpre": _t(gpre)}
    bad = []
    for k, v in got.items():
        top = np.abs(ref64[k]).max()
        e, dev, env = _rel(v, ref64[k]), _rel(ref32[k], ref64[k]), envelope[k].max() / top
        usual = max(FWD_TOL if k == "log_prob" else BWD_TOL, REF_FACTOR * dev)
        print(f"NT={_nt(M, A)} N={N} E={E} M={M} A={A} low_noise near a mode: {k} error {e:.3e}, fp32 restatement's own {dev:.3e}, "
              f"usual bound {usual:.3e}, one-ulp envelope {env:.3e}, largest |{k}| {top:.3e}")
        if not e <= usual:
            bad.append((k, e, usual))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------
# 6. the sampler
# ---------------------------------------------------------------------------------------------------

# (M, A) -> E; the seeds per (M, A, N) were checked on the CPU: in float64 no row's u is within 1e-5 of an interior CDF boundary,
# and the drawn mode's tanh(mean) is at least 1e-4 from every other mode's in some component (an fp32 product of E <= 36 terms of
# order 1 and a 2-ulp tanh are within ~3e-6 of float64, so the nearest mode is the drawn one without ambiguity)
SAMPLER_E = {(1, 63): 36, (16, 1): 8, (3, 64): 20, (3, 21): 36, (7, 18): 20}
SAMPLER_SEEDS = {(1, 63, 65): 1000, (1, 63, 31): 1000, (16, 1, 65): 1003, (16, 1, 31): 1001, (3, 64, 65): 1001, (3, 64, 31): 1000,
                 (3, 21, 65): 1000, (3, 21, 31): 1000, (7, 18, 65): 1000, (7, 18, 31): 1000}
SAMPLER_LAYOUTS = [(65, "view", 5), (31, "dense", 31)]


def _sampler_inputs(M, A, N, seed):
    E = SAMPLER_E[(M, A)]
    head = _head(E, A, M, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    return head, torch.randn(N, E, generator=gen), torch.rand(N, generator=gen), torch.randn(N, A, generator=gen)


def _sampler_condition(head, feats2, u, M, A):
    """In float64: (smallest margin of u from an interior CDF boundary, smallest distance -- largest component -- of a row's drawn
    tanh(mean) from another mode's, number of modes drawn)."""
    sd64 = {k: v.double() for k, v in head.state_dict().items()}
    N = feats2.shape[0]
    zero = torch.zeros(N, A, dtype=torch.float64)
    drawn, modes, margin = gmm_ref.sample_by_inverse_cdf(sd64, feats2.double(), u.double(), zero, M, A)
    mu = torch.tanh(gmm_ref.decoder(sd64, feats2.double(), M, A)[0])                # [N, M, A]
    d = (mu - drawn.unsqueeze(1)).abs().amax(-1)                                    # [N, M]
    d[torch.arange(N), modes] = float("inf")
    return float(margin.min()), float(d.min()), len(set(modes.tolist()))


@pytest.mark.parametrize("N,layout,T", SAMPLER_LAYOUTS)
@pytest.mark.parametrize("M,A", list(SAMPLER_E))
def test_sampler_matches_the_float64_sampler(ops, M, A, N, layout, T):
    head, feats2, u, eps = _sampler_inputs(M, A, N, SAMPLER_SEEDS[(M, A, N)])
    margin, apart, drawn = _sampler_condition(head, feats2, u, M, A)
    print(f"M={M} A={A} N={N}: smallest CDF margin {margin:.3e}, the drawn mode at least {apart:.3e} from the others, {drawn} modes drawn")
    assert margin >= 1e-5, "the seeds must leave every row away from the CDF boundaries"
    assert apart >= 1e-4 and drawn >= min(M, 3)
    sd64 = {k: v.double() for k, v in head.state_dict().items()}
    sd32 = dict(head.state_dict())
    head = head.cuda()
    params = tuple(p.detach() for p in head._params())
    feats = _layout(feats2, layout, T)
    mu64 = torch.tanh(gmm_ref.decoder(sd64, feats2.double(), M, A)[0])
    zero = torch.zeros(N, A).cuda()
    for act in ("softplus", "exp", "low_noise"):
        low = act == "low_noise"
        kw = dict(min_std=MIN_STD, std_activation="softplus" if low else act, low_noise=low)
        want, modes, m64 = gmm_ref.sample_by_inverse_cdf(sd64, feats2.double(), u.double(), eps.double(), M, A, **kw)
        want32 = gmm_ref.sample_by_inverse_cdf(sd32, feats2, u, eps, M, A, **kw)[0]
        keep = m64 >= 1e-5
        assert bool(keep.all())                                                     # the share of excluded rows is 0
        got = ops.gmm_sample(feats, params, M, A, u.cuda(), eps.cuda(), MODES[act], MIN_STD)
        assert got.shape == (N, A)
        assert torch.equal(got, ops.gmm_sample(feats, params, M, A, u.cuda(), eps.cuda(), MODES[act], MIN_STD))
        tag = f"NT={_nt(M, A)} N={N} E={feats2.shape[1]} M={M} A={A} {act} {layout} sampler"
        _compare(tag, {"sample": _t(got)}, {"sample": _t(want)}, {"sample": _t(want32)})
        # eps = 0: the output is tanh(mean) of the chosen mode, which is recovered as the nearest mode, for every row
        plain = ops.gmm_sample(feats, params, M, A, u.cuda(), zero, MODES[act], MIN_STD).cpu().double()
        nearest = (plain.unsqueeze(1) - mu64).abs().amax(-1).argmin(-1)
        assert torch.equal(nearest, modes), f"{tag}: rows {(nearest != modes).nonzero().flatten().tolist()} drew another mode"
        if M == 1:
            assert int(modes.max()) == 0
        # u = 0 picks the first mode, u just below 1 the last
        first = ops.gmm_sample(feats, params, M, A, torch.zeros(N).cuda(), zero, MODES[act], MIN_STD)
        last = ops.gmm_sample(feats, params, M, A, torch.full((N,), 1.0 - 2.0 ** -24).cuda(), zero, MODES[act], MIN_STD)
        assert _rel(_t(first), _t(mu64[:, 0])) <= FWD_TOL and _rel(_t(last), _t(mu64[:, M - 1])) <= FWD_TOL
