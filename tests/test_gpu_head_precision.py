"""GPU: the output heads' bf16 / bf16x3 matrix-pipe modes (ActionHead / GMMActionHead.set_matmul_precision; the _mp_f32 entry
points of csrc/lipvq_action_head.hip and csrc/lipvq_gmm.hip over lq_head_product_bf16, csrc/lipvq_head_product.h).

What is bit-compared, and why it is a property and not the code against itself:
 1. the product: the head's pre-activations against ops.linear_<mode> -- another kernel (gemm_bf16_kernel) -- on the dense rows and the
    stacked, zero-padded parameters: include/lipvq.h promises both the same chain, and that a row's bits depend on no tile;
 2. the epilogue: every output of a bf16-mode call against the FP32-mode call on an input whose fp32 product reproduces those
    pre-activations exactly (x' = [pre | 0], identity weights, zero bias): the epilogue is the fp32 head's, untouched;
 3. isolation (a NaN / Inf / overflowing row changes its own outputs only; fenced outputs through the C ABI);
 4. the backward: gradients against ops.linear_nn_<mode> / ops.wgrad_<mode> on the zero-padded gpre of the fp32 backward kernel;
 6. the modules: set and restored, graph replay against eager, the captured policy step, PromptedPolicy.
What is measured against float64 (5.): the bf16 mode against the restatements tests/action_head_ref.py / tests/gmm_ref.py on
operands rounded with gpt_bf16_ref.bf16_round (FWD_TOL = 1e-5, BWD_TOL = 1e-4 of the maximum: with the rounding restated only the
fp32 accumulation differs), the bf16x3 pre-activations against float64 on the unrounded operands within the header's bound.
Every figure is printed before it is asserted.  Inputs are drawn from seeds."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import action_head_ref
import gemm_bf16x3_ref as x3
import gmm_ref
import gpt_bf16_ref
from fenced import _Fenced

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 1e-5, 1e-4
MODES = ("bf16", "bf16x3")
MATMUL = {"fp32": 0, "bf16": 1, "bf16x3": 2}
MIXED = (0.5, 2.0, 0.25)
MIN_STD = 0.01


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _linear(ops, m):
    return {"bf16": ops.linear_bf16, "bf16x3": ops.linear_bf16x3}[m]


def _linear_nn(ops, m):
    return {"bf16": ops.linear_nn_bf16, "bf16x3": ops.linear_nn_bf16x3}[m]


def _wgrad(ops, m):
    return {"bf16": ops.wgrad_bf16, "bf16x3": ops.wgrad_bf16x3}[m]


def pad8(W, b):
    """Weights [P, E] and bias [P] extended with zero rows to a multiple of 8."""
    P = W.shape[0]
    P8 = (P + 7) // 8 * 8
    return F.pad(W, (0, 0, 0, P8 - P)).contiguous(), F.pad(b, (0, P8 - P)).contiguous()


def _action_head(E, A, seed=0):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.action_head import ActionHead
    torch.manual_seed(seed)
    return ActionHead(E, A)


def _gmm_head(E, A, M, seed=0, **kw):
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd.gmm import GMMActionHead
    torch.manual_seed(seed)
    return GMMActionHead(E, A, num_modes=M, min_std=MIN_STD, **kw)


def _view(rows, T, E, seed):
    """feats [B, T, E]: the view [:, -T:] of a [B, 3T, E] tensor (never contiguous for B > 1), and its rows [rows, E]."""
    B = rows // T
    assert B * T == rows
    full = torch.randn(B, 3 * T, E, generator=torch.Generator().manual_seed(seed)).cuda()
    feats = full[:, -T:]
    assert B == 1 or not feats.is_contiguous()
    return feats, feats.reshape(rows, E)


ROWS = ((1, 1), (31, 1), (33, 1), (80, 10))                    # (rows, T)


# ---------------------------------------------------------------------------------------------------
# 1. the product is the gemm's, bit for bit
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", [8, 72, 512, 1024])
@pytest.mark.parametrize("m", MODES)
def test_action_head_product_is_the_gemms(ops, m, E):
    for A in (1, 12, 33, 64):
        head = _action_head(E, A, seed=E + A).cuda()
        W, b = head.nets["action"].weight.detach(), head.nets["action"].bias.detach()
        W8, b8 = pad8(W, b)
        for rows, T in ROWS:
            feats, feats2 = _view(rows, T, E, seed=rows + A)
            pre = ops.action_head(feats, W, b, want_pre=True, precision=m)["pre"]
            want = _linear(ops, m)(feats2, W8, b8)[:, :A]
            bad = (pre != want).sum().item()
            assert pre.shape == (rows, A) and torch.equal(pre, want), f"E={E} A={A} rows={rows} T={T}: {bad} elements differ"
            if rows * A >= 960:                                                     # ... and it is not the fp32 chain (enough elements to tell)
                assert not torch.equal(pre, ops.action_head(feats, W, b, want_pre=True)["pre"])


GMM_SHAPES = ((1, 1), (5, 12), (5, 25), (16, 15), (8, 31))     # (M, A): P = 3; 125 (NT 1); 255 (NT 2); 496 (NT 4); 504


def _stack(params):
    Wm, bm, Ws, bs, Wl, bl = params
    return torch.cat((Wm, Ws, Wl), 0), torch.cat((bm, bs, bl), 0)


@pytest.mark.parametrize("E", [8, 512])
@pytest.mark.parametrize("M,A", GMM_SHAPES)
@pytest.mark.parametrize("m", MODES)
def test_gmm_product_is_the_gemms(ops, m, M, A, E):
    P = M * (2 * A + 1)
    head = _gmm_head(E, A, M, seed=M + A).cuda()
    params = tuple(p.detach() for p in head._params())
    W8, b8 = pad8(*_stack(params))
    for rows, T in ((33, 1), (80, 10)):
        feats, feats2 = _view(rows, T, E, seed=rows + P)
        pre = ops.gmm_head(feats, params, M, A, want_pre=True, precision=m)["pre"]
        want = _linear(ops, m)(feats2, W8, b8)[:, :P]
        bad = (pre != want).sum().item()
        assert pre.shape == (rows, P) and torch.equal(pre, want), f"E={E} M={M} A={A} rows={rows}: {bad} elements differ"


# ---------------------------------------------------------------------------------------------------
# 2. the epilogue is the fp32 head's, bit for bit
# ---------------------------------------------------------------------------------------------------

def _embed(pre, B, T):
    """(x' [B, T, E'], identity rows [P, E'], zero bias [P]): an fp32-mode product that reproduces pre [B T, P] exactly
    (0 + pre 1 + zeros, every step exact)."""
    N, P = pre.shape
    E2 = (P + 3) // 4 * 4
    x = F.pad(pre, (0, E2 - P)).contiguous().view(B, T, E2)
    return x, torch.eye(P, E2, device=pre.device), torch.zeros(P, device=pre.device)


@pytest.mark.parametrize("E,A,rows,T", [(512, 12, 80, 10), (72, 33, 33, 1), (8, 1, 31, 1), (1024, 64, 33, 1)])
@pytest.mark.parametrize("m", MODES)
def test_action_head_epilogue_is_the_fp32_heads(ops, m, E, A, rows, T):
    head = _action_head(E, A, seed=3 + A).cuda()
    W, b = head.nets["action"].weight.detach(), head.nets["action"].bias.detach()
    feats, _ = _view(rows, T, E, seed=rows)
    feats = feats * 3.0                                                             # pre-activations on both sides of tanh's knee
    target = (torch.rand(rows, A, generator=torch.Generator().manual_seed(A)) * 3.0 - 1.5).cuda()
    got = ops.action_head(feats, W, b, target, MIXED, want_pre=True, precision=m)
    assert bool(torch.isfinite(got["pre"]).all())
    x2, eye, zero = _embed(got["pre"], rows // T, T)
    want = ops.action_head(x2, eye, zero, target, MIXED, want_pre=True)
    assert torch.equal(want["pre"], got["pre"]), "the fp32 call does not reproduce the pre-activations: the test's own premise"
    for k in ("actions", "losses"):
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("E,M,A", [(512, 5, 12), (8, 1, 1), (72, 5, 25), (512, 16, 15), (8, 8, 31)])
@pytest.mark.parametrize("m", MODES)
def test_gmm_epilogue_is_the_fp32_heads(ops, m, E, M, A):
    rows, T = 80, 10
    B, P = rows // T, M * (2 * A + 1)
    for act, kw in (("softplus", {}), ("exp", {"std_activation": "exp"})):
        head = _gmm_head(E, A, M, seed=5 + M, **kw).cuda()
        params = tuple(p.detach() for p in head._params())
        mode = {"softplus": ops.GMM_SOFTPLUS, "exp": ops.GMM_EXP}[act]
        feats, _ = _view(rows, T, E, seed=P)
        gen = torch.Generator().manual_seed(P + 1)
        actions = (torch.rand(rows, A, generator=gen) * 2.0 - 1.0).cuda()
        u, eps = torch.rand(rows, generator=gen).cuda(), torch.randn(rows, A, generator=gen).cuda()
        snap = torch.tensor([1234, 7], dtype=torch.int64).cuda()
        streams = torch.tensor([11, 3, 0, 5, 2 ** 33, 9, 1, 4], dtype=torch.int64).cuda()
        got = ops.gmm_head(feats, params, M, A, actions, mode, MIN_STD, want_pre=True, want_params=True, want_sum=True, precision=m)
        assert bool(torch.isfinite(got["pre"]).all())
        x2, eye, zero = _embed(got["pre"], B, T)
        MA = M * A
        p2 = (eye[:MA], zero[:MA], eye[MA:2 * MA], zero[MA:2 * MA], eye[2 * MA:], zero[2 * MA:])
        want = ops.gmm_head(x2, p2, M, A, actions, mode, MIN_STD, want_pre=True, want_params=True, want_sum=True)
        assert torch.equal(want["pre"], got["pre"]), "the fp32 call does not reproduce the pre-activations: the test's own premise"
        for k in ("log_prob", "sum", "mean", "scale", "logits"):
            assert torch.equal(got[k], want[k]), f"{act}: {k}"
        assert torch.equal(ops.gmm_sample(feats, params, M, A, u, eps, mode, MIN_STD, precision=m),
                           ops.gmm_sample(x2, p2, M, A, u, eps, mode, MIN_STD)), f"{act}: sample"
        assert torch.equal(ops.gmm_sample_draw(feats, params, M, A, snap, streams, mode, MIN_STD, precision=m),
                           ops.gmm_sample_draw(x2, p2, M, A, snap, streams, mode, MIN_STD)), f"{act}: drawn sample"


# ---------------------------------------------------------------------------------------------------
# 3. isolation
# ---------------------------------------------------------------------------------------------------

def _rows_differ(a, b):
    n = a.shape[0]
    return ((a != b) & ~(torch.isnan(a) & torch.isnan(b))).reshape(n, -1).any(1).nonzero().flatten().tolist()


def _ah_row_outputs(ops, feats, W, b, m):
    out = ops.action_head(feats, W, b, want_pre=True, precision=m)
    return {"pre": out["pre"], "actions": out["actions"]}


def _gmm_row_outputs(ops, feats, params, M, A, actions, u, eps, m):
    out = ops.gmm_head(feats, params, M, A, actions, ops.GMM_SOFTPLUS, MIN_STD, want_pre=True, want_params=True, precision=m)
    out["sample"] = ops.gmm_sample(feats, params, M, A, u, eps, ops.GMM_SOFTPLUS, MIN_STD, precision=m)
    return out


DIRTY = {"a NaN and an Inf": ((3, float("nan")), (5, float("inf"))), "3.4e38": ((2, 3.4e38),), "-3.4e38": ((6, -3.4e38),)}


@pytest.mark.parametrize("what", list(DIRTY))
@pytest.mark.parametrize("m", MODES)
def test_a_non_finite_or_overflowing_row_changes_its_own_outputs_only(ops, m, what):
    """3.4e38 is finite in fp32 and rounds to Inf in bf16 (include/lipvq.h: from the bit pattern 0x7f7f8000 up): the row is
    non-finite in both modes, where the fp32 head's is finite."""
    rows, T, E = 80, 10, 72
    for r in (0, 37, 79):                                                           # first and last row, one inside a tile
        feats, _ = _view(rows, T, E, seed=r)
        dirty = feats.clone()
        for k, v in DIRTY[what]:
            dirty[r // T, r % T, k] = v
        others = [i for i in range(rows) if i != r]
        head = _action_head(E, 12, seed=1).cuda()
        W, b = head.nets["action"].weight.detach(), head.nets["action"].bias.detach()
        clean, got = _ah_row_outputs(ops, feats, W, b, m), _ah_row_outputs(ops, dirty, W, b, m)
        for k in clean:
            assert _rows_differ(got[k][others], clean[k][others]) == [], f"action head {k}: a row other than {r} changed"
        assert not bool(torch.isfinite(got["pre"][r]).any()), f"action head: row {r} of pre is {got['pre'][r]}"
        assert bool(torch.isfinite(got["pre"][others]).all())
        M, A = 5, 12
        gh = _gmm_head(E, A, M, seed=2).cuda()
        params = tuple(p.detach() for p in gh._params())
        gen = torch.Generator().manual_seed(r)
        actions = (torch.rand(rows, A, generator=gen) * 2.0 - 1.0).cuda()
        u, eps = torch.rand(rows, generator=gen).cuda(), torch.randn(rows, A, generator=gen).cuda()
        clean = _gmm_row_outputs(ops, feats, params, M, A, actions, u, eps, m)
        got = _gmm_row_outputs(ops, dirty, params, M, A, actions, u, eps, m)
        for k in clean:
            assert _rows_differ(got[k][others], clean[k][others]) == [], f"gmm head {k}: a row other than {r} changed"
        assert not bool(torch.isfinite(got["pre"][r]).any()) and not bool(torch.isfinite(got["log_prob"][r]))
        assert bool(torch.isnan(got["sample"][r]).all())                            # no draw from weights that are not numbers


AH_ORDER = ("actions", "pre", "losses", "workspace")
GMM_ORDER = ("log_prob", "pre", "mean", "scale", "logits", "sum", "workspace")


@pytest.mark.parametrize("N", [1, 33])
@pytest.mark.parametrize("m", MODES)
def test_outputs_are_written_inside_fenced_buffers(ops, m, N):
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    lib, check, stream = _capi.lib, _capi.check, lipvq_vae_amd.ops._stream
    E, A, M = 72, 33, 3
    gen = torch.Generator().manual_seed(N)
    x = torch.randn(N, E, generator=gen).cuda()
    # the action head
    head = _action_head(E, A, seed=N).cuda()
    W, b = head.nets["action"].weight.detach(), head.nets["action"].bias.detach()
    target = (torch.rand(N, A, generator=gen) * 3.0 - 1.5).cuda()
    want = ops.action_head(x, W, b, target, MIXED, want_pre=True, precision=m)
    nbytes = lib.lipvq_action_head_workspace_bytes(N)
    f = {"actions": _Fenced("actions", N, A, offset_words=1), "pre": _Fenced("pre", N, A, offset_words=1),
         "losses": _Fenced("losses", 4, offset_words=1), "workspace": _Fenced("workspace", nbytes // 4, offset_words=1)}
    check(lib.lipvq_action_head_mp_f32(x.data_ptr(), N * E, W.data_ptr(), b.data_ptr(), target.data_ptr(), *[f[k].ptr() for k in AH_ORDER],
                                       N, N, E, A, *MIXED, MATMUL[m], stream()), "lipvq_action_head_mp_f32")
    torch.cuda.synchronize()
    for k in AH_ORDER:
        t = f[k].check()
        assert k == "workspace" or torch.equal(t.reshape(want[k].shape), want[k]), k
    # the GMM head, its sampler and its drawing sampler
    P = M * (2 * A + 1)
    gh = _gmm_head(E, A, M, seed=N + 1).cuda()
    params = tuple(p.detach() for p in gh._params())
    pp = [p.data_ptr() for p in params]
    actions = (torch.rand(N, A, generator=gen) * 2.0 - 1.0).cuda()
    u, eps = torch.rand(N, generator=gen).cuda(), torch.randn(N, A, generator=gen).cuda()
    snap = torch.tensor([99, 3], dtype=torch.int64).cuda()
    want = ops.gmm_head(x, params, M, A, actions, 0, MIN_STD, want_pre=True, want_params=True, want_sum=True, precision=m)
    nbytes = lib.lipvq_gmm_workspace_bytes(N)
    f = {"log_prob": _Fenced("log_prob", N, offset_words=1), "pre": _Fenced("pre", N, P, offset_words=1),
         "mean": _Fenced("mean", N, M, A, offset_words=1), "scale": _Fenced("scale", N, M, A, offset_words=1),
         "logits": _Fenced("logits", N, M, offset_words=1), "sum": _Fenced("lp_sum", 1, offset_words=1),
         "workspace": _Fenced("workspace", nbytes // 4, offset_words=1)}
    check(lib.lipvq_gmm_head_mp_f32(x.data_ptr(), N * E, *pp, actions.data_ptr(), *[f[k].ptr() for k in GMM_ORDER], N, N, E, M, A, 0, MIN_STD,
                                    MATMUL[m], stream()), "lipvq_gmm_head_mp_f32")
    torch.cuda.synchronize()
    for k in GMM_ORDER:
        t = f[k].check()
        assert k == "workspace" or torch.equal(t.reshape(want[k].shape), want[k]), k
    action = _Fenced("action", N, A, offset_words=1)
    check(lib.lipvq_gmm_sample_mp_f32(x.data_ptr(), N * E, *pp, u.data_ptr(), eps.data_ptr(), action.ptr(), N, N, E, M, A, 0, MIN_STD,
                                      MATMUL[m], stream()), "lipvq_gmm_sample_mp_f32")
    torch.cuda.synchronize()
    assert torch.equal(action.check(), ops.gmm_sample(x, params, M, A, u, eps, 0, MIN_STD, precision=m))
    action = _Fenced("action", N, A, offset_words=1)
    check(lib.lipvq_gmm_sample_draw_mp_f32(x.data_ptr(), N * E, *pp, snap.data_ptr(), None, action.ptr(), N, N, E, M, A, 0, MIN_STD,
                                           MATMUL[m], stream()), "lipvq_gmm_sample_draw_mp_f32")
    torch.cuda.synchronize()
    assert torch.equal(action.check(), ops.gmm_sample_draw(x.view(1, N, E), params, M, A, snap, None, 0, MIN_STD, precision=m))


# ---------------------------------------------------------------------------------------------------
# 4. the backward
# ---------------------------------------------------------------------------------------------------

def _expected_grads(ops, m, gpre, feats2, W, b):
    """gx, gW, gb from linear_nn_<m> / wgrad_<m> on gpre's columns and the stacked weight's rows extended with zeros to 8 ceil(P / 8)."""
    P = gpre.shape[1]
    W8, _ = pad8(W, b)
    g8 = F.pad(gpre, (0, W8.shape[0] - P)).contiguous()
    gW, gb = _wgrad(ops, m)(g8, feats2.contiguous())
    return _linear_nn(ops, m)(g8, W8), gW[:P], gb[:P]


@pytest.mark.parametrize("E,A,rows,T", [(512, 12, 80, 10), (72, 33, 33, 1), (8, 64, 31, 1)])
@pytest.mark.parametrize("m", MODES)
def test_action_head_backward_runs_on_the_modes_gemms(ops, m, E, A, rows, T):
    head = _action_head(E, A, seed=7 + A).cuda().set_matmul_precision(m)
    W, b = head.nets["action"].weight, head.nets["action"].bias
    feats, feats2 = _view(rows, T, E, seed=A)
    target = (torch.rand(rows // T, T, A, generator=torch.Generator().manual_seed(E)) * 3.0 - 1.5).cuda()
    pre = ops.action_head(feats, W.detach(), b.detach(), want_pre=True, precision=m)["pre"]
    gpre = ops.action_head_bwd(pre, target, g=torch.tensor([0.0, 0.0, 0.0, 1.0]).cuda(), weights=MIXED)
    gx, gW, gb = _expected_grads(ops, m, gpre, feats2, W.detach(), b.detach())
    runs = []
    for _ in range(2):
        head.zero_grad(set_to_none=True)
        x = feats.detach().requires_grad_(True)
        head.losses(x, target, *MIXED)["action_loss"].backward()
        runs.append((x.grad.clone(), W.grad.clone(), b.grad.clone()))
    assert all(torch.equal(p, q) for p, q in zip(*runs)), "a second forward and backward gave other bits"
    assert torch.equal(runs[0][0].reshape(rows, E), gx) and torch.equal(runs[0][1], gW) and torch.equal(runs[0][2], gb)
    # frozen weights; an input that needs no gradient
    head.zero_grad(set_to_none=True)
    head.requires_grad_(False)
    x = feats.detach().requires_grad_(True)
    head.losses(x, target, *MIXED)["action_loss"].backward()
    assert torch.equal(x.grad, runs[0][0]) and W.grad is None and b.grad is None
    head.requires_grad_(True)
    x = feats.detach()
    head.losses(x, target, *MIXED)["action_loss"].backward()
    assert x.grad is None and torch.equal(W.grad, gW) and torch.equal(b.grad, gb)


@pytest.mark.parametrize("E,M,A", [(512, 5, 12), (8, 1, 1), (72, 8, 31)])
@pytest.mark.parametrize("m", MODES)
def test_gmm_backward_runs_on_the_modes_gemms(ops, m, E, M, A):
    rows, T = 80, 10
    MA = M * A
    head = _gmm_head(E, A, M, seed=9 + M).cuda().train().set_matmul_precision(m)
    params = head._params()
    det = tuple(p.detach() for p in params)
    feats, feats2 = _view(rows, T, E, seed=M)
    actions = (torch.rand(rows // T, T, A, generator=torch.Generator().manual_seed(E)) * 2.0 - 1.0).cuda()
    pre = ops.gmm_head(feats, det, M, A, want_pre=True, precision=m)["pre"]
    s = torch.zeros((), device="cuda", requires_grad=True)                          # the gradient autograd hands the sum: that of -s / rows
    (-s / rows).backward()
    gpre = ops.gmm_head_bwd(pre, actions.reshape(rows, A), None, s.grad, M, A, ops.GMM_SOFTPLUS, MIN_STD)
    gx, gW, gb = _expected_grads(ops, m, gpre, feats2, *_stack(det))
    want = (gW[:MA], gb[:MA], gW[MA:2 * MA], gb[MA:2 * MA], gW[2 * MA:], gb[2 * MA:])
    runs = []
    for _ in range(2):
        head.zero_grad(set_to_none=True)
        x = feats.detach().requires_grad_(True)
        head.nll(x, actions).backward()
        runs.append((x.grad.clone(),) + tuple(p.grad.clone() for p in params))
    assert all(torch.equal(p, q) for p, q in zip(*runs)), "a second forward and backward gave other bits"
    assert torch.equal(runs[0][0].reshape(rows, E), gx)
    for i, (got, w) in enumerate(zip(runs[0][1:], want)):
        assert torch.equal(got, w), gmm_ref.KEYS[i]
    head.zero_grad(set_to_none=True)
    head.requires_grad_(False)
    x = feats.detach().requires_grad_(True)
    head.nll(x, actions).backward()
    assert torch.equal(x.grad, runs[0][0]) and all(p.grad is None for p in params)
    head.requires_grad_(True)
    x = feats.detach()
    head.nll(x, actions).backward()
    assert x.grad is None and all(torch.equal(p.grad, w) for p, w in zip(params, want))


# ---------------------------------------------------------------------------------------------------
# 5. accuracy, printed before it is asserted
# ---------------------------------------------------------------------------------------------------

def _t(x):
    return x.detach().cpu().double().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def _report(tag, got, want, forward_keys):
    bad = []
    for k, v in got.items():
        tol = FWD_TOL if k in forward_keys else BWD_TOL
        e = _rel(v, want[k])
        print(f"{tag}: {k} error {e:.3e} of the maximum, bound {tol:.1e}")
        if not e <= tol:
            bad.append((k, e, tol))
    assert not bad, bad


@pytest.fixture
def rounded_linear(monkeypatch):
    """F.linear of the two restatements replaced by gpt_bf16_ref's rounded Linear: both matrix operands rounded to bf16 in the
    forward, g, W and x rounded in the two backward products, gb the plain column sums."""
    monkeypatch.setattr(action_head_ref, "F", gpt_bf16_ref._Functional())
    monkeypatch.setattr(gmm_ref, "F", gpt_bf16_ref._Functional())


@pytest.mark.parametrize("E,A,rows,T", [(512, 12, 80, 10), (72, 33, 33, 1)])
def test_bf16_action_head_against_float64_on_rounded_operands(ops, rounded_linear, E, A, rows, T):
    head = _action_head(E, A, seed=11).set_matmul_precision("bf16")
    sd = {k: v.detach().double().requires_grad_(True) for k, v in head.state_dict().items()}
    head = head.cuda()
    feats, feats2 = _view(rows, T, E, seed=3)
    target = torch.rand(rows, A, generator=torch.Generator().manual_seed(4)) * 3.0 - 1.5
    x64 = feats2.cpu().double().requires_grad_(True)
    y = action_head_ref.actions(sd, x64)
    losses = action_head_ref.compute_losses(y, target.double(), MIXED)
    losses["action_loss"].backward()
    want = {"actions": _t(y), "gx": _t(x64.grad), "gW": _t(sd[action_head_ref.KEYS[0]].grad), "gb": _t(sd[action_head_ref.KEYS[1]].grad)}
    want.update({k: _t(v) for k, v in losses.items()})
    x = feats.detach().requires_grad_(True)
    out = head.losses(x, target.cuda().view(rows // T, T, A), *MIXED)
    out["action_loss"].backward()
    got = {"actions": _t(head(feats)).reshape(rows, A), "gx": _t(x.grad).reshape(rows, E), "gW": _t(head.nets["action"].weight.grad),
           "gb": _t(head.nets["action"].bias.grad)}
    got.update({k: _t(v) for k, v in out.items()})
    _report(f"bf16 action head E={E} A={A} rows={rows}", got, want, ("actions",) + action_head_ref.LOSS_KEYS)


@pytest.mark.parametrize("E,M,A", [(512, 5, 12), (72, 8, 31)])
def test_bf16_gmm_head_against_float64_on_rounded_operands(ops, rounded_linear, E, M, A):
    """Measured on an MI355X: forward <= 2.7e-7; gradients <= 5.2e-6 at (512, 5, 12) and <= 9.9e-5 at (72, 8, 31), P = 504 -- there
    the figure is not accumulation: the backward products round gpre to bf16, the kernel's fp32 gpre and the restatement's float64
    gpre differ in the last bits, and of 80 x 504 elements a few fall on the other side of a bf16 rounding boundary (2^-9 of one
    term of an 80-term sum)."""
    rows, T = 80, 10
    head = _gmm_head(E, A, M, seed=13).train().set_matmul_precision("bf16")
    sd = {k: v.detach().double().requires_grad_(True) for k, v in head.state_dict().items()}
    head = head.cuda()
    feats, feats2 = _view(rows, T, E, seed=5)
    actions = torch.rand(rows, A, generator=torch.Generator().manual_seed(6)) * 2.0 - 1.0
    x64 = feats2.cpu().double().requires_grad_(True)
    means, scales, logits = gmm_ref.decoder(sd, x64, M, A)
    means, scales = gmm_ref.activate(means, scales, MIN_STD)
    lp = gmm_ref.mixture(means, scales, logits).log_prob(actions.double())
    nll = -lp.mean()
    nll.backward()
    want = {"log_prob": _t(lp), "nll": _t(nll), "mean": _t(means), "scale": _t(scales), "logits": _t(logits), "gx": _t(x64.grad)}
    want.update({"g." + k: _t(sd[k].grad) for k in gmm_ref.KEYS})
    x = feats.detach().requires_grad_(True)
    loss = head.nll(x, actions.cuda().view(rows // T, T, A))
    loss.backward()
    dist = head.forward_train(feats)
    got = {"log_prob": _t(head.log_prob(feats, actions.cuda().view(rows // T, T, A))).reshape(rows), "nll": _t(loss),
           "mean": _t(dist.component_distribution.base_dist.loc).reshape(rows, M, A),
           "scale": _t(dist.component_distribution.base_dist.scale).reshape(rows, M, A),
           "gx": _t(x.grad).reshape(rows, E)}
    # (Categorical normalises its logits: the raw ones come from the launch)
    got["logits"] = _t(ops.gmm_head(feats, tuple(p.detach() for p in head._params()), M, A, want_params=True, precision="bf16")["logits"])
    got.update({"g." + k: _t(p.grad) for k, p in zip(gmm_ref.KEYS, head._params())})
    _report(f"bf16 gmm head E={E} M={M} A={A}", got, want, ("log_prob", "nll", "mean", "scale", "logits"))


@pytest.mark.parametrize("E", [72, 512, 1024])
def test_bf16x3_pre_activations_are_within_the_headers_bound(ops, E):
    """Per element, |pre - exact| <= 3 2^-16 (1 + 2^-7) sum |x| |W|  +  (3 E + 1) 2^-24 sum (|x_hi W_hi| + |x_hi W_lo| + |x_lo W_hi|)
    (include/lipvq.h, the bf16x3 section) +  2^-24 |pre|: the bias is added after the chain, one more fp32 rounding of at most half
    an ulp of the result.  exact = the float64 product of the unrounded operands plus the bias; the bound in float64 from the inputs."""
    rows, T, M, A = 80, 10, 5, 12
    feats, feats2 = _view(rows, T, E, seed=E)
    x = feats2.cpu()
    heads = ((_action_head(E, A, seed=15), None), (_gmm_head(E, A, M, seed=16), (M, A)))
    for head, gmm in heads:
        head = head.cuda()
        if gmm:
            params = tuple(p.detach() for p in head._params())
            W, b = _stack(params)
            pre = ops.gmm_head(feats, params, M, A, want_pre=True, precision="bf16x3")["pre"]
        else:
            W, b = head.nets["action"].weight.detach(), head.nets["action"].bias.detach()
            pre = ops.action_head(feats, W, b, want_pre=True, precision="bf16x3")["pre"]
        W, b = W.cpu(), b.cpu()
        exact, R_exact = x3.product_exact("NT", x, W)
        _, R3 = x3.product3("NT", x, W)
        exact = exact + b.double()
        bound = x3.SPLIT_REL * R_exact + (3 * E + 1) * x3.EPS * R3 + x3.EPS * exact.abs()
        err = (pre.cpu().double() - exact).abs()
        worst = float((err / bound).max())
        print(f"bf16x3 {'gmm' if gmm else 'action'} head E={E}: max error {float(err.max()):.3e}, max error / bound {worst:.3f}, "
              f"relative to max |pre| {float(err.max() / exact.abs().max()):.3e}")
        assert worst <= 1.0
        plain = (ops.action_head(feats, W.cuda(), b.cuda(), want_pre=True, precision="bf16")["pre"] if not gmm else
                 ops.gmm_head(feats, params, M, A, want_pre=True, precision="bf16")["pre"])
        e1 = float((plain.cpu().double() - exact).abs().max())
        print(f"    (the bf16 mode's max error on the same inputs: {e1:.3e})")
        assert float(err.max()) < e1 / 16                                           # the split really ran


# ---------------------------------------------------------------------------------------------------
# 6. the modules
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", MODES)
def test_set_and_restored_is_an_untouched_head(ops, m):
    B, T, E, A, M = 8, 10, 512, 12, 5
    feats, _ = _view(B * T, T, E, seed=1)
    gen = torch.Generator().manual_seed(2)
    target = (torch.rand(B, T, A, generator=gen) * 2.0 - 1.0).cuda()
    u, eps = torch.rand(B, T, generator=gen).cuda(), torch.randn(B, T, A, generator=gen).cuda()

    def run_action(head):
        x = feats.detach().requires_grad_(True)
        out = head.losses(x, target, *MIXED)
        out["action_loss"].backward()
        return [head(feats).detach(), torch.stack(list(out.values())).detach(), x.grad, head.nets["action"].weight.grad.clone()]

    def run_gmm(head):
        x = feats.detach().requires_grad_(True)
        loss = head.nll(x, target)
        loss.backward()
        d = head.forward_train(feats)
        return [loss.detach(), x.grad, head.nets["scale"].weight.grad.clone(), head.log_prob(feats, target).detach(),
                d.component_distribution.base_dist.scale.detach(), head(feats, u=u, eps=eps)]

    for make, run in ((lambda: _action_head(E, A, seed=3).cuda(), run_action), (lambda: _gmm_head(E, A, M, seed=4).cuda().train(), run_gmm)):
        untouched, head = make(), make()
        want = run(untouched)
        other = run(head.set_matmul_precision(m))
        head.zero_grad(set_to_none=True)
        back = run(head.set_matmul_precision("fp32"))
        assert all(torch.equal(p, q) for p, q in zip(back, want)), "fp32 after a mode is not the default's bits"
        assert not any(torch.equal(p, q) for p, q in zip(other, want)), "the mode did not reach one of the paths"


@pytest.mark.parametrize("m", MODES)
def test_graphed_eval_replays_the_mode_it_was_captured_in(ops, m):
    from lipvq_vae_amd.nnfn import GraphedEval
    B, T, E, A, M = 8, 10, 512, 12, 5
    gen = torch.Generator().manual_seed(5)
    xs = [torch.randn(B, T, E, generator=gen).cuda() for _ in range(3)]
    for head in (_action_head(E, A, seed=6).cuda().eval(), _gmm_head(E, A, M, seed=7).cuda().eval().set_sample_source("kernel", seed=21)):
        head.set_matmul_precision(m)
        graphed = GraphedEval(head, torch.zeros_like(xs[0]))
        is_gmm = hasattr(head, "sample_state")
        for i, x in enumerate(xs):
            if is_gmm:
                state = head.sample_state.clone()
            got = graphed(x).clone()
            if is_gmm:
                head.sample_state.copy_(state)                                      # the eager call draws what the replay drew
            with torch.no_grad():
                assert torch.equal(got, head(x)), f"replay {i}"
        # the captured graph keeps its mode: the module's setting now differs, the replay does not
        head.set_matmul_precision("fp32")
        if is_gmm:
            state = head.sample_state.clone()
        got = graphed(xs[0]).clone()
        head.set_matmul_precision(m)
        if is_gmm:
            head.sample_state.copy_(state)
        with torch.no_grad():
            assert torch.equal(got, head(xs[0])), "the replay followed the module's later setting"


def test_graphed_policy_step_in_bf16_equals_eager_steps(golden_dir):
    """Backbone (the gpt_small shape: E = 64, two layers) + ActionHead, both in "bf16": zero_grad -> losses -> backward -> Adam,
    captured; replay k equals eager step k bit for bit, in parameters and loss."""
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd import optim
    from lipvq_vae_amd.gpt import GPTBackbone
    from lipvq_vae_amd.icl import GraphedPolicyStep
    g = np.load(golden_dir / "gpt_small.npz", allow_pickle=False)
    cfg = {k: int(g[k]) for k in ("seed", "B", "L", "E", "H", "layers", "causal")}
    B, L, E, T, A = 4, cfg["L"], cfg["E"], cfg["L"] // 3, 7

    def batch(seed):
        gen = torch.Generator().manual_seed(seed)
        return torch.randn(B, L, E, generator=gen).cuda(), (torch.rand(B, T, A, generator=gen) * 3.0 - 1.5).cuda()

    runs = []
    for graphed in (False, True):
        torch.manual_seed(cfg["seed"])
        net = GPTBackbone(embed_dim=E, context_length=L, causal=bool(cfg["causal"]), num_layers=cfg["layers"], num_heads=cfg["H"],
                          attn_dropout=0.0, block_output_dropout=0.0).cuda().train().set_matmul_precision("bf16")
        head = _action_head(E, A, seed=42).cuda().train().set_matmul_precision("bf16")
        params = list(net.parameters()) + list(head.parameters())
        opt = optim.Adam(params, lr=torch.tensor(1e-3, device="cuda"), max_grad_norm=1.0)
        loss_fn = lambda x, a: head.losses(net(x)[:, -T:], a, *MIXED)["action_loss"]      # noqa: E731
        if graphed:
            step = GraphedPolicyStep(loss_fn, params, opt, batch(0), warmup=3)
        record = []
        for k in (1, 2):
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
        assert all(torch.equal(p, q) for p, q in zip(eager, replay)), f"replay {k} differs from eager step {k}"
    assert not torch.equal(runs[0][0][-1], runs[0][1][-1])                                  # the head's bias moved
    # ... and the step is the mode's: the fp32 head on the same backbone gives another loss
    with torch.no_grad():
        x, a = batch(1)
        both = loss_fn(x, a)
        head.set_matmul_precision("fp32")
        assert not torch.equal(loss_fn(x, a), both)


def test_prompted_policy_sets_backbone_and_head_together():
    from lipvq_vae_amd.embedding import ICLInputEmbedding
    from lipvq_vae_amd.gpt import GPTBackbone
    from lipvq_vae_amd.icl import PromptedPolicy
    T, E, DIN, A, B = 3, 64, 16, 7, 5
    torch.manual_seed(21)
    emb = ICLInputEmbedding(DIN, E, T, emb_dropout=0.1).cuda().eval()
    net = GPTBackbone(E, 3 * T, num_layers=2, num_heads=4).cuda().eval()
    head = _action_head(E, A, seed=22).cuda().eval()
    gen = torch.Generator().manual_seed(23)
    obs, ctx_obs, ctx_act = (torch.randn(B, T, DIN, generator=gen).cuda() for _ in range(3))
    policy = PromptedPolicy(emb, net, head)
    policy.set_prompt(ctx_obs, ctx_act)
    fp32 = policy(obs).clone()
    assert policy.set_matmul_precision("bf16") is policy
    assert net.matmul_precision == "bf16" and head.matmul_precision == "bf16"
    for call in (policy, policy.features):
        with pytest.raises(RuntimeError, match=r"call set_prompt\(\) first"):
            call(obs)
    policy.set_prompt(ctx_obs, ctx_act)
    with torch.no_grad():
        want = head(net(emb(obs, ctx_obs, context_actions=ctx_act))[:, 2 * T:])
    got = policy(obs)
    assert got.shape == (B, T, A) and torch.equal(got, want) and not torch.equal(got, fp32)
    policy.set_matmul_precision("fp32").set_prompt(ctx_obs, ctx_act)
    assert torch.equal(policy(obs), fp32)                                           # "fp32" restores the default bit for bit
