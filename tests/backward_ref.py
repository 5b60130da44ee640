"""float64 restatement of the backward pass (include/lipvq.h, "backward" section), for tests/test_gpu_backward.py,
tests/test_oracle_backward.py and tests/test_gpu_fused.py.

torch on the CPU, float64, stock ops and autograd only: nothing here is shared with the HIP kernels or with the C oracle
(oracle/lipvq_oracle.c), whose gradients were written from the same derivation as the kernels'.  Inputs may be numpy arrays or
tensors on any device; results are float64 CPU tensors.

Error budgets.  ``dot_bound`` is the classical forward bound of an fp32 dot product of length L in ANY summation order
(Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5): |fl(a.b) - a.b| <= gamma_L |a|.|b|, gamma_L = L u / (1 - L u),
u = 2^-24.  A fused multiply-add chain (what the MFMA runs) makes one rounding per term and is inside it.  The budget functions
below carry that bound through the closed forms; they take no number from the code under test.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_GELU, ACT_SIGMOID, ACT_RELU = 0, 1, 2, 3
U32 = 2.0 ** -24                      # unit roundoff of fp32


def f64(t):
    """float64 CPU tensor of a numpy array / tensor (None stays None)."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    return t.detach().cpu().double()


# delta_act of the budgets below: the absolute error of the fp32 activation derivatives against the exact float64 forms (how they
# were measured, and the device's allowance for its straight-line GELU': tests/test_gpu_backward.py, which re-exports them)
GELU_GRAD_ABS_ERR = 1.51e-7
SIGMOID_GRAD_ABS_ERR = 8.9e-8
GELU_DEVICE_ALLOWANCE = 3e-7
DELTA_ACT = {ACT_NONE: 0.0, ACT_RELU: 0.0, ACT_SIGMOID: SIGMOID_GRAD_ABS_ERR, ACT_GELU: GELU_GRAD_ABS_ERR + GELU_DEVICE_ALLOWANCE}


def gamma(L):
    L = float(L)
    return L * U32 / (1.0 - L * U32)


def dot_bound(absA, absB, L):
    """gamma_L (|A| . |B|) in float64: the forward error bound of every element of the fp32 product A . B whose contraction
    length is L (absA [.., L], absB [L, ..], both non-negative)."""
    return gamma(L) * (f64(absA) @ f64(absB))


def ulp32(x):
    """Spacing of fp32 at |x| (float64 tensor): what rounding the exact result to fp32 may cost, twice over."""
    a = f64(x).abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


# ---- activations ------------------------------------------------------------------------------------------------------------

def act_ref(v, act):
    v = f64(v)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    return v


def act_grad_ref(v, act):
    """d act / d v at the pre-activation v, exact float64 forms: Phi(v) + v phi(v), s (1 - s), v > 0, 1."""
    v = f64(v)
    if act == ACT_GELU:
        return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)
    if act == ACT_SIGMOID:
        s = torch.sigmoid(v)
        return s * (1.0 - s)
    if act == ACT_RELU:
        return (v > 0).double()                    # 0 at +0.0 and -0.0, as torch's threshold_backward
    return torch.ones_like(v)


def act_sweep():
    """The dense pre-activation sweep of test_gelu_derivative_on_device_tracks_the_canonical_one (fp32 numpy)."""
    return np.concatenate([np.linspace(-12, 12, 200001), [4.2426405, 4.2426410, -4.2426405, 0.0, 1e-30, 88.0, -88.0]]).astype(np.float32)


PLANTED = np.array([0.0, -0.0, 9.0, -9.0, 40.0, -40.0, 100.0, -100.0], np.float32)


# ---- the three-layer stack ---------------------------------------------------------------------------------------------------

def mlp3_bwd_ref(gy, pre, W0, W1, W2, acts):
    """(g2, g1, g0, gx) of y = act2(W2 act1(W1 act0(W0 x + b0) + b1) + b2): dL/d(pre-activation) of the three layers and
    dL/dx from gy = dL/dy and the saved pre-activations (pre[2] may be None when acts[2] is the identity)."""
    gy, W0, W1, W2 = f64(gy), f64(W0), f64(W1), f64(W2)
    g2 = gy if acts[2] == ACT_NONE else gy * act_grad_ref(pre[2], acts[2])
    g1 = (g2 @ W2) * act_grad_ref(pre[1], acts[1])
    g0 = (g1 @ W1) * act_grad_ref(pre[0], acts[0])
    return g2, g1, g0, g0 @ W0


def layer_ref_and_budget(g_in, W, pre, act, delta_act):
    """One link of the chain, from the kernel's OWN upstream gradient g_in [N, J] and W [J, Kd]:
    (reference (g_in . W) * act'(pre) in float64, allowed |error| per element)
        allowed = 2 dot_bound(|g_in|, |W|, J) |act'| + |dot| delta_act + one fp32 ulp of the result
    (2: the rounding of the product with act' and of the store, each at most u |result| <= dot_bound at J >= 1;
    delta_act: the absolute error of the fp32 activation derivative, a measured constant of the test file)."""
    g_in, W = f64(g_in), f64(W)
    dot = g_in @ W
    d = act_grad_ref(pre, act) if pre is not None else torch.ones_like(dot)
    ref = dot * d
    allowed = 2.0 * dot_bound(g_in.abs(), W.abs(), W.shape[0]) * d.abs() + dot.abs() * delta_act + ulp32(ref)
    return ref, allowed


def elementwise_ref_and_budget(g, pre, act, delta_act):
    """g * act'(pre): a "dot product" of length 1."""
    g = f64(g)
    d = act_grad_ref(pre, act)
    ref = g * d
    return ref, 2.0 * gamma(1) * g.abs() * d.abs() + g.abs() * delta_act + ulp32(ref)


# ---- weight gradient, scaled difference ----------------------------------------------------------------------------------------

def wgrad_ref(G, H, h_act=ACT_NONE, hidx=None):
    """(gW [J, Kd], gb [J]) = (G^T act(H), column sums of G); with hidx row n of H is H[hidx[n]]."""
    G, H = f64(G), f64(H)
    if hidx is not None:
        H = H[hidx.detach().cpu().long()]
    return G.t() @ act_ref(H, h_act), G.sum(0)


def scaled_diff_ref(a, b, alpha, gscale=None, c=None):
    """alpha * gscale * (a - b) + c in float64."""
    out = float(alpha) * (1.0 if gscale is None else float(f64(gscale).reshape(-1)[0])) * (f64(a) - f64(b))
    return out if c is None else out + f64(c)


def scaled_diff_fp32(a, b, alpha, gscale=None, c=None):
    """The same expression in fp32 with every operation rounded on its own (no contraction): f = alpha * gscale,
    v = f * (a - b), v + c -- what lipvq_scaled_diff_f32 promises bit for bit.  fp32 CPU tensor."""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    f = torch.tensor(float(alpha), dtype=torch.float32)
    if gscale is not None:
        f = f * gscale.detach().cpu().float().reshape(())
    v = f * (a - b)
    return v if c is None else v + c.detach().cpu().float()


# ---- Lipschitz normalisation ---------------------------------------------------------------------------------------------------

def lipschitz_bwd_ref(W, ci, gWn):
    """(gW, gci, ratio) of Wn = W * minimum(1, softplus(ci)[:, None] / |W|.sum(1, keepdim=True)) by autograd; ratio [D] =
    softplus(ci) / sum|W| in float64 (inf for an all-zero row).  For an all-zero row autograd multiplies a zero upstream
    gradient by d(sp / s)/ds = -inf and returns NaN; the row is inactive (scale 1 on a neighbourhood in ci), so its
    gradients are the defined ones: gW = gWn, gci = 0."""
    W = f64(W).clone().requires_grad_(True)
    ci = f64(ci).clone().requires_grad_(True)
    gWn = f64(gWn)
    rowsum = W.abs().sum(1, keepdim=True)
    ratio = F.softplus(ci).unsqueeze(1) / rowsum
    Wn = W * torch.minimum(torch.ones((), dtype=torch.float64), ratio)
    Wn.backward(gWn)
    gW, gci = W.grad.clone(), ci.grad.clone()
    zero = rowsum.detach().reshape(-1) == 0
    gW[zero] = gWn[zero]
    gci[zero] = 0.0
    return gW, gci, ratio.detach().reshape(-1)


def lipschitz_band(H):
    """Rows whose float64 ratio is within this of 1 may legitimately take the other branch in fp32: the fp32 row sum of H
    terms is (H - 1) u off at most, softplus and the division a few u more."""
    return 4.0 * H * U32


# relative error allowed to the fp32 softplus / sigmoid of ci: lq_softplus measures 4.45 u and lq_sigmoid 2.39 u against float64
# over 400 001 points of ci in [-30, 88] (tests/test_oracle_backward.py::test_measured_constants_hold re-measures both)
LIP_FUNC_REL = 5.0 * U32


def lipschitz_budget(W, ci, gWn):
    """Allowed |error| of (gW, gci) for an fp32 evaluation of the closed form on the ACTIVE rows
        sc = sp / s,  k = -gsc sp / s^2,  gW_j = gWn_j sc + k sign(w_j),  gci = gsc sigmoid(ci) / s
    with s = sum|w_j| and gsc = sum gWn_j w_j the two length-H sums: E_s = dot_bound(|W|, 1, H), E_g = dot_bound(|gWn|, |W|, H),
    eps = LIP_FUNC_REL for softplus / sigmoid.  First order in the errors:
        d(sc)  = sc (E_s / s + eps)
        d(k)   = (sp / s^2) E_g + |k| (2 E_s / s + eps)
        d(gW)  = |gWn_j| d(sc) + d(k) + ulp(gW_j)
        d(gci) = (sigmoid / s) E_g + |gci| (E_s / s + eps) + ulp(gci)
    Inactive rows are exact (gW = gWn * 1, gci = 0) and get no allowance here: the tests compare them with ==."""
    W, ci, gWn = f64(W), f64(ci), f64(gWn)
    H = W.shape[1]
    s = W.abs().sum(1)
    s = torch.where(s == 0, torch.ones_like(s), s)              # (all-zero rows are inactive: unused)
    gsc = (gWn * W).sum(1)
    E_s = gamma(H) * s
    E_g = gamma(H) * (gWn.abs() * W.abs()).sum(1)
    sp, sg = F.softplus(ci), torch.sigmoid(ci)
    sc, k = sp / s, -gsc * sp / (s * s)
    d_sc = sc * (E_s / s + LIP_FUNC_REL)
    d_k = sp / (s * s) * E_g + k.abs() * (2.0 * E_s / s + LIP_FUNC_REL)
    gW = gWn * sc[:, None] + k[:, None] * torch.sign(W)
    gci = gsc * sg / s
    d_gW = gWn.abs() * d_sc[:, None] + d_k[:, None] + ulp32(gW)
    d_gci = sg / s * E_g + gci.abs() * (E_s / s + LIP_FUNC_REL) + ulp32(gci)
    return d_gW, d_gci


def mixed_ci(W, seed, lo=0.25, hi=4.0):
    """fp32 ci [D] such that softplus(ci) / sum|W| is log-uniform in [lo, hi] per row: about half the rows clamp."""
    W = f64(W)
    rng = np.random.default_rng(seed)
    ratio = np.exp(rng.uniform(math.log(lo), math.log(hi), W.shape[0]))
    return ci_for_ratio(W, ratio)


def ci_for_ratio(W, ratio):
    """fp32 ci with softplus(ci) = ratio * sum|W| per row (rows without weight get ci = 0)."""
    s = f64(W).abs().sum(1).numpy()
    target = np.maximum(np.asarray(ratio, np.float64) * s, 1e-30)
    ci = np.where(target > 30.0, target, np.log(np.expm1(np.minimum(target, 30.0))))      # inverse softplus
    return np.where(s == 0, 0.0, ci).astype(np.float32)


def lipschitz_case(D, H, seed):
    """Seeded (W [D, H], ci [D], gWn [D, H]) fp32 numpy arrays for the Lipschitz backward tests, and the row roles:
    rows at a log-uniform ratio in [0.25, 4] (mixed branches in one matrix, ragged 16-row groups at D % 16 != 0), then -- as far as
    D has room, from the last row backwards -- six rows at ratio 1 +- {1e-3, 2e-4, max(1e-5, 8 H u)} (close to the switch but
    outside lipschitz_band), a row with exact-zero entries, an all-zero row, and six rows at ci = -30, -5, 0, 5, 30, 88."""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((D, H)).astype(np.float32)
    gWn = rng.standard_normal((D, H)).astype(np.float32)
    ci = mixed_ci(W, seed + 1)
    roles = {}
    free = list(range(D - 1, 0, -1))                            # row 0 always stays a plain random row
    near = max(1e-5, 8.0 * H * U32)
    for off in (1e-3, -1e-3, 2e-4, -2e-4, near, -near):
        if not free:
            break
        r = free.pop(0)
        ci[r] = ci_for_ratio(W[r:r + 1], [1.0 + off])[0]
        roles.setdefault("near", []).append(r)
    if free:
        r = free.pop(0)
        W[r, ::3] = 0.0
        W[r, 1] = -0.0
        ci[r] = ci_for_ratio(W[r:r + 1], [0.5])[0]               # active: the sign term is live on the non-zero entries
        roles["zero_entries"] = r
    if free:
        r = free.pop(0)
        W[r] = 0.0
        ci[r] = 1.0
        roles["zero_row"] = r
    for v in (-30.0, -5.0, 0.0, 5.0, 30.0, 88.0):
        if not free:
            break
        r = free.pop(0)
        ci[r] = v
        roles.setdefault("fixed_ci", []).append(r)
    return W, ci, gWn, roles


LIPSCHITZ_D = (1, 15, 16, 17, 37, 64, 208, 512)
LIPSCHITZ_H = (32, 96, 128, 200, 256)


# ---- whole modules ---------------------------------------------------------------------------------------------------------

def llfq_encode64(p, x):
    """x [N, A] -> z_e [N, D] of LLFQVAE_V4 (encoder, Lipschitz normalisation, sigmoid) on a dict of float64 tensors."""
    h = F.gelu(F.linear(x, p["encoder.0.weight"], p["encoder.0.bias"]))
    h = F.gelu(F.linear(h, p["encoder.2.weight"], p["encoder.2.bias"]))
    W, b, ci = p["to_latent.W"], p["to_latent.b"], p["to_latent.ci"]
    rowsum = torch.sum(torch.abs(W), dim=1, keepdim=True)
    scale = torch.minimum(torch.ones((), dtype=W.dtype), F.softplus(ci).unsqueeze(1) / rowsum)
    return torch.sigmoid(torch.matmul(h, (W * scale).T) + b)


def autograd_grads(params, x, idx, kind, gscale, commitment_cost=0.25):
    """Parameter gradients of gscale * loss by torch autograd on the CPU in float64 with the code indices given (the [N, K, D]
    distance tensor of the reference's argmin is 17 GB at large batches; index parity is what other tests are for).
    kind "llfq": LLFQVAE_V4's loss, "vq": the plain VQVAE's.  Returns (dict of float64 gradients, info); info["relu_margin"] is
    the smallest |pre-activation| under a ReLU ("vq"; inf otherwise): where it is below the fp32 forward's error the two
    precisions may sit on different sides of the kink."""
    p = {k: f64(v).clone().requires_grad_(True) for k, v in params.items()}
    x = f64(x)
    idx = torch.as_tensor(idx).detach().cpu().long()
    margin = float("inf")
    if kind == "llfq":
        z_e = llfq_encode64(p, x)
        z_q = p["quantizer.codebook"][idx]
        h = F.gelu(F.linear(z_q, p["decoder.0.weight"], p["decoder.0.bias"]))
        h = F.gelu(F.linear(h, p["decoder.2.weight"], p["decoder.2.bias"]))
        x_rec = F.linear(h, p["to_output.weight"], p["to_output.bias"])
        loss = F.mse_loss(x_rec, x) + 0.25 * F.mse_loss(z_q.detach(), z_e) + 0.25 * F.mse_loss(z_q, z_e.detach())
    else:
        h = x
        for i in (0, 2, 4):
            pre = F.linear(h, p[f"encoder.{i}.weight"], p[f"encoder.{i}.bias"])
            margin = min(margin, float(pre.detach().abs().min()))
            h = F.relu(pre)
        z_e = h
        z_q = F.embedding(idx, p["embedding.weight"])
        q_loss = F.mse_loss(z_q, z_e.detach()) + float(commitment_cost) * F.mse_loss(z_q.detach(), z_e)
        h = z_e + (z_q - z_e).detach()
        for i in (0, 2, 4):
            pre = F.linear(h, p[f"decoder.{i}.weight"], p[f"decoder.{i}.bias"])
            margin = min(margin, float(pre.detach().abs().min()))
            h = F.relu(pre)
        loss = F.mse_loss(h, x) + q_loss
    (loss * gscale).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}
    return grads, {"relu_margin": margin}


def oracle_grads_cpu(model, xt, kind, gscale):
    """autograd_grads for a module on the GPU after its forward: parameters from the module, code indices from the launch
    (model.last_indices); float64 so that the comparison sees the launches' rounding only -- a sequential fp32 index_add_ over
    the thousands of rows of one code is itself 1e-5 off.  fp32 CPU tensors."""
    grads, _ = autograd_grads(dict(model.named_parameters()), xt, model.last_indices, kind, gscale,
                              commitment_cost=float(getattr(model, "commitment_cost", 0.25)))
    return {k: v.float() for k, v in grads.items()}


# module-level cases (A, D, K, hidden) and batch sizes shared by the GPU and the CPU-oracle tests
MODULE_SHAPES = ((7, 64, 256, 128), (12, 208, 128, 128), (9, 48, 200, 32), (5, 37, 64, 192), (7, 256, 300, 128))
MODULE_ROWS = (80, 333, 500)
# a ReLU pre-activation of the float64 forward closer to zero than this may be on the other side of the kink in fp32 (the fp32
# forward's error at these widths: <= 256 terms of magnitude O(0.1), a few 1e-7): inputs are drawn until none is
RELU_BAND = 1e-6
