"""Planted NaN / +inf / -inf inputs for the kernels that feed the policy, their float64 torch restatements, the two cones of
outputs a plant may reach and the rule an implementation is judged by -- plain seeded torch on the CPU, no GPU.
tests/test_gpu_nonfinite.py runs the kernels on these inputs; tests/test_nonfinite_cases_host.py checks the cones and the judge.

A GROUP is one operation at one shape with clean seeded inputs, a list of plants (input name, index) and a restatement
``ref(inputs, loose) -> {output name: tensor}`` in the dtype of its inputs.  A CASE is a group with ONE element of one input
set to NaN, +inf or -inf.  The restatement exists in two formulations:

  strict   masks are applied by SELECTION (``where`` / indexing): a closed or dropped attention position contributes nothing,
           whatever its key or value row holds -- the mathematical dependence;
  loose    stock torch's formulation (``gpt_ref.attention_ref``): a masked probability of exactly 0 still multiplies its value
           row, and 0 * NaN = NaN.

Operations without a mask have one formulation (``masked = False``: the two cones must then be equal).  A cone is traced with
the strongest tracer there is: the outputs that are NaN when the plant is a NaN, together with those the case's own value moves.
``judge`` holds a result to: inside the strict cone, non-finite wherever the float64 strict reference is (a reference +-inf
admits only the same sign or a NaN) and finite and within the operation's tolerance of it elsewhere; outside the loose cone,
bit-equal to the same call on the clean input; between the two, either (or the loose reference's verdict).

Tolerances are the suite's own: ``max(TOL, REF_FACTOR * dev)`` of the output's scale with ``xf_edge_inputs.FWD_TOL`` /
``BWD_TOL`` / ``REF_FACTOR`` (the constants of test_gpu_gpt.py, test_gpu_gmm.py, test_gpu_action_head.py and
test_gpu_embed_edges.py), ``dev`` being the stock-fp32 restatement's own distance from float64 on the clean inputs.

The sampler's restatement adds one rule to ``gmm_ref.sample_by_inverse_cdf``: a row whose mixture weights are not all finite
has no defined draw and its sample is NaN (stock torch compares u with a NaN CDF, finds every comparison false and returns
mode 0's finite draw -- a swallow in the reference itself).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import action_head_ref
import backward_ref as R
import embed_ref
import gmm_ref
import gpt_ref
import xf_edge_inputs as X
from oracle import lipvq_oracle as O

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
VALUES = {"nan": NAN, "+inf": PINF, "-inf": NINF}
ACTS = {"none": R.ACT_NONE, "gelu": R.ACT_GELU, "sigmoid": R.ACT_SIGMOID, "relu": R.ACT_RELU}
TORCH_ACT = {R.ACT_NONE: lambda v: v, R.ACT_GELU: F.gelu, R.ACT_SIGMOID: torch.sigmoid, R.ACT_RELU: F.relu}
FWD, BWD = X.FWD_TOL, X.BWD_TOL


def _gen(*key):
    return X._gen("nonfinite", *key)


def _differs(a, b):
    return ~((a == b) | (a.isnan() & b.isnan()))


def _to(inputs, dtype):
    return {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in inputs.items()}


class Group:
    """One operation at one shape: clean inputs, plants, restatement, tolerances (output name -> FWD | BWD)."""

    def __init__(self, name, op, params, inputs, plants, ref, tol, masked=False, values=("nan", "+inf", "-inf"), touch=None,
                 unordered=()):
        self.name, self.op, self.params, self.inputs, self.plants, self.ref, self.tol = name, op, params, inputs, plants, ref, tol
        self.masked, self.values = masked, values
        # outputs the kernel accumulates with fp32 atomics in an order that differs from run to run (two CLEAN calls differ in the
        # last bits): "bit-equal to the clean call" is not defined for them, so outside the cone they are held to the in-cone rule
        # against the float64 reference instead -- finite and within the tolerance; a 0 * NaN leak still fails
        self.unordered = frozenset(unordered)
        self._traces = {}
        self.touch = touch         # (key, index) -> {output: index} that depends on the plant even where no value shows it (relu'(-inf) = relu'(-1))

    def run(self, inputs, loose, dtype):
        with torch.enable_grad():
            out = self.ref(_to(inputs, dtype), loose and self.masked, **self.params)
        return {k: v.detach() for k, v in out.items()}

    @functools.cached_property
    def clean(self):
        """{'strict' | 'loose' | 'fp32': outputs on the clean inputs}, dev and bound per output"""
        c = {"strict": self.run(self.inputs, False, torch.float64), "fp32": self.run(self.inputs, True, torch.float32)}
        c["loose"] = self.run(self.inputs, True, torch.float64) if self.masked else c["strict"]
        for k, v in c["strict"].items():
            assert bool(v.isfinite().all()), f"{self.name}: the clean reference's {k} is not finite"
        c["dev"] = {k: X.rel(c["fp32"][k].numpy(), c["strict"][k].numpy()) for k in c["strict"]}
        c["bound"] = {k: X.bound(self.tol[k], c["dev"][k]) for k in c["strict"]}
        return c

    def cases(self):
        return [Case(self, key, index, v) for key, index in self.plants for v in self.values]

    def nan_trace(self, case, loose):
        """the float64 outputs with a NaN at the case's plant: one evaluation per (plant, formulation), shared by its values"""
        key = (case.key, case.index, loose)
        if key not in self._traces:
            self._traces[key] = self.run(case.planted(NAN), loose, torch.float64)
        return self._traces[key]

    def __repr__(self):
        return self.name


class Case:
    def __init__(self, group, key, index, value_name):
        self.group, self.key, self.index, self.value_name, self.value = group, key, tuple(index), value_name, VALUES[value_name]
        self.name = f"{group.name} {key}{list(index)}={value_name}"

    def planted(self, value=None):
        """the group's inputs with the one element set (the other tensors are shared, read-only)"""
        d = dict(self.group.inputs)
        t = d[self.key].clone()
        t[self.index] = self.value if value is None else value
        d[self.key] = t
        return d

    @functools.cached_property
    def analysis(self):
        """ref (strict, float64, the case's value), ref_loose, and the two cones, per output"""
        g = self.group
        out = {}
        for form in ("strict", "loose") if g.masked else ("strict",):
            loose = form == "loose"
            act = g.nan_trace(self, loose) if self.value != self.value else g.run(self.planted(), loose, torch.float64)
            nan = act if self.value != self.value else g.nan_trace(self, loose)
            out["ref_" + form] = act
            out[form] = {k: nan[k].isnan() | _differs(act[k], g.clean[form][k]) for k in act}
            for k, i in (g.touch(self.key, self.index) if g.touch else {}).items():
                out[form][k][i] = True
        if not g.masked:
            out["ref_loose"], out["loose"] = out["ref_strict"], out["strict"]
        return out

    def stock_fp32(self):
        """(got, clean_got) of the stock-torch fp32 restatement: what judge must accept"""
        return self.group.run(self.planted(), True, torch.float32), self.group.clean["fp32"]

    def cone_sizes(self):
        a = self.analysis
        return {k: (int(a["strict"][k].sum()), int(a["loose"][k].sum()), a["strict"][k].numel()) for k in a["strict"]}

    def __repr__(self):
        return self.name


def _np32(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    t = np.asarray(t, np.float32)
    return np.ascontiguousarray(t).reshape(t.shape)                 # (ascontiguousarray alone makes a 0-d array 1-d)


def _in_rule(got, ref, bound):
    """per element: the rule inside a cone against the float64 reference `ref`"""
    ref_fin = np.isfinite(ref)
    scale = float(np.abs(ref[ref_fin]).max()) if ref_fin.any() else 0.0
    with np.errstate(invalid="ignore"):
        close = np.isfinite(got) & (np.abs(got.astype(np.float64) - np.where(ref_fin, ref, 0.0)) <= bound * max(scale, 1e-30))
        sign_ok = np.isnan(got) | np.isnan(ref) | (np.isinf(got) & (np.sign(got) == np.sign(ref)))
    return np.where(ref_fin, close, ~np.isfinite(got) & sign_ok)


def judge(got, clean_got, case):
    """Raises AssertionError naming the first offending elements; returns the cone sizes {output: (strict, loose, all)}.
    got / clean_got: {output name: fp32 array or tensor} of the planted and of the clean call."""
    a, g = case.analysis, case.group
    problems = []
    for k in a["ref_strict"]:
        gk, ck = _np32(got[k]), _np32(clean_got[k])
        ref_s, ref_l = a["ref_strict"][k].numpy(), a["ref_loose"][k].numpy()
        assert gk.shape == ref_s.shape == ck.shape, (case.name, k, gk.shape, ref_s.shape, ck.shape)
        strict, loose = a["strict"][k].numpy(), a["loose"][k].numpy()
        bound = g.clean["bound"][k]
        inside = _in_rule(gk, ref_s, bound)
        same = inside if k in g.unordered else gk.view(np.uint32) == ck.view(np.uint32)
        # (inside the strict cone the stock formulation's verdict is admitted as well: with a keep mask an element may depend on
        # the plant through a finite path AND be reached by a 0 * NaN product; for an operation without a mask ref_l is ref_s)
        either = inside | _in_rule(gk, ref_l, bound)
        ok = np.where(strict, either, np.where(loose, either | same, same))
        if not ok.all():
            bad = np.argwhere(~ok)
            i = tuple(bad[0])
            zone = "inside the strict cone" if strict[i] else "between the cones" if loose[i] else "outside the loose cone"
            problems.append(f"{k}: {len(bad)} elements, first at {list(i)} ({zone}): got {gk[i]!r}, clean {ck[i]!r}, float64 {ref_s[i]!r}, "
                            f"bound {bound:.1e} of the scale")
    if problems:
        raise AssertionError(f"{case.name}: " + "; ".join(problems))
    return case.cone_sizes()


# ---------------------------------------------------------------------------------------------------
# Linear, the three-layer stack, elementwise backward, weight gradient
# ---------------------------------------------------------------------------------------------------

def linear_ref(t, loose, act):
    return {"y": TORCH_ACT[act](F.linear(t["x"], t["W"], t["b"]))}


def _linear_group(N, Kin, E, act_name, plants):
    g = _gen("linear", N, Kin, E)
    inputs = {"x": torch.randn(N, Kin, generator=g), "W": torch.randn(E, Kin, generator=g) / math.sqrt(Kin), "b": torch.randn(E, generator=g)}
    return Group(f"linear N={N} Kin={Kin} E={E} {act_name}", "linear", {"act": ACTS[act_name]}, inputs, plants, linear_ref, {"y": FWD})


LINEAR_SMALL = (33, 65, 129)


def linear_groups():
    N, Kin, E = LINEAR_SMALL
    small = [_linear_group(N, Kin, E, a, [("x", (0, 0)), ("x", (32, 64)), ("W", (0, 0)), ("W", (128, 64)), ("b", (128,))]) for a in ACTS]
    big = [_linear_group(N, Kin, E, "gelu", [("x", (N - 1, Kin - 1)), ("W", (E - 1, 0))]) for N, Kin, E in embed_ref.LINEAR_BIG[:2]]     # (the two smallest: 128 x 128 and 256 x 64 tiles)
    return small + big


MLP3_N = (70, 4097, 65536 + 45)                        # test_gpu_mlp3_edges.py's: one sub-tile per workgroup, two, mlp3_lds_kernel
MLP3_TRIPLES = {"relu": (R.ACT_RELU,) * 3, "gelu": (R.ACT_GELU,) * 3, "sigmoid": (R.ACT_SIGMOID,) * 3}
MLP3_WIDTHS = (7, 64, 128, 37)


def mlp3_ref(t, loose, acts):
    out, h = {}, t["x"]
    for i in range(3):
        pre = F.linear(h, t[f"W{i}"], t[f"b{i}"])
        out[f"pre{i}"] = pre
        h = TORCH_ACT[acts[i]](pre)
    out["y"] = h
    return out


def mlp3_groups():
    K0, J0, J1, J2 = MLP3_WIDTHS
    groups = []
    for N in MLP3_N:
        g = _gen("mlp3", N)
        inputs = {"x": torch.randn(N, K0, generator=g), "W0": 0.5 * torch.randn(J0, K0, generator=g), "b0": torch.randn(J0, generator=g),
                  "W1": 0.2 * torch.randn(J1, J0, generator=g), "b1": torch.randn(J1, generator=g),
                  "W2": 0.2 * torch.randn(J2, J1, generator=g), "b2": torch.randn(J2, generator=g)}
        plants = [("x", (r, (3 * n + 1) % K0)) for n, r in enumerate((0, 31, 32, N - 1))]
        for name, acts in MLP3_TRIPLES.items():
            groups.append(Group(f"mlp3 N={N} {name}", "mlp3", {"acts": acts}, inputs, plants, mlp3_ref,
                                {"y": FWD, "pre0": FWD, "pre1": FWD, "pre2": FWD}))
    return groups


ACT_BWD_N = 130


def act_bwd_ref(t, loose, act):
    pre = t["pre"].clone().requires_grad_(True)
    TORCH_ACT[act](pre).backward(t["g"])
    return {"out": pre.grad}


def act_bwd_groups():
    g = _gen("act_bwd")
    inputs = {"pre": 2.0 * torch.randn(ACT_BWD_N, generator=g), "g": torch.randn(ACT_BWD_N, generator=g)}
    neg = int((inputs["pre"] < 0).nonzero()[0])                    # (the first negative and the last positive pre-activation)
    pos = int((inputs["pre"] > 0).nonzero()[-1])
    plants = [("pre", (neg,)), ("pre", (pos,)), ("g", (neg,)), ("g", (pos,))]
    return [Group(f"act_bwd {a}", "act_bwd", {"act": ACTS[a]}, inputs, plants, act_bwd_ref, {"out": BWD}, touch=lambda key, index: {"out": index})
            for a in ("gelu", "sigmoid", "relu")]


WGRAD_SHAPE = (129, 196, 100)                          # N, J, Kd


def wgrad_ref(t, loose, h_act):
    return {"gW": t["G"].t() @ TORCH_ACT[h_act](t["H"]), "gb": t["G"].sum(0)}


def wgrad_groups():
    N, J, Kd = WGRAD_SHAPE
    g = _gen("wgrad")
    inputs = {"G": torch.randn(N, J, generator=g), "H": torch.randn(N, Kd, generator=g)}
    return [Group(f"wgrad N={N} J={J} Kd={Kd} h_act={a}", "wgrad", {"h_act": ACTS[a]}, inputs, [("G", (N - 1, J - 1)), ("H", (0, Kd - 1))],
                  wgrad_ref, {"gW": BWD, "gb": BWD}) for a in ("none", "relu")]


# ---------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------

LN_SHAPES = ((5, 252), (5, 1024))


def layernorm_ref(t, loose):
    E = t["a"].shape[-1]
    s = (t["a"] + t["b"]).clone().requires_grad_(True)
    w, bias = t["w"].clone().requires_grad_(True), t["bias"].clone().requires_grad_(True)
    y = F.layer_norm(s, (E,), w, bias, X.LN_EPS)
    (y * t["gy"]).sum().backward()
    with torch.no_grad():
        sd = s.detach()
        mean = sd.mean(-1, keepdim=True)
        rstd = torch.rsqrt(sd.var(-1, unbiased=False, keepdim=True) + X.LN_EPS)
    return {"s": sd, "y": y, "xhat": (sd - mean) * rstd, "rstd": rstd[:, 0], "gs": s.grad + t["gres"], "gw": w.grad, "gb": bias.grad}


def layernorm_groups():
    groups = []
    for N, E in LN_SHAPES:
        g = _gen("layernorm", N, E)
        inputs = {"a": torch.randn(N, E, generator=g), "b": torch.randn(N, E, generator=g), "w": 1 + 0.1 * torch.randn(E, generator=g),
                  "bias": 0.1 * torch.randn(E, generator=g), "gy": torch.randn(N, E, generator=g), "gres": torch.randn(N, E, generator=g)}
        plants = [("a", (2, E - 1)), ("b", (2, 0)), ("w", (E - 1,)), ("gy", (2, 0)), ("gres", (4, 1))]
        groups.append(Group(f"layernorm N={N} E={E}", "layernorm", {}, inputs, plants, layernorm_ref,
                            {"s": FWD, "y": FWD, "xhat": FWD, "rstd": FWD, "gs": BWD, "gw": BWD, "gb": BWD}))
    return groups


# ---------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------

def _sel_matmul(P, sel, V):
    """sum over j with sel[.., i, j] of P[.., i, j] V[.., j, :]: an unselected position contributes nothing, whatever V's row
    holds.  P is 0 where sel is false.  The finite part of V goes through one matmul (0 * finite = 0 exactly); the few rows of V
    with a non-finite element are added for their selected partners alone."""
    fin = V.isfinite()
    out = P @ torch.where(fin, V, torch.zeros_like(V))
    for idx in (~fin).any(-1).nonzero().tolist():
        *lead, j = idx
        lead = tuple(lead)
        s = sel[lead][:, j]
        extra = torch.where(fin[lead][j], torch.zeros_like(V[lead][j]), V[lead][j])
        o = out[lead]
        o[s] = o[s] + P[lead][s, j, None] * extra
    return out


def attention_strict(qkv, gout, H, causal, keep, keep_prob):
    """out, lse and the gradient of (out * gout).sum() with respect to qkv [B, L, 3E], every mask applied by selection."""
    B, L, E3 = qkv.shape
    E = E3 // 3
    dh = E // H
    scale = 1.0 / math.sqrt(dh)
    q, k, v = (qkv[..., i * E:(i + 1) * E].view(B, L, H, dh).transpose(1, 2) for i in range(3))
    go = gout.view(B, L, H, dh).transpose(1, 2)
    is_open = (gpt_ref.causal_mask(L, causal) != 0).expand(B, H, L, L)
    sel = is_open if keep is None else is_open & (keep != 0)
    sc = ((q @ k.transpose(-2, -1)) * scale).masked_fill(~is_open, NINF)
    lse = torch.logsumexp(sc, -1)
    zero = torch.zeros_like(sc)
    P = torch.where(is_open, torch.softmax(sc, -1), zero)
    Pk = torch.where(sel, P / keep_prob, zero)
    out = _sel_matmul(Pk, sel, v)
    delta = (go * out).sum(-1, keepdim=True)
    dP = torch.where(sel, (go @ v.transpose(-2, -1)) / keep_prob, zero)
    dS = torch.where(is_open, P * (dP - delta), zero)
    dq = scale * _sel_matmul(dS, is_open, k)
    dk = scale * _sel_matmul(dS.transpose(-2, -1), is_open.transpose(-2, -1), q)
    dv = _sel_matmul(Pk.transpose(-2, -1), sel.transpose(-2, -1), go)
    back = lambda t: t.transpose(1, 2).reshape(B, L, E)
    return {"out": back(out), "lse": lse, "gqkv": torch.cat([back(dq), back(dk), back(dv)], -1)}


def attention_loose(qkv, gout, H, causal, keep, keep_prob):
    x = qkv.clone().requires_grad_(True)
    out = gpt_ref.attention_ref(x, H, gpt_ref.causal_mask(qkv.shape[1]) if causal else None, keep, keep_prob)
    (out * gout).sum().backward()
    sc = X.scores64(qkv, H, causal).to(qkv.dtype) if qkv.dtype != torch.float64 else X.scores64(qkv, H, causal)
    return {"out": out, "lse": torch.logsumexp(sc, -1), "gqkv": x.grad}


def gpt_attention_ref(t, loose, H, causal, keep_prob):
    f = attention_loose if loose else attention_strict
    return f(t["qkv"], t["gout"], H, causal, t.get("keep"), keep_prob)


GPT_ATT_B, GPT_ATT_H = 2, 2
GPT_ATT_SHAPES = tuple((dh, L) for dh in (16, 64) for L in (33, 128))


def _qkv_index(b, row, part, h, d, H, dh):
    """index into qkv [B, L, 3 H dh] of element d of head h of q (part 0), k (1) or v (2) of row `row`"""
    return (b, row, part * H * dh + h * dh + d)


def gpt_attention_groups():
    B, H = GPT_ATT_B, GPT_ATT_H
    groups = []
    for dh, L in GPT_ATT_SHAPES:
        qkv, gout = X.attention_inputs("control", B, L, H, dh)
        ix = functools.partial(_qkv_index, H=H, dh=dh)
        plants = [("qkv", ix(1, 5, 0, 1, 3)), ("qkv", ix(1, 32, 1, 0, dh - 1)), ("qkv", ix(1, 31, 2, 0, 0)), ("qkv", ix(1, L - 1, 2, 0, 5)),
                  ("gout", (1, 6, dh + 2))]
        for causal in (True, False):
            for drop in (False, True):
                inputs = {"qkv": qkv, "gout": gout}
                if drop:
                    # the edge keep mask, with the planted value rows' own last partners kept: at one kept probability in ten the rows
                    # v(1, 31, h0) and v(1, L - 1, h0) would otherwise reach no output at all under the causal mask
                    inputs["keep"] = X.keep_mask(B, L, H).clone()
                    inputs["keep"][1, 0, 32, 31] = 1
                    inputs["keep"][1, 0, L - 1, L - 1] = 1
                groups.append(Group(f"gpt_attention dh={dh} L={L} {'causal' if causal else 'full'}{' keep' if drop else ''}", "gpt_attention",
                                    {"H": H, "causal": causal, "keep_prob": X.KEEP_PROB if drop else 1.0}, inputs, plants, gpt_attention_ref,
                                    {"out": FWD, "lse": FWD, "gqkv": BWD}, masked=causal or drop))
    return groups


PREFIX_SHAPES = ((20, 10), (33, 31))                   # (P, Lq)
PREFIX_DH = 32


def prefix_ref(t, loose, H):
    B, Lq, E3 = t["qkv"].shape
    P = t["prefix"].shape[1]
    cat = torch.cat([t["prefix"].expand(B, P, E3), t["qkv"]], 1)
    gout = torch.zeros(B, P + Lq, E3 // 3, dtype=cat.dtype)
    f = attention_loose if loose else attention_strict
    return {"out": f(cat, gout, H, True, None, 1.0)["out"][:, P:]}


def prefix_groups():
    B, H, dh = GPT_ATT_B, GPT_ATT_H, PREFIX_DH
    groups = []
    for P, Lq in PREFIX_SHAPES:
        for Bp in (B, 1):
            g = _gen("prefix", P, Lq, Bp)
            inputs = {"prefix": torch.randn(Bp, P, 3 * H * dh, generator=g), "qkv": torch.randn(B, Lq, 3 * H * dh, generator=g)}
            ix = functools.partial(_qkv_index, H=H, dh=dh)
            plants = [("prefix", ix(Bp - 1, P - 1, 1, 0, 1)), ("prefix", ix(Bp - 1, 3, 2, 1, 0)), ("qkv", ix(1, Lq - 2, 2, 0, dh - 1))]
            groups.append(Group(f"gpt_attention_prefix P={P} Lq={Lq} Bp={Bp}", "gpt_attention_prefix", {"H": H}, inputs, plants, prefix_ref,
                                {"out": FWD}, masked=True))
    return groups


XF_SHAPE = (17, 64, 4)                                 # S, D, H


def xf_attention_ref(t, loose, H):
    r = attention_strict(t["qkv"][None], t["gout"][None], H, False, None, 1.0)
    return {k: v[0] for k, v in r.items()}


def xf_attention_groups():
    S, D, H = XF_SHAPE
    dh = D // H
    qkv, gout = X.attention_inputs("control", 1, S, H, dh)
    inputs = {"qkv": qkv[0], "gout": gout[0]}
    plants = [("qkv", (5, 1 * dh + 3)), ("qkv", (S - 1, D + 0 * dh + 2)), ("qkv", (16, 2 * D + 3 * dh + dh - 1))]
    return [Group(f"attention S={S} D={D} H={H}", "attention", {"H": H}, inputs, plants, xf_attention_ref,
                  {"out": FWD, "lse": FWD, "gqkv": BWD})]


# ---------------------------------------------------------------------------------------------------
# embedding rows
# ---------------------------------------------------------------------------------------------------

EMBED_SHAPE = (33, 3, 252, 40)                         # N, T, E, table rows


def embed_ref_fn(t, loose, T):
    r = embed_ref.embed_run(t["src"], t["idx"], t["pos"], T, t["w"], t["bias"], t["gout"], t["src"].dtype)
    return {k: r[k] for k in ("y", "rstd", "g_src", "g_pos", "g_lnw", "g_lnb")}


def embed_groups():
    N, T, E, K = EMBED_SHAPE
    g = _gen("embed")
    inputs = {"src": torch.randn(K, E, generator=g), "idx": torch.randperm(K, generator=g)[:N], "pos": 0.1 * torch.randn(T, E, generator=g),
              "w": 1 + 0.1 * torch.randn(E, generator=g), "bias": 0.1 * torch.randn(E, generator=g), "gout": torch.randn(N, E, generator=g)}
    plants = [("src", (int(inputs["idx"][32]), 7)), ("pos", (1, 0)), ("w", (E - 1,))]
    return [Group(f"embed_rows N={N} T={T} E={E}", "embed_rows", {"T": T}, inputs, plants, embed_ref_fn,
                  {"y": FWD, "rstd": FWD, "g_src": BWD, "g_pos": BWD, "g_lnw": BWD, "g_lnb": BWD}, unordered=("g_pos", "g_lnw", "g_lnb"))]


# ---------------------------------------------------------------------------------------------------
# the two output heads
# ---------------------------------------------------------------------------------------------------

GMM_SHAPE = (33, 64, 5, 7)                             # N, E, M, A
GMM_MIN_STD = 0.01


def gmm_ref_fn(t, loose, M, A, std):
    sd = {"nets." + k: t[k] for k in ("mean.weight", "mean.bias", "scale.weight", "scale.bias", "logits.weight", "logits.bias")}
    pm, ps, lg = gmm_ref.decoder(sd, t["feats"], M, A)
    pre = torch.cat([pm.reshape(-1, M * A), ps.reshape(-1, M * A), lg], 1).detach().requires_grad_(True)
    MA = M * A
    pm, ps, lg = pre[:, :MA].view(-1, M, A), pre[:, MA:2 * MA].view(-1, M, A), pre[:, 2 * MA:]
    mu, sg = gmm_ref.activate(pm, ps, GMM_MIN_STD, std)
    lp = gmm_ref.mixture(mu, sg, lg).log_prob(t["actions"])
    gpre, = torch.autograd.grad((lp * t["g"]).sum() + lp.sum() * t["gsum"], pre, retain_graph=True)
    gpar, = torch.autograd.grad((mu * t["gmean"]).sum() + (sg * t["gscale"]).sum() + (lg * t["glogits"]).sum(), pre)
    sample, _, _ = gmm_ref.sample_by_inverse_cdf(sd, t["feats"], t["u"], t["eps"], M, A, GMM_MIN_STD, std)
    sample = torch.where(torch.softmax(lg.detach(), -1).isfinite().all(-1, keepdim=True), sample, torch.full_like(sample, NAN))
    return {"log_prob": lp, "pre": pre, "mean": mu, "scale": sg, "logits": lg, "sum": lp.sum(), "gpre": gpre, "gpre_params": gpar,
            "sample": sample}


def gmm_groups():
    N, E, M, A = GMM_SHAPE
    groups = []
    for std in ("softplus", "exp"):
        g = _gen("gmm", std)
        rn = lambda *s, k=1.0: k * torch.randn(*s, generator=g)
        inputs = {"feats": rn(N, E), "mean.weight": rn(M * A, E, k=E ** -0.5), "mean.bias": rn(M * A, k=0.1),
                  "scale.weight": rn(M * A, E, k=0.5 * E ** -0.5), "scale.bias": rn(M * A, k=0.1), "logits.weight": rn(M, E, k=E ** -0.5),
                  "logits.bias": rn(M, k=0.1), "actions": rn(N, A, k=0.5), "g": rn(N), "gsum": rn(()), "gmean": rn(N, M, A),
                  "gscale": rn(N, M, A), "glogits": rn(N, M), "u": torch.rand(N, generator=g), "eps": rn(N, A)}
        plants = [("feats", (32, 0)), ("actions", (0, 6)), ("logits.bias", (2,))]
        tol = {"log_prob": FWD, "pre": FWD, "mean": FWD, "scale": FWD, "logits": FWD, "sum": FWD, "sample": FWD, "gpre": BWD, "gpre_params": BWD}
        groups.append(Group(f"gmm {std}", "gmm", {"M": M, "A": A, "std": std}, inputs, plants, gmm_ref_fn, tol))
        if std == "exp":
            groups.append(Group("gmm exp scale bias", "gmm", {"M": M, "A": A, "std": std}, inputs, [("scale.bias", (M * A - 1,))], gmm_ref_fn, tol,
                                values=("+inf",)))
    return groups


ACTION_HEAD_SHAPE = (33, 64, 7)                        # N, E, A
ACTION_HEAD_WEIGHTS = (0.5, 2.0, 0.25)                 # test_gpu_action_head.py's MIXED: all three loss terms on


def action_head_ref_fn(t, loose):
    pre = F.linear(t["feats"], t["W"], t["b"]).detach().requires_grad_(True)
    acts = torch.tanh(pre)
    losses = action_head_ref.compute_losses(acts, t["target"], ACTION_HEAD_WEIGHTS)
    lv = torch.stack([losses[k] for k in action_head_ref.LOSS_KEYS])
    gpre, = torch.autograd.grad((lv * t["g"]).sum() + (acts * t["gy"]).sum(), pre)
    return {"actions": acts, "pre": pre, "losses": lv, "gpre": gpre}


def action_head_groups():
    N, E, A = ACTION_HEAD_SHAPE
    g = _gen("action_head")
    inputs = {"feats": torch.randn(N, E, generator=g), "W": torch.randn(A, E, generator=g) / math.sqrt(E), "b": 0.1 * torch.randn(A, generator=g),
              "target": torch.rand(N, A, generator=g) * 2 - 1, "g": torch.randn(4, generator=g), "gy": torch.randn(N, A, generator=g)}
    return [Group(f"action_head N={N} E={E} A={A}", "action_head", {}, inputs, [("feats", (32, 0)), ("target", (5, 2)), ("W", (6, 63)), ("W", (0, 5))],
                  action_head_ref_fn, {"actions": FWD, "pre": FWD, "losses": FWD, "gpre": BWD})]


# ---------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------

GPT_MODULE = dict(num_layers=2, num_heads=2, E=64, L=12, B=3)


def gpt_module_state(seed=0):
    """state_dict (reference names, fp32) of a two-layer backbone: seeded, LayerNorm weights off 1, biases off 0"""
    E, L, nl = GPT_MODULE["E"], GPT_MODULE["L"], GPT_MODULE["num_layers"]
    g = _gen("gpt_module", seed)
    rn = lambda *s, k=1.0: k * torch.randn(*s, generator=g)
    sd = {"nets.output_ln.weight": 1 + rn(E, k=0.1), "nets.output_ln.bias": rn(E, k=0.1)}
    for i in range(nl):
        p = f"nets.transformer.{i}.nets."
        sd.update({p + "ln1.weight": 1 + rn(E, k=0.1), p + "ln1.bias": rn(E, k=0.1), p + "ln2.weight": 1 + rn(E, k=0.1), p + "ln2.bias": rn(E, k=0.1),
                   p + "attention.nets.qkv.weight": rn(3 * E, E, k=E ** -0.5), p + "attention.nets.output.weight": rn(E, E, k=E ** -0.5),
                   p + "attention.nets.output.bias": rn(E, k=0.1), p + "attention.mask": gpt_ref.causal_mask(L),
                   p + "mlp.0.weight": rn(4 * E, E, k=E ** -0.5), p + "mlp.0.bias": rn(4 * E, k=0.1),
                   p + "mlp.2.weight": rn(E, 4 * E, k=(4 * E) ** -0.5), p + "mlp.2.bias": rn(E, k=0.1)})
    return sd


def gpt_module_ref(t, loose, sd):
    """gpt_ref.gpt_forward (loose), or the same op sequence with the attention's causal mask applied by selection (strict)"""
    x = t["x"]
    sd = {k: v.to(x.dtype) for k, v in sd.items()}
    nl, H = GPT_MODULE["num_layers"], GPT_MODULE["num_heads"]
    if loose:
        return {"y": gpt_ref.gpt_forward(sd, x, nl, H)}
    E = x.shape[-1]
    for i in range(nl):
        p = f"nets.transformer.{i}.nets."
        y = F.layer_norm(x, (E,), sd[p + "ln1.weight"], sd[p + "ln1.bias"], 1e-5)
        qkv = F.linear(y, sd[p + "attention.nets.qkv.weight"])
        y = attention_strict(qkv, torch.zeros_like(x), H, True, None, 1.0)["out"]
        x = x + F.linear(y, sd[p + "attention.nets.output.weight"], sd[p + "attention.nets.output.bias"])
        y = F.layer_norm(x, (E,), sd[p + "ln2.weight"], sd[p + "ln2.bias"], 1e-5)
        y = F.linear(F.gelu(F.linear(y, sd[p + "mlp.0.weight"], sd[p + "mlp.0.bias"])), sd[p + "mlp.2.weight"], sd[p + "mlp.2.bias"])
        x = x + y
    return {"y": F.layer_norm(x, (E,), sd["nets.output_ln.weight"], sd["nets.output_ln.bias"], 1e-5)}


def gpt_module_groups():
    m = GPT_MODULE
    inputs = {"x": torch.randn(m["B"], m["L"], m["E"], generator=_gen("gpt_module", "x"))}
    return [Group("GPTBackbone eval", "gpt_module", {"sd": gpt_module_state()}, inputs, [("x", (1, 7, 3))], gpt_module_ref, {"y": FWD},
                  masked=True)]


VQ_MODULE = dict(A=7, D=32, K=64, N=80)


def vq_module_case():
    """(clean params as fp32 numpy, planted params, x): encoder.0.weight[3, 2] = NaN"""
    m = VQ_MODULE
    p = O.make_params(5, m["A"], m["D"], m["K"], regime="trained", variant="vq")
    planted = {k: np.array(v) for k, v in p.items()}
    planted["encoder.0.weight"][3, 2] = np.nan
    return p, planted, O.make_inputs(5, m["N"], m["A"])


def vq_module_ref(p, x, dtype=torch.float64):
    """(loss, {parameter name: gradient}) of oracle.torch_vq_forward with every parameter a leaf"""
    tp = {k: torch.from_numpy(np.array(v)).to(dtype).requires_grad_(True) for k, v in p.items()}
    _, loss, _ = O.torch_vq_forward(tp, torch.from_numpy(np.array(x)).to(dtype))
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in tp.items()}


ALL_GROUPS = (linear_groups, mlp3_groups, act_bwd_groups, wgrad_groups, layernorm_groups, gpt_attention_groups, prefix_groups,
              xf_attention_groups, embed_groups, gmm_groups, action_head_groups, gpt_module_groups)


@functools.lru_cache(maxsize=None)
def groups(op=None):
    """every group (computed once, shared read-only), or those of one operation"""
    out = [g for f in ALL_GROUPS for g in f()]
    for g in out:
        for v in g.inputs.values():
            if isinstance(v, torch.Tensor):
                v.requires_grad_(False)
    return tuple(g for g in out if op is None or g.op == op)
