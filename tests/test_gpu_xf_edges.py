"""GPU: the transformer kernels (csrc/lipvq_gpt.hip: batched attention, the LayerNorm family; csrc/lipvq_xf.hip: the unbatched
attention) on inputs that are NOT unit-normal, at the tile edges, and with their outputs fenced in.

tests/test_gpu_gpt.py and tests/test_gpu_default.py draw every input from torch.randn: scores stay inside +-5, rows have mean 0
and variance 1, nine keep bytes in ten are set, and every output is a fresh torch.empty.  Here the inputs come from
tests/xf_edge_inputs.py (peaked, offset, uniform, one-hot and far-apart scores; rows of 1000 + noise, 1e-20, 1e15, constants,
one-hot, cancelling sums; keep masks that drop whole rows and columns) and each result is held to that file's yardstick:
error <= max(tolerance, 4 x the deviation of stock fp32 torch on the CPU from float64 on the same inputs).  Every figure is
printed (class, shape, error, the reference's own, their ratio, the bound) before it is asserted.  The guard-band tests call
the C ABI on output slices inside sentinel-filled buffers: no word outside may change, none inside may keep the sentinel.
No input anywhere in this file is non-finite.

What these tests found when they were written (figures as fractions of the float64 maximum, against their bounds):
the unbatched forward on 'peaked16' -- out 4.07e-5 > 2.11e-5 at S = 17, D = 128, H = 4 with the keep mask and 1.16e-5 > 1e-5
at S = 65, D = 64, H = 8 (an fp32 score chain is ~1e-4 off at |s| ~ 500; the scores are float64 chains now, out <= 3.8e-7 on
every class); gpt_layernorm_kernel on 'plus1000' -- y 4.10e-5 > 1.21e-5 at N = 5, E = 256 and 5.24e-5 > 4.93e-5 at N = 1,
E = 252 (the fp32 row mean ~1e-4 off; the row is centred twice now, y <= 1.6e-7 there without b).
A constant row's gs is NOT gres: xhat = 0 leaves gs = rstd (g w - mean(g w)) + gres, which the yardstick checks like any row.
"""
import math

import numpy as np
import pytest
import torch

import xf_edge_inputs as X
from fenced import PAD, SENTINEL, _Fenced  # noqa: F401  (the guard bands: sentinel word, pad length, fenced output)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _assert_all(results):
    for what, err, bound in results:
        assert err <= bound, (what, err, bound)


def _head(t, h, dh, part=0, E=0):
    """Columns of head h in part (0 q / out, 1 k, 2 v) of a [..., (3) E] tensor."""
    return t[..., part * E + h * dh:part * E + (h + 1) * dh]


def _attention_results(tag, case, out, lse, gq, delta=None):
    """The yardstick rows of one attention case, the lse bound and the closed forms its class and keep mask give."""
    ref, dev = case["ref"], case["dev"]
    out, lse, gq = out.cpu(), lse.cpu(), gq.cpu()
    results = [X.report(f"{tag} out", X.rel(out, ref["out"]), dev["out"], X.FWD_TOL),
               X.report(f"{tag} gqkv", X.rel(gq, ref["gqkv"]), dev["gqkv"], X.BWD_TOL)]
    if delta is not None:
        results.append(X.report(f"{tag} delta", X.rel(delta.cpu(), ref["delta"]), dev["delta"], X.BWD_TOL))
    e_lse = float((lse.double() - ref["lse"]).abs().max())
    print(f"{tag} lse: abs error {e_lse:.3e}, largest |score| {ref['score_max']:.1f}, bound {X.lse_bound(case):.3e}")
    results.append((f"{tag} lse", e_lse, X.lse_bound(case)))
    return results


def _attention_closed_forms(cls, case, out, lse, gq, B, L, H, dh, causal):
    E = H * dh
    out, lse, gq = out.cpu().double(), lse.cpu().double(), gq.cpu()
    v = case["qkv"][..., 2 * E:].double()
    if cls == "uniform":                                            # q = 0: every open key weighs the same
        n = torch.arange(1, L + 1, dtype=torch.float64) if causal else torch.full((L,), float(L), dtype=torch.float64)
        assert (lse - n.log()).abs().max() <= 1e-5
        if case["keep"] is None:
            want = v.cumsum(1) / n.view(1, L, 1) if causal else v.mean(1, keepdim=True).expand(B, L, E)
            assert X.rel(out, want) <= X.FWD_TOL
    if cls == "dominant" and case["keep"] is None:                  # the softmax is one-hot to fp32: the row is the dominant key's value
        for b, h, i, j in X.dominant_pairs(B, L, H):
            assert X.rel(_head(out[b, i], h, dh), _head(v[b, j], h, dh)) <= X.FWD_TOL, (b, h, i, j)
    if case["keep"] is not None:
        for b, h, row, col in X.dropped_rows(B, L, H):
            assert (_head(out[b, row], h, dh) == 0).all(), "a query that keeps no key has a zero output row"
            assert (_head(gq[b, row], h, dh, 0, E) == 0).all(), "... and an exactly zero q-gradient"
            assert (_head(gq[b, col], h, dh, 2, E) == 0).all(), "a key nobody keeps has an exactly zero v-gradient"


# ---------------------------------------------------------------------------------------------------
# batched attention (lipvq_gpt_attention_f32 / _bwd_f32)
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("L", X.GPT_L)
@pytest.mark.parametrize("dh", X.GPT_DH)
def test_batched_attention_classes(ops, dh, L, causal):
    B, H = X.GPT_B, X.GPT_H
    results = []
    for cls in X.ATTENTION_CLASSES:
        for drop in (False, True):
            case = X.attention_case(cls, B, L, H, dh, causal, drop)
            qc, gc = case["qkv"].cuda(), case["gout"].cuda()
            kc, kp = (case["keep"].cuda() if drop else None), case["keep_prob"]
            out, lse = ops.gpt_attention(qc, H, causal, kc, kp)
            gq = ops.gpt_attention_bwd(qc, out, gc, lse, H, causal, kc, kp)
            assert torch.equal(gq, ops.gpt_attention_bwd(qc, out, gc, lse, H, causal, kc, kp)), "the backward does not repeat bit for bit"
            tag = f"gpt_attention {cls} dh={dh} L={L} causal={causal} drop={drop}"
            results += _attention_results(tag, case, out, lse, gq)
            _attention_closed_forms(cls, case, out, lse, gq, B, L, H, dh, causal)
    _assert_all(results)


@pytest.mark.parametrize("L", [65, 127])
@pytest.mark.parametrize("dh", X.GPT_DH)
def test_causal_rows_ignore_large_later_rows(ops, dh, L):
    """Rows >= j of qkv overwritten with +-1e4 (scores of 1e8 and more behind the mask): the rows before j keep their bits."""
    B, H = X.GPT_B, X.GPT_H
    qkv = X.attention_inputs("control", B, L, H, dh)[0].cuda()
    out, lse = ops.gpt_attention(qkv, H, True)
    g = torch.Generator().manual_seed(L + dh)
    for j in (1, 32, 33, L - 1):
        q2 = qkv.clone()
        q2[:, j:] = (1e4 * torch.sign(torch.randn(B, L - j, qkv.shape[2], generator=g))).cuda()
        out2, lse2 = ops.gpt_attention(q2, H, True)
        assert torch.isfinite(out2).all() and torch.isfinite(lse2).all()
        assert torch.equal(out2[:, :j], out[:, :j]) and torch.equal(lse2[..., :j], lse[..., :j]), j
        assert not torch.equal(out2[:, j:], out[:, j:])


# ---------------------------------------------------------------------------------------------------
# unbatched attention (lipvq_attention_f32 / _bwd_f32)
# ---------------------------------------------------------------------------------------------------

def _capi():
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    return _capi.lib, _capi.check, lipvq_vae_amd.ops._stream


def _attention_bwd_capi(qkv, out, gout, lse, H, keep, kp, gqkv=None, delta=None):
    """lipvq_attention_bwd_f32 as ops.attention_bwd calls it, with the delta it keeps for itself handed back."""
    lib, check, stream = _capi()
    gqkv = torch.empty_like(qkv) if gqkv is None else gqkv
    delta = torch.empty_like(lse) if delta is None else delta
    S, D = out.shape
    check(lib.lipvq_attention_bwd_f32(qkv.data_ptr(), out.data_ptr(), gout.data_ptr(), lse.data_ptr(), gqkv.data_ptr(), delta.data_ptr(),
                                      None if keep is None else keep.data_ptr(), float(kp), S, D, H, stream()), "lipvq_attention_bwd_f32")
    return gqkv, delta


@pytest.mark.parametrize("D,H", X.XF_DH_HEADS)
@pytest.mark.parametrize("S", X.XF_S)
def test_unbatched_attention_classes(ops, S, D, H):
    dh = D // H
    results = []
    for cls in X.ATTENTION_CLASSES:
        for drop in (False, True):
            case = X.attention_case(cls, 1, S, H, dh, False, drop)
            qc, gc = case["qkv"][0].cuda(), case["gout"][0].cuda()
            kc, kp = (case["keep"][0].cuda() if drop else None), case["keep_prob"]
            out, lse = ops.attention(qc, H, kc, kp)
            gq = ops.attention_bwd(qc, out, gc, lse, H, kc, kp)
            gq2, delta = _attention_bwd_capi(qc, out, gc, lse, H, kc, kp)
            assert torch.equal(gq, gq2), "the backward does not repeat bit for bit"
            tag = f"attention {cls} S={S} D={D} H={H} drop={drop}"
            results += _attention_results(tag, case, out[None], lse[None], gq[None], delta[None])
            _attention_closed_forms(cls, case, out[None], lse[None], gq[None], 1, S, H, dh, False)
    _assert_all(results)


# ---------------------------------------------------------------------------------------------------
# LayerNorm (lipvq_gpt_layernorm_f32 / _bwd_f32)
# ---------------------------------------------------------------------------------------------------

def _cuda(t):
    return None if t is None else t.cuda()


@pytest.mark.parametrize("N", X.LN_N)
@pytest.mark.parametrize("E", X.LN_E)
def test_layernorm_classes(ops, E, N):
    results = []
    for with_b, want_s, with_gres in X.LN_VARIANTS:
        for classes in X.layernorm_groups(N):
            case = X.layernorm_case(classes, N, E, with_b, with_gres)
            a, b, w, bias, gy, gres = (_cuda(case[k]) for k in ("a", "b", "w", "bias", "gy", "gres"))
            s, y, xhat, rstd = ops.gpt_layernorm(a, b, w, bias, X.LN_EPS, want_s=want_s, save=True)
            assert (s is None) == (not want_s)
            gs, gw, gb = ops.gpt_layernorm_bwd(gy, xhat, rstd, w, gres)
            gs2, gw2, gb2 = ops.gpt_layernorm_bwd(gy, xhat, rstd, w, gres)
            assert torch.equal(gw2, gw) and torch.equal(gb2, gb) and torch.equal(gs2, gs), "the backward does not repeat bit for bit"
            got = {k: v.cpu() for k, v in dict(s=s, y=y, xhat=xhat, rstd=rstd, gs=gs, gw=gw, gb=gb).items() if v is not None}
            tag = f"N={N} E={E} b={with_b} s={want_s} gres={with_gres}"
            for cls in classes:
                sl = case["rows"][cls]
                for k in X.ROW_TENSORS:
                    if k in got:
                        results.append(X.report(f"layernorm {cls} {tag} {k}", X.rel(got[k][sl], case["ref"][k][sl]),
                                                X.layernorm_dev(case, k, cls), X.BWD_TOL if k == "gs" else X.FWD_TOL))
                if cls == "constant":
                    _constant_rows_are_exact(got, bias.cpu(), sl)
            for k in X.COLUMN_TENSORS:
                results.append(X.report(f"layernorm {'+'.join(classes)} {tag} {k}", X.rel(got[k], case["ref"][k]),
                                        X.layernorm_dev(case, k), X.BWD_TOL))
    _assert_all(results)


def _constant_rows_are_exact(got, bias, sl):
    """E copies of 3.0 add up exactly in fp32 in any order: mean = 3, every centred value and the variance are exactly 0."""
    assert (got["xhat"][sl] == 0).all()
    assert torch.equal(got["y"][sl], bias.expand_as(got["y"][sl]))
    want = 1.0 / math.sqrt(float(np.float32(X.LN_EPS)))
    assert (got["rstd"][sl].double() - want).abs().max() <= float(np.spacing(np.float32(want)))         # 1 ulp


# ---------------------------------------------------------------------------------------------------
# guard bands and full coverage of the outputs, through the C ABI
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [33, 127])
@pytest.mark.parametrize("dh", X.GPT_DH)
def test_batched_attention_writes_its_outputs_and_nothing_else(dh, L):
    lib, check, stream = _capi()
    B, H = X.GPT_B, X.GPT_H                                         # (dh = 16 is E = 32: gpt_store_t's d0 < DH is live)
    E = H * dh
    results = []
    for causal in (True, False):
        for drop in (False, True):
            case = X.attention_case("control", B, L, H, dh, causal, drop)
            qc, gc = case["qkv"].cuda(), case["gout"].cuda()
            kc, kp = (case["keep"].cuda() if drop else None), case["keep_prob"]
            kptr = None if kc is None else kc.data_ptr()
            out, lse = _Fenced("out", B, L, E), _Fenced("lse", B, H, L)
            gq, delta = _Fenced("gqkv", B, L, 3 * E), _Fenced("delta", B, H, L)
            check(lib.lipvq_gpt_attention_f32(qc.data_ptr(), out.ptr(), lse.ptr(), kptr, float(kp), B, L, E, H, int(causal), stream()),
                  "lipvq_gpt_attention_f32")
            check(lib.lipvq_gpt_attention_bwd_f32(qc.data_ptr(), out.ptr(), gc.data_ptr(), lse.ptr(), gq.ptr(), delta.ptr(), kptr, float(kp),
                                                  B, L, E, H, int(causal), stream()), "lipvq_gpt_attention_bwd_f32")
            torch.cuda.synchronize()
            tag = f"gpt_attention fenced dh={dh} L={L} causal={causal} drop={drop}"
            results += _attention_results(tag, case, out.check(), lse.check(), gq.check(), delta.check())
    _assert_all(results)


@pytest.mark.parametrize("D,H", X.XF_DH_HEADS)
@pytest.mark.parametrize("S", [17, 65])
def test_unbatched_attention_writes_its_outputs_and_nothing_else(S, D, H):
    lib, check, stream = _capi()
    results = []
    for drop in (False, True):
        case = X.attention_case("control", 1, S, H, D // H, False, drop)
        qc, gc = case["qkv"][0].cuda(), case["gout"][0].cuda()
        kc, kp = (case["keep"][0].cuda() if drop else None), case["keep_prob"]
        out, lse = _Fenced("out", S, D), _Fenced("lse", H, S)
        gq, delta = _Fenced("gqkv", S, 3 * D), _Fenced("delta", H, S)
        check(lib.lipvq_attention_f32(qc.data_ptr(), out.ptr(), lse.ptr(), None if kc is None else kc.data_ptr(), float(kp), S, D, H, stream()),
              "lipvq_attention_f32")
        _attention_bwd_capi(qc, out.t, gc, lse.t, H, kc, kp, gq.t, delta.t)
        torch.cuda.synchronize()
        tag = f"attention fenced S={S} D={D} H={H} drop={drop}"
        results += _attention_results(tag, case, out.check()[None], lse.check()[None], gq.check()[None], delta.check()[None])
    _assert_all(results)


@pytest.mark.parametrize("N,E", [(5, 260), (2053, 1020)])
def test_layernorm_writes_its_outputs_and_nothing_else(N, E):
    lib, check, stream = _capi()
    results = []
    for with_b, want_s, with_gres in ((True, True, True), (False, False, False)):
        case = X.layernorm_case(("control",), N, E, with_b, with_gres)
        a, b, w, bias, gy, gres = (_cuda(case[k]) for k in ("a", "b", "w", "bias", "gy", "gres"))
        f = {k: _Fenced(k, N, E) for k in ("y", "xhat", "gs")}
        f.update(rstd=_Fenced("rstd", N), gw=_Fenced("gw", E), gb=_Fenced("gb", E))
        if want_s:
            f["s"] = _Fenced("s", N, E)
        nbytes = lib.lipvq_gpt_layernorm_bwd_workspace_bytes(N, E)
        assert nbytes > 0 and nbytes % 4 == 0
        ws = _Fenced("workspace", nbytes // 4)                      # exactly the bytes the library asks for
        check(lib.lipvq_gpt_layernorm_f32(a.data_ptr(), None if b is None else b.data_ptr(), w.data_ptr(), bias.data_ptr(), X.LN_EPS,
                                          f["s"].ptr() if want_s else None, f["y"].ptr(), f["xhat"].ptr(), f["rstd"].ptr(), N, E, stream()),
              "lipvq_gpt_layernorm_f32")
        check(lib.lipvq_gpt_layernorm_bwd_f32(gy.data_ptr(), f["xhat"].ptr(), f["rstd"].ptr(), w.data_ptr(),
                                              None if gres is None else gres.data_ptr(), f["gs"].ptr(), f["gw"].ptr(), f["gb"].ptr(),
                                              ws.ptr(), N, E, stream()), "lipvq_gpt_layernorm_bwd_f32")
        torch.cuda.synchronize()
        ws.check()
        tag = f"layernorm fenced N={N} E={E} b={with_b} s={want_s} gres={with_gres}"
        for k, fenced in f.items():
            results.append(X.report(f"{tag} {k}", X.rel(fenced.check().cpu(), case["ref"][k]),
                                    X.layernorm_dev(case, k, None if k in X.COLUMN_TENSORS else "control"),
                                    X.BWD_TOL if k in ("gs", "gw", "gb") else X.FWD_TOL))
    _assert_all(results)


# ---------------------------------------------------------------------------------------------------
# the alignment contract
# ---------------------------------------------------------------------------------------------------

def _off4(t):
    """The same values, contiguous, 4 bytes past a 16-byte boundary."""
    o = torch.empty(t.numel() + 1, device="cuda")[1:].view(t.shape)
    o.copy_(t)
    assert o.is_contiguous() and o.data_ptr() % 16 == 4
    return o


def test_misaligned_inputs_are_refused(ops):
    from lipvq_vae_amd._capi import LipvqLibraryError
    B, L, H, dh = 2, 33, 2, 16
    qkv, gout = (t.cuda() for t in X.attention_inputs("control", B, L, H, dh))
    out, lse = ops.gpt_attention(qkv, H, True)
    with pytest.raises(LipvqLibraryError, match="aligned"):
        ops.gpt_attention(_off4(qkv), H, True)
    for args in ((_off4(qkv), out, gout), (qkv, _off4(out), gout), (qkv, out, _off4(gout))):
        with pytest.raises(LipvqLibraryError, match="aligned"):
            ops.gpt_attention_bwd(*args, lse, H, True)
    case = X.layernorm_case(("control",), 5, 260, True, True)
    a, b, w, bias, gy, gres = (_cuda(case[k]) for k in ("a", "b", "w", "bias", "gy", "gres"))
    s, y, xhat, rstd = ops.gpt_layernorm(a, b, w, bias, X.LN_EPS, want_s=True, save=True)
    for i in range(4):
        args = [a, b, w, bias]
        args[i] = _off4(args[i])
        with pytest.raises(LipvqLibraryError, match="aligned"):
            ops.gpt_layernorm(*args, X.LN_EPS)
    for i in (0, 1, 3, 4):
        args = [gy, xhat, rstd, w, gres]
        args[i] = _off4(args[i])
        with pytest.raises(LipvqLibraryError, match="aligned"):
            ops.gpt_layernorm_bwd(*args)
    torch.cuda.synchronize()


def test_a_refused_call_launches_nothing():
    """A misaligned OUTPUT through the C ABI: the status comes back and not one word of the buffer around it has changed."""
    lib, check, stream = _capi()
    B, L, H, dh = 2, 33, 2, 16
    E = H * dh
    qkv, gout = (t.cuda() for t in X.attention_inputs("control", B, L, H, dh))
    out, lse = _Fenced("out", B, L, E, offset_words=1), _Fenced("lse", B, H, L)
    assert lib.lipvq_gpt_attention_f32(qkv.data_ptr(), out.ptr(), lse.ptr(), None, 1.0, B, L, E, H, 1, stream()) != 0
    assert b"aligned" in lib.lipvq_last_error()
    gq, delta = _Fenced("gqkv", B, L, 3 * E, offset_words=1), _Fenced("delta", B, H, L)
    good_out, good_lse = torch.zeros(B, L, E, device="cuda"), torch.zeros(B, H, L, device="cuda")
    assert lib.lipvq_gpt_attention_bwd_f32(qkv.data_ptr(), good_out.data_ptr(), gout.data_ptr(), good_lse.data_ptr(), gq.ptr(), delta.ptr(),
                                           None, 1.0, B, L, E, H, 1, stream()) != 0
    assert b"aligned" in lib.lipvq_last_error()
    N, E = 5, 260
    a, w, bias = torch.randn(N, E, device="cuda"), torch.ones(E, device="cuda"), torch.zeros(E, device="cuda")
    y, xhat, rstd = _Fenced("y", N, E, offset_words=1), _Fenced("xhat", N, E), _Fenced("rstd", N)
    assert lib.lipvq_gpt_layernorm_f32(a.data_ptr(), None, w.data_ptr(), bias.data_ptr(), X.LN_EPS, None, y.ptr(), xhat.ptr(), rstd.ptr(),
                                       N, E, stream()) != 0
    assert b"aligned" in lib.lipvq_last_error()
    gs, gw, gb = _Fenced("gs", N, E, offset_words=1), _Fenced("gw", E), _Fenced("gb", E)
    ws = _Fenced("workspace", lib.lipvq_gpt_layernorm_bwd_workspace_bytes(N, E) // 4)
    good_rstd = torch.ones(N, device="cuda")
    assert lib.lipvq_gpt_layernorm_bwd_f32(a.data_ptr(), a.data_ptr(), good_rstd.data_ptr(), w.data_ptr(), None, gs.ptr(), gw.ptr(), gb.ptr(),
                                           ws.ptr(), N, E, stream()) != 0
    assert b"aligned" in lib.lipvq_last_error()
    torch.cuda.synchronize()
    for fenced in (out, lse, gq, delta, y, xhat, rstd, gs, gw, gb, ws):
        assert fenced.untouched(), fenced.what


def test_non_contiguous_views_give_the_bits_of_their_copies(ops):
    B, L, H, dh = 3, 33, 2, 16
    E = H * dh
    g = torch.Generator().manual_seed(5)
    transposed = torch.randn(L, B, 3 * E, generator=g).cuda().transpose(0, 1)
    sliced = torch.randn(B, L, 3 * E + 8, generator=g).cuda()[..., 4:3 * E + 4]
    gout_nc = torch.randn(B, L, E + 4, generator=g).cuda()[..., 2:E + 2]
    for qkv in (transposed, sliced):
        assert not qkv.is_contiguous()
        out, lse = ops.gpt_attention(qkv, H, True)
        out_c, lse_c = ops.gpt_attention(qkv.contiguous(), H, True)
        assert torch.equal(out, out_c) and torch.equal(lse, lse_c)
        assert torch.equal(ops.gpt_attention_bwd(qkv, out, gout_nc, lse, H, True),
                           ops.gpt_attention_bwd(qkv.contiguous(), out_c, gout_nc.contiguous(), lse_c, H, True))
    N, E = 5, 260
    a, b, gy = (torch.randn(N, E + 4, generator=g).cuda()[:, 1:E + 1] for _ in range(3))
    w, bias = torch.randn(2 * E, generator=g).cuda()[::2], torch.randn(E, generator=g).cuda()
    assert not a.is_contiguous() and not w.is_contiguous()
    got = ops.gpt_layernorm(a, b, w, bias, X.LN_EPS, want_s=True, save=True)
    want = ops.gpt_layernorm(a.contiguous(), b.contiguous(), w.contiguous(), bias, X.LN_EPS, want_s=True, save=True)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    got_b = ops.gpt_layernorm_bwd(gy, got[2], got[3], w, b)
    want_b = ops.gpt_layernorm_bwd(gy.contiguous(), want[2], want[3], w.contiguous(), b.contiguous())
    assert all(torch.equal(x, y) for x, y in zip(got_b, want_b))
