"""GPU: the in-kernel dropout source at the C ABI and in ``ops`` for the kernels outside the backbone (include/lipvq.h,
"in-kernel dropout for the embedding stage and the default action branch"): the unbatched attention kernels, the Linear
epilogue with its act-backward, and the embed_rows stream launches.

Every claim is an equality of bits against the library's own keep-byte or plain path, the decisions materialised by
ops.dropout_keep (which tests/test_dropout_host.py holds to a numpy restatement) and applied by a torch multiply."""
import numpy as np
import pytest
import torch

from fenced import _Fenced

pytestmark = pytest.mark.gpu

SEED = 2 ** 63 + 977
EINVAL = -1


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _snap(seed, step=0):
    words = [v - 2 ** 64 if v >= 2 ** 63 else v for v in (seed & (2 ** 64 - 1), step & (2 ** 64 - 1))]
    return torch.tensor(words, dtype=torch.int64).cuda()


def _inv_keep(p):
    return float(np.float32(1.0) / np.float32(1.0 - p))


def _scale(ops, snap, site, rows, cols, p):
    """inv_keep where (row, col) is kept, 0 where it is dropped, fp32 [rows, cols]"""
    return ops.dropout_keep(snap, site, rows, cols, p).float() * _inv_keep(p)


def _randn(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same(a, b, tag):
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True, msg=lambda m: f"{tag}: {m}")


# ---------------------------------------------------------------------------------------------------
# 1. unbatched attention: head widths 8, 16 and 26 (the 32 instance); one row, a ragged second query block, 2 and 3 key tiles
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 17, 65, 130])
@pytest.mark.parametrize("D,H", [(64, 8), (128, 8), (208, 8)])
def test_attention_equals_the_keep_byte_kernels(ops, D, H, S):
    from lipvq_vae_amd._capi import check, lib
    qkv, gout = _randn(S + D, S, 3 * D), _randn(S + D + 1, S, D)
    plain_out, plain_lse = ops.attention(qkv, H)
    for p in (0.1, 0.9):
        site, snap = ops.DROPOUT_SITE_DEFAULT + 4, _snap(SEED, 5)
        keep = ops.dropout_keep(snap, site, H * S, S, p).view(H, S, S)
        want_out, want_lse = ops.attention(qkv, H, keep, 1.0 - p)
        want_g = ops.attention_bwd(qkv, want_out, gout, want_lse, H, keep, 1.0 - p)
        f = dict(out=_Fenced("out", S, D), lse=_Fenced("lse", H, S), gqkv=_Fenced("gqkv", S, 3 * D), delta=_Fenced("delta", H, S))
        check(lib.lipvq_attention_drop_f32(qkv.data_ptr(), f["out"].ptr(), f["lse"].ptr(), snap.data_ptr(), site, p, S, D, H, _stream()),
              "lipvq_attention_drop_f32")
        check(lib.lipvq_attention_bwd_drop_f32(qkv.data_ptr(), f["out"].ptr(), gout.data_ptr(), f["lse"].ptr(), f["gqkv"].ptr(),
                                               f["delta"].ptr(), snap.data_ptr(), site, p, S, D, H, _stream()), "lipvq_attention_bwd_drop_f32")
        torch.cuda.synchronize()
        got = {k: v.check() for k, v in f.items()}
        tag = (D, H, S, p)
        assert torch.equal(got["out"], want_out), tag
        assert torch.equal(got["lse"], want_lse) and torch.equal(got["lse"], plain_lse), tag      # (dropout acts after the softmax)
        assert torch.equal(got["gqkv"], want_g), tag
        if S > 1:
            assert not torch.equal(got["out"], plain_out), tag
        # a query row all of whose keys are dropped behaves as the byte path does: a zero output row, its lse unchanged
        dead = keep.sum(-1) == 0                                      # [H, S]
        if S == 1 and p == 0.9:
            assert bool(dead.any()), "the fixture has no head whose only key is dropped"
        if bool(dead.any()):
            rows = got["out"].view(S, H, D // H).permute(1, 0, 2)[dead]
            assert not bool(rows.any()), tag
        # and through ops
        out, lse = ops.attention(qkv, H, dropout=(snap, site, p))
        g = ops.attention_bwd(qkv, out, gout, lse, H, dropout=(snap, site, p))
        assert torch.equal(out, want_out) and torch.equal(lse, want_lse) and torch.equal(g, want_g), tag
        # another site or step is another field
        if S > 1:
            assert not torch.equal(ops.attention(qkv, H, dropout=(snap, site + 4, p))[0], out), tag
            assert not torch.equal(ops.attention(qkv, H, dropout=(_snap(SEED, 6), site, p))[0], out), tag


# ---------------------------------------------------------------------------------------------------
# 2. the Linear epilogue and its act-backward: each side of lipvq_linear_act_f32's kernel choice
# ---------------------------------------------------------------------------------------------------

LINEAR_SHAPES = [(33, 12, 100), (1, 7, 4), (32769, 64, 256), (131077, 8, 60)]      # small, small with Kin % 4 != 0, big<2,2>, big<4,1>


@pytest.mark.parametrize("act", ["NONE", "GELU", "RELU"])
@pytest.mark.parametrize("N,Kin,E", LINEAR_SHAPES)
def test_linear_epilogue_equals_plain_times_mask(ops, N, Kin, E, act):
    from lipvq_vae_amd._capi import check, lib
    from lipvq_vae_amd.nnfn import LinearFn
    act = getattr(ops, "ACT_" + act)
    p, site, snap = 0.3, ops.DROPOUT_SITE_DEFAULT + 3, _snap(SEED, 11)
    x0, W0, b0, R = _randn(1, N, Kin), _randn(2, E, Kin, scale=0.3), _randn(3, E, scale=0.3), _randn(4, N, E)
    m = _scale(ops, snap, site, N, E, p)
    y_plain, pre_plain = ops.linear(x0, W0, b0, act=act, save_pre=True)
    fy, fpre = _Fenced("y", N, E), _Fenced("pre", N, E)
    check(lib.lipvq_linear_act_drop_f32(x0.data_ptr(), W0.data_ptr(), b0.data_ptr(), fy.ptr(), fpre.ptr(), snap.data_ptr(), site, p, N, Kin,
                                        E, act, _stream()), "lipvq_linear_act_drop_f32")
    torch.cuda.synchronize()
    tag = (N, Kin, E, act)
    assert torch.equal(fy.check(), y_plain * m), tag
    assert torch.equal(fpre.check(), pre_plain), tag
    y, pre = ops.linear(x0, W0, b0, act, save_pre=True, dropout=(snap, site, p))
    assert torch.equal(y, y_plain * m) and torch.equal(pre, pre_plain), tag
    assert torch.equal(ops.linear(x0, W0, None, act, dropout=(snap, site, p)), ops.linear(x0, W0, None, act=act) * m), tag
    # the act-backward's first step, fenced, then the three gradients under autograd
    fg = _Fenced("gpre", N, E)
    check(lib.lipvq_act_bwd_drop_f32(R.data_ptr(), pre_plain.data_ptr(), fg.ptr(), snap.data_ptr(), site, p, N, E, act, _stream()),
          "lipvq_act_bwd_drop_f32")
    torch.cuda.synchronize()
    want_gpre = ops.act_bwd(R * m, pre_plain, act)
    assert torch.equal(fg.check(), want_gpre), tag

    def grads(fn):
        x, W, b = (t.clone().requires_grad_(True) for t in (x0, W0, b0))
        (fn(x, W, b) * R).sum().backward()
        return x.grad, W.grad, b.grad

    got = grads(lambda x, W, b: LinearFn.apply(x, W, b, act, "fp32", (snap, site, p)))
    want = grads(lambda x, W, b: LinearFn.apply(x, W, b, act) * m)
    for name, g, w in zip(("gx", "gW", "gb"), got, want):
        assert torch.equal(g, w), (tag, name)


def test_linear_epilogue_keeps_a_nan_at_a_dropped_output(ops):
    N, Kin, E, p, site, snap = 33, 12, 100, 0.5, ops.DROPOUT_SITE_DEFAULT + 7, _snap(SEED, 2)
    x, W, b = _randn(1, N, Kin), _randn(2, E, Kin, scale=0.3), _randn(3, E, scale=0.3)
    x[17, 5] = float("nan")                                          # row 17 of the result is a NaN in every column
    keep = ops.dropout_keep(snap, site, N, E, p)
    assert 0 < int(keep[17].sum()) < E, "the fixture's row has no dropped (or no kept) column"
    m = keep.float() * _inv_keep(p)
    for act in (ops.ACT_NONE, ops.ACT_GELU, ops.ACT_RELU):
        y = ops.linear(x, W, b, act, dropout=(snap, site, p))
        _same(y, ops.linear(x, W, b, act=act) * m, act)
        assert bool(torch.isnan(y[17]).all()), "a NaN at a dropped output must stay a NaN (the mask is a product)"
        assert not bool(torch.isnan(y[:17]).any()) and not bool(torch.isnan(y[18:]).any())


# ---------------------------------------------------------------------------------------------------
# 3. embed_rows: one width per instance, all three call shapes, dense and index + codebook streams
# ---------------------------------------------------------------------------------------------------

def _embedding(E, T, p=0.25, Din=9):
    from lipvq_vae_amd.embedding import ICLInputEmbedding
    torch.manual_seed(100 + E)
    net = ICLInputEmbedding(Din, embed_dim=E, context_length=T, emb_dropout=p).cuda()
    with torch.no_grad():                                            # (the reference initialises these to zeros / ones: move them)
        net.params["embed_timestep"].normal_(0.0, 0.5)
        net.nets["embed_ln"].weight.normal_(1.0, 0.2)
        net.nets["embed_ln"].bias.normal_(0.0, 0.2)
    return net


def _embed_call(net, kind, stream, inp):
    tokens = dict(action_indices=inp["idx"], codebook=inp["codebook"]) if stream == "index" else {}
    if kind == "forward":
        return net(inp["obs"], inp["cobs"], None if tokens else inp["cact"], **tokens)
    if kind == "prompt":
        return net.prompt_embedding(inp["cobs"], None if tokens else inp["cact"], **tokens)
    return net.input_embedding_tokens(inp["idx"], inp["codebook"]) if tokens else net.input_embedding(inp["obs"])


# The gradients that the atomic backward entry points add with fp32 atomics (1 - 2 ulp from run to run there): the LayerNorm
# weight and bias and the time embedding.  ops.embed_rows_bwd takes lipvq_embed_rows_bwd_det_f32, which sums them as per-workgroup
# partial sums added in workgroup order, so they are held to torch.equal like every other gradient, and must repeat.
ATOMIC = ("nets.embed_ln.weight", "nets.embed_ln.bias", "params.embed_timestep")


def _embed_compare(ops, net, kind, stream, inp, S, p):
    """(kernel source output and gradients) against (the plain module, times m by torch), same module, same inputs"""
    B, E = inp["obs"].shape[0], net.embed_dim
    R = _randn(5, B, S, E)
    dense = [k for k in ("obs", "cobs", "cact") if inp[k].requires_grad]

    def run(call):
        for t in list(net.parameters()) + [inp[k] for k in dense]:
            t.grad = None
        out = call()
        (out * R).sum().backward()
        grads = {k: q.grad.clone() for k, q in net.named_parameters() if q.grad is not None}
        grads.update({"in." + k: inp[k].grad.clone() for k in dense if inp[k].grad is not None})
        return out.detach(), grads

    net.train().set_dropout_source("kernel", seed=SEED)
    net.reseed_dropout(SEED, step=7)
    got, got_g = run(lambda: _embed_call(net, kind, stream, inp))
    assert net.dropout_state.tolist() == [SEED - 2 ** 64, 8], "one dropout_begin per forward"
    m = _scale(ops, _snap(SEED, 7), ops.DROPOUT_SITE_EMBED, B * S, E, p).view(B, S, E)
    net.eval()                                                       # the plain path: no dropout, the same launches otherwise
    want, want_g = run(lambda: _embed_call(net, kind, stream, inp) * m)
    again, again_g = run(lambda: _embed_call(net, kind, stream, inp) * m)
    for k in sorted(want_g):                                         # (figures first: the kernel source's miss, and the plain path's own repeat)
        miss = float((got_g[k] - want_g[k]).abs().max()) if k in got_g else float("nan")
        own = float((again_g[k] - want_g[k]).abs().max())
        print(f"embed {kind}/{stream} E={E} {k}: |kernel - plain*m| max {miss:.3e}, plain*m run to run {own:.3e}, scale {float(want_g[k].abs().max()):.3e}")
    _EMBED_AGAIN.append(again_g)
    return got, got_g, want, want_g


_EMBED_RUNS = {}
_EMBED_AGAIN = []


def _embed_case(ops, E, kind, stream):
    """one kernel-source run and one plain-times-m run per case, shared by the two tests below"""
    key = (E, kind, stream)
    if key not in _EMBED_RUNS:
        B, T, p, Din = 3, 5, 0.25, 9
        net = _embedding(E, T, p, Din)
        inp = {k: _randn(i, B, T, Din).requires_grad_(True) for i, k in enumerate(("obs", "cobs", "cact"))}
        inp["codebook"] = _randn(9, 40, Din)
        inp["idx"] = torch.randperm(40, generator=torch.Generator().manual_seed(3))[:B * T].view(B, T).cuda()      # (one writer per table row)
        S = {"forward": 3 * T, "prompt": 2 * T, "input": T}[kind]
        _EMBED_RUNS[key] = (B, S, p) + _embed_compare(ops, net, kind, stream, inp, S, p)
        _EMBED_RUNS[key + ("again",)] = _EMBED_AGAIN[-1]            # the second plain-times-m run's gradients
    return _EMBED_RUNS[key]


def _embed_big_case(ops):
    """B T = 32 770 indexed rows through the module: ops.embed_rows_bwd takes lipvq_embed_rows_bwd_det_f32, whose table gradient
    goes through the counting-sort scatter at this size"""
    if "big" not in _EMBED_RUNS:
        from lipvq_vae_amd._capi import lib
        B, T, E, p, Din, K = 3277, 10, 64, 0.25, 9, 64
        assert lib.lipvq_embed_rows_bwd_ws_supported(B * T, T, E, K) == 1
        net = _embedding(E, T, p, Din)
        inp = {k: _randn(i, B, T, Din) for i, k in enumerate(("obs", "cobs", "cact"))}
        inp["codebook"] = _randn(9, K, Din)
        inp["idx"] = torch.randint(0, K, (B, T), generator=torch.Generator().manual_seed(3)).cuda()
        _EMBED_RUNS["big"] = _embed_compare(ops, net, "input", "index", inp, T, p)
    return _EMBED_RUNS["big"]


EMBED_CASES = [(E, kind, stream) for E in (8, 192, 512, 1024) for kind in ("forward", "prompt", "input") for stream in ("dense", "index")]


@pytest.mark.parametrize("E,kind,stream", EMBED_CASES)
def test_embed_rows_drop_the_output_slot(ops, E, kind, stream):
    """The output, and every gradient whose sum has a fixed order: the dense inputs and the embed_encoder (one writer per row of
    the pre-LayerNorm gradient, then LinearFn's kernels)."""
    B, S, p, got, got_g, want, want_g = _embed_case(ops, E, kind, stream)
    tag = (E, kind, stream)
    assert got.shape == (B, S, E) and torch.equal(got, want), tag     # m is indexed by the OUTPUT row: the slot, not the stream row
    assert float((got == 0).float().mean()) > 0.5 * p, tag
    assert sorted(got_g) == sorted(want_g) and len(got_g) >= 4, (tag, sorted(got_g))
    fixed = [k for k in want_g if k not in ATOMIC]
    assert "nets.embed_encoder.weight" in fixed and len(fixed) >= (2 if (kind, stream) == ("input", "index") else 3), (tag, fixed)
    for k in fixed:
        assert torch.equal(got_g[k], want_g[k]), (tag, k)


@pytest.mark.parametrize("E,kind,stream", EMBED_CASES)
def test_embed_rows_drop_atomically_summed_gradients(ops, E, kind, stream):
    """The LayerNorm weight and bias and the time embedding, torch.equal as for every other gradient: the fixed-order backward
    (partial sums per workgroup, added in workgroup order) gives the kernel source and the plain module times m the same bits,
    and the plain path repeats its own."""
    B, S, p, got, got_g, want, want_g = _embed_case(ops, E, kind, stream)
    for k in ATOMIC:
        assert torch.equal(got_g[k], want_g[k]), ((E, kind, stream), k)
        assert torch.equal(_EMBED_RUNS[(E, kind, stream, "again")][k], want_g[k]), ((E, kind, stream), k, "the plain path does not repeat")


def test_embed_rows_drop_large_indexed_batch_takes_the_workspace_route(ops):
    """B T = 32 770 indexed rows (the gv kernel and the counting-sort scatter inside lipvq_embed_rows_bwd_det_f32): the output
    and the embed_encoder's gradients, which come through the table gradient the scatter adds in a fixed order.  The _ws_drop
    entry point itself is called in test_atomic_and_workspace_drop_entry_points below."""
    got, got_g, want, want_g = _embed_big_case(ops)
    assert torch.equal(got, want)
    assert sorted(got_g) == sorted(want_g)
    for k in ("nets.embed_encoder.weight", "nets.embed_encoder.bias"):
        assert torch.equal(got_g[k], want_g[k]), k


def test_embed_rows_drop_large_indexed_batch_atomically_summed_gradients(ops):
    """The same run's LayerNorm and time-embedding gradients: 1020 workgroups' partial sums, added in workgroup order."""
    got, got_g, want, want_g = _embed_big_case(ops)
    for k in ATOMIC:
        assert torch.equal(got_g[k], want_g[k]), k


# ---------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------

def test_entry_points_refuse_p_zero_and_one(ops):
    from lipvq_vae_amd._capi import lib
    S, D, H, N, Kin, E, T = 17, 64, 8, 15, 12, 64, 5
    qkv, gout, snap, site = _randn(1, S, 3 * D), _randn(2, S, D), _snap(3), ops.DROPOUT_SITE_DEFAULT
    out, lse = ops.attention(qkv, H)
    x, W, y = _randn(3, N, Kin), _randn(4, E, Kin), _Fenced("y", N, E)
    src, ln, o, st = _randn(5, N, E), torch.ones(E).cuda(), _Fenced("out", N, E), _Fenced("stats", N, 2)
    for p in (0.0, 1.0):
        fo, fl, fg, fd = _Fenced("o", S, D), _Fenced("l", H, S), _Fenced("g", S, 3 * D), _Fenced("d", H, S)
        assert lib.lipvq_attention_drop_f32(qkv.data_ptr(), fo.ptr(), fl.ptr(), snap.data_ptr(), site, p, S, D, H, _stream()) == EINVAL
        assert lib.lipvq_attention_bwd_drop_f32(qkv.data_ptr(), out.data_ptr(), gout.data_ptr(), lse.data_ptr(), fg.ptr(), fd.ptr(),
                                                snap.data_ptr(), site, p, S, D, H, _stream()) == EINVAL
        assert lib.lipvq_linear_act_drop_f32(x.data_ptr(), W.data_ptr(), None, y.ptr(), None, snap.data_ptr(), site, p, N, Kin, E, 0,
                                             _stream()) == EINVAL
        assert lib.lipvq_act_bwd_drop_f32(src.data_ptr(), src.data_ptr(), y.ptr(), snap.data_ptr(), site, p, N, E, 1, _stream()) == EINVAL
        assert lib.lipvq_embed_rows_drop_f32(src.data_ptr(), None, None, ln.data_ptr(), ln.data_ptr(), 1e-5, o.ptr(), st.ptr(),
                                             snap.data_ptr(), site, p, N, T, E, N, T * E, E, 0, _stream()) == EINVAL
        assert lib.lipvq_embed_rows_bwd_drop_f32(src.data_ptr(), src.data_ptr(), None, None, src.data_ptr(), ln.data_ptr(), y.ptr(), None,
                                                 None, None, snap.data_ptr(), site, p, N, T, E, N, T * E, E, 0, _stream()) == EINVAL
        torch.cuda.synchronize()
        for f in (fo, fl, fg, fd, y, o, st):
            assert f.untouched(), (p, f.what)
        for call in (lambda: ops.attention(qkv, H, dropout=(snap, site, p)), lambda: ops.linear(x, W, None, 0, dropout=(snap, site, p)),
                     lambda: ops.act_bwd(src, src, 1, dropout=(snap, site, p))):
            with pytest.raises(ValueError):
                call()


def test_attention_refuses_keep_bytes_and_dropout_together(ops):
    """The unbatched wrappers take one mask source: keep bytes or the in-kernel dropout, never both.  Nothing is launched."""
    S, D, H = 17, 64, 8
    qkv, gout, snap = _randn(1, S, 3 * D), _randn(2, S, D), _snap(3)
    keep = torch.ones(H, S, S, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.attention(qkv, H, keep, 0.5, dropout=(snap, ops.DROPOUT_SITE_DEFAULT, 0.5))
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.attention_bwd(qkv, gout, gout, torch.zeros(H, S, device="cuda"), H, keep, 0.5, dropout=(snap, ops.DROPOUT_SITE_DEFAULT, 0.5))


def test_modules_refuse_p_one_and_a_state_on_another_device(ops):
    import warnings
    from lipvq_vae_amd.default_branch import DefaultActionNetwork
    emb = _embedding(64, 5, p=1.0).train().set_dropout_source("kernel", seed=1)
    obs = _randn(1, 2, 5, 9)
    with pytest.raises(ValueError, match="ICLInputEmbedding: embed_drop p=1.0"):
        emb.input_embedding(obs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(2)
        net = DefaultActionNetwork(7, 64, num_layers=1).cuda().train().set_dropout_source("kernel", seed=1)
    x = _randn(2, 11, 7)
    net(x)
    net[5].layers[0].dropout.p = 1.0
    with pytest.raises(ValueError, match="DefaultActionNetwork: dropout p=1.0"):
        net(x)
    net[5].layers[0].dropout.p = 0.1
    for mod, call in ((net, lambda: net(x)), (_embedding(64, 5).train().set_dropout_source("kernel", seed=1), None)):
        mod._buffers["_dropout_state"] = mod._buffers["_dropout_state"].cpu()          # (what a partial move leaves behind)
        with pytest.raises(RuntimeError, match="dropout state is not on the input's device"):
            call() if call else mod.input_embedding(obs)


# ---------------------------------------------------------------------------------------------------
# 5. the fixed-order backward itself: repeats in bits, agrees with the atomic kernel to its summation accuracy
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("B,T,E", [(3, 5, 8), (37, 10, 192), (1500, 3, 64)])      # one workgroup per step; several; the cap of 1024 / T
def test_fixed_order_backward_repeats_and_matches_the_atomic_kernel(ops, B, T, E, indexed):
    from lipvq_vae_amd._capi import check, lib
    N, K = B * T, 7                                                  # (indexed: few table rows, so every row has many writers)
    src = _randn(1, K if indexed else N, E)
    idx = torch.randint(0, K, (N,), generator=torch.Generator().manual_seed(2)).cuda() if indexed else None
    pos, w, b = _randn(3, T, E, scale=0.3), 1.0 + _randn(4, E, scale=0.1), _randn(5, E, scale=0.1)
    out, gout = torch.zeros(B, 2 * T, E, device="cuda"), _randn(6, B, 2 * T, E)
    layout = (2 * T * E, 2 * E, E)
    stats = ops.embed_rows(src, idx, pos, w, b, 1e-5, out, N, T, *layout, want_stats=True)

    def run(det):
        g = [torch.zeros_like(src), torch.zeros_like(pos), torch.zeros(E, device="cuda"), torch.zeros(E, device="cuda")]
        if det:
            ops.embed_rows_bwd(gout, src, idx, pos, stats, w, *g, N, T, *layout)
        else:
            check(lib.lipvq_embed_rows_bwd_f32(gout.data_ptr(), src.data_ptr(), None if idx is None else idx.data_ptr(), pos.data_ptr(),
                                               stats.data_ptr(), w.data_ptr(), *(t.data_ptr() for t in g), N, T, E, src.shape[0], *layout,
                                               _stream()), "lipvq_embed_rows_bwd_f32")
        return g

    first, again, atomic = run(True), run(True), run(False)
    for name, a, c, o in zip(("g_src", "g_pos", "g_lnw", "g_lnb"), first, again, atomic):
        assert torch.equal(a, c), (name, "two runs differ")
        scale = float(o.abs().max())
        # two fp32 summation orders: the bound tests/test_gpu_embed.py holds the workspace route to against the atomic kernel
        print(f"fixed-order vs atomic B={B} T={T} E={E} indexed={indexed} {name}: {float((a - o).abs().max()):.3e} at scale {scale:.3e}")
        assert float((a - o).abs().max()) <= 2e-4 * scale, (name, float((a - o).abs().max()), scale)
    # accumulation: a second call on the same buffers adds the same sums again
    g = run(True)
    ops.embed_rows_bwd(gout, src, idx, pos, stats, w, *g, N, T, *layout)
    for name, a, c in zip(("g_pos", "g_lnw", "g_lnb"), g[1:], first[1:]):
        assert torch.equal(a, 2.0 * c), name


# ---------------------------------------------------------------------------------------------------
# 6. the two _drop backward entry points the module does not take: lipvq_embed_rows_bwd_drop_f32 (the atomic kernel's DROP
#    instances) and lipvq_embed_rows_bwd_ws_drop_f32, at the C ABI with a real snap
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,E,K,indexed", [(3, 5, 8, 40, False), (3, 5, 192, 40, True), (7, 4, 512, 9, True), (5, 3, 1024, 0, False),
                                             (3277, 10, 64, 64, True), (4100, 8, 192, 0, False)],
                         ids=["E8-dense", "E192-index", "E512-index-dup", "E1024-dense", "ws-32770-index", "ws-32800-dense"])
def test_atomic_and_workspace_drop_entry_points(ops, B, T, E, K, indexed):
    """gout * m regenerated inside lipvq_embed_rows_bwd_drop_f32 (every NJ instance of embed_rows_bwd_kernel<NJ, true>) and, from
    32 768 rows on, lipvq_embed_rows_bwd_ws_drop_f32, against the PLAIN entry point of the same route fed gout * m formed by
    torch: the slot row (streams interleaved: t stride 2 E, offset E, so the field row is not the stream row) and the column
    of every draw.  g_src with one writer per row, and the workspace route's table gradient, are equal in every bit; what these
    two routes add with fp32 atomics is held to the bound tests/test_gpu_embed.py holds the same sums to (2e-4 of scale)."""
    from lipvq_vae_amd._capi import check, lib
    N, S, p, site, snap = B * T, 2 * T, 0.3, ops.DROPOUT_SITE_EMBED, _snap(SEED, 13)
    src = _randn(1, K if indexed else N, E)
    idx = None
    if indexed:                                                      # K >= N: one writer per table row; else every row has many
        g = torch.Generator().manual_seed(2)
        idx = (torch.randperm(K, generator=g)[:N] if K >= N else torch.randint(0, K, (N,), generator=g)).cuda()
    pos, w, b = _randn(3, T, E, scale=0.3), 1.0 + _randn(4, E, scale=0.1), _randn(5, E, scale=0.1)
    out, gout = torch.zeros(B, S, E, device="cuda"), _randn(6, B, S, E)
    layout = (S * E, 2 * E, E)
    stats = ops.embed_rows(src, idx, pos, w, b, 1e-5, out, N, T, *layout, want_stats=True)
    m = _scale(ops, snap, site, B * S, E, p).view(B, S, E)
    gm = (gout * m).contiguous()
    ws_route = N >= 32768
    if ws_route and indexed:
        assert lib.lipvq_embed_rows_bwd_ws_supported(N, T, E, K) == 1
    nbytes = lib.lipvq_embed_rows_bwd_workspace_bytes(N, T, E, K) if (ws_route and indexed) else 0

    def run(drop, g_in):
        g = [_Fenced("g_src", *src.shape), _Fenced("g_pos", T, E), _Fenced("g_lnw", E), _Fenced("g_lnb", E)]
        for f in g:
            f.t.zero_()
        ws = _Fenced("workspace", max(4, nbytes // 4))
        head = (g_in.data_ptr(), src.data_ptr(), None if idx is None else idx.data_ptr(), pos.data_ptr(), stats.data_ptr(), w.data_ptr(),
                *(f.ptr() for f in g))
        mid = ((ws.ptr() if nbytes else None,) if ws_route else ()) + ((snap.data_ptr(), site, p) if drop else ())
        name = "lipvq_embed_rows_bwd_" + ("ws_" if ws_route else "") + ("drop_" if drop else "") + "f32"
        check(getattr(lib, name)(*head, *mid, N, T, E, src.shape[0], *layout, _stream()), name)
        torch.cuda.synchronize()
        fenced = g + [ws]                                            # (the workspace need not be written in full: its bands only)
        lo = [f.buf[:f.words.storage_offset()] for f in fenced] + [f.buf[f.words.storage_offset() + f.n:] for f in fenced]
        from fenced import SENTINEL
        assert all(bool((x == SENTINEL).all()) for x in lo), name + ": a word outside an output was written"
        return [f.t.clone() for f in g]

    got, want = run(True, gout), run(False, gm)
    fixed_src = (not indexed) or K >= N or ws_route                  # one writer per row, or the counting-sort scatter
    for name, a, c in zip(("g_src", "g_pos", "g_lnw", "g_lnb"), got, want):
        scale = float(c.abs().max())
        miss = float((a - c).abs().max())
        print(f"{'ws_' if ws_route else ''}drop B={B} T={T} E={E} indexed={indexed} {name}: {miss:.3e} at scale {scale:.3e}")
        if name == "g_src" and fixed_src:
            assert torch.equal(a, c), name
        else:
            assert miss <= 2e-4 * scale, (name, miss, scale)
    assert float(got[0].abs().max()) > 0 and not torch.equal(got[1], run(False, gout)[1]), "the mask changed nothing"
