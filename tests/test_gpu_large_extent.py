"""GPU: every kernel family on an operand past 2^31 elements (and so past byte offset 2^32), tests/extent_cases.py's cases.

The small-shape suite cannot see a 32-bit index product: the rows it would move lie past row 2^31 // W.  Each case here runs its
entry point ONCE on the big operand and then checks

  whole tensor, no tolerance   the same entry point on consecutive chunks of at most 2^26 elements (an extent the small-shape suite
                               covers) must give the bits of the big call's rows -- a row's bits do not depend on N (the Linears
                               document that for both of their instances);
  guard bands                  the big output lies in a sentinel-filled buffer (tests/fenced.py, _FencedBig): every word inside is
                               written, none outside;
  fine check                   the window rows (the head, 64 rows on each side of element 2^30 and 2^31, the tail) against the
                               canonical oracle or a float64 restatement, at the budget of the kernel's small-shape test;
  reductions over rows         exact-sum operands (small integers on the window rows, ones on every eighth row): the fp32 result
                               must equal the int64 answer bit for bit, so a row added twice, skipped or read from a wrapped
                               address changes the result.

Inputs are drawn on the device chunk by chunk from a seeded generator; only window rows are ever copied to the host.  A case whose
declared memory (+ 10 %) is not free is skipped with both numbers in the reason.
"""
import gc
import math
import time

import numpy as np
import pytest
import torch

import backward_ref as R
import dropout_ref
import extent_cases as X
from fenced import _FencedBig

pytestmark = pytest.mark.gpu

SEED, STEP = 2 ** 63 + 977, 2 ** 32 - 3
LN_EPS = 1e-5
FWD_TOL, BWD_TOL, REF_FACTOR = 1e-5, 1e-4, 4.0           # tests/test_gpu_gpt.py's (tests/xf_edge_inputs.py)


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


@pytest.fixture(autouse=True)
def _time_and_free(request):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"\n[extent] {request.node.name}: {dt:.2f} s, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    gc.collect()
    torch.cuda.empty_cache()


def _case(name):
    case = X.BY_NAME[name]
    need = int(case.need * 1.1)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{name}: {free} bytes of device memory free, the case needs {need}")
    return case


def _lib():
    from lipvq_vae_amd._capi import check, lib
    return check, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _snap():
    words = [v - 2 ** 64 if v >= 2 ** 63 else v for v in (SEED, STEP)]
    return torch.tensor(words, dtype=torch.int64).cuda()


def _inv_keep(p):
    return float(np.float32(1.0) / np.float32(1.0 - p))


def _small(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _empty(N, W=None):
    return torch.empty((N,) if W is None else (N, W), device="cuda", dtype=torch.float32)


def _steps(N, W):
    cr = X.chunk_rows(W)
    return [(a, min(N, a + cr)) for a in range(0, N, cr)]


def _randn_big(seed, N, W=None):
    """fp32 [N, W] (or [N]) of standard normals, drawn on the device chunk by chunk, one generator seed per chunk."""
    t = _empty(N, W)
    g = torch.Generator(device="cuda")
    for i, (a, b) in enumerate(_steps(N, W or 1)):
        g.manual_seed(seed * 100003 + i)
        t[a:b].normal_(generator=g)
    return t


def _zeros_big(N, W):
    t = _empty(N, W)
    for a, b in _steps(N, W):
        t[a:b].zero_()
    return t


def _exact_dev(rows, W, salt):
    return torch.from_numpy(X.exact_values(rows, W, salt).astype(np.float32)).cuda()


def _plant_exact(t, case_or_wins, salt):
    """Write the exact-sum operand `salt` onto the window rows of t [N, W] (zero elsewhere is the caller's)."""
    for a, b in case_or_wins:
        v = _exact_dev(np.arange(a, b), t.shape[1] if t.dim() == 2 else 1, salt)
        t[a:b] = v if t.dim() == 2 else v[:, 0]


def _plant_count(t, value=1.0):
    """value on every row with r % 8 == 0 (chunk by chunk), all columns."""
    N, W = t.shape
    for a, b in _steps(N, W):
        t[a:b][(-a) % 8::8] = value


def _bits(t):
    return t.view(torch.int32)


def _chunks_equal(N, W, big, chunk_fn):
    """chunk_fn(a, b) -> {name: rows a..b from a call on that chunk alone}: the bits of big[name][a:b], for every chunk."""
    for a, b in _steps(N, W):
        got = chunk_fn(a, b)
        for k, v in got.items():
            assert v.shape == big[k][a:b].shape, (k, a, b)
            assert torch.equal(_bits(v), _bits(big[k][a:b])), f"{k}: rows {a} .. {b} of the big call differ from a call on those rows alone"
        del got


def _win(t, wins):
    """The window rows of a device tensor, on the host (numpy)."""
    return torch.cat([t[a:b] for a, b in wins]).cpu().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def _f32(a):
    return torch.from_numpy(np.asarray(a, np.float32)).cuda()


# ---------------------------------------------------------------------------------------------------
# A. the Linear (lipvq_linear_act_f32): wide output and wide input, both kernels
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("act", ["NONE", "GELU"])
@pytest.mark.parametrize("name", ["linear_wide_out_k8", "linear_wide_out_k6", "linear_wide_in"])
def test_linear(ops, oracle, name, act):
    """k8: linear_big_kernel for the big call and the chunks of the wide output (the wide input's chunks run linear_kernel:
    the documented equal bits); k6 (Kin % 4 != 0): linear_kernel at the big extent."""
    check, lib = _lib()
    case = _case(name)
    N, (Kin, E) = case.N, case.dims
    act = getattr(ops, "ACT_" + act)
    x = _randn_big(11, N, Kin)
    W, bias = _small(12, E, Kin, scale=1.0 / math.sqrt(Kin)), _small(13, E)
    fy, fpre = _FencedBig("y", N, E), _FencedBig("pre", N, E)
    check(lib.lipvq_linear_act_f32(x.data_ptr(), W.data_ptr(), bias.data_ptr(), fy.ptr(), fpre.ptr(), N, Kin, E, act, _stream()),
          "lipvq_linear_act_f32")
    torch.cuda.synchronize()
    big = {"y": fy.check(), "pre": fpre.check()}
    _chunks_equal(N, max(Kin, E), big, lambda a, b: dict(zip(("y", "pre"), ops.linear(x[a:b], W, bias, act, save_pre=True))))
    wins = X.windows(N, case.W)
    y_ref, pre_ref = oracle.linear_act(_win(x, wins), W.cpu().numpy(), bias.cpu().numpy(), act, save_pre=True)
    assert np.array_equal(_win(big["pre"], wins), pre_ref) and np.array_equal(_win(big["y"], wins), y_ref)


def _pipe_refs(mode, layout, A, B):
    """(float64 product of the operands as the mode reads them, sum of |terms|, reduction length) -- tests/gemm_bf16_cases.py's and
    tests/gemm_bf16x3_ref.py's restatements, the budget of tests/test_gpu_gemm_bf16.py / _bf16x3.py: error / RN bound <= 2."""
    import gemm_bf16_cases as C
    import gemm_bf16x3_ref as X3
    L = A.shape[1]
    if mode == "bf16":
        want, Rsum = C.product64(layout, A, B)
        return want, Rsum, L
    want, Rsum = X3.product3(layout, A, B)
    return want, Rsum, 3 * L


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("name", ["linear_pipe_wide_out", "linear_pipe_wide_in"])
def test_linear_pipe(ops, name, mode):
    """lipvq_linear_act_bf16 / _bf16x3: a row's bits depend neither on its position nor on the rows of the launch (include/lipvq.h),
    so the chunked calls owe the big call's bits whatever tile they pick."""
    import gemm_bf16_cases as C
    check, lib = _lib()
    case = _case(name)
    N, (Kin, E) = case.N, case.dims
    act = ops.ACT_GELU
    x = _randn_big(15, N, Kin)
    W, bias = _small(16, E, Kin, scale=1.0 / math.sqrt(Kin)), _small(17, E)
    fy, fpre = _FencedBig("y", N, E), _FencedBig("pre", N, E)
    entry = "lipvq_linear_act_" + mode
    check(getattr(lib, entry)(x.data_ptr(), W.data_ptr(), bias.data_ptr(), fy.ptr(), fpre.ptr(), N, Kin, E, act, _stream()), entry)
    torch.cuda.synchronize()
    big = {"y": fy.check(), "pre": fpre.check()}
    fn = getattr(ops, "linear_" + mode)
    _chunks_equal(N, max(Kin, E), big, lambda a, b: dict(zip(("y", "pre"), fn(x[a:b], W, bias, act, save_pre=True))))
    wins = X.windows(N, case.W)
    want, Rsum, L = _pipe_refs(mode, "NT", torch.from_numpy(_win(x, wins)), W.cpu())
    pre = torch.from_numpy(_win(big["pre"], wins))
    assert C.ratio(f"{name} {mode} pre", pre, want + bias.cpu().double(), Rsum, L) <= 2.0
    ref = torch.nn.functional.gelu(pre.double())
    assert float((torch.from_numpy(_win(big["y"], wins)).double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_linear_nn_pipe(ops, mode):
    """gx [N, 8] = g [N, 2048] . W [2048, 8]: the wide operand is the gradient."""
    import gemm_bf16_cases as C
    check, lib = _lib()
    case = _case("linear_nn_pipe")
    N, (J, K) = case.N, case.dims
    g = _randn_big(18, N, J)
    W = _small(19, J, K, scale=1.0 / math.sqrt(K))
    fgx = _FencedBig("gx", N, K)
    entry = "lipvq_linear_nn_" + mode
    check(getattr(lib, entry)(g.data_ptr(), W.data_ptr(), fgx.ptr(), N, J, K, _stream()), entry)
    torch.cuda.synchronize()
    gx = fgx.check()
    fn = getattr(ops, "linear_nn_" + mode)
    _chunks_equal(N, J, {"gx": gx}, lambda a, b: {"gx": fn(g[a:b], W)})
    wins = X.windows(N, case.W)
    want, Rsum, L = _pipe_refs(mode, "NN", torch.from_numpy(_win(g, wins)), W.cpu())
    assert C.ratio(f"linear_nn {mode} gx", torch.from_numpy(_win(gx, wins)), want, Rsum, L) <= 2.0


def test_linear_dropout_epilogue(ops):
    """lipvq_linear_act_drop_f32 at the wide-output shape: plain x keep field x inv_keep, bit for bit over the whole tensor (the plain
    Linear per chunk; the field from lipvq_dropout_keep_u8 in one call of N x 2048 bytes), pre the plain one; the field's window rows
    against the numpy restatement."""
    check, lib = _lib()
    case = _case("linear_drop")
    N, (Kin, E), p = case.N, case.dims, case.p
    act, site, snap = ops.ACT_GELU, ops.DROPOUT_SITE_DEFAULT + 3, _snap()
    x = _randn_big(21, N, Kin)
    W, bias = _small(22, E, Kin, scale=1.0 / math.sqrt(Kin)), _small(23, E)
    keep = ops.dropout_keep(snap, site, N, E, p)
    fy, fpre = _FencedBig("y", N, E), _FencedBig("pre", N, E)
    check(lib.lipvq_linear_act_drop_f32(x.data_ptr(), W.data_ptr(), bias.data_ptr(), fy.ptr(), fpre.ptr(), snap.data_ptr(), site, p, N, Kin, E,
                                        act, _stream()), "lipvq_linear_act_drop_f32")
    torch.cuda.synchronize()
    big = {"y": fy.check(), "pre": fpre.check()}
    inv = _inv_keep(p)

    def chunk(a, b):
        y, pre = ops.linear(x[a:b], W, bias, act, save_pre=True)
        return {"y": y * (keep[a:b].float() * inv), "pre": pre}
    _chunks_equal(N, E, big, chunk)
    for a, b in X.windows(N, E):
        assert np.array_equal(keep[a:b].cpu().numpy(), dropout_ref.keep_field(SEED, STEP, site, b - a, E, p, row0=a)), (a, b)
    # through ops: the field's row is the call's own row, so only the first chunk's rows can be compared -- past 2^31 elements it is
    # the C entry point above that is checked, not the ops wrapper (the same holds for act_bwd and gpt_layernorm with dropout=)
    a, b = _steps(N, E)[0]
    assert torch.equal(_bits(ops.linear(x[a:b], W, bias, act, dropout=(snap, site, p))), _bits(big["y"][a:b]))


def test_act_bwd_dropout(ops):
    """lipvq_act_bwd_drop_f32 [N, 2048]: (g m) act'(pre), the bits of the plain act-backward of g x field x inv_keep, chunk by chunk."""
    check, lib = _lib()
    case = _case("act_bwd_drop")
    N, E, p = case.N, case.W, case.p
    act, site, snap = ops.ACT_GELU, ops.DROPOUT_SITE_DEFAULT + 5, _snap()
    g, pre = _randn_big(31, N, E), _randn_big(32, N, E)
    keep = ops.dropout_keep(snap, site, N, E, p)
    fo = _FencedBig("gpre", N, E)
    check(lib.lipvq_act_bwd_drop_f32(g.data_ptr(), pre.data_ptr(), fo.ptr(), snap.data_ptr(), site, p, N, E, act, _stream()),
          "lipvq_act_bwd_drop_f32")
    torch.cuda.synchronize()
    inv = _inv_keep(p)
    _chunks_equal(N, E, {"gpre": fo.check()}, lambda a, b: {"gpre": ops.act_bwd(g[a:b] * (keep[a:b].float() * inv), pre[a:b], act)})
    a, b = _steps(N, E)[0]
    assert torch.equal(_bits(ops.act_bwd(g[a:b], pre[a:b], act, dropout=(snap, site, p))), _bits(fo.t[a:b]))


def test_dropout_keep_field(ops):
    """lipvq_dropout_keep_u8 on a field of more than 2^32 bytes: fenced, every byte 0 or 1, the window rows at byte 2^31 and byte
    2^32 against the numpy restatement, the first chunk against a call of that many rows.  (The entry point has no row offset:
    the whole-tensor agreement of two independent kernels on such a field is test_linear_dropout_epilogue's.)"""
    check, lib = _lib()
    case = _case("dropout_keep")
    N, W, p = case.N, case.W, case.p
    site, snap = 9, _snap()
    f = _FencedBig("keep", N, W, dtype=torch.uint8)
    check(lib.lipvq_dropout_keep_u8(snap.data_ptr(), site, N, W, p, f.ptr(), _stream()), "lipvq_dropout_keep_u8")
    torch.cuda.synchronize()
    field = f.check()
    over = torch.zeros((), dtype=torch.int64, device="cuda")
    kept = torch.zeros((), dtype=torch.int64, device="cuda")
    for a, b in _steps(N, W):
        over += (field[a:b] > 1).sum()
        kept += field[a:b].sum(dtype=torch.int64)
    assert int(over) == 0
    # 8.6e9 independent decisions: the kept fraction is within six standard deviations of 1 - p
    frac, sd = int(kept) / (N * W), math.sqrt(p * (1 - p) / (N * W))
    print(f"kept fraction {frac:.7f}, 1 - p = {1 - p}, six standard deviations {6 * sd:.2e}")
    assert abs(frac - (1 - p)) <= 6 * sd
    for a, b in X.windows(N, W, case.boundaries):
        assert np.array_equal(field[a:b].cpu().numpy(), dropout_ref.keep_field(SEED, STEP, site, b - a, W, p, row0=a)), (a, b)
    a, b = _steps(N, W)[0]
    assert torch.equal(ops.dropout_keep(snap, site, b, W, p), field[:b])


# ---------------------------------------------------------------------------------------------------
# A. LayerNorm of the backbone (lipvq_gpt_layernorm_f32 / _bwd_f32 and their dropout forms), E = 1024
# ---------------------------------------------------------------------------------------------------

def _ln_window_check(what, got, ref64, ref32, tol):
    err, dev = _rel(got, ref64), _rel(ref32, ref64)
    bound = max(tol, REF_FACTOR * dev)
    print(f"{what}: error {err:.3e}, fp32 torch's own {dev:.3e}, bound {bound:.3e}")
    assert err <= bound, what


def _ln_ref(s, w, bias, dtype):
    s, w, bias = (torch.from_numpy(np.asarray(t)).to(dtype) for t in (s, w, bias))
    return torch.nn.functional.layer_norm(s, (s.shape[-1],), w, bias, LN_EPS).numpy()


@pytest.mark.parametrize("name", ["layernorm_b_s", "layernorm_save"])
def test_layernorm(ops, name):
    check, lib = _lib()
    case = _case(name)
    N, E = case.N, case.W
    with_b = name == "layernorm_b_s"
    a = _randn_big(41, N, E)
    b = _randn_big(42, N, E) if with_b else None
    w, bias = _small(43, E) * 0.1 + 1.0, _small(44, E)
    f = {"y": _FencedBig("y", N, E)}
    if with_b:
        f["s"] = _FencedBig("s", N, E)
        rstd = None
    else:
        f["xhat"] = _FencedBig("xhat", N, E)
        rstd = _empty(N)
    check(lib.lipvq_gpt_layernorm_f32(a.data_ptr(), b.data_ptr() if with_b else None, w.data_ptr(), bias.data_ptr(), LN_EPS,
                                      f["s"].ptr() if with_b else None, f["y"].ptr(), None if with_b else f["xhat"].ptr(),
                                      None if with_b else rstd.data_ptr(), N, E, _stream()), "lipvq_gpt_layernorm_f32")
    torch.cuda.synchronize()
    big = {k: v.check() for k, v in f.items()}
    if rstd is not None:
        big["rstd"] = rstd

    def chunk(i, j):
        if with_b:
            s, y = ops.gpt_layernorm(a[i:j], b[i:j], w, bias, LN_EPS, want_s=True)
            return {"s": s, "y": y}
        _, y, xhat, rs = ops.gpt_layernorm(a[i:j], None, w, bias, LN_EPS, want_s=False, save=True)
        return {"y": y, "xhat": xhat, "rstd": rs}
    _chunks_equal(N, E, big, chunk)
    wins = X.windows(N, E)
    s_host = _win(a, wins) if not with_b else _win(a, wins) + _win(b, wins)                    # (fp32 sum, as the kernel forms it)
    if with_b:
        assert np.array_equal(_win(big["s"], wins), s_host)
    wc, bc = w.cpu().numpy(), bias.cpu().numpy()
    _ln_window_check(f"{name} y", _win(big["y"], wins), _ln_ref(s_host, wc, bc, torch.float64), _ln_ref(s_host, wc, bc, torch.float32), FWD_TOL)


def test_layernorm_dropout(ops):
    """lipvq_gpt_layernorm_drop_f32: the bits of the plain call on (a, b x field x inv_keep), chunk by chunk."""
    check, lib = _lib()
    case = _case("layernorm_drop")
    N, E, p = case.N, case.W, case.p
    site, snap = 4 * 2 + 1, _snap()
    a, b = _randn_big(51, N, E), _randn_big(52, N, E)
    w, bias = _small(53, E) * 0.1 + 1.0, _small(54, E)
    keep = ops.dropout_keep(snap, site, N, E, p)
    fy = _FencedBig("y", N, E)
    check(lib.lipvq_gpt_layernorm_drop_f32(a.data_ptr(), b.data_ptr(), w.data_ptr(), bias.data_ptr(), LN_EPS, snap.data_ptr(), site, p,
                                           None, fy.ptr(), None, None, N, E, _stream()), "lipvq_gpt_layernorm_drop_f32")
    torch.cuda.synchronize()
    inv = _inv_keep(p)
    _chunks_equal(N, E, {"y": fy.check()},
                  lambda i, j: {"y": ops.gpt_layernorm(a[i:j], b[i:j] * (keep[i:j].float() * inv), w, bias, LN_EPS, want_s=False)[1]})
    i, j = _steps(N, E)[0]
    assert torch.equal(_bits(ops.gpt_layernorm(a[i:j], b[i:j], w, bias, LN_EPS, want_s=False, dropout=(snap, site, p))[1]), _bits(fy.t[i:j]))


@pytest.mark.parametrize("name", ["layernorm_bwd", "layernorm_bwd_drop"])
def test_layernorm_bwd(ops, name):
    """gs (and the dropped branch's gradient): chunk-equal.  gw = sum_rows gy xhat and gb = sum_rows gy on the exact-sum operands: the
    int64 answer, bit for bit.  xhat is a fenced input: the call may not write it."""
    check, lib = _lib()
    case = _case(name)
    N, E, p = case.N, case.W, case.p
    drop = name.endswith("_drop")
    site, snap = 4 * 3 + 2, _snap()
    wins = X.windows(N, E)
    gy = _zeros_big(N, E)
    _plant_exact(gy, wins, 4)
    fx = _FencedBig("xhat", N, E)
    for i, j in _steps(N, E):
        fx.t[i:j].zero_()
    _plant_exact(fx.t, wins, 5)
    xhat = fx.t
    rstd = _randn_big(61, N).abs_().add_(0.5)
    w = _small(62, E) * 0.1 + 1.0
    f = {"gs": _FencedBig("gs", N, E)}
    gw, gb = _empty(E), _empty(E)
    ws = torch.empty(max(1, lib.lipvq_gpt_layernorm_bwd_workspace_bytes(N, E)), device="cuda", dtype=torch.uint8)
    if drop:
        f["gbr"] = _FencedBig("gbranch", N, E)
        check(lib.lipvq_gpt_layernorm_bwd_drop_f32(gy.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), w.data_ptr(), None, snap.data_ptr(), site, p,
                                                   f["gs"].ptr(), f["gbr"].ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), N, E, _stream()),
              "lipvq_gpt_layernorm_bwd_drop_f32")
    else:
        check(lib.lipvq_gpt_layernorm_bwd_f32(gy.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), w.data_ptr(), None, f["gs"].ptr(), gw.data_ptr(),
                                              gb.data_ptr(), ws.data_ptr(), N, E, _stream()), "lipvq_gpt_layernorm_bwd_f32")
    torch.cuda.synchronize()
    big = {k: v.check() for k, v in f.items()}
    fx.check()
    rows = X.window_rows(N, E)
    g64, x64 = X.exact_values(rows, E, 4), X.exact_values(rows, E, 5)
    assert np.array_equal(_win(xhat, wins), x64.astype(np.float32))                             # the input still holds what was planted
    want_gw, want_gb = (g64 * x64).sum(0), g64.sum(0)
    assert np.array_equal(gw.cpu().numpy(), want_gw.astype(np.float32)) and np.array_equal(gb.cpu().numpy(), want_gb.astype(np.float32))
    if drop:
        keep = ops.dropout_keep(snap, site, N, E, p)
        inv = _inv_keep(p)

        def chunk(i, j):
            gs = ops.gpt_layernorm_bwd(gy[i:j], xhat[i:j], rstd[i:j], w)[0]
            return {"gs": gs, "gbr": gs * (keep[i:j].float() * inv)}
    else:
        def chunk(i, j):
            return {"gs": ops.gpt_layernorm_bwd(gy[i:j], xhat[i:j], rstd[i:j], w)[0]}
    _chunks_equal(N, E, big, chunk)
    # fine check: rstd (g w - mean(g w) - xhat mean(g w xhat)) on the window rows, float64 against fp32 torch's own distance
    rs = _win(rstd, wins)[:, None]

    def ref(dtype):
        g, xh, r, ww = (torch.from_numpy(np.asarray(t, np.float32)).to(dtype) for t in (g64, x64, rs, w.cpu().numpy()))
        gw_ = g * ww
        return (r * (gw_ - gw_.mean(-1, keepdim=True) - xh * (gw_ * xh).mean(-1, keepdim=True))).numpy()
    _ln_window_check(f"{name} gs", _win(big["gs"], wins), ref(torch.float64), ref(torch.float32), BWD_TOL)


# ---------------------------------------------------------------------------------------------------
# A. the embedding stage's forward (lipvq_embed_rows_f32), E = 1024: the interleaved output past element 2^31
# ---------------------------------------------------------------------------------------------------

def _embed_three(embed_rows, out, table, idx, dense, pos, w, b, B, T, E):
    """The three calls of the interleave out [B][3 T][E] (tests/test_gpu_embed.py): indexed rows and dense rows with the time table
    on alternating slots of the first 2 T, dense rows without it on the last T.  Returns the indexed call's stats."""
    bs = 3 * T * E
    st = embed_rows(table, idx, pos, w, b, LN_EPS, out, B * T, T, bs, 2 * E, E, want_stats=True)
    embed_rows(dense, None, pos, w, b, LN_EPS, out, B * T, T, bs, 2 * E, 0)
    embed_rows(dense, None, None, w, b, LN_EPS, out, B * T, T, bs, E, 2 * T * E)
    return st


def test_embed_rows(ops, oracle):
    """Indexed and dense rows; batch stride 3 T E, time strides 2 E and E, offsets 0, E and 2 T E: the last batch's slots lie past
    element 2^31 of `out`.  Chunks are runs of whole batches; the fine check is the canonical oracle on the window batches, bit for
    bit (tests/test_gpu_embed.py's budget)."""
    case = _case("embed_rows")
    E, (T, B) = case.W, case.dims
    N, K = B * T, 1024
    assert B * 3 * T == case.N
    table, pos = _small(91, K, E), _small(92, T, E, scale=0.1)
    w, b = _small(93, E) * 0.1 + 1.0, _small(94, E, scale=0.1)
    idx = torch.randint(0, K, (N,), device="cuda", dtype=torch.int64, generator=torch.Generator(device="cuda").manual_seed(95))
    dense = _randn_big(96, N, E)
    fo = _FencedBig("out", B, 3 * T, E)
    st = _embed_three(ops.embed_rows, fo.t, table, idx, dense, pos, w, b, B, T, E)
    torch.cuda.synchronize()
    out = fo.check()
    per = max(1, X.CHUNK_ELEMS // (3 * T * E))
    for b0 in range(0, B, per):
        b1 = min(B, b0 + per)
        oc = torch.empty((b1 - b0, 3 * T, E), device="cuda")
        sc = _embed_three(ops.embed_rows, oc, table, idx[b0 * T:b1 * T], dense[b0 * T:b1 * T], pos, w, b, b1 - b0, T, E)
        assert torch.equal(_bits(oc), _bits(out[b0:b1])), f"out: batches {b0} .. {b1} of the big call differ from a call on them alone"
        assert torch.equal(_bits(sc), _bits(st[b0 * T:b1 * T])), f"stats: batches {b0} .. {b1}"
    tn, pn, wn, bn = (t.cpu().numpy() for t in (table, pos, w, b))
    for a_row, b_row in X.windows(case.N, E):                          # windows of output rows -> the batches that hold them
        b0, b1 = a_row // (3 * T), -(-b_row // (3 * T))
        ref = np.zeros((b1 - b0, 3 * T, E), np.float32)
        dn, ixn = dense[b0 * T:b1 * T].cpu().numpy(), idx[b0 * T:b1 * T].cpu().numpy()
        bs = 3 * T * E
        st_ref = oracle.embed_rows(tn, ixn, pn, wn, bn, LN_EPS, ref, T, bs, 2 * E, E, want_stats=True)
        oracle.embed_rows(dn, None, pn, wn, bn, LN_EPS, ref, T, bs, 2 * E, 0)
        oracle.embed_rows(dn, None, None, wn, bn, LN_EPS, ref, T, bs, E, 2 * T * E)
        assert np.array_equal(out[b0:b1].cpu().numpy(), ref), (b0, b1)
        assert np.array_equal(st[b0 * T:b1 * T].cpu().numpy(), st_ref), (b0, b1)


# ---------------------------------------------------------------------------------------------------
# A. the backbone's attention (lipvq_gpt_attention_f32 / _bwd_f32 / _prefix_f32 and the in-kernel source's forms), L = 128
# ---------------------------------------------------------------------------------------------------

def _batch_windows(case, per):
    """[(first batch entry, end)]: the runs of whole batch entries (`per` rows of the big operand each) that hold the case's windows."""
    out = []
    for a, b in X.windows(case.N, case.W, case.boundaries):
        b0, b1 = a // per, -(-b // per)
        assert b0 * per <= a and b <= b1 * per <= case.N and b1 - b0 <= 128 // per + 2
        out.append((b0, b1))
    return out


def _batch_steps(B, elems_per_batch):
    per = max(1, X.CHUNK_ELEMS // elems_per_batch)
    return [(b0, min(B, b0 + per)) for b0 in range(0, B, per)]


def _same_big(a, b, steps):
    """torch.equal on the int32 views, a run of batch entries at a time."""
    return all(torch.equal(_bits(a[i:j]), _bits(b[i:j])) for i, j in steps)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("name", ["gpt_attention_dh16", "gpt_attention_dh64"])
def test_gpt_attention(ops, name, causal):
    """Forward and backward, chunked over B.  dh16 (H = 32): with keep bytes [B, H, L, L] of more than 2^32 bytes, and the in-kernel
    source's forms bit-equal to the keep-byte forms over the whole tensors.  dh64 (H = 8): no dropout."""
    import gpt_ref
    check, lib = _lib()
    case = _case(name)
    (L, E, H, B), p = case.dims, case.p
    site, snap = 4 * 1 + 0, _snap()
    qkv = _randn_big(101, B * L, 3 * E).view(B, L, 3 * E)
    gout = _randn_big(102, B * L, E).view(B, L, E)
    keep, kp = None, 1.0
    if p:
        keep, kp = ops.dropout_keep(snap, site, B * H * L, L, p).view(B, H, L, L), 1.0 - p
        assert keep.numel() > X.B32
    f = {"out": _FencedBig("out", B, L, E), "lse": _FencedBig("lse", B, H, L), "gqkv": _FencedBig("gqkv", B, L, 3 * E), "delta": _FencedBig("delta", B, H, L)}
    kptr = keep.data_ptr() if p else None
    check(lib.lipvq_gpt_attention_f32(qkv.data_ptr(), f["out"].ptr(), f["lse"].ptr(), kptr, kp, B, L, E, H, int(causal), _stream()), "lipvq_gpt_attention_f32")
    check(lib.lipvq_gpt_attention_bwd_f32(qkv.data_ptr(), f["out"].ptr(), gout.data_ptr(), f["lse"].ptr(), f["gqkv"].ptr(), f["delta"].ptr(), kptr, kp,
                                          B, L, E, H, int(causal), _stream()), "lipvq_gpt_attention_bwd_f32")
    torch.cuda.synchronize()
    big = {k: v.check() for k, v in f.items()}
    steps = _batch_steps(B, L * 3 * E)
    for b0, b1 in steps:
        kc = keep[b0:b1] if p else None
        out, lse = ops.gpt_attention(qkv[b0:b1], H, causal, kc, kp)
        gq = ops.gpt_attention_bwd(qkv[b0:b1], out, gout[b0:b1], lse, H, causal, kc, kp)
        for k, v in (("out", out), ("lse", lse), ("gqkv", gq)):
            assert torch.equal(_bits(v), _bits(big[k][b0:b1])), f"{k}: batch entries {b0} .. {b1} of the big call differ from a call on them alone"
        del out, lse, gq
    if p:
        out2, lse2 = ops.gpt_attention(qkv, H, causal, dropout=(snap, site, p))
        assert _same_big(out2, big["out"], steps) and _same_big(lse2, big["lse"], steps)
        gq2 = ops.gpt_attention_bwd(qkv, out2, gout, lse2, H, causal, dropout=(snap, site, p))
        assert _same_big(gq2, big["gqkv"], steps)
        del out2, lse2, gq2
    mask = gpt_ref.causal_mask(L, causal)
    for b0, b1 in _batch_windows(case, L):
        qd = qkv[b0:b1].cpu().double().requires_grad_(True)
        ref = gpt_ref.attention_ref(qd, H, mask, keep[b0:b1].cpu() if p else None, kp)
        (ref * gout[b0:b1].cpu().double()).sum().backward()
        e_out, e_gq = _rel(big["out"][b0:b1].cpu(), ref.detach()), _rel(big["gqkv"][b0:b1].cpu(), qd.grad)
        print(f"{name} causal={causal} batch entries {b0} .. {b1}: out {e_out:.3e} gqkv {e_gq:.3e}")
        assert e_out <= FWD_TOL and e_gq <= BWD_TOL


def test_gpt_attention_prefix(ops):
    """64 new tokens over 64 cached ones, one prompt per sequence: both qkv tensors pass 2^31 elements.  Chunked over B; on the window
    batch entries the bits of gpt_attention over the concatenated tensor (the entry point's contract)."""
    check, lib = _lib()
    case = _case("gpt_attention_prefix")
    P, E, H, B = case.dims
    Lq = P
    pre = _randn_big(111, B * P, 3 * E).view(B, P, 3 * E)
    qkv = _randn_big(112, B * Lq, 3 * E).view(B, Lq, 3 * E)
    fo = _FencedBig("out", B, Lq, E)
    check(lib.lipvq_gpt_attention_prefix_f32(pre.data_ptr(), qkv.data_ptr(), fo.ptr(), B, B, P, Lq, E, H, _stream()), "lipvq_gpt_attention_prefix_f32")
    torch.cuda.synchronize()
    out = fo.check()
    for b0, b1 in _batch_steps(B, Lq * 3 * E):
        assert torch.equal(_bits(ops.gpt_attention_prefix(pre[b0:b1], qkv[b0:b1], H)), _bits(out[b0:b1])), (b0, b1)
    for b0, b1 in _batch_windows(case, Lq):
        whole = ops.gpt_attention(torch.cat([pre[b0:b1], qkv[b0:b1]], 1), H, True)[0]
        assert torch.equal(_bits(whole[:, P:].contiguous()), _bits(out[b0:b1])), (b0, b1)


# ---------------------------------------------------------------------------------------------------
# A. the policy's output heads (lipvq_gmm_head_f32, its sampling forms and backward; lipvq_action_head_f32 and its backward)
# ---------------------------------------------------------------------------------------------------

def _head_inputs(case, seed):
    N, E = case.N, case.W
    M, A = case.dims
    feats = _randn_big(seed, N, E)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    actions = torch.rand((N, A), device="cuda", generator=g) * 3.0 - 1.5
    return feats, actions, g


def _dicts_equal(N, E, big, keys, chunk_fn):
    _chunks_equal(N, E, {k: big[k] for k in keys}, lambda a, b: {k: v for k, v in chunk_fn(a, b).items() if k in keys})


def test_gmm_head(ops):
    """Per-row outputs (log_prob, pre, mean, scale, logits, the two samplers' actions, the backward's gpre): chunk-equal.  The summed
    log-probability: within 32 2^-24 sum |log_prob| of the float64 sum of the kernel's own rows, formed on the device
    (tests/test_gpu_gmm_edges.py, test_the_sum_is_every_tile_added_once).  pre on the windows: float64, any-order fp32 bound."""
    case = _case("heads")
    N, E = case.N, case.W
    M, A = case.dims
    feats, actions, g = _head_inputs(case, 131)
    sc = 1.0 / math.sqrt(E)
    params = (_small(133, M * A, E, scale=sc), _small(134, M * A), _small(135, M * A, E, scale=sc), _small(136, M * A),
              _small(137, M, E, scale=sc), _small(138, M))
    out = ops.gmm_head(feats, params, M, A, actions, want_pre=True, want_params=True, want_sum=True)
    keys = ("log_prob", "pre", "mean", "scale", "logits")
    _dicts_equal(N, E, out, keys, lambda a, b: ops.gmm_head(feats[a:b], params, M, A, actions[a:b], want_pre=True, want_params=True))
    lp = out["log_prob"].double()
    err, bound = abs(float(out["sum"].double() - lp.sum())), 32.0 * 2.0 ** -24 * float(lp.abs().sum())
    print(f"gmm sum: off its rows' float64 sum by {err:.3e}, rounding bound {bound:.3e}")
    assert err <= bound
    # the product stage on the windows
    wins = X.windows(N, E)
    xw = torch.from_numpy(_win(feats, wins)).double()
    Wall = torch.cat([params[0], params[2], params[4]]).cpu().double()
    ball = torch.cat([params[1], params[3], params[5]]).cpu().double()
    ref = xw @ Wall.t() + ball
    tol = R.gamma(E + 1) * (xw.abs() @ Wall.abs().t() + ball.abs()) + R.ulp32(ref)
    assert bool(((torch.from_numpy(_win(out["pre"], wins)).double() - ref).abs() <= tol).all())
    # the samplers: given noise (chunk-equal), and drawn in the kernel = the given-noise form on the noise written out
    u = torch.rand((N,), device="cuda", generator=g)
    eps = torch.randn((N, A), device="cuda", generator=g)
    act = ops.gmm_sample(feats, params, M, A, u, eps)
    _chunks_equal(N, E, {"action": act}, lambda a, b: {"action": ops.gmm_sample(feats[a:b], params, M, A, u[a:b], eps[a:b])})
    snap = _snap()
    drawn = ops.gmm_sample_draw(feats.view(1, N, E), params, M, A, snap)
    un, en = ops.gmm_noise(snap, 1, N, A)
    assert torch.equal(_bits(drawn), _bits(ops.gmm_sample(feats, params, M, A, un.view(-1), en.view(N, A))))
    # the backward from the saved pre (lipvq_gmm_head_bwd_f32 and lipvq_action_head_bwd_f32 write gpre [N, P] and nothing summed: the
    # weight and bias gradients of the heads are lipvq_wgrad_f32's, test_wgrad)
    gl = torch.randn((N,), device="cuda", generator=g)
    gpre = ops.gmm_head_bwd(out["pre"], actions, gl, None, M, A)
    _chunks_equal(N, E, {"gpre": gpre}, lambda a, b: {"gpre": ops.gmm_head_bwd(out["pre"][a:b], actions[a:b], gl[a:b], None, M, A)})


def test_action_head(ops):
    """actions and pre: chunk-equal, pre on the windows against float64; the backward's gpre from a gradient at the actions: chunk-equal."""
    case = _case("heads")
    N, E = case.N, case.W
    A = case.dims[1]
    feats, target, g = _head_inputs(case, 141)
    W, b = _small(143, A, E, scale=1.0 / math.sqrt(E)), _small(144, A)
    weights = (1.0, 0.5, 0.25)
    out = ops.action_head(feats, W, b, target=target, weights=weights, want_actions=True, want_pre=True)
    _dicts_equal(N, E, out, ("actions", "pre"), lambda i, j: ops.action_head(feats[i:j], W, b, want_actions=True, want_pre=True))
    # the four summed losses against tests/action_head_ref.py on the kernel's own per-row actions, float64 on the device, at the
    # budget of tests/test_gpu_action_head.py: max(1e-5, 4 x the fp32 restatement's own distance), relative
    import action_head_ref
    ref64 = action_head_ref.compute_losses(out["actions"].double(), target.double(), weights)
    ref32 = action_head_ref.compute_losses(out["actions"], target, weights)
    for i, k in enumerate(action_head_ref.LOSS_KEYS):
        want = float(ref64[k])
        err, dev = abs(float(out["losses"][i]) - want) / abs(want), abs(float(ref32[k]) - want) / abs(want)
        print(f"action head {k}: error {err:.3e}, fp32 restatement's own {dev:.3e}")
        assert err <= max(FWD_TOL, REF_FACTOR * dev), k
    wins = X.windows(N, E)
    xw = torch.from_numpy(_win(feats, wins)).double()
    ref = xw @ W.cpu().double().t() + b.cpu().double()
    tol = R.gamma(E + 1) * (xw.abs() @ W.cpu().double().abs().t() + b.cpu().double().abs()) + R.ulp32(ref)
    assert bool(((torch.from_numpy(_win(out["pre"], wins)).double() - ref).abs() <= tol).all())
    gy = torch.randn((N, A), device="cuda", generator=g)
    gpre = ops.action_head_bwd(out["pre"], gy=gy)
    _chunks_equal(N, E, {"gpre": gpre}, lambda i, j: {"gpre": ops.action_head_bwd(out["pre"][i:j], gy=gy[i:j])})


# ---------------------------------------------------------------------------------------------------
# A. flat elementwise kernels: 2^31 + 4099 elements, and 2^32 + 4099 (a uint32 element index wraps there)
# ---------------------------------------------------------------------------------------------------

def _flat_inputs(case, seed):
    """Two read-only views, X.FLAT_SHIFT elements apart, of one buffer of standard normals."""
    n = case.N
    buf = _randn_big(seed, n + X.FLAT_SHIFT)
    return buf, buf[:n], buf[X.FLAT_SHIFT:X.FLAT_SHIFT + n]


@pytest.mark.parametrize("size", ["2p31", "2p32"])
def test_ste(ops, oracle, size):
    check, lib = _lib()
    case = _case("ste_" + size)
    n = case.N
    buf, ze, zq = _flat_inputs(case, 71)
    fo = _FencedBig("out", n)
    check(lib.lipvq_ste_f32(ze.data_ptr(), zq.data_ptr(), fo.ptr(), n, _stream()), "lipvq_ste_f32")
    torch.cuda.synchronize()
    out = fo.check()
    _chunks_equal(n, 1, {"out": out}, lambda a, b: {"out": ops.ste(ze[a:b], zq[a:b])})
    wins = X.windows(n, 1, case.boundaries)
    assert np.array_equal(_win(out, wins), oracle.ste(_win(ze, wins).reshape(-1, 1), _win(zq, wins).reshape(-1, 1)).reshape(-1))


@pytest.mark.parametrize("size", ["2p31", "2p32"])
def test_scaled_diff(ops, size):
    check, lib = _lib()
    case = _case("scaled_diff_" + size)
    n = case.N
    buf, a, b = _flat_inputs(case, 72)
    alpha, gscale = 0.37, torch.tensor([1.7], device="cuda")
    fo = _FencedBig("out", n)
    check(lib.lipvq_scaled_diff_f32(a.data_ptr(), b.data_ptr(), None, alpha, gscale.data_ptr(), fo.ptr(), n, _stream()), "lipvq_scaled_diff_f32")
    torch.cuda.synchronize()
    out = fo.check()
    _chunks_equal(n, 1, {"out": out}, lambda i, j: {"out": ops.scaled_diff(a[i:j], b[i:j], alpha, gscale=gscale)})
    wins = X.windows(n, 1, case.boundaries)
    want = R.scaled_diff_fp32(torch.from_numpy(_win(a, wins)), torch.from_numpy(_win(b, wins)), alpha, gscale)
    assert np.array_equal(_win(out, wins), want.numpy())


@pytest.mark.parametrize("size", ["2p31", "2p32"])
def test_act_bwd(ops, size):
    check, lib = _lib()
    case = _case("act_bwd_" + size)
    n = case.N
    buf, g, pre = _flat_inputs(case, 73)
    act = ops.ACT_GELU
    fo = _FencedBig("out", n)
    check(lib.lipvq_act_bwd_f32(g.data_ptr(), pre.data_ptr(), fo.ptr(), n, act, _stream()), "lipvq_act_bwd_f32")
    torch.cuda.synchronize()
    out = fo.check()
    _chunks_equal(n, 1, {"out": out}, lambda a, b: {"out": ops.act_bwd(g[a:b], pre[a:b], act)})
    wins = X.windows(n, 1, case.boundaries)
    ref, tol = R.elementwise_ref_and_budget(_win(g, wins), _win(pre, wins), act, R.DELTA_ACT[act])
    err = (torch.from_numpy(_win(out, wins)).double() - ref).abs()
    print(f"act_bwd {size}: largest error / budget {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())


# ---------------------------------------------------------------------------------------------------
# B. reductions over rows: exact-sum operands, the int64 answer bit for bit
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("name", ["wgrad_wide_g", "wgrad_wide_h"])
def test_wgrad(ops, name, mode):
    """ops.wgrad, ops.wgrad_bf16, ops.wgrad_bf16x3: integers |v| <= 8 are bf16 numbers (their lo part is 0), so all three modes owe
    the int64 products bit for bit.  The gathered form (hidx) exists for lipvq_wgrad_f32 only: the bf16 entry points take no index."""
    case = _case(name)
    wgrad = {"fp32": ops.wgrad, "bf16": ops.wgrad_bf16, "bf16x3": ops.wgrad_bf16x3}[mode]
    N, (J, Kd) = case.N, case.dims
    wins = X.windows(N, case.W)
    rows = X.window_rows(N, case.W)
    G, H = _zeros_big(N, J), _zeros_big(N, Kd)
    g64, h64 = X.exact_values(rows, J, 1), X.exact_values(rows, Kd, 2)

    def same(got, want, what):
        gW, gb = got
        wW, wb = want
        assert np.array_equal(gW.cpu().numpy(), wW.astype(np.float32)), f"{name} {mode} {what}: gW"
        assert np.array_equal(gb.cpu().numpy(), wb.astype(np.float32)), f"{name} {mode} {what}: gb"

    _plant_exact(G, wins, 1)
    _plant_exact(H, wins, 2)
    same(wgrad(G, H), (g64.T @ h64, g64.sum(0)), "values x values")
    if name == "wgrad_wide_g" and mode == "fp32":
        # the gathered form: row n of H is table[hidx[n]]
        T = 1000
        t64 = X.exact_values(np.arange(T), Kd, 8)
        table = torch.from_numpy(t64.astype(np.float32)).cuda()
        hidx = (torch.arange(N, device="cuda", dtype=torch.int64) * 7 + 5) % T
        same(ops.wgrad(G, table, hidx=hidx), (g64.T @ t64[(rows * 7 + 5) % T], g64.sum(0)), "values x gathered table")
        del hidx
    # count operands: ones on EVERY row with r % 8 == 0 -- each of those rows is added exactly once
    ncount = len(X.count_rows(N))
    cw = np.isin(rows, X.count_rows(N))
    for a, b in wins:
        G[a:b].zero_()
    _plant_count(G)
    same(wgrad(G, H), (np.broadcast_to(h64[cw].sum(0), (J, Kd)), np.full(J, ncount)), "count x values")
    for a, b in wins:
        H[a:b].zero_()
    _plant_count(H)
    same(wgrad(G, H), (np.full((J, Kd), ncount), np.full(J, ncount)), "count x count")
    for a, b in _steps(N, J):
        G[a:b].zero_()                                     # (every count row goes: G is the values again)
    _plant_exact(G, wins, 1)
    same(wgrad(G, H), (np.repeat(g64[cw].sum(0)[:, None], Kd, 1), g64.sum(0)), "values x count")


@pytest.mark.parametrize("route", list(X.SCATTER_ROUTES) + ["deterministic"])
def test_scatter_add(ops, route):
    case = _case("scatter_add")
    N, D, (K, _) = case.N, case.W, case.dims
    wins = X.windows(N, D)
    rows = X.window_rows(N, D)
    r = torch.arange(N, device="cuda", dtype=torch.int64)
    idx = (r * 5 + r // 64 + 3) % K
    del r
    assert np.array_equal(_win(idx, wins), X.scatter_code(rows, K))
    if route == "deterministic":
        assert ops._scatter_route(N, K, D, True) == "sequential_sorted"

    def run(g):
        return ops.scatter_add(g, idx, K, deterministic=True) if route == "deterministic" else ops.scatter_add(g, idx, K, route=route)
    g = _zeros_big(N, D)
    _plant_exact(g, wins, 3)
    v64 = X.exact_values(rows, D, 3)
    want = np.zeros((K, D), np.int64)
    np.add.at(want, X.scatter_code(rows, K), v64)
    assert np.array_equal(run(g).cpu().numpy(), want.astype(np.float32)), f"{route}: values"
    for a, b in wins:
        g[a:b].zero_()
    _plant_count(g)
    counts = np.bincount(X.scatter_code(X.count_rows(N), K), minlength=K)
    assert np.array_equal(run(g).cpu().numpy(), np.repeat(counts[:, None], D, 1).astype(np.float32)), f"{route}: count"


def test_mse_pair(ops):
    """The sums run in double: the integer sum is exact, the stored mean is float32(sum / n).  The big pair in each position."""
    case = _case("mse_pair")
    n = case.N
    wins = X.windows(n, 1, case.boundaries)
    xr, x = _zeros_big(n, 1).view(-1), _zeros_big(n, 1).view(-1)
    _plant_exact(xr, wins, 6)
    _plant_exact(x, wins, 7)
    S = X.mse_exact_sum(n)
    nz = 1000
    z64 = X.exact_values(np.arange(nz), 1, 8)[:, 0], X.exact_values(np.arange(nz), 1, 9)[:, 0]
    zq, ze = _f32(z64[0]), _f32(z64[1])
    Sz = int(((z64[0] - z64[1]) ** 2).sum())
    m_big, m_small = np.float32(S / n), np.float32(Sz / nz)
    assert m_big > 0
    assert np.array_equal(ops.mse_pair(xr, x, zq, ze).cpu().numpy(), np.array([m_big, m_small], np.float32))
    assert np.array_equal(ops.mse_pair(zq, ze, xr, x).cpu().numpy(), np.array([m_small, m_big], np.float32))
    w = np.float32(0.25)
    q = w * m_big
    assert np.array_equal(ops.mse_pair_loss(zq, ze, xr, x, 0.25, ops.LOSS_LLFQ).cpu().numpy(),
                          np.array([m_small, m_big, (m_small + q) + q], np.float32))
    assert np.array_equal(ops.mse_pair_loss(zq, ze, xr, x, 0.25, ops.LOSS_VQ).cpu().numpy(),
                          np.array([m_small, m_big, m_small + (m_big + q)], np.float32))


def test_grad_norm_and_scale(ops):
    """clip_grad_norm_'s three launches on a gradient list whose first tensor has 2^31 + 4099 elements.  lipvq_grad_sumsq_f32 +
    lipvq_clip_coef_f64 on the exact-sum operands: sumsq is the integer, exactly (the sums run in double).  lipvq_grad_scale_f32
    (in place, fenced) on standard normals: the bits of the same call on a copy of each chunk, and g * (float)clip_coef on the windows."""
    from lipvq_vae_amd.optim import _GradNorm, _numels, _ptrs
    check, lib = _lib()
    case = _case("grad_norm")
    n = case.N
    wins = X.windows(n, 1, case.boundaries)
    f = _FencedBig("g", n)
    g = f.t
    for a, b in _steps(n, 1):
        g[a:b].zero_()
    _plant_exact(g, wins, 10)
    g2 = _f32(X.exact_values(np.arange(1000), 1, 11)[:, 0])
    S = X.grad_exact_sumsq(n, 1000)
    stats = _GradNorm().run([g, g2], 1.0).cpu()
    assert float(stats[2]) == float(S) and abs(float(stats[0]) - math.sqrt(S)) <= 2.0 ** -52 * math.sqrt(S)
    assert float(stats[1]) == 1.0 / (float(stats[0]) + 1e-6) and float(stats[1]) < 1.0
    # the scale, in place, on standard normals
    gen = torch.Generator(device="cuda")
    for i, (a, b) in enumerate(_steps(n, 1)):
        gen.manual_seed(121 * 100003 + i)
        g[a:b].normal_(generator=gen)
    orig = _empty(n)
    for a, b in _steps(n, 1):
        orig[a:b].copy_(g[a:b])
    stats = _GradNorm().run([g, g2], 1000.0)
    coef = float(stats[1].cpu())
    assert 0.0 < coef < 1.0                                                   # (the norm is about 46 341: the scale really scales)
    check(lib.lipvq_grad_scale_f32(_ptrs([g]), _numels([g]), 1, stats.data_ptr(), _stream()), "lipvq_grad_scale_f32")
    torch.cuda.synchronize()
    f.check()

    def chunk(a, b):
        c = orig[a:b].clone()
        check(lib.lipvq_grad_scale_f32(_ptrs([c]), _numels([c]), 1, stats.data_ptr(), _stream()), "lipvq_grad_scale_f32")
        return {"g": c}
    _chunks_equal(n, 1, {"g": g}, chunk)
    assert np.array_equal(_win(g, wins), _win(orig, wins) * np.float32(coef))


# ---------------------------------------------------------------------------------------------------
# C. the binning tokenizer: lipvq_bin_discretize_f32's [A][N] int64 output, lipvq_bin_hidden_f32's h [N, 256]
# ---------------------------------------------------------------------------------------------------

def test_bin_discretize(ops, oracle):
    case = _case("bin_discretize")
    N, A, nb = case.N, case.W, case.dims[0]
    x = _randn_big(151, N, A)
    rmin, rmax = torch.full((A,), -2.5, device="cuda"), torch.full((A,), 2.75, device="cuda")       # (values outside: the clamps)
    bins = ops.bin_discretize(x, rmin, rmax, nb)
    assert bins.shape == (A, N) and bins.numel() > X.B31
    for a, b in _steps(N, A):
        assert torch.equal(ops.bin_discretize(x[a:b], rmin, rmax, nb), bins[:, a:b]), (a, b)
    for a, b in X.windows(N, A):
        want = oracle.bin_discretize(x[a:b].cpu().numpy(), rmin.cpu().numpy(), rmax.cpu().numpy(), nb)
        assert np.array_equal(bins[:, a:b].cpu().numpy(), want), (a, b)


def test_bin_hidden(ops, oracle):
    check, lib = _lib()
    case = _case("bin_hidden")
    N, H, nb, A = case.N, case.W, case.dims[0], X.BIN_A
    g = torch.Generator(device="cuda").manual_seed(152)
    bins = torch.randint(0, nb, (A, N), device="cuda", dtype=torch.int64, generator=g)
    P, b1 = _small(153, A, nb, H, scale=0.5), _small(154, H)
    fh, fpre = _FencedBig("h", N, H), _FencedBig("pre", N, H)
    check(lib.lipvq_bin_hidden_f32(bins.data_ptr(), P.data_ptr(), b1.data_ptr(), fh.ptr(), fpre.ptr(), N, A, nb, H, _stream()), "lipvq_bin_hidden_f32")
    torch.cuda.synchronize()
    big = {"h": fh.check(), "pre": fpre.check()}
    _chunks_equal(N, H, big, lambda a, b: dict(zip(("h", "pre"), ops.bin_hidden(bins[:, a:b].contiguous(), P, b1, save_pre=True))))
    for a, b in X.windows(N, H):
        h_ref, pre_ref = oracle.bin_hidden(bins[:, a:b].cpu().numpy(), P.cpu().numpy(), b1.cpu().numpy(), save_pre=True)
        assert np.array_equal(big["pre"][a:b].cpu().numpy(), pre_ref) and np.array_equal(big["h"][a:b].cpu().numpy(), h_ref), (a, b)


def _adam_ref64(p, g, m, v, lr, b1, b2, eps, wd, decoupled, coef):
    """One step (t = 1) of torch.optim.AdamW (decoupled) / Adam with L2 (not), the gradient scaled by coef first: float64 numpy."""
    p, g, m, v = (np.asarray(t, np.float64) for t in (p, g, m, v))
    g = g * coef
    if decoupled:
        p = p * (1.0 - lr * wd)
    elif wd:
        g = g + wd * p
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    return p - lr / (1.0 - b1) * (m / (np.sqrt(v) / math.sqrt(1.0 - b2) + eps)), m, v


@pytest.mark.parametrize("form", ["adamw", "adam_decoupled", "adam_l2_clipped"])
def test_adam_step(ops, form):
    """The fused step on one tensor of 2^31 + 4099 elements: lipvq_adamw_f32, and lipvq_adam_f32 in its decoupled form and as Adam
    with L2 and a clip coefficient.  p, exp_avg and exp_avg_sq are updated in place inside fences; the bits of the same call on every
    chunk of the inputs (regenerated from their seeds); the windows against float64 at tests/test_gpu_update_edges.py's bounds
    (2e-6 max(1, max|p|) on the parameters, rtol 1e-5 on exp_avg_sq); exp_avg within its three roundings."""
    from lipvq_vae_amd.optim import _numels, _ptrs
    check, lib = _lib()
    case = _case("adam_step")
    n = case.N
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    decoupled = form != "adam_l2_clipped"
    stats = torch.tensor([3.0, 0.37, 9.0, 1.2321], dtype=torch.float64, device="cuda") if form == "adam_l2_clipped" else None
    coef = 0.37 if stats is not None else 1.0
    gen = torch.Generator(device="cuda")

    def piece(kind, i, out):
        """Chunk i of p (0), exp_avg (1) or exp_avg_sq (2) as it is before the step, into `out`."""
        gen.manual_seed((160 + kind) * 100003 + i)
        out.normal_(generator=gen)
        if kind == 1:
            out.mul_(0.1)
        if kind == 2:
            out.square_()
        return out
    f = [_FencedBig(w, n) for w in ("p", "exp_avg", "exp_avg_sq")]
    steps = _steps(n, 1)
    for kind, fb in enumerate(f):
        for i, (a, b) in enumerate(steps):
            piece(kind, i, fb.t[a:b])
    g = _randn_big(165, n)
    wins = X.windows(n, 1, case.boundaries)
    before = [_win(fb.t, wins) for fb in f]
    ws = torch.empty(lib.lipvq_adamw_workspace_bytes() // 4, dtype=torch.float32, device="cuda")

    def run(p, gr, m, v):
        step = torch.zeros((), dtype=torch.float32, device="cuda")
        args = (_ptrs([p]), _ptrs([gr]), _ptrs([m]), _ptrs([v]), _ptrs([step]), _numels([p]), 1, lr, b1, b2, eps, wd)
        if form == "adamw":
            check(lib.lipvq_adamw_f32(*args, ws.data_ptr(), _stream()), "lipvq_adamw_f32")
        else:
            check(lib.lipvq_adam_f32(*args, int(decoupled), None, None if stats is None else stats.data_ptr(), ws.data_ptr(), _stream()),
                  "lipvq_adam_f32")
        return step
    step = run(f[0].t, g, f[1].t, f[2].t)
    torch.cuda.synchronize()
    assert float(step) == 1.0
    big = {w: fb.check() for w, fb in zip(("p", "m", "v"), f)}
    for i, (a, b) in enumerate(steps):
        c = [piece(kind, i, _empty(b - a)) for kind in range(3)]
        run(c[0], g[a:b], c[1], c[2])
        for w, t in zip(("p", "m", "v"), c):
            assert torch.equal(_bits(t), _bits(big[w][a:b])), f"{w}: elements {a} .. {b} of the big step differ from a step on them alone"
    p64, m64, v64 = _adam_ref64(before[0], _win(g, wins), before[1], before[2], lr, b1, b2, eps, wd, decoupled, coef)
    gp, gm, gv = (_win(big[w], wins) for w in ("p", "m", "v"))
    assert np.abs(gp - p64).max() <= 2e-6 * max(1.0, np.abs(p64).max())
    assert np.allclose(gv, v64, rtol=1e-5, atol=1e-12)
    # exp_avg = m + (g' - m)(1 - b1) is three fp32 roundings on terms no larger than |m| + |g'|: four units of 2^-24 of that
    g1 = np.abs(np.asarray(_win(g, wins), np.float64) * coef) + (0.0 if decoupled else wd * np.abs(before[0]))
    assert bool((np.abs(gm - m64) <= 4.0 * 2.0 ** -24 * (np.abs(before[1]) + g1)).all())


def test_ema_update_counts(ops):
    """lipvq_ema_update_f32 with the counts a batch past 2^31 elements produces (the usage of 10.3 M rows), and with counts that are
    themselves above 2^31: float64 at tests/test_gpu_update_edges.py's bound, 1e-5 (1 + |want|)."""
    case = _case("scatter_add")
    N, D, K = case.N, case.W, case.dims[0]
    counts = torch.zeros(K, dtype=torch.int64, device="cuda")
    r = torch.arange(N, device="cuda", dtype=torch.int64)
    counts += torch.bincount((r * 5 + r // 64 + 3) % K, minlength=K)
    del r
    assert int(counts.sum()) == N
    decay, eps = 0.99, 1e-5
    for shift in (0, X.B31 + 12345):
        cnt = counts + shift
        cs, es, dw, cb = _small(171, K).abs() * 1e6 + 1.0, _small(172, K, D), _small(173, K, D) * 1e3, torch.zeros(K, D, device="cuda")
        cs0, es0 = cs.cpu().double(), es.cpu().double()
        ops.ema_update(cs, es, cnt, dw, cb, decay, eps)
        cs1 = decay * cs0 + (1.0 - decay) * cnt.cpu().double()
        es1 = decay * es0 + (1.0 - decay) * dw.cpu().double()
        tot = cs1.sum()
        want = es1 / ((cs1 + eps) / (tot + K * eps) * tot)[:, None]
        for got, ref, what in ((cs, cs1, "cluster_size"), (es, es1, "embed_sum"), (cb, want, "codebook")):
            assert bool(((got.cpu().double() - ref).abs() <= 1e-5 * (1.0 + ref.abs())).all()), (what, shift)


def test_embed_rows_bwd(ops):
    """lipvq_embed_rows_bwd_det_f32 (the fixed-order route ops.embed_rows_bwd takes) with gout [B][3 T][E] past 2^31 elements, on the
    exact-sum operands of extent_cases.embed_bwd_expected: g_pos, g_lnw, g_lnb and g_src equal numerator / 1024, bit for bit, indexed
    (the table's gradient through the counting-sort scatter) and dense (g_src holds every row's gradient: zero off the windows)."""
    case = _case("embed_rows_bwd")
    E, (T, B) = case.W, case.dims
    N, K = B * T, X.EMBED_K
    gout = _zeros_big(case.N, E)
    _plant_exact(gout, X.windows(case.N, E), 13)
    stats = torch.zeros((N, 2), device="cuda")
    stats[:, 1] = 1.0
    ln_w = torch.ones(E, device="cuda")
    bs = 3 * T * E

    def f32(num):
        return (np.asarray(num, np.float64) / E).astype(np.float32)
    # indexed: the table, the time table
    x = X.embed_bwd_expected(case, True)
    table = _exact_dev(np.arange(K), E, 12)
    pos = torch.from_numpy((X.exact_values(np.arange(T), E, 14) // 4).astype(np.float32)).cuda()
    n_dev = torch.arange(N, device="cuda", dtype=torch.int64)
    idx = (n_dev * 7 + n_dev // 13 + 5) % K
    del n_dev
    assert np.array_equal(idx[torch.from_numpy(x["n"]).cuda()].cpu().numpy(), X.embed_index(x["n"]))
    g_src, g_pos, g_lnw, g_lnb = (torch.zeros(sh, device="cuda") for sh in ((K, E), (T, E), (E,), (E,)))
    ops.embed_rows_bwd(gout, table, idx, pos, stats, ln_w, g_src, g_pos, g_lnw, g_lnb, N, T, bs, 2 * E, E)
    for got, what in ((g_src, "g_src"), (g_pos, "g_pos"), (g_lnw, "g_lnw"), (g_lnb, "g_lnb")):
        assert np.array_equal(got.cpu().numpy(), f32(x[what])), f"indexed {what}"
    del idx, g_src
    # dense rows, no time table: g_src is every row's own gradient
    x = X.embed_bwd_expected(case, False)
    rows = torch.from_numpy(x["n"]).cuda()
    src = _zeros_big(N, E)
    src[rows] = _exact_dev(x["n"], E, 15)
    g_src = _empty(N, E)
    g_pos, g_lnw, g_lnb = (torch.zeros(sh, device="cuda") for sh in ((T, E), (E,), (E,)))
    ops.embed_rows_bwd(gout, src, None, None, stats, ln_w, g_src, g_pos, g_lnw, g_lnb, N, T, bs, E, 2 * T * E)
    for got, what in ((g_pos, "g_pos"), (g_lnw, "g_lnw"), (g_lnb, "g_lnb")):
        assert np.array_equal(got.cpu().numpy(), f32(x[what])), f"dense {what}"
    assert np.array_equal(g_src[rows].cpu().numpy(), f32(x["gv"]))
    live = torch.zeros((), dtype=torch.int64, device="cuda")
    for a, b in _steps(N, E):
        live += (g_src[a:b] != 0).any(1).sum()
    assert int(live) == int((x["gv"] != 0).any(1).sum())                       # every other row's gradient is zero


@pytest.mark.parametrize("entry", ["nearest_norm", "nearest_sqsum", "nearest_rows"])
def test_nearest(ops, oracle, entry):
    """The exact nearest-code kernels on z [N, 208], N = 10.3 M, K = 64: ops.nearest under both distance rules
    (nearest_direct_kernel) and ops.nearest_rows (nearest_rows_kernel, whose row count travels as an int).  idx and z_q: chunk-equal;
    usage: the int64 sum of the chunks' usage and the histogram of idx; the windows against the canonical oracle, bit for bit."""
    case = _case("nearest")
    N, D, K = case.N, case.W, case.dims[0]
    z, cb = _randn_big(181, N, D), _small(182, K, D)
    dist = ops.DIST_SQSUM if entry == "nearest_sqsum" else ops.DIST_NORM

    def run(zz):
        usage = torch.zeros(K, dtype=torch.int64, device="cuda")
        if entry == "nearest_rows":
            idx, zq = ops.nearest_rows(zz, cb, usage=usage)            # (the default route: above 4 096 rows it is the row kernels)
        else:
            idx, zq, _ = ops.nearest(zz, cb, dist, usage=usage)
        return idx, zq, usage
    idx, zq, usage = run(z)
    total = torch.zeros(K, dtype=torch.int64, device="cuda")
    for a, b in _steps(N, D):
        ic, qc, uc = run(z[a:b])
        assert torch.equal(ic, idx[a:b]) and torch.equal(_bits(qc), _bits(zq[a:b])), (a, b)
        total += uc
    assert torch.equal(usage, total) and torch.equal(usage, torch.bincount(idx, minlength=K)) and int(usage.sum()) == N
    for a, b in X.windows(N, D):
        i_ref, q_ref, _ = oracle.nearest(z[a:b].cpu().numpy(), cb.cpu().numpy(), dist)
        assert np.array_equal(idx[a:b].cpu().numpy(), i_ref) and np.array_equal(zq[a:b].cpu().numpy(), q_ref), (a, b)


# ---------------------------------------------------------------------------------------------------
# C. the tokenizer path: the three-layer stack with y [N, 256], the screened search and the fused launches with z [N, 208]
# ---------------------------------------------------------------------------------------------------

def _mlp_weights(dims, seed):
    K0, J0, J1, J2 = dims
    rng = np.random.default_rng(seed)
    W = [rng.standard_normal(sh).astype(np.float32) * sc for sh, sc in (((J0, K0), 0.5), ((J1, J0), 0.2), ((J2, J1), 0.2))]
    b = [rng.standard_normal(J).astype(np.float32) for J in (J0, J1, J2)]
    return W, b


@pytest.mark.parametrize("name", ["mlp3", "mlp3_wg"])
def test_mlp3(ops, oracle, name):
    """lipvq_mlp3_f32 with y [N, 256]: hidden (128, 64) runs the LDS-resident kernel, hidden (32, 32) the workgroup kernel.  y and the
    saved pre-activations: chunk-equal, the windows against the canonical oracle bit for bit.  mlp3: then lipvq_mlp3_loss_f32 on the
    same rows -- its y the same bits, its two means and loss within 1e-7 of lipvq_mse_pair_loss_f32's (tests/test_gpu_fused.py's budget)."""
    check, lib = _lib()
    case = _case(name)
    N, dims = case.N, case.dims
    K0, J0, J1, J2 = dims
    acts = (ops.ACT_GELU, ops.ACT_GELU, ops.ACT_NONE)
    W, b = _mlp_weights(dims, 191)
    packed = ops.mlp3_pack(*(_f32(t) for t in (W[0], b[0], W[1], b[1], W[2], b[2])))
    x = _randn_big(192, N, K0)
    full = name == "mlp3"
    fy = _FencedBig("y", N, J2)
    fp2 = _FencedBig("pre2", N, J2) if full else None
    pre0, pre1 = (_empty(N, J0), _empty(N, J1)) if full else (None, None)
    check(lib.lipvq_mlp3_f32(x.data_ptr(), None, packed.buf.data_ptr(), fy.ptr(), pre0.data_ptr() if full else None,
                             pre1.data_ptr() if full else None, fp2.ptr() if full else None, N, K0, J0, J1, J2, *acts, _stream()), "lipvq_mlp3_f32")
    torch.cuda.synchronize()
    big = {"y": fy.check()}
    if full:
        big.update(pre0=pre0, pre1=pre1, pre2=fp2.check())

    def chunk(i, j):
        if not full:
            return {"y": ops.mlp3(x[i:j], packed, acts)}
        y, pre = ops.mlp3(x[i:j], packed, acts, save_pre=True)
        return {"y": y, "pre0": pre[0], "pre1": pre[1], "pre2": pre[2]}
    _chunks_equal(N, J2, big, chunk)
    wins = X.windows(N, J2)
    y_ref, pre_ref = oracle.mlp3(_win(x, wins), W[0], b[0], W[1], b[1], W[2], b[2], acts, save_pre=True)
    assert np.array_equal(_win(big["y"], wins), y_ref)
    if not full:
        return
    for k in range(3):
        assert np.array_equal(_win(big[f"pre{k}"], wins), pre_ref[k]), k
    del pre0, pre1, big["pre0"], big["pre1"]
    target, latent = _randn_big(193, N, J2), _randn_big(194, N, K0)
    assert ops.mlp3_loss_supported(N, packed)
    y2, none, l3 = ops.mlp3_loss(x, packed, acts, None, target, latent, 0.25, ops.LOSS_LLFQ)
    assert none is None
    for i, j in _steps(N, J2):
        assert torch.equal(_bits(y2[i:j]), _bits(big["y"][i:j])), (i, j)
    l3_u = ops.mse_pair_loss(y2, target, x, latent, 0.25, ops.LOSS_LLFQ)
    print(f"mlp3_loss {l3.tolist()} against the separate launches' {l3_u.tolist()}")
    assert torch.allclose(l3, l3_u, rtol=1e-7, atol=0)


def test_mlp3_bwd(ops):
    """lipvq_mlp3_bwd_f32 with gy [N, 256] down to gx [N, 8]: g1, g0 and gx chunk-equal; on the windows each link against float64 from
    the kernel's own upstream gradient, at tests/test_gpu_backward.py's layer budget."""
    case = _case("mlp3_bwd")
    N, dims = case.N, case.dims
    K0, J0, J1, J2 = dims
    acts = (ops.ACT_GELU, ops.ACT_GELU, ops.ACT_NONE)
    W, _ = _mlp_weights(dims, 195)
    packed_bwd = ops.mlp3_pack_bwd(*(_f32(t) for t in W))
    gy, pre0, pre1 = _randn_big(196, N, J2), _randn_big(197, N, J0), _randn_big(198, N, J1)
    g2, g1, g0, gx = ops.mlp3_bwd(gy, (pre0, pre1, None), packed_bwd, acts)
    assert g2 is gy
    big = {"g1": g1, "g0": g0, "gx": gx}

    def chunk(i, j):
        _, c1, c0, cx = ops.mlp3_bwd(gy[i:j], (pre0[i:j], pre1[i:j], None), packed_bwd, acts)
        return {"g1": c1, "g0": c0, "gx": cx}
    _chunks_equal(N, J2, big, chunk)
    wins = X.windows(N, J2)
    w = {k: torch.from_numpy(_win(t, wins)) for k, t in (("gy", gy), ("pre0", pre0), ("pre1", pre1), ("g1", g1), ("g0", g0), ("gx", gx))}
    for got, up, Wl, pre, act in (("g1", "gy", W[2], w["pre1"], acts[1]), ("g0", "g1", W[1], w["pre0"], acts[0]), ("gx", "g0", W[0], None, ops.ACT_NONE)):
        ref, tol = R.layer_ref_and_budget(w[up], torch.from_numpy(Wl), pre, act, R.DELTA_ACT[act])
        err = (w[got].double() - ref).abs()
        print(f"mlp3_bwd {got}: largest error / budget {float((err / tol).max()):.3f}")
        assert bool((err <= tol).all()), got


def _search_outputs_agree(N, D, K, big, run, z_of, oracle_rows):
    """idx, z_q (and z_e): chunk-equal; usage = the int64 sum of the chunks' usage = the histogram of idx; windows bit for bit."""
    total = torch.zeros(K, dtype=torch.int64, device="cuda")
    for a, b in _steps(N, D):
        got = run(a, b)
        for k in ("idx", "zq", "ze"):
            if k in big:
                assert torch.equal(got[k] if k == "idx" else _bits(got[k]), big[k][a:b] if k == "idx" else _bits(big[k][a:b])), (k, a, b)
        total += got["usage"]
        del got
    assert torch.equal(big["usage"], total) and torch.equal(total, torch.bincount(big["idx"], minlength=K)) and int(total.sum()) == N
    for a, b in X.windows(N, D):
        want = oracle_rows(a, b)
        for k, v in want.items():
            assert np.array_equal(big[k][a:b].cpu().numpy(), v), (k, a, b)


@pytest.mark.parametrize("dist", ["norm", "sqsum"])
def test_nearest_screened(ops, oracle, dist):
    """lipvq_nearest_screened_f32 / lipvq_vq_nearest_screened_f32 (the MFMA screen, then the list and scanning kernels for the rows it
    leaves) on z [N, 208], K = 64."""
    case = _case("nearest_screened")
    N, D, K = case.N, case.W, case.dims[0]
    rule = ops.DIST_SQSUM if dist == "sqsum" else ops.DIST_NORM
    z, cb = _randn_big(211, N, D), _small(212, K, D)
    prep = ops.nearest_prepare(cb)

    def run(a, b):
        usage = torch.zeros(K, dtype=torch.int64, device="cuda")
        idx, zq = ops.nearest_screened(z[a:b], cb, prep, usage=usage, dist=rule)
        return {"idx": idx, "zq": zq, "usage": usage}

    def rows(a, b):
        i, q, _ = oracle.nearest(z[a:b].cpu().numpy(), cb.cpu().numpy(), rule)
        return {"idx": i, "zq": q}
    _search_outputs_agree(N, D, K, run(0, N), run, None, rows)


@pytest.mark.parametrize("variant", ["llfq", "vq"])
def test_tokenize(ops, oracle, variant):
    """The fused encode + quantize launches at N = 10.3 M (the path the metric batch takes): lipvq_tokenize_f32 against the canonical
    oracle's encoder and search on the windows, lipvq_vq_tokenize_f32 against the unfused lipvq_mlp3_f32 + lipvq_nearest_f32 there
    (tests/test_gpu_fused.py's checks: bits); idx, z_q, z_e chunk-equal, usage the int64 sum of the chunks' usage."""
    from oracle import lipvq_oracle as O
    from lipvq_vae_amd.tokenizer import LLFQVAE_V4, VQVAE
    case = _case("tokenize")
    N, D = case.N, case.W
    A, J0, J1, K = case.dims
    assert ops.tokenize_supported(A, J0, J1, D, K)
    x = torch.rand((N, A), device="cuda", generator=torch.Generator(device="cuda").manual_seed(221)) * 2.0 - 1.0
    if variant == "llfq":
        p = O.make_params(222, A, D, K, oracle=oracle)
        model = LLFQVAE_V4(A, D, num_codes=K).cuda()
        model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()})
        packed, _, Wn = model._packed_encoder()
        w0, b0, w1, b1, _, b2, _ = (t.detach() for t in model._enc_params())
        raw = (w0, b0, w1, b1, Wn, b2)
        cb = model.quantizer.codebook.detach()
    else:
        torch.manual_seed(223)
        model = VQVAE(A, D, num_embeddings=K).cuda()
        with torch.no_grad():
            model.embedding.weight.uniform_(0.0, 0.5)
        model.invalidate_caches()
        packed, cb = model._packed_encoder(), model.embedding.weight.detach()
    prep = ops.nearest_prepare(cb)

    def run(a, b):
        usage = torch.zeros(K, dtype=torch.int64, device="cuda")
        if variant == "llfq":
            idx, zq, ze, _ = ops.tokenize(x[a:b], packed, raw, cb, prep, usage=usage, want_ze=True)
        else:
            idx, zq, ze, _ = ops.vq_tokenize(x[a:b], packed, cb, prep, usage=usage)
        return {"idx": idx, "zq": zq, "ze": ze, "usage": usage}

    def rows(a, b):
        if variant == "llfq":
            ze = oracle.llfq_encode(p, x[a:b].cpu().numpy())
            i, q, _ = oracle.nearest(ze, p["quantizer.codebook"])
            return {"ze": ze, "idx": i, "zq": q}
        ze = ops.mlp3(x[a:b].contiguous(), packed, model._ENC_ACTS)
        i, q, _ = ops.nearest(ze, cb, ops.DIST_SQSUM)
        return {"ze": ze.cpu().numpy(), "idx": i.cpu().numpy(), "zq": q.cpu().numpy()}
    _search_outputs_agree(N, D, K, run(0, N), run, None, rows)


# ---------------------------------------------------------------------------------------------------
# C. the default branch's unbatched attention (lipvq_attention_f32 / _bwd_f32): keep bytes [H][S][S] past 2^32
# ---------------------------------------------------------------------------------------------------

def test_attention_unbatched(ops):
    """H = 8, D = 64, S = 23 200: no chunking is possible (every query meets every key), so out and gqkv are held against a float64
    restatement of tests/test_gpu_default.py's _attention_ref and its hand-derived backward, one head at a time on the device, over
    ALL rows and on the 64-query windows (the first queries, both sides of the query whose keep bytes cross 2^32, the last) at that
    file's budgets, 1e-5 and 1e-4 of the largest reference value.  The dropout= forms: the bits of the keep-byte forms."""
    case = _case("attention_unbatched")
    (S, D, H), p = case.dims, case.p
    dh, kp = D // H, 1.0 - case.p
    site, snap = ops.DROPOUT_SITE_DEFAULT + 4, _snap()
    qkv, gout = _small(231, S, 3 * D), _small(232, S, D)
    keep = ops.dropout_keep(snap, site, H * S, S, p).view(H, S, S)
    assert keep.numel() > X.B32
    out, lse = ops.attention(qkv, H, keep, kp)
    gq = ops.attention_bwd(qkv, out, gout, lse, H, keep, kp)
    out2, lse2 = ops.attention(qkv, H, dropout=(snap, site, p))
    gq2 = ops.attention_bwd(qkv, out2, gout, lse2, H, dropout=(snap, site, p))
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(lse2), _bits(lse)) and torch.equal(_bits(gq2), _bits(gq))
    ref_out, ref_gq = torch.empty((S, D), dtype=torch.float64, device="cuda"), torch.empty((S, 3 * D), dtype=torch.float64, device="cuda")
    qd, god = qkv.double(), gout.double()
    scale = 1.0 / math.sqrt(dh)
    for h in range(H):
        sl = slice(h * dh, (h + 1) * dh)
        q, k, v, go = qd[:, sl], qd[:, D + h * dh:D + (h + 1) * dh], qd[:, 2 * D + h * dh:2 * D + (h + 1) * dh], god[:, sl]
        P = torch.softmax((q @ k.t()) * scale, dim=-1)
        m = keep[h].double().div_(kp)
        dP = (go @ v.t()).mul_(m)                                # d loss / d P
        ref_out[:, sl] = (P * m) @ v
        ref_gq[:, 2 * D + h * dh:2 * D + (h + 1) * dh] = (P * m).t() @ go
        del m
        dS = dP.sub_((dP * P).sum(-1, keepdim=True)).mul_(P)
        del P
        ref_gq[:, sl] = (dS @ k) * scale
        ref_gq[:, D + h * dh:D + (h + 1) * dh] = (dS.t() @ q) * scale
        del dS, dP
    def rel(a, b):
        return float((a.double() - b).abs().max() / b.abs().max())
    qb = X.B32 // S - (H - 1) * S                                # the query of head H - 1 whose keep bytes hold byte 2^32
    assert 64 <= qb < S - 165
    e_out, e_gq = rel(out, ref_out), rel(gq, ref_gq)
    print(f"unbatched attention S={S}: out {e_out:.3e}, gqkv {e_gq:.3e} over all rows")
    assert e_out <= 1e-5 and e_gq <= 1e-4
    for a, b in ((0, 64), (qb - 64, qb + 64), (S - 101, S)):
        e_out, e_gq = rel(out[a:b], ref_out[a:b]), rel(gq[a:b], ref_gq[a:b])
        print(f"  queries / keys {a} .. {b}: out {e_out:.3e}, gqkv {e_gq:.3e}")
        assert e_out <= 1e-5 and e_gq <= 1e-4


def test_bin_minmax(ops):
    """Standard normals (|v| < 40 in fp32's normal sampler) with each column's extrema planted in the last window."""
    case = _case("bin_minmax")
    N, A = case.N, case.W
    x = _randn_big(81, N, A)
    want_min, want_max = np.empty(A, np.float32), np.empty(A, np.float32)
    for c in range(A):
        x[N - 50 - c, c] = -100.0 - c
        x[N - 30 - c, c] = 100.0 + c
        want_min[c], want_max[c] = -100.0 - c, 100.0 + c
    rmin, rmax = torch.full((A,), float("inf"), device="cuda"), torch.full((A,), float("-inf"), device="cuda")
    ops.bin_minmax(x, rmin, rmax)
    assert np.array_equal(rmin.cpu().numpy(), want_min) and np.array_equal(rmax.cpu().numpy(), want_max)
    # and the statistics of the rows before the last window, against torch's own chunked reduction
    lo, hi = torch.full((A,), float("inf"), device="cuda"), torch.full((A,), float("-inf"), device="cuda")
    for a, b in _steps(N - 101, A):
        lo, hi = torch.minimum(lo, x[a:b].amin(0)), torch.maximum(hi, x[a:b].amax(0))
    rmin.fill_(float("inf"))
    rmax.fill_(float("-inf"))
    for c in range(A):
        x[N - 50 - c, c] = 0.0
        x[N - 30 - c, c] = 0.0
    ops.bin_minmax(x, rmin, rmax)
    tail_lo, tail_hi = x[N - 101:].amin(0), x[N - 101:].amax(0)
    assert torch.equal(rmin, torch.minimum(lo, tail_lo)) and torch.equal(rmax, torch.maximum(hi, tail_hi))
