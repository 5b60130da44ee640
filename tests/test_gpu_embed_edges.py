"""GPU: the embedding stage (csrc/lipvq_embed.hip: linear_kernel / linear_big_kernel, embed_rows_kernel and its two backward
kernels) on inputs that are NOT unit-normal, at the dispatch and tile edges, over every path of the forward's row stepping, and
with its outputs fenced in.

tests/test_gpu_embed.py draws every row from randn and compares the forward with an oracle that shares its formula; its widths
stop at E = 512 in the backward and its large batches are multiples of T.  Here
  1. / 2.  the LayerNorm classes of tests/xf_edge_inputs.py (rows of 1000 + noise, 1e-20, 1e15, constants, one-hot, cancelling
     sums) go through embed_rows and its backward, dense and indexed, at the NJ dispatch edges of both, and are held to that
     file's yardstick: error <= max(tolerance, 4 x the deviation of stock fp32 torch on the CPU from float64), per class;
  3.  the forward's incremental (b, t) stepping runs with chunk = 1, 2, 3, 8, 16, T below, at and above 16, ragged last items
     and a second grid-stride iteration, into one stream of the three-stream layout inside a sentinel-filled buffer;
  4.  the backward's NJ = 3 and 4 instances, a ragged N, T = 1000 and 1024 and absent outputs run on both routes, against
     float64 autograd on the device;
  5.  the activation / pre epilogue of the large-N Linear tilings and the 64-wide K chunk edges of the small one, bit for bit
     against the oracle, fenced.
Every yardstick figure is printed (class, shape, error, the reference's own, their ratio, the bound) before it is asserted.
No input is non-finite; the only non-finite outputs are the rows of a bad index, which are NaN by definition.

What these tests found when they were written (the library before them = "before"; e/b = largest error / bound of any case):
1.  before: 'constant' (rows of 3.0) y 6.1e-5 ... 9.8e-5 > 1e-5 at E = 252 and 1020, N = 5 and 2053, dense with and without pos
    and indexed, and 'plus100' y 1.079e-5 > 1.016e-5 at E = 132, N = 5 with pos -- the figures the oracle gives on the CPU, to the
    digit (fl(1/E) is inexact, the mean of a constant row one ulp off, rstd = 316 multiplies the residue).  The row is centred
    twice now, in the kernel and in the oracle: y e/b 0.29 ('plus1000', N = 5, E = 252, pos), rstd 0.26, constant rows error 0.
2.  before: passed, e/b 0.56 (g_lnw, N = 5, E = 1020, indexed), 0.31 (g_src / g_pos, 'plus1000', N = 2053, E = 4), 0.18 on the
    workspace route (g_lnw, E = 772).  The backward kernels are unchanged; stats now hold the corrected mean: g_lnw 0.19
    (N = 5, E = 260, pos), g_src / g_pos 0.31, workspace route 0.08.
3.  before: passed (bit-equal to the oracle of its own formula on all eight (N, T)); now the same.  Nothing to fix in the stepping.
4.  before and now: passed; every figure <= 6.0e-6 of the gradient's scale against the 2e-4 bound (e/b 0.03: g_src, collapsed codes,
    E = 772); absent outputs leave the others' bits (dense g_src, the workspace route's table gradient) or stay within 1.5e-6 of
    their scale (atomics, other order).
5.  before and now: passed, bit for bit.
"""
import numpy as np
import pytest
import torch

import embed_ref as R
import xf_edge_inputs as X
from fenced import PAD, SENTINEL, _Fenced

pytestmark = pytest.mark.gpu

EPS = X.LN_EPS


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _capi():
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    return _capi.lib, _capi.check, lipvq_vae_amd.ops._stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _cuda(t):
    return None if t is None else t.cuda()


def _np(t):
    return None if t is None else t.numpy()


def _assert_all(results):
    for what, err, bound in results:
        assert err <= bound, (what, err, bound)


# ---------------------------------------------------------------------------------------------------
# 1. / 2.  edge values, forward and backward
# ---------------------------------------------------------------------------------------------------

def _edge_forward(ops, case, N, E):
    """embed_rows on one edge case (B = ceil(N / T) batches of T contiguous rows): (y [N, E], stats [N, 2], device inputs)."""
    T = case["T"]
    B = -(-N // T)
    dev = {k: _cuda(case[k]) for k in ("src", "idx", "pos", "w", "bias")}
    out = torch.zeros(B * T, E, device="cuda")
    stats = ops.embed_rows(dev["src"], dev["idx"], dev["pos"], dev["w"], dev["bias"], EPS, out, N, T, T * E, E, 0, want_stats=True)
    return out[:N], stats, dev


def _edge_backward(ops, case, stats, dev, N, E):
    T = case["T"]
    B = -(-N // T)
    gout = torch.zeros(B * T, E, device="cuda")
    gout[:N] = case["gout"].cuda()
    g = {"g_src": torch.zeros_like(dev["src"]), "g_pos": None if dev["pos"] is None else torch.zeros_like(dev["pos"]),
         "g_lnw": torch.zeros(E, device="cuda"), "g_lnb": torch.zeros(E, device="cuda")}
    ops.embed_rows_bwd(gout, dev["src"], dev["idx"], dev["pos"], stats, dev["w"], g["g_src"], g["g_pos"], g["g_lnw"], g["g_lnb"],
                       N, T, T * E, E, 0)
    return {k: v.cpu() for k, v in g.items() if v is not None}


def _forward_results(tag, case, classes, y, stats):
    got = {"y": y.cpu(), "rstd": stats[:, 1].cpu()}
    return [X.report(f"{tag} {cls} {k}", R.edge_err(case, k, got[k], cls), R.edge_dev(case, k, cls), X.FWD_TOL)
            for cls in classes for k in R.ROW_OUT]


def _backward_results(tag, case, classes, got):
    res = [X.report(f"{tag} {cls} {k}", R.edge_err(case, k, got[k], cls), R.edge_dev(case, k, cls), X.BWD_TOL)
           for cls in classes for k in R.ROW_SRC if k in got]
    return res + [X.report(f"{tag} {'+'.join(classes)} {k}", R.edge_err(case, k, got[k]), R.edge_dev(case, k), X.BWD_TOL) for k in R.COLUMNS]


@pytest.mark.parametrize("N", R.EDGE_N)
@pytest.mark.parametrize("E", R.EDGE_E)
def test_edge_values_forward(ops, oracle, E, N):
    """Bit-equal to the oracle, and y and rstd inside the float64 yardstick per class (a constant row: inside FWD_TOL)."""
    results, differs = [], []
    for route, with_pos in R.EDGE_ROUTES:
        for classes in X.layernorm_groups(N):
            case = R.edge_case(classes, N, E, route, with_pos)
            y, stats, _ = _edge_forward(ops, case, N, E)
            tag = f"embed fwd N={N} E={E} {route} pos={with_pos}"
            results += _forward_results(tag, case, classes, y, stats)
            ref = np.empty((1, N, E), np.float32)
            st_ref = oracle.embed_rows(_np(case["src"]), _np(case["idx"]), _np(case["pos"]), _np(case["w"]), _np(case["bias"]), EPS, ref,
                                       N, N * E, E, 0, want_stats=True)
            if not (np.array_equal(y.cpu().numpy(), ref[0]) and np.array_equal(stats.cpu().numpy(), st_ref)):
                differs.append(tag + " " + "+".join(classes))
    assert not differs, ("the kernel and the oracle differ in some bit", differs)
    _assert_all(results)


@pytest.mark.parametrize("N", R.EDGE_N)
@pytest.mark.parametrize("E", R.EDGE_E)
def test_edge_values_backward(ops, E, N):
    """The atomic route (N < 32768): g_src and g_pos per class, g_lnw and g_lnb over the tensor."""
    results = []
    for route, with_pos in R.EDGE_ROUTES:
        for classes in X.layernorm_groups(N):
            case = R.edge_case(classes, N, E, route, with_pos)
            _, stats, dev = _edge_forward(ops, case, N, E)
            got = _edge_backward(ops, case, stats, dev, N, E)
            assert ("g_pos" in got) == with_pos
            results += _backward_results(f"embed bwd N={N} E={E} {route} pos={with_pos}", case, classes, got)
    _assert_all(results)


@pytest.mark.parametrize("E", R.WS_EDGE_E)
def test_edge_values_backward_workspace_route(ops, E):
    """Dense rows of a large ragged batch (N = 32773 = 7 * 4681 + 6, pos = None), all ten classes in one tensor."""
    N, T = R.WS_EDGE_N, R.WS_EDGE_T
    (classes,) = X.layernorm_groups(N)
    case = R.edge_case(classes, N, E, "dense", False, T)
    y, stats, dev = _edge_forward(ops, case, N, E)
    tag = f"embed workspace N={N} T={T} E={E} dense"
    results = _forward_results(tag, case, classes, y, stats)
    results += _backward_results(tag, case, classes, _edge_backward(ops, case, stats, dev, N, E))
    _assert_all(results)


# ---------------------------------------------------------------------------------------------------
# 3.  row stepping of the forward
# ---------------------------------------------------------------------------------------------------

def _same_words(got, want, nan_rows, what):
    """int32 words equal everywhere; on the rows listed (flat word ranges) both sides are NaN and the sentinel is gone."""
    got, want = got.copy(), want.copy()
    for lo, hi in nan_rows:
        assert np.isnan(got[lo:hi].view(np.float32)).all() and np.isnan(want[lo:hi].view(np.float32)).all(), (what, lo)
        assert (got[lo:hi] != SENTINEL).all(), (what, lo)
        got[lo:hi] = want[lo:hi]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8])


@pytest.mark.parametrize("N,T", R.STEP_CASES)
def test_row_stepping(oracle, N, T):
    """Indexed rows into the slots 2t + 1 and dense rows into the slots 2t of a [B][3T][E] buffer of sentinels: out and stats
    equal the oracle's bit for bit (the first and the last indexed row carry a bad index: NaN rows, compared by position),
    and the third stream's slots, a ragged last batch's unused slots and the guard bands keep the sentinel."""
    lib, check, stream = _capi()
    E, K = R.STEP_E, R.STEP_K
    B = -(-N // T)
    g = torch.Generator().manual_seed(N + T)
    table, dense, pos = torch.randn(K, E, generator=g), torch.randn(N, E, generator=g), 0.1 * torch.randn(T, E, generator=g)
    w, bias = 1 + 0.1 * torch.randn(E, generator=g), 0.1 * torch.randn(E, generator=g)
    idx = torch.randint(0, K, (N,), generator=g)
    idx[0], idx[-1] = K + 2, -1
    ct, cd, cp, cw, cb, ci = (t.cuda() for t in (table, dense, pos, w, bias, idx))
    out, st_i, st_d = _Fenced("out", B, 3 * T, E), _Fenced("indexed stats", N, 2), _Fenced("dense stats", N, 2)
    bs, ts = 3 * T * E, 2 * E
    check(lib.lipvq_embed_rows_f32(_ptr(ct), _ptr(ci), _ptr(cp), _ptr(cw), _ptr(cb), EPS, out.ptr(), st_i.ptr(), N, T, E, K, bs, ts, E, stream()),
          "lipvq_embed_rows_f32")
    check(lib.lipvq_embed_rows_f32(_ptr(cd), None, _ptr(cp), _ptr(cw), _ptr(cb), EPS, out.ptr(), st_d.ptr(), N, T, E, N, bs, ts, 0, stream()),
          "lipvq_embed_rows_f32")
    torch.cuda.synchronize()
    ref = np.full((B, 3 * T, E), SENTINEL, np.int32).view(np.float32)
    ri = oracle.embed_rows(table.numpy(), idx.numpy(), pos.numpy(), w.numpy(), bias.numpy(), EPS, ref, T, bs, ts, E, N=N, want_stats=True)
    rd = oracle.embed_rows(dense.numpy(), None, pos.numpy(), w.numpy(), bias.numpy(), EPS, ref, T, bs, ts, 0, N=N, want_stats=True)
    want = np.full(out.buf.numel(), SENTINEL, np.int32)                # the guard bands too
    want[PAD:PAD + ref.size] = ref.view(np.int32).ravel()
    slot = lambda n: PAD + (n // T) * bs + (n % T) * ts + E            # noqa: E731  (first word of indexed row n)
    _same_words(out.buf.cpu().numpy(), want, [(slot(0), slot(0) + E), (slot(N - 1), slot(N - 1) + E)], "out")
    _same_words(st_i.check().cpu().numpy().view(np.int32).ravel(), ri.view(np.int32).ravel(), [(0, 2), (2 * N - 2, 2 * N)], "indexed stats")
    _same_words(st_d.check().cpu().numpy().view(np.int32).ravel(), rd.view(np.int32).ravel(), [], "dense stats")


# ---------------------------------------------------------------------------------------------------
# 4.  wide rows and shape edges of the backward, both routes
# ---------------------------------------------------------------------------------------------------

TAIL = 4096                                                          # bytes of 0xA5 behind the workspace the library asks for


def _bwd(route, t, want=("g_src", "g_pos", "g_lnw", "g_lnb"), pos=True):
    """One backward call through the C ABI: route 'atomic' (lipvq_embed_rows_bwd_f32) or 'ws' (lipvq_embed_rows_bwd_ws_f32, on
    exactly the workspace bytes the library asks for, followed by TAIL bytes that must survive).  `want`: the outputs asked for."""
    lib, check, stream = _capi()
    N, T, E, Rws = t["N"], t["T"], t["E"], t["src"].shape[0]
    p = t["pos"] if pos else None
    st = t["stats"] if pos else t["stats_nopos"]
    g = {"g_src": torch.zeros_like(t["src"]), "g_pos": torch.zeros_like(t["pos"]) if pos else None,
         "g_lnw": torch.zeros(E, device="cuda"), "g_lnb": torch.zeros(E, device="cuda")}
    g = {k: (v if k in want else None) for k, v in g.items()}
    head = (_ptr(t["gout"]), _ptr(t["src"]), _ptr(t["idx"]), _ptr(p), _ptr(st), _ptr(t["w"]), _ptr(g["g_src"]), _ptr(g["g_pos"]),
            _ptr(g["g_lnw"]), _ptr(g["g_lnb"]))
    tail = (N, T, E, Rws) + t["layout"] + (stream(),)
    if route == "atomic":
        check(lib.lipvq_embed_rows_bwd_f32(*head, *tail), "lipvq_embed_rows_bwd_f32")
    else:
        ws = None
        if t["idx"] is not None:
            nbytes = lib.lipvq_embed_rows_bwd_workspace_bytes(N, T, E, Rws)
            assert lib.lipvq_embed_rows_bwd_ws_supported(N, T, E, Rws) and nbytes >= N * E * 4 + N * 8
            ws = torch.full((nbytes + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
        check(lib.lipvq_embed_rows_bwd_ws_f32(*head, _ptr(ws), *tail), "lipvq_embed_rows_bwd_ws_f32")
        if ws is not None:
            assert bool((ws[-TAIL:] == 0xA5).all()), "a byte behind the workspace was written"
    return g


def _wide_setup(ops, N, T, E, K, kind, indexed, seed):
    """randn inputs on the device, the middle stream of the [B][3T][E] layout, the forward's stats with and without pos, and the
    float64 autograd results of both."""
    B = -(-N // T)
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows = K if indexed else N
    t = {"N": N, "T": T, "E": E, "src": torch.randn(rows, E, device="cuda", generator=g),
         "pos": 0.1 * torch.randn(T, E, device="cuda", generator=g), "w": 1 + 0.1 * torch.randn(E, device="cuda", generator=g),
         "bias": 0.1 * torch.randn(E, device="cuda", generator=g), "idx": None, "layout": (3 * T * E, 2 * E, E)}
    if indexed:
        t["idx"] = torch.randint(0, K, (N,), device="cuda", generator=g)
        if kind == "collapsed":
            t["idx"][torch.rand(N, device="cuda", generator=g) < 0.9] = 5
    t["gout"] = torch.randn(B, 3 * T, E, device="cuda", generator=g)
    out = torch.zeros(B, 3 * T, E, device="cuda")
    t["stats"] = ops.embed_rows(t["src"], t["idx"], t["pos"], t["w"], t["bias"], EPS, out, N, T, *t["layout"], want_stats=True)
    t["stats_nopos"] = ops.embed_rows(t["src"], t["idx"], None, t["w"], t["bias"], EPS, out, N, T, *t["layout"], want_stats=True)
    sel = t["gout"][:, 1:2 * T:2].reshape(B * T, E)[:N]
    t["ref"] = R.embed_run(t["src"], t["idx"], t["pos"], T, t["w"], t["bias"], sel, torch.float64)
    t["ref_nopos"] = R.embed_run(t["src"], t["idx"], None, T, t["w"], t["bias"], sel, torch.float64)
    return t


NAMES = ("g_src", "g_pos", "g_lnw", "g_lnb")


def _wide_close(tag, got, ref, results):
    """|got - ref| <= WIDE_TOL x the gradient's scale, for every output that is there; figures first."""
    for k in NAMES:
        if got.get(k) is not None:
            scale = float(ref[k].abs().max()) + 1e-30
            err = float((got[k].double() - ref[k].double()).abs().max()) / scale
            print(f"{tag} {k}: error {err:.3e} of the gradient's scale, bound {R.WIDE_TOL:.1e}")
            results.append((f"{tag} {k}", err, R.WIDE_TOL))


def _absent_outputs(route, t, full, exact_src, tag, results):
    """Each of g_src / g_pos / (g_lnw, g_lnb) absent in turn, and pos absent altogether: what is left matches the full call."""
    for absent in (("g_src",), ("g_pos",), ("g_lnw", "g_lnb")):
        part = _bwd(route, t, tuple(k for k in NAMES if k not in absent))
        assert all(part[k] is None for k in absent)
        if "g_src" not in absent and exact_src:
            assert torch.equal(part["g_src"], full["g_src"]), (tag, "g_src without", absent)
        _wide_close(f"{tag} without {'+'.join(absent)} vs all outputs", part, full, results)
    nopos = _bwd(route, t, ("g_src", "g_lnw", "g_lnb"), pos=False)
    _wide_close(f"{tag} pos=None", nopos, t["ref_nopos"], results)
    return nopos


@pytest.mark.parametrize("indexed", [True, False], ids=["indexed", "dense"])
@pytest.mark.parametrize("E", R.WIDE_E)
def test_wide_rows_backward_atomic_route(ops, E, indexed):
    B, T = R.WIDE_BT
    t = _wide_setup(ops, B * T, T, E, 7, "uniform", indexed, 100 + E)
    tag = f"embed bwd atomic E={E} {'indexed' if indexed else 'dense'}"
    results = []
    full = _bwd("atomic", t)
    _wide_close(tag, full, t["ref"], results)
    _absent_outputs("atomic", t, full, not indexed, tag, results)       # dense: one writer per row; indexed: atomics, other order
    _assert_all(results)


@pytest.mark.parametrize("E,T,K,kind,indexed", R.WS_CASES)
def test_wide_rows_backward_workspace_route(ops, E, T, K, kind, indexed):
    N = R.WS_N
    t = _wide_setup(ops, N, T, E, K, kind, indexed, 200 + E + T)
    tag = f"embed bwd N={N} T={T} E={E} {kind} {'indexed' if indexed else 'dense'}"
    results = []
    full, again, atomic = _bwd("ws", t), _bwd("ws", t), _bwd("atomic", t)
    assert torch.equal(full["g_src"], again["g_src"]), "the source gradient does not repeat bit for bit"
    _wide_close(tag + " workspace", full, t["ref"], results)
    _wide_close(tag + " atomic", atomic, t["ref"], results)
    _wide_close(tag + " workspace vs atomic", full, atomic, results)
    via_ops = {k: torch.zeros_like(v) for k, v in full.items()}
    ops.embed_rows_bwd(t["gout"], t["src"], t["idx"], t["pos"], t["stats"], t["w"], *(via_ops[k] for k in NAMES), N, T, *t["layout"])
    assert torch.equal(via_ops["g_src"], full["g_src"]), "ops.embed_rows_bwd did not take the workspace route"
    _absent_outputs("ws", t, full, True, tag + " workspace", results)
    _assert_all(results)


def test_workspace_bytes_are_zero_exactly_where_the_route_is_unsupported():
    lib, _, _ = _capi()
    supported = {(32768, 10, 512, 1024): True, (32767, 10, 512, 1024): False, (R.WS_N, 1024, 64, 300): True,
                 (R.WS_N, 1025, 64, 300): False, (R.WS_N, 0, 64, 300): False, (40000, 10, 1028, 300): False, (40000, 10, 6, 300): False,
                 (40000, 10, 4, 2): True, (40000, 10, 4, 1): False, (40000, 10, 512, 16384): True, (40000, 10, 512, 16385): False, (R.WS_N, 10, 772, 300): True,
                 (R.WS_N, 1, 1024, 5): True, (1 << 22, 10, 1024, 16384): None, (1 << 31, 10, 1024, 1024): None}
    for (N, T, E, K), want in supported.items():
        s, nbytes = lib.lipvq_embed_rows_bwd_ws_supported(N, T, E, K), lib.lipvq_embed_rows_bwd_workspace_bytes(N, T, E, K)
        assert (nbytes == 0) == (s == 0), (N, T, E, K, s, nbytes)
        if want is not None:
            assert bool(s) == want, (N, T, E, K)
        if s:
            assert nbytes >= N * E * 4 + N * 8, (N, T, E, K, nbytes)


# ---------------------------------------------------------------------------------------------------
# 5.  Linear: K chunk edges of the small kernel, activation and pre epilogue of the large-N tilings
# ---------------------------------------------------------------------------------------------------

def _linear_inputs(N, Kin, E):
    rng = np.random.default_rng(N + Kin + E)
    return (rng.standard_normal((N, Kin)).astype(np.float32), (rng.standard_normal((E, Kin)) / np.sqrt(Kin)).astype(np.float32),
            rng.standard_normal(E).astype(np.float32))


def _linear_fenced(x, W, b, act, save_pre):
    lib, check, stream = _capi()
    N, Kin = x.shape
    E = W.shape[0]
    y, pre = _Fenced("y", N, E), (_Fenced("pre", N, E) if save_pre else None)
    check(lib.lipvq_linear_act_f32(_ptr(x), _ptr(W), _ptr(b), y.ptr(), None if pre is None else pre.ptr(), N, Kin, E, int(act), stream()),
          "lipvq_linear_act_f32")
    torch.cuda.synchronize()
    return y.check().cpu().numpy(), (None if pre is None else pre.check().cpu().numpy())


@pytest.mark.parametrize("Kin", R.LINEAR_SMALL[2])
def test_linear_k_chunk_edges(ops, oracle, Kin):
    N, E, _ = R.LINEAR_SMALL
    x, W, b = _linear_inputs(N, Kin, E)
    cx, cW, cb = (torch.from_numpy(a).cuda() for a in (x, W, b))
    for bias, cbias in ((b, cb), (None, None)):
        y, _ = _linear_fenced(cx, cW, cbias, ops.ACT_NONE, False)
        assert np.array_equal(y, oracle.linear(x, W, bias)), (Kin, bias is not None)
        for act in (ops.ACT_GELU, ops.ACT_RELU):
            y, pre = _linear_fenced(cx, cW, cbias, act, True)
            y_ref, pre_ref = oracle.linear_act(x, W, bias, act, save_pre=True)
            assert np.array_equal(y, y_ref) and np.array_equal(pre, pre_ref), (Kin, bias is not None, act)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("N,Kin,E", R.LINEAR_BIG)
def test_linear_big_tilings_activation_and_pre(ops, oracle, N, Kin, E, with_bias):
    tr, tc = (256, 64) if E <= 64 else (128, 128)
    assert -(-N // tr) * -(-E // tc) >= 512 and Kin % 4 == 0          # the large-N kernel's condition (lipvq_linear_act_f32)
    x, W, b = _linear_inputs(N, Kin, E)
    bias = b if with_bias else None
    cx, cW, cb = torch.from_numpy(x).cuda(), torch.from_numpy(W).cuda(), (torch.from_numpy(b).cuda() if with_bias else None)
    for act in (ops.ACT_GELU, ops.ACT_RELU):
        y, pre = _linear_fenced(cx, cW, cb, act, True)
        y_ref, pre_ref = oracle.linear_act(x, W, bias, act, save_pre=True)
        assert np.array_equal(pre, pre_ref), (act, "pre")
        assert np.array_equal(y, y_ref), (act, "y")
