"""GPU: the backward kernels (csrc/lipvq_bwd.hip, the backward instances of csrc/lipvq_mlp.hip, act_bwd, scaled_diff, the spectral
norm) through the C ABI on outputs of the test's own: what they write, what they read, and that every row is added exactly once.

tests/test_gpu_backward.py holds the VALUES of these kernels to float64 budgets, through the ops.* wrappers (outputs from
torch.empty, whose allocations are rounded up to 512 bytes).  Here every output sits inside a sentinel-filled buffer
(tests/fenced.py): no word outside may change, none inside may keep the sentinel; operands sit between NaN words; weight
gradients of small-integer operands must equal an int64 product bit for bit at every row count where the chunking or the reduce
loop changes; one planted NaN / Inf must reach exactly the elements the operation's definition says (tests/backward_edge_cases.py
has the maps and every parameter list, tests/test_backward_edge_cases_host.py checks them without a GPU).

Every comparison is on bits (torch.equal on the int32 view, or NaN masks plus bits elsewhere) except the spectral norm's values,
which are held to the per-element budgets derived in backward_edge_cases.spectral_ref_and_budget.

Output alignment, read from the kernels before launching anything 4 bytes off: the three wgrad kernels store their slab and
wgrad_reduce_kernel its sums one element at a time; mlp3_wg_kernel and mlp3_lds_kernel test pointer and row stride (al16) before
every 16-byte store and fall back to element stores, mlp3_kernel stores elements; the elementwise kernels store elements.  No
backward kernel assumes an aligned output, so the offset_out cases below are legal calls.
"""
import functools
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import backward_edge_cases as B  # noqa: E402
import backward_ref as R  # noqa: E402
from fenced import SENTINEL, _Fenced  # noqa: E402
from test_gpu_backward import close  # noqa: E402  (prints the worst err/allowed before asserting)

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -2                        # include/lipvq.h


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _capi():
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    return _capi.lib, _capi.check, lipvq_vae_amd.ops._stream


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def outside_untouched(f):
    """The guard words of a _Fenced (its inside may be anything)."""
    o = f.words.storage_offset()
    return bool((f.buf[:o] == SENTINEL).all()) and bool((f.buf[o + f.n:] == SENTINEL).all())


def between_nans(t, offset_words=0):
    """A device copy of the fp32 tensor t in the middle of a buffer of NaN sentinel words (4 KiB on either side)."""
    f = _Fenced("operand", *t.shape, offset_words=offset_words)
    f.t.copy_(t)
    return f


# ---------------------------------------------------------------------------------------------------------------------------
# wgrad
# ---------------------------------------------------------------------------------------------------------------------------
def _wgrad(G, H, hidx, act, N, J, Kd, want_gb=True, offset=0):
    """lipvq_wgrad_f32 on fenced gW, gb and a fenced workspace of exactly the bytes the library asks for."""
    lib, check, stream = _capi()
    gW, gb = _Fenced("gW", J, Kd, offset_words=offset), (_Fenced("gb", J, offset_words=offset) if want_gb else None)
    nbytes = lib.lipvq_wgrad_workspace_bytes(N, J, Kd)
    assert nbytes == B.wgrad_chunks(N) * (J * Kd + J) * 4
    ws = _Fenced("workspace", nbytes // 4, offset_words=offset)
    check(lib.lipvq_wgrad_f32(G.data_ptr(), H.data_ptr(), None if hidx is None else hidx.data_ptr(), int(act), gW.ptr(),
                              None if gb is None else gb.ptr(), ws.ptr(), N, J, Kd, stream()), "lipvq_wgrad_f32")
    torch.cuda.synchronize()
    assert outside_untouched(ws), "a word outside the workspace was written"       # (its inside: the header promises nothing)
    return gW.check(), (None if gb is None else gb.check())


@pytest.mark.parametrize("N,J,Kd,mode", B.WGRAD_EXTENT_CASES)
def test_wgrad_write_extent(ops, N, J, Kd, mode):
    """gW, gb and the workspace between guard words, per kernel family and tile raggedness, one chunk (the kernel's tile-shaped slab
    is the result) and three chunks plus the reduce; the values are those of the wrapper's plain allocations, bit for bit."""
    G, H = (t.cuda() for t in B.wgrad_case(N, J, Kd, N * 1009 + J * 31 + Kd))
    act = B.ACT_GELU if Kd % 2 == 0 else B.ACT_NONE
    want_W, want_b = ops.wgrad(G, H, h_act=act)
    if mode == "misaligned":
        gf, hf = between_nans(G, 1), between_nans(H, 1)
        G, H = gf.t, hf.t
        assert G.data_ptr() % 16 == 4 and H.data_ptr() % 16 == 4
    gW, gb = _wgrad(G, H, None, act, N, J, Kd, want_gb=mode != "nobias", offset=1 if mode == "offset_out" else 0)
    assert same_bits(gW, want_W)
    assert gb is None if mode == "nobias" else same_bits(gb, want_b)
    assert torch.isfinite(gW).all()


@pytest.mark.parametrize("N,J,Kd,act,gather", B.EXACT_SUM_CASES)
def test_wgrad_exact_sums(N, J, Kd, act, gather):
    """Small-integer operands: every partial sum in any order is an exact fp32 integer, so gW and gb must equal the int64 product
    bit for bit -- a row counted twice or not at all in any corner of the chunking or of the reduce loop changes gW[0][0] = gb[0] = N
    (and nearly every other element).  A second call returns the same bits."""
    c = B.integer_wgrad_case(N, J, Kd, 1 + N % 1000, gather)
    G, H = c["G"].cuda(), c["H"].cuda()
    hidx = None if c["hidx"] is None else c["hidx"].cuda()
    gW, gb = _wgrad(G, H, hidx, act, N, J, Kd)
    want_W, want_b = c["gW"][act].float().cuda(), c["gb"].float().cuda()
    bad = (gW != want_W).nonzero()
    assert same_bits(gW, want_W), f"{bad.shape[0]} elements of gW differ, first {bad[0].tolist()}: {float(gW[tuple(bad[0])])} != {float(want_W[tuple(bad[0])])}"
    assert same_bits(gb, want_b), f"gb[0] = {float(gb[0])}, N = {N}"
    assert float(gb[0]) == N and float(gW[0, 0]) == N
    gW2, gb2 = _wgrad(G, H, hidx, act, N, J, Kd)
    assert same_bits(gW2, gW) and same_bits(gb2, gb)


@pytest.mark.parametrize("J,Kd", B.POISON_JK)
@pytest.mark.parametrize("N", B.POISON_N)
def test_wgrad_poison_isolation(N, J, Kd):
    """One NaN in G (under a GELU on H), then one Inf in H (identity), at row 0, the last row of a chunk, the first of the next and
    the last row of the batch: the non-finite set of (gW, gb) is the map's, every other element keeps the bits of the clean run."""
    G, H = B.wgrad_case(N, J, Kd, N + J)
    G[:, 3] = 0.0                                                  # Inf * 0: NaN, not Inf, in row 3 of the Inf column
    Gd, Hd = G.cuda(), H.cuda()
    clean = {act: _wgrad(Gd, Hd, None, act, N, J, Kd) for act in (B.ACT_GELU, B.ACT_NONE)}
    for t in clean.values():
        assert torch.isfinite(t[0]).all() and torch.isfinite(t[1]).all()
    for n in B.poison_rows(N):
        j, k = (5 * n + J - 1) % J, (3 * n + Kd - 1) % Kd
        Gp = G.clone()
        Gp[n, j] = float("nan")
        cW, cb = B.wgrad_poison_map(Gp, H, n, B.ACT_GELU)
        gW, gb = _wgrad(Gp.cuda(), Hd, None, B.ACT_GELU, N, J, Kd)
        B.assert_follows_poison_map(gW, clean[B.ACT_GELU][0], cW, f"gW, NaN at G[{n}, {j}]")
        B.assert_follows_poison_map(gb, clean[B.ACT_GELU][1], cb, f"gb, NaN at G[{n}, {j}]")
        assert int(torch.isnan(gW).sum()) == Kd and int(torch.isnan(gb).sum()) == 1
        Hp = H.clone()
        Hp[n, k] = float("inf")
        cW, cb = B.wgrad_poison_map(G, Hp, n, B.ACT_NONE)
        gW, gb = _wgrad(Gd, Hp.cuda(), None, B.ACT_NONE, N, J, Kd)
        B.assert_follows_poison_map(gW, clean[B.ACT_NONE][0], cW, f"gW, Inf at H[{n}, {k}]")
        B.assert_follows_poison_map(gb, clean[B.ACT_NONE][1], cb, f"gb, Inf at H[{n}, {k}]")
        assert int((~torch.isfinite(gW)).sum()) == J and bool(torch.isnan(gW[3, k]))


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("J,Kd", [(196, 100), (66, 130), (320, 100), (7, 128), (64, 7), (512, 64)])
@pytest.mark.parametrize("N", [33, 129])
def test_wgrad_read_extent(N, J, Kd, gather):
    """G and H (and the gather's table and indices) between NaN words: the padded lanes of a ragged tile and the rows past the last
    chunk's end load from clamped addresses and are masked, so nothing outside the operands may reach an accumulator -- the result
    is finite and has the bits of the same operands in plain allocations."""
    G, H = B.wgrad_case(N, J, Kd, N + Kd)
    hidx = pad_idx = None
    if gather:                                                     # rows 0, 3, ..., 27 of a table; the unused rows are NaN
        H = H[:30].contiguous()
        H[[r for r in range(30) if r % 3]] = float("nan")
        hidx = (torch.randint(0, 10, (N,), generator=torch.Generator().manual_seed(N)) * 3).cuda()
    Gd, Hd = G.cuda(), H.cuda()
    want = _wgrad(Gd, Hd, hidx, B.ACT_GELU, N, J, Kd)
    gf, hf = between_nans(Gd), between_nans(Hd)
    if gather:                                                     # the indices between entries that point at a NaN row of the table
        pad_idx = torch.ones(N + 1024, dtype=torch.int64, device="cuda")
        pad_idx[512:512 + N] = hidx
        hidx = pad_idx[512:512 + N]
    got = _wgrad(gf.t, hf.t, hidx, B.ACT_GELU, N, J, Kd)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert outside_untouched(gf) and outside_untouched(hf)


# ---------------------------------------------------------------------------------------------------------------------------
# mlp3_bwd
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _mlp3_dev(dims):
    """The shared case of `dims` on the device, its backward pack, and the wrapper's (plain-allocation) outputs."""
    import lipvq_vae_amd
    ops = lipvq_vae_amd.ops
    case = B.mlp3_bwd_case(*dims)
    pk = ops.mlp3_pack_bwd(*(w.cuda() for w in case["W"]))
    gy, pre = case["gy"].cuda(), [None if p is None else p.cuda() for p in case["pre"]]
    g2, g1, g0, gx = ops.mlp3_bwd(gy, pre, pk, case["acts"], want_gx=True)
    torch.cuda.synchronize()
    return case, pk, gy, pre, {"g2": g2, "g1": g1, "g0": g0, "gx": gx}


def _mlp3_bwd(pk, gy, pre, dims, want_g2=True, want_gx=True, offset=0):
    """lipvq_mlp3_bwd_f32 on fenced outputs -> dict of checked tensors (None for an output not asked for)."""
    lib, check, stream = _capi()
    N, K0, J0, J1, J2, acts = dims
    f = {"g2": _Fenced("g2", N, J2, offset_words=offset) if want_g2 else None, "g1": _Fenced("g1", N, J1, offset_words=offset),
         "g0": _Fenced("g0", N, J0, offset_words=offset), "gx": _Fenced("gx", N, K0, offset_words=offset) if want_gx else None}
    ptr = {k: (None if v is None else v.ptr()) for k, v in f.items()}
    check(lib.lipvq_mlp3_bwd_f32(gy.data_ptr(), pre[0].data_ptr(), pre[1].data_ptr(), None if pre[2] is None else pre[2].data_ptr(),
                                 pk.buf.data_ptr(), ptr["g2"], ptr["g1"], ptr["g0"], ptr["gx"], N, K0, J0, J1, J2, *(int(a) for a in acts),
                                 stream()), "lipvq_mlp3_bwd_f32")
    torch.cuda.synchronize()
    return {k: (None if v is None else v.check()) for k, v in f.items()}


@pytest.mark.parametrize("name,dims,mode", B.MLP3_EXTENT_CASES, ids=[c[0] for c in B.MLP3_EXTENT_CASES])
def test_mlp3_bwd_write_extent(name, dims, mode):
    """g2, g1, g0, gx between guard words on each of the four kernels (odd K0: the element-store side of the last link), with g2 or
    gx left out, and with every output 4 bytes off a 16-byte boundary; the bits are those of the wrapper's plain allocations."""
    case, pk, gy, pre, want = _mlp3_dev(dims)
    out = _mlp3_bwd(pk, gy, pre, dims, want_g2=mode != "no_g2", want_gx=mode != "no_gx", offset=1 if mode == "offset_out" else 0)
    for k, v in out.items():
        if v is None:
            assert (k, mode) in (("g2", "no_g2"), ("gx", "no_gx"))
        else:
            assert same_bits(v, want[k]), k
    if dims[5][2] == B.ACT_NONE:
        assert same_bits(want["g2"], gy)                          # an identity output layer: g2 is gy


@pytest.mark.parametrize("name,dims", B.MLP3_ISOLATION_CASES, ids=[c[0] for c in B.MLP3_ISOLATION_CASES])
def test_mlp3_bwd_row_isolation(name, dims):
    """One NaN in gy at the first / last row of a 32-row tile, the first row of the second sub-tile and the last row of the batch:
    that row of g1, g0 and gx is all NaN, g2 follows the map (the one planted element), every other row keeps its bits."""
    case, pk, gy, pre, clean = _mlp3_dev(dims)
    N, J2 = dims[0], dims[4]
    for v in clean.values():
        assert torch.isfinite(v).all()
    zero = torch.zeros((), dtype=torch.int32, device="cuda")
    for row in B.mlp3_isolation_rows(N):
        col = row % J2
        masks = [m.cuda() for m in B.mlp3_poison_map(case, row, col)]
        gyp = gy.clone()
        gyp[row, col] = float("nan")
        out = _mlp3_bwd(pk, gyp, pre, dims)
        for (k, got), m in zip(out.items(), masks):
            assert torch.equal(torch.isnan(got), m), f"{k}: NaN set differs from the map (NaN at gy[{row}, {col}])"
            assert torch.equal(torch.where(m, zero, bits(got)), torch.where(m, zero, bits(clean[k]))), f"{k}: a row other than {row} changed"
            if k != "g2":
                assert bool(m[row].all()) and int(m.sum()) == m.shape[1]


@pytest.mark.parametrize("dims", B.MLP3_PERMUTATION_CASES, ids=[f"N={d[0]} J2={d[4]}" for d in B.MLP3_PERMUTATION_CASES])
def test_mlp3_bwd_row_permutation_and_repeat(dims):
    """Permuting the rows of gy and of the saved pre-activations permutes the rows of every output bit for bit (no dependence on the
    position in tile, sub-tile or workgroup); the same call twice gives the same bits."""
    case, pk, gy, pre, want = _mlp3_dev(dims)
    N = dims[0]
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(N)).cuda()
    out = _mlp3_bwd(pk, gy[perm].contiguous(), [None if p is None else p[perm].contiguous() for p in pre], dims)
    for k, v in out.items():
        assert same_bits(v, want[k][perm]), k
    again = _mlp3_bwd(pk, gy, pre, dims)
    for k, v in again.items():
        assert same_bits(v, want[k]), k


@pytest.mark.parametrize("term,a_form,b_form", B.VQ_FORMS)
def test_mlp3_bwd_vq_equals_scaled_diff_then_mlp3_bwd(ops, term, a_form, b_form):
    """lipvq_mlp3_bwd_vq_f32 at the smallest batch it takes, every operand form (rows, or a table and an index vector): the header
    promises the numbers of lipvq_scaled_diff_f32 followed by lipvq_mlp3_bwd_f32 -- asserted on bits, on fenced outputs."""
    lib, check, stream = _capi()
    c = B.vq_case(term, 17 + len(term))
    N, K0, J0, J1, J2 = c["dims"]
    acts = c["acts"]
    assert N == B.LDS_ROWS and lib.lipvq_mlp3_bwd_vq_supported(N, K0, J0, J1, J2) == 1
    assert lib.lipvq_mlp3_bwd_vq_supported(N - 1, K0, J0, J1, J2) == 0
    W, b = [w.cuda() for w in c["W"]], [v.cuda() for v in c["b"]]
    y, pre = ops.mlp3(c["x"].cuda(), ops.mlp3_pack(W[0], b[0], W[1], b[1], W[2], b[2]), acts, save_pre=True)
    pk = ops.mlp3_pack_bwd(*W)
    gs = torch.tensor([3.0], device="cuda")
    alpha = 0.37 if term == "in" else 0.011
    tab = {nm: (c[nm + "_table"].cuda(), c[nm + "_idx"].cuda()) for nm in ("a", "b_op")}
    rows = {nm: t[i].contiguous() for nm, (t, i) in tab.items()}

    def operand(nm, form):                                        # (pointer, index pointer) of one operand in the asked form
        return (rows[nm].data_ptr(), None) if form == "rows" else (tab[nm][0].data_ptr(), tab[nm][1].data_ptr())

    f = {"g2": _Fenced("g2", N, J2), "g1": _Fenced("g1", N, J1), "g0": _Fenced("g0", N, J0), "gx": _Fenced("gx", N, K0)}
    if term == "in":                                              # gy := alpha gscale (act2(pre2) - B): y is the forward's own act2(pre2)
        gy = ops.scaled_diff(y, rows["b_op"], alpha, gscale=gs)
        want = ops.mlp3_bwd(gy, pre, pk, acts, want_gx=True)
        bp, bi = operand("b_op", b_form)
        args = (None, bp, bi, alpha, None, None, None, None, 0.0)
    else:                                                         # gx := alpha gscale (A - B) + gx
        gy = c["gy"].cuda()
        g2, g1, g0, gx = ops.mlp3_bwd(gy, pre, pk, acts, want_gx=True)
        want = (g2, g1, g0, ops.scaled_diff(rows["a"], rows["b_op"], alpha, gscale=gs, c=gx))
        (ap, ai), (bp, bi) = operand("a", a_form), operand("b_op", b_form)
        args = (gy.data_ptr(), None, None, 0.0, ap, ai, bp, bi, alpha)
    check(lib.lipvq_mlp3_bwd_vq_f32(args[0], pre[0].data_ptr(), pre[1].data_ptr(), pre[2].data_ptr(), pk.buf.data_ptr(),
                                    f["g2"].ptr(), f["g1"].ptr(), f["g0"].ptr(), f["gx"].ptr(), N, K0, J0, J1, J2, *(int(a) for a in acts),
                                    *args[1:], gs.data_ptr(), stream()), "lipvq_mlp3_bwd_vq_f32")
    torch.cuda.synchronize()
    for k, w in zip(("g2", "g1", "g0", "gx"), want):
        assert torch.isfinite(w).all() and same_bits(f[k].check(), w), k


# ---------------------------------------------------------------------------------------------------------------------------
# elementwise and small kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", B.ACT_BWD_N)
def test_act_bwd_extent(ops, n):
    """n on both sides of one block of 256, of one block's 1024 grid elements and of the 4096-block cap (grid-stride loop)."""
    lib, check, stream = _capi()
    g = torch.Generator().manual_seed(n)
    gin, pre = torch.randn(n, generator=g).cuda(), (torch.randn(n, generator=g) * 3.0).cuda()
    pre[:: max(1, n // 7)] = 0.0
    for act in (B.ACT_NONE, B.ACT_GELU, B.ACT_SIGMOID, B.ACT_RELU):
        for off in (0, 1):
            out = _Fenced("out", n, offset_words=off)
            check(lib.lipvq_act_bwd_f32(gin.data_ptr(), pre.data_ptr(), out.ptr(), n, act, stream()), "lipvq_act_bwd_f32")
            torch.cuda.synchronize()
            assert same_bits(out.check(), ops.act_bwd(gin.view(n, 1), pre.view(n, 1), act).view(n)), (act, off)
        if act == B.ACT_NONE:
            assert same_bits(out.t, gin)
        if act == B.ACT_RELU:                                     # g * 1 or g * 0 (a zero of either sign)
            assert torch.equal(out.t, torch.where(pre > 0, gin, torch.zeros_like(gin)))


@pytest.mark.parametrize("n", B.SDIFF_N)
def test_scaled_diff_extent(n):
    """n on both sides of one block and of the 2048-block cap; the fp32 expression of backward_ref.scaled_diff_fp32, bit for bit."""
    lib, check, stream = _capi()
    g = torch.Generator().manual_seed(n)
    a, b, c = (torch.randn(n, generator=g) for _ in range(3))
    gs = torch.tensor([3.7])
    alpha = 2.0 / 7.0
    ad, bd, cd, gsd = a.cuda(), b.cuda(), c.cuda(), gs.cuda()
    for with_c in (False, True):
        for off in (0, 1):
            out = _Fenced("out", n, offset_words=off)
            check(lib.lipvq_scaled_diff_f32(ad.data_ptr(), bd.data_ptr(), cd.data_ptr() if with_c else None, alpha, gsd.data_ptr(),
                                            out.ptr(), n, stream()), "lipvq_scaled_diff_f32")
            torch.cuda.synchronize()
            want = R.scaled_diff_fp32(a, b, float(torch.tensor(alpha, dtype=torch.float32)), gs, c if with_c else None)
            assert same_bits(out.check().cpu(), want), (with_c, off)


@pytest.mark.parametrize("D,H", B.LIPB_DH)
def test_lipschitz_bwd_extent(ops, D, H):
    """(D, H) on both sides of the 16-row workgroup and of the 256-thread staging pass (16 H = 256), H up to the 256 limit."""
    lib, check, stream = _capi()
    g = torch.Generator().manual_seed(1000 * D + H)
    W, gWn = torch.randn(D, H, generator=g), torch.randn(D, H, generator=g)
    ci = torch.from_numpy(R.mixed_ci(W, D + H))
    Wd, cid, gd = W.cuda(), ci.cuda(), gWn.cuda()
    want_W, want_ci = ops.lipschitz_bwd(Wd, cid, gd)
    for off in (0, 1):
        gW, gci = _Fenced("gW", D, H, offset_words=off), _Fenced("gci", D, offset_words=off)
        check(lib.lipvq_lipschitz_bwd_f32(Wd.data_ptr(), cid.data_ptr(), gd.data_ptr(), gW.ptr(), gci.ptr(), D, H, stream()), "lipvq_lipschitz_bwd_f32")
        torch.cuda.synchronize()
        assert same_bits(gW.check(), want_W) and same_bits(gci.check(), want_ci)
    assert torch.isfinite(want_W).all() and torch.isfinite(want_ci).all()


def test_lipschitz_bwd_refusal_leaves_the_outputs_alone():
    lib, _, stream = _capi()
    D, H = 8, B.LIPB_HMAX + 1
    W = torch.randn(D, H, device="cuda")
    gW, gci = _Fenced("gW", D, H), _Fenced("gci", D)
    rc = lib.lipvq_lipschitz_bwd_f32(W.data_ptr(), torch.ones(D, device="cuda").data_ptr(), W.data_ptr(), gW.ptr(), gci.ptr(), D, H, stream())
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED and gW.untouched() and gci.untouched()


# ---------------------------------------------------------------------------------------------------------------------------
# spectral norm
# ---------------------------------------------------------------------------------------------------------------------------
def _spectral(W, u, v, training):
    """lipvq_spectral_norm_f32 with every output (and u, v, which it may write) between guard words."""
    lib, check, stream = _capi()
    J, K = W.shape
    f = {"Wsn": _Fenced("Wsn", J, K), "sigma": _Fenced("sigma", 1), "u": between_nans(u.cuda()), "v": between_nans(v.cuda())}
    Wd = W.cuda()
    check(lib.lipvq_spectral_norm_f32(Wd.data_ptr(), f["u"].ptr(), f["v"].ptr(), f["Wsn"].ptr(), f["sigma"].ptr(), J, K, int(training),
                                      B.SPECTRAL_EPS, stream()), "lipvq_spectral_norm_f32")
    torch.cuda.synchronize()
    return {k: x.check() for k, x in f.items()}


def _spectral_bwd(gWsn, out):
    lib, check, stream = _capi()
    J, K = gWsn.shape
    gW = _Fenced("gW", J, K)
    gd = gWsn.cuda()
    check(lib.lipvq_spectral_norm_bwd_f32(gd.data_ptr(), out["Wsn"].data_ptr(), out["u"].data_ptr(), out["v"].data_ptr(), out["sigma"].data_ptr(),
                                          gW.ptr(), J, K, stream()), "lipvq_spectral_norm_bwd_f32")
    torch.cuda.synchronize()
    return gW.check()


def unit_norm_allowance(L):
    """|x / fl(|x|)| - 1 for an fp32 chain of L squares, one root and L divisions: the chain is gamma_L off in the SQUARE (half of it
    in the norm), root and division one rounding each; first order, doubled."""
    return R.gamma(L) + 4.0 * R.U32


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("J,K", B.SPECTRAL_JK)
def test_spectral_norm_extent_and_budget(J, K, training):
    c = B.spectral_case(J, K, 31 * J + K)
    ref = B.spectral_ref_and_budget(c["W"], c["u"], c["v"], training)
    out = _spectral(c["W"], c["u"], c["v"], training)
    tag = f"spectral J={J} K={K} training={training}"
    if training:                                                  # written back, unit norm
        close(out["u"], ref["u"], ref["d_u"], tag + " u")
        close(out["v"], ref["v"], ref["d_v"], tag + " v")
        assert abs(float(out["u"].double().norm()) - 1.0) <= unit_norm_allowance(J)
        assert abs(float(out["v"].double().norm()) - 1.0) <= unit_norm_allowance(K)
    else:                                                         # eval mode leaves u and v alone, bit for bit
        assert same_bits(out["u"].cpu(), c["u"]) and same_bits(out["v"].cpu(), c["v"])
    close(out["sigma"], ref["sigma"].reshape(1), ref["d_sigma"].reshape(1), tag + " sigma")
    close(out["Wsn"], ref["Wsn"], ref["d_Wsn"], tag + " Wsn")
    gW = _spectral_bwd(c["gWsn"], out)
    gref, allowed = B.spectral_bwd_ref_and_budget(c["gWsn"], out["Wsn"], out["u"], out["v"], out["sigma"])
    close(gW, gref, allowed, tag + " gW (from the kernel's own Wsn, u, v, sigma)")
    again = _spectral(c["W"], c["u"], c["v"], training)
    assert all(same_bits(again[k], out[k]) for k in out)


@pytest.mark.parametrize("J,K", B.SPECTRAL_REFUSED)
def test_spectral_norm_refuses_wider_than_256(J, K):
    lib, _, stream = _capi()
    W, u, v = torch.randn(J, K, device="cuda"), between_nans(torch.ones(J, device="cuda")), between_nans(torch.ones(K, device="cuda"))
    Wsn, sigma = _Fenced("Wsn", J, K), _Fenced("sigma", 1)
    rc = lib.lipvq_spectral_norm_f32(W.data_ptr(), u.ptr(), v.ptr(), Wsn.ptr(), sigma.ptr(), J, K, 1, B.SPECTRAL_EPS, stream())
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED and Wsn.untouched() and sigma.untouched()
    assert outside_untouched(u) and outside_untouched(v) and bool((u.t == 1).all()) and bool((v.t == 1).all())


def test_spectral_norm_rank_one():
    """W = p q^T: one power iteration lands on the singular vectors, sigma = |p| |q| (to the budget plus the rounding of W itself)."""
    J, K = 64, 7
    c = B.spectral_case(J, K, 5, "rank_one")
    ref = B.spectral_ref_and_budget(c["W"], c["u"], c["v"], True)
    out = _spectral(c["W"], c["u"], c["v"], True)
    close(out["sigma"], torch.tensor([c["sigma_exact"]], dtype=torch.float64), (ref["d_sigma"] + 2.0 * R.U32 * c["sigma_exact"]).reshape(1), "rank-one sigma")
    close(out["Wsn"], ref["Wsn"], ref["d_Wsn"], "rank-one Wsn")


def test_spectral_norm_all_zero_matrix_matches_torch_classes():
    """An all-zero W in training mode: torch's eps clamp gives u = v = 0, sigma = 0, W / sigma = NaN; every output element must be of
    the class (zero / NaN / Inf) that torch.nn.utils.spectral_norm produces on the CPU."""
    J, K = 9, 5
    c = B.spectral_case(J, K, 2, "zero")
    lin = torch.nn.Linear(K, J, bias=False)
    with torch.no_grad():
        lin.weight.zero_()
    sn = torch.nn.utils.spectral_norm(lin, n_power_iterations=1, eps=B.SPECTRAL_EPS)
    with torch.no_grad():
        sn.weight_u.copy_(c["u"])
        sn.weight_v.copy_(c["v"])
    sn.train()
    sn(torch.zeros(1, K))                                          # the forward pre-hook runs the power iteration and sets .weight
    out = _spectral(c["W"], c["u"], c["v"], True)
    assert torch.equal(B.value_class(out["u"]), B.value_class(sn.weight_u)) and torch.equal(B.value_class(out["v"]), B.value_class(sn.weight_v))
    assert torch.equal(B.value_class(out["Wsn"]), B.value_class(sn.weight))
    assert bool((B.value_class(sn.weight) == 2).all()) and bool((B.value_class(sn.weight_u) == 1).all())
    assert B.value_class(out["sigma"]).tolist() == [1]             # sigma = u . (W v) = 0
