"""GPU: the Lipschitz scale, the straight-through value and the mean-squared-error pair (csrc/lipvq_misc.hip) at their loop
seams, alignments and special values.

lipschitz_scale and ste are compared with == against the canonical oracle / numpy fp32.  mse_pair has no bit-exact reference
(its summation order is the kernel's own); its reference is float64: every fp32 pair widened to double, differenced and
squared exactly as the kernel does, summed EXACTLY (math.fsum) and divided by n.  The kernel adds at most 2^22 such squares in
double -- a relative error below 2^22 * 2^-53 = 5e-10, against fp32's 6e-8 -- and rounds once to fp32, so the result may differ
from float32(ref) only where ref sits within 5e-10 relative of a rounding boundary: |out - float32(ref)| <= 1 fp32 ulp of ref.
The data (1000 + randn on both sides) makes an fp32 accumulation miss that bound by orders of magnitude.

mse_partial_kernel runs 2048 x 256 = 524 288 threads (nth); its two-float4-in-flight main loop needs n / 4 > nth.  Sizes: 4 nth
(no thread enters the main loop), 4 nth + 4 (one thread does), 8 nth + 4003 (main loop, single float4 step and a 3-element
tail), and 1 ... 1023 for the scalar tail alone.  One-hot probes (zeros against zeros with a single 1.0) at every loop seam
must give exactly float32(1 / n): a dropped or doubled element shows as 0 or 2 / n.
"""
import numpy as np
import pytest
import torch

import seed_kernel_edges as E

pytestmark = pytest.mark.gpu

NTH = E.MSE_THREADS
EINVAL, EUNSUPPORTED = -1, -2           # include/lipvq.h
SENTINEL = -7777.25


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _at(a, off):
    """A device copy of the 1-D array `a` that starts `off` floats into a 16-byte aligned allocation."""
    buf = torch.empty(a.size + off + 4, device="cuda", dtype=torch.float32)
    v = buf[off:off + a.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


# ---------------------------------------------------------------------------------------------------------------------------
# lipschitz_scale
# ---------------------------------------------------------------------------------------------------------------------------
LIP_CLASSES = ("zero", "neg_zero", "overflow", "denormal", "zero_over_zero", "nan_ci")


def _lipschitz_case(D, H):
    rng = np.random.default_rng(D * 1000 + H)
    W = rng.standard_normal((D, H)).astype(np.float32)
    ci = rng.uniform(-3.0, 6.0, D).astype(np.float32)             # softplus(ci) on both sides of the row sums: scales < 1 and = 1
    rows = []
    for r in (0, D - 1, 15, 16, D // 2, 1, 2, D - 2):              # group seams of the 16-row workgroups first
        if 0 <= r < D and r not in rows:
            rows.append(r)
    planted = {}
    for i, r in enumerate(rows[:len(LIP_CLASSES)]):
        cls = LIP_CLASSES[(i + D + H) % len(LIP_CLASSES)]
        planted[r] = cls
        if cls == "zero":
            W[r] = 0.0
        elif cls == "neg_zero":
            W[r] = -0.0
        elif cls == "overflow":                                    # two elements of 3e38: the |w| sum overflows, the scale is 0
            W[r, :2] = 3e38
        elif cls == "denormal":
            W[r] = np.float32(1e-40) * np.sign(W[r])
        elif cls == "zero_over_zero":                              # softplus(-200) = 0 over a zero sum: NaN, clamped to 1 by !(sc < 1)
            W[r] = 0.0
            ci[r] = -200.0
        elif cls == "nan_ci":
            ci[r] = np.nan
    return W, ci, planted


@pytest.mark.parametrize("D,H", [(1, 1), (15, 255), (16, 256), (17, 129), (33, 7), (208, 128), (512, 64)])
def test_lipschitz_scale_bit_exact(ops, oracle, D, H):
    """Signed weights (the index-ordered |w| chain), a partial last 16-row group, H up to LIPS_HMAX, and planted rows: all zeros,
    all -0.0, an overflowing sum, denormals only, 0 / 0, ci = NaN.  scale and Wn equal the oracle; NULL scale / NULL Wn write
    the other output alone."""
    W, ci, planted = _lipschitz_case(D, H)
    sc_ref, wn_ref = oracle.lipschitz_scale(W, ci)
    for r, cls in planted.items():                               # the oracle's answers for the planted rows are the contract's
        if cls in ("zero", "neg_zero", "denormal", "zero_over_zero", "nan_ci"):
            assert sc_ref[r] == 1.0, (r, cls)
        if cls == "overflow" and H >= 2:
            assert sc_ref[r] == 0.0 and (wn_ref[r] == 0).all()
    assert not np.isnan(sc_ref).any() and not np.isnan(wn_ref).any()
    Wd, cid = dev(W), dev(ci)
    sc, wn = ops.lipschitz_scale(Wd, cid)
    assert np.array_equal(sc.cpu().numpy(), sc_ref)
    assert np.array_equal(wn.cpu().numpy(), wn_ref)
    assert np.array_equal(np.signbit(wn.cpu().numpy()), np.signbit(wn_ref))          # (-0.0 rows stay -0.0)
    # one output NULL: the other is written, nothing else
    sc2 = torch.full((D + 2,), SENTINEL, device="cuda")
    wn2 = torch.full((D * H + 2,), SENTINEL, device="cuda")
    assert ops.lib.lipvq_lipschitz_scale_f32(Wd.data_ptr(), cid.data_ptr(), sc2.data_ptr() + 4, None, D, H, _stream()) == 0
    assert ops.lib.lipvq_lipschitz_scale_f32(Wd.data_ptr(), cid.data_ptr(), None, wn2.data_ptr() + 4, D, H, _stream()) == 0
    torch.cuda.synchronize()
    sc2, wn2 = sc2.cpu().numpy(), wn2.cpu().numpy()
    assert np.array_equal(sc2[1:-1], sc_ref) and np.array_equal(wn2[1:-1].reshape(D, H), wn_ref)
    assert sc2[0] == sc2[-1] == wn2[0] == wn2[-1] == np.float32(SENTINEL)


def test_lipschitz_scale_refuses_rows_wider_than_256(ops):
    D, H = 3, 257
    W = torch.ones(D, H, device="cuda")
    ci = torch.ones(D, device="cuda")
    sc = torch.full((D,), SENTINEL, device="cuda")
    wn = torch.full((D, H), SENTINEL, device="cuda")
    rc = ops.lib.lipvq_lipschitz_scale_f32(W.data_ptr(), ci.data_ptr(), sc.data_ptr(), wn.data_ptr(), D, H, _stream())
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED
    assert bool((sc == SENTINEL).all()) and bool((wn == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------
# ste
# ---------------------------------------------------------------------------------------------------------------------------
def _ste_case(n):
    rng = np.random.default_rng(n)
    ze = rng.standard_normal(n).astype(np.float32)
    zq = rng.standard_normal(n).astype(np.float32)
    plant = [(np.inf, np.inf), (-3e38, 3e38), (-0.0, -0.0), (0.0, -0.0), (1e-40, 3e-40), (-1e-40, 1e-45), (np.nan, 1.0), (1.0, -np.inf)]
    for i, (a, b) in enumerate(plant):                           # (ze, zq): inf - inf, 3e38 - (-3e38), signed zeros, denormals
        for p in ((i * 37) % n, n - 1 - (i * 41) % n):
            ze[p], zq[p] = a, b
    return ze, zq


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257, NTH - 1, NTH, NTH + 1, 3 * NTH + 5])
def test_ste_bit_exact(ops, n, off):
    """ze + (zq - ze) in fp32, elementwise, against numpy: one thread, the 256-thread block seam, the 2048-block grid cap
    (524 288 threads: from 524 289 elements on the grid-stride loop makes a second pass; 3 x 524 288 + 5 makes four), planted
    inf - inf, overflow, signed zeros and denormals; aligned tensors and all three offset by one float."""
    ze, zq = _ste_case(n)
    with np.errstate(all="ignore"):
        ref = ze + (zq - ze)
    assert ref.dtype == np.float32
    zed, zqd = _at(ze, off), _at(zq, off)
    buf = torch.full((n + off + 2,), SENTINEL, device="cuda")
    out = buf[off:off + n]
    if not off:
        assert np.array_equal(ops.ste(zed, zqd).cpu().numpy(), ref, equal_nan=True)
    assert ops.lib.lipvq_ste_f32(zed.data_ptr(), zqd.data_ptr(), out.data_ptr(), n, _stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, ref, equal_nan=True)
    assert np.array_equal(np.signbit(got[ref == 0]), np.signbit(ref[ref == 0]))
    rest = torch.cat([buf[:off], buf[off + n:]])
    assert bool((rest == SENTINEL).all()), "ste wrote outside its n elements"


def test_ste_of_nothing_is_a_no_op(ops):
    a = torch.full((8,), SENTINEL, device="cuda")
    assert ops.lib.lipvq_ste_f32(a.data_ptr(), a.data_ptr(), a.data_ptr(), 0, _stream()) == 0
    assert ops.lib.lipvq_ste_f32(None, None, None, 0, _stream()) == 0
    assert ops.lib.lipvq_ste_f32(a.data_ptr(), a.data_ptr(), a.data_ptr(), -1, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((a == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------
# mse_pair
# ---------------------------------------------------------------------------------------------------------------------------
MSE_SIZES = (1, 3, 4, 5, 1023, 4 * NTH, 4 * NTH + 4, 8 * NTH + 4003)
# (a offset, b offset) in floats from a 16-byte boundary: any misalignment of either operand takes the scalar path
ALIGNMENTS = {"aligned": (0, 0), "a+1": (1, 0), "b+3": (0, 3), "both+2": (2, 2)}


@pytest.fixture(scope="module")
def mse_data():
    """Per size and role: the two fp32 operands (1000 + randn) and the exact float64 mean of their squared differences."""
    out = {}
    for role in (0, 1):
        for n in MSE_SIZES:
            rng = np.random.default_rng(n * 2 + role)
            a = (1000.0 + rng.standard_normal(n)).astype(np.float32)
            b = (1000.0 + rng.standard_normal(n)).astype(np.float32)
            out[role, n] = (a, b, E.mse_ref(a, b))
    return out


def _mse_pair(ops, a0, b0, a1, b1, fn=None):
    out = torch.full((4,), SENTINEL, device="cuda")
    ws = torch.empty(ops.lib.lipvq_mse_workspace_bytes(), device="cuda", dtype=torch.uint8)
    rc = ops.lib.lipvq_mse_pair_f32(a0.data_ptr(), b0.data_ptr(), a0.numel(), a1.data_ptr(), b1.data_ptr(), a1.numel(),
                                    out.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, ops.lib.lipvq_last_error()
    o = out.cpu().numpy()
    assert o[2] == o[3] == np.float32(SENTINEL)
    return o[:2]


def _within_one_ulp(got, ref, what):
    r32 = np.float32(ref)
    err = abs(float(got) - float(r32))
    print(f"{what}: got {float(got)!r} float32(ref) {float(r32)!r} err/ulp {err / E.ulp32(r32):.2f}")
    assert err <= E.ulp32(r32), (what, float(got), float(r32))


@pytest.mark.parametrize("align", list(ALIGNMENTS))
def test_mse_pair_against_float64(ops, mse_data, align):
    """Every size on either side (nx and nz paired independently: size i with size 3 i + 1 mod 8), every alignment."""
    oa, ob = ALIGNMENTS[align]
    onto = {}
    for key, (a, b, _) in mse_data.items():
        onto[key] = (_at(a, oa), _at(b, ob))
    for i, nx in enumerate(MSE_SIZES):
        nz = MSE_SIZES[(3 * i + 1) % len(MSE_SIZES)]
        got = _mse_pair(ops, *onto[0, nx], *onto[1, nz])
        _within_one_ulp(got[0], mse_data[0, nx][2], f"{align} nx={nx}")
        _within_one_ulp(got[1], mse_data[1, nz][2], f"{align} nz={nz}")
    # fp32 accumulation would not pass: the bound separates the kernel from the naive sum on this data
    a, b, ref = mse_data[0, MSE_SIZES[-1]]
    naive = np.cumsum(((a - b) * (a - b)).astype(np.float32), dtype=np.float32)[-1] / np.float32(a.size)
    assert abs(float(naive) - ref) > 4 * E.ulp32(ref)


@pytest.mark.parametrize("align", ["aligned", "a+1"])
def test_mse_pair_one_hot_probes(ops, align):
    """Zeros against zeros with a single 1.0 at each seam of mse_partial_kernel's loops (mse_probe_positions), one launch per
    position: the mean is exactly float32(1 / n)."""
    oa, ob = ALIGNMENTS[align]
    nmax = MSE_SIZES[-1]
    abuf = torch.zeros(nmax + 8, device="cuda")
    bbuf = torch.zeros(nmax + 8, device="cuda")
    small_a, small_b = torch.zeros(5, device="cuda"), torch.zeros(5, device="cuda")
    launches = 0
    for n in MSE_SIZES:
        a, b = abuf[oa:oa + n], bbuf[ob:ob + n]
        for k, p in enumerate(E.mse_probe_positions(n, align == "aligned")):
            hot, cold = (a, b) if k % 2 == 0 else (b, a)           # the 1.0 on either operand: (+1)^2 and (-1)^2
            hot[p] = 1.0
            small_b[k % 5] = 1.0
            got = _mse_pair(ops, a, b, small_a, small_b)
            hot[p] = 0.0
            small_b[k % 5] = 0.0
            assert got[0] == np.float32(1.0 / n), f"n={n} position {p}: {got[0]!r} != 1/n = {np.float32(1.0 / n)!r}"
            assert got[1] == np.float32(1.0 / 5), (n, p, got[1])
            launches += 1
    assert launches >= 20
    assert _mse_pair(ops, abuf[oa:oa + 7], bbuf[ob:ob + 7], small_a, small_b).tolist() == [0.0, 0.0]


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("which", [0, 1])
def test_mse_pair_non_finite_stays_in_its_pair(ops, mse_data, which, bad):
    """One non-finite difference in one pair: that mean is inf (NaN for a NaN), the other pair's stays within its bound."""
    nx, nz = MSE_SIZES[-1], 1023
    a0, b0, r0 = mse_data[0, nx]
    a1, b1, r1 = mse_data[1, nz]
    t = [_at(a0, 0), _at(b0, 0), _at(a1, 0), _at(b1, 0)]
    t[2 * which][(4 * NTH + 17) % t[2 * which].numel()] = float(bad)
    got = _mse_pair(ops, *t)
    if np.isnan(bad):
        assert np.isnan(got[which])
    else:
        assert got[which] == np.inf
    _within_one_ulp(got[1 - which], (r0, r1)[1 - which], f"the other pair (bad in {which})")


@pytest.mark.parametrize("w", [0.0, 1.0, 0.25])
def test_mse_pair_loss_association(ops, mse_data, w):
    """out[2] from out[0], out[1] in the association include/lipvq.h writes down, in fp32: LLFQ (m0 + w m1) + w m1, VQ
    m0 + (m1 + w m1); the means equal lipvq_mse_pair_f32's."""
    a0, b0, _ = mse_data[0, 1023]
    a1, b1, _ = mse_data[1, 4 * NTH + 4]
    t = [dev(v) for v in (a0, b0, a1, b1)]
    plain = ops.mse_pair(*t).cpu().numpy()
    for form in (ops.LOSS_LLFQ, ops.LOSS_VQ):
        o = ops.mse_pair_loss(*t, w, form).cpu().numpy()
        assert np.array_equal(o[:2], plain)
        m0, m1, wf = np.float32(o[0]), np.float32(o[1]), np.float32(w)
        q = np.float32(wf * m1)
        want = np.float32(np.float32(m0 + q) + q) if form == ops.LOSS_LLFQ else np.float32(m0 + np.float32(m1 + q))
        assert o[2] == want, (form, w, o[2], want)
        if w == 0.0:
            assert o[2] == np.float32(m0 + m1) if form == ops.LOSS_VQ else o[2] == m0


def test_mse_pair_errors(ops):
    a = torch.ones(8, device="cuda")
    out = torch.full((3,), SENTINEL, device="cuda")
    ws = torch.empty(ops.lib.lipvq_mse_workspace_bytes(), device="cuda", dtype=torch.uint8)
    p, o, w = a.data_ptr(), out.data_ptr(), ws.data_ptr()
    assert ops.lib.lipvq_mse_pair_f32(p, p, 0, p, p, 8, o, w, _stream()) == EINVAL
    assert ops.lib.lipvq_mse_pair_f32(p, p, 8, p, p, 0, o, w, _stream()) == EINVAL
    assert ops.lib.lipvq_mse_pair_loss_f32(p, p, 8, p, p, 8, o, 0.25, 2, w, _stream()) == EINVAL
    assert ops.lib.lipvq_mse_pair_loss_f32(p, p, 8, p, p, 8, o, 0.25, -1, w, _stream()) == EINVAL
    assert ops.lib.lipvq_mse_pair_loss_f32(p, p, 0, p, p, 8, o, 0.25, 0, w, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
