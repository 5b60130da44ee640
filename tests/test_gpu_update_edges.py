"""GPU: the kernels a training step needs after the backward pass, where their one or two happy-path tests do not go: the EMA
codebook update (lipvq_ema_update_f32: K above one workgroup's 1024 threads, K D above the 2048-block grid-stride cap, zero counts,
decay 0 and 1, one code), the fused AdamW (lipvq_adamw_f32: more than the 32 tensors of one launch, two groups, six gradient
regimes) and the loss reductions (mse_partial_kernel's scalar path for operands off a 16-byte boundary, n % 4 != 0, the
two-float4-in-flight loop from 2 097 152 elements on; ste at one element and one past the grid-stride cap).

Yardsticks (tests/bin_ref.py; conditions in tests/test_bin_ref_host.py): float64 statements of each rule on the CPU -- for AdamW
torch.optim.AdamW itself on float64 copies -- at the project's existing bounds: EMA 1e-5 (1 + |want|), non-finite results the same
kind in the same place; AdamW 2e-6 max(1, max|p|) on parameters and rtol 1e-5 on exp_avg_sq; the two means 1e-6 relative."""
import numpy as np
import pytest
import torch

import bin_ref as B
from fenced import _Fenced

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ---- EMA ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,D", B.EMA_SHAPES)
def test_ema_update_states(oracle, ops, K, D):
    assert K == 1 or K * D > 0
    for state in B.EMA_STATES:
        s = B.ema_state(K, D, state)
        cs, es, cb = _Fenced("cluster_size", K, offset_words=1), _Fenced("embed_sum", K, D, offset_words=1), _Fenced("codebook", K, D)
        cs.t.copy_(cuda(s["cs"]))
        es.t.copy_(cuda(s["es"]))
        ops.ema_update(cs.t, es.t, cuda(s["counts"]), cuda(s["dw"]), cb.t, s["decay"], s["eps"])
        torch.cuda.synchronize()
        got = [host(f.check()) for f in (cs, es, cb)]
        want = B.ema_f64(s)
        orc = oracle.ema_update(s["cs"], s["es"], s["counts"], s["dw"], s["decay"], s["eps"])
        for name, g, w, o in zip(("cluster_size", "embed_sum", "codebook"), got, want, orc):
            fin = np.isfinite(w)
            used = float((np.abs(g[fin] - w[fin]) / (1e-5 * (1.0 + np.abs(w[fin])))).max()) if fin.any() else 0.0
            print(f"K={K} D={D} {state}: {name} uses {used:.3f} of the bound against float64, {int((~fin).sum())} non-finite")
            assert B.within_or_same_kind(g, w), (state, name)
            assert B.within_or_same_kind(g, o), (state, name, "oracle")
        if state in B.EMA_NONFINITE:
            assert np.isnan(got[2]).all()


# ---- AdamW -------------------------------------------------------------------------------------------------------------------

def _adamw_run(groups, regime, scale):
    """groups: list of (sizes, kwargs).  Runs ADAMW_STEPS steps of the fused AdamW on the GPU and torch.optim.AdamW on float64 CPU
    copies with the same fp32 gradients; asserts after every step."""
    from lipvq_vae_amd.optim import AdamW
    gp, cp, index = [], [], 0
    for sizes, kw in groups:
        init = B.adamw_params(sizes, scale, seed=len(sizes))
        gp.append(dict(params=[cuda(p).requires_grad_(True) for p in init], **kw))
        cp.append(dict(params=[torch.from_numpy(p).double().requires_grad_(True) for p in init], **kw))
    ours, ref = AdamW(gp, lr=1e-3, weight_decay=1e-4), torch.optim.AdamW(cp, lr=1e-3, weight_decay=1e-4)
    flat_g = [p for g in gp for p in g["params"]]
    flat_c = [p for g in cp for p in g["params"]]
    worst_p, worst_v = 0.0, 0.0
    for step in range(B.ADAMW_STEPS):
        updated = []
        for index, (a, b) in enumerate(zip(flat_g, flat_c)):
            g = B.adamw_grad(regime, a.numel(), step, index)
            a.grad = None if g is None else cuda(g)
            b.grad = None if g is None else torch.from_numpy(g).double()
            updated.append(g is not None)
        before = [a._version for a in flat_g]
        ours.step()
        ref.step()
        for index, (a, b) in enumerate(zip(flat_g, flat_c)):
            assert (a._version > before[index]) == updated[index], (step, index)
            err = float((a.detach().cpu().double() - b.detach()).abs().max())
            bound = 2e-6 * max(1.0, float(b.detach().abs().max()))
            worst_p = max(worst_p, err / bound)
            assert err <= bound, (regime, scale, step, index, a.numel(), err, bound)
    for index, (a, b) in enumerate(zip(flat_g, flat_c)):
        sa, sb = ours.state[a], ref.state[b]
        assert (len(sa) == 0) == (len(sb) == 0)
        assert float(sa["step"]) == float(sb["step"]), index
        va, vb = sa["exp_avg_sq"].cpu().double(), sb["exp_avg_sq"]
        assert torch.allclose(va, vb, rtol=1e-5, atol=1e-12), (regime, scale, index)
        rel = ((va - vb).abs() / vb.abs().clamp(min=1e-7)).max()
        worst_v = max(worst_v, float(rel) / 1e-5)
    steps = {float(ours.state[a]["step"]) for a in flat_g}
    assert steps == {float(B.ADAMW_STEPS), float(B.ADAMW_STEPS - 2)}                        # some parameters skipped two steps
    print(f"{regime} scale {scale:g} {[len(s) for s, _ in groups]} tensors: parameters use {worst_p:.3f} of 2e-6 max(1, max|p|), "
          f"exp_avg_sq {worst_v:.3f} of rtol 1e-5")


@pytest.mark.parametrize("count", (33, 65))
@pytest.mark.parametrize("regime", B.ADAMW_REGIMES)
def test_adamw_more_tensors_than_one_launch(regime, count):
    for scale in (1.0, 1e4):
        _adamw_run([(B.adamw_sizes(count), {})], regime, scale)


@pytest.mark.parametrize("regime", ("randn_decades", "spike"))
def test_adamw_two_groups(regime):
    sizes = B.adamw_sizes(33)
    _adamw_run([(sizes[:20], dict(lr=3e-3, betas=(0.8, 0.99), weight_decay=0.1)),
                (sizes[20:], dict(lr=1e-4, betas=(0.95, 0.9999), weight_decay=0.0))], regime, 1.0)


# ---- loss reductions ---------------------------------------------------------------------------------------------------------

def _off_boundary(t):
    """The same values as a view one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    v = buf[1:]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("nx,nz", list(zip(B.MSE_N, B.MSE_N[3:] + B.MSE_N[:3])))
def test_mse_pair_sizes_and_alignment(ops, nx, nz):
    assert nx != nz
    for big in (False, True):
        arrays = B.mse_pair_case(nx, nz, big=big)
        want = (B.mse_f64(arrays[0], arrays[1]), B.mse_f64(arrays[2], arrays[3]))
        dev = [cuda(a) for a in arrays]
        assert all(d.data_ptr() % 16 == 0 for d in dev)
        for shifted in (None, 0, 1, 2, 3):
            args = [(_off_boundary(d) if i == shifted else d) for i, d in enumerate(dev)]
            out = ops.mse_pair(*args)
            o = host(out).astype(np.float64)
            rel = [abs(o[i] - want[i]) / abs(want[i]) for i in range(2)]
            print(f"nx={nx} nz={nz} big={big} operand off its boundary: {shifted}: relative errors {rel[0]:.2e} {rel[1]:.2e}")
            assert rel[0] <= 1e-6 and rel[1] <= 1e-6
            for w, form in ((0.25, ops.LOSS_LLFQ), (0.37, ops.LOSS_VQ)):
                o3 = ops.mse_pair_loss(*args, w, form)
                m0, m1 = o3[0], o3[1]
                fold = (m0 + m1 * w) + m1 * w if form == ops.LOSS_LLFQ else m0 + (m1 + w * m1)
                assert torch.equal(o3[:2], out) and torch.equal(o3[2], fold)


@pytest.mark.parametrize("n", B.STE_N)
def test_ste_sizes(ops, n):
    rng = B.rng_of(n, 13)
    ze, zq = rng.uniform(0, 1, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
    ze[-1], zq[-1] = np.float32(1e-3), np.float32(0.7)                                      # ze + (zq - ze) != zq in fp32
    out = _Fenced("ste", n, offset_words=1)
    from lipvq_vae_amd import _capi
    tze, tzq = cuda(ze), cuda(zq)
    assert _capi.lib.lipvq_ste_f32(tze.data_ptr(), tzq.data_ptr(), out.ptr(), n, ops._stream()) == 0
    torch.cuda.synchronize()
    want = ze + (zq - ze)
    assert np.array_equal(host(out.check()), want)
    assert np.array_equal(host(ops.ste(tze, tzq)), want)
