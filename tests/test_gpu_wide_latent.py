"""GPU: nearest-code search at latent widths 209 ... 512 -- the wide screening instances (S = 16, 24, 32 k-steps, chunked
column sweep), the widened small-batch kernel and the modules that route through them -- equals the oracle bit for bit, and
the wide screen's error bound holds with a >= 4x margin."""
import numpy as np
import pytest
import torch

from oracle import lipvq_oracle as O

pytestmark = pytest.mark.gpu
GAMMA_WIDE = 2.0 ** -16          # LIPVQ_SCREEN_GAMMA_WIDE (lipvq_screen.h): the bound the wide instances certify with


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ops():
    import lipvq_vae_amd
    return lipvq_vae_amd.ops


def _case(seed, N, K, D, spread=1.0):
    rng = np.random.default_rng(seed)
    cb = (0.5 + spread * (rng.uniform(0, 1, (K, D)) - 0.5)).astype(np.float32)
    z = rng.uniform(0, 1, (N, D)).astype(np.float32)
    m = min(N, K) // 2
    z[:m] = cb[rng.permutation(K)[:m]] + (0.02 * rng.standard_normal((m, D))).astype(np.float32)
    return z, cb


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("dist", [O.DIST_NORM, O.DIST_SQSUM])
@pytest.mark.parametrize("N,K,D", [(4096, 1024, 256), (1000, 256, 209), (700, 1000, 384), (513, 2048, 512), (33, 37, 300),
                                   (1, 5, 512)])
def test_wide_screened_equals_oracle(ops, oracle, N, K, D, dist):
    assert ops.nearest_screen_supported(K, D) and not ops.screen_is_coarse(K, D)
    z, cb = _case(N + K + D + dist, N, K, D)
    if K > 3:
        cb[K - 1] = cb[1]                       # exact duplicate -> a tie only the exact stage decides
        z[: min(N, 8)] = cb[1]
    idx_ref, zq_ref, usage_ref = oracle.nearest(z, cb, dist=dist)
    cbd = dev(cb)
    usage = torch.zeros(K, dtype=torch.int64, device="cuda")
    idx, zq, ws = ops.nearest_screened(dev(z), cbd, ops.nearest_prepare(cbd), usage=usage, return_workspace=True, dist=dist)
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    assert np.array_equal(zq.cpu().numpy(), zq_ref)
    assert np.array_equal(usage.cpu().numpy(), usage_ref)
    n_exact = int(ws[0])
    if K > 3:
        assert n_exact >= int((idx_ref == 1).sum()) >= 1        # rows on the duplicated code reached the exact stage
    if N >= 500:
        assert n_exact < N // 2, "the screen certified too little"


@pytest.mark.parametrize("D", [256, 384, 512])
def test_wide_error_bound_holds(ops, D):
    """|d~ - d| against float64 stays below 1/4 of the bound the wide instances use, over spreads and magnitudes."""
    worst = 0.0
    K, N = 512, 256
    for i, (spread, scale) in enumerate([(0.2, 1.0), (1.0, 1.0), (3.0, 1.0), (1.0, 1e-6), (1.0, 1e-3), (1.0, 1e3), (1.0, 1e6)]):
        z, cb = _case(D + i, N, K, D, spread)
        z, cb = (z * scale).astype(np.float32), (cb * scale).astype(np.float32)
        cbd = dev(cb)
        prep = ops.nearest_prepare(cbd)
        _, _, dt = ops.nearest_screened(dev(z), cbd, prep, debug_gamma=GAMMA_WIDE)
        dt = dt.cpu().numpy().astype(np.float64)[:, :K]
        mu = cb.astype(np.float64).mean(0)
        zc, ec = z.astype(np.float64) - mu, cb.astype(np.float64) - mu
        d = (ec * ec).sum(1)[None, :] - 2.0 * zc @ ec.T
        e2max = (ec * ec).sum(1).max()
        bound = GAMMA_WIDE * (e2max + 2.0 * np.sqrt((zc * zc).sum(1)) * np.sqrt(e2max))
        worst = max(worst, (np.abs(dt - d) / bound[:, None]).max())
    assert worst < 0.25, f"screening error reached {worst:.3f} of its bound"


@pytest.mark.parametrize("dist", [O.DIST_NORM, O.DIST_SQSUM])
@pytest.mark.parametrize("D", [212, 256, 300, 388, 512])         # (300, 388: the small route's run-time width, LDS image > 64 KiB)
@pytest.mark.parametrize("N", [1, 80, 500, 4096])
def test_wide_nearest_rows_both_routes(ops, oracle, N, D, dist):
    K = 1024
    z, cb = _case(N * 3 + D, N, K, D)
    cb[K - 1] = cb[2]
    idx_ref, zq_ref, usage_ref = oracle.nearest(z, cb, dist=dist)
    zd, cbd = dev(z), dev(cb)
    for route in ("small", "rows"):
        usage = torch.zeros(K, dtype=torch.int64, device="cuda")
        idx, zq = ops.nearest_rows(zd, cbd, usage=usage, dist=dist, route=route)
        assert np.array_equal(idx.cpu().numpy(), idx_ref), route
        assert np.array_equal(zq.cpu().numpy(), zq_ref), route
        assert np.array_equal(usage.cpu().numpy(), usage_ref), route


def test_small_batch_kernel_covers_wide_latents(ops):
    assert ops.lib.lipvq_nearest_small_supported(80, 1024, 512) == 1
    assert ops.lib.lipvq_nearest_small_supported(500, 1024, 256) == 1
    assert ops.lib.lipvq_nearest_small_supported(80, 1024, 516) == 0       # (the first multiple of 4 above the limit)
    assert ops.lib.lipvq_nearest_small_supported(80, 1024, 510) == 0       # (a multiple of 4 only)


@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("tri", [False, True])
def test_wide_near_ties_match_the_oracle(ops, oracle, D, tri):
    K = 1024
    N = K // 2 if tri else 2048                        # (make_neartie3_case moves one code per row: N <= K / 2)
    z, cb = (O.make_neartie3_case if tri else O.make_neartie_case)(D + int(tri), N, K, D)
    zd, cbd = dev(z), dev(cb)
    prep = ops.nearest_prepare(cbd)
    for dist in (O.DIST_NORM, O.DIST_SQSUM):
        idx_ref, zq_ref, _ = oracle.nearest(z, cb, dist=dist)
        idx, zq = ops.nearest_screened(zd, cbd, prep, dist=dist)
        assert np.array_equal(idx.cpu().numpy(), idx_ref) and np.array_equal(zq.cpu().numpy(), zq_ref)


def test_llfq_module_at_latent_width_256(ops, oracle):
    """LLFQVAE_V4(12, 256, 1024): a 65 536-row tokenize takes the wide screen (trained-like codebook: the exact stage has little
    to do), training steps of 80 and 500 rows take the small-batch kernel; values and gradients against the oracle."""
    from lipvq_vae_amd.tokenizer import LLFQVAE_V4
    A, D, K = 12, 256, 1024
    assert not ops.tokenize_supported(A, 64, 128, D, K)        # (no fused launch at this width: the unfused encoder + screen)
    p = O.make_params(31, A, D, K, oracle=oracle)
    model = LLFQVAE_V4(A, D, num_codes=K).cuda()
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()})
    x = O.make_inputs(32, 65536, A)
    idx_ref, zq_ref, _ = oracle.nearest(oracle.llfq_encode(p, x), p["quantizer.codebook"])
    idx, zq = model.tokenize(_cuda(x), count_usage=False)
    assert np.array_equal(idx.cpu().numpy(), idx_ref) and np.array_equal(zq.cpu().numpy(), zq_ref)
    assert model.last_exact_rows is not None
    assert int(model.last_exact_rows[0]) < 65536 // 20
    for N in (80, 500):
        model.zero_grad()
        xs = O.make_inputs(N, N, A)
        f = oracle.llfq_forward(p, xs)
        z, loss = model(_cuda(xs))
        assert np.array_equal(z.detach().cpu().numpy(), f["z_q"]) and np.array_equal(model.last_indices.cpu().numpy(), f["indices"])
        assert abs(loss.item() - f["loss"]) <= 1e-5 * abs(f["loss"])
        loss.backward()
        g = oracle.llfq_grads(p, xs, fwd=f)
        for k, prm in model.named_parameters():
            scale = np.abs(g[k]).max() + 1e-12
            assert np.abs(prm.grad.cpu().numpy() - g[k]).max() <= 2e-5 * scale, (N, k)


def test_vqvae_module_at_latent_width_256(ops, oracle):
    """VQVAE(12, 256, 1024): tokenize through the wide screen (K >= SCREEN_MIN_CODES) and training steps of 80 and 500 rows."""
    from lipvq_vae_amd.tokenizer import VQVAE
    A, D, K = 12, 256, 1024
    p = O.make_params(41, A, D, K, variant="vq", oracle=oracle)
    model = VQVAE(A, D, num_embeddings=K).cuda()
    assert K >= model.SCREEN_MIN_CODES
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()})
    x = O.make_inputs(42, 65536, A)
    f = oracle.vq_forward(p, x)
    idx, zst = model.tokenize(_cuda(x), count_usage=False)               # (VQVAE.tokenize returns z_e + (z_q - z_e))
    assert np.array_equal(idx.cpu().numpy(), f["indices"]) and np.array_equal(zst.cpu().numpy(), f["z_latent"])
    assert model.last_exact_rows is not None
    for N in (80, 500):
        model.zero_grad()
        xs = O.make_inputs(N + 1, N, A)
        f = oracle.vq_forward(p, xs)
        z, loss = model(_cuda(xs))
        assert np.array_equal(model.last_indices.cpu().numpy(), f["indices"])
        assert abs(loss.item() - f["loss"]) <= 1e-5 * abs(f["loss"])
        loss.backward()
        g = oracle.vq_grads(p, xs, fwd=f)
        for k, prm in model.named_parameters():
            scale = np.abs(g[k]).max() + 1e-12
            assert np.abs(prm.grad.cpu().numpy() - g[k]).max() <= 2e-5 * scale, (N, k)


@pytest.mark.parametrize("N", [80, 500])
def test_graphed_training_step_at_latent_width_256_equals_eager(oracle, N):
    import copy
    from lipvq_vae_amd.icl import GraphedTokenizerStep, VQTokenizerTrainer
    from lipvq_vae_amd.tokenizer import LLFQVAE_V4
    A, D, K = 12, 256, 1024
    p = O.make_params(51, A, D, K, oracle=oracle)
    model = LLFQVAE_V4(A, D, num_codes=K).cuda()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in p.items()})
    twin = copy.deepcopy(model)
    twin.invalidate_caches()
    tr, tw = VQTokenizerTrainer(model), VQTokenizerTrainer(twin)
    xs = [torch.from_numpy(O.make_inputs(600 + N + i, N, A)).cuda() for i in range(4)]
    g = GraphedTokenizerStep(model, xs[0], optimizer_state=tr.vq_optimizer.state_dict(), warmup=2)
    for i in range(1, 4):
        _, loss = g.step(xs[i])
        idx_g = model.last_indices.clone()
        _, ref_loss = tw.train_on_actions(xs[i])
        assert torch.equal(idx_g, twin.last_indices), i            # the quantizer's decisions: identical
        assert abs(float(loss) - float(ref_loss)) <= 2e-5 * abs(float(ref_loss)), i
    torch.cuda.synchronize()
    # (the small-batch weight gradients are summed in an order that may differ between a replay and an eager step: the same
    # tolerance as tests/test_gpu_icl.py's small-batch graphed step)
    for (k, a), (_, b) in zip(model.state_dict().items(), twin.state_dict().items()):
        assert torch.isfinite(a).all(), k
        assert float((a - b).abs().max()) <= 5e-5, (k, float((a - b).abs().max()))


@pytest.mark.parametrize("dist", [O.DIST_NORM, O.DIST_SQSUM])
@pytest.mark.parametrize("N,K,D", [(5000, 1024, 256), (3000, 300, 512), (777, 1000, 384), (2049, 37, 263), (1, 5, 300)])
def test_wide_all_pairs_equals_oracle(ops, oracle, N, K, D, dist):
    """The all-pairs exact kernel (ops.nearest, the route of batches the screen monitor keeps away from the screen) at wide widths:
    LDS-staged, the first minimum, an exact duplicate code; and the best distance it reports."""
    z, cb = _case(N + 7 * D + dist, N, K, D)
    if K > 3:
        cb[K - 1] = cb[1]
        z[: min(N, 8)] = cb[1]
    idx_ref, zq_ref, usage_ref, best_ref = oracle.nearest(z, cb, dist=dist, want_best=True)
    usage = torch.zeros(K, dtype=torch.int64, device="cuda")
    idx, zq, best = ops.nearest(dev(z), dev(cb), dist, usage=usage, want_best=True)
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    assert np.array_equal(zq.cpu().numpy(), zq_ref)
    assert np.array_equal(usage.cpu().numpy(), usage_ref)
    assert np.array_equal(best.cpu().numpy(), best_ref)


@pytest.mark.parametrize("D", [256, 384, 512])
def test_wide_screen_certifies_with_the_wide_gamma(ops, D):
    """Rows whose two best codes are separated by 3 x 2^-18 of the bound's scale (E2max + 2 |z'| Emax): a screen that certified with
    the narrow instances' 2^-18 would certify them (margin 2 gamma), the wide instances' 2^-16 must not -- every such row goes to the
    exact stage on the default route, while the debug hook with gamma = 2^-18 certifies most of them."""
    rng = np.random.default_rng(D)
    K, N = 512, 256
    cb = rng.uniform(0, 1, (K, D)).astype(np.float32)
    a = rng.integers(0, K, N)
    b = (a + 1 + rng.integers(0, K - 1, N)) % K
    mu = cb.astype(np.float64).mean(0)
    ec = cb.astype(np.float64) - mu
    e2max = (ec * ec).sum(1).max()
    m = 0.5 * (cb[a].astype(np.float64) + cb[b].astype(np.float64))
    u = cb[a].astype(np.float64) - cb[b].astype(np.float64)
    scale = e2max + 2.0 * np.sqrt(((m - mu) ** 2).sum(1)) * np.sqrt(e2max)
    gap = 3.0 * 2.0 ** -18 * scale                                   # |z - e_b|^2 - |z - e_a|^2 at z = m + t u: 2 t |u|^2
    t = gap / (2.0 * (u * u).sum(1))
    z = (m + t[:, None] * u).astype(np.float32)
    zc = z.astype(np.float64) - mu
    d = (ec * ec).sum(1)[None, :] - 2.0 * zc @ ec.T
    srt = np.sort(d, axis=1)
    real_gap = (srt[:, 1] - srt[:, 0]) / (e2max + 2.0 * np.sqrt((zc * zc).sum(1)) * np.sqrt(e2max))
    sel = (real_gap > 2.4 * 2.0 ** -18) & (real_gap < 6.0 * 2.0 ** -18)     # between 2 x 2^-18 and 2 x 2^-16, with room
    assert sel.sum() > N // 2
    cbd, zd = dev(cb), dev(z)
    prep = ops.nearest_prepare(cbd)
    _, _, ws = ops.nearest_screened(zd, cbd, prep, return_workspace=True)
    assert int(ws[0]) >= int(sel.sum())
    _, _, ws_n, _ = ops.nearest_screened(zd, cbd, prep, return_workspace=True, debug_gamma=2.0 ** -18)
    assert int(ws_n[0]) < N - int(sel.sum()) // 2
