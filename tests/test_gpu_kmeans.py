"""GPU: the opt-in k-means extension (lipvq_kmeans_* via ops.kmeans_*, kmeans.py, the tokenizers' init_codebook_ /
revive_dead_codes_) against the numpy restatement of its sampling rule (tests/kmeans_ref.py) and the CPU oracle, bit for bit."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import lipvq_oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import kmeans_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NORM, SQSUM = R.DIST_NORM, R.DIST_SQSUM


def _rows(seed, N, D):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, D)).astype(np.float32)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("N,K,D,dist", [(3000, 256, 64, NORM), (20000, 1024, 64, NORM), (5000, 512, 208, NORM),
                                        (4000, 300, 300, NORM), (777, 37, 7, SQSUM), (3000, 128, 64, SQSUM),
                                        (100, 256, 64, NORM)])
def test_seed_is_exact(oracle, N, K, D, dist):
    from lipvq_vae_amd import ops
    z = _rows(N + K + D, N, D)
    u = np.random.default_rng(K).random(K)
    init = np.random.default_rng(D).uniform(-1, 1, (K, D)).astype(np.float32)
    cb, picks, written = ops.kmeans_seed(torch.from_numpy(z).cuda(), K, torch.from_numpy(u).cuda(), dist,
                                         out=torch.from_numpy(init).cuda())
    ref_cb, ref_picks, ref_written = R.seed(oracle, z, K, u, dist, init=init)
    assert np.array_equal(picks.cpu().numpy(), ref_picks)
    assert int(written.item()) == ref_written
    assert _bits_equal(cb.cpu().numpy(), ref_cb)
    p = ref_picks[ref_picks >= 0]
    assert _bits_equal(cb.cpu().numpy()[: len(p)], z[p])               # written codes are their rows, bit for bit
    if N < K:
        assert ref_written <= N


@pytest.mark.parametrize("dist", [NORM, SQSUM])
def test_seed_with_duplicate_rows(oracle, dist):
    """A VQVAE-like latent: ReLU zeros and a few distinct rows repeated -- exactly M codes are written, all distinct."""
    from lipvq_vae_amd import ops
    M, K, D, N = 20, 64, 32, 5000
    rng = np.random.default_rng(5)
    base = np.maximum(rng.standard_normal((M, D)), 0).astype(np.float32)
    base[0] = 0.0
    z = base[rng.integers(0, M, N)]
    z[:M] = base                                                        # every distinct row occurs
    init = rng.uniform(-1, 1, (K, D)).astype(np.float32)
    u = rng.random(K)
    cb, picks, written = ops.kmeans_seed(torch.from_numpy(z).cuda(), K, torch.from_numpy(u).cuda(), dist,
                                         out=torch.from_numpy(init).cuda())
    cb, picks = cb.cpu().numpy(), picks.cpu().numpy()
    assert int(written.item()) == M
    assert (picks[:M] >= 0).all() and (picks[M:] == -1).all()
    assert len({cb[k].tobytes() for k in range(M)}) == M
    assert {cb[k].tobytes() for k in range(M)} == {b.tobytes() for b in base}
    assert _bits_equal(cb[M:], init[M:])
    ref_cb, ref_picks, ref_written = R.seed(oracle, z, K, u, dist, init=init)
    assert ref_written == M and np.array_equal(picks, ref_picks) and _bits_equal(cb, ref_cb)


@pytest.mark.parametrize("N,K,D,dist", [(6000, 128, 64, NORM), (1500, 64, 20, SQSUM), (3000, 96, 208, NORM)])
def test_kmeans_iteration_is_exact(oracle, N, K, D, dist):
    """kmeans(iters=2) = seeding, then per step: oracle.nearest assignment, sequential fp32 sums, fp32 division, refill of the
    empty codes -- restated with the same generator stream."""
    from lipvq_vae_amd.kmeans import kmeans
    z = _rows(7 * N + D, N, D)
    z[: N // 3] = z[N // 3: 2 * (N // 3)]                               # duplicates: some codes end up empty
    zt = torch.from_numpy(z).cuda()
    cb = torch.zeros(K, D, device="cuda")
    kmeans(zt, cb, iters=2, generator=torch.Generator().manual_seed(11), dist=dist)
    g = torch.Generator().manual_seed(11)
    u0 = torch.rand(K, dtype=torch.float64, generator=g).numpy()
    ref, _, _ = R.seed(oracle, z, K, u0, dist)
    for _ in range(2):
        ref, _, _ = R.lloyd_step(oracle, z, ref, torch.rand(K, dtype=torch.float64, generator=g).numpy(), dist)
    assert _bits_equal(cb.cpu().numpy(), ref)


def test_lloyd_step_refills_empty_codes(oracle):
    from lipvq_vae_amd.kmeans import lloyd_step
    N, K, D = 4000, 64, 64
    z = _rows(3, N, D)
    cb0 = z[:K].copy()
    cb0[K // 2:] = 50.0 + cb0[K // 2:]                                  # far away: empty after the assignment
    cb = torch.from_numpy(cb0).cuda()
    idx, counts = lloyd_step(torch.from_numpy(z).cuda(), cb, NORM, torch.Generator().manual_seed(2))
    u = torch.rand(K, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).numpy()
    ref, ref_idx, ref_counts = R.lloyd_step(oracle, z, cb0, u, NORM)
    assert (ref_counts[K // 2:] == 0).all()
    assert np.array_equal(idx.cpu().numpy(), ref_idx) and np.array_equal(counts.cpu().numpy(), ref_counts)
    assert _bits_equal(cb.cpu().numpy(), ref)
    rows = {r.tobytes() for r in z}
    assert all(ref[k].tobytes() in rows for k in range(K // 2, K))


@pytest.mark.parametrize("dist", [NORM, SQSUM])
def test_ops_revive_matches_restatement(oracle, dist):
    from lipvq_vae_amd import ops
    N, K, D = 5000, 200, 64
    z = _rows(17, N, D)
    cb0 = np.random.default_rng(4).uniform(-1, 1, (K, D)).astype(np.float32)
    idx = oracle.nearest(z, cb0, dist)[0]
    counts = np.bincount(idx, minlength=K).astype(np.int64)
    u = np.random.default_rng(9).random(K)
    cb = torch.from_numpy(cb0).cuda()
    for max_codes in (None, 3):
        cb.copy_(torch.from_numpy(cb0))
        picks, written = ops.kmeans_revive_(cb, torch.from_numpy(z).cuda(), torch.from_numpy(idx).cuda(),
                                            torch.from_numpy(counts).cuda(), 20, torch.from_numpy(u).cuda(), dist, max_codes=max_codes)
        ref_cb, ref_picks, ref_written = R.revive(oracle, z, cb0, idx, counts, 20, u, dist, max_codes=max_codes)
        assert 3 < (counts < 20).sum() < K
        assert np.array_equal(picks.cpu().numpy(), ref_picks) and int(written.item()) == ref_written
        assert _bits_equal(cb.cpu().numpy(), ref_cb)


def _llfq(oracle, A, D, K, regime, seed=3):
    from lipvq_vae_amd.tokenizer import LLFQVAE_V4
    p = O.make_params(seed, A, D, K, regime=regime, oracle=oracle)
    m = LLFQVAE_V4(A, D, num_codes=K).cuda()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()})
    return m, p


def _vq(oracle, A, D, K, regime, seed=3):
    from lipvq_vae_amd.tokenizer import VQVAE
    p = O.make_params(seed, A, D, K, regime=regime, variant="vq", oracle=oracle)
    m = VQVAE(A, D, num_embeddings=K).cuda()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()})
    return m, p


def test_revive_dead_codes_with_ema(oracle):
    from lipvq_vae_amd.ema import EMACodebook
    A, D, K, N = 7, 64, 256, 6000
    model, p = _llfq(oracle, A, D, K, "trained")
    xt = torch.from_numpy(O.make_inputs(1, N, A)).cuda()
    model.reset_usage()
    model.tokenize(xt)
    usage = model.code_usage.cpu().numpy().copy()
    dead = usage < 3
    assert 0 < dead.sum() < K
    ema = EMACodebook(model.quantizer.codebook)
    ema.cluster_size.fill_(5.0)
    ema.embed_sum.mul_(2.0)
    cs0, es0 = ema.cluster_size.cpu().numpy().copy(), ema.embed_sum.cpu().numpy().copy()
    cb0 = model.quantizer.codebook.detach().cpu().numpy().copy()
    revived = model.revive_dead_codes_(xt, threshold=3, generator=torch.Generator().manual_seed(8), ema=ema).cpu().numpy()
    cb = model.quantizer.codebook.detach().cpu().numpy()
    z = model.encode(xt).cpu().numpy()
    u = torch.rand(K, dtype=torch.float64, generator=torch.Generator().manual_seed(8)).numpy()
    ref_cb, ref_picks, _ = R.revive(oracle, z, cb0, oracle.nearest(z, cb0)[0], usage, 3, u, NORM)
    assert _bits_equal(cb, ref_cb)
    assert np.array_equal(revived, np.nonzero(ref_picks >= 0)[0])
    assert _bits_equal(cb[~dead], cb0[~dead])                           # live codes untouched
    assert len(revived) == dead.sum()
    assert len({cb[k].tobytes() for k in revived}) == len(revived)
    rows = {r.tobytes() for r in z}
    assert all(cb[k].tobytes() in rows for k in revived)
    cs, es = ema.cluster_size.cpu().numpy(), ema.embed_sum.cpu().numpy()
    other = np.setdiff1d(np.arange(K), revived)
    assert (cs[revived] == 1.0).all() and _bits_equal(es[revived], cb[revived])
    assert _bits_equal(cs[other], cs0[other]) and _bits_equal(es[other], es0[other])
    assert (model.code_usage == 0).all()


def _routes_agree(model, xt, want):
    """the new codebook on each route: fused / screened (N > 2048) and the small-batch exact kernel"""
    idx, _ = model.tokenize(xt)
    assert model.last_exact_rows is not None                            # the screen ran: the monitor's bypass is gone
    assert np.array_equal(idx.cpu().numpy(), want)
    ze = model.encode(xt)
    idx_s, _ = model._quantize(ze, None, screen=True)
    assert np.array_equal(idx_s.cpu().numpy(), want)
    idx_small, _ = model._quantize(model.encode(xt[:80]), None)         # 80 rows: the small-batch exact kernel
    assert model.last_exact_rows is None
    assert np.array_equal(idx_small.cpu().numpy(), want[:80])


def test_init_codebook_llfq_from_collapsed(oracle):
    A, D, K, N = 7, 64, 1024, 16384
    model, p = _llfq(oracle, A, D, K, "default")
    x = O.make_inputs(2, N, A)
    xt = torch.from_numpy(x).cuda()
    for _ in range(3):                                                  # arms the screen monitor's bypass on the collapsed codebook
        idx0, _ = model.tokenize(xt)
        torch.cuda.synchronize()
    assert len(np.unique(idx0.cpu().numpy())) <= 4                      # one code at the reference's initialisation
    with torch.no_grad():
        loss0 = model(xt)[1].item()
    model.init_codebook_(xt, iters=10, generator=torch.Generator().manual_seed(0))
    assert model._screen_monitor.bypass_calls == 0
    cb = model.quantizer.codebook.detach().cpu().numpy()
    want = oracle.nearest(oracle.llfq_encode(p, x), cb)[0]
    assert model.fused_shape()
    _routes_agree(model, xt, want)
    assert len(np.unique(want)) >= K // 2
    with torch.no_grad():
        assert model(xt)[1].item() < loss0


def test_init_codebook_vq(oracle):
    A, D, K, N = 7, 64, 256, 16384
    model, p = _vq(oracle, A, D, K, "default")
    x = O.make_inputs(4, N, A)
    xt = torch.from_numpy(x).cuda()
    idx0, _ = model.tokenize(xt)
    used0 = len(np.unique(idx0.cpu().numpy()))
    with torch.no_grad():
        loss0 = model(xt)[1].item()
    model.init_codebook_(xt, iters=10, generator=torch.Generator().manual_seed(0))
    cb = model.embedding.weight.detach().cpu().numpy()
    R3 = (O.ACT_RELU, O.ACT_RELU, O.ACT_RELU)
    ze = oracle.mlp3(x, p["encoder.0.weight"], p["encoder.0.bias"], p["encoder.2.weight"], p["encoder.2.bias"],
                     p["encoder.4.weight"], p["encoder.4.bias"], R3)
    want = oracle.nearest(ze, cb, SQSUM)[0]
    _routes_agree(model, xt, want)
    used = len(np.unique(want))
    assert used >= K // 2 and used > used0
    with torch.no_grad():
        assert model(xt)[1].item() < loss0


def test_same_generator_same_codebook(oracle):
    A, D, K, N = 7, 64, 256, 8000
    xt = torch.from_numpy(O.make_inputs(6, N, A)).cuda()
    out = []
    for _ in range(2):
        model, _ = _llfq(oracle, A, D, K, "default")
        model.init_codebook_(xt, iters=3, generator=torch.Generator().manual_seed(123), seed_rows=5000)
        out.append(model.quantizer.codebook.detach().cpu().numpy())
    assert _bits_equal(out[0], out[1])


def test_seed_under_graph_capture():
    from lipvq_vae_amd import ops
    N, K, D = 4000, 48, 64
    z = torch.from_numpy(_rows(21, N, D)).cuda()
    u = torch.from_numpy(np.random.default_rng(1).random(K)).cuda()
    eager = [t.cpu() for t in ops.kmeans_seed(z, K, u)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.kmeans_seed(z, K, u)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.kmeans_seed(z, K, u)
    for t in out:
        t.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a.cpu(), b)


def test_bad_input_raises():
    from lipvq_vae_amd import ops
    z = torch.zeros(100, 8, device="cuda")
    u = torch.zeros(10, dtype=torch.float64, device="cuda")
    with pytest.raises(TypeError):
        ops.kmeans_seed(z.double(), 10, u)
    with pytest.raises(TypeError):
        ops.kmeans_seed(z, 10, u.float())
    with pytest.raises(RuntimeError):
        ops.kmeans_seed(z.cpu(), 10, u)
    with pytest.raises(ValueError, match="draws"):
        ops.kmeans_seed(z, 11, u)
    with pytest.raises(ValueError, match="K must be"):
        ops.kmeans_seed(z, 0, u)
    cb = torch.zeros(10, 8, device="cuda")
    idx = torch.zeros(100, dtype=torch.int64, device="cuda")
    counts = torch.zeros(10, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="draws"):
        ops.kmeans_revive_(cb, z, idx, counts, 1, u[:5])
    with pytest.raises(ValueError, match="contiguous"):
        ops.kmeans_revive_(torch.zeros(8, 10, device="cuda").t(), z, idx, counts, 1, u)
    with pytest.raises(TypeError):
        ops.kmeans_means_(cb, cb, counts.int())
    with pytest.raises(ValueError):
        ops.kmeans_means_(cb, torch.zeros(9, 8, device="cuda"), counts)
