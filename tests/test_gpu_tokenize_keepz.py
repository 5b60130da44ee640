"""GPU: the fused launch's KEEPZ instances (latent width <= 64, rows decided in place, caller wants no z_e) keep z_e in registers
and hand an uncertified row to the exact decision through LDS -- no z_e store at all.  The answers must be the oracle's and the
storing instance's (want_ze=True), bit for bit, above all on the rows that take the in-place path: the codebooks here carry every
lower-half code twice (the copy one ulp away in one coordinate), so that a large share of the rows is a near-tie no screen can
certify.  Also here: the deferred z_e stores' counted waits in a row block whose last waves have no valid row (tok_defer_ze = 1).

Near-tie share of the construction, oracle alone on the CPU (rows whose best and second-best distances differ by < 1e-6 relative;
make_params' trained regime, the numpy twin of bench.trained_like_): every one of 549 rows, at D = 64, K = 1024 and at D = 32,
K = 256, five seeds each -- the lower-half codes sit on the data, so every row's winner has its copy.  (Launches with a fraction of
a percent of uncertified rows among certified ones: tests/test_gpu_fused.py, whose calls without z_e run these instances too.)"""
import numpy as np
import pytest
import torch

from oracle import lipvq_oracle as O

pytestmark = pytest.mark.gpu

A = 7
SHAPES = [(64, 1024), (32, 256)]
_cases = {}


def _dup_codes_(cb):
    """cb[c] for c >= K/2 becomes cb[c - K/2] moved by one ulp in coordinate c % D (in place)."""
    K, D = cb.shape
    half = K // 2
    cb[half:] = cb[:half]
    j = np.arange(half) % D
    cb[half + np.arange(half), j] = np.nextafter(cb[np.arange(half), j], np.float32(2.0))
    return cb


def _case(D, K):
    """(model on the GPU, its parameters as numpy arrays): bench.trained_like_ parameters with the upper half of the codebook
    overwritten by near-copies of the lower half.  Built once per shape, never modified."""
    if (D, K) not in _cases:
        import bench
        from lipvq_vae_amd.tokenizer import LLFQVAE_V4
        torch.manual_seed(1000 + D)
        model = LLFQVAE_V4(A, D, num_codes=K).cuda()
        bench.trained_like_(model, A, seed=D)
        cb = _dup_codes_(model.quantizer.codebook.detach().cpu().numpy().copy())
        with torch.no_grad():
            model.quantizer.codebook.copy_(torch.from_numpy(cb).cuda())
        p = {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in model.state_dict().items()}
        _cases[(D, K)] = (model, p)
    return _cases[(D, K)]


def _oracle_answers(oracle, p, x):
    ze = oracle.llfq_encode(p, x)
    idx, zq, usage = oracle.nearest(ze, p["quantizer.codebook"])
    return ze, idx, zq, usage


def _run_keepz(model, xt):
    """model.tokenize: want_ze=False, so a width <= 64 with a small codebook runs the KEEPZ instance.  -> idx, zq, usage, exact rows"""
    model.reset_usage()
    idx, zq = model.tokenize(xt)
    exact = int(model.last_exact_rows[0])
    return idx, zq, model.code_usage.clone(), exact


def _run_storing(model, xt):
    """the same launch with the caller asking for z_e: the storing instance, rows re-read from memory for the decision"""
    idx, zq, ze = model._tokenize_fused(xt, None, want_ze=True)
    return idx, zq, ze


def _check_against_oracle(oracle, model, p, x, min_exact=0):
    N = x.shape[0]
    xt = torch.from_numpy(x).cuda()
    ze_ref, idx_ref, _, usage_ref = _oracle_answers(oracle, p, x)
    idx, zq, usage, exact = _run_keepz(model, xt)
    print(f"N={N} D={model.latent_dim} K={model.num_codes}: rows decided in place {exact} ({100.0 * exact / N:.1f} %), floor {min_exact}")
    assert exact >= min_exact, (exact, min_exact)
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    assert torch.equal(zq, model.quantizer.codebook.detach()[idx])
    assert int(usage.sum()) == N and np.array_equal(usage.cpu().numpy(), usage_ref)
    idx_s, zq_s, ze_s = _run_storing(model, xt)
    assert torch.equal(idx_s, idx) and torch.equal(zq_s, zq)
    assert np.array_equal(ze_s.cpu().numpy(), ze_ref)


@pytest.mark.parametrize("shape", ["w8rg1", "w4rg1"])
@pytest.mark.parametrize("D,K", SHAPES)
def test_dense_inplace_path(oracle, lipvq_option, no_screen_monitor, D, K, shape):
    """Two full 256-row blocks and a ragged one (8 waves: 37 rows = one full wave, one with five rows, six with none); more than a
    quarter of the rows uncertified -- a launch that certifies everything has tested nothing."""
    model, p = _case(D, K)
    lipvq_option("tok_shape", shape)
    N = 2 * 256 + 37
    x = O.make_inputs(40 + D, N, A)
    _check_against_oracle(oracle, model, p, x, min_exact=N // 4 + 1)


@pytest.mark.parametrize("D,K", SHAPES)
def test_full_wave_of_one_neartie_row(oracle, lipvq_option, no_screen_monitor, D, K):
    """Rows 32 .. 63 -- all of wave 1 of the first block, both lane halves of every row pair -- are copies of one near-tie row."""
    model, p = _case(D, K)
    lipvq_option("tok_shape", "w8rg1")
    N = 256 + 3
    x = O.make_inputs(50 + D, N, A)
    ze = oracle.llfq_encode(p, x)
    d = np.sort(oracle.distances(ze, p["quantizer.codebook"]), axis=1)
    tie = np.flatnonzero((d[:, 1] - d[:, 0]) < 1e-6 * d[:, 0])
    assert tie.size > 0
    x[32:64] = x[tie[0]]
    _check_against_oracle(oracle, model, p, x, min_exact=32)


@pytest.mark.parametrize("N", [1, 31, 33, 4 * 32 * 1 + 5])
@pytest.mark.parametrize("D,K", SHAPES)
def test_small_launches(oracle, no_screen_monitor, D, K, N):
    """Less than, one more than and just past one row block of the 4-wave instance (the default shape of a small launch)."""
    model, p = _case(D, K)
    x = O.make_inputs(60 + N, N, A)
    _check_against_oracle(oracle, model, p, x)


@pytest.mark.parametrize("D,K", SHAPES)
def test_nonfinite_rows(lipvq_option, no_screen_monitor, D, K):
    """One input row of NaN, one of +1e30 and one of -1e30 among finite rows: whatever the storing instance answers, so does this one."""
    model, _ = _case(D, K)
    for shape in ("w8rg1", "w4rg1"):
        lipvq_option("tok_shape", shape)
        N = 256 + 70
        x = O.make_inputs(70 + D, N, A)
        x[5] = np.nan
        x[40] = 1e30
        x[300] = -1e30
        xt = torch.from_numpy(x).cuda()
        idx, zq, usage, _ = _run_keepz(model, xt)
        idx_s, zq_s, _ = _run_storing(model, xt)
        assert torch.equal(idx, idx_s) and torch.equal(zq, zq_s)
        assert int(idx.min()) >= 0 and int(idx.max()) < K and int(usage.sum()) == N


@pytest.mark.parametrize("shape", ["w8rg1", "w4rg1"])
@pytest.mark.parametrize("rem", [1, 32, 33, 224])
def test_deferred_ze_stores_with_empty_waves(oracle, lipvq_option, no_screen_monitor, rem, shape):
    """tok_defer_ze = 1 in the storing instance: the last row block has one valid wave up to all but one.  A wave without a valid
    row issues no deferred store and must not count any in its waits for the first two stages of the codebook."""
    D, K = 64, 1024
    model, p = _case(D, K)
    lipvq_option("tok_shape", shape)
    lipvq_option("tok_defer_ze", "1")
    N = 256 + rem
    x = O.make_inputs(80 + rem, N, A)
    ze_ref, idx_ref, zq_ref, _ = _oracle_answers(oracle, p, x)
    idx, zq, ze = _run_storing(model, torch.from_numpy(x).cuda())
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    assert np.array_equal(ze.cpu().numpy(), ze_ref)
    assert np.array_equal(zq.cpu().numpy(), zq_ref)
