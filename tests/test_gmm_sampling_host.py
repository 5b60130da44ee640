"""CPU: the GMM head's in-kernel sampling noise (include/lipvq.h, "in-kernel sampling") without a GPU -- the library's host mirror
against the numpy restatement tests/gmm_sampling_ref.py bit for bit, the inverse normal CDF over ALL 2^23 grid arguments, the
statistics of the draws at fixed seeds, the stream addressing, GMMActionHead's source state on CPU tensors and the new entry
points' argument checks.  The kernels are held to the same functions on the GPU in tests/test_gpu_gmm_sampling.py."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import gmm_sampling_ref as R
import lipvq_vae_amd  # noqa: F401
from lipvq_vae_amd import nnfn, ops
from lipvq_vae_amd.gmm import GMMActionHead

SEED = 0x9E3779B97F4A7C15                  # both key words set
FWD_TOL = 1e-5                             # of the maximum magnitude: the forward bound of tests/test_gpu_gmm.py


def _bits(t):
    return (t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float32)).view(np.uint32)


# ---------------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------------

def test_site_constant_is_exported_and_collides_with_no_dropout_site():
    assert ops.SAMPLE_SITE_GMM == 0xC0000000 == R.SITE_U
    layers = range(0, 1 << 20, 4099)
    taken = {4 * la + k for la in layers for k in range(3)} | {ops.DROPOUT_SITE_EMBED} | {ops.DROPOUT_SITE_DEFAULT + 4 * la + k for la in layers for k in range(4)}
    assert ops.SAMPLE_SITE_GMM not in taken and ops.SAMPLE_SITE_GMM + 1 not in taken
    assert ops.DROPOUT_SITE_DEFAULT + 4 * ((1 << 28) - 1) + 3 < ops.SAMPLE_SITE_GMM       # no default-branch layer reaches it


@pytest.mark.parametrize("A", [1, 3, 4, 5, 12, 64])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 11), (8, 10)])
def test_noise_host_is_the_restatement_bit_for_bit(B, T, A):
    ids = [(7 * b + 3) % 11 + (2 ** 40 + 5 if b == 2 else 0) for b in range(B)]          # one id past 2^32: only its low bits count
    for step in (0, 1, 2 ** 32 + 1):
        for streams in (None, ids):
            u, eps = ops.gmm_noise_host(SEED, step, B, T, A, None if streams is None else torch.tensor(streams, dtype=torch.int64))
            ru, reps = R.noise32(SEED, step, B, T, A, streams)
            assert u.shape == (B, T) and eps.shape == (B, T, A) and u.dtype == eps.dtype == torch.float32
            assert np.array_equal(_bits(u), _bits(ru)), (step, streams)
            assert np.array_equal(_bits(eps), _bits(reps)), (step, streams)
    first = ops.gmm_noise_host(SEED, 1, B, T, A)
    wrapped = ops.gmm_noise_host(SEED, 2 ** 32 + 1, B, T, A)
    assert torch.equal(first[0], wrapped[0]) and torch.equal(first[1], wrapped[1])       # only the step's low 32 bits enter
    other = ops.gmm_noise_host(SEED, 0, B, T, A)
    assert not torch.equal(first[1], other[1])


def test_uniform_and_normal_fields_are_unrelated_words():
    u, eps = ops.gmm_noise_host(SEED, 3, 64, 1, 4)
    ru = R.uniform_of(R.uniform_words(SEED, 3, 64, 1))
    assert np.array_equal(_bits(u).ravel(), _bits(ru))
    w = R.normal_words(SEED, 3, 64, 1, 4)
    assert not np.array_equal(w[:, 0], R.uniform_words(SEED, 3, 64, 1))                  # another site word, another field
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0 and bool(torch.isfinite(eps).all())


# ---------------------------------------------------------------------------------------------------
# the transform, over all 2^23 arguments
# ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sweep():
    """(eps float32 [2^23] in the order of v, float64 inverse CDF of the same v): computed once."""
    k = np.arange(1 << 23, dtype=np.uint32)
    eps = ops.normal_icdf_host(k << np.uint32(9)).numpy()
    ref = R.ndtri64((2.0 * k.astype(np.float64) + 1.0) * 2.0 ** -24)
    return eps, ref


def test_icdf_is_finite_monotone_and_antisymmetric_over_the_whole_grid(sweep):
    eps, _ = sweep
    assert np.isfinite(eps).all()
    assert (np.diff(eps) >= 0).all()                                                    # non-decreasing in v
    assert np.array_equal(eps.view(np.uint32), (-eps[::-1]).view(np.uint32))            # icdf(1 - v) == -icdf(v), every bit
    assert abs(float(eps[-1]) - 5.2947) < 1e-4 and abs(float(eps[0]) + 5.2947) < 1e-4
    low = ops.normal_icdf_host(np.array([0, 0x1FF, 0x200, 0xFFFFFFFF], dtype=np.uint32))  # the low 9 bits of a word do not enter
    assert float(low[0]) == float(low[1]) == float(eps[0]) and float(low[2]) == float(eps[1]) and float(low[3]) == float(eps[-1])


def test_icdf_stays_within_the_forward_bound_of_float64_ndtri(sweep):
    eps, ref = sweep
    dev = float(np.abs(eps.astype(np.float64) - ref).max()) / float(np.abs(ref).max())
    print(f"lq_normal_icdf vs float64 ndtri over 2^23 arguments: max deviation {dev:.3e} of the maximum magnitude {np.abs(ref).max():.4f}")
    assert dev <= FWD_TOL


def test_icdf_restatement_agrees_on_a_stride_of_the_grid(sweep):
    eps, _ = sweep
    k = np.concatenate([np.arange(0, 1 << 23, 257, dtype=np.uint32), np.arange(4096, dtype=np.uint32), np.arange((1 << 23) - 4096, 1 << 23, dtype=np.uint32),
                        np.arange(629000, 630000, dtype=np.uint32)])                     # tails, and the switch of formulas at v = 0.075
    v = ((2.0 * k.astype(np.float64) + 1.0) * 2.0 ** -24).astype(np.float32)
    assert np.array_equal(R.normal_icdf32(v).view(np.uint32), eps[k].view(np.uint32))


# ---------------------------------------------------------------------------------------------------
# statistics at fixed seeds: the draws are deterministic, so each of these holds or does not
# ---------------------------------------------------------------------------------------------------

N = 1 << 20
STAT_SEED = 20240521


@pytest.fixture(scope="module")
def normals():
    """eps [65536, 16] float64 at steps 5 and 6 (row = stream id, T = 1), and an ideal-grid reference of the same size: the float64
    inverse CDF at grid points whose words come from numpy's generator."""
    a = ops.gmm_noise_host(STAT_SEED, 5, 65536, 1, 16)[1].numpy().reshape(65536, 16).astype(np.float64)
    b = ops.gmm_noise_host(STAT_SEED, 6, 65536, 1, 16)[1].numpy().reshape(65536, 16).astype(np.float64)
    words = np.random.default_rng(7).integers(0, 1 << 32, size=(2, 65536, 16), dtype=np.uint64).astype(np.uint32)
    ideal = R.ndtri64(R.open_of(words))
    return a, b, ideal[0], ideal[1]


def _moment_figures(x):
    return abs(float(x.mean())), abs(float(x.var()) - 1.0), R.ks_distance(x)


def test_normal_moments_and_ks(normals):
    a, _, ideal, _ = normals
    caps = (5.0 / math.sqrt(N), 5.0 * math.sqrt(2.0 / N), 1.95 / math.sqrt(N))
    ref = _moment_figures(ideal)
    got = _moment_figures(a)
    print(f"caps |mean| {caps[0]:.3e} |var - 1| {caps[1]:.3e} KS {caps[2]:.3e}; ideal grid {ref[0]:.3e} {ref[1]:.3e} {ref[2]:.3e}; "
          f"library {got[0]:.3e} {got[1]:.3e} {got[2]:.3e}")
    assert all(r <= c for r, c in zip(ref, caps)), "the ideal-grid reference itself leaves a cap"
    assert a.size == N and all(g <= c for g, c in zip(got, caps))


def test_normal_lag_correlations(normals):
    a, b, ia, ib = normals
    cap = 5.0 / math.sqrt(N)

    def figures(x, y):
        return (abs(R.corr(x[:, :-1], x[:, 1:])),           # neighbouring columns (words of one draw, and across draws)
                abs(R.corr(x, y)),                          # steps s and s + 1
                abs(R.corr(x[:-1], x[1:])))                 # streams i and i + 1
    ref, got = figures(ia, ib), figures(a, b)
    print(f"cap {cap:.3e}; ideal grid {ref[0]:.3e} {ref[1]:.3e} {ref[2]:.3e}; library columns {got[0]:.3e} steps {got[1]:.3e} streams {got[2]:.3e}")
    assert all(r <= cap for r in ref), "the ideal-grid reference itself leaves the cap"
    assert all(g <= cap for g in got)


def test_uniform_chi_squared_over_256_buckets():
    u = ops.gmm_noise_host(STAT_SEED, 5, N, 1, 1)[0].numpy().reshape(-1)
    cap = R.chi2_quantile(255)
    assert abs(cap - 330.52) < 0.01 and abs(R.chi2_quantile(2) + 2.0 * math.log(0.001)) < 1e-6
    ideal = R.uniform_of(np.random.default_rng(8).integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32))
    ref, got = R.chi2_uniform(ideal), R.chi2_uniform(u)
    print(f"chi-squared, 255 degrees of freedom: cap {cap:.2f}; ideal {ref:.2f}; library {got:.2f}")
    assert ref < cap, "the ideal reference itself leaves the cap"
    assert u.size == N and got < cap
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0


# ---------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,A", [(1, 5), (4, 12)])
def test_a_stream_draws_the_same_noise_wherever_it_sits(T, A):
    ids = [7, 3, 0, 9, 2]
    u, eps = ops.gmm_noise_host(SEED, 4, 5, T, A, torch.tensor(ids))
    for pos, i in enumerate(ids):
        u1, e1 = ops.gmm_noise_host(SEED, 4, 1, T, A, torch.tensor([i]))
        assert torch.equal(u[pos], u1[0]) and torch.equal(eps[pos], e1[0]), i
    un, en = ops.gmm_noise_host(SEED, 4, 5, T, A)
    ua, ea = ops.gmm_noise_host(SEED, 4, 5, T, A, torch.arange(5))
    assert torch.equal(un, ua) and torch.equal(en, ea)                                   # None = arange(B)
    assert torch.equal(u[2], un[0]) and torch.equal(eps[2], en[0])                       # id 0 at position 2 = position 0 by default


def test_streams_are_validated():
    with pytest.raises(ValueError, match="streams"):
        ops.gmm_noise_host(SEED, 0, 5, 2, 3, torch.arange(4))
    with pytest.raises(ValueError, match="streams"):
        ops.gmm_noise_host(SEED, 0, 5, 2, 3, torch.arange(5, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------
# the module's state, on CPU tensors
# ---------------------------------------------------------------------------------------------------

def test_sample_source_state_rules():
    torch.manual_seed(3)
    head = GMMActionHead(32, 12)
    after_head = torch.get_rng_state()
    torch.manual_seed(3)
    [nn.Linear(32, 60), nn.Linear(32, 60), nn.Linear(32, 5)]
    assert torch.equal(after_head, torch.get_rng_state())                                # construction: the three Linears' draws only
    assert isinstance(head, nnfn.KernelSampleSource)
    assert head.sample_source == "torch" and head.sample_state is None
    keys = list(head.state_dict().keys())
    with pytest.raises(ValueError, match="GMMActionHead"):
        head.set_sample_source("philox")
    assert head.sample_source == "torch" and head.sample_state is None
    with pytest.raises(RuntimeError, match=r"GMMActionHead\.reseed_sampling"):
        head.reseed_sampling(1)
    assert head.set_sample_source("torch") is head and head.sample_state is None         # "torch" creates nothing
    before = torch.get_rng_state()
    assert head.set_sample_source("kernel") is head
    assert torch.equal(before, torch.get_rng_state())
    assert head.sample_source == "kernel"
    st = head.sample_state
    assert st.dtype == torch.int64 and st.shape == (2,) and st.tolist() == [torch.initial_seed(), 0]
    assert list(head.state_dict().keys()) == keys                                        # a non-persistent buffer
    assert "_sample_state" in dict(head.named_buffers())                                 # ... that .to() moves
    head.set_sample_source("kernel")                                                     # no seed: the state stays
    head.reseed_sampling(2 ** 63 + 5, step=9)
    assert head.sample_state is st and st.tolist() == [2 ** 63 + 5 - 2 ** 64, 9]         # the bit pattern, as int64
    head.set_sample_source("kernel", seed=11)
    assert st.tolist() == [11, 0]
    head.set_sample_source("torch")
    assert head.sample_source == "torch" and head.sample_state is st                     # the state survives the way back
    assert torch.equal(before, torch.get_rng_state())
    plain = GMMActionHead(32, 12)
    plain.load_state_dict(head.state_dict(), strict=True)


def test_first_kernel_call_with_a_seed_uses_it():
    head = GMMActionHead(32, 3).set_sample_source("kernel", seed=SEED)
    assert head.sample_state.tolist() == [SEED - 2 ** 64, 0]


# ---------------------------------------------------------------------------------------------------
# argument checks without a GPU
# ---------------------------------------------------------------------------------------------------

def test_new_entry_points_refuse_before_any_launch():
    """Argument checks come before any launch, so they can be exercised with null pointers on a host without a GPU."""
    from lipvq_vae_amd import _capi
    lib = _capi.lib

    def draw(N, T, E, M, A, mode=0, bstride=0):
        return lib.lipvq_gmm_sample_draw_f32(None, bstride, *([None] * 9), N, T, E, M, A, mode, 0.01, None)

    def sample(N, T, E, M, A, mode=0, bstride=0):
        return lib.lipvq_gmm_sample_f32(None, bstride, *([None] * 9), N, T, E, M, A, mode, 0.01, None)

    # the checks are lipvq_gmm_sample_f32's, code for code: a shape outside the limits is refused (LIPVQ_EUNSUPPORTED = -2, the
    # code every GMM entry point gives its limits), a bad size, mode or stride and a null pointer are LIPVQ_EINVAL = -1
    for bad in ((80, 10, 512, 17, 12), (80, 10, 512, 0, 12), (80, 10, 512, 5, 65), (80, 10, 512, 13, 20), (80, 10, 1028, 5, 12), (80, 10, 510, 5, 12)):
        assert draw(*bad) == sample(*bad) == -2, bad
    assert draw(80, 10, 512, 5, 12, mode=3) == sample(80, 10, 512, 5, 12, mode=3) == -1
    assert draw(80, 10, 512, 5, 12, bstride=15362) == -1 and draw(80, 0, 512, 5, 12) == -1 and draw(-1, 10, 512, 5, 12) == -1
    assert draw(80, 10, 512, 5, 12) == -1 and b"null" in lib.lipvq_last_error()          # limits pass, then the pointers
    assert draw(0, 10, 512, 5, 12) == 0                                                  # zero rows: no-op
    assert lib.lipvq_gmm_noise_f32(None, None, None, None, 8, 10, 12, None) == -1 and b"null" in lib.lipvq_last_error()
    assert lib.lipvq_gmm_noise_f32(None, None, None, None, 8, 10, 65, None) == -2
    assert lib.lipvq_gmm_noise_f32(None, None, None, None, 8, 0, 12, None) == -1
    assert lib.lipvq_gmm_noise_f32(None, None, None, None, 0, 10, 12, None) == 0
    assert lib.lipvq_gmm_noise_host(1, 0, None, 8, 10, 12, None, None) == -1 and b"null" in lib.lipvq_last_error()
    assert lib.lipvq_gmm_noise_host(1, 0, None, 8, 10, 0, None, None) == -2
    assert lib.lipvq_gmm_noise_host(1, 0, None, 0, 10, 12, None, None) == 0
    assert lib.lipvq_normal_icdf_host(None, None, 4) == -1 and lib.lipvq_normal_icdf_host(None, None, 0) == 0
    assert lib.lipvq_normal_icdf_host(None, None, -1) == -1
    assert lib.lipvq_abi_version() == 1


def test_cpu_input_still_raises_under_the_kernel_source():
    head = GMMActionHead(64, 7).set_sample_source("kernel", seed=1)
    with pytest.raises(RuntimeError, match="HIP library only"):
        head(torch.zeros(2, 3, 64))
    assert head.sample_state.tolist() == [1, 0]                                          # refused before the state moved
